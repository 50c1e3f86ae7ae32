// The packed 3x3 weight images, each layout defined ONCE: the index maps that the packers
// (conv3x3_pack_kernel, convh_pack_kernel, both kernels of conv_pack.hip) write through, and the
// shape rule that decides which image a (cin, kout) layer gets.  The kernels that READ an image
// (conv3x3_kernel, convh_kernel) address it by fragment and are documented where they live.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

struct PackCoord {
  int co, ci, tap;       // output channel and contraction channel OF THE PASS, tap = 3 kh + kw
};

// Element offset of coordinate c in the OIHW weight w (element strides sk, sc, sh, sw):
//   forward:                    B[ci][co] = w[co][ci][kh][kw]
//   transposed (backward-data): B[ci][co] = w[ci][co][2 - kh][2 - kw]   (contraction over w's k)
__host__ __device__ __forceinline__ int64_t pack_src_offset(PackCoord c, int64_t sk, int64_t sc,
                                                            int64_t sh, int64_t sw,
                                                            int transposed) {
  const int kh = c.tap / 3, kw = c.tap % 3;
  return transposed ? c.ci * sk + c.co * sc + (2 - kh) * sh + (2 - kw) * sw
                    : c.co * sk + c.ci * sc + kh * sh + kw * sw;
}

// Shapes whose weight slice fits the register file get the register image (conv64.hip), the
// other supported shapes the LDS image (convh.hip).
__host__ __device__ constexpr bool pack_reg_shape(int cin, int kout) {
  return (cin == 64 || cin == 128) && (kout == 64 || kout == 128);
}

// Register image (conv3x3_kernel): [n-tile kout / 32][k-step 9 * cin / 16][lane 64][8]; lane (j, h)
// of k-step ks holds output channel 32 nt + j, contraction channels 16 (ks % SPT) + 8 h .. + 7 of
// tap ks / SPT, SPT = cin / 16.
__host__ __device__ __forceinline__ PackCoord pack_reg_coord(int64_t idx, int cin) {
  const int spt = cin / 16, ks_n = 9 * spt;
  const int e = idx & 7, lane = (idx >> 3) & 63, ks = (int)((idx >> 9) % ks_n);
  const int nt = (int)(idx / ((int64_t)ks_n * 512));
  return PackCoord{32 * nt + (lane & 31), 16 * (ks % spt) + 8 * (lane >> 5) + e, ks / spt};
}
// ... and its inverse for a 16-byte unit: the index of (co, contraction channels 8 piece .. + 7, tap)
__host__ __device__ __forceinline__ int64_t pack_reg_index(int co, int piece, int tap, int cin) {
  const int spt = cin / 16, ks = tap * spt + (piece >> 1);
  return (((int64_t)(co >> 5) * 9 * spt + ks) * 64 + (co & 31) + 32 * (piece & 1)) * 8;
}

// LDS image (convh_kernel): [n-block kout / 128][chunk cin / 32][tap 9][piece g 4][k 128][8]: the
// 8 KB of a (chunk, tap) step as they lie in LDS; element e of piece g is contraction channel
// 32 cc + 8 g + e.
__host__ __device__ __forceinline__ PackCoord pack_lds_coord(int64_t idx, int cin) {
  const int e = idx & 7, k = (idx >> 3) & 127, g = (idx >> 10) & 3;
  const int64_t rest = idx >> 12;                      // (nb * CC + cc) * 9 + tap
  const int cc_n = cin / 32;
  const int cc = (rest / 9) % cc_n, nb = rest / 9 / cc_n;
  return PackCoord{128 * nb + k, 32 * cc + 8 * g + e, (int)(rest % 9)};
}
__host__ __device__ __forceinline__ int64_t pack_lds_index(int co, int piece, int tap, int cin) {
  return (((int64_t)(co >> 7) * (cin / 32) + (piece >> 2)) * 9 + tap) * 4096 +
         ((piece & 3) * 128 + (co & 127)) * 8;
}
