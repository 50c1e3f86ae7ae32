// Batch assembly from a device-resident bank of uint8 frames (train/frame_bank.py): every output
// frame k is one frame of `bank` (slots[k] >= 0) or of `extra` (slots[k] < 0: frame -slots[k]-1),
// widened byte by byte to float32 — the same float32 the host's .astype(np.float32) makes, every
// uint8 being exact in it.
//
// Pure streaming: frame_bytes in, 4 frame_bytes out, no reuse, no LDS.  A lane takes four source
// bytes (one dword) and stores them as one 16-byte float4, so a wave instruction reads 256
// contiguous bytes and writes 1 KiB; kUnroll such groups per lane, all loads issued before the
// first store.  grid = (chunks of a frame, n).
//
// Alignment is decided PER FRAME (a block serves one frame, so the decision is block-uniform):
//   * output frame k starts at out + 4 k frame_bytes, 16-byte aligned only when frame_bytes is a
//     multiple of 4 (and `out` is): the first `head` (0..3) values of a frame are stored one by
//     one until the address is 16-byte aligned, the float4 body follows, then a tail of 0..3;
//   * the source of the body starts at src + head; where that address is not a multiple of 4 (odd
//     frame sizes, a bank that is a view at a byte offset) the four bytes of a group are loaded
//     one by one — still 256 contiguous bytes per wave instruction — and stored as a float4.
// A slot outside its source (a bookkeeping bug above this layer) reads nothing and fills its
// output frame with NaN.
//
// Further down: scl_frames_resize, the loaders' 8-bit bilinear resize applied from host-made
// tables (util/cv.py resize_plan; util/device_cv.py).
#include "scl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                         // float4 groups per lane
constexpr int kChunkGroups = kThreads * kUnroll;   // 4-byte groups per workgroup: 4 KiB in, 16 KiB out

__device__ __forceinline__ f32x4 widen4(unsigned w) {
  return f32x4{(float)(w & 0xffu), (float)((w >> 8) & 0xffu), (float)((w >> 16) & 0xffu),
               (float)(w >> 24)};
}

__global__ __launch_bounds__(kThreads) void frames_gather_kernel(
    const unsigned char* __restrict__ bank, long long bank_slots,
    const unsigned char* __restrict__ extra, long long extra_slots, const int* __restrict__ slots,
    long long frame_bytes, float* __restrict__ out) {
  const int k = blockIdx.y, tid = threadIdx.x;
  const int s = slots[k];
  const unsigned char* src = nullptr;
  if (s >= 0) {
    if (s < bank_slots) src = bank + (long long)s * frame_bytes;
  } else {
    const long long e = -((long long)s + 1);
    if (e < extra_slots) src = extra + e * frame_bytes;
  }
  float* dst = out + (long long)k * frame_bytes;
  const float nan = __builtin_nanf("");

  // values in front of the first 16-byte aligned output address (dst is 4-byte aligned)
  long long head = (long long)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);
  if (head > frame_bytes) head = frame_bytes;
  const long long groups = (frame_bytes - head) >> 2;
  const long long tail = head + 4 * groups;       // first byte after the body

  if (blockIdx.x == 0 && tid < 8) {               // head: lanes 0..3, tail: lanes 4..7
    const long long i = tid < 4 ? tid : tail + (tid - 4);
    const bool mine = tid < 4 ? tid < head : i < frame_bytes;
    if (mine) dst[i] = src ? (float)src[i] : nan;
  }

  const long long g0 = (long long)blockIdx.x * kChunkGroups + tid;
  f32x4* body = reinterpret_cast<f32x4*>(dst + head);
  if (!src) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long g = g0 + u * kThreads;
      if (g < groups) body[g] = f32x4{nan, nan, nan, nan};
    }
    return;
  }
  const unsigned char* sb = src + head;
  unsigned w[kUnroll];
  if ((((uintptr_t)sb) & 3u) == 0) {
    const unsigned* sw = reinterpret_cast<const unsigned*>(sb);
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long g = g0 + u * kThreads;
      w[u] = g < groups ? sw[g] : 0u;
    }
  } else {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long g = g0 + u * kThreads;
      w[u] = 0u;
      if (g < groups) {
        const unsigned char* p = sb + 4 * g;
        w[u] = (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const long long g = g0 + u * kThreads;
    if (g < groups) body[g] = widen4(w[u]);
  }
}

// ---- the 8-bit bilinear resize of util/cv.py (resize_plan / apply_plan) ----------------------
// The host splits OpenCV's float32 coordinate computation into four int32 tables per axis (two
// source indices, two 11-bit weights); the device only applies them, in the int32 arithmetic of
// apply_plan, so its pixels are the host's by construction:
//   S0 = src[y0][x0] a0 + src[y0][x1] a1,  S1 the same on row y1,
//   v  = clip((((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2, 0, 255).
// One work-item per output pixel, all channels: the stores of a wave are contiguous (768 bytes of
// float32 at c = 3).  The loads are a sparse gather — at 1280 x 960 -> 240 x 180 an output value
// touches 2 x 2 source pixels of every 5.3 x 5.3 — served by L2; plain byte loads, any alignment.
// grid = (chunks of a frame's pixels, n).
// The tables are device memory the launcher cannot see: every index read from one is clamped to
// [0, sw-1] or [0, sh-1], so a wrong table gives wrong pixels but never a read outside the frame
// (products are taken modulo 2^32 like NumPy's int32, so a wrong weight is no undefined
// behaviour either).
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int wrap_mul(int a, int b) { return (int)((unsigned)a * (unsigned)b); }

template <int C, typename Out>
__global__ __launch_bounds__(kThreads) void frames_resize_kernel(
    const unsigned char* __restrict__ src, int sh, int sw, const int* __restrict__ xtab, int ow,
    const int* __restrict__ ytab, int oh, Out* __restrict__ out) {
  const int pix = blockIdx.x * kThreads + threadIdx.x;       // oh ow <= 2^28
  if (pix >= oh * ow) return;
  const int oy = pix / ow, ox = pix - oy * ow;
  const int x0 = clampi(xtab[ox], sw - 1) * C, x1 = clampi(xtab[ow + ox], sw - 1) * C;
  const int a0 = xtab[2 * ow + ox], a1 = xtab[3 * ow + ox];
  const int y0 = clampi(ytab[oy], sh - 1), y1 = clampi(ytab[oh + oy], sh - 1);
  const int b0 = ytab[2 * oh + oy], b1 = ytab[3 * oh + oy];
  const long long row = (long long)sw * C;
  const unsigned char* frame = src + (long long)blockIdx.y * sh * row;
  const unsigned char* r0 = frame + y0 * row;
  const unsigned char* r1 = frame + y1 * row;
  Out* dst = out + ((long long)blockIdx.y * oh * ow + pix) * C;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const int s0 = wrap_mul(r0[x0 + ch], a0) + wrap_mul(r0[x1 + ch], a1);
    const int s1 = wrap_mul(r1[x0 + ch], a0) + wrap_mul(r1[x1 + ch], a1);
    const int v = ((wrap_mul(b0, s0 >> 4) >> 16) + (wrap_mul(b1, s1 >> 4) >> 16) + 2) >> 2;
    dst[ch] = (Out)clampi(v, 255);
  }
}

template <int C, typename Out>
void launch_resize(const void* src, int n, int sh, int sw, const int* xtab, int ow, const int* ytab,
                   int oh, void* out, hipStream_t stream) {
  const dim3 grid((unsigned)(((long long)oh * ow + kThreads - 1) / kThreads), (unsigned)n);
  SCL_LAUNCH("frames_resize_kernel", (frames_resize_kernel<C, Out>), grid, dim3(kThreads), 0, stream,
             static_cast<const unsigned char*>(src), sh, sw, xtab, ow, ytab, oh,
             static_cast<Out*>(out));
}

}  // namespace

extern "C" int scl_frames_resize(const void* src, int n, int sh, int sw, int c, const int* xtab,
                                 int ow, const int* ytab, int oh, int out_kind, void* out,
                                 void* stream) {
  if (!src || !xtab || !ytab || !out) return SCL_E_NULL;
  const int side_cap = 16384;
  if (n < 1 || n > 65535 || (c != 1 && c != 3)) return SCL_E_SHAPE;
  if (sh < 1 || sw < 1 || sh > side_cap || sw > side_cap) return SCL_E_SHAPE;
  if (oh < 1 || ow < 1 || oh > side_cap || ow > side_cap) return SCL_E_SHAPE;
  if (out_kind != SCL_FRAMES_U8 && out_kind != SCL_FRAMES_F32) return SCL_E_SHAPE;
  if (out_kind == SCL_FRAMES_F32 && (((uintptr_t)out) & 3u)) return SCL_E_SHAPE;
  const hipStream_t st = (hipStream_t)stream;
  if (out_kind == SCL_FRAMES_U8) {
    if (c == 1) launch_resize<1, unsigned char>(src, n, sh, sw, xtab, ow, ytab, oh, out, st);
    else launch_resize<3, unsigned char>(src, n, sh, sw, xtab, ow, ytab, oh, out, st);
  } else {
    if (c == 1) launch_resize<1, float>(src, n, sh, sw, xtab, ow, ytab, oh, out, st);
    else launch_resize<3, float>(src, n, sh, sw, xtab, ow, ytab, oh, out, st);
  }
  return scl_launch_status();
}

extern "C" int scl_frames_gather(const void* bank, long long bank_slots, const void* extra,
                                 long long extra_slots, const int* slots, int n,
                                 long long frame_bytes, void* out, void* stream) {
  if (!out || !slots || (!bank && bank_slots > 0) || (!extra && extra_slots > 0)) return SCL_E_NULL;
  const long long slot_cap = 1LL << 31, byte_cap = 1LL << 30;
  if (n < 1 || n > 65535 || frame_bytes < 1 || frame_bytes > byte_cap) return SCL_E_SHAPE;
  if (bank_slots < 0 || extra_slots < 0 || bank_slots >= slot_cap || extra_slots >= slot_cap ||
      (bank_slots == 0 && extra_slots == 0))
    return SCL_E_SHAPE;
  if (((uintptr_t)out) & 3u) return SCL_E_SHAPE;            // float32 output
  // a head of at most 3 values leaves at most frame_bytes / 4 groups
  const long long chunks = (frame_bytes / 4 + kChunkGroups - 1) / kChunkGroups;
  const dim3 grid((unsigned)(chunks > 0 ? chunks : 1), (unsigned)n);
  SCL_LAUNCH("frames_gather_kernel", frames_gather_kernel, grid, dim3(kThreads), 0,
             (hipStream_t)stream, static_cast<const unsigned char*>(bank), bank_slots,
             static_cast<const unsigned char*>(extra), extra_slots, slots, frame_bytes,
             static_cast<float*>(out));
  return scl_launch_status();
}
