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
// tables (util/cv.py resize_plan; util/device_cv.py), and scl_frames_debayer, raw Bayer frames through
// the RobotCar SDK's demosaic and undistortion (util/robotcar.py), alone or fused with that resize.
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

// ---- raw Bayer frames: bilinear demosaic + look-up-table undistortion (util/robotcar.py) -----------
// One undistorted pixel reads the demosaiced 2 x 2 patch (y0..y1, x0..x1) at the table's coordinate,
// i.e. the 4 x 4 raw window (y0-1..y0+2, x0-1..x0+2): sixteen byte loads serve all three channels.
// Everything that depends on the pixel and not on the frame — the table's coordinate, floor, the four
// float64 weights, the sixteen window offsets (the border rule applied) and the colour of the site each
// of them reads — is a DebayerSite, made once; a thread then walks its frames with it, so a batch
// reads the table once.
//   demosaic   q_c = sum of 4 H_c x (raw where the site READ has colour c) over the 3 x 3 taps, in
//              integers (quarter units, at most 2295), the value (double)q * 0.25: exact;
//   undistort  acc = 0; acc += (v00 wy0) wx0; acc += (v01 wy0) tx; acc += (v10 ty) wx0; acc += (v11 ty) tx,
//              float64, every operation rounded on its own (contraction off: the order is the definition);
//   byte       acc truncated toward zero, low 8 bits (under 'reflect' border values reach 573.75 and wrap).
// y1 = min(y0+1, sh-1): in the last row the patch's second row IS its first (the select below), the same
// for columns.  Indices: y0, x0 come from the table only after the inside test (a NaN fails it), are
// clamped again after the conversion, and every window index is clamped to the frame after the border
// rule — a wrong table gives wrong pixels, never a read outside raw.  Without a table (lut == nullptr)
// the coordinate is the pixel itself: weights 1 and 0, the demosaic alone.
// Fused with the resize: a thread owns one OUTPUT pixel and evaluates the four undistorted pixels
// (Y0|Y1, X0|X1) its tables name (clamped as in frames_resize_kernel) and nothing else, then applies
// frames_resize_kernel's int32 formula to those bytes.
// grid = (chunks of the evaluated frame's pixels, groups of `fpt` frames).
struct DebayerSite {
  int row[4], col[4];      // window offsets: row index * sw, column index
  unsigned colour;         // 2 bits per window entry (4 i + j): 0 R, 1 G, 2 B
  double wy0, ty, wx0, tx;
  bool inside, last_row, last_col;
};

__device__ __forceinline__ int border_index(int p, int n, int mirror) {
  if (p < 0) p = mirror ? 1 : 0;
  else if (p >= n) p = mirror ? n - 2 : n - 1;
  return clampi(p, n - 1);                       // (p = n + 1 below the last row: a value never used)
}

__device__ __forceinline__ DebayerSite debayer_site(const double* __restrict__ lut, int py, int px,
                                                    int sh, int sw, unsigned sites, int mirror) {
#pragma clang fp contract(off)
  DebayerSite s;
  double ly = (double)py, lx = (double)px;
  if (lut) {
    const long long p = (long long)py * sw + px;
    lx = lut[p];
    ly = lut[(long long)sh * sw + p];
  }
  s.inside = ly >= 0.0 && ly <= (double)(sh - 1) && lx >= 0.0 && lx <= (double)(sw - 1);
  if (!s.inside) ly = lx = 0.0;
  const double fy = floor(ly), fx = floor(lx);
  s.ty = ly - fy;
  s.tx = lx - fx;
  s.wy0 = 1.0 - s.ty;
  s.wx0 = 1.0 - s.tx;
  const int y0 = clampi((int)fy, sh - 1), x0 = clampi((int)fx, sw - 1);
  s.last_row = y0 == sh - 1;
  s.last_col = x0 == sw - 1;
  int prow[4], pcol[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = border_index(y0 - 1 + i, sh, mirror), x = border_index(x0 - 1 + i, sw, mirror);
    s.row[i] = y * sw;
    s.col[i] = x;
    prow[i] = y & 1;
    pcol[i] = x & 1;
  }
  s.colour = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      s.colour |= ((sites >> (2 * (2 * prow[i] + pcol[j]))) & 3u) << (2 * (4 * i + j));
  return s;
}

// the three bytes (R, G, B) of one undistorted pixel of one frame
__device__ __forceinline__ void debayer_eval(const DebayerSite& s, const unsigned char* __restrict__ frame,
                                             int rgb[3]) {
#pragma clang fp contract(off)
  int plane[3][4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = frame[s.row[i] + s.col[j]];              // sh sw <= 2^28
      const unsigned c = (s.colour >> (2 * (4 * i + j))) & 3u;
#pragma unroll
      for (int k = 0; k < 3; ++k) plane[k][i][j] = c == (unsigned)k ? v : 0;
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int q[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int(*w)[4] = plane[k];
        const int cross = w[a][b + 1] + w[a + 1][b] + w[a + 1][b + 2] + w[a + 2][b + 1];
        const int diag = w[a][b] + w[a][b + 2] + w[a + 2][b] + w[a + 2][b + 2];
        q[a][b] = k == 1 ? 4 * w[a + 1][b + 1] + cross : 4 * w[a + 1][b + 1] + 2 * cross + diag;
      }
    if (s.last_row) { q[1][0] = q[0][0]; q[1][1] = q[0][1]; }
    if (s.last_col) { q[0][1] = q[0][0]; q[1][1] = q[1][0]; }
    double acc = 0.0;
    acc += (((double)q[0][0] * 0.25) * s.wy0) * s.wx0;
    acc += (((double)q[0][1] * 0.25) * s.wy0) * s.tx;
    acc += (((double)q[1][0] * 0.25) * s.ty) * s.wx0;
    acc += (((double)q[1][1] * 0.25) * s.ty) * s.tx;
    rgb[k] = s.inside ? ((int)acc & 255) : 0;                // 0 <= acc < 2^10
  }
}

template <bool Fused, typename Out>
__global__ __launch_bounds__(kThreads) void frames_debayer_kernel(
    const unsigned char* __restrict__ raw, int n, int fpt, int sh, int sw, unsigned sites, int mirror,
    const double* __restrict__ lut, const int* __restrict__ xtab, int ow, const int* __restrict__ ytab,
    int oh, Out* __restrict__ out) {
  const int pix = blockIdx.x * kThreads + threadIdx.x;       // oh ow <= 2^28
  if (pix >= oh * ow) return;
  const int oy = pix / ow, ox = pix - oy * ow;
  const long long frame_bytes = (long long)sh * sw;
  const int first = blockIdx.y * fpt, last = min(first + fpt, n);
  if constexpr (!Fused) {
    const DebayerSite s = debayer_site(lut, oy, ox, sh, sw, sites, mirror);
    for (int f = first; f < last; ++f) {
      int rgb[3];
      debayer_eval(s, raw + f * frame_bytes, rgb);
      Out* dst = out + ((long long)f * oh * ow + pix) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) dst[k] = (Out)rgb[k];
    }
  } else {
    const int x0 = clampi(xtab[ox], sw - 1), x1 = clampi(xtab[ow + ox], sw - 1);
    const int a0 = xtab[2 * ow + ox], a1 = xtab[3 * ow + ox];
    const int y0 = clampi(ytab[oy], sh - 1), y1 = clampi(ytab[oh + oy], sh - 1);
    const int b0 = ytab[2 * oh + oy], b1 = ytab[3 * oh + oy];
    DebayerSite s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      s[e] = debayer_site(lut, e < 2 ? y0 : y1, (e & 1) ? x1 : x0, sh, sw, sites, mirror);
    for (int f = first; f < last; ++f) {
      const unsigned char* frame = raw + f * frame_bytes;
      int u[4][3];
#pragma unroll
      for (int e = 0; e < 4; ++e) debayer_eval(s[e], frame, u[e]);
      Out* dst = out + ((long long)f * oh * ow + pix) * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int s0 = wrap_mul(u[0][k], a0) + wrap_mul(u[1][k], a1);
        const int s1 = wrap_mul(u[2][k], a0) + wrap_mul(u[3][k], a1);
        const int v = ((wrap_mul(b0, s0 >> 4) >> 16) + (wrap_mul(b1, s1 >> 4) >> 16) + 2) >> 2;
        dst[k] = (Out)clampi(v, 255);
      }
    }
  }
}

// the colours of the sites (0,0), (0,1), (1,0), (1,1), 2 bits each (0 R, 1 G, 2 B), for SCL_BAYER_*
constexpr unsigned kBayerSites[4] = {
    0u | 1u << 2 | 1u << 4 | 2u << 6,     // rggb
    2u | 1u << 2 | 1u << 4 | 0u << 6,     // bggr
    1u | 0u << 2 | 2u << 4 | 1u << 6,     // grbg
    1u | 2u << 2 | 0u << 4 | 1u << 6,     // gbrg
};
// Work-items the grid aims at before a thread takes more than one frame: eight waves a SIMD on 256 CUs.
constexpr long long kDebayerTargetItems = 256LL * 4 * 8 * 64;

template <bool Fused, typename Out>
void launch_debayer(const void* raw, int n, int sh, int sw, int pattern, int border, const double* lut,
                    const int* xtab, int ow, const int* ytab, int oh, void* out, hipStream_t stream) {
  const long long pixels = (long long)oh * ow;
  // frames per thread: all of them once the pixels alone fill the device, fewer for small outputs
  long long fpt = (pixels * n + kDebayerTargetItems - 1) / kDebayerTargetItems;
  fpt = fpt < 1 ? 1 : (fpt > n ? n : fpt);
  const dim3 grid((unsigned)((pixels + kThreads - 1) / kThreads), (unsigned)((n + fpt - 1) / fpt));
  SCL_LAUNCH("frames_debayer_kernel", (frames_debayer_kernel<Fused, Out>), grid, dim3(kThreads), 0, stream,
             static_cast<const unsigned char*>(raw), n, (int)fpt, sh, sw, kBayerSites[pattern], border, lut,
             xtab, ow, ytab, oh, static_cast<Out*>(out));
}

}  // namespace

extern "C" int scl_frames_debayer(const void* raw, int n, int sh, int sw, int pattern, int border,
                                  const double* lut, const int* xtab, int ow, const int* ytab, int oh,
                                  int out_kind, void* out, void* stream) {
  if (!raw || !out || (!xtab) != (!ytab)) return SCL_E_NULL;
  const int side_cap = 16384;
  const bool fused = xtab != nullptr;
  if (n < 1 || n > 65535) return SCL_E_SHAPE;
  if (sh < 2 || sw < 2 || sh > side_cap || sw > side_cap) return SCL_E_SHAPE;
  if (fused && (oh < 1 || ow < 1 || oh > side_cap || ow > side_cap)) return SCL_E_SHAPE;
  if (pattern < SCL_BAYER_RGGB || pattern > SCL_BAYER_GBRG) return SCL_E_SHAPE;
  if (border != SCL_BAYER_REFLECT && border != SCL_BAYER_MIRROR) return SCL_E_SHAPE;
  if (out_kind != SCL_FRAMES_U8 && out_kind != SCL_FRAMES_F32) return SCL_E_SHAPE;
  if (out_kind == SCL_FRAMES_F32 && (((uintptr_t)out) & 3u)) return SCL_E_SHAPE;
  if (((uintptr_t)lut) & 7u) return SCL_E_SHAPE;
  const hipStream_t st = (hipStream_t)stream;
  if (!fused) { oh = sh; ow = sw; }
  if (out_kind == SCL_FRAMES_U8) {
    if (fused) launch_debayer<true, unsigned char>(raw, n, sh, sw, pattern, border, lut, xtab, ow, ytab, oh, out, st);
    else launch_debayer<false, unsigned char>(raw, n, sh, sw, pattern, border, lut, xtab, ow, ytab, oh, out, st);
  } else {
    if (fused) launch_debayer<true, float>(raw, n, sh, sw, pattern, border, lut, xtab, ow, ytab, oh, out, st);
    else launch_debayer<false, float>(raw, n, sh, sw, pattern, border, lut, xtab, ow, ytab, oh, out, st);
  }
  return scl_launch_status();
}

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
