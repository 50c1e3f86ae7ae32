// Match saliency (evaluation/saliency.py; include/scl_hip.h has the contract): what parts of a frame
// made it match a place.  Two entry points:
//
//   scl_saliency_map      (activation, gradient) at the conv5_3 map [B, P, 512] -> one number per
//                         position [B, P] and the largest of them per image [B]
//   scl_saliency_overlay  that map, stretched bilinearly over the frame, through a colour table and
//                         blended into the uint8 frame
//
// ---- the map ------------------------------------------------------------------------------------
//   GRADCAM   w[b,c] = (sum_p grad[b,p,c]) (1/P),  map[b,p] = max(0, sum_c w[b,c] act[b,p,c])
//   GRADNORM  map[b,p] = sqrt(sum_c grad[b,p,c]^2)
// The channel weights of an image need every position of its gradient before the first position of
// its map can be written, and the call has no workspace to hand partial sums from workgroup to
// workgroup: ONE workgroup of 16 waves per image does both passes, the weights living in LDS in
// between — one launch.  What it costs is bandwidth, 2 P 512 elements per image through one CU
// (0.7 MB of float32 at 11 x 15, 4.9 MB at 30 x 40); the images of a batch run side by side.
//
// A wave owns whole positions (p = wave, wave + 16, ...): a position's 512 channels are one row of
// 2 KiB (float32; 1 KiB bf16) that the wave reads with 16-byte loads, eight channels per lane, four
// rows in flight per lane.  float32: lane l holds channels 4 l .. 4 l + 3 and 256 + 4 l .. 256 + 4 l + 3
// (two loads, each 1 KiB contiguous per wave); bf16: channels 8 l .. 8 l + 7 (one load).
//
// All sums are float32 in an order the code fixes: a lane adds its positions in ascending order, the
// 16 waves' partial sums are added wave 0 first, the channel sum of a position is the lane's eight
// products in channel order and then the xor butterfly over the lanes (every lane ends with the same
// bits: each step adds the same two numbers on both sides).  No atomics: the same input gives the
// same bits.  The maximum is taken with fmaxf from +0: every value written is >= +0 or NaN, a NaN
// stays in the map and does not become the maximum.
//
// ---- the overlay --------------------------------------------------------------------------------
// The host makes the axis tables (saliency.upsample_plan: two source indices and a float32 weight
// per destination row / column: they depend on the sizes alone); the kernel applies them in float32
// with every operation rounded on its own (overlay_value: contraction off, IEEE division), so
// overlay_np gives the same bytes.  A thread makes four adjacent pixels of the flat [B H W] pixel
// list: 12 bytes in, 12 bytes out, as three dwords where frame and out are 4-byte aligned (a thread's
// first byte is at 12 t), byte by byte otherwise and for the last, short group.  The colour table
// (768 bytes) is staged in LDS.  The tables are device memory the launcher cannot see: every index
// read from one is clamped into the map, so a wrong table gives wrong pixels and never a read outside.
#include "scl_common.h"

namespace {

constexpr int kC = SCL_VLAD_D;                     // channels of the conv5_3 map
constexpr int kMapThreads = 1024;
constexpr int kMapWaves = kMapThreads / SCL_WAVE;
constexpr int kRows = 4;                           // rows in flight per wave (8 measured the same: the CU's
                                                   // bandwidth is the limit, not the round trips)
static_assert(kC == 8 * SCL_WAVE, "eight channels per lane");

// the lane's eight channels of one row
template <typename T>
struct Row8;
template <>
struct Row8<float> {
  static __device__ __forceinline__ int channel(int lane, int i) {
    return (i < 4 ? 0 : kC / 2 - 4) + 4 * lane + i;
  }
  static __device__ __forceinline__ void load(const float* row, int lane, float* v) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(row + 4 * lane);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(row + kC / 2 + 4 * lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = lo[i];
      v[4 + i] = hi[i];
    }
  }
};
template <>
struct Row8<unsigned short> {
  static __device__ __forceinline__ int channel(int lane, int i) { return 8 * lane + i; }
  static __device__ __forceinline__ void load(const unsigned short* row, int lane, float* v) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(row + 8 * lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
};

template <typename T, int MODE>
__global__ __launch_bounds__(kMapThreads) void saliency_map_kernel(
    const T* __restrict__ act, const T* __restrict__ grad, int P, float inv_p,
    float* __restrict__ map_out, float* __restrict__ max_out) {
  __shared__ float part[kMapWaves][kC];            // 32 KiB: the waves' partial channel sums
  __shared__ float weight[kC];
  __shared__ float wave_top[kMapWaves];
  const int tid = threadIdx.x, lane = tid & (SCL_WAVE - 1), wave = tid / SCL_WAVE;
  const long long image = (long long)blockIdx.x * P * kC;
  const T* g = grad + image;
  float w8[8];
  if (MODE == SCL_SALIENCY_GRADCAM) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
    for (int p0 = wave; p0 < P; p0 += kRows * kMapWaves) {
      float v[kRows][8];
#pragma unroll
      for (int u = 0; u < kRows; ++u) {
        const int p = p0 + u * kMapWaves;
        if (p < P) Row8<T>::load(g + (long long)p * kC, lane, v[u]);
      }
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        if (p0 + u * kMapWaves < P) {
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] += v[u][i];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) part[wave][Row8<T>::channel(lane, i)] = acc[i];
    __syncthreads();
    if (tid < kC) {
      float s = part[0][tid];
      for (int k = 1; k < kMapWaves; ++k) s += part[k][tid];
      weight[tid] = s * inv_p;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) w8[i] = weight[Row8<T>::channel(lane, i)];
  }
  const T* src = MODE == SCL_SALIENCY_GRADCAM ? act + image : g;
  float* map = map_out + (long long)blockIdx.x * P;
  float top = 0.f;
  for (int p0 = wave; p0 < P; p0 += kRows * kMapWaves) {
    float v[kRows][8];
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const int p = p0 + u * kMapWaves;
      if (p < P) Row8<T>::load(src + (long long)p * kC, lane, v[u]);
    }
#pragma unroll
    for (int u = 0; u < kRows; ++u) {
      const int p = p0 + u * kMapWaves;
      if (p < P) {                                   // (the whole wave)
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d += (MODE == SCL_SALIENCY_GRADCAM ? w8[i] : v[u][i]) * v[u][i];
        d = wave_sum(d);
        const float r = MODE == SCL_SALIENCY_GRADCAM ? (d > 0.f ? d : (d != d ? d : 0.f)) : sqrtf(d);
        if (lane == 0) map[p] = r;
        top = fmaxf(top, r);
      }
    }
  }
  if (lane == 0) wave_top[wave] = top;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < kMapWaves; ++k) top = fmaxf(top, wave_top[k]);
    max_out[blockIdx.x] = top;
  }
}

template <typename T>
void launch_map(const void* act, const void* grad, int B, int P, int mode, float* map_out,
                float* max_out, hipStream_t st) {
  const float inv_p = 1.0f / (float)P;
  const T* a = static_cast<const T*>(act);
  const T* g = static_cast<const T*>(grad);
  if (mode == SCL_SALIENCY_GRADCAM)
    SCL_LAUNCH("saliency_map_kernel<GRADCAM>", (saliency_map_kernel<T, SCL_SALIENCY_GRADCAM>),
               dim3((unsigned)B), dim3(kMapThreads), 0, st, a, g, P, inv_p, map_out, max_out);
  else
    SCL_LAUNCH("saliency_map_kernel<GRADNORM>", (saliency_map_kernel<T, SCL_SALIENCY_GRADNORM>),
               dim3((unsigned)B), dim3(kMapThreads), 0, st, a, g, P, inv_p, map_out, max_out);
}

// ---- the overlay ----------------------------------------------------------------------------------
constexpr int kOvThreads = 256;
constexpr int kOvPixels = 4;                       // adjacent pixels per thread: 12 bytes
constexpr int kLutBytes = 256 * 3;

__device__ __forceinline__ int clamp_index(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the colour index of one pixel: float32, every operation rounded on its own
__device__ __forceinline__ int overlay_index(float m00, float m01, float m10, float m11, float tx,
                                             float ty, float scale) {
#pragma clang fp contract(off)
  const float top = m00 + (m01 - m00) * tx;
  const float bot = m10 + (m11 - m10) * tx;
  const float v = top + (bot - top) * ty;
  float r = scale > 0.f ? v / scale : 0.f;
  r = (r == r) ? (r < 0.f ? 0.f : (r > 1.f ? 1.f : r)) : 0.f;
  return (int)(r * 255.f + 0.5f);
}

__global__ __launch_bounds__(kOvThreads) void saliency_overlay_kernel(
    const float* __restrict__ map, const float* __restrict__ scale, int h, int w,
    const unsigned char* __restrict__ frame, int H, int W, long long total,
    const int* __restrict__ y0t, const int* __restrict__ y1t, const float* __restrict__ tyt,
    const int* __restrict__ x0t, const int* __restrict__ x1t, const float* __restrict__ txt,
    const unsigned char* __restrict__ lut, int alpha, unsigned char* __restrict__ out, int dwords) {
  __shared__ unsigned char table[kLutBytes];
  for (int i = threadIdx.x; i < kLutBytes; i += kOvThreads) table[i] = lut[i];
  __syncthreads();
  const long long first = ((long long)blockIdx.x * kOvThreads + threadIdx.x) * kOvPixels;
  if (first >= total) return;
  const int count = total - first < kOvPixels ? (int)(total - first) : kOvPixels;
  const bool wide = dwords && count == kOvPixels;
  const unsigned char* in = frame + 3 * first;
  unsigned char* dst = out + 3 * first;
  unsigned char px[3 * kOvPixels];
  if (wide) {
    const unsigned* in4 = reinterpret_cast<const unsigned*>(in);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const unsigned word = in4[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) px[4 * k + j] = (unsigned char)(word >> (8 * j));
    }
  } else {
    for (int k = 0; k < 3 * count; ++k) px[k] = in[k];
  }
  const long long frame_pixels = (long long)H * W;
  long long b = first / frame_pixels;
  const long long rest = first - b * frame_pixels;
  int y = (int)(rest / W), x = (int)(rest - (long long)y * W);
#pragma unroll
  for (int k = 0; k < kOvPixels; ++k) {
    if (k < count) {
      const float* m = map + b * h * w;
      const int y0 = clamp_index(y0t[y], h - 1) * w, y1 = clamp_index(y1t[y], h - 1) * w;
      const int x0 = clamp_index(x0t[x], w - 1), x1 = clamp_index(x1t[x], w - 1);
      const int q = overlay_index(m[y0 + x0], m[y0 + x1], m[y1 + x0], m[y1 + x1], txt[x], tyt[y], scale[b]);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        px[3 * k + c] = (unsigned char)((alpha * table[3 * q + c] + (256 - alpha) * px[3 * k + c] + 128) >> 8);
      if (++x == W) {
        x = 0;
        if (++y == H) {
          y = 0;
          ++b;
        }
      }
    }
  }
  if (wide) {
    unsigned* dst4 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      dst4[k] = (unsigned)px[4 * k] | ((unsigned)px[4 * k + 1] << 8) | ((unsigned)px[4 * k + 2] << 16) |
                ((unsigned)px[4 * k + 3] << 24);
  } else {
    for (int k = 0; k < 3 * count; ++k) dst[k] = px[k];
  }
}

bool saliency_aligned(const void* p, unsigned bytes) { return (((uintptr_t)p) & (bytes - 1u)) == 0; }

}  // namespace

extern "C" int scl_saliency_map(const void* act, const void* grad, int dtype, int B, int h, int w,
                                int mode, float* map_out, float* max_out, void* stream) {
  if (!grad || !map_out || !max_out || (mode == SCL_SALIENCY_GRADCAM && !act)) return SCL_E_NULL;
  if (B < 1 || B > SCL_SALIENCY_MAX_B || h < 1 || w < 1 || h > SCL_SALIENCY_MAX_SIDE ||
      w > SCL_SALIENCY_MAX_SIDE || (long long)h * w > SCL_SALIENCY_MAX_P)
    return SCL_E_SHAPE;
  if (!saliency_aligned(grad, 16) || (act && !saliency_aligned(act, 16)) || !saliency_aligned(map_out, 4) ||
      !saliency_aligned(max_out, 4))
    return SCL_E_SHAPE;
  if (dtype != SCL_DT_F32 && dtype != SCL_DT_BF16) return SCL_E_KIND;
  if (mode != SCL_SALIENCY_GRADCAM && mode != SCL_SALIENCY_GRADNORM) return SCL_E_KIND;
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == SCL_DT_F32)
    launch_map<float>(act, grad, B, h * w, mode, map_out, max_out, st);
  else
    launch_map<unsigned short>(act, grad, B, h * w, mode, map_out, max_out, st);
  return scl_launch_status();
}

extern "C" int scl_saliency_overlay(const float* map, const float* scale, int B, int h, int w,
                                    const void* frame, int H, int W, const int* y0, const int* y1,
                                    const float* ty, const int* x0, const int* x1, const float* tx,
                                    const void* lut, int alpha, void* out, void* stream) {
  if (!map || !scale || !frame || !y0 || !y1 || !ty || !x0 || !x1 || !tx || !lut || !out) return SCL_E_NULL;
  if (B < 1 || B > SCL_SALIENCY_MAX_B || h < 1 || w < 1 || h > SCL_SALIENCY_MAX_SIDE ||
      w > SCL_SALIENCY_MAX_SIDE || (long long)h * w > SCL_SALIENCY_MAX_P)
    return SCL_E_SHAPE;
  if (H < 1 || W < 1 || H > SCL_SALIENCY_MAX_SIDE || W > SCL_SALIENCY_MAX_SIDE) return SCL_E_SHAPE;
  const long long total = (long long)B * H * W;
  if (total > (1LL << 32) || alpha < 0 || alpha > 256) return SCL_E_SHAPE;
  if (!saliency_aligned(map, 4) || !saliency_aligned(scale, 4) || !saliency_aligned(ty, 4) ||
      !saliency_aligned(tx, 4) || !saliency_aligned(y0, 4) || !saliency_aligned(y1, 4) ||
      !saliency_aligned(x0, 4) || !saliency_aligned(x1, 4))
    return SCL_E_SHAPE;
  const int dwords = saliency_aligned(frame, 4) && saliency_aligned(out, 4);
  const long long groups = (total + kOvPixels - 1) / kOvPixels;
  const dim3 grid((unsigned)((groups + kOvThreads - 1) / kOvThreads));
  SCL_LAUNCH("saliency_overlay_kernel", saliency_overlay_kernel, grid, dim3(kOvThreads), 0,
             (hipStream_t)stream, map, scale, h, w, static_cast<const unsigned char*>(frame), H, W, total,
             y0, y1, ty, x0, x1, tx, static_cast<const unsigned char*>(lut), alpha,
             static_cast<unsigned char*>(out), dwords);
  return scl_launch_status();
}
