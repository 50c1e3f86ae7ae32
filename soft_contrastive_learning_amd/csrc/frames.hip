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

}  // namespace

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
