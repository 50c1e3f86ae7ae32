// The parameter update: TensorFlow's ApplyAdam / ApplyMomentum over a list of float32 segments in
// one launch (scl_apply_adam, scl_apply_momentum), and one pass over the flat gradient buffer for
// its squared norm and a non-finite flag (scl_grad_stats).  train/optim.py is the caller.
//
// BIT-EXACT BY CONSTRUCTION.  oracle/adam_np.py states the update as a sequence of float32
// operations, each rounded on its own.  The pragma below keeps the compiler from contracting
// a * b + c into a fused multiply-add anywhere in this file; `/` and sqrtf are hipcc's default
// correctly rounded expansions (v_div_scale / v_div_fmas / v_div_fixup, the scaled and refined
// v_sqrt_f32) and float32 denormals are kept (the kernel descriptor's float_denorm_mode_32 = 3).
// The constants 1 - beta1, 1 - beta2 are float32 subtractions of the float32 betas, as NumPy's are
// (1 - float32(0.9) = 0.100000024, not 0.1).
//
// Pure streaming: 28 bytes per element for Adam (var, m, v read and written, g read), no reuse,
// no LDS.  A workgroup serves one chunk — SCL_OPTIM_CHUNK_GROUPS 16-byte groups, kUnroll per lane,
// every load issued before the first store — of ONE segment, which it finds by binary search over
// the rows' first_chunk.  Alignment is decided per segment, as csrc/frames.hip does per frame: the
// 0..3 values in front of var's first 16-byte boundary and the last 0..3 go one by one (chunk 0's
// first eight lanes); the body is 16-byte vectors, aligned for var; the other three arrays of a
// row — the gradients above all, views into one flat buffer — may sit at another alignment behind
// the same head, so they go through a vector type that promises 4 bytes only (one dwordx4
// instruction on gfx950, whose global memory path takes it at any dword address).
#pragma clang fp contract(off)
#include "scl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                          // 16-byte groups per lane
constexpr int kChunkGroups = SCL_OPTIM_CHUNK_GROUPS;
static_assert(kThreads * kUnroll == kChunkGroups, "a workgroup serves exactly one chunk");

// The rows hold plain addresses; the kernels know them to be device memory (global_load / global_store
// instead of the flat forms).
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float cgfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) const f32x4 cgf32x4;
// the same four floats at an address that is only 4-byte aligned
typedef __attribute__((address_space(1), aligned(4))) f32x4 gf32x4_a4;
typedef __attribute__((address_space(1), aligned(4))) const f32x4 cgf32x4_a4;

__device__ __forceinline__ f32x4 ld4(cgfloat* p) { return *reinterpret_cast<cgf32x4_a4*>(p); }
__device__ __forceinline__ void st4(gfloat* p, f32x4 x) { *reinterpret_cast<gf32x4_a4*>(p) = x; }

// what every element of one call shares
struct AdamConst {
  float one_minus_b1, one_minus_b2, alpha, eps;
};
struct MomentumConst {
  float lr, momentum;
};

__device__ __forceinline__ void update1(const AdamConst& k, float g, float& var, float& m, float& v) {
#pragma clang fp contract(off)
  m = m + (g - m) * k.one_minus_b1;
  v = v + (g * g - v) * k.one_minus_b2;
  var = var - (m * k.alpha) / (sqrtf(v) + k.eps);
}
__device__ __forceinline__ void update1(const MomentumConst& k, float g, float& var, float& a, float&) {
#pragma clang fp contract(off)
  a = a * k.momentum + g;
  var = var - k.lr * a;
}

// `count` (<= kChunkGroups) 16-byte groups of one chunk; FULL: count == kChunkGroups, no lane is idle
// and no load waits behind a branch
template <int SLOTS, bool FULL, class K>
__device__ __forceinline__ void apply_groups(gfloat* bv, cgfloat* bg, gfloat* b0, gfloat* b1, int count,
                                             const K& k) {
  const int tid = threadIdx.x;
  f32x4 x[kUnroll], g[kUnroll], a[kUnroll], b[kUnroll];
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int gi = tid + u * kThreads;
    if (FULL || gi < count) {
      x[u] = *reinterpret_cast<cgf32x4*>(bv + 4 * gi);
      g[u] = ld4(bg + 4 * gi);
      a[u] = ld4(b0 + 4 * gi);
      if (SLOTS == 2) b[u] = ld4(b1 + 4 * gi);
    }
  }
#pragma unroll
  for (int u = 0; u < kUnroll; ++u) {
    const int gi = tid + u * kThreads;
    if (FULL || gi < count) {
      if (SLOTS != 2) b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float xv = x[u][j], av = a[u][j], bw = b[u][j];
        update1(k, g[u][j], xv, av, bw);
        x[u][j] = xv;
        a[u][j] = av;
        b[u][j] = bw;
      }
      *reinterpret_cast<gf32x4*>(bv + 4 * gi) = x[u];
      st4(b0 + 4 * gi, a[u]);
      if (SLOTS == 2) st4(b1 + 4 * gi, b[u]);
    }
  }
}

// SLOTS = 2: Adam (m, v); 1: momentum (the accumulator; slot1 is never touched)
template <int SLOTS, class K>
__device__ __forceinline__ void apply_chunk(const SclOptimSeg& s, long long chunk, const K& k) {
  const int tid = threadIdx.x;
  gfloat* var = (gfloat*)s.var;
  cgfloat* grad = (cgfloat*)s.grad;
  gfloat* s0 = (gfloat*)s.slot0;
  gfloat* s1 = SLOTS == 2 ? (gfloat*)s.slot1 : nullptr;
  const long long n = s.n;

  // values in front of var's first 16-byte aligned address (var is 4-byte aligned)
  long long head = (long long)(((16u - (unsigned)((uintptr_t)var & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const long long groups = (n - head) >> 2;
  const long long tail = head + 4 * groups;        // first element after the body

  if (chunk == 0 && tid < 8) {                     // head: lanes 0..3, tail: lanes 4..7
    const long long i = tid < 4 ? tid : tail + (tid - 4);
    const bool mine = tid < 4 ? tid < head : i < n;
    if (mine) {
      float x = var[i], a = s0[i], b = SLOTS == 2 ? s1[i] : 0.f;
      update1(k, grad[i], x, a, b);
      var[i] = x;
      s0[i] = a;
      if (SLOTS == 2) s1[i] = b;
    }
  }

  const long long first = chunk * kChunkGroups;
  if (first >= groups) return;                     // block-uniform
  // 16-byte aligned for var; the other three as they come
  gfloat* bv = var + head + 4 * first;
  cgfloat* bg = grad + head + 4 * first;
  gfloat* b0 = s0 + head + 4 * first;
  gfloat* b1 = SLOTS == 2 ? s1 + head + 4 * first : nullptr;
  if (groups - first >= kChunkGroups)              // every chunk of a segment but its last
    apply_groups<SLOTS, true>(bv, bg, b0, b1, kChunkGroups, k);
  else
    apply_groups<SLOTS, false>(bv, bg, b0, b1, (int)(groups - first), k);
}

// the row that serves chunk b: the last one whose first_chunk is <= b
__device__ __forceinline__ int find_row(const SclOptimSeg* __restrict__ segs, int nseg, long long b) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].first_chunk <= b)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void apply_adam_kernel(
    const SclOptimSeg* __restrict__ segs, int nseg, SclOptimState* state, const float* __restrict__ lr,
    float beta1, float beta2, float epsilon, const unsigned* __restrict__ skip) {
  const bool skipped = skip != nullptr && *skip != 0u;
  const float b1p = state->beta1_power, b2p = state->beta2_power;
  if (!skipped) {
    AdamConst k;
    k.one_minus_b1 = 1.0f - beta1;
    k.one_minus_b2 = 1.0f - beta2;
    k.alpha = (*lr * sqrtf(1.0f - b2p)) / (1.0f - b1p);
    k.eps = epsilon;
    const long long b = blockIdx.x;
    const SclOptimSeg s = segs[find_row(segs, nseg, b)];
    const long long chunk = b - s.first_chunk;
    if (chunk >= 0 && s.n >= 1) apply_chunk<2>(s, chunk, k);
  }
  // The state advances once, after every workgroup has read the old powers: a workgroup draws its
  // ticket behind a barrier that all its lanes reach with their reads of the state complete (the
  // barrier's release fence keeps the compiler from sinking them, its wait keeps the hardware),
  // and only the one that draws the last ticket writes.  Nothing waits for anything.
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = atomicAdd(&state->ticket, 1u);
    if (t == gridDim.x - 1) {
      if (!skipped) {
        state->beta1_power = b1p * beta1;
        state->beta2_power = b2p * beta2;
        state->step = state->step + 1;
      }
      atomicExch(&state->ticket, 0u);
    }
  }
}

__global__ __launch_bounds__(kThreads) void apply_momentum_kernel(
    const SclOptimSeg* __restrict__ segs, int nseg, const float* __restrict__ lr, float momentum,
    const unsigned* __restrict__ skip) {
  if (skip != nullptr && *skip != 0u) return;
  MomentumConst k;
  k.lr = *lr;
  k.momentum = momentum;
  const long long b = blockIdx.x;
  const SclOptimSeg s = segs[find_row(segs, nseg, b)];
  const long long chunk = b - s.first_chunk;
  if (chunk >= 0 && s.n >= 1) apply_chunk<1>(s, chunk, k);
}

// ---- scl_grad_stats ------------------------------------------------------------------------

constexpr int kStatsMaxBlocks = 1024;
constexpr long long kStatsMaxN = 1LL << 40;

struct Stats {
  double ss;
  double bad;
};
__device__ __forceinline__ void take(Stats& s, float x) {
  if ((__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) {
    s.bad += 1.0;
  } else {
    const double d = (double)x;
    s.ss += d * d;
  }
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// the same value in every lane of wave 0; one fixed order
__device__ __forceinline__ Stats block_sum(Stats s, double* scratch /* 2 * waves */) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = kThreads / 64;
  s.ss = wave_sum_f64(s.ss);
  s.bad = wave_sum_f64(s.bad);
  if (lane == 0) {
    scratch[2 * wid] = s.ss;
    scratch[2 * wid + 1] = s.bad;
  }
  __syncthreads();
  Stats r{scratch[0], scratch[1]};
  for (int i = 1; i < nw; ++i) {
    r.ss += scratch[2 * i];
    r.bad += scratch[2 * i + 1];
  }
  return r;
}

__global__ __launch_bounds__(kThreads) void grad_stats_partial_kernel(const float* __restrict__ g,
                                                                      long long n,
                                                                      double* __restrict__ partial) {
  __shared__ double scratch[2 * (kThreads / 64)];
  const int tid = threadIdx.x;
  long long head = (long long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);
  if (head > n) head = n;
  const long long groups = (n - head) >> 2;
  const long long tail = head + 4 * groups;
  Stats s{0.0, 0.0};
  if (blockIdx.x == 0 && tid < 8) {                // head: lanes 0..3, tail: lanes 4..7
    const long long i = tid < 4 ? tid : tail + (tid - 4);
    const bool mine = tid < 4 ? tid < head : i < n;
    if (mine) take(s, g[i]);
  }
  const f32x4* body = reinterpret_cast<const f32x4*>(g + head);
  const long long stride = (long long)gridDim.x * kChunkGroups;
  for (long long base = (long long)blockIdx.x * kChunkGroups; base < groups; base += stride) {
    f32x4 x[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long gi = base + u * kThreads + tid;
      if (gi < groups) x[u] = body[gi];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long long gi = base + u * kThreads + tid;
      if (gi < groups) {
#pragma unroll
        for (int j = 0; j < 4; ++j) take(s, x[u][j]);
      }
    }
  }
  const Stats r = block_sum(s, scratch);
  if (tid == 0) {
    partial[2 * blockIdx.x] = r.ss;
    partial[2 * blockIdx.x + 1] = r.bad;
  }
}

__global__ __launch_bounds__(kThreads) void grad_stats_finish_kernel(const double* __restrict__ partial,
                                                                     int nblocks, double* __restrict__ out,
                                                                     unsigned* __restrict__ flag) {
  __shared__ double scratch[2 * (kThreads / 64)];
  Stats s{0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += kThreads) {
    s.ss += partial[2 * i];
    s.bad += partial[2 * i + 1];
  }
  const Stats r = block_sum(s, scratch);
  if (threadIdx.x == 0) {
    out[0] = r.ss;
    out[1] = r.bad;
    *flag = r.bad > 0.0 ? 1u : 0u;
  }
}

int stats_blocks(long long n) {
  const long long chunks = (n / 4 + kChunkGroups - 1) / kChunkGroups;
  return (int)(chunks < 1 ? 1 : (chunks > kStatsMaxBlocks ? kStatsMaxBlocks : chunks));
}

int check_table(const void* segs, int nseg, long long total_chunks, const void* lr) {
  if (!segs || !lr) return SCL_E_NULL;
  if (nseg < 1 || nseg > (1 << 20) || total_chunks < nseg || total_chunks > (1LL << 24))
    return SCL_E_SHAPE;
  return 0;
}

}  // namespace

extern "C" int scl_apply_adam(const SclOptimSeg* segs, int nseg, long long total_chunks,
                              SclOptimState* state, const float* lr, float beta1, float beta2,
                              float epsilon, const unsigned* skip, void* stream) {
  if (!state) return SCL_E_NULL;
  if (const int e = check_table(segs, nseg, total_chunks, lr)) return e;
  SCL_LAUNCH("apply_adam_kernel", apply_adam_kernel, dim3((unsigned)total_chunks), dim3(kThreads), 0,
             (hipStream_t)stream, segs, nseg, state, lr, beta1, beta2, epsilon, skip);
  return scl_launch_status();
}

extern "C" int scl_apply_momentum(const SclOptimSeg* segs, int nseg, long long total_chunks,
                                  const float* lr, float momentum, const unsigned* skip, void* stream) {
  if (const int e = check_table(segs, nseg, total_chunks, lr)) return e;
  SCL_LAUNCH("apply_momentum_kernel", apply_momentum_kernel, dim3((unsigned)total_chunks),
             dim3(kThreads), 0, (hipStream_t)stream, segs, nseg, lr, momentum, skip);
  return scl_launch_status();
}

extern "C" size_t scl_grad_stats_workspace_bytes(long long n) {
  if (n < 1 || n > kStatsMaxN) return 0;
  return scl_round256((size_t)stats_blocks(n) * 2 * sizeof(double));
}

extern "C" int scl_grad_stats(const float* g, long long n, double* out, unsigned* flag, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!g || !out || !flag || !workspace) return SCL_E_NULL;
  if (n < 1 || n > kStatsMaxN || (((uintptr_t)g) & 3u)) return SCL_E_SHAPE;
  if (workspace_bytes < scl_grad_stats_workspace_bytes(n) || !scl_aligned256(workspace))
    return SCL_E_WORKSPACE;
  const int blocks = stats_blocks(n);
  double* partial = static_cast<double*>(workspace);
  SCL_LAUNCH("grad_stats_partial_kernel", grad_stats_partial_kernel, dim3(blocks), dim3(kThreads), 0,
             (hipStream_t)stream, g, n, partial);
  SCL_LAUNCH("grad_stats_finish_kernel", grad_stats_finish_kernel, dim3(1), dim3(kThreads), 0,
             (hipStream_t)stream, static_cast<const double*>(partial), blocks, out, flag);
  return scl_launch_status();
}
