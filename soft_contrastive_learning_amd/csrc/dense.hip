// Dense reduction heads on gfx950: the `tf.layers.dense` stack the reference puts on top of the
// descriptor with --reduction 1fc|2fc|3fc (train/train.py:631-644, evaluation/inference.py:97-109).
//
// Skinny float32 GEMMs: M = 1..256 rows (images) against a large weight W [K, N] in TF's kernel
// layout (row k = input feature, N contiguous).  At M <= 32 each weight element takes part in 32
// padded rows = 16 FLOP per byte read, below the float32-MFMA ridge point (155 TF / 6.3 TB/s): the
// three kernels below are built to stream W (or dW) once at HBM rate.
//   1. dense_fwd_kernel     Y = X W (+ b, ReLU).  A wave owns 128 output columns x 32 or 64 rows
//                           and one K slice; every lane loads float4s of W (4 columns) so that one
//                           wave-instruction reads two 512-byte row segments, and runs each of the
//                           4 columns through its own v_mfma_f32_32x32x2_f32 accumulator.  The K
//                           split S is a function of (K, N) only; S > 1 writes f32 partial slabs.
//   2. dense_bwd_data_kernel dX = dY' W^T, dY' = dY masked by Y > 0 for a ReLU layer.  A wave
//                           owns 32 columns of dX (32 rows of W, 128 contiguous bytes of each per
//                           unit of 32 contraction values) and one N slice; partial slabs as above.
//   3. dense_reduce_kernel  sums the slabs in slice order (+ b, ReLU): fixed order, no atomics —
//                           results are bitwise reproducible, and since S
//                           does not depend on M, row m of Y / dX is the same bits whatever other
//                           rows share the call (the reference's padded inference passes).
//   4. dense_wgrad_kernel   dW = X^T dY', db = sum_m dY'.  Rank-M update, bound by writing dW: a
//                           wave owns a 32 x 128 tile, loops over M in fixed order and stores each
//                           accumulator register as float4s (two 512-byte row segments per
//                           instruction).  No split, no workspace.
// v_mfma_f32_32x32x2_f32 is an exact f32 product chain; all sums are plain float32.
#include "scl_common.h"

namespace {

constexpr int kThreads = 256;          // four independent waves per workgroup
constexpr int kTargetWaves = 2048;     // waves a split aims for (8 per CU on 256 CUs)
constexpr int kMinFwdSlice = 256;      // K rows per forward slice at the least
constexpr int kMinBwdSlice = 256;      // N values per backward-data slice at the least

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// four consecutive floats p[0..3] of which the first `valid` exist (valid <= 0: none)
template <bool VEC>
__device__ __forceinline__ f32x4 load4(const float* p, int valid) {
  if (VEC && valid >= 4) return *reinterpret_cast<const f32x4*>(p);
  f32x4 r = zero4();
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < valid) r[c] = p[c];
  return r;
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, f32x4 v, int valid) {
  if (VEC && valid >= 4) {
    *reinterpret_cast<f32x4*>(p) = v;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (c < valid) p[c] = v[c];
}

// ReLU' of a layer output: g where y > 0, +0 elsewhere
__device__ __forceinline__ f32x4 relu_grad4(f32x4 g, f32x4 y) {
  f32x4 r;
#pragma unroll
  for (int c = 0; c < 4; ++c) r[c] = y[c] > 0.f ? g[c] : 0.f;
  return r;
}

// ---- forward --------------------------------------------------------------------------------
// wave -> (m chunk fastest, then 128-column group, then K slice).  Lane l = (j = l & 31, h = l >> 5)
// loads, per unit of 8 K rows kb..kb+7, W[kb + 4h + q][n .. n+3] (q = 0..3, n = col0 + 4j) and
// X[m][kb + 4h .. +3]; MFMA (q, c) takes A[i][h] = X[m0 + i][kb + 4h + q] and
// B[h][j] = W[kb + 4h + q][n + c], so accumulator c holds Y[m0 + row][n + c].
template <int MB, bool VEC>
struct FwdStage {
  f32x4 w[2][4];
  f32x4 x[2][MB];
};

template <int MB, bool VEC>
__device__ __forceinline__ void fwd_load(FwdStage<MB, VEC>& st, const float* __restrict__ x, int64_t ld_x,
                                         const float* __restrict__ w, int64_t ld_w, int M, int N,
                                         int kb, int kend, int m0, int n, int j, int h) {
  const int ncols = N - n;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int k4 = kb + 8 * u + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kr = k4 + q;
      st.w[u][q] = kr < kend ? load4<VEC>(w + (int64_t)kr * ld_w + n, ncols) : zero4();
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      const int m = m0 + 32 * mb + j;
      st.x[u][mb] = m < M ? load4<VEC>(x + (int64_t)m * ld_x + k4, kend - k4) : zero4();
    }
  }
}

template <int MB, bool VEC>
__global__ __launch_bounds__(kThreads) void dense_fwd_kernel(
    const float* __restrict__ x, int64_t ld_x, const float* __restrict__ w, int64_t ld_w,
    const float* __restrict__ bias, int M, int K, int N, int relu, float* __restrict__ out,
    int64_t ld_out, int64_t slab, int S, int kslice, int nmc, int ncg) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (wv >= (int64_t)nmc * ncg * S) return;
  const int mc = (int)(wv % nmc);
  const int64_t rest = wv / nmc;
  const int cg = (int)(rest % ncg), s = (int)(rest / ncg);
  const int j = lane & 31, h = lane >> 5;
  const int m0 = mc * 32 * MB, n = cg * 128 + 4 * j;
  const int kbeg = s * kslice, kend = min(K, kbeg + kslice);

  f32x16 acc[MB][4];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[mb][c] = zero16();

  FwdStage<MB, VEC> cur, nxt;
  fwd_load<MB, VEC>(cur, x, ld_x, w, ld_w, M, N, kbeg, kend, m0, n, j, h);
  for (int kb = kbeg; kb < kend; kb += 16) {
    if (kb + 16 < kend) fwd_load<MB, VEC>(nxt, x, ld_x, w, ld_w, M, N, kb + 16, kend, m0, n, j, h);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[mb][c] = mfma32(cur.x[u][mb][q], cur.w[u][q][c], acc[mb][c]);
    cur = nxt;
  }

  float* dst = out + (int64_t)s * slab;
  const int ncols = N - n;
  f32x4 b = zero4();
  const bool epi = S == 1;
  if (epi && bias) b = load4<false>(bias + n, ncols);
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * mb + acc_row(r, h);
      if (m >= M || ncols <= 0) continue;
      f32x4 v = f32x4{acc[mb][0][r], acc[mb][1][r], acc[mb][2][r], acc[mb][3][r]};
      if (epi) {
        v += b;
        if (relu)
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c], 0.f);
      }
      store4<VEC>(dst + (int64_t)m * ld_out + n, v, ncols);
    }
}

// ---- backward data --------------------------------------------------------------------------
// wave -> (m chunk fastest, then 32-column tile of dX, then N slice).  Lane (j, h) loads, per unit
// of 32 contraction values nb..nb+31, W[k0 + j][nb + 16h + 4f .. +3] (f = 0..3: 64 contiguous bytes;
// the lane pair covers 128) and dY'[m][same columns]; MFMA (f, e) takes
// A[i][h] = dY'[m0 + i][nb + 16h + 4f + e] and B[h][j] = W[k0 + j][nb + 16h + 4f + e].
template <int MB>
struct BwdStage {
  f32x4 w[4];
  f32x4 g[MB][4];
};

template <int MB, bool VEC>
__device__ __forceinline__ void bwd_load(BwdStage<MB>& st, const float* __restrict__ gy, int64_t ld_gy,
                                         const float* __restrict__ y, int64_t ld_y,
                                         const float* __restrict__ w, int64_t ld_w, int M, int K,
                                         int nb, int nend, int m0, int k, int j, int h) {
  const int c0 = nb + 16 * h;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int c = c0 + 4 * f;
    st.w[f] = k < K ? load4<VEC>(w + (int64_t)k * ld_w + c, nend - c) : zero4();
  }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = m0 + 32 * mb + j;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int c = c0 + 4 * f;
      f32x4 g = m < M ? load4<VEC>(gy + (int64_t)m * ld_gy + c, nend - c) : zero4();
      if (y && m < M) g = relu_grad4(g, load4<VEC>(y + (int64_t)m * ld_y + c, nend - c));
      st.g[mb][f] = g;
    }
  }
}

template <int MB, bool VEC>
__global__ __launch_bounds__(kThreads) void dense_bwd_data_kernel(
    const float* __restrict__ gy, int64_t ld_gy, const float* __restrict__ y, int64_t ld_y,
    const float* __restrict__ w, int64_t ld_w, int M, int K, int N, float* __restrict__ out,
    int64_t ld_out, int64_t slab, int S, int nslice, int nmc, int nkt) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (wv >= (int64_t)nmc * nkt * S) return;
  const int mc = (int)(wv % nmc);
  const int64_t rest = wv / nmc;
  const int kt = (int)(rest % nkt), s = (int)(rest / nkt);
  const int j = lane & 31, h = lane >> 5;
  const int m0 = mc * 32 * MB, k = kt * 32 + j;
  const int nbeg = s * nslice, nend = min(N, nbeg + nslice);

  f32x16 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) acc[mb] = zero16();

  BwdStage<MB> cur, nxt;
  bwd_load<MB, VEC>(cur, gy, ld_gy, y, ld_y, w, ld_w, M, K, nbeg, nend, m0, k, j, h);
  for (int nb = nbeg; nb < nend; nb += 32) {
    if (nb + 32 < nend) bwd_load<MB, VEC>(nxt, gy, ld_gy, y, ld_y, w, ld_w, M, K, nb + 32, nend, m0, k, j, h);
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[mb] = mfma32(cur.g[mb][f][e], cur.w[f][e], acc[mb]);
    cur = nxt;
  }

  float* dst = out + (int64_t)s * slab;
  const int kc = kt * 32 + j;                     // output column of this lane
  if (kc >= K) return;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + 32 * mb + acc_row(r, h);
      if (m < M) dst[(int64_t)m * ld_out + kc] = acc[mb][r];
    }
}

// ---- slab reduction: out[m][n] = sum_s part[s][m][n] (+ bias[n], ReLU), s in order -----------
__global__ __launch_bounds__(kThreads) void dense_reduce_kernel(
    const float* __restrict__ part, int64_t ld_part, int64_t slab, int S, const float* __restrict__ bias,
    int relu, int M, int N, float* __restrict__ out, int64_t ld_out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)M * N) return;
  const int m = (int)(i / N), n = (int)(i % N);
  const float* p = part + (int64_t)m * ld_part + n;
  float v = p[0];
  for (int s = 1; s < S; ++s) v += p[(int64_t)s * slab];
  if (bias) v += bias[n];
  if (relu) v = fmaxf(v, 0.f);
  out[(int64_t)m * ld_out + n] = v;
}

// ---- weight and bias gradient -----------------------------------------------------------------
// wave -> (128-column group fastest, then 32-row tile of dW).  Lane (j, h) supplies, per pair of
// rows m, m + 1: A[i = j][h] = X[m + h][k0 + j] and B[h][j] = dY'[m + h][n + c] (n = col0 + 4j);
// accumulator c holds dW[k0 + row][n + c].  Four pairs are loaded ahead of their MFMAs.
template <bool VEC>
struct WgStage {
  float a[4];
  f32x4 b[4];
};

template <bool VEC>
__device__ __forceinline__ void wg_load(WgStage<VEC>& st, const float* __restrict__ x, int64_t ld_x,
                                        const float* __restrict__ gy, int64_t ld_gy,
                                        const float* __restrict__ y, int64_t ld_y, int M, int K,
                                        int N, int mb, int k, int n, int h) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int m = mb + 2 * p + h;
    const bool ok = m < M;
    st.a[p] = ok && k < K ? x[(int64_t)m * ld_x + k] : 0.f;
    f32x4 g = ok ? load4<VEC>(gy + (int64_t)m * ld_gy + n, N - n) : zero4();
    if (y && ok) g = relu_grad4(g, load4<VEC>(y + (int64_t)m * ld_y + n, N - n));
    st.b[p] = g;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void dense_wgrad_kernel(
    const float* __restrict__ x, int64_t ld_x, const float* __restrict__ gy, int64_t ld_gy,
    const float* __restrict__ y, int64_t ld_y, int M, int K, int N, float* __restrict__ gw,
    int64_t ld_gw, float* __restrict__ gb, int nkt, int ncg) {
  const int lane = threadIdx.x & 63;
  const int64_t wv = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (wv >= (int64_t)nkt * ncg) return;
  const int cg = (int)(wv % ncg), kt = (int)(wv / ncg);
  const int j = lane & 31, h = lane >> 5;
  const int k0 = kt * 32, k = k0 + j, n = cg * 128 + 4 * j;

  f32x16 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = zero16();
  WgStage<VEC> cur, nxt;
  wg_load<VEC>(cur, x, ld_x, gy, ld_gy, y, ld_y, M, K, N, 0, k, n, h);
  for (int mb = 0; mb < M; mb += 8) {
    if (mb + 8 < M) wg_load<VEC>(nxt, x, ld_x, gy, ld_gy, y, ld_y, M, K, N, mb + 8, k, n, h);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = mfma32(cur.a[p], cur.b[p][c], acc[c]);
    cur = nxt;
  }

  const int ncols = N - n;
  if (ncols > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = k0 + acc_row(r, h);
      if (row < K)
        store4<VEC>(gw + (int64_t)row * ld_gw + n, f32x4{acc[0][r], acc[1][r], acc[2][r], acc[3][r]},
                    ncols);
    }
  }
  // db: the waves of the first row tile, lanes of the lower half, rows in order
  if (gb && kt == 0 && h == 0 && ncols > 0) {
    f32x4 sum = zero4();
    for (int m = 0; m < M; ++m) {
      f32x4 g = load4<VEC>(gy + (int64_t)m * ld_gy + n, ncols);
      if (y) g = relu_grad4(g, load4<VEC>(y + (int64_t)m * ld_y + n, ncols));
      sum += g;
    }
    store4<false>(gb + n, sum, ncols);
  }
}

// ---- host side ----------------------------------------------------------------------------------
bool valid_shape(int M, int K, int N) { return M >= 1 && M <= 256 && K >= 1 && N >= 1; }
int chunk_rows(int M) { return M <= 32 ? 32 : 64; }
bool al16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
bool ld4(int64_t ld) { return (ld & 3) == 0; }
int64_t round4(int64_t v) { return (v + 3) & ~(int64_t)3; }
int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// K split of the forward: a function of (K, N) only — never of M — so a row's bits do not
// depend on the rows that share the call.  Slices are whole 16-row stages.
void fwd_split(int K, int N, int* S, int* kslice) {
  const int ncg = cdiv(N, 128);
  int s = cdiv(kTargetWaves, ncg);
  const int smax = cdiv(K, kMinFwdSlice);
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  int ks = cdiv(cdiv(K, s), 16) * 16;
  *kslice = ks;
  *S = cdiv(K, ks);
}

void bwd_split(int K, int N, int* S, int* nslice) {
  const int nkt = cdiv(K, 32);
  int s = cdiv(kTargetWaves, nkt);
  const int smax = cdiv(N, kMinBwdSlice);
  if (s > smax) s = smax;
  if (s < 1) s = 1;
  int ns = cdiv(cdiv(N, s), 32) * 32;
  *nslice = ns;
  *S = cdiv(N, ns);
}

int launch_reduce(const float* part, int64_t ld_part, int64_t slab, int S, const float* bias,
                  int relu, int M, int N, float* out, int64_t ld_out, hipStream_t st) {
  const int blocks = cdiv((int64_t)M * N, kThreads);
  SCL_LAUNCH("dense_reduce_kernel", dense_reduce_kernel, dim3(blocks), dim3(kThreads), 0, st, part,
             ld_part, slab, S, bias, relu, M, N, out, ld_out);
  return scl_launch_status();
}

}  // namespace

extern "C" size_t scl_dense_fwd_workspace_bytes(int M, int K, int N) {
  if (!valid_shape(M, K, N)) return 0;
  int S, ks;
  fwd_split(K, N, &S, &ks);
  return S > 1 ? scl_round256((size_t)S * M * round4(N) * sizeof(float)) : 0;
}

extern "C" size_t scl_dense_bwd_data_workspace_bytes(int M, int K, int N) {
  if (!valid_shape(M, K, N)) return 0;
  int S, ns;
  bwd_split(K, N, &S, &ns);
  return S > 1 ? scl_round256((size_t)S * M * round4(K) * sizeof(float)) : 0;
}

extern "C" int scl_dense_fwd(const float* x, int64_t ld_x, const float* w, int64_t ld_w,
                             const float* bias, int M, int K, int N, int relu, float* y,
                             int64_t ld_y, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !w || !y) return SCL_E_NULL;
  if (!valid_shape(M, K, N) || ld_x < K || ld_w < N || ld_y < N) return SCL_E_SHAPE;
  int S, kslice;
  fwd_split(K, N, &S, &kslice);
  const size_t need = scl_dense_fwd_workspace_bytes(M, K, N);
  if (need && (!workspace || workspace_bytes < need || !scl_aligned256(workspace)))
    return SCL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* out = S > 1 ? static_cast<float*>(workspace) : y;
  const int64_t ld_out = S > 1 ? round4(N) : ld_y;
  const int64_t slab = S > 1 ? (int64_t)M * ld_out : 0;
  const bool vec = al16(x) && al16(w) && al16(out) && ld4(ld_x) && ld4(ld_w) && ld4(ld_out);
  const int rows = chunk_rows(M), nmc = cdiv(M, rows), ncg = cdiv(N, 128);
  const int blocks = cdiv((int64_t)nmc * ncg * S, kThreads / 64);
#define SCL_DENSE_FWD(MB, V)                                                                       \
  SCL_LAUNCH("dense_fwd_kernel", (dense_fwd_kernel<MB, V>), dim3(blocks), dim3(kThreads), 0, st, x, \
             ld_x, w, ld_w, bias, M, K, N, relu, out, ld_out, slab, S, kslice, nmc, ncg)
  if (rows == 32) {
    if (vec) SCL_DENSE_FWD(1, true); else SCL_DENSE_FWD(1, false);
  } else {
    if (vec) SCL_DENSE_FWD(2, true); else SCL_DENSE_FWD(2, false);
  }
#undef SCL_DENSE_FWD
  int e = scl_launch_status();
  if (e || S == 1) return e;
  return launch_reduce(out, ld_out, slab, S, bias, relu, M, N, y, ld_y, st);
}

extern "C" int scl_dense_bwd_data(const float* gy, int64_t ld_gy, const float* y, int64_t ld_y,
                                  const float* w, int64_t ld_w, int M, int K, int N, float* gx,
                                  int64_t ld_gx, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  if (!gy || !w || !gx) return SCL_E_NULL;
  if (!valid_shape(M, K, N) || ld_gy < N || ld_w < N || ld_gx < K || (y && ld_y < N))
    return SCL_E_SHAPE;
  int S, nslice;
  bwd_split(K, N, &S, &nslice);
  const size_t need = scl_dense_bwd_data_workspace_bytes(M, K, N);
  if (need && (!workspace || workspace_bytes < need || !scl_aligned256(workspace)))
    return SCL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float* out = S > 1 ? static_cast<float*>(workspace) : gx;
  const int64_t ld_out = S > 1 ? round4(K) : ld_gx;
  const int64_t slab = S > 1 ? (int64_t)M * ld_out : 0;
  const bool vec = al16(gy) && al16(w) && ld4(ld_gy) && ld4(ld_w) && (!y || (al16(y) && ld4(ld_y)));
  const int rows = chunk_rows(M), nmc = cdiv(M, rows), nkt = cdiv(K, 32);
  const int blocks = cdiv((int64_t)nmc * nkt * S, kThreads / 64);
#define SCL_DENSE_BWD(MB, V)                                                                        \
  SCL_LAUNCH("dense_bwd_data_kernel", (dense_bwd_data_kernel<MB, V>), dim3(blocks), dim3(kThreads), \
             0, st, gy, ld_gy, y, ld_y, w, ld_w, M, K, N, out, ld_out, slab, S, nslice, nmc, nkt)
  if (rows == 32) {
    if (vec) SCL_DENSE_BWD(1, true); else SCL_DENSE_BWD(1, false);
  } else {
    if (vec) SCL_DENSE_BWD(2, true); else SCL_DENSE_BWD(2, false);
  }
#undef SCL_DENSE_BWD
  int e = scl_launch_status();
  if (e || S == 1) return e;
  return launch_reduce(out, ld_out, slab, S, nullptr, 0, M, K, gx, ld_gx, st);
}

extern "C" int scl_dense_wgrad(const float* x, int64_t ld_x, const float* gy, int64_t ld_gy,
                               const float* y, int64_t ld_y, int M, int K, int N, float* gw,
                               int64_t ld_gw, float* gb, void* stream) {
  if (!x || !gy || !gw) return SCL_E_NULL;
  if (!valid_shape(M, K, N) || ld_x < K || ld_gy < N || ld_gw < N || (y && ld_y < N))
    return SCL_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = al16(gy) && al16(gw) && ld4(ld_gy) && ld4(ld_gw) && (!y || (al16(y) && ld4(ld_y)));
  const int nkt = cdiv(K, 32), ncg = cdiv(N, 128);
  const int blocks = cdiv((int64_t)nkt * ncg, kThreads / 64);
  if (vec)
    SCL_LAUNCH("dense_wgrad_kernel", dense_wgrad_kernel<true>, dim3(blocks), dim3(kThreads), 0, st, x,
               ld_x, gy, ld_gy, y, ld_y, M, K, N, gw, ld_gw, gb, nkt, ncg);
  else
    SCL_LAUNCH("dense_wgrad_kernel", dense_wgrad_kernel<false>, dim3(blocks), dim3(kThreads), 0, st,
               x, ld_x, gy, ld_gy, y, ld_y, M, K, N, gw, ld_gw, gb, nkt, ncg);
  return scl_launch_status();
}
