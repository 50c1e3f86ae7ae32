// The reference's weighted residual-determinant losses on gfx950: wrd_loss, prodwrd_loss and
// sumwrd_loss (model/losses.py:373-437; wrd is the trainer's default --loss, train/train.py:1252).
//
// Per tuple the reference takes the singular values of the weighted residual rows
// diag(w) (x_j - a), j = 1..S, on a positive and a negative side, and the loss is
// mean_t(prod_pos - prod_neg) + margin with prod = the product of the `dimensions` largest.
// With Z = [a; x_1 .. x_S] and G = Z Z^T ("Spectral losses") everything after the
// Gram is (S+1)^2 work: the residual Gram R_ij = G_ij - G_i0 - G_0j + G_00, the similarities
// sim_j = G_0j that prodwrd / sumwrd feed into the row weights, the eigenvalues of W R W (the
// squared singular values) and a coefficient matrix C with d loss / d Z = C Z, which
// scl_gram_loss_bwd multiplies out.
//
//   1. spectral_gram_kernel    one pass over z.  Workgroup = (E slice of 384 columns, tuple): the
//                              slice is staged in LDS as float32, a thread owns a 4 x 4 block of
//                              the upper block triangle and one of 8 column phases, multiplies
//                              and accumulates in FLOAT64 (a float32 Gram leaves the gradient 1e-4
//                              off the float64 SVD), the phases are summed in order through LDS.
//                              One partial per slice: no atomics.
//   2. spectral_solve_kernel   workgroup = (side, tuple).  Sums the slice partials in slice order,
//                              builds W R W and runs a cyclic Jacobi eigen-solve on it in LDS in
//                              float64: round-robin ordering, n/2 disjoint rotations per step,
//                              thread (ka, kb) updates the 2 x 2 block of pair ka's rows and pair
//                              kb's columns (J_ka^T . J_kb), the eigenvectors ride along.  A pair is
//                              rotated while a_pq^2 > 2^-100 a_pp a_qq — a relative test: the
//                              negatives' rows sit at e^-40 on the positive side — and the solve
//                              ends with the first sweep that rotates nothing, or after kMaxSweeps.
//                              Then the k largest, their product and this side's coefficient block.
//   3. spectral_finish_kernel  coef = (C_pos - C_neg) / T in float32, loss = sum over tuples in
//                              tuple order / T + margin.
// Every sum has a fixed order: two calls on the same input return the same bits.
//
// The eigenvalue and residual losses (residual_det, residual_trace, swrd, ntuplet_evmm,
// ntuplet_trace, neg_eigenvalue; model/losses.py:310-370, 613-624) take the same Gram pass and the
// same Jacobi solve on a side-sized matrix: eigen_solve_kernel and eigen_finish_kernel below.
#include "scl_common.h"

namespace {

constexpr int kMaxS = 32;                   // others per tuple (positives + negatives)
constexpr int kMaxRows = kMaxS + 1;         // rows of Z
constexpr int kBlk = 4;                     // Gram register block
constexpr int kNb = (kMaxRows + kBlk - 1) / kBlk;            // 9 block rows
constexpr int kUpper = kNb * (kNb + 1) / 2;                  // 45 blocks with bi <= bj
constexpr int kPartial = kUpper * kBlk * kBlk;               // 720 doubles per (tuple, slice)
constexpr int kPhases = 8;                  // column phases per block
constexpr int kGramThreads = kUpper * kPhases;               // 360
constexpr int kSlice = 384;                 // columns of E per workgroup
constexpr int kLdz = kSlice + 2;            // row stride (floats): 2 mod 64 spreads the block rows
constexpr int kStageRows = kNb * kBlk;      // 36
constexpr int kSolveThreads = 256;
constexpr int kLd = kMaxRows;               // odd row stride (doubles) of the LDS matrices
constexpr int kCoef = kMaxRows * kMaxRows;  // doubles per (tuple, side) coefficient block
constexpr int kMaxSweeps = 30;
constexpr double kRotTol = 8.8817841970012523e-16;           // 2^-50

static_assert(kPhases * kPartial * sizeof(double) <= (size_t)kStageRows * kLdz * sizeof(float),
              "the phase sums reuse the staging buffer");

// first upper-triangle block of block row bi
__host__ __device__ constexpr int upper_offset(int bi) { return bi * kNb - bi * (bi - 1) / 2; }

__global__ __launch_bounds__(kGramThreads) void spectral_gram_kernel(
    const float* __restrict__ z, int S1, int E, int nslice, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float stage[kStageRows * kLdz];
  const int tid = threadIdx.x, slice = blockIdx.x, t = blockIdx.y;
  const int e0 = slice * kSlice;
  const int ncols = min(kSlice, E - e0);
  const float* zt = z + (int64_t)t * S1 * E;

  for (int i = tid; i < kStageRows * kSlice; i += kGramThreads) {
    const int r = i / kSlice, c = i - r * kSlice;
    stage[r * kLdz + c] = (r < S1 && c < ncols) ? zt[(int64_t)r * E + e0 + c] : 0.f;
  }
  __syncthreads();

  const int b = tid / kPhases, q = tid - b * kPhases;
  int bi = 0, rem = b;
  while (rem >= kNb - bi) {
    rem -= kNb - bi;
    ++bi;
  }
  const int bj = bi + rem;
  double acc[kBlk][kBlk];
#pragma unroll
  for (int r = 0; r < kBlk; ++r)
#pragma unroll
    for (int c = 0; c < kBlk; ++c) acc[r][c] = 0.0;
  if (bi * kBlk < S1 && bj * kBlk < S1) {
    const float* ra = stage + bi * kBlk * kLdz;
    const float* rb = stage + bj * kBlk * kLdz;
    for (int c = q; c < ncols; c += kPhases) {
      double a[kBlk], bb[kBlk];
#pragma unroll
      for (int r = 0; r < kBlk; ++r) {
        a[r] = (double)ra[r * kLdz + c];
        bb[r] = (double)rb[r * kLdz + c];
      }
#pragma unroll
      for (int r = 0; r < kBlk; ++r)
#pragma unroll
        for (int cc = 0; cc < kBlk; ++cc) acc[r][cc] = fma(a[r], bb[cc], acc[r][cc]);
    }
  }
  __syncthreads();                              // the staged rows are dead: reuse them
  double* red = reinterpret_cast<double*>(stage);
#pragma unroll
  for (int r = 0; r < kBlk; ++r)
#pragma unroll
    for (int c = 0; c < kBlk; ++c) red[q * kPartial + b * (kBlk * kBlk) + r * kBlk + c] = acc[r][c];
  __syncthreads();
  double* dst = part + ((int64_t)t * nslice + slice) * kPartial;
  for (int i = tid; i < kPartial; i += kGramThreads) {
    double v = red[i];
    for (int p = 1; p < kPhases; ++p) v += red[p * kPartial + i];
    dst[i] = v;
  }
}

// G[i][j] of the block-triangular partial layout (any i, j)
__device__ __forceinline__ int partial_index(int i, int j) {
  if (i > j) {
    const int s = i;
    i = j;
    j = s;
  }
  const int bi = i / kBlk, bj = j / kBlk;
  return (upper_offset(bi) + bj - bi) * (kBlk * kBlk) + (i - bi * kBlk) * kBlk + (j - bj * kBlk);
}

// partner lists of the round-robin tournament on n2 (even) players: in step s the pairs are
// (n2 - 1, s) and ((s + k) mod m, (s - k) mod m), k = 1 .. n2/2 - 1, m = n2 - 1
__device__ __forceinline__ void tournament_pair(int n2, int step, int k, int* p, int* q) {
  const int m = n2 - 1;
  int a, b;
  if (k == 0) {
    a = m;
    b = step;
  } else {
    a = (step + k) % m;
    b = (step - k + m) % m;
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}

// Gs = the Gram of tuple t, full symmetric: the slice partials summed in slice order
__device__ __forceinline__ void load_gram(const double* __restrict__ part, int t, int nslice, int S1,
                                          double* Gs, int tid) {
  const double* pt = part + (int64_t)t * nslice * kPartial;
  for (int i = tid; i < S1 * S1; i += kSolveThreads) {
    const int r = i / S1, c = i - r * S1;
    if (r > c) continue;
    const double* src = pt + partial_index(r, c);
    double v = src[0];
#pragma unroll 8
    for (int s = 1; s < nslice; ++s) v += src[(int64_t)s * kPartial];
    Gs[r * kLd + c] = v;
    Gs[c * kLd + r] = v;
  }
  __syncthreads();
}

// Cyclic Jacobi on the symmetric n2 x n2 matrix A (n2 even, row stride kLd) with V = I on entry:
// on return A's diagonal holds the eigenvalues and V's columns the eigenvectors.  At most
// kMaxSweeps sweeps; every thread of the workgroup calls it.
__device__ __forceinline__ void jacobi_solve(double* A, double* V, int n2, int tid) {
  __shared__ double rot_c[kMaxS / 2], rot_s[kMaxS / 2];
  __shared__ int rot_p[kMaxS / 2], rot_q[kMaxS / 2];
  __shared__ int rotated;
  const int npairs = n2 / 2;
  if (tid == 0) rotated = 0;
  __syncthreads();
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    for (int step = 0; step < n2 - 1; ++step) {
      if (tid < npairs) {
        int p, q;
        tournament_pair(n2, step, tid, &p, &q);
        const double app = A[p * kLd + p], aqq = A[q * kLd + q], apq = A[p * kLd + q];
        double c = 1.0, s = 0.0;
        if (apq * apq > kRotTol * kRotTol * fabs(app * aqq)) {
          // t = sign(tau) / (|tau| + sqrt(1 + tau^2)), tau = (a_qq - a_pp) / (2 a_pq), with one
          // square root, one divide and one reciprocal square root
          const double d = aqq - app;
          const double tt = (d >= 0.0 ? 2.0 : -2.0) * apq / (fabs(d) + sqrt(d * d + 4.0 * apq * apq));
          c = rsqrt(1.0 + tt * tt);
          s = tt * c;
          if (s != 0.0) rotated = 1;
        }
        rot_c[tid] = c;
        rot_s[tid] = s;
        rot_p[tid] = p;
        rot_q[tid] = q;
      }
      __syncthreads();
      // A <- J^T A J by 2 x 2 blocks (rows of pair ka, columns of pair kb); J = [c s; -s c]
      for (int i = tid; i < npairs * npairs; i += kSolveThreads) {
        const int ka = i / npairs, kb = i - ka * npairs;
        const int pa = rot_p[ka], qa = rot_q[ka], pb = rot_p[kb], qb = rot_q[kb];
        const double ca = rot_c[ka], sa = rot_s[ka], cb = rot_c[kb], sb = rot_s[kb];
        const double a00 = A[pa * kLd + pb], a01 = A[pa * kLd + qb];
        const double a10 = A[qa * kLd + pb], a11 = A[qa * kLd + qb];
        const double r00 = ca * a00 - sa * a10, r01 = ca * a01 - sa * a11;   // J_a^T . block
        const double r10 = sa * a00 + ca * a10, r11 = sa * a01 + ca * a11;
        A[pa * kLd + pb] = cb * r00 - sb * r01;
        A[pa * kLd + qb] = sb * r00 + cb * r01;
        A[qa * kLd + pb] = cb * r10 - sb * r11;
        A[qa * kLd + qb] = sb * r10 + cb * r11;
      }
      // V <- V J
      for (int i = tid; i < n2 * npairs; i += kSolveThreads) {
        const int k = i / n2, r = i - k * n2;
        const int p = rot_p[k], q = rot_q[k];
        const double c = rot_c[k], s = rot_s[k];
        const double vp = V[r * kLd + p], vq = V[r * kLd + q];
        V[r * kLd + p] = c * vp - s * vq;
        V[r * kLd + q] = s * vp + c * vq;
      }
      __syncthreads();
    }
    const int any = rotated;                    // the same word for every thread
    __syncthreads();
    if (tid == 0) rotated = 0;
    __syncthreads();
    if (!any) break;
  }
}

// order[r] = the index of the r-th largest of lam[0 .. n) (ties: the lower index first)
__device__ __forceinline__ void rank_descending(const double* lam, int* order, int n, int tid) {
  if (tid < n) {
    const double li = lam[tid];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const double lj = lam[j];
      rank += (lj > li || (lj == li && j < tid)) ? 1 : 0;
    }
    order[rank] = tid;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kSolveThreads) void spectral_solve_kernel(
    int kind, const double* __restrict__ part, int nslice, const float* __restrict__ pos_w,
    const float* __restrict__ neg_w, int S, int T, int dimensions, float f_alpha_p, float f_alpha_n,
    float f_lamb, double* __restrict__ prods_out, double* __restrict__ side_coef) {
  __shared__ double Gs[kMaxRows * kLd];         // Gram of Z, full symmetric
  __shared__ double A[kMaxS * kLd];             // W R W, then M0
  __shared__ double V[kMaxS * kLd];             // eigenvectors in columns
  __shared__ double w[kMaxS], dw[kMaxS], lam[kMaxS], dcoef[kMaxS], qv[kMaxS], rsum[kMaxS];
  __shared__ int order[kMaxS];

  const int tid = threadIdx.x, side = blockIdx.x, t = blockIdx.y;
  const int S1 = S + 1;
  const int n2 = S + (S & 1);

  load_gram(part, t, nslice, S1, Gs, tid);

  // ---- row weights of this side ----
  if (tid < kMaxS) {
    double wj = 0.0, dwj = 0.0;
    if (tid < S) {
      const double w0 = (double)(side == 0 ? pos_w : neg_w)[(int64_t)t * S + tid];
      if (kind == 0) {
        wj = w0;
      } else {
        const double sim = Gs[tid + 1];
        const double slope = side == 0 ? (double)f_alpha_p : -(double)f_alpha_n;
        const double f = 1.0 / (1.0 + exp(slope * (sim - (double)f_lamb)));
        const double df = -f * (1.0 - f) * slope;
        if (kind == 1) {
          wj = w0 * f;
          dwj = w0 * df;
        } else {
          wj = w0 + f;
          dwj = df;
        }
      }
    }
    w[tid] = wj;
    dw[tid] = dwj;
  }
  __syncthreads();

  // ---- A = W R W (zero in the padding row of an odd S), V = I ----
  for (int i = tid; i < n2 * n2; i += kSolveThreads) {
    const int r = i / n2, c = i - r * n2;
    double a = 0.0;
    if (r < S && c < S) {
      const double res = Gs[(r + 1) * kLd + c + 1] - Gs[(r + 1) * kLd] - Gs[c + 1] + Gs[0];
      a = w[r] * res * w[c];
    }
    A[r * kLd + c] = a;
    V[r * kLd + c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();

  jacobi_solve(A, V, n2, tid);

  // ---- the k largest eigenvalues, their product, d prod / d s_i / s_i ----
  if (tid < kMaxS) {
    lam[tid] = tid < S ? A[tid * kLd + tid] : 0.0;
    order[tid] = 0;                             // (stays in range whatever the comparisons say)
  }
  __syncthreads();
  rank_descending(lam, order, S, tid);
  if (tid < S) {
    int rank = -1;
    for (int r = 0; r < dimensions; ++r)
      if (order[r] == tid) rank = r;
    double d = 0.0;
    if (rank >= 0) {
      double others = 1.0;                      // c_i: the other singular values, largest first
      for (int r = 0; r < dimensions; ++r)
        if (r != rank) others *= sqrt(fmax(lam[order[r]], 0.0));
      const double si = sqrt(fmax(lam[tid], 0.0));
      d = si > 0.0 ? others / si : 0.0;         // an exactly zero singular value: no term
    }
    dcoef[tid] = d;
  }
  if (tid == 0) {
    double prod = 1.0;
    for (int r = 0; r < dimensions; ++r) prod *= sqrt(fmax(lam[order[r]], 0.0));
    prods_out[(int64_t)t * 2 + side] = prod;
  }
  __syncthreads();

  // ---- M0 = U diag(d) U^T over A ----
  for (int i = tid; i < S * S; i += kSolveThreads) {
    const int r = i / S, c = i - r * S;
    double m = 0.0;
    for (int e = 0; e < S; ++e) m += dcoef[e] * V[r * kLd + e] * V[c * kLd + e];
    A[r * kLd + c] = m;
  }
  __syncthreads();
  // q_j = dw_j sum_l M0_jl w_l R_lj,  rsum_j = sum_l (W M0 W)_jl
  if (tid < S) {
    const int j = tid;
    double qs = 0.0, rs = 0.0;
    for (int l = 0; l < S; ++l) {
      const double m = A[j * kLd + l] * w[l];
      const double res = Gs[(l + 1) * kLd + j + 1] - Gs[(l + 1) * kLd] - Gs[j + 1] + Gs[0];
      qs += m * res;
      rs += m;
    }
    qv[j] = dw[j] * qs;
    rsum[j] = w[j] * rs;
  }
  __syncthreads();
  double* cs = side_coef + ((int64_t)t * 2 + side) * kCoef;
  for (int i = tid; i < S1 * S1; i += kSolveThreads) {
    const int r = i / S1, c = i - r * S1;
    double v;
    if (r > 0 && c > 0) {
      v = w[r - 1] * A[(r - 1) * kLd + c - 1] * w[c - 1];
    } else if (r > 0) {
      v = qv[r - 1] - rsum[r - 1];
    } else if (c > 0) {
      v = qv[c - 1] - rsum[c - 1];              // M0 is symmetric: column sums = row sums
    } else {
      v = 0.0;
      for (int j = 0; j < S; ++j) v += rsum[j];
    }
    cs[i] = v;
  }
}

__global__ __launch_bounds__(256) void spectral_finish_kernel(
    const double* __restrict__ prods, const double* __restrict__ side_coef, int T, int S1,
    float margin, float* __restrict__ loss_out, float* __restrict__ coef_out) {
  const int t = blockIdx.x;
  if (coef_out) {
    const double* cp = side_coef + (int64_t)t * 2 * kCoef;
    const double* cn = cp + kCoef;
    float* dst = coef_out + (int64_t)t * S1 * S1;
    for (int i = threadIdx.x; i < S1 * S1; i += blockDim.x) dst[i] = (float)((cp[i] - cn[i]) / (double)T);
  }
  if (t == 0 && threadIdx.x == 0) {
    double sum = 0.0;
    for (int i = 0; i < T; ++i) sum += prods[2 * i] - prods[2 * i + 1];
    *loss_out = (float)(sum / (double)T + (double)margin);
  }
}

// ---------------------------------------------------------------------------------------------
// The eigenvalue and residual losses on the same Gram (model/losses.py:310-370, 613-624).  What
// differs from wrd is the matrix of a side and the function of its eigenvalues:
//   residual kinds   W R W over the side's own rows (P x P or N x N), w = 1 except for swrd
//   Gram kinds       the plain Gram block of the rows {0} u side ((P + 1)^2 or (N + 1)^2 <= 32^2)
// and a diagonal d with the side's coefficient block M = U diag(d) U^T:
//   det / swrd   term = prod of the k largest s_i,  d_i = (prod_{l != i} s_l) / s_i in the top k
//   trace        term = sum of the k largest s_i,   d_i = 1 / s_i in the top k
//   l_min/l_max  term = that eigenvalue,            d_i = 2 at its index
//   tr(Gram)     term = sum_i G_ii, no solve,       d_i = 2 everywhere (M = 2 I)
// (s_i = sqrt(lambda_i); an exactly zero s_i gives no term, as in spectral_solve_kernel).
// Workgroup = (side, tuple); neg_eigenvalue launches the negative side only (side0 = 1).
__global__ __launch_bounds__(kSolveThreads) void eigen_solve_kernel(
    int kind, const double* __restrict__ part, int nslice, const float* __restrict__ pos_w,
    const float* __restrict__ neg_w, int P, int N, int dimensions, int side0,
    double* __restrict__ terms_out, double* __restrict__ side_coef) {
  __shared__ double Gs[kMaxRows * kLd];         // Gram of Z, full symmetric
  __shared__ double A[kMaxS * kLd];             // the side's matrix, then M
  __shared__ double V[kMaxS * kLd];             // eigenvectors in columns
  __shared__ double w[kMaxS], lam[kMaxS], dcoef[kMaxS], rsum[kMaxS];
  __shared__ int order[kMaxS];

  const int tid = threadIdx.x, side = blockIdx.x + side0, t = blockIdx.y;
  const int S1 = P + N + 1;
  const bool residual = kind <= SCL_EIGEN_SWRD;
  const int m = side == 0 ? P : N;              // this side's rows of Z are off + 1 .. off + m
  const int off = side == 0 ? 0 : P;
  const int n = residual ? m : m + 1;           // the Gram kinds take the anchor as row 0
  const int n2 = n + (n & 1);

  load_gram(part, t, nslice, S1, Gs, tid);

  if (tid < kMaxS) {
    double wj = 0.0;
    if (tid < m)
      wj = kind == SCL_EIGEN_SWRD ? (double)(side == 0 ? pos_w : neg_w)[(int64_t)t * m + tid] : 1.0;
    w[tid] = wj;
  }
  __syncthreads();

  // ---- the side's matrix (zero in the padding row of an odd n), V = I ----
  for (int i = tid; i < n2 * n2; i += kSolveThreads) {
    const int r = i / n2, c = i - r * n2;
    double a = 0.0;
    if (r < n && c < n) {
      if (residual) {
        const int gi = off + 1 + r, gj = off + 1 + c;
        const double res = Gs[gi * kLd + gj] - Gs[gi * kLd] - Gs[gj] + Gs[0];
        a = w[r] * res * w[c];
      } else {
        a = Gs[(r == 0 ? 0 : off + r) * kLd + (c == 0 ? 0 : off + c)];
      }
    }
    A[r * kLd + c] = a;
    V[r * kLd + c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();

  if (kind != SCL_EIGEN_NTUPLET_TRACE) jacobi_solve(A, V, n2, tid);   // the trace: diagonal only

  if (tid < kMaxS) {
    lam[tid] = tid < n ? A[tid * kLd + tid] : 0.0;
    order[tid] = 0;                             // (stays in range whatever the comparisons say)
  }
  __syncthreads();
  rank_descending(lam, order, n, tid);

  // ---- the term and d ----
  const bool det = kind == SCL_EIGEN_RESIDUAL_DET || kind == SCL_EIGEN_SWRD;
  // index of the one eigenvalue of evmm / neg_eigenvalue: l_min, but l_max on evmm's negative side
  const int pick = order[(kind == SCL_EIGEN_NTUPLET_EVMM && side == 1) ? 0 : n - 1];
  if (tid < n) {
    double d = 0.0;
    if (residual) {
      int rank = -1;
      for (int r = 0; r < dimensions; ++r)
        if (order[r] == tid) rank = r;
      if (rank >= 0) {
        double others = 1.0;                    // det: the other singular values, largest first
        if (det)
          for (int r = 0; r < dimensions; ++r)
            if (r != rank) others *= sqrt(fmax(lam[order[r]], 0.0));
        const double si = sqrt(fmax(lam[tid], 0.0));
        d = si > 0.0 ? others / si : 0.0;       // an exactly zero singular value: no term
      }
    } else if (kind == SCL_EIGEN_NTUPLET_TRACE || tid == pick) {
      d = 2.0;
    }
    dcoef[tid] = d;
  }
  if (tid == 0) {
    double term;
    if (det) {
      term = 1.0;
      for (int r = 0; r < dimensions; ++r) term *= sqrt(fmax(lam[order[r]], 0.0));
    } else if (kind == SCL_EIGEN_RESIDUAL_TRACE) {
      term = 0.0;
      for (int r = 0; r < dimensions; ++r) term += sqrt(fmax(lam[order[r]], 0.0));
    } else if (kind == SCL_EIGEN_NTUPLET_TRACE) {
      term = 0.0;
      for (int j = 0; j < n; ++j) term += lam[j];
    } else {
      term = lam[pick];
    }
    terms_out[(int64_t)t * 2 + side] = term;
    if (kind == SCL_EIGEN_NEG_EIGENVALUE) terms_out[(int64_t)t * 2] = 0.0;
  }
  __syncthreads();

  // ---- M = U diag(d) U^T over A ----
  for (int i = tid; i < n * n; i += kSolveThreads) {
    const int r = i / n, c = i - r * n;
    double v = 0.0;
    for (int e = 0; e < n; ++e) v += dcoef[e] * V[r * kLd + e] * V[c * kLd + e];
    A[r * kLd + c] = v;
  }
  __syncthreads();
  if (residual && tid < m) {                    // rsum_j = sum_l (W M W)_jl; M is symmetric
    double rs = 0.0;
    for (int l = 0; l < m; ++l) rs += A[tid * kLd + l] * w[l];
    rsum[tid] = w[tid] * rs;
  }
  __syncthreads();

  // ---- scatter into this side's (S+1)^2 block of C: residual kinds C[I,I] += W M W,
  // C[I,0] -= rowsum, C[0,I] -= colsum, C[0,0] += sum; Gram kinds C[J,J] += M, J = {0} u I ----
  double* cs = side_coef + ((int64_t)t * 2 + side) * kCoef;
  for (int i = tid; i < S1 * S1; i += kSolveThreads) {
    const int r = i / S1, c = i - r * S1;
    const int lr = r - 1 - off, lc = c - 1 - off;          // side-local row numbers of r, c > 0
    const bool in_r = r > 0 && lr >= 0 && lr < m, in_c = c > 0 && lc >= 0 && lc < m;
    double v = 0.0;
    if (residual) {
      if (in_r && in_c) {
        v = w[lr] * A[lr * kLd + lc] * w[lc];
      } else if (in_r && c == 0) {
        v = -rsum[lr];
      } else if (r == 0 && in_c) {
        v = -rsum[lc];
      } else if (r == 0 && c == 0) {
        for (int j = 0; j < m; ++j) v += rsum[j];
      }
    } else if ((r == 0 || in_r) && (c == 0 || in_c)) {
      v = A[(r == 0 ? 0 : lr + 1) * kLd + (c == 0 ? 0 : lc + 1)];
    }
    cs[i] = v;
  }
}

// float64, tuple order.  The hinge of ntuplet_evmm / ntuplet_trace is active at an argument >= 0:
// TensorFlow's maximum(x, y) sends the gradient to x where x >= y, so a tie at exactly 0 still
// passes the gradient (and adds 0 to the loss).
__global__ __launch_bounds__(256) void eigen_finish_kernel(
    int kind, const double* __restrict__ terms, const double* __restrict__ side_coef, int T, int S1,
    float margin, float* __restrict__ loss_out, float* __restrict__ coef_out) {
  const int t = blockIdx.x;
  const bool hinge = kind == SCL_EIGEN_NTUPLET_EVMM || kind == SCL_EIGEN_NTUPLET_TRACE;
  if (coef_out) {
    const double* cp = side_coef + (int64_t)t * 2 * kCoef;
    const double* cn = cp + kCoef;
    float* dst = coef_out + (int64_t)t * S1 * S1;
    const bool active = !hinge || (double)margin + terms[2 * t] - terms[2 * t + 1] >= 0.0;
    for (int i = threadIdx.x; i < S1 * S1; i += blockDim.x) {
      double v = 0.0;
      if (kind == SCL_EIGEN_NEG_EIGENVALUE) {
        v = -cn[i] / (double)T;
      } else if (active) {
        v = (cp[i] - cn[i]) / (double)T;
      }
      dst[i] = (float)v;
    }
  }
  if (t == 0 && threadIdx.x == 0) {
    double sum = 0.0;
    for (int i = 0; i < T; ++i) {
      const double diff = terms[2 * i] - terms[2 * i + 1];
      sum += hinge ? fmax((double)margin + diff, 0.0) : diff;
    }
    double loss = sum / (double)T;
    if (kind <= SCL_EIGEN_SWRD) loss += (double)margin;
    *loss_out = (float)loss;
  }
}

bool valid_shape(int T, int S, int E) { return T >= 1 && T <= 65535 && S >= 1 && S <= kMaxS && E >= 1; }
int slices(int E) { return (E + kSlice - 1) / kSlice; }
size_t partial_bytes(int T, int E) { return scl_round256((size_t)T * slices(E) * kPartial * sizeof(double)); }

}  // namespace

extern "C" size_t scl_spectral_loss_workspace_bytes(int T, int S, int E) {
  if (!valid_shape(T, S, E)) return 0;
  return partial_bytes(T, E) + scl_round256((size_t)T * 2 * kCoef * sizeof(double));
}

extern "C" int scl_spectral_loss_fwd(int kind, const float* z, const float* pos_w,
                                     const float* neg_w, int T, int S, int E, float margin,
                                     int dimensions, float f_alpha_p, float f_alpha_n, float f_lamb,
                                     float* loss_out, double* prods_out, float* coef_out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!z || !pos_w || !neg_w || !loss_out || !prods_out || !workspace) return SCL_E_NULL;
  if (!valid_shape(T, S, E) || dimensions < 1 || dimensions > S) return SCL_E_SHAPE;
  if (kind < 0 || kind > 2) return SCL_E_KIND;
  if (!scl_aligned256(workspace) || workspace_bytes < scl_spectral_loss_workspace_bytes(T, S, E))
    return SCL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nslice = slices(E);
  double* part = static_cast<double*>(workspace);
  double* side_coef = reinterpret_cast<double*>(static_cast<char*>(workspace) + partial_bytes(T, E));
  SCL_LAUNCH("spectral_gram_kernel", spectral_gram_kernel, dim3(nslice, T), dim3(kGramThreads), 0, st,
             z, S + 1, E, nslice, part);
  SCL_LAUNCH("spectral_solve_kernel", spectral_solve_kernel, dim3(2, T), dim3(kSolveThreads), 0, st,
             kind, (const double*)part, nslice, pos_w, neg_w, S, T, dimensions, f_alpha_p, f_alpha_n,
             f_lamb, prods_out, side_coef);
  SCL_LAUNCH("spectral_finish_kernel", spectral_finish_kernel, dim3(T), dim3(256), 0, st,
             (const double*)prods_out, (const double*)side_coef, T, S + 1, margin, loss_out, coef_out);
  return scl_launch_status();
}

extern "C" size_t scl_eigen_loss_workspace_bytes(int T, int P, int N, int E) {
  if (P < 0 || N < 1 || !valid_shape(T, (P > 0 ? P : 1) + N, E)) return 0;
  return scl_spectral_loss_workspace_bytes(T, (P > 0 ? P : 1) + N, E);
}

extern "C" int scl_eigen_loss_fwd(int kind, const float* z, const float* pos_w, const float* neg_w,
                                  int T, int P, int N, int E, float margin, int dimensions,
                                  float* loss_out, double* terms_out, float* coef_out,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!z || !loss_out || !terms_out || !workspace) return SCL_E_NULL;
  if (kind < SCL_EIGEN_RESIDUAL_DET || kind > SCL_EIGEN_NEG_EIGENVALUE) return SCL_E_KIND;
  if (kind == SCL_EIGEN_SWRD && (!pos_w || !neg_w)) return SCL_E_NULL;
  // neg_eigenvalue has no positive side: P = 0 is its shape alone, and N + 1 rows must fit
  const int min_p = kind == SCL_EIGEN_NEG_EIGENVALUE ? 0 : 1;
  if (P < min_p || N < 1 || P > kMaxS || N > kMaxS || !valid_shape(T, (P > 0 ? P : 1) + N, E))
    return SCL_E_SHAPE;
  // the residual kinds take the `dimensions` largest of a side's min(rows, E) singular values
  if (kind <= SCL_EIGEN_SWRD && (dimensions < 1 || dimensions > (P < N ? P : N))) return SCL_E_SHAPE;
  if (!scl_aligned256(workspace) || workspace_bytes < scl_eigen_loss_workspace_bytes(T, P, N, E))
    return SCL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nslice = slices(E);
  const int side0 = kind == SCL_EIGEN_NEG_EIGENVALUE ? 1 : 0;
  double* part = static_cast<double*>(workspace);
  double* side_coef = reinterpret_cast<double*>(static_cast<char*>(workspace) + partial_bytes(T, E));
  SCL_LAUNCH("spectral_gram_kernel", spectral_gram_kernel, dim3(nslice, T), dim3(kGramThreads), 0, st,
             z, P + N + 1, E, nslice, part);
  SCL_LAUNCH("eigen_solve_kernel", eigen_solve_kernel, dim3(2 - side0, T), dim3(kSolveThreads), 0, st,
             kind, (const double*)part, nslice, pos_w, neg_w, P, N, dimensions, side0, terms_out,
             side_coef);
  SCL_LAUNCH("eigen_finish_kernel", eigen_finish_kernel, dim3(T), dim3(256), 0, st, kind,
             (const double*)terms_out, (const double*)side_coef, T, P + N + 1, margin, loss_out,
             coef_out);
  return scl_launch_status();
}
