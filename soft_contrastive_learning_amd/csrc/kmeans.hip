// k-means on conv5_3 descriptors (model/vlad_init.py; include/scl_hip.h has the contract): the
// Lloyd step that seeds a NetVLAD head.  A Lloyd step is NetVLAD with a hard assignment — scores
// x . c, an argmax over 64 clusters, the per-cluster sum of x — so both halves run on the float32
// matrix instruction v_mfma_f32_32x32x2_f32, which is an exact fmaf chain: on integer-valued data
// every number below is exact, and tests/test_gpu_vlad_init.py asks for the bits.
//
// kmeans_assign_kernel, one workgroup of four waves per SCL_KMEANS_ROWS = 128 rows:
//   scores   wave w owns rows 32 w .. 32 w + 31 of the block and both 32-cluster tiles: two
//            accumulators, 256 steps of k = 2 each, d ascending.  The instruction takes A[i][k] from
//            lane (i = l & 31, k = l >> 5): the lower half of the wave feeds the even d, the upper
//            half the odd d.  x comes straight from global memory, one 16-byte load per two steps
//            (both halves load the same four floats and keep two).  The centres come from the
//            operand image a prologue kernel writes to the workspace — even and odd d in two planes,
//            so a lane's 16-byte load is four steps of ITS half — and stay in L2: 128 KB that every
//            workgroup reads once per 32 rows.  Why not LDS: the instruction issues once per 64
//            cycles per SIMD; between two of them a wave needs 3/4 of a 16-byte load per lane, far
//            below what the vector memory path delivers from L1/L2, so neither a 128 KB LDS image
//            (one workgroup per CU, a 128 KB fill in front of 128 rows of work) nor a split of d
//            over the waves (which would cut the one chain over d into four) buys time here.
//   argmax   register r of lane (j, half) is score[row acc_row(r, half)][cluster j (+32)]: a
//            butterfly over the 32 lanes of the half merges (best, k, second) by the order
//            (score descending, k ascending); NaN and -inf never enter.
//   sums     part_sum[g] = onehot^T X: wave w owns d in [128 w, 128 w + 128) as four tiles times the
//            two cluster tiles, eight accumulators, 64 steps over the block's rows in ascending
//            order.  Column j of tile t is d = 128 w + 4 j + t, so B is one 16-byte load per lane and
//            step, coalesced, and a register of the four tiles is one 16-byte store.  Rows without a
//            label enter as zeros (0 x NaN would poison every cluster).
//   counts and inertia: from the labels in LDS, in row order, by single lanes.
// kmeans_update_kernel: a thread per (k, d) adds the G partials in float64, g ascending.
// No atomics; G = ceil(N / 128) whatever the device.
#include "scl_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = SCL_KMEANS_ROWS;
constexpr int kD = SCL_VLAD_D;
constexpr int kK = SCL_VLAD_K;
constexpr int kHalfD = kD / 2;
constexpr int kNoCluster = 0x7fffffff;

static_assert(kRows == 32 * (kThreads / SCL_WAVE), "a 32-row tile per wave");
static_assert(kD == 128 * (kThreads / SCL_WAVE), "128 columns of the sums per wave");
static_assert(kK == 64, "two 32-cluster tiles");

struct KmWorkspace {
  float* image;      // [2 planes][64 clusters][256]: plane h, entry i is centre coordinate 2 i + h
  float* off;        // [64], +inf from K on
  size_t bytes;
};
KmWorkspace km_carve(void* base) {
  Carver c(base);
  KmWorkspace w;
  w.image = c.take((size_t)2 * kK * kHalfD);
  w.off = c.take(kK);
  w.bytes = c.off;
  return w;
}

__global__ __launch_bounds__(kThreads) void kmeans_image_kernel(const float* __restrict__ centres,
                                                                const float* __restrict__ offsets, int K,
                                                                float* __restrict__ image,
                                                                float* __restrict__ off) {
  const int e = blockIdx.x * kThreads + threadIdx.x;       // (plane, cluster, i)
  if (e < 2 * kK * kHalfD) {
    const int i = e % kHalfD, c = (e / kHalfD) % kK, h = e / (kHalfD * kK);
    image[e] = c < K ? centres[(size_t)c * kD + 2 * i + h] : 0.f;
  }
  if (e < kK) off[e] = e < K ? offsets[e] : __builtin_inff();
}

// the first two entries of a set of scores in the order (score descending, k ascending); an empty
// slot is (-inf, kNoCluster), which comes after every score that takes part
struct Top2 {
  float best;
  int k;
  float second;
};
__device__ __forceinline__ Top2 top2_of(float v, int k) {
  const bool in = v > -__builtin_inff();                   // false for NaN and for -inf
  return Top2{in ? v : -__builtin_inff(), in ? k : kNoCluster, -__builtin_inff()};
}
__device__ __forceinline__ Top2 top2_merge(Top2 a, Top2 o) {
  const bool o_first = o.best > a.best || (o.best == a.best && o.k < a.k);
  Top2 r;
  r.best = o_first ? o.best : a.best;
  r.k = o_first ? o.k : a.k;
  r.second = o_first ? fmaxf(a.best, o.second) : fmaxf(a.second, o.best);
  return r;
}

template <bool kSums>
__global__ __launch_bounds__(kThreads) void kmeans_assign_kernel(
    const float* __restrict__ x, int N, const float* __restrict__ image, const float* __restrict__ off,
    int K, int* __restrict__ label, float* __restrict__ best, float* __restrict__ second,
    float* __restrict__ part_sum, int* __restrict__ part_cnt, double* __restrict__ part_inertia) {
  __shared__ int s_label[kRows];
  __shared__ float s_best[kRows];
  __shared__ double s_sq[kRows];
  const int tid = threadIdx.x, wave = tid / SCL_WAVE, lane = tid & (SCL_WAVE - 1);
  const int j = lane & 31, half = lane >> 5;
  const long long block_row = (long long)blockIdx.x * kRows;

  // ---- scores -----------------------------------------------------------------------------------
  {
    long long row = block_row + wave * 32 + j;
    if (row > N - 1) row = N - 1;                            // rows past the end read the last row
    const float* xr = x + row * kD;
    const float* c0 = image + ((size_t)half * kK + j) * kHalfD;
    const float* c1 = c0 + (size_t)32 * kHalfD;
    f32x16 acc0 = zero16(), acc1 = zero16();
    double sq = 0.0;
#pragma unroll 2
    for (int q = 0; q < kD / 8; ++q) {                       // 8 coordinates: 4 steps
      const f32x4 xa = Elem<float>::ld4(xr + 8 * q), xb = Elem<float>::ld4(xr + 8 * q + 4);
      const f32x4 b0 = Elem<float>::ld4(c0 + 4 * q), b1 = Elem<float>::ld4(c1 + 4 * q);
      const float a[4] = {half ? xa[1] : xa[0], half ? xa[3] : xa[2], half ? xb[1] : xb[0],
                          half ? xb[3] : xb[2]};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc0 = mfma32(a[s], b0[s], acc0);
        acc1 = mfma32(a[s], b1[s], acc1);
        sq = fma((double)a[s], (double)a[s], sq);
      }
    }
    sq += __shfl_xor(sq, 32, SCL_WAVE);                      // even d + odd d
    if (half == 0) s_sq[wave * 32 + j] = sq;

    // ---- argmax -----------------------------------------------------------------------------------
    const float off0 = off[j], off1 = off[j + 32];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      Top2 t = top2_merge(top2_of(acc0[r] - off0, j), top2_of(acc1[r] - off1, j + 32));
#pragma unroll
      for (int m = 1; m < 32; m <<= 1) {
        Top2 o;
        o.best = __shfl_xor(t.best, m, SCL_WAVE);
        o.k = __shfl_xor(t.k, m, SCL_WAVE);
        o.second = __shfl_xor(t.second, m, SCL_WAVE);
        t = top2_merge(t, o);
      }
      if (j == 0) {
        const int local = wave * 32 + acc_row(r, half);
        const long long n = block_row + local;
        const bool live = n < N;
        const int lab = (live && t.k != kNoCluster) ? t.k : -1;
        s_label[local] = lab;
        s_best[local] = t.best;
        if (live) {
          label[n] = lab;
          best[n] = t.best;
          second[n] = t.second;
        }
      }
    }
  }
  if (!kSums) return;
  __syncthreads();

  // ---- counts and inertia ---------------------------------------------------------------------------
  if (tid < K) {
    int cnt = 0;
    for (int n = 0; n < kRows; ++n) cnt += s_label[n] == tid;
    part_cnt[(size_t)blockIdx.x * K + tid] = cnt;
  }
  if (tid == kThreads - 1) {
    double sum = 0.0;
    for (int n = 0; n < kRows; ++n)
      if (s_label[n] >= 0) sum += s_sq[n] - 2.0 * (double)s_best[n];
    part_inertia[blockIdx.x] = sum;
  }

  // ---- sums: onehot^T X ---------------------------------------------------------------------------
  const int d0 = wave * 128 + 4 * j;
  f32x16 acc[2][4];
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[kt][t] = zero16();
#pragma unroll 2
  for (int s = 0; s < kRows / 2; ++s) {
    const int local = 2 * s + half;
    long long n = block_row + local;
    if (n > N - 1) n = N - 1;
    const int lab = s_label[local];
    f32x4 xv = Elem<float>::ld4(x + n * kD + d0);
    if (lab < 0) xv = f32x4{0.f, 0.f, 0.f, 0.f};
    const float one0 = lab == j ? 1.f : 0.f, one1 = lab == j + 32 ? 1.f : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc[0][t] = mfma32(one0, xv[t], acc[0][t]);
      acc[1][t] = mfma32(one1, xv[t], acc[1][t]);
    }
  }
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = 32 * kt + acc_row(r, half);
      if (k < K)
        *reinterpret_cast<f32x4*>(part_sum + ((size_t)blockIdx.x * K + k) * kD + d0) =
            f32x4{acc[kt][0][r], acc[kt][1][r], acc[kt][2][r], acc[kt][3][r]};
    }
}

// grid (kD / kThreads, K): a thread per coordinate of a centre
__global__ __launch_bounds__(kThreads) void kmeans_update_kernel(
    const float* __restrict__ part_sum, const int* __restrict__ part_cnt,
    const double* __restrict__ part_inertia, int G, int K, const float* __restrict__ old_centres,
    float* __restrict__ new_centres, int* __restrict__ counts, double* __restrict__ inertia) {
  const int k = blockIdx.y, d = blockIdx.x * kThreads + threadIdx.x;
  long long cnt = 0;
  double sum = 0.0;
  const float* p = part_sum + (size_t)k * kD + d;
  const size_t step = (size_t)K * kD;
#pragma unroll 8
  for (int g = 0; g < G; ++g) {
    cnt += part_cnt[(size_t)g * K + k];
    sum += (double)p[g * step];
  }
  const size_t at = (size_t)k * kD + d;
  new_centres[at] = cnt > 0 ? (float)(sum / (double)cnt) : old_centres[at];
  if (d == 0) counts[k] = (int)cnt;
  if (d == 1 && k == 0) {
    double total = 0.0;
    for (int g = 0; g < G; ++g) total += part_inertia[g];
    inertia[0] = total;
  }
}

bool km_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }
bool km_shape(int N, int K) { return N >= 1 && N <= SCL_KMEANS_MAX_N && K >= 1 && K <= kK; }

}  // namespace

extern "C" size_t scl_kmeans_workspace_bytes(int N, int K) {
  if (!km_shape(N, K)) return 0;
  return km_carve(nullptr).bytes;
}

extern "C" int scl_kmeans_assign(const float* x, int N, const float* centres, const float* offsets, int K,
                                 int* label, float* best, float* second, float* part_sum, int* part_cnt,
                                 double* part_inertia, void* work, size_t work_bytes, void* stream) {
  if (!x || !centres || !offsets || !label || !best || !second || !work) return SCL_E_NULL;
  if (part_sum && (!part_cnt || !part_inertia)) return SCL_E_NULL;
  if (!km_shape(N, K)) return SCL_E_SHAPE;
  if (!km_aligned16(x) || !km_aligned16(centres) || !km_aligned16(part_sum)) return SCL_E_SHAPE;
  const KmWorkspace ws = km_carve(work);
  if (work_bytes < ws.bytes || !scl_aligned256(work)) return SCL_E_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  SCL_LAUNCH("kmeans_image_kernel", kmeans_image_kernel, dim3(2 * kK * kHalfD / kThreads), dim3(kThreads), 0,
             st, centres, offsets, K, ws.image, ws.off);
  const dim3 grid((unsigned)(((long long)N + kRows - 1) / kRows));
  if (part_sum)
    SCL_LAUNCH("kmeans_assign_kernel<sums>", kmeans_assign_kernel<true>, grid, dim3(kThreads), 0, st, x, N,
               ws.image, ws.off, K, label, best, second, part_sum, part_cnt, part_inertia);
  else
    SCL_LAUNCH("kmeans_assign_kernel<labels>", kmeans_assign_kernel<false>, grid, dim3(kThreads), 0, st, x, N,
               ws.image, ws.off, K, label, best, second, part_sum, part_cnt, part_inertia);
  return scl_launch_status();
}

extern "C" int scl_kmeans_update(const float* part_sum, const int* part_cnt, const double* part_inertia,
                                 int G, int K, const float* old_centres, float* new_centres, int* counts,
                                 double* inertia, void* stream) {
  if (!part_sum || !part_cnt || !part_inertia || !old_centres || !new_centres || !counts || !inertia)
    return SCL_E_NULL;
  if (G < 1 || G > SCL_KMEANS_MAX_N / kRows || K < 1 || K > kK) return SCL_E_SHAPE;
  if (!km_aligned16(part_sum) || !km_aligned16(old_centres) || !km_aligned16(new_centres) ||
      old_centres == new_centres)
    return SCL_E_SHAPE;
  SCL_LAUNCH("kmeans_update_kernel", kmeans_update_kernel, dim3(kD / kThreads, (unsigned)K), dim3(kThreads),
             0, (hipStream_t)stream, part_sum, part_cnt, part_inertia, G, K, old_centres, new_centres,
             counts, inertia);
  return scl_launch_status();
}
