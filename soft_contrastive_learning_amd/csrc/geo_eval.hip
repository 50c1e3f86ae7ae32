// Geographic ground truth and hit distances (evaluation/geo.py; include/scl_hip.h has the contract):
// what evaluation/top-n.py:110-113 reads out of its [Q, R] table of position distances, computed
// from the positions themselves.
//
//   d2(q, j) = dx*dx + dy*dy,  dx = x_j - qx,  dy = y_j - qy      float64, every operation rounded
//                                                                  on its own (geo_d2_key)
//
// scl_geo_nearest wants the lexicographically smallest (d2, j) per query.  d2 is never negative, so
// its BIT PATTERN, read as an unsigned 64-bit integer, orders like the value: +0 < every finite
// value < +inf (0x7ff0..0) < every NaN (a NaN whose sign is set lies above them all).  The kernels
// keep (key, j) pairs with the empty pair (kNoKey, -1): kNoKey is the smallest NaN pattern, so +inf
// beats "nothing yet", no NaN ever does, and one integer compare per pair is the whole rule.  j is
// compared as an unsigned number, so -1 loses every tie.
//
// Q r pair evaluations on 16 bytes per reference: arithmetic, not memory.  Two routes, both
// grid = (query blocks, splits of the reference axis), both write one (key, j) per (query, split)
// to the workspace; geo_finish_kernel (a wave per query) merges the splits of a query by the same rule:
//   * geo_nearest_queries_kernel (Q > SCL_GEO_SMALL_Q): one query per lane, its position and its
//     running pair in registers.  The workgroup stages SCL_GEO_SLAB references in LDS, one 16-byte
//     load per lane, and every lane then reads the SAME slab entry per step: one ds_read_b128 whose
//     64 addresses are equal is a broadcast, no bank conflict.  j ascends, so a strict `<` keeps
//     the lower row of a tie.
//   * geo_nearest_refs_kernel (Q <= SCL_GEO_SMALL_Q): a workgroup per (query, split), the lanes
//     over the references (16-byte loads, a wave reads 1 KiB contiguous); each lane's j ascends; the
//     lanes of a wave merge by a butterfly of __shfl_xor, the waves through LDS, every step by
//     (key, j).
// No atomics and no order that depends on scheduling: the minimum of a set of distinct pairs does
// not depend on how the set is cut.
#include "scl_common.h"

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kSlab = SCL_GEO_SLAB;
constexpr u64 kNoKey = 0x7ff0000000000001ull;     // above +inf, at or below every NaN

static_assert(SCL_GEO_BLOCK_QUERIES == kThreads, "one query per lane");
static_assert(kSlab <= kThreads, "a slab is staged with one load per lane");

__device__ __forceinline__ double geo_d2(f64x2 r, f64x2 p) {
#pragma clang fp contract(off)
  const double dx = r.x - p.x, dy = r.y - p.y;
  return dx * dx + dy * dy;
}
__device__ __forceinline__ u64 geo_d2_key(f64x2 r, f64x2 p) {
  return (u64)__double_as_longlong(geo_d2(r, p));
}
// (ka, ja) before (kb, jb)?
__device__ __forceinline__ bool geo_before(u64 ka, int ja, u64 kb, int jb) {
  return ka < kb || (ka == kb && (unsigned)ja < (unsigned)jb);
}

struct GeoPlan {
  int small;              // lanes over references
  int qblocks;
  int slabs_per_split;
  int splits;
};
GeoPlan geo_plan(int R, int Q) {
  GeoPlan p;
  p.small = Q <= SCL_GEO_SMALL_Q;
  p.qblocks = p.small ? Q : (int)(((long long)Q + SCL_GEO_BLOCK_QUERIES - 1) / SCL_GEO_BLOCK_QUERIES);
  const int slabs = (int)(((long long)R + kSlab - 1) / kSlab);
  const int want = p.qblocks >= SCL_GEO_TARGET_BLOCKS ? 1 : SCL_GEO_TARGET_BLOCKS / p.qblocks;
  p.slabs_per_split = (slabs + want - 1) / want;
  p.splits = (slabs + p.slabs_per_split - 1) / p.slabs_per_split;
  return p;
}
// Pairs the workspace holds: Q splits is at most Q slabs, and at most SCL_GEO_TARGET_BLOCKS
// SCL_GEO_BLOCK_QUERIES where there is more than one split (splits <= want <= TARGET_BLOCKS / qblocks,
// qblocks >= Q / BLOCK_QUERIES).  This bound, not the product itself, sizes the workspace: it grows
// with Q and with R, the product does not (a query more can halve the split count).
size_t geo_pairs(int R, int Q) {
  const size_t slabs = ((size_t)R + kSlab - 1) / kSlab;
  const size_t cap = (size_t)SCL_GEO_TARGET_BLOCKS * SCL_GEO_BLOCK_QUERIES;
  const size_t most = (size_t)Q > cap ? (size_t)Q : cap;
  return (size_t)Q * slabs < most ? (size_t)Q * slabs : most;
}
struct GeoWorkspace {
  u64* key;               // [Q][splits]
  int* row;               // [Q][splits]
  size_t bytes;
};
GeoWorkspace geo_carve(void* base, size_t pairs) {
  Carver c(base);
  GeoWorkspace w;
  w.key = c.take<u64>(pairs);
  w.row = c.take<int>(pairs);
  w.bytes = c.off;
  return w;
}

// the references [first, last) of a split
__device__ __forceinline__ void geo_split_range(int R, int slabs_per_split, int split, long long* first,
                                                long long* last) {
  const long long span = (long long)slabs_per_split * kSlab;
  *first = split * span;
  *last = *first + span < R ? *first + span : R;
}

__global__ __launch_bounds__(kThreads) void geo_nearest_queries_kernel(
    const f64x2* __restrict__ ref, int R, const f64x2* __restrict__ query, int Q, int slabs_per_split,
    int splits, u64* __restrict__ part_key, int* __restrict__ part_row) {
  __shared__ f64x2 slab[kSlab];
  const int tid = threadIdx.x, split = blockIdx.y;
  const long long q = (long long)blockIdx.x * kThreads + tid;
  const bool live = q < Q;
  const f64x2 p = live ? query[q] : f64x2{0.0, 0.0};
  long long first, last;
  geo_split_range(R, slabs_per_split, split, &first, &last);
  u64 best = kNoKey;
  int row = -1;
  for (long long base = first; base < last; base += kSlab) {
    const int count = last - base < kSlab ? (int)(last - base) : kSlab;
    __syncthreads();                                  // the slab before has been read by every wave
    if (tid < count) slab[tid] = ref[base + tid];
    __syncthreads();
    const int j0 = (int)base;
    if (count == kSlab) {
#pragma unroll 8
      for (int i = 0; i < kSlab; ++i) {
        const u64 k = geo_d2_key(slab[i], p);
        const bool take = k < best;
        best = take ? k : best;
        row = take ? j0 + i : row;
      }
    } else {
      for (int i = 0; i < count; ++i) {
        const u64 k = geo_d2_key(slab[i], p);
        const bool take = k < best;
        best = take ? k : best;
        row = take ? j0 + i : row;
      }
    }
  }
  if (live) {
    part_key[q * splits + split] = best;
    part_row[q * splits + split] = row;
  }
}

// the smallest (key, row) of the wave's 64 pairs, in every lane: a butterfly, every step by (key, row)
__device__ __forceinline__ void geo_wave_merge(u64& best, int& row) {
#pragma unroll
  for (int m = 1; m < SCL_WAVE; m <<= 1) {
    const unsigned lo = __shfl_xor((unsigned)best, m, SCL_WAVE);
    const unsigned hi = __shfl_xor((unsigned)(best >> 32), m, SCL_WAVE);
    const int orow = __shfl_xor(row, m, SCL_WAVE);
    const u64 okey = ((u64)hi << 32) | lo;
    if (geo_before(okey, orow, best, row)) {
      best = okey;
      row = orow;
    }
  }
}

__global__ __launch_bounds__(kThreads) void geo_nearest_refs_kernel(
    const f64x2* __restrict__ ref, int R, const f64x2* __restrict__ query, int slabs_per_split,
    int splits, u64* __restrict__ part_key, int* __restrict__ part_row) {
  __shared__ u64 wave_key[kThreads / SCL_WAVE];
  __shared__ int wave_row[kThreads / SCL_WAVE];
  const int tid = threadIdx.x, q = blockIdx.x, split = blockIdx.y;
  const f64x2 p = query[q];
  long long first, last;
  geo_split_range(R, slabs_per_split, split, &first, &last);
  u64 best = kNoKey;
  int row = -1;
  for (long long j = first + tid; j < last; j += kThreads) {
    const u64 k = geo_d2_key(ref[j], p);
    const bool take = k < best;                       // the lane's j ascends: the lower row stays
    best = take ? k : best;
    row = take ? (int)j : row;
  }
  geo_wave_merge(best, row);
  if ((tid & (SCL_WAVE - 1)) == 0) {
    wave_key[tid / SCL_WAVE] = best;
    wave_row[tid / SCL_WAVE] = row;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kThreads / SCL_WAVE; ++w)
      if (geo_before(wave_key[w], wave_row[w], best, row)) {
        best = wave_key[w];
        row = wave_row[w];
      }
    part_key[(long long)q * splits + split] = best;
    part_row[(long long)q * splits + split] = row;
  }
}

// one wave per query: the lanes go over the query's splits (a lane alone would read up to
// SCL_GEO_TARGET_BLOCKS dependent pairs one after the other), then the wave merges
__global__ __launch_bounds__(kThreads) void geo_finish_kernel(
    const u64* __restrict__ part_key, const int* __restrict__ part_row, int Q, int splits,
    int64_t* __restrict__ idx_out, double* __restrict__ dist_out) {
  const int lane = threadIdx.x & (SCL_WAVE - 1);
  const long long q = (long long)blockIdx.x * (kThreads / SCL_WAVE) + threadIdx.x / SCL_WAVE;
  if (q >= Q) return;                                  // (the whole wave)
  u64 best = kNoKey;
  int row = -1;
  for (int s = lane; s < splits; s += SCL_WAVE) {
    const u64 k = part_key[q * splits + s];
    const int r = part_row[q * splits + s];
    if (geo_before(k, r, best, row)) {
      best = k;
      row = r;
    }
  }
  geo_wave_merge(best, row);
  if (lane == 0) {
    idx_out[q] = row;
    dist_out[q] = row < 0 ? __builtin_inf() : sqrt(__longlong_as_double((long long)best));
  }
}

__global__ __launch_bounds__(kThreads) void geo_hit_dist_kernel(
    const f64x2* __restrict__ ref, int R, const f64x2* __restrict__ query, long long total, int n,
    const int64_t* __restrict__ idx, double* __restrict__ dist_out) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int64_t j = idx[i];
  double d = __builtin_inf();
  if (j >= 0 && j < R) d = sqrt(geo_d2(ref[j], query[i / n]));      // nothing is read for any other j
  dist_out[i] = d;
}

bool geo_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

}  // namespace

extern "C" size_t scl_geo_nearest_workspace_bytes(int R, int Q) {
  if (R < 1 || Q < 1) return 0;
  return geo_carve(nullptr, geo_pairs(R, Q)).bytes;
}

extern "C" int scl_geo_nearest(const double* ref_xy, int R, const double* query_xy, int Q,
                               int64_t* idx_out, double* dist_out, void* workspace,
                               size_t workspace_bytes, void* stream) {
  if (!ref_xy || !query_xy || !idx_out || !dist_out || !workspace) return SCL_E_NULL;
  if (R < 1 || Q < 1) return SCL_E_SHAPE;
  if (!geo_aligned16(ref_xy) || !geo_aligned16(query_xy)) return SCL_E_SHAPE;
  const GeoPlan plan = geo_plan(R, Q);
  const GeoWorkspace ws = geo_carve(workspace, geo_pairs(R, Q));
  if (workspace_bytes < ws.bytes || !scl_aligned256(workspace)) return SCL_E_WORKSPACE;
  const hipStream_t st = (hipStream_t)stream;
  const f64x2* ref = reinterpret_cast<const f64x2*>(ref_xy);
  const f64x2* query = reinterpret_cast<const f64x2*>(query_xy);
  const dim3 grid((unsigned)plan.qblocks, (unsigned)plan.splits);
  if (plan.small)
    SCL_LAUNCH("geo_nearest_refs_kernel", geo_nearest_refs_kernel, grid, dim3(kThreads), 0, st, ref, R,
               query, plan.slabs_per_split, plan.splits, ws.key, ws.row);
  else
    SCL_LAUNCH("geo_nearest_queries_kernel", geo_nearest_queries_kernel, grid, dim3(kThreads), 0, st,
               ref, R, query, Q, plan.slabs_per_split, plan.splits, ws.key, ws.row);
  const int per_block = kThreads / SCL_WAVE;        // a wave per query
  const dim3 fgrid((unsigned)(((long long)Q + per_block - 1) / per_block));
  SCL_LAUNCH("geo_finish_kernel", geo_finish_kernel, fgrid, dim3(kThreads), 0, st, ws.key, ws.row, Q,
             plan.splits, idx_out, dist_out);
  return scl_launch_status();
}

extern "C" int scl_geo_hit_dist(const double* ref_xy, int R, const double* query_xy, int Q,
                                const int64_t* idx, int n, double* dist_out, void* stream) {
  if (!ref_xy || !query_xy || !idx || !dist_out) return SCL_E_NULL;
  if (R < 1 || Q < 1 || n < 1) return SCL_E_SHAPE;
  const long long total = (long long)Q * n;
  if (total > (1LL << 38)) return SCL_E_SHAPE;
  if (!geo_aligned16(ref_xy) || !geo_aligned16(query_xy)) return SCL_E_SHAPE;
  const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
  SCL_LAUNCH("geo_hit_dist_kernel", geo_hit_dist_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream,
             reinterpret_cast<const f64x2*>(ref_xy), R, reinterpret_cast<const f64x2*>(query_xy), total,
             n, idx, dist_out);
  return scl_launch_status();
}
