// Soft contrastive loss, DIAGNOSTIC BUILD ONLY (csrc/Makefile: libscl_hip_diag.so, -DSCL_DIAG): the
// forward launch structures the product dispatch in gram_loss.hip no longer takes, reachable through
// scl_debug_set_variant for same-box A/B timing and parity runs.
//   41      the ONE-launch persistent forward for 32 < B <= 208 (gram16x6_persist_kernel,
//           gram16_persist_kernel: the Gram and persist_tail behind grid barriers); bit-identical to
//           the product's launches and slower (profiles/r06/loss_one_launch_persistent.txt)
//   39, 40  the same with no patience at the barriers (the repair path) / with clock stamps
//   37      round 5's four launches: gram16x6_kernel in front of the three finishing kernels
// gram_loss.hip calls gram_loss_fwd_diag after its argument checks; it returns false for every other
// variant, and the product dispatch runs.
#include "gram_loss.hip"

namespace {

//
// Cross-workgroup visibility (MI355X_MICROARCH.md, "Valid forms", first row of the table): every
// handed-off byte is stored sc1 (write-through), every storing wave drains its stores, a workgroup
// barrier, ONE lane's agent-scope add to the arrival counter; consumers poll the counter with an
// sc1 load, join a workgroup barrier and read every handed-off byte with sc1 loads.  No fence.
//
// The barrier SPINS, so the grid must be co-resident: the host only takes this path with at most
// one workgroup per CU of the device.  Correctness still never depends on it: the spin is bounded
// (a few ms), a workgroup that runs out of patience raises the ABORT bit, every workgroup that sees
// it leaves at once, and the LAST workgroup to leave the kernel — by then every slab is complete —
// runs phases 2-4 alone with the same routines (partition 0 of 1: the same sums in the same order,
// the same bits).  That is what happens when two such kernels from two streams each hold part of
// the chip, or when another kernel holds CUs for longer than the limit.
// sync words (8-byte aligned, zero on entry, zero on return): [0] arrivals | ABORT bit, [1] leavers.

typedef __attribute__((address_space(1))) unsigned* u32_gptr_t;
constexpr unsigned kAbortBit = 0x80000000u;
constexpr int kPersistSpinLimit = 20000;        // x (poll + s_sleep) ~ 5-10 ms

struct PersistArgs {
  unsigned* sync;
  const float* distances;
  const int64_t* labels;
  LossParams lp;
  const float* slabs;        // [S][P][256]
  float* gsum;               // [P][256] summed pair tiles
  float *gn, *gc, *rn, *rowloss;
  float* coef;
  float* loss_out;
  int S, T, P, B;
  int spin_limit;
  unsigned long long* stamps;   // diagnostics (scl_debug_set_variant(40), scripts/loss_stamps.py):
                                // [workgroup][16] shader-clock stamps of thread 0; null otherwise
};
#define PSTAMP(a, k)                                                                         \
  do {                                                                                       \
    if (SCL_DIAG_ONLY((a).stamps != nullptr) && threadIdx.x == 0)                            \
      (a).stamps[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime();                      \
  } while (0)

__device__ __forceinline__ void st_sc1_f32(float* p, float v) {
  __hip_atomic_store((__attribute__((address_space(1))) float*)p, v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_sc1_f32(__amdgpu_buffer_rsrc_t rsrc, unsigned byte_off) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, byte_off, 0, 16));
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_of(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}

// Arrive at the grid barrier number `phase` (1, 2, 3) and wait for the others.  false: aborted.
// flag: one LDS word.  Every wave's stores are drained before the arrival is counted.
__device__ __forceinline__ bool persist_barrier(unsigned* sync, unsigned target, int limit, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(sync, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int ok = 0;
    for (int spins = 0;; ++spins) {
      const unsigned x = __hip_atomic_load((u32_gptr_t)sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (x & kAbortBit) break;
      if (x >= target) {
        ok = 1;
        break;
      }
      if (spins >= limit) {
        __hip_atomic_fetch_or(sync, kAbortBit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
    *flag = ok;
  }
  __syncthreads();
  const int ok = *flag;
  __syncthreads();
  return ok != 0;
}

// entry (r, c) of the summed Gram: tile (min, max) of the upper triangle, lane 16 (row >> 2) + col,
// register row & 3 (gram16 / gram16x6 accumulator layout).  Diagonal tiles are read directly, as
// gram_reduce_kernel writes them.
__device__ __forceinline__ unsigned gsum_offset(int r, int c, int T) {
  int tr = r >> 4, tc = c >> 4, rr = r & 15, cc = c & 15;
  if (tr > tc) {
    const int t = tr;
    tr = tc;
    tc = t;
    const int q = rr;
    rr = cc;
    cc = q;
  }
  const int pair = tr * T - tr * (tr - 1) / 2 + (tc - tr);
  return (unsigned)(((pair * 64 + 16 * (rr >> 2) + cc) * 4 + (rr & 3)) * 4);
}

// phase 2: partition w of W.  lds: [4][64] f32x4.
__device__ __forceinline__ void persist_reduce(const PersistArgs& a, int w, int W, f32x4* part) {
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int N = 64 * a.P;
  const int lo = (int)(((long)N * w) / W), hi = (int)(((long)N * (w + 1)) / W);
  const __amdgpu_buffer_rsrc_t rsrc = rsrc_of(a.slabs, (unsigned)((size_t)a.S * a.P * 1024));
  constexpr int U = 16;                                        // gram_reduce_kernel's batches
  for (int base = lo; base < hi; base += 64) {
    const int item = base + lane < hi ? base + lane : hi - 1;   // (idle lanes re-read the last item)
    f32x4 acc4 = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = wid; s0 < a.S; s0 += 4 * U) {
      f32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {                            // (branch-free: clamped, masked below)
        const int sidx = s0 + 4 * u < a.S ? s0 + 4 * u : a.S - 1;
        v[u] = ld_sc1_x4(rsrc, (unsigned)((sidx * a.P * 64 + item) * 16));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) acc4 += s0 + 4 * u < a.S ? v[u] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    part[wid * 64 + lane] = acc4;
    __syncthreads();
    if (wid == 0 && base + lane < hi) {
      const f32x4 v = (part[lane] + part[64 + lane]) + (part[128 + lane] + part[192 + lane]);
      st_sc1_x4(a.gsum + (int64_t)(base + lane) * 4, v);
    }
    __syncthreads();
  }
}

// phase 3: rows i = w + W wid, + 4 W, ..: one wave per row, as gram_rows_wave_kernel<C>.
template <int C>
__device__ __forceinline__ void persist_rows(const PersistArgs& a, int w, int W) {
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int B = a.B;
  const __amdgpu_buffer_rsrc_t gs = rsrc_of(a.gsum, (unsigned)(a.P * 1024));
  const LossParams& lp = a.lp;
  for (int i = w + W * wid; i < B; i += 4 * W) {               // (wave-uniform)
    const float gii = ld_sc1_f32(gs, gsum_offset(i, i, a.T));
    float gij[C], gjj[C], d[C], gn[C], g[C];
    int same[C];
    const int64_t labi = a.labels ? a.labels[i] : 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = lane + 64 * c;
      const int jj = j < B ? j : B - 1;                        // (clamped: no branch around a load)
      gij[c] = ld_sc1_f32(gs, gsum_offset(i, jj, a.T));
      gjj[c] = ld_sc1_f32(gs, gsum_offset(jj, jj, a.T));
      d[c] = 0.f;
      same[c] = 0;
      if (j < B) {
        if (lp.mask_kind == SCL_MASK_LABELS)
          same[c] = a.labels[j] == labi;
        else
          d[c] = lp.dist_rank3 ? a.distances[(int64_t)j * B + i] : a.distances[(int64_t)i * B + j];
      }
    }
    const float rni = 1.0f / sqrtf(fmaxf(gii, 1e-12f));
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = lane + 64 * c;
      const float rnj = 1.0f / sqrtf(fmaxf(gjj[c], 1e-12f));
      gn[c] = j < B ? gij[c] * rni * rnj : 0.f;
    }
    const float rl = wave_row_eval<C>(i, B, lane, gn, d, same, lp, 1.0f / (float)B, g);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int j = lane + 64 * c;
      if (j < B) {
        st_sc1_f32(a.gn + (int64_t)i * B + j, gn[c]);
        st_sc1_f32(a.gc + (int64_t)i * B + j, g[c]);
      }
    }
    if (lane == 0) {
      st_sc1_f32(a.rowloss + i, rl);
      st_sc1_f32(a.rn + i, rni);
    }
  }
}

// phase 4: rows i = w, w + W, ..: the whole workgroup per row, as gram_coef_kernel (B <= 256:
// thread j holds column j).  scratch: 32 floats.
__device__ __forceinline__ void persist_coef(const PersistArgs& a, int w, int W, float* scratch) {
  const int B = a.B, j = threadIdx.x;
  const __amdgpu_buffer_rsrc_t rgn = rsrc_of(a.gn, (unsigned)(B * B * 4)), rgc = rsrc_of(a.gc, (unsigned)(B * B * 4)),
                               rrn = rsrc_of(a.rn, (unsigned)(B * 4)), rrl = rsrc_of(a.rowloss, (unsigned)(B * 4));
  const int jj = j < B ? j : B - 1;
  if (w == 0) {
    float s = j < B ? ld_sc1_f32(rrl, (unsigned)(jj * 4)) : 0.f;
    s = block_reduce<0>(s, scratch);
    if (threadIdx.x == 0) *a.loss_out = s / (float)B;
  }
  if (!a.coef) return;
  const float rnj = ld_sc1_f32(rrn, (unsigned)(jj * 4));
  for (int i = w; i < B; i += W) {
    const float gs = ld_sc1_f32(rgc, (unsigned)((i * B + jj) * 4)) + ld_sc1_f32(rgc, (unsigned)((jj * B + i) * 4));
    float c = j < B ? gs * ld_sc1_f32(rgn, (unsigned)((i * B + jj) * 4)) : 0.f;
    c = block_reduce<0>(c, scratch);
    const float rni = ld_sc1_f32(rrn, (unsigned)(i * 4));
    const bool clamped = rni >= 1.0e6f;                        // see gram_coef_kernel
    if (j < B) {
      float m = rni * rnj * gs;
      if (j == i && !clamped) m -= rni * rni * c;
      a.coef[(int64_t)i * B + j] = m;
    }
    __syncthreads();                                           // scratch is reused by the next row
  }
}

__device__ __forceinline__ void persist_rows_any(const PersistArgs& a, int w, int W) {
  if (a.B <= 64)
    persist_rows<1>(a, w, W);
  else if (a.B <= 128)
    persist_rows<2>(a, w, W);
  else if (a.B <= 192)
    persist_rows<3>(a, w, W);
  else
    persist_rows<4>(a, w, W);
}

// Everything behind the Gram phase of a 256-thread workgroup.  lds: >= 4.5 KB, dead Gram data.
// One loop body serves both the normal run (partition blockIdx of gridDim, grid barriers between
// the phases) and the repair run of the last workgroup out (partition 0 of 1, its own barriers).
__device__ __forceinline__ void persist_tail(const PersistArgs& a, float* lds) {
  f32x4* part = reinterpret_cast<f32x4*>(lds);                 // [4][64]
  float* scratch = lds + 1024;                                 // [32]
  int* flag = reinterpret_cast<int*>(lds + 1024 + 32);
  int W = gridDim.x, w = blockIdx.x;
  bool solo = false;
  for (;;) {
    auto barrier = [&](unsigned k) -> bool {
      if (solo) {                                              // own stores -> own sc1 loads
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        return true;
      }
      return persist_barrier(a.sync, k * gridDim.x, a.spin_limit, flag);
    };
    PSTAMP(a, 2);
    bool ok = barrier(1u);
    PSTAMP(a, 3);
    if (ok) {
      persist_reduce(a, w, W, part);
      PSTAMP(a, 4);
      ok = barrier(2u);
      PSTAMP(a, 5);
    }
    if (ok) {
      persist_rows_any(a, w, W);
      PSTAMP(a, 6);
      ok = barrier(3u);
      PSTAMP(a, 7);
    }
    if (ok) persist_coef(a, w, W, scratch);
    PSTAMP(a, 8);
    if (solo) break;
    // ---- leave.  The last workgroup out repairs an aborted run; it puts the words back to zero.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned left = __hip_atomic_fetch_add(a.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int role = 0;
      if (left == gridDim.x - 1) {
        const unsigned x = __hip_atomic_load((u32_gptr_t)a.sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        role = (x & kAbortBit) ? 2 : 1;
      }
      *flag = role;
    }
    __syncthreads();
    const int role = *flag;
    __syncthreads();
    if (role == 0) return;
    if (role == 1) break;
    solo = true;                                               // every slab is complete by now
    w = 0;
    W = 1;
  }
  if (threadIdx.x == 0) {
    __hip_atomic_store(a.sync, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(a.sync + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}


template <bool DUAL, int SMAX>
__global__ __launch_bounds__(256) void gram16x6_persist_kernel(const float* __restrict__ emb, int64_t ld,
                                                               float* __restrict__ slabs, PersistArgs pa) {
  extern __shared__ __attribute__((aligned(16))) unsigned x6p_lds[];
  PSTAMP(pa, 0);
  gram16x6p_body<DUAL, SMAX, true>(emb, ld, pa.B, pa.T, pa.P, slabs, SCL_DIAG_ONLY(pa.stamps));
  persist_tail(pa, reinterpret_cast<float*>(x6p_lds));
}

// 32 < B <= 64: the exact-float32 Gram of gram16_kernel in front of the same tail.
template <int PWMAX, bool FULL>
__global__ __launch_bounds__(256) void gram16_persist_kernel(const float* __restrict__ emb, int64_t ld,
                                                             int E, int kchunk, int KS, int vec_ok,
                                                             float* __restrict__ slabs, PersistArgs pa) {
  extern __shared__ __attribute__((aligned(16))) float g16_lds[];
  PSTAMP(pa, 0);
  gram16_body<PWMAX, FULL, false, true>(emb, ld, pa.B, E, pa.T, pa.P, kchunk, KS, vec_ok, slabs, FinalArgs{});
  persist_tail(pa, g16_lds);
}

template <bool DUAL, int SMAX>
void launch_x6_persist(const float* emb, int64_t ld, int E, float* slabs, const PersistArgs& pa,
                       hipStream_t st) {
  static SclDeviceOnce once;
  scl_call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gram16x6_persist_kernel<DUAL, SMAX>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  });
  const size_t lds = (size_t)2 * 3 * 8 * (16 * pa.T + 1) * 16;
  SCL_LAUNCH("gram16x6_persist_kernel", (gram16x6_persist_kernel<DUAL, SMAX>), dim3(E / 128), dim3(256), lds, st,
             emb, ld, slabs, pa);
}


template <int PWMAX, bool FULL>
void launch_gram16_persist(const Gram16Plan& p, const float* emb, int64_t ld, int E, int vec_ok,
                           float* slabs, const PersistArgs& pa, hipStream_t st) {
  static SclDeviceOnce once;
  scl_call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&gram16_persist_kernel<PWMAX, FULL>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, 132 * 1024);
  });
  size_t lds = gram16_lds(p);
  if (lds < 8 * 1024) lds = 8 * 1024;                         // persist_tail's tables
  SCL_LAUNCH("gram16_persist_kernel", (gram16_persist_kernel<PWMAX, FULL>), dim3(p.S), dim3(256), lds, st,
             emb, ld, E, p.kchunk, p.KS, vec_ok, slabs, pa);
}

}  // namespace

static bool gram_loss_fwd_diag(const float* emb, int64_t ld_emb, int B, int E, const float* distances,
                               const int64_t* labels, const LossParams& lp, float* coef, float* loss_out,
                               void* sync_words, int vec_ok, const GramWs& w, hipStream_t st, int* rc) {
  const int v = scl_variant();
  if (B > kFastB || (v != 37 && v != 39 && v != 40 && v != 41)) return false;
  // the product's plan (none of these variants is a pin): its Gram kernel decides the persistent one
  const GramFwdPlan f = gram_fwd_plan(B, E, vec_ok, sync_words != nullptr, GramPins{});
  const Gram16Plan& p = f.p;
  const bool x6p = f.route == GramFwd::X6p, x6 = x6p || f.route == GramFwd::X6;
  if (v != 37) {
    const int grid = p.S;
    if (!(B > 32 && sync_words && ((uintptr_t)sync_words % 8) == 0 && (x6p || (!x6 && B <= 64)) &&
          grid <= scl_device_cus()))
      return false;
    PersistArgs pa;
    pa.sync = (unsigned*)sync_words;
    pa.distances = distances;
    pa.labels = labels;
    pa.lp = lp;
    pa.slabs = w.slabs;
    pa.gsum = w.gsum;
    pa.gn = w.gn;
    pa.gc = w.gc;
    pa.rn = w.rn;
    pa.rowloss = w.rowloss;
    pa.coef = coef;
    pa.loss_out = loss_out;
    pa.S = grid;
    pa.T = p.T;
    pa.P = p.P;
    pa.B = B;
    pa.spin_limit = v == 39 ? 0 : kPersistSpinLimit;   // 39: no patience (the repair path)
    pa.stamps = v == 40 ? w.stamps : nullptr;          // 40: clock stamps
    if (x6p) {
      if ((p.P + 3) / 4 <= 20)
        launch_x6_persist<true, 11>(emb, ld_emb, E, w.slabs, pa, st);
      else
        launch_x6_persist<false, 13>(emb, ld_emb, E, w.slabs, pa, st);
    } else if (f.pw == 3 && f.full)
      launch_gram16_persist<3, true>(p, emb, ld_emb, E, vec_ok, w.slabs, pa, st);
    else if (f.pw <= 3)
      launch_gram16_persist<3, false>(p, emb, ld_emb, E, vec_ok, w.slabs, pa, st);
    else if (f.pw <= 5)
      launch_gram16_persist<5, false>(p, emb, ld_emb, E, vec_ok, w.slabs, pa, st);
    else
      return false;
    *rc = scl_launch_status();
    return true;
  }
  // 37: the bf16x6 route through gram16x6_kernel (B > 64 there), then the product's finishing launches
  if (!x6) return false;
  const GramFwdCall c = {emb, ld_emb, B, E, vec_ok, w.slabs, st};
  if (f.pw <= 9)
    launch_gram16x6<9, true>(p, x6_lds_bytes(p.T), c);
  else if (f.pw <= 20)
    launch_gram16x6<20, true>(p, x6_lds_bytes(p.T), c);
  else
    launch_gram16x6<34, false>(p, x6_lds_bytes(p.T), c);
  SCL_LAUNCH("gram_reduce_kernel", gram_reduce_kernel, dim3(p.P), dim3(256), 0, st,
             (const float*)w.slabs, p.S, p.T, p.P, B, w.gfull);
  const dim3 rg((B + 3) / 4);
#define SCL_ROWS(C)                                                                          \
  SCL_LAUNCH("gram_rows_wave_kernel", gram_rows_wave_kernel<C>, rg, dim3(256), 0, st,             \
             (const float*)w.gfull, B, distances, labels, lp, w.gn, w.gc, w.rn, w.rowloss)
  if (B <= 128)
    SCL_ROWS(2);
  else if (B <= 192)
    SCL_ROWS(3);
  else
    SCL_ROWS(4);
#undef SCL_ROWS
  SCL_LAUNCH("gram_coef_kernel", gram_coef_kernel, dim3(coef ? B : 1), dim3(256), 0, st, w.gn, w.gc, w.rn,
             w.rowloss, B, coef, loss_out);
  *rc = scl_launch_status();
  return true;
}
