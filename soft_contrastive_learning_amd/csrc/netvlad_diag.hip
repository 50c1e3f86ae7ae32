// NetVLAD head, DIAGNOSTIC BUILD ONLY (csrc/Makefile: libscl_hip_diag.so, -DSCL_DIAG): the kernels
// and launch structures the product dispatch in netvlad.hip no longer takes, reachable through
// scl_debug_set_variant for same-box A/B timing, ablations and parity runs.
//   1 .. 7   rowtile16_kernel<ASSIGN> ablations (scripts/ablate_rowtile.py; results meaningless):
//            the float32-MFMA forward (vlad_f32_forward) with the ablated kernel, on either map type;
//            backward as 8
//   8        a bf16 map through the plain float32-MFMA kernels, forward and backward (the only
//            place their unsigned short instantiations exist; it needs the saved logits)
//   916, 922 round 3's four-wave fused kernels vlad_fwd_kernel / vlad_bwd_kernel (916: clock stamps)
//   918      vlad_fwd8_kernel with clock stamps when it saves (scripts/vlad_stamps.py)
//   920      round 3's launch structure: separate plane split, finish_sum, finish_norm, bwd_dots,
//            bwd_du, wgrad_partial and wgrad_finish kernels around the four-wave kernels
// (917, 918 without saving, 921, 923, 924 are knobs of the product launches: vlad_plan, netvlad.hip.)
// netvlad.hip calls netvlad_fwd_diag / netvlad_bwd_diag after its argument checks, plan and carve; they
// return false for every other variant, and the product dispatch runs.  The launch structures here call
// the product's helpers (vlad_fwd_args, launch_vlad_finish, launch_bwd_prologue, ...) and swap only the
// kernel, LDS size and block size their variant swaps.
#include "netvlad.hip"

namespace {

// ---- what only the four-wave kernels and round 3's launch structure use
constexpr int VF_AHEAD = 6;                      // A fragments in flight in the aggregation (<= 7)
constexpr int VF_EXCH = 4 * VF_STEP * 16;         // [wave][location][up to 4 floats]
constexpr size_t kVladFusedLds = (size_t)VF_NST * VF_STAGE + 4 * VF_CF + VF_EXCH;   // 118,784 B
// counted wait on the wave's vector-memory queue (immediate operand: a small switch)
__device__ __forceinline__ void vf_wait_vm(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

// W [512][64] float32 -> register images of the fused kernels: 16-byte unit
// ((w * 16 + s) * VF_NPL + plane) * 64 + lane  holds  W_plane[ch 32 s + 8 g + e][cluster 16 w + i],
// e = 0..7, for lane = 16 g + i: wave w loads its 48 fragments with coalesced 16-byte loads.
// VF_WREP identical copies, workgroups take copy (slice index) % VF_WREP.  (Tried with 4: every
// workgroup reads this image in the same order at the same time, but the prologue — 8.3 k cycles
// for 192 KB + 64 KB of x — did not move: it runs at the CU's L2 -> register rate, 30 B per cycle,
// not into a hot L2 channel.  Left at 1.)
// grid (64, VF_WREP), block 64 (block = (w, s)).
constexpr int VF_WREP = 1;
constexpr int VF_WIMG = VF_NPL * D * K;           // bf16 elements per copy
__global__ __launch_bounds__(64) void vlad_split_w_kernel(const float* __restrict__ w,
                                                          unsigned short* __restrict__ img) {
  const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
  const int wv = blockIdx.x >> 4, s = blockIdx.x & 15;
  img += (int64_t)blockIdx.y * VF_WIMG;
  unsigned short h[3][8];
#pragma unroll
  for (int e = 0; e < 8; ++e)
    split3_bf16(w[(32 * s + 8 * g + e) * K + 16 * wv + i], h[0][e], h[1][e], h[2][e]);
#pragma unroll
  for (int pl = 0; pl < VF_NPL; ++pl) {
    uint4 v;
    v.x = (unsigned)h[pl][0] | ((unsigned)h[pl][1] << 16);
    v.y = (unsigned)h[pl][2] | ((unsigned)h[pl][3] << 16);
    v.z = (unsigned)h[pl][4] | ((unsigned)h[pl][5] << 16);
    v.w = (unsigned)h[pl][6] | ((unsigned)h[pl][7] << 16);
    reinterpret_cast<uint4*>(img)[(((wv * 16 + s) * VF_NPL + pl) * 64) + lane] = v;
  }
}

// =======================================================================================
// Fused kernels for bf16 feature maps (round 3): ONE pass over x per direction.
//
// vlad_fwd_kernel: soft-assignment AND aggregation of one (image, location slice) per
// workgroup.  What bounded the two-kernel form (rowtile_ring + aggregate16b) was bytes per CU,
// not matrix or LDS time: every 128 locations re-streamed the 196 KB operand image of W
// through the CU's L2 -> LDS path (12-13 B per cycle and CU), and x and the assignments made a
// second trip for the aggregation.  Here
//   * W^T lives in REGISTERS for the whole kernel: wave w owns clusters 16 w .. 16 w + 15 as
//     three bf16 planes (16 k-steps x 3 planes x 4 registers = 192 per lane);
//   * the partial VLAD of the slice lives in REGISTERS too: V[512 channels][the wave's 16
//     clusters] = 32 accumulator tiles = 128 per lane (one wave per SIMD, 512-register budget);
//   * only x moves: 32-location steps through a 3-stage LDS ring filled by LDS-DMA (32 KB per
//     stage, two stages in flight), each x tile consumed twice while it is in LDS — row-wise
//     (ds_read_b128) as the B operand of the logits, column-wise (ds_read_b64_tr_b16) as the A
//     operand of the aggregation.  Unit u(loc, c) = 64 loc + (c ^ (loc & 15)) (c = 16-byte
//     chunk of the row) makes both kinds of read conflict-free (scripts/lds_conflicts.py); the
//     swizzle sits on the DMA's source address.
// The logits run with the operands SWAPPED (S^T = W^T x^T), so a lane holds four consecutive
// clusters of ONE location: the softmax needs two cross-lane steps instead of four per value, and
// a / logits leave as 16-byte stores.  Row norms come from the matrix cores as well: x_frag is
// both operands of one more MFMA per k-step, whose diagonal is sum_d x^2 (bf16 products are
// exact in float32).  The softmax over the 64 clusters spans the four waves: each wave
// publishes (max, sum exp) of its 16 clusters per location, ONE barrier, then every wave
// finishes a = e^(s - m_w) e^(m_w - M) / total.  The coefficients a * rn then go through a
// per-wave [32 loc][16 cl] x 3-plane LDS image (8-byte writes, transposed reads) to become
// the B operand of the aggregation — no round trip through HBM, no second read of x.
// Contraction index k = 8 g + e of the aggregation is location pi(k) of the step (see vf_pi):
// any permutation works as long as both operands use it, and this one keeps the transposed
// reads of the x tile conflict-free.
// Output: a, logits, rn (training), the slice's slab in accumulator order and its column sums
// of a.  grid (S slices, B images), block 256, one workgroup per CU.
//
// What its stamps showed, and why round 4 went to the eight-wave kernels of netvlad.hip
// (profiles/r03/vlad_stamps_fwd.txt): a 32-location step takes 6.4 k cycles, of which 160 MFMAs x 16
// cycles = 2.6 k are matrix work; the rest is the softmax / coefficient arithmetic and its cross-lane
// and LDS traffic (2.1 k), LDS latency in front of the aggregation's products, and two barriers — all
// strictly one after the other, because a wave that owns a SIMD alone issues in order: a vector
// instruction costs it 4 cycles (2 with a second wave on the SIMD) and nothing runs while it waits.
template <bool SAVE>
__global__ __launch_bounds__(256, 1) void vlad_fwd_kernel(VladFwdArgs p) {
  // 1 KB alignment: the transposed-read addresses are formed by XOR on (stage base + offset)
  extern __shared__ __attribute__((aligned(1024))) unsigned char vf_lds[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  // image on blockIdx.x: workgroup b + B * sl, so with B a multiple of 8 all slices of an image
  // run on one XCD (round-robin placement: speed only) and their slabs meet in one L2
  const int b = blockIdx.x, sl = blockIdx.y, B = gridDim.x;
  const int nsteps_img = (p.N + VF_STEP - 1) / VF_STEP;
  const int st_lo = sl * p.steps_per_slice;
  const int st_hi = st_lo + p.steps_per_slice < nsteps_img ? st_lo + p.steps_per_slice : nsteps_img;
  const int nst = st_hi - st_lo;                           // >= 1 by the host's choice of S
  const unsigned lds0 = lds_byte_of(vf_lds);
  const unsigned cf0 = lds0 + VF_NST * VF_STAGE + wid * VF_CF;
  float* exch = reinterpret_cast<float*>(vf_lds + VF_NST * VF_STAGE + 4 * VF_CF);
  const unsigned short* xb = p.x + (int64_t)b * p.N * D;
  unsigned long long* stp =
      (SCL_DIAG_ONLY(p.dbg) & 16) && threadIdx.x == 0 ? p.stamps + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 32 : nullptr;
#define VF_STAMP(k)                                         \
  do {                                                      \
    if (SCL_DIAG_ONLY(p.dbg) & 16) {                                       \
      __builtin_amdgcn_sched_barrier(0);                    \
      if (stp) stp[k] = __builtin_amdgcn_s_memtime();       \
      __builtin_amdgcn_sched_barrier(0);                    \
    }                                                       \
  } while (0)
  VF_STAMP(0);
  // (the finish kernel behind this one polls these words: they must be zero when it starts)
  if (sl == 0 && threadIdx.x < 8) p.gran[b * 8 + threadIdx.x] = 0ull;

  // ---- x stage by LDS-DMA: wave w brings rows w, w + 4, .. of the step; lane l of row r
  // fetches chunk l ^ (r & 15) into unit 64 r + l (rows past the end re-read the last row)
  auto stage = [&](int step) {
    const unsigned base = lds0 + (unsigned)((step - st_lo) % VF_NST) * VF_STAGE;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int r = wid + 4 * v;
      int n = VF_STEP * step + r;
      n = n < p.N ? n : p.N - 1;
      glds16(xb + (int64_t)n * D + ((lane ^ (r & 15)) << 3), base + r * 1024);
    }
  };
  stage(st_lo);
  if (nst > 1) stage(st_lo + 1);

  // ---- the wave's slice of W^T: 16 k-steps x 3 planes
  u32x4 wf[16][VF_NPL];
  {
    const u32x4* src = reinterpret_cast<const u32x4*>(p.wimg + (int64_t)(sl % VF_WREP) * VF_WIMG) +
                       (int64_t)wid * 16 * VF_NPL * 64 + lane;
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int pl = 0; pl < VF_NPL; ++pl) wf[s][pl] = src[(s * VF_NPL + pl) * 64];
  }

  if (SCL_DIAG_ONLY(p.dbg) & 16) {
    VF_STAMP(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    VF_STAMP(2);
  }
  f32x4 accv[32];
#pragma unroll
  for (int ct = 0; ct < 32; ++ct) accv[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float cs[4] = {0.f, 0.f, 0.f, 0.f};

  // per-lane address parts.  Row fragment of (t, s): unit (16 t + i, 4 s + g):
  //   byte = 1024 (16 t + i) + 64 (s ^ (i >> 2)) + 16 (g ^ (i & 3));  s ^ ih = (s & ~3) | ((s & 3) ^ ih)
  unsigned rowoff[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) rowoff[k] = 1024u * i + 64u * (k ^ (i >> 2)) + 16u * (g ^ (i & 3));
  // Transposed fragment (half h): lane 4 q + p of group g reads 8 bytes at row pi(8 g + 4 h + q),
  // channels 16 ct + 4 p ..: byte = 1024 row + ((32 Rh + 16 (pb ^ R0) + 8 (p & 1)) ^ 32 ct)
  float dsel[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dsel[j] = (g == (i >> 2) && (i & 3) == j) ? 1.0f : 0.0f;
  const int q = (lane >> 2) & 3, pp = lane & 3;
  unsigned troff[2], cfoff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = 16 * (g >> 1) + 2 * (4 * (g & 1) + q) + h;     // vf_pi(g, 4 h + q)
    const int R = row & 15;
    troff[h] = 1024u * row + 32u * (R >> 1) + 16u * ((pp >> 1) ^ (R & 1)) + 8u * (pp & 1);
    cfoff[h] = (unsigned)row * VF_CFLD + 8u * pp;
  }

#pragma unroll 1
  for (int st = 0; st < nst; ++st) {
    const int step = st_lo + st;
    // This stage's DMA must have landed; younger than it in the wave's queue, and allowed to
    // stay in flight: the next stage's DMA (8) and the previous step's stores (5 when saving).
    vf_wait_vm((st + 1 < nst ? 8 : 0) + (st >= 1 && SAVE ? 5 : 0));
    __builtin_amdgcn_s_barrier();         // landed for every wave; the stage read in step - 1 is free
    if (st < 4) VF_STAMP(4 + 6 * st);
    const unsigned sb = lds0 + (unsigned)(st % VF_NST) * VF_STAGE;

    // ---- logits (swapped: lane = location, registers = 4 consecutive clusters) + row norms
    f32x4 accl[2], accn[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      accl[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      accn[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    u32x4 xf[4][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        xf[s][t] = vf_ldsr128(sb + rowoff[s & 3] + 256u * (s >> 2) + 16384u * t);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s + 2 < 16) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
          xf[(s + 2) & 3][t] =
              vf_ldsr128(sb + rowoff[(s + 2) & 3] + 256u * ((s + 2) >> 2) + 16384u * t);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int pl = 0; pl < VF_NPL; ++pl) accl[t] = mfma16b(wf[s][pl], xf[s & 3][t], accl[t]);
        accn[t] = mfma16b(xf[s & 3][t], xf[s & 3][t], accn[t]);
      }
    }

    if (st < 4) VF_STAMP(5 + 6 * st);
    // ---- softmax over the 64 clusters (this wave: 16 of them), coefficients, outputs
    float av[2][4], ev[2][4], mloc[2], rnv[2];
    bool ok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n = VF_STEP * step + 16 * t + i;
      ok[t] = n < p.N;
      // diagonal of the tile's Gram: row 4 g + j == column i (dsel: 1 on that register, else 0)
      float d = accn[t][0] * dsel[0] + accn[t][1] * dsel[1] + accn[t][2] * dsel[2] + accn[t][3] * dsel[3];
      d = vf_gsum(d);
      rnv[t] = p.pre_l2 ? rsqrtf(fmaxf(d, 1e-12f)) : 1.0f;
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ev[t][j] = accl[t][j] * rnv[t];                    // the logit
        m = fmaxf(m, ev[t][j]);
      }
      m = vf_gmax(m);
      mloc[t] = m;
      if (SAVE)
        *reinterpret_cast<f32x4*>(ok[t] ? p.logit + ((int64_t)b * p.N + n) * K + 16 * wid + 4 * g
                                        : p.trash + 4 * lane) =
            f32x4{ev[t][0], ev[t][1], ev[t][2], ev[t][3]};
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ev[t][j] = __expf(ev[t][j] - m);
        sum += ev[t][j];
      }
      sum = vf_gsum(sum);
      if (g == 0) *reinterpret_cast<f32x2*>(exch + (wid * VF_STEP + 16 * t + i) * 2) = f32x2{m, sum};
    }
    __builtin_amdgcn_s_barrier();
    if (st < 4) VF_STAMP(6 + 6 * st);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n = VF_STEP * step + 16 * t + i;
      f32x2 ms[4];
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2)
        ms[w2] = *reinterpret_cast<const f32x2*>(exch + (w2 * VF_STEP + 16 * t + i) * 2);
      const float M = fmaxf(fmaxf(ms[0][0], ms[1][0]), fmaxf(ms[2][0], ms[3][0]));
      float tot = 0.f;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) tot += ms[w2][1] * __expf(ms[w2][0] - M);
      const float sc = __fdividef(__expf(mloc[t] - M), tot);
      unsigned short h[3][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        av[t][j] = ev[t][j] * sc;
        const float a_ok = ok[t] ? av[t][j] : 0.f;
        cs[j] += a_ok;
        split3_bf16(a_ok * rnv[t], h[0][j], h[1][j], h[2][j]);
      }
      if (SAVE)
        *reinterpret_cast<f32x4*>(ok[t] ? p.assign + ((int64_t)b * p.N + n) * K + 16 * wid + 4 * g
                                        : p.trash + 4 * lane) =
            f32x4{av[t][0], av[t][1], av[t][2], av[t][3]};
#pragma unroll
      for (int pl = 0; pl < VF_NPL; ++pl) {
        vf_ldsw64(cf0 + pl * VF_CFPL + (16 * t + i) * VF_CFLD + 8 * g,
                  (unsigned)h[pl][0] | ((unsigned)h[pl][1] << 16),
                  (unsigned)h[pl][2] | ((unsigned)h[pl][3] << 16));
      }
    }
    if (SAVE) {   // rn: wave w writes the step's locations 8 w .. 8 w + 7 (one store per wave)
      const int t = wid >> 1;
      const int n = VF_STEP * step + 16 * t + i;
      const float r = t == 0 ? rnv[0] : rnv[1];
      const bool mine = g == 0 && (i >> 3) == (wid & 1) && n < p.N;
      *(mine ? p.rnorm + (int64_t)b * p.N + n : p.trash + 4 * lane) = r;
    }

    if (st < 4) VF_STAMP(7 + 6 * st);
    if (st + 2 < nst) stage(step + 2);     // into the stage of step - 1

    // ---- aggregation: V[ch][cl] += sum_loc x[loc][ch] * (a rn)[loc][cl]
    u32x4 bfr[VF_NPL];
#pragma unroll
    for (int pl = 0; pl < VF_NPL; ++pl) {
      const uint2 lo = lds_tr16_at(cf0 + pl * VF_CFPL + cfoff[0]);
      const uint2 hi = lds_tr16_at(cf0 + pl * VF_CFPL + cfoff[1]);
      bfr[pl] = u32x4{lo.x, lo.y, hi.x, hi.y};
    }
    // address of the transposed fragment of channel tile ct: (stage + troff[h]) ^ 32 ct touches
    // address bits 5..9 only, and (Rh ^ ct) = (ct & 24) | ((ct & 7) ^ Rh): eight per-lane bases
    // (ct & 7) per half, the rest is an immediate offset — no address arithmetic in the loop
    unsigned ta[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c7 = 0; c7 < 8; ++c7) ta[h][c7] = sb + (troff[h] ^ (32u * c7));
    // A fragments VF_AHEAD channel tiles ahead of the matrix work (an LDS round trip is several
    // times the MFMAs of a tile)
    u32x4 af[8];
#pragma unroll
    for (int ct = 0; ct < VF_AHEAD; ++ct) {
      const uint2 lo = lds_tr16_at(ta[0][ct & 7] + 32u * (ct & 24)), hi = lds_tr16_at(ta[1][ct & 7] + 32u * (ct & 24));
      af[ct] = u32x4{lo.x, lo.y, hi.x, hi.y};
    }
#pragma unroll
    for (int ct = 0; ct < 32; ++ct) {
      if (ct + VF_AHEAD < 32) {
        const int cn = ct + VF_AHEAD;
        const uint2 lo = lds_tr16_at(ta[0][cn & 7] + 32u * (cn & 24)),
                    hi = lds_tr16_at(ta[1][cn & 7] + 32u * (cn & 24));
        af[cn & 7] = u32x4{lo.x, lo.y, hi.x, hi.y};
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pl = 0; pl < VF_NPL; ++pl) accv[ct] = mfma16b(af[ct & 7], bfr[pl], accv[ct]);
    }
    if (st < 4) VF_STAMP(8 + 6 * st);
  }
  VF_STAMP(28);

  // ---- the slice's slab, in accumulator order, and the column sums of a
  f32x4* slab = reinterpret_cast<f32x4*>(p.slab) + ((((int64_t)sl * B + b) * 4 + wid) * 32) * 64 + lane;
#pragma unroll
  for (int ct = 0; ct < 32; ++ct) slab[ct * 64] = accv[ct];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) cs[j] += __shfl_xor(cs[j], m, 64);
  }
  if (i == 0)
    *reinterpret_cast<f32x4*>(p.colsum + ((int64_t)sl * B + b) * K + 16 * wid + 4 * g) =
        f32x4{cs[0], cs[1], cs[2], cs[3]};
  if (SCL_DIAG_ONLY(p.dbg) & 16) {
    VF_STAMP(29);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    VF_STAMP(30);
  }
#undef VF_STAMP
}

// U = sum of the slices' slabs + C * asum for one 16-channel tile -> vlad[b] (natural [513][64]
// layout, the saved pre-norm VLAD) and the tile's column sums of squares.  Slabs are in
// accumulator order: 16-byte unit ((w * 32 + ct) * 64 + lane) = U[16 ct + 4 g + 0..3][16 w + i].
// grid (B, 32 channel tiles), block 256: thread = (wave w, lane); all S loads of a thread are in
// flight together (31 MB of slabs at 24 x 1200: a reader with one load at a time took 20 us).
// Image on blockIdx.x like vlad_fwd_kernel: with B a multiple of 8 an image's slabs are read on
// the XCD whose L2 they were written through (placement is speed only).
constexpr int VF_MAXS = 16;
__global__ __launch_bounds__(256) void vlad_finish_sum_kernel(const float* __restrict__ slab,
                                                              const float* __restrict__ colsum,
                                                              const float* __restrict__ centers,
                                                              int S, float* __restrict__ vlad,
                                                              float* __restrict__ colsq_part) {
  const int b = blockIdx.x, ct = blockIdx.y, B = gridDim.x;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int k = 16 * w + i;
  const f32x4* src = reinterpret_cast<const f32x4*>(slab) + (((int64_t)b * 4 + w) * 32 + ct) * 64 + lane;
  const int64_t sstride = (int64_t)B * 4 * 32 * 64;          // units between slices
  f32x4 u = f32x4{0.f, 0.f, 0.f, 0.f};
  float asum = 0.f;
  for (int s0 = 0; s0 < S; s0 += VF_MAXS) {
    f32x4 v[VF_MAXS];
    float a[VF_MAXS];
#pragma unroll
    for (int s = 0; s < VF_MAXS; ++s) {
      const bool ok = s0 + s < S;
      v[s] = ok ? src[(s0 + s) * sstride] : f32x4{0.f, 0.f, 0.f, 0.f};
      a[s] = ok ? colsum[((int64_t)(s0 + s) * B + b) * K + k] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < VF_MAXS; ++s) {                       // fixed order: bitwise reproducible
      u += v[s];
      asum += a[s];
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = 16 * ct + 4 * g + j;
    const float v = u[j] + centers[d * K + k] * asum;
    vlad[((int64_t)b * VROWS + d) * K + k] = v;
    ss = fmaf(v, v, ss);
  }
  if (ct == 0 && g == 0) vlad[((int64_t)b * VROWS + D) * K + k] = asum;
  ss = vf_gsum(ss);
  if (g == 0) colsq_part[((int64_t)b * 32 + ct) * K + k] = ss;
}

// vlad_bwd_kernel: the backward twin of vlad_fwd_kernel — x.dU[b], the softmax backward and the
// weight-gradient aggregation x^T.(ds rn) of one (image, location slice) in one pass over x.
// The image's dU^T sits in registers (the same register image the forward uses for W^T), the slice's
// partial dW in the accumulators.  The four partial sums P1 .. P4 each wave publishes per location
// and what follows the ONE barrier: vlad_bwd8_kernel's comment (netvlad.hip); here lg are the SAVED
// logits.  Outputs: ds, rowdot, the slice's dW slab.
__global__ __launch_bounds__(256, 1) void vlad_bwd_kernel(VladBwdArgs p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char vf_lds[];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int b = blockIdx.x, sl = blockIdx.y, B = gridDim.x;
  const int nsteps_img = (p.N + VF_STEP - 1) / VF_STEP;
  const int st_lo = sl * p.steps_per_slice;
  const int st_hi = st_lo + p.steps_per_slice < nsteps_img ? st_lo + p.steps_per_slice : nsteps_img;
  const int nst = st_hi - st_lo;
  const unsigned lds0 = lds_byte_of(vf_lds);
  const unsigned cf0 = lds0 + VF_NST * VF_STAGE + wid * VF_CF;
  float* exch = reinterpret_cast<float*>(vf_lds + VF_NST * VF_STAGE + 4 * VF_CF);   // [wave][loc][4]
  const unsigned short* xb = p.x + (int64_t)b * p.N * D;

  auto stage = [&](int step) {
    const unsigned base = lds0 + (unsigned)((step - st_lo) % VF_NST) * VF_STAGE;
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int r = wid + 4 * v;
      int n = VF_STEP * step + r;
      n = n < p.N ? n : p.N - 1;
      glds16(xb + (int64_t)n * D + ((lane ^ (r & 15)) << 3), base + r * 1024);
    }
  };
  stage(st_lo);
  if (nst > 1) stage(st_lo + 1);

  u32x4 wf[16][VF_NPL];
  {
    const u32x4* src =
        reinterpret_cast<const u32x4*>(p.duimg) + ((int64_t)b * 4 + wid) * 16 * VF_NPL * 64 + lane;
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int pl = 0; pl < VF_NPL; ++pl) wf[s][pl] = src[(s * VF_NPL + pl) * 64];
  }
  const f32x4 cd = *reinterpret_cast<const f32x4*>(p.cdu + b * K + 16 * wid + 4 * g);

  f32x4 accv[32];
#pragma unroll
  for (int ct = 0; ct < 32; ++ct) accv[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  unsigned rowoff[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) rowoff[k] = 1024u * i + 64u * (k ^ (i >> 2)) + 16u * (g ^ (i & 3));
  const int q = (lane >> 2) & 3, pp = lane & 3;
  unsigned troff[2], cfoff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int row = 16 * (g >> 1) + 2 * (4 * (g & 1) + q) + h;
    const int R = row & 15;
    troff[h] = 1024u * row + 32u * (R >> 1) + 16u * ((pp >> 1) ^ (R & 1)) + 8u * (pp & 1);
    cfoff[h] = (unsigned)row * VF_CFLD + 8u * pp;
  }

#pragma unroll 1
  for (int st = 0; st < nst; ++st) {
    const int step = st_lo + st;
    // younger than this stage's DMA and allowed in flight: the next stage's DMA (8) and the
    // previous step's three stores (its loads were waited for when they were used)
    vf_wait_vm((st + 1 < nst ? 8 : 0) + (st >= 1 ? 3 : 0));
    __builtin_amdgcn_s_barrier();
    const unsigned sb = lds0 + (unsigned)(st % VF_NST) * VF_STAGE;

    // the step's saved forward values, in flight under the matrix work
    f32x4 a4[2], l4[2];
    float rn2[2];
    bool ok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n = VF_STEP * step + 16 * t + i;
      ok[t] = n < p.N;
      const int64_t row = (int64_t)b * p.N + (ok[t] ? n : p.N - 1);
      a4[t] = *reinterpret_cast<const f32x4*>(p.a + row * K + 16 * wid + 4 * g);
      l4[t] = *reinterpret_cast<const f32x4*>(p.lg + row * K + 16 * wid + 4 * g);
      rn2[t] = p.rn[row];
    }

    f32x4 accl[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) accl[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 xf[4][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        xf[s][t] = vf_ldsr128(sb + rowoff[s & 3] + 256u * (s >> 2) + 16384u * t);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      if (s + 2 < 16) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
          xf[(s + 2) & 3][t] =
              vf_ldsr128(sb + rowoff[(s + 2) & 3] + 256u * ((s + 2) >> 2) + 16384u * t);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int pl = 0; pl < VF_NPL; ++pl) accl[t] = mfma16b(wf[s][pl], xf[s & 3][t], accl[t]);
    }

    float tv[2][4], dav[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float p1 = 0.f, p2 = 0.f, p3 = 0.f, p4 = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        tv[t][j] = accl[t][j] * rn2[t];                    // xhat . dU
        dav[t][j] = tv[t][j] + cd[j];
        const float ad = a4[t][j] * dav[t][j];
        p1 += ad;
        p2 = fmaf(a4[t][j], tv[t][j], p2);
        p3 = fmaf(ad, l4[t][j], p3);
        p4 = fmaf(a4[t][j], l4[t][j], p4);
      }
      p1 = vf_gsum(p1);
      p2 = vf_gsum(p2);
      p3 = vf_gsum(p3);
      p4 = vf_gsum(p4);
      if (g == 0) *reinterpret_cast<f32x4*>(exch + (wid * VF_STEP + 16 * t + i) * 4) = f32x4{p1, p2, p3, p4};
    }
    __builtin_amdgcn_s_barrier();
    float rd2[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int n = VF_STEP * step + 16 * t + i;
      f32x4 ps = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2)
        ps += *reinterpret_cast<const f32x4*>(exch + (w2 * VF_STEP + 16 * t + i) * 4);
      const float dot = ps[0];
      rd2[t] = ps[1] + ps[2] - dot * ps[3];
      float dsv[4];
      unsigned short h[3][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        dsv[j] = a4[t][j] * (dav[t][j] - dot);
        split3_bf16(ok[t] ? dsv[j] * rn2[t] : 0.f, h[0][j], h[1][j], h[2][j]);
      }
      *reinterpret_cast<f32x4*>(ok[t] ? p.ds + ((int64_t)b * p.N + n) * K + 16 * wid + 4 * g
                                      : p.trash + 4 * lane) = f32x4{dsv[0], dsv[1], dsv[2], dsv[3]};
#pragma unroll
      for (int pl = 0; pl < VF_NPL; ++pl)
        vf_ldsw64(cf0 + pl * VF_CFPL + (16 * t + i) * VF_CFLD + 8 * g,
                  (unsigned)h[pl][0] | ((unsigned)h[pl][1] << 16),
                  (unsigned)h[pl][2] | ((unsigned)h[pl][3] << 16));
    }
    {   // rowdot: wave w writes the step's locations 8 w .. 8 w + 7
      const int t = wid >> 1;
      const int n = VF_STEP * step + 16 * t + i;
      const float r = t == 0 ? rd2[0] : rd2[1];
      const bool mine = g == 0 && (i >> 3) == (wid & 1) && n < p.N;
      *(mine ? p.rowdot + (int64_t)b * p.N + n : p.trash + 4 * lane) = r;
    }
    if (st + 2 < nst) stage(step + 2);

    u32x4 bfr[VF_NPL];
#pragma unroll
    for (int pl = 0; pl < VF_NPL; ++pl) {
      const uint2 lo = lds_tr16_at(cf0 + pl * VF_CFPL + cfoff[0]);
      const uint2 hi = lds_tr16_at(cf0 + pl * VF_CFPL + cfoff[1]);
      bfr[pl] = u32x4{lo.x, lo.y, hi.x, hi.y};
    }
    // address of the transposed fragment of channel tile ct: (stage + troff[h]) ^ 32 ct touches
    // address bits 5..9 only, and (Rh ^ ct) = (ct & 24) | ((ct & 7) ^ Rh): eight per-lane bases
    // (ct & 7) per half, the rest is an immediate offset — no address arithmetic in the loop
    unsigned ta[2][8];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c7 = 0; c7 < 8; ++c7) ta[h][c7] = sb + (troff[h] ^ (32u * c7));
    // A fragments VF_AHEAD channel tiles ahead of the matrix work (an LDS round trip is several
    // times the MFMAs of a tile)
    u32x4 af[8];
#pragma unroll
    for (int ct = 0; ct < VF_AHEAD; ++ct) {
      const uint2 lo = lds_tr16_at(ta[0][ct & 7] + 32u * (ct & 24)), hi = lds_tr16_at(ta[1][ct & 7] + 32u * (ct & 24));
      af[ct] = u32x4{lo.x, lo.y, hi.x, hi.y};
    }
#pragma unroll
    for (int ct = 0; ct < 32; ++ct) {
      if (ct + VF_AHEAD < 32) {
        const int cn = ct + VF_AHEAD;
        const uint2 lo = lds_tr16_at(ta[0][cn & 7] + 32u * (cn & 24)),
                    hi = lds_tr16_at(ta[1][cn & 7] + 32u * (cn & 24));
        af[cn & 7] = u32x4{lo.x, lo.y, hi.x, hi.y};
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int pl = 0; pl < VF_NPL; ++pl) accv[ct] = mfma16b(af[ct & 7], bfr[pl], accv[ct]);
    }
  }

  f32x4* slab = reinterpret_cast<f32x4*>(p.slab) + ((((int64_t)sl * B + b) * 4 + wid) * 32) * 64 + lane;
#pragma unroll
  for (int ct = 0; ct < 32; ++ct) slab[ct * 64] = accv[ct];
}


constexpr int VW_GROUPS = kWgradGroups;   // BwdWs::wpartial holds this many group sums
// grad_w[d,k] = sum over all (slice, image) slabs, in two levels so that every CU reads its share
// of the 31 MB: vlad_wgrad_partial_kernel, grid (32 channel tiles, VW_GROUPS), sums one group's
// slabs (VF_MAXS loads in flight) into partial[group][...]; vlad_wgrad_finish_kernel, grid 32,
// adds the groups in order and forms grad_c[d,k] = sum_b dU[b,d,k] * asum[b,k].  Fixed orders
// throughout: bitwise reproducible.  Slabs in accumulator order (see vlad_finish_sum_kernel).

__global__ __launch_bounds__(256) void vlad_wgrad_partial_kernel(const float* __restrict__ slab,
                                                                 int total,
                                                                 float* __restrict__ partial) {
  const int ct = blockIdx.x, grp = blockIdx.y;
  const int per = (total + VW_GROUPS - 1) / VW_GROUPS;
  const int lo = grp * per, hi = lo + per < total ? lo + per : total;
  const int64_t unit = ((int64_t)(threadIdx.x >> 6) * 32 + ct) * 64 + (threadIdx.x & 63);
  const f32x4* src = reinterpret_cast<const f32x4*>(slab) + unit;
  const int64_t stride = (int64_t)4 * 32 * 64;                // units between (slice, image) slabs
  f32x4 u = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s0 = lo; s0 < hi; s0 += VF_MAXS) {
    f32x4 v[VF_MAXS];
#pragma unroll
    for (int s = 0; s < VF_MAXS; ++s)
      v[s] = s0 + s < hi ? src[(s0 + s) * stride] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < VF_MAXS; ++s) u += v[s];
  }
  reinterpret_cast<f32x4*>(partial)[grp * stride + unit] = u;
}

__global__ __launch_bounds__(256) void vlad_wgrad_finish_kernel(const float* __restrict__ partial,
                                                                const float* __restrict__ du,
                                                                const float* __restrict__ save_vlad,
                                                                int B, float* __restrict__ grad_w,
                                                                float* __restrict__ grad_c) {
  const int ct = blockIdx.x;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int k = 16 * w + i;
  const int64_t stride = (int64_t)4 * 32 * 64;
  const f32x4* src = reinterpret_cast<const f32x4*>(partial) + ((int64_t)w * 32 + ct) * 64 + lane;
  f32x4 v[VW_GROUPS];
#pragma unroll
  for (int s = 0; s < VW_GROUPS; ++s) v[s] = src[s * stride];
  f32x4 u = v[0];
#pragma unroll
  for (int s = 1; s < VW_GROUPS; ++s) u += v[s];
  float gc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < B; b0 += 8) {
    float as8[8], dv[8][4];
#pragma unroll
    for (int bb = 0; bb < 8; ++bb) {
      const int b = b0 + bb < B ? b0 + bb : B - 1;
      as8[bb] = b0 + bb < B ? save_vlad[((int64_t)b * VROWS + D) * K + k] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) dv[bb][j] = du[((int64_t)b * D + 16 * ct + 4 * g + j) * K + k];
    }
#pragma unroll
    for (int bb = 0; bb < 8; ++bb)
#pragma unroll
      for (int j = 0; j < 4; ++j) gc[j] = fmaf(dv[bb][j], as8[bb], gc[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int d = 16 * ct + 4 * g + j;
    grad_w[d * K + k] = u[j];
    grad_c[d * K + k] = gc[j];
  }
}

// bwd_dots_kernel: grid (8, B), block 256 (k = t & 63, dq = t >> 6): the four partial dots of
// one 64-channel block -> dots[b][blk][4][64].

__global__ __launch_bounds__(256) void bwd_dots_kernel(const float* __restrict__ save_vlad,
                                                       const float* __restrict__ grad_out,
                                                       const float* __restrict__ centers,
                                                       float* __restrict__ dots) {
  __shared__ float buf[4][4 * 64];
  const int blk = blockIdx.x, b = blockIdx.y, k = threadIdx.x & 63, dq = threadIdx.x >> 6;
  float sa = 0.f, sc = 0.f, sb = 0.f, sd = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int d = blk * 64 + dq * 16 + i;
    const float u = save_vlad[((int64_t)b * VROWS + d) * K + k];
    const float go = grad_out[(int64_t)b * D * K + d * K + k];
    const float c = centers[d * K + k];
    sa = fmaf(go, u, sa);
    sc = fmaf(u, u, sc);
    sb = fmaf(go, c, sb);
    sd = fmaf(u, c, sd);
  }
  buf[0][dq * 64 + k] = sa;
  buf[1][dq * 64 + k] = sc;
  buf[2][dq * 64 + k] = sb;
  buf[3][dq * 64 + k] = sd;
  __syncthreads();
  // wave dq finishes dot number dq
  const float* src = buf[dq];
  dots[(((int64_t)b * 8 + blk) * 4 + dq) * K + k] =
      (src[k] + src[64 + k]) + (src[128 + k] + src[192 + k]);
}


// bwd_du_kernel: grid (8, B), block 256: dU of one 64-channel block as float32 [d][k] (and
// transposed, for the float32-MFMA row-tile kernel), c.dU from block 0, and for bf16 feature maps
// the two REGISTER IMAGES the fused kernels load with coalesced 16-byte reads:
//   duimg  (vlad_bwd_kernel): unit ((w * 16 + s) * VF_NPL + plane) * 64 + lane =
//          dU_plane[ch 32 s + 8 g + e][cluster 16 w + i] — eight consecutive CHANNELS of a
//          cluster: what this thread holds in registers;
//   dximg  (vlad_dx_kernel):  unit (((w * 8 + nt) * 2 + s) * 2 + plane) * 64 + lane =
//          dU_plane[ch 128 w + 16 nt + i][cluster 32 s + 8 g + e] — eight consecutive CLUSTERS
//          of a channel: the other orientation, through a [64 ch][64 k] LDS tile;
//   wdximg (image 0's workgroups): the same image of W, shared by all images.
constexpr int DU_TLD = 65;                                // floats per tile row (conflict-free columns)
__global__ __launch_bounds__(256) void bwd_du_kernel(const float* __restrict__ save_vlad,
                                                     const float* __restrict__ grad_out,
                                                     const float* __restrict__ dots,
                                                     float* __restrict__ du,
                                                     float* __restrict__ dut,
                                                     unsigned short* __restrict__ duimg,
                                                     unsigned short* __restrict__ dximg,
                                                     const float* __restrict__ assign_w,
                                                     unsigned short* __restrict__ wdximg,
                                                     float* __restrict__ cdu) {
  __shared__ float tile[64 * DU_TLD];
  const int blk = blockIdx.x, b = blockIdx.y, k = threadIdx.x & 63, dq = threadIdx.x >> 6;
  float dot[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float s = 0.f;
#pragma unroll
    for (int bl = 0; bl < 8; ++bl) s += dots[(((int64_t)b * 8 + bl) * 4 + j) * K + k];
    dot[j] = s;
  }
  const float ak = dot[0], col = dot[1], bk = dot[2], dk = dot[3];
  const float q = 1.0f / sqrtf(col + 1e-12f);
  const float tot = wave_sum(q * q * col);
  const float g = 1.0f / sqrtf(tot + 1e-12f);
  const float s1 = wave_sum(q * ak);
  const float r = g * (q * ak - g * g * s1 * q * q * col);
  const float cu = q * q * (g * g * g * s1 + r);   // coefficient of U
  const float cg = q * g;                          // coefficient of go
  float vals[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int d = blk * 64 + dq * 16 + i;
    const float u = save_vlad[((int64_t)b * VROWS + d) * K + k];
    const float go = grad_out[(int64_t)b * D * K + d * K + k];
    vals[i] = cg * go - cu * u;
    du[((int64_t)b * D + d) * K + k] = vals[i];
  }
  if (blk == 0 && dq == 0) cdu[b * K + k] = cg * bk - cu * dk;
  if (dut) {   // transposed float32 copy (float32-MFMA row-tile kernel only)
    float* trow = dut + ((int64_t)b * K + k) * D + blk * 64 + dq * 16;
#pragma unroll
    for (int i = 0; i < 16; i += 4)
      *reinterpret_cast<f32x4*>(trow + i) = f32x4{vals[i], vals[i + 1], vals[i + 2], vals[i + 3]};
  }
  if (!duimg) return;                                      // (uniform over the launch)
  {
    // this thread's 16 channels are k-step s = 2 blk + (dq >> 1), lane groups g = 2 (dq & 1) and
    // + 1, of wave k >> 4
    unsigned short h[3][16];
#pragma unroll
    for (int i = 0; i < 16; ++i) split3_bf16(vals[i], h[0][i], h[1][i], h[2][i]);
    uint4* img = reinterpret_cast<uint4*>(duimg + (int64_t)b * VF_NPL * D * K);
    const int wv = k >> 4, ii = k & 15, s = 2 * blk + (dq >> 1);
#pragma unroll
    for (int pl = 0; pl < VF_NPL; ++pl) {
      unsigned w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        w[i] = (unsigned)h[pl][2 * i] | ((unsigned)h[pl][2 * i + 1] << 16);
      const int g0 = 2 * (dq & 1);
      img[((wv * 16 + s) * VF_NPL + pl) * 64 + 16 * g0 + ii] = make_uint4(w[0], w[1], w[2], w[3]);
      img[((wv * 16 + s) * VF_NPL + pl) * 64 + 16 * (g0 + 1) + ii] = make_uint4(w[4], w[5], w[6], w[7]);
    }
  }
  // the other orientation through LDS: tile[channel of the block][cluster]
#pragma unroll
  for (int i = 0; i < 16; ++i) tile[(dq * 16 + i) * DU_TLD + k] = vals[i];
  __syncthreads();
  const int wv = blk >> 1;                                  // the block's channels: wave wv, tiles 4 (blk & 1) ..
#pragma unroll
  for (int rep = 0; rep < 2; ++rep) {
    const int u = threadIdx.x + 256 * rep;                  // 512 units: (tile nt', k-step s, lane)
    const int ntl = u >> 7, s = (u >> 6) & 1, lane = u & 63, i = lane & 15, gq = lane >> 4;
    const float* row = &tile[(16 * ntl + i) * DU_TLD + 32 * s + 8 * gq];
    const f32x4 v0{row[0], row[1], row[2], row[3]}, v1{row[4], row[5], row[6], row[7]};
    u32x4 hi, lo;
    split2x8(v0, v1, hi, lo);
    u32x4* img = reinterpret_cast<u32x4*>(dximg) + (int64_t)b * (4 * 8 * 2 * 2 * 64) +
                 (((wv * 8 + 4 * (blk & 1) + ntl) * 2 + s) * 2) * 64 + lane;
    img[0] = hi;
    img[64] = lo;
    if (b == 0) {                                           // W in the same orientation
      const float* wr = assign_w + (int64_t)(64 * blk + 16 * ntl + i) * K + 32 * s + 8 * gq;
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(wr), w1 = *reinterpret_cast<const f32x4*>(wr + 4);
      split2x8(w0, w1, hi, lo);
      u32x4* wimg = reinterpret_cast<u32x4*>(wdximg) +
                    (((wv * 8 + 4 * (blk & 1) + ntl) * 2 + s) * 2) * 64 + lane;
      wimg[0] = hi;
      wimg[64] = lo;
    }
  }
}

template <typename T, int VAR>
void launch_variant_one(const RowTileArgs& a, hipStream_t st) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rowtile16_kernel<T, ASSIGN, VAR>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRowTile16Lds);
  const dim3 grid(((a.N + 15) / 16 + 3) / 4, a.B);
  SCL_LAUNCH("rowtile16_kernel<ASSIGN>", (rowtile16_kernel<T, ASSIGN, VAR>), grid, dim3(256), kRowTile16Lds,
             st, a);
}
// the ablated stand-in for launch_rowtile<T, ASSIGN> (vlad_f32_forward's launcher parameter)
template <typename T>
void launch_rowtile_variant(const RowTileArgs& a, hipStream_t st) {
  switch (scl_variant() & 7) {
    case 1: launch_variant_one<T, 1>(a, st); break;
    case 2: launch_variant_one<T, 2>(a, st); break;
    case 3: launch_variant_one<T, 3>(a, st); break;
    case 4: launch_variant_one<T, 4>(a, st); break;
    case 5: launch_variant_one<T, 5>(a, st); break;
    case 6: launch_variant_one<T, 6>(a, st); break;
    default: launch_variant_one<T, 7>(a, st); break;
  }
}

}  // namespace

// scl_debug_set_variant(920): round 3's launch structure
inline bool old_launches() { return scl_variant() == 920; }
// scl_debug_set_variant(922): the four-wave fused kernels of round 3 instead of the eight-wave ones
inline bool four_waves() { return scl_variant() == 922 || scl_variant() == 920 || scl_variant() == 916; }

static bool netvlad_fwd_diag(const void* x, int x_dtype, const float* assign_w, const float* centers,
                             const void* w_planes, int B, int N, int pre_l2, float* out, float* save_assign,
                             float* save_logit, float* save_rnorm, float* save_vlad, const FwdWs& w,
                             const VladPlan& pl_call, hipStream_t st, int* rc) {
  const int v = scl_variant();
  const bool bf16 = x_dtype == SCL_DT_BF16;
  if (v >= 1 && v <= 7) {
    // the float32-MFMA forward with an ablated row-tile kernel, whatever the map's type
    *rc = bf16 ? vlad_f32_forward<unsigned short>(x, assign_w, centers, B, N, pre_l2, out, save_assign, save_logit,
                                                  save_rnorm, save_vlad, w, st, launch_rowtile_variant<unsigned short>)
               : vlad_f32_forward<float>(x, assign_w, centers, B, N, pre_l2, out, save_assign, save_logit,
                                         save_rnorm, save_vlad, w, st, launch_rowtile_variant<float>);
    return true;
  }
  if (v == 8 && bf16) {   // a bf16 map through the plain float32-MFMA kernels (A/B timing and parity runs)
    *rc = vlad_f32_forward<unsigned short>(x, assign_w, centers, B, N, pre_l2, out, save_assign, save_logit,
                                           save_rnorm, save_vlad, w, st);
    return true;
  }
  // (the four-wave kernels write and read logits; variant 918 without saving runs the product kernels)
  const bool save = save_assign && save_rnorm && (save_logit || !four_waves());
  if (!bf16 || !(four_waves() || (v == 918 && save))) return false;
  static SclDeviceOnce once;
  scl_call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_fwd_kernel<true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVladFusedLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_fwd_kernel<false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVladFusedLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_fwd8_kernel<true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVlad8Lds);
  });
  // always the sliced form: the four-wave kernels have no finish in their tail (pl_call.fin)
  const VladPlan pl = pl_call.fin ? vlad_plan(B, N, VLAD_TRAIN) : pl_call;
  const unsigned short* planes = w.wplanes;
  if (old_launches())
    SCL_LAUNCH("vlad_split_w_kernel", vlad_split_w_kernel, dim3(64, VF_WREP), dim3(64), 0, st, assign_w,
               w.wplanes);
  else
    planes = vlad_w_planes(w_planes, assign_w, w.wplanes, st);
  VladFwdArgs fa = vlad_fwd_args(x, planes, N, pre_l2, save, save_assign, save_logit, save_rnorm, w, pl);
  if (v == 916) fa.dbg = 16;   // scripts/vlad_stamps.py (918: the plan's)
  if (!four_waves())
    SCL_LAUNCH("vlad_fwd8_kernel<stamps>", (vlad_fwd8_kernel<true, true>), dim3(B, pl.S), dim3(512), kVlad8Lds,
               st, fa);
  else if (save)
    SCL_LAUNCH("vlad_fwd_kernel<true>", vlad_fwd_kernel<true>, dim3(B, pl.S), dim3(256), kVladFusedLds, st, fa);
  else
    SCL_LAUNCH("vlad_fwd_kernel<false>", vlad_fwd_kernel<false>, dim3(B, pl.S), dim3(256), kVladFusedLds, st,
               fa);
  if (old_launches()) {
    float* vlad = save_vlad ? save_vlad : w.vlad;
    SCL_LAUNCH("vlad_finish_sum_kernel", vlad_finish_sum_kernel, dim3(B, 32), dim3(256), 0, st,
               (const float*)w.part, (const float*)w.colsum, centers, pl.S, vlad, w.colsq);
    SCL_LAUNCH("finish_norm_kernel", finish_norm_kernel, dim3(8, B), dim3(256), 0, st, vlad,
               (const float*)w.colsq, 32, out);
  } else {
    launch_vlad_finish(centers, B, out, save_vlad, w, pl, st);
  }
  *rc = scl_launch_status();
  return true;
}

static bool netvlad_bwd_diag(const void* x, int x_dtype, const float* assign_w, const float* centers,
                             const void* w_planes, const float* grad_out, const float* save_assign,
                             const float* save_logit, const float* save_rnorm, float* save_vlad, int B, int N,
                             int pre_l2, void* grad_x, float* grad_w, float* grad_c, const BwdWs& w,
                             const VladPlan& pl, hipStream_t st, int* rc) {
  const int v = scl_variant();
  const bool bf16 = x_dtype == SCL_DT_BF16;
  if (v >= 1 && v <= 8) {
    if (!bf16) return false;             // a float32 map: the product route is the float32-MFMA one
    // a bf16 map through the plain float32-MFMA kernels, which read the saved logits
    *rc = save_logit ? vlad_f32_backward<unsigned short>(x, assign_w, centers, grad_out, save_assign, save_logit,
                                                         save_rnorm, save_vlad, B, N, pre_l2, grad_x, grad_w,
                                                         grad_c, w, pl, st)
                     : SCL_E_NULL;
    return true;
  }
  if (!four_waves() || (!bf16 && !old_launches())) return false;
  if (!save_logit) {                     // the four-wave kernels read the saved logits
    *rc = SCL_E_NULL;
    return true;
  }
  const unsigned short* wdx = w.wdximg;
  if (old_launches()) {
    SCL_LAUNCH("bwd_dots_kernel", bwd_dots_kernel, dim3(8, B), dim3(256), 0, st, (const float*)save_vlad,
               grad_out, centers, w.dots);
    SCL_LAUNCH("bwd_du_kernel", bwd_du_kernel, dim3(8, B), dim3(256), 0, st, (const float*)save_vlad,
               grad_out, (const float*)w.dots, w.du, bf16 ? (float*)nullptr : w.dut,
               bf16 ? w.duimg : (unsigned short*)nullptr, w.dximg, assign_w, w.wdximg, w.cdu);
  } else {
    wdx = vlad_w_planes(w_planes, assign_w, w.wdximg, st) + VP_FWD_ELEMS;
    launch_bwd_prologue(grad_out, centers, save_vlad, B, true, w, pl, st);
  }
  if (!bf16) {                           // variant 920, float32 feature maps: the row-tile route
    *rc = vlad_f32_grads<float>(x, assign_w, save_assign, save_logit, save_rnorm, save_vlad, B, N, pre_l2, grad_x,
                                grad_w, grad_c, w, st);
    return true;
  }
  static SclDeviceOnce once;
  scl_call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_bwd_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVladFusedLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_dx_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVladDxLds);
  });
  const VladBwdArgs ba = vlad_bwd_args(x, save_assign, save_logit, save_rnorm, N, w, pl);
  SCL_LAUNCH("vlad_bwd_kernel", vlad_bwd_kernel, dim3(B, pl.S), dim3(256), kVladFusedLds, st, ba);
  VladDxArgs da =
      vlad_dx_args(x, wdx, save_assign, save_rnorm, save_vlad, B, N, pre_l2, grad_x, grad_w, grad_c, w, pl);
  if (old_launches()) da.wslab = nullptr;   // no tail: the two kernels below sum the slabs
  SCL_LAUNCH("vlad_dx_kernel", vlad_dx_kernel, dim3(B, pl.S), dim3(256), kVladDxLds, st, da);
  if (old_launches()) {
    SCL_LAUNCH("vlad_wgrad_partial_kernel", vlad_wgrad_partial_kernel, dim3(32, VW_GROUPS), dim3(256), 0, st,
               (const float*)w.wpart, pl.S * B, w.wpartial);
    SCL_LAUNCH("vlad_wgrad_finish_kernel", vlad_wgrad_finish_kernel, dim3(32), dim3(256), 0, st,
               (const float*)w.wpartial, (const float*)w.du, (const float*)save_vlad, B, grad_w, grad_c);
  }
  *rc = scl_launch_status();
  return true;
}
