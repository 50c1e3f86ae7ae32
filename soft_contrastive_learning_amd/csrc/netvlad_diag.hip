// NetVLAD head, DIAGNOSTIC BUILD ONLY (csrc/Makefile: libscl_hip_diag.so, -DSCL_DIAG): the kernels
// and launch structures the product dispatch in netvlad.hip no longer takes, reachable through
// scl_debug_set_variant for same-box A/B timing, ablations and parity runs.
//   1 .. 7   rowtile16_kernel<ASSIGN> ablations (scripts/ablate_rowtile.py; results meaningless)
//   916, 922 round 3's four-wave fused kernels vlad_fwd_kernel / vlad_bwd_kernel (916: clock stamps)
//   918      vlad_fwd8_kernel with clock stamps when it saves (scripts/vlad_stamps.py)
//   920      round 3's launch structure: separate plane split, finish_sum, finish_norm, bwd_dots,
//            bwd_du, wgrad_partial and wgrad_finish kernels around the four-wave kernels
// netvlad.hip calls netvlad_fwd_diag / netvlad_bwd_diag after its argument checks; they return
// false for every other variant, and the product dispatch runs.
#include "netvlad.hip"

namespace {

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
void launch_variant_one(const RowTileArgs& a, dim3 grid, hipStream_t st) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rowtile16_kernel<T, ASSIGN, VAR>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRowTile16Lds);
  SCL_LAUNCH("rowtile16_kernel<ASSIGN>", (rowtile16_kernel<T, ASSIGN, VAR>), grid, dim3(256), kRowTile16Lds,
             st, a);
}
template <typename T>
void launch_rowtile_variant(const RowTileArgs& a, dim3 grid, hipStream_t st) {
  switch (scl_variant() & 7) {
    case 1: launch_variant_one<T, 1>(a, grid, st); break;
    case 2: launch_variant_one<T, 2>(a, grid, st); break;
    case 3: launch_variant_one<T, 3>(a, grid, st); break;
    case 4: launch_variant_one<T, 4>(a, grid, st); break;
    case 5: launch_variant_one<T, 5>(a, grid, st); break;
    case 6: launch_variant_one<T, 6>(a, grid, st); break;
    default: launch_variant_one<T, 7>(a, grid, st); break;
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
                             hipStream_t st, int* rc) {
  const int v = scl_variant();
  if (v >= 1 && v <= 7) {
    // the float32-MFMA route of netvlad.hip with an ablated row-tile kernel
    float* assign = save_assign ? save_assign : w.assign;
    float* rnorm = save_rnorm ? save_rnorm : w.rnorm;
    SCL_LAUNCH("transpose_w_kernel", transpose_w_kernel, dim3(D * K / 256), dim3(256), 0, st, assign_w,
               w.wt);
    RowTileArgs a{};
    a.x = x;
    a.bt = w.wt;
    a.bt_stride = 0;
    a.B = B;
    a.N = N;
    a.pre_l2 = pre_l2 ? 1 : 0;
    a.assign = assign;
    a.logit = save_logit;
    a.rnorm = rnorm;
    const dim3 grid(((N + 15) / 16 + 3) / 4, B);
    if (x_dtype == SCL_DT_F32) {
      launch_rowtile_variant<float>(a, grid, st);
      SCL_LAUNCH("aggregate_kernel<float>", aggregate_kernel<float>, dim3(D / 64, NSPLIT, B), dim3(256), 0,
                 st, x, (const float*)assign, (const float*)rnorm, N, w.part, w.colsum);
    } else {
      launch_rowtile_variant<unsigned short>(a, grid, st);
      SCL_LAUNCH("aggregate_kernel<bf16>", aggregate_kernel<unsigned short>, dim3(D / 64, NSPLIT, B),
                 dim3(256), 0, st, x, (const float*)assign, (const float*)rnorm, N, w.part, w.colsum);
    }
    float* vlad = save_vlad ? save_vlad : w.vlad;
    SCL_LAUNCH("finish_sum_kernel", finish_sum_kernel, dim3(8, B), dim3(256), 0, st,
               (const float*)w.part, (const float*)w.colsum, centers, vlad, w.colsq);
    SCL_LAUNCH("finish_norm_kernel", finish_norm_kernel, dim3(8, B), dim3(256), 0, st, vlad,
               (const float*)w.colsq, 8, out);
    *rc = scl_launch_status();
    return true;
  }
  // (the four-wave kernels write and read logits; variant 918 without saving runs the product kernels)
  const bool save = save_assign && save_rnorm && (save_logit || !four_waves());
  if (x_dtype != SCL_DT_BF16 || !(four_waves() || (v == 918 && save))) return false;
  static SclDeviceOnce once;
  scl_call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_fwd_kernel<true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVladFusedLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_fwd_kernel<false>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVladFusedLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_fwd8_kernel<true, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVlad8Lds);
  });
  const VladPlan pl = vlad_plan(B, N);
  const unsigned short* planes = (const unsigned short*)w_planes;
  if (old_launches()) {
    SCL_LAUNCH("vlad_split_w_kernel", vlad_split_w_kernel, dim3(64, VF_WREP), dim3(64), 0, st, assign_w,
               w.wplanes);
    planes = w.wplanes;
  } else if (!planes) {
    SCL_LAUNCH("vlad_planes_kernel", vlad_planes_kernel, dim3(VP_WAVES / 4), dim3(256), 0, st, assign_w,
               w.wplanes);
    planes = w.wplanes;
  }
  VladFwdArgs fa{};
  fa.x = (const unsigned short*)x;
  fa.wimg = planes;
  fa.N = N;
  fa.pre_l2 = pre_l2 ? 1 : 0;
  fa.steps_per_slice = pl.steps_per_slice;
  fa.slab = w.part;
  fa.colsum = w.colsum;
  fa.trash = w.trash;
  fa.gran = w.gran;
  fa.dbg = (v == 916 || v == 918) ? 16 : 0;   // scripts/vlad_stamps.py
  fa.stamps = w.stamps;
  if (save) {
    fa.assign = save_assign;
    fa.logit = save_logit;
    fa.rnorm = save_rnorm;
  }
  if (!four_waves())
    SCL_LAUNCH("vlad_fwd8_kernel<stamps>", (vlad_fwd8_kernel<true, true>), dim3(B, pl.S), dim3(512), kVlad8Lds,
               st, fa);
  else if (save)
    SCL_LAUNCH("vlad_fwd_kernel<true>", vlad_fwd_kernel<true>, dim3(B, pl.S), dim3(256), kVladFusedLds, st, fa);
  else
    SCL_LAUNCH("vlad_fwd_kernel<false>", vlad_fwd_kernel<false>, dim3(B, pl.S), dim3(256), kVladFusedLds, st,
               fa);
  float* vlad = save_vlad ? save_vlad : w.vlad;
  if (old_launches()) {
    SCL_LAUNCH("vlad_finish_sum_kernel", vlad_finish_sum_kernel, dim3(B, 32), dim3(256), 0, st,
               (const float*)w.part, (const float*)w.colsum, centers, pl.S, vlad, w.colsq);
    SCL_LAUNCH("finish_norm_kernel", finish_norm_kernel, dim3(8, B), dim3(256), 0, st, vlad,
               (const float*)w.colsq, 32, out);
  } else {
    VladFinishArgs na{};
    na.slab = w.part;
    na.colsum = w.colsum;
    na.centers = centers;
    na.S = pl.S;
    na.B = B;
    na.vlad = vlad;
    na.out = out;
    na.gran = w.gran;
    na.spin_limit = spin_limit();
    SCL_LAUNCH("vlad_finish_kernel", vlad_finish_kernel, dim3(8, B), dim3(256), 0, st, na);
  }
  *rc = scl_launch_status();
  return true;
}

static bool netvlad_bwd_diag(const void* x, int x_dtype, const float* assign_w, const float* centers,
                             const void* w_planes, const float* grad_out, const float* save_assign,
                             const float* save_logit, const float* save_rnorm, float* save_vlad, int B, int N,
                             int pre_l2, void* grad_x, float* grad_w, float* grad_c, const BwdWs& w,
                             hipStream_t st, int* rc) {
  const bool fused = x_dtype == SCL_DT_BF16 && use_fused();
  if (!four_waves() || (!fused && !old_launches())) return false;
  if (!save_logit) {                     // the four-wave kernels read the saved logits
    *rc = SCL_E_NULL;
    return true;
  }
  const unsigned short* wdx = w_planes ? (const unsigned short*)w_planes + VP_FWD_ELEMS : nullptr;
  if (old_launches()) {
    SCL_LAUNCH("bwd_dots_kernel", bwd_dots_kernel, dim3(8, B), dim3(256), 0, st, (const float*)save_vlad,
               grad_out, centers, w.dots);
    SCL_LAUNCH("bwd_du_kernel", bwd_du_kernel, dim3(8, B), dim3(256), 0, st, (const float*)save_vlad,
               grad_out, (const float*)w.dots, w.du, fused ? (float*)nullptr : w.dut,
               fused ? w.duimg : (unsigned short*)nullptr, w.dximg, assign_w, w.wdximg, w.cdu);
    wdx = w.wdximg;
  } else {
    if (!wdx) {
      SCL_LAUNCH("vlad_planes_kernel", vlad_planes_kernel, dim3(VP_WAVES / 4), dim3(256), 0, st, assign_w,
                 w.wdximg);
      wdx = w.wdximg + VP_FWD_ELEMS;
    }
    VladProArgs pa{};
    pa.save_vlad = save_vlad;
    pa.grad_out = grad_out;
    pa.centers = centers;
    pa.du = w.du;
    pa.dut = nullptr;
    pa.duimg = w.duimg;
    pa.dximg = w.dximg;
    pa.cdu = w.cdu;
    pa.spin_limit = spin_limit();
    SCL_LAUNCH("vlad_bwd_prologue_kernel", vlad_bwd_prologue_kernel, dim3(8, B), dim3(256), 0, st, pa);
  }
  if (!fused) {                          // variant 920, float32 feature maps: the row-tile route
    RowTileArgs a{};
    a.x = x;
    a.bt = w.dut;
    a.bt_stride = (int64_t)D * K;
    a.B = B;
    a.N = N;
    a.pre_l2 = pre_l2 ? 1 : 0;
    a.a_in = save_assign;
    a.logit_in = save_logit;
    a.rn_in = save_rnorm;
    a.cdu = w.cdu;
    a.ds = w.ds;
    a.rowdot = w.rowdot;
    const dim3 dxgrid(((N + 15) / 16 + 3) / 4, B);
    if (x_dtype == SCL_DT_F32) {
      launch_rowtile<float, DASSIGN>(a, st);
      SCL_LAUNCH("aggregate_kernel<float>", aggregate_kernel<float>, dim3(D / 64, NSPLIT, B), dim3(256), 0,
                 st, x, (const float*)w.ds, save_rnorm, N, w.wpart, (float*)nullptr);
      SCL_LAUNCH("dx16_kernel<float>", dx16_kernel<float>, dxgrid, dim3(256), kDx16Lds, st, x, save_assign,
                 (const float*)w.ds, save_rnorm, (const float*)w.rowdot, (const float*)w.du, assign_w,
                 N, pre_l2 ? 1 : 0, grad_x);
    } else {
      launch_rowtile<unsigned short, DASSIGN>(a, st);
      SCL_LAUNCH("aggregate_kernel<bf16>", aggregate_kernel<unsigned short>, dim3(D / 64, NSPLIT, B),
                 dim3(256), 0, st, x, (const float*)w.ds, save_rnorm, N, w.wpart, (float*)nullptr);
      SCL_LAUNCH("dx16_kernel<bf16>", dx16_kernel<unsigned short>, dxgrid, dim3(256), kDx16Lds, st, x,
                 save_assign, (const float*)w.ds, save_rnorm, (const float*)w.rowdot,
                 (const float*)w.du, assign_w, N, pre_l2 ? 1 : 0, grad_x);
    }
    SCL_LAUNCH("wgrad_finish_kernel", wgrad_finish_kernel, dim3(D * K / 64), dim3(256), 0, st,
               (const float*)w.wpart, (const float*)w.du, save_vlad, B, grad_w, grad_c);
    *rc = scl_launch_status();
    return true;
  }
  static SclDeviceOnce once;
  scl_call_once(once, [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_bwd_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVladFusedLds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vlad_dx_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVladDxLds);
  });
  const VladPlan pl = vlad_plan(B, N);
  VladBwdArgs ba{};
  ba.x = (const unsigned short*)x;
  ba.duimg = w.duimg;
  ba.a = save_assign;
  ba.lg = save_logit;
  ba.rn = save_rnorm;
  ba.cdu = w.cdu;
  ba.N = N;
  ba.steps_per_slice = pl.steps_per_slice;
  ba.ds = w.ds;
  ba.rowdot = w.rowdot;
  ba.slab = w.wpart;
  ba.trash = w.trash;
  SCL_LAUNCH("vlad_bwd_kernel", vlad_bwd_kernel, dim3(B, pl.S), dim3(256), kVladFusedLds, st, ba);
  VladDxArgs da{};
  da.x = (const unsigned short*)x;
  da.a = save_assign;
  da.ds = w.ds;
  da.rn = save_rnorm;
  da.rowdot = w.rowdot;
  da.dximg = w.dximg;
  da.wdximg = wdx;
  da.N = N;
  da.pre_l2 = pre_l2 ? 1 : 0;
  da.steps_per_slice = pl.steps_per_slice;
  da.gx = (unsigned short*)grad_x;
  da.trash = (unsigned short*)w.trash;
  da.stamps = w.stamps;
  if (!old_launches()) {                 // the parameter gradients ride in the tail of this launch
    da.wslab = w.wpart;
    da.nslab = pl.S * B;
    da.du = w.du;
    da.save_vlad = save_vlad;
    da.B = B;
    da.grad_w = grad_w;
    da.grad_c = grad_c;
  }
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
