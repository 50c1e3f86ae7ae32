// 3x3 / stride 1 / same-padding convolution for the deeper VGG16 layers (128 .. 512
// channels, model/nets.py:44-63) on bf16 channels-last activations: forward and, with the
// weights transposed and the taps flipped, backward-data.  The register-resident-weights
// kernel of conv64.hip does not scale past 128 channels; here the weights stream through LDS.
// Kernel (32x32x16 MFMA), pack kernel and launcher; conv_lds.hip owns the entry points, validates and
// chooses: this kernel where cin % 64 != 0, or pinned by scl_debug_set_variant(40000 + v).
//
// Implicit GEMM on v_mfma_f32_32x32x16_bf16 with a large M tile so that a staged weight chunk
// is reused by many pixels:
//   * workgroup = [12 rows x 40 cols] of output pixels (15 m-tiles of 4 x 8 pixels; 40
//     divides the widths 160 / 80 / 40 of conv3_x .. conv5_x) x 128 output channels; eight
//     waves, wave (mg, ng) owns 4 of the m-tiles x 64 of the channels: 128 accumulators, two
//     waves per SIMD, 6 LDS fragment reads per 8 MFMAs;
//   * K loop over (32-channel chunk, tap): the [14][42][32 ch] halo window of the chunk is
//     staged once per chunk, the [128 k][32 c] weight slice once per (chunk, tap), both
//     double-buffered in LDS behind register prefetches; one barrier per TWO (chunk, tap)
//     steps = per 60 MFMAs per wave;
//   * A fragment = 16 bytes (8 channels of one window pixel) at a per-tap address offset —
//     no im2col; B fragment = 16 bytes of a weight row.
//   * epilogue as conv64.hip: bf16 through a per-wave LDS transpose, optional bias (+ ReLU).
#include <mutex>

#include "conv_lds.h"
#include "conv_pack_layout.h"

namespace {

constexpr int BW = 40;                              // output block width (block height: GCfg)
constexpr int GWC = BW + 4;                         // halo window: 42 columns used, 44 staged —
                                                    // with 80-byte pixels and the lane -> pixel
                                                    // map below every ds_read_b128 service group
                                                    // of an A fragment hits 16 different slots
constexpr int CCH = 32;                             // channels per staged chunk
constexpr int GPIX = CCH + 8;                       // bf16 per staged pixel / weight row (80 B)
static_assert(CCH == 32 && GPIX == LDS_CONV_ROW, "scl_convg_workspace_bytes sizes this image");
constexpr int NTHR = 512;                           // 8 waves: two per SIMD
constexpr int NB = 128;                             // output channels per workgroup
constexpr int GWT = NB * GPIX;                      // bf16 per weight buffer (5120)
constexpr int GSCR_LD = 40;
constexpr int GSCR = 32 * GSCR_LD;
constexpr int TPB = 3;                              // (chunk, tap) steps per barrier: one
                                                    // tap row of a chunk
// two windows + two weight buffers; the epilogue's per-wave scratch reuses the windows
// Block height 12 (15 m-tiles of 4 x 8 pixels; wave = 4 m-tile slots x 2 n-tiles) or 8 (10
// m-tiles; wave = one tile row of 5 x 1 n-tile) — the lower block for maps whose few 12-row
// blocks leave CUs idle (30 x 40: 288 workgroups on 256 CUs -> 384 smaller ones).
template <int BHv>
struct GCfg {
  static constexpr int BH = BHv;
  static constexpr int GWR = BH + 2;
  static constexpr int GWIN = GWR * GWC * GPIX;       // bf16 per window buffer
  static constexpr int NMT = BH / 4 * 5;              // m-tiles
  static constexpr int MS = BH == 12 ? 4 : 5;         // m-tile slots per wave
  static constexpr int NS = BH == 12 ? 2 : 1;         // 32-channel n-tiles per wave
  static constexpr int GSLOTS = GWR * GWC * 5;        // 16-byte slots of a window (4 data + pad)
  static constexpr int GCHUNKS = (GSLOTS + 63) / 64;  // 1-KB DMA chunks per window
  static constexpr int GNI = (GCHUNKS + 7) / 8;       // per wave
  // two windows + two weight buffers; the epilogue's per-wave scratch reuses the windows
  static constexpr size_t LDS = (2 * (size_t)GWIN + 2 * TPB * (size_t)GWT) * 2;
  static_assert(8 * GSCR <= GWIN, "epilogue scratch must fit ONE window buffer");
};

// Lane -> pixel of a 4 x 8 m-tile.  The hardware serves a ds_read_b128 in the lane groups
// {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (per 32-lane half); giving the first group the
// tile rows 0 and 2 and the second the rows 1 and 3 makes (row * 44 + col) * 5 cover all 16
// 16-byte slots within each group (PMC: SQ_LDS_BANK_CONFLICT was 58 % of the LDS cycles with
// the plain row-major map).
__device__ __forceinline__ int tile_row(int l) {
  return l < 4 ? 0 : l < 12 ? 1 : l < 16 ? 0 : l < 20 ? 3 : l < 28 ? 2 : 3;
}
__device__ __forceinline__ int tile_col(int l) {
  return l < 4 ? l : l < 12 ? l - 4 : l < 16 ? l - 8 : l < 20 ? l - 16 : l < 28 ? l - 20 : l - 24;
}

// Weights -> [n-block][chunk][tap][k 128][c 32 + 8 pad] bf16: the exact LDS image of a step
// (10 KB slices in the order the kernel stages them, copied by LDS-DMA as they are).
// Forward / transposed: pack_src_offset (conv_pack_layout.h).
__global__ __launch_bounds__(256) void convg_pack_kernel(const void* __restrict__ w,
                                                         int64_t sk, int64_t sc, int64_t sh,
                                                         int64_t sw, int flags, int cin,
                                                         int kout,
                                                         unsigned short* __restrict__ packed) {
  const int transposed = flags & 1, wf32 = flags & 2;   // SCL_CONV_TRANSPOSED | SCL_W_F32
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)9 * (cin / CCH) * kout * GPIX;
  if (idx >= total) return;
  const int c = idx % GPIX, k = (idx / GPIX) & 127;
  const int64_t rest = idx / (GPIX * 128);           // (nb * CC + cc) * 9 + tap
  const int tap = rest % 9;
  const int cc = (rest / 9) % (cin / CCH), nb = rest / 9 / (cin / CCH);
  if (c >= CCH) {
    packed[idx] = 0;
    return;
  }
  const int64_t off = pack_src_offset(PackCoord{NB * nb + k, CCH * cc + c, tap}, sk, sc, sh, sw, transposed);
  packed[idx] = weight_bf16(w, off, wf32);
}

// Staging is LDS-DMA (glds16, scl_cdna4.h); the kernel counts vmcnt itself.
constexpr int WCHK = TPB * GWT * 2 / 1024;           // chunks per weight step group (30)

// grid (pixel blocks, kout / 128); block 512.  EPI: 0 plain, 1 + bias (+ ReLU),
// 2 out = conv * [mask > 0] (the ReLU' of the layer below, for backward-data),
// 3 out = relu(maxpool2x2(conv) + bias) [B,H/2,W/2,kout] and pidx = the window position of each
//   maximum (one byte), no full-size output (conv3_3 / conv4_3 forward).
template <int EPI, int BHv>
__global__ __launch_bounds__(NTHR, 1) void convg_kernel(const unsigned short* __restrict__ x,
                                                       const unsigned short* __restrict__ packed,
                                                       int B, int H, int W, int cin, int kout,
                                                       unsigned short* __restrict__ out,
                                                       const float* __restrict__ bias, int relu,
                                                       const unsigned short* __restrict__ mask,
                                                       unsigned char* __restrict__ pidx,
                                                       int vblocks) {
  using G = GCfg<BHv>;
  constexpr int BH = G::BH, GWR = G::GWR, GWIN = G::GWIN, NMT = G::NMT, MS = G::MS, NS = G::NS;
  constexpr int GCHUNKS = G::GCHUNKS, GNI = G::GNI;
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  unsigned short* win = lds;
  unsigned short* wts = lds + 2 * GWIN;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  // epilogue scratch: window buffer 1 — a tile's last chunk (CC is even) — which is dead after
  // the K loop; buffer 0 already receives the NEXT tile's first window by then
  unsigned short* scr = lds + GWIN + wid * GSCR;
  // PERSISTENT workgroups: block v of the virtual grid goes to workgroup v % gridDim.x.
  // XCD-aware order of the virtual grid: workgroups are handed to the 8 XCDs round-robin by
  // linear id, and every 128-channel output block nb of a pixel block reads the same windows —
  // so the kb blocks of a pixel block get virtual ids 8 apart (same XCD, same moment, gridDim.x
  // being a multiple of 8 kb): their window fetches meet in that XCD's L2 instead of going out
  // to the Infinity Cache once per output block.
  const int kb = kout / NB;
  const int blocks_x = (W + BW - 1) / BW, blocks_y = (H + BH - 1) / BH;
  const int CC = cin / CCH, S = 9 * CC;
  const int wid_s = __builtin_amdgcn_readfirstlane(wid);
  const unsigned short* zeros = reinterpret_cast<const unsigned short*>(zero_block);
  const int dbg = SCL_DIAG_ONLY(relu >> 1);            // timing diagnostics (scl_debug_set_variant(3000 + bits))
  relu &= 1;
  // Staging is LDS-DMA.  Weights: the packed image IS the LDS image, 20 chunks of 1 KB per
  // step pair.  Window: lane l of chunk j owns slot 64 j + l = (pixel, piece), piece 4 the
  // pad (not fetched); where that pixel lies in the image is fixed for a tile.
  int nb = 0, b = 0, y0 = 0, x0 = 0;
  int woff[GNI];            // element offset at chunk 0; -1 outside the image; -2 not fetched
  auto locate = [&](int vb) -> bool {                 // virtual block -> tile; false: padding
    const int grp = vb / (8 * kb), rem = vb - grp * 8 * kb;
    const int pblk = grp * 8 + (rem & 7);
    nb = rem >> 3;
    if (pblk >= B * blocks_x * blocks_y) return false;
    b = pblk / (blocks_x * blocks_y);
    const int t2 = pblk % (blocks_x * blocks_y);
    y0 = (t2 / blocks_x) * BH;
    x0 = (t2 % blocks_x) * BW;
#pragma unroll
    for (int i = 0; i < GNI; ++i) {
      const int slot = 64 * (wid_s + 8 * i) + lane;
      const int pix = slot / 5, piece = slot - 5 * pix;
      const int y = y0 - 1 + pix / GWC, xx = x0 - 1 + pix % GWC;
      const bool inimg = y >= 0 && y < H && xx >= 0 && xx < W;
      woff[i] = (piece == 4 || pix >= GWR * GWC) ? -2
                : inimg ? ((b * H + y) * W + xx) * cin + 8 * piece : -1;
    }
    return true;
  };
  auto issue_win = [&](int cc, int buf) {
    const unsigned base = lds_byte_of(win) + buf * GWIN * 2;
#pragma unroll
    for (int i = 0; i < GNI; ++i) {
      const int j = wid_s + 8 * i;
      if (j < GCHUNKS && woff[i] != -2)
        glds16(woff[i] >= 0 ? x + woff[i] + CCH * cc : zeros, base + j * 1024);
    }
  };
  auto issue_wts = [&](int s, int buf) {
    const unsigned short* src = packed + ((int64_t)nb * S + s) * GWT + lane * 8;
    const unsigned base = lds_byte_of(wts) + buf * TPB * GWT * 2;
#pragma unroll
    for (int i = 0; i < (WCHK + 7) / 8; ++i) {
      const int j = wid_s + 8 * i;
      if (j < WCHK) glds16(src + j * 512, base + j * 1024);
    }
  };
  // Wave (mg, ng) of the 8 owns m-tiles 4 mg .. 4 mg + 3 (the block has 15: the last slot of
  // mg = 3 repeats tile 14 and is dropped in the epilogue) and output channels 64 ng .. + 63
  // (two n-tiles): 8 accumulators = 128 registers, so TWO waves share a SIMD and cover each
  // other's LDS / barrier waits; per k-step 4 A + 2 B fragment reads for 8 MFMAs.
  // lane (r, h): pixel (tile_row(r), tile_col(r)) of an m-tile, channels 8 h .. + 7 of a k-step
  const int mg = BH == 12 ? wid >> 1 : wid >> 2, ng = BH == 12 ? wid & 1 : wid & 3;
  int aoff[MS];
#pragma unroll
  for (int j = 0; j < MS; ++j) {
    const int mt = MS * mg + j < NMT ? MS * mg + j : NMT - 1;
    aoff[j] = ((4 * (mt / 5)) * GWC + 8 * (mt % 5)) * GPIX;
  }
  const int lane_a = (tile_row(r) * GWC + tile_col(r)) * GPIX + 8 * h;
  const int lane_b = (32 * NS * ng + r) * GPIX + 8 * h;

  bool staged = false;      // the current tile's first weights + window are already in flight
  for (int vb = blockIdx.x; vb < vblocks; vb += gridDim.x) {
  if (!staged) {
    if (!locate(vb)) continue;                          // padding of the last group of 8
    issue_wts(0, 0);
    issue_win(0, 0);
  }
  staged = false;
  const int nb_t = nb, b_t = b, y0_t = y0, x0_t = x0;   // this tile (locate() moves on below)

  f32x16 acc[MS * NS];                                // [m-tile slot][n-tile]
#pragma unroll
  for (int mt = 0; mt < MS * NS; ++mt) acc[mt] = zero16();

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();        // stage 0 landed; every wave is done with the previous tile's epilogue

  // S = 9 * CC steps in groups of three (one tap row of a chunk) per barrier.
  // The DMA of the next group's weights runs under this group; the window of chunk cc + 1 is
  // issued (after the weights) at tap row 0 of chunk cc and may stay in flight across this
  // group's barrier — the DMAs complete in order, so the counted wait below covers the weights
  // and the next group's full wait covers the window, two groups before it is read.
#pragma unroll 1
  for (int s = 0; s < S; s += TPB) {
    if (s + TPB < S && !(dbg & 1)) issue_wts(s + TPB, ((s / TPB) + 1) & 1);
    const int cc0 = s / 9, tap0 = s - 9 * cc0;
    const bool win_issued = tap0 == 0 && cc0 + 1 < CC && !(dbg & 2);
    if (win_issued) issue_win(cc0 + 1, (cc0 + 1) & 1);
    // 2 TPB groups of 8 MFMAs (tap u = g / 2, 16-channel k-step g % 2); the fragments of
    // group g + 1 (4 A + 2 B reads) fly under the MFMAs of group g, also across taps — only
    // the first group after a barrier waits for its operands
    u32x4 af[2][MS], bf[2][NS];
    auto load_group = [&](int g, u32x4 (&a4)[MS], u32x4 (&b2)[NS]) {
      const int u = g >> 1, ks2 = g & 1;
      const int su = s + u;
      const int cc = su / 9, tap = su - 9 * cc;
      const unsigned short* wa =
          win + (cc & 1) * GWIN + lane_a + ((tap / 3) * GWC + tap % 3) * GPIX + 16 * ks2;
      const unsigned short* wbp = wts + (((s / TPB) & 1) * TPB + u) * GWT + lane_b + 16 * ks2;
#pragma unroll
      for (int n = 0; n < NS; ++n) b2[n] = *reinterpret_cast<const u32x4*>(wbp + (32 * n) * GPIX);
#pragma unroll
      for (int j = 0; j < MS; ++j) a4[j] = *reinterpret_cast<const u32x4*>(wa + aoff[j]);
    };
    load_group(0, af[0], bf[0]);
#pragma unroll
    for (int g = 0; g < 2 * TPB; ++g) {
      if (g + 1 < 2 * TPB) load_group(g + 1, af[(g + 1) & 1], bf[(g + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < MS; ++j)
#pragma unroll
        for (int n = 0; n < NS; ++n)
          acc[NS * j + n] = mfma32b(af[g & 1][j], bf[g & 1][n], acc[NS * j + n]);
    }
    if (!win_issued)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (wid_s < GCHUNKS - 8 * (GNI - 1))           // this wave issued GNI window chunks
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GNI) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(GNI - 1) : "memory");
    __syncthreads();
  }

  // The next tile's first weights and window go out NOW, under this tile's epilogue (with one
  // workgroup per CU nothing else would cover their latency): every wave is past the K loop's
  // last barrier, so window buffer 0 and weight buffer 0 are free; the epilogue's scratch lives
  // in window buffer 1, which the next tile only refills after its first barrier.
  {
    const int vn = vb + gridDim.x;
    if (vn < vblocks && locate(vn)) {
      issue_wts(0, 0);
      issue_win(0, 0);
      staged = true;
    }
  }

  // epilogue: slot j <-> m-tile 4 mg + j, n <-> channels 64 ng + 32 n ..; accumulator register
  // q <-> pixel acc_row(q, h) of the tile, lane r <-> channel r of the n-tile
  if (EPI == 3) {
    // 2x2 pooling in the accumulator layout: with the conflict-free pixel map a window's upper
    // and lower row sit in the two half-waves (lanes l, l ^ 32) under the SAME register pair
    // (q, q + 1) — one cross-lane exchange per window; lanes of the first half store.
    const int PH = H / 2, PW = W / 2;
#pragma unroll
    for (int j = 0; j < MS; ++j) {
      const int mt = MS * mg + j;
      if (mt >= NMT) break;                           // wave-uniform
      const int mr = mt / 5, mc = mt % 5;
#pragma unroll
      for (int n = 0; n < NS; ++n) {
        const int ch = NB * nb_t + 32 * NS * ng + 32 * n + r;
        const float bias_r = bias[ch];
#pragma unroll
        for (int q0 = 0; q0 < 16; q0 += 2) {
          const float v0 = acc[NS * j + n][q0], v1 = acc[NS * j + n][q0 + 1];
          const float lm = fmaxf(v0, v1);
          const int li = v0 >= v1 ? 0 : 1;
          const float om = __shfl_xor(lm, 32);
          const int oi = __shfl_xor(li, 32);
          const int qq = q0 >> 2;
          const bool upper = (h == 0) == (qq == 0 || qq == 3);
          const float mu = upper ? lm : om, ml = upper ? om : lm;
          const int iu = upper ? li : oi, il = upper ? oi : li;
          const float m = fmaxf(mu, ml);
          const int k = mu >= ml ? iu : 2 + il;         // first maximum in raster order
          const int p0 = acc_row(q0, 0);                // the first-half lane's pixel
          const int py = (y0_t + 4 * mr + tile_row(p0)) >> 1, px = (x0_t + 8 * mc + tile_col(p0)) >> 1;
          if (h == 0 && py < PH && px < PW) {
            const int64_t po = (((int64_t)b_t * PH + py) * PW + px) * kout + ch;
            out[po] = f32_to_bf16(fmaxf(m + bias_r, 0.f));
            pidx[po] = (unsigned char)k;
          }
        }
      }
    }
  } else {
#pragma unroll
  for (int j = 0; j < MS; ++j) {
    const int mt = MS * mg + j;
    if (mt >= NMT) break;                             // wave-uniform
    const int mr = mt / 5, mc = mt % 5;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      const float bias_r = EPI == 1 ? bias[NB * nb_t + 32 * NS * ng + 32 * n + r] : 0.f;
      const int px = lane >> 1, hf = lane & 1;
      const int oy = y0_t + 4 * mr + tile_row(px), ox = x0_t + 8 * mc + tile_col(px);
      const bool inside = oy < H && ox < W;
      const int64_t o_off =
          (((int64_t)b_t * H + oy) * W + ox) * kout + NB * nb_t + 32 * NS * ng + 32 * n + 8 * hf;
      // instruction i of the two covers channels 16 i + 8 hf .. + 7: a lane pair writes (and
      // reads the mask as) 32 contiguous bytes — whole sectors
      u32x4 y0v = u32x4{0u, 0u, 0u, 0u}, y1v = y0v;
      if (EPI == 2 && inside) {                          // in flight under the transpose
        y0v = *reinterpret_cast<const u32x4*>(mask + o_off);
        y1v = *reinterpret_cast<const u32x4*>(mask + o_off + 16);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        float v = acc[NS * j + n][q] + bias_r;
        if (EPI == 1 && relu) v = fmaxf(v, 0.f);
        scr[acc_row(q, h) * GSCR_LD + r] = f32_to_bf16(v);
      }
      __builtin_amdgcn_wave_barrier();
      u32x4 v0 = *reinterpret_cast<const u32x4*>(scr + px * GSCR_LD + 8 * hf);
      u32x4 v1 = *reinterpret_cast<const u32x4*>(scr + px * GSCR_LD + 8 * hf + 16);
      __builtin_amdgcn_wave_barrier();
      if (EPI == 2) {
        v0 = relu_mask(v0, y0v);
        v1 = relu_mask(v1, y1v);
      }
      if (inside) {
        *reinterpret_cast<u32x4*>(out + o_off) = v0;
        *reinterpret_cast<u32x4*>(out + o_off + 16) = v1;
      }
    }
  }
  }   // EPI != 3
  }   // persistent loop over this workgroup's tiles
}

}  // namespace

// c: validated by conv_lds.hip; the packed weights take the whole scl_convg_workspace_bytes
template <int E, int BHV>
static void convg_run(const LdsConvCall& c, const unsigned short* packed, const LdsConvGrid& g,
                      int relu) {
  SCL_LAUNCH("convg_kernel", (convg_kernel<E, BHV>), dim3(g.gsize), dim3(NTHR), GCfg<BHV>::LDS,
             c.stream, (const unsigned short*)c.x, packed, c.B, c.H, c.W, c.cin, c.kout,
             (unsigned short*)c.out, c.bias, relu, (const unsigned short*)c.mask,
             (unsigned char*)c.pidx, g.vblocks);
}
template <int BHV>
static void convg_epilogue(const LdsConvCall& c, const unsigned short* packed, const LdsConvGrid& g,
                           int dbgbits) {
  if (c.pidx) convg_run<3, BHV>(c, packed, g, 0);
  else if (c.mask) convg_run<2, BHV>(c, packed, g, 0);
  else if (c.bias) convg_run<1, BHV>(c, packed, g, c.relu ? 1 : 0);
  else convg_run<0, BHV>(c, packed, g, dbgbits);
}

int convg_launch(const LdsConvCall& c) {
  static SclDeviceOnce once;
  scl_call_once(once, [] {        // (in the order the kernels are emitted: their code depends on it)
#define SCL_CONVG_ATTR(E, BHV)                                                                 \
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&convg_kernel<E, BHV>),              \
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)GCfg<BHV>::LDS);
    SCL_CONVG_ATTR(0, 12) SCL_CONVG_ATTR(1, 12) SCL_CONVG_ATTR(2, 12) SCL_CONVG_ATTR(3, 12)
    SCL_CONVG_ATTR(0, 8) SCL_CONVG_ATTR(1, 8) SCL_CONVG_ATTR(2, 8) SCL_CONVG_ATTR(3, 8)
#undef SCL_CONVG_ATTR
  });
  const int dv = SCL_DIAG_ONLY(c.dv);
  unsigned short* packed = (unsigned short*)c.workspace;
  const int64_t total = (int64_t)9 * (c.cin / CCH) * c.kout * GPIX;
  SCL_LAUNCH("convg_pack_kernel", convg_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256),
             0, c.stream, c.w, c.sk, c.sc, c.sh, c.sw, c.flags, c.cin, c.kout, packed);
  // block height: 12 rows, or 8 where the 12-row blocks would be too few or pad more
  const int bx = (c.W + BW - 1) / BW, kb = c.kout / NB;
  const int64_t wg12 = (int64_t)c.B * ((c.H + 11) / 12) * bx * kb, wg8 = (int64_t)c.B * ((c.H + 7) / 8) * bx * kb;
  const int cus = scl_conv_cus();
  // rounds of workgroups (one per CU) x rows per block = time in units of a block row
  const int64_t t12 = ((wg12 + cus - 1) / cus) * 12, t8 = ((wg8 + cus - 1) / cus) * 8;
  // scl_debug_set_variant(3012 / 3008) pins the block height (tests cover both variants)
  const bool low = dv == 3012 ? false : dv == 3008 ? true : t8 < t12;
  const int dbgbits = (dv >= 3001 && dv <= 3003) ? (dv & 3) << 1 : 0;
  const LdsConvGrid g = lds_conv_grid((low ? wg8 : wg12) / kb, kb, cus, dv);
  if (low) convg_epilogue<8>(c, packed, g, dbgbits);
  else convg_epilogue<12>(c, packed, g, dbgbits);
  return scl_launch_status();
}
