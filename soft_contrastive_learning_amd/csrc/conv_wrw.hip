// The weight gradient of EVERY 3x3 / stride 1 / same-padding convolution on bf16 channels-last
// activations (channel counts multiples of 64, up to 1024),
//   dW[k][c][kh][kw] = sum_{b,y,x} gz[b,y,x,k] * x[b, y+kh-1, x+kw-1, c],
// with the bias gradient on the side.  Entry points (include/scl_hip.h), front door and kernels in
// launch order; the host side is the end of this file, the diagnostic build's variants are
// conv_wrw_diag.hip.
//
// scl_wrw3x3_bias / _pooled (scl_wrw3x3_ex, scl_wrw3x3, scl_wrw64): each fills a WrwCall; wrw3x3_run
// checks it and cuts the work with ONE WrwPlan (wrw_plan; the workspace: wrw_space).
//   wrw64_kernel<TWv, NKB, PL, SCHED> [64 c] x [64 NKB k] blocks over pixel splits -> slabs (+ bias
//                              partials); tile width, blocks, pooled form and schedule (whole tiles; half
//                              tiles with waves 4-7 half a tile behind: diagnostic library only, wrw_sched)
//                              chosen once: for_wrw_shape, wrw_launch
//   wrw64_reduce_kernel<RG>    slabs -> gw at its strides (+ grad_bias): wrw_reduce
//
// wrw64_kernel: the contraction runs over pixels — the SLOW index of both channels-last operands — so
// both MFMA operands are read with ds_read_b64_tr_b16 out of row-major LDS tiles (an x halo
// window and the gz tile); a tap row is a window-row offset and a tap column a
// pixel offset of the x read: both shifts are LDS addresses, every MFMA operand is an aligned
// register tuple as loaded and no vector instruction assembles one (see the loop).
//   * v_mfma_f32_32x32x16_bf16 with M = 32 input channels, N = 32 output channels, 16 pixels
//     per step; wave (mt, nt) keeps all nine taps of its 32 x 32 block: 144 accumulators;
//   * persistent grid, one workgroup per CU accumulating over all its tiles, then ONE slab
//     [9][64][64] float32 per workgroup; wrw64_reduce_kernel sums the slabs in a fixed order
//     into the weight's own layout (bf16).
// LDS layout: each staged tile is TWO planes of 32 channels with 64-byte pixels and no padding.
// A ds_read_b64_tr_b16 is served 32 lanes at a time (8-byte units, 32 of them per cycle); the
// 32 lanes of a group address 4 pixels x (2 x 16 channels): unit = 8 * pixel + 4 * (channel
// half) + piece, all distinct mod 32 — conflict-free; the four pixels of a group are consecutive
// in one window row, so a read that starts one or two pixels further right (kw = 1, 2) only
// rotates the units.  (One 64-channel plane at 144 B per
// pixel, fine for ds_read_b128, makes every transposed read 2-way conflicted: unit 18 * pixel.)
// The planes are filled by LDS-DMA (global_load_lds_dwordx4: no staging registers, no
// ds_write pass, 80 KB in flight per CU): one wave-instruction writes 1 KB = 16 pixels of a
// plane, lane -> (pixel lane >> 2, 16-byte piece lane & 3) — the image is lane-linear as the
// DMA requires.  Out-of-image halo pixels are fetched from a zero block.  Round 3: the DMA
// instructions of a tile go out one at a time between the products (back to back they parked the
// wave for 2,100 cycles), with a scalar base + constant lane offset for tiles off the border;
// the grid is 1-D with the workgroups that share tiles on one XCD; PL = 1 builds the gz tile from
// the pooled gradient + window index instead.
#include "scl_common.h"

namespace {

constexpr int C64 = 64;
constexpr int WPL = 32;                              // bf16 per pixel and plane

// The bits of wrw64_kernel's DBG.  The product launches DBG 0 only; the others are instantiated by
// conv_wrw_diag.hip (scl_debug_set_variant(2001 ..), its header has the table).
enum : int {
  kDbgNoRestage = 2,     // no staging after the first tile: timing only, WRONG results
  kDbgStamps = 4,        // s_memtime stamps instead of the bias partials (see the tile loop)
  kDbgLaneBorders = 8,   // per-lane border tests for every tile at the image border, as before the
                         // buffer path (TilePos::mode 1): A/B partner, correct results
  kDbgMfma16 = 16,       // the products on v_mfma_f32_16x16x32_bf16: timing only, RESULTS MEANINGLESS
};

// grid (pixel splits P, C / 64, K / 64): workgroup (p, cb, kb) accumulates the [9][64][64]
// block (input channels 64 cb .., output channels 64 kb ..) over the tiles p, p + P, ...
// Geometry of a variant: TWv = tile width (32 or 8), NKB = 64-channel output blocks per
// workgroup (1: [64 c] x [64 k], waves = 2 x 2 blocks x 2 pixel halves of a 256-pixel tile;
// 2: [64 c] x [128 k], waves = 2 x 4 blocks over a whole 128-pixel tile — the x window is
// fetched once for twice the output channels: 24 % fewer bytes per FLOP, which is what the
// kernel is bound by once the staging is DMA: 76 KB per 72 MFMAs of every wave).
// SCHED (the schedule, see wrw64_kernel): 0 = whole tiles in two buffers, the eight waves in step;
// 1 (NKB = 2) = HALF tiles — the left / right 16 columns of a wide tile, the upper / lower 8 rows
// of a tall one: steps 0-3 and 4-7 of a wave — in a ring of four slots, waves 4-7 one half behind
// waves 0-3.  The staged unit (SW x SH pixels, its halo window WCv x WRv) is the tile or the half.
template <int TWv, int NKB, int SCHED = 0>
struct WrwCfg {
  static_assert(SCHED == 0 || NKB == 2, "the half-tile schedule is built for [64 c] x [128 k] blocks");
  static constexpr int PIXELS = 256 / NKB;
  static constexpr int THv = PIXELS / TWv;             // the tile's height
  static constexpr int SW = SCHED && TWv == 32 ? TWv / 2 : TWv, SH = SCHED && TWv != 32 ? THv / 2 : THv;
  static constexpr int NSTEP = SCHED ? 4 : 8;          // steps of 16 pixels per wave and unit
  static constexpr int WCv = SW + 2, WRv = SH + 2;
  static constexpr int XCHv = (WRv * WCv + 15) / 16;   // 1-KB chunks per x plane
  static constexpr int GCHv = SW * SH / 16;            // per gz plane
  static constexpr int XPL = XCHv * 16 * WPL, GPL = GCHv * 16 * WPL;
  static constexpr int BUF = 2 * XPL + 2 * NKB * GPL;  // one staged (x window, gz tile) pair
  static constexpr int CHUNKS = 2 * XCHv + 2 * NKB * GCHv;
  static constexpr int NBUF = SCHED ? 4 : 2;
  static constexpr size_t LDS = NBUF * (size_t)BUF * sizeof(unsigned short);
};

// TWv: tile width, 32 (8 x 32 tiles, a step = 16 pixels of a row) or 8 (32 x 8 tiles for
// narrow maps, a step = two rows of 8): the same 256 pixels, 340-pixel windows and LDS image
// either way — only the pixel <-> address maps differ; the host takes the shape that pads the
// map less (W = 80: 96 -> 80 columns; 30 x 40: 32 x 64 -> 32 x 40).
//
// PL = 1: the layer ends in a 2x2 max-pooling, and `gz` is the POOLED gradient [B][H/2][W/2][K]
// with `pidx` the window position (2 dy + dx) of every maximum (scl_conv3x3_pool_idx): the
// full-size gradient — one non-zero per window and channel — is never in memory.  Its tile is
// built in LDS instead: every thread loads 16 bytes of the pooled gradient and their 8 index
// bytes for the NEXT tile when the tile starts (512 threads = the tile's pooled pixels x planes x
// pieces exactly), and writes the four 16-byte pixels of the window at the tile's end.  The gz
// part of the stream shrinks from 2 to 0.75 bytes per element; H and W are even (host check),
// so a window is inside or outside the image as a whole.
template <int DBG, int TWv, int NKB, int PL = 0, int SCHED = 0>
__global__ __launch_bounds__(512, 1) void wrw64_kernel(const unsigned short* __restrict__ x,
                                                       const unsigned short* __restrict__ gz,
                                                       int B, int H, int W, int C, int K,
                                                       float* __restrict__ slabs,
                                                       float* __restrict__ bslabs,
                                                       const unsigned char* __restrict__ pidx) {
  extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  using Cfg = WrwCfg<TWv, NKB, SCHED>;
  static_assert(SCHED == 0 || (DBG & ~kDbgStamps) == 0, "the half-tile schedule carries the stamps only");
  // Workgroup -> (pixel split p, input block cb, output block kz).  The 1-D grid is dealt to the
  // eight XCDs round robin (workgroup L runs on XCD L % 8) and every workgroup is resident at
  // once.  The n_cb * n_kz workgroups of one p walk the same tiles at the same time — each x
  // window is read by n_kz of them, each gz tile by n_cb — so they are put on ONE XCD: its L2
  // then serves all but the first request (33 instead of 13 bytes per cycle and CU into the LDS;
  // with p on the fast grid axis the siblings sat on different XCDs and every one of them
  // fetched from the Infinity Cache: the staging stream, 58 KB per tile, was the kernel's bound).
  const int n_cb = C / C64, n_kz = K / (NKB * C64), n_sib = n_cb * n_kz;
  const int n_p = gridDim.x / n_sib;
  int wg_p, wg_sib;
  if (n_p % 8 == 0) {
    const int s_ = blockIdx.x >> 3;
    wg_sib = s_ % n_sib;
    wg_p = (blockIdx.x & 7) + 8 * (s_ / n_sib);
  } else {
    wg_p = blockIdx.x % n_p;
    wg_sib = blockIdx.x / n_p;
  }
  const int wg_cb = wg_sib % n_cb, wg_kz = wg_sib / n_cb;
  constexpr int XCH = Cfg::XCHv, GCH = Cfg::GCHv, XPLANE = Cfg::XPL, GPLANE = Cfg::GPL;
  constexpr int WBUF = Cfg::BUF, WCHUNKS = Cfg::CHUNKS;
  // eight waves, two per SIMD.  NKB = 1: wave (mt, nt, ph) accumulates block (mt, nt) over the
  // steps of pixel half ph of the tile; the two halves write separate slabs.  NKB = 2: wave
  // (mt, nt of 4) over the whole tile.  Eight steps of 16 pixels per wave and tile either way.
  const int mt = wid & 1, nt = NKB == 1 ? (wid >> 1) & 1 : wid >> 1, ph = NKB == 1 ? wid >> 2 : 0;
  // transposed-read role of this lane: 16-lane group gq = lane >> 4 covers channels
  // 16 (gq & 1) .. + 15 and pixels 8 (gq >> 1) + q (+ 4); lane 4q + p addresses row q,
  // columns 4p .. 4p + 3
  // SW x SH: the staged unit — the tile, or (SCHED 1) a half of it — and its window WCv x WRv
  constexpr int THv = Cfg::THv, SW = Cfg::SW, SH = Cfg::SH, WCv = Cfg::WCv, WRv = Cfg::WRv;
  const int q = (lane >> 2) & 3, pp = lane & 3, gq = lane >> 4;
  const int ch0 = 16 * (gq & 1) + 4 * pp;
  // the lane's pixel inside a step: (row, column) relative to the step's first pixel
  const int lrow = TWv == 32 ? 0 : (gq >> 1), lcol = TWv == 32 ? 8 * (gq >> 1) + q : q;

  const int tiles_x = (W + TWv - 1) / TWv, tiles_y = (H + THv - 1) / THv;
  const int per_img = tiles_x * tiles_y;
  const int ntiles = B * per_img;

  // wave wid issues chunks j = wid, wid + 8, ... of the 76: [x plane 0][x plane 1][gz 0][gz 1]
  // (PL: of the x planes only).  Which pixel of the window / tile a lane fetches for its i-th
  // chunk does not depend on the tile: (row << 8 | column) once, -1 for the slack behind the
  // window.  A wave whose last index is past the end issues the last chunk once more (the same
  // bytes to the same place as the wave that owns it): stage_chunk has no branches, it sits
  // between the products of the unrolled tile loop.
  constexpr int NCH = PL ? 2 * XCH : WCHUNKS;
  // (SCHED 1: a wave stages in steps 0-3 of its own tile only — the four waves 0-3 a whole even
  // half, waves 4-7 a whole odd one — so of a SIMD's two waves one is issuing DMA and one is not)
  constexpr int NSW = SCHED ? 4 : 8;
  constexpr int NI = (NCH + NSW - 1) / NSW;
  const int wid_s = __builtin_amdgcn_readfirstlane(wid);
  const int pl = lane >> 2, piece = lane & 3;
  int rel[NI], roff[NI];      // roff: element offset from the tile's first (halo) pixel
  int ldst[NI];               // (wave-uniform) LDS byte offset of the chunk inside a buffer
  bool is_x[NI];              // (wave-uniform) x window or gz tile
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int j = wid_s % NSW + NSW * i < NCH ? wid_s % NSW + NSW * i : NCH - 1;
    is_x[i] = j < 2 * XCH;
    if (j < 2 * XCH) {
      const int plane = j >= XCH ? 1 : 0;
      const int pix = 16 * (j - XCH * plane) + pl;
      rel[i] = pix < WRv * WCv ? ((pix / WCv) << 8) | (pix % WCv) : -1;
      // (the slack lanes behind the window point at its first pixel: never read, always mapped)
      const int pv = pix < WRv * WCv ? pix : 0;
      roff[i] = ((pv / WCv) * W + pv % WCv) * C + C64 * wg_cb + 8 * piece + 32 * plane;
      ldst[i] = (plane * XPLANE + (j - XCH * plane) * 512) * 2;
    } else {
      const int jj = j - 2 * XCH;
      const int plane = jj / GCH;
      const int pix = 16 * (jj - GCH * plane) + pl;
      rel[i] = ((pix / SW) << 8) | (pix % SW);
      roff[i] = ((pix / SW) * W + pix % SW) * K + NKB * C64 * wg_kz + 8 * piece + 32 * plane;
      ldst[i] = (2 * XPLANE + plane * GPLANE + (jj - GCH * plane) * 512) * 2;
    }
  }
  const unsigned short* zeros = reinterpret_cast<const unsigned short*>(zero_block);
  // One chunk (i) of a tile's staging; the whole of it = stage_issue.  Inside the tile loop the
  // chunks go out one at a time between the products (stage_chunk at every fifth): the s_memtime
  // stamps (scripts/wrw_stamps.py) showed a wave that issues its ten DMA instructions back to back
  // blocked for 2,100 cycles — the queue in front of the LDS takes them at the rate the data
  // arrives (58 KB at 13 B per cycle), and the wave's 72 products only started afterwards.
  struct TilePos {
    int ty, tx, xo, go;      // first pixel; element offsets of the window's / tile's first pixel
    int mode;                // 0: the whole halo window lies inside the image; 1: its COLUMNS do
                             // (rows may not): the buffer path; 2: per-lane border tests
    int b, xi, gi;           // image; the same offsets relative to the image's first element
  };
  // (hf: SCHED 1, the half of the tile)
  auto tile_pos = [&](int tile, int hf = 0) {
    const int b = tile / per_img, t2 = tile % per_img;
    TilePos t;
    t.ty = (t2 / tiles_x) * THv + (TWv == 32 ? 0 : SH * hf);
    t.tx = (t2 % tiles_x) * TWv + (TWv == 32 ? SW * hf : 0);
    // (< 2^31: host check; the window's may be negative at the image border — those lanes are
    // masked by `ok`)
    t.xo = ((b * H + t.ty - 1) * W + t.tx - 1) * C;
    t.go = ((b * H + t.ty) * W + t.tx) * K;
    const bool colin = t.tx >= 1 && t.tx + SW < W;
    // (one scalar: as two bools hipcc rebuilt them as lane masks at every chunk)
    t.mode = __builtin_amdgcn_readfirstlane(
        colin && t.ty >= 1 && t.ty + SH < H ? 0 : (colin && !(DBG & kDbgLaneBorders) ? 1 : 2));
    t.b = b;
    t.xi = ((t.ty - 1) * W + t.tx - 1) * C;      // (negative in the first tile row)
    t.gi = (t.ty * W + t.tx) * K;
    return t;
  };
  auto stage_chunk = [&](const TilePos& tp, int buf, int i) __attribute__((always_inline)) {
    const int ty = tp.ty, tx = tp.tx, xo = tp.xo, go = tp.go;
    const unsigned dst = __builtin_amdgcn_readfirstlane(lds_byte_of(lds) + buf * WBUF * 2 + ldst[i]);
    if (tp.mode == 0) {
      // (wave-uniform) no border in sight: scalar base + the lane's constant offset
      glds16_s(is_x[i] ? x + xo : gz + go, 2u * (unsigned)roff[i], dst);
    } else if (tp.mode == 1) {
      // (wave-uniform) rows above / below the image: the resource of image b bounds every lane's
      // offset; a negative one wraps and is out of range too — zeros, like the zero block's
      const u32x4 rs = is_x[i] ? image_rsrc(x, (int64_t)tp.b * H * W * C, (unsigned)(H * W * C) * 2u)
                               : image_rsrc(gz, (int64_t)tp.b * H * W * K, (unsigned)(H * W * K) * 2u);
      blds16(rs, 2u * (unsigned)((is_x[i] ? tp.xi : tp.gi) + roff[i]), dst);
    } else {
      const int halo = is_x[i] ? 1 : 0;
      const int y = ty - halo + (rel[i] >> 8), xx = tx - halo + (rel[i] & 255);
      const bool ok = rel[i] >= 0 && (unsigned)y < (unsigned)H && (unsigned)xx < (unsigned)W;
      const unsigned short* src = (is_x[i] ? x : gz) + ((is_x[i] ? xo : go) + roff[i]);
      glds16(ok ? src : zeros, dst);
    }
  };
  auto stage_issue = [&](int tile, int buf, int hf = 0) __attribute__((always_inline)) {
    const TilePos tp = tile_pos(tile, hf);
#pragma unroll
    for (int i = 0; i < NI; ++i) stage_chunk(tp, buf, i);
  };
  // PL: this thread's window of the unit = pooled pixel (pr, pc), 8 channels (plane, piece).  SCHED 1:
  // a half has 256 of them — waves 0-3 build the even halves, waves 4-7 the odd ones.
  constexpr int NPC = SW / 2, NPR = SH / 2;
  const int p_tid = (SCHED ? threadIdx.x & 255 : threadIdx.x) >> 2;
  const int p_piece = threadIdx.x & 3, p_pc = p_tid % NPC;
  const int p_pr = (p_tid / NPC) % NPR, p_plane = p_tid / (NPC * NPR);
  const int Ho = H >> 1, Wo = W >> 1;
  u32x4 pg = {0u, 0u, 0u, 0u};
  uint2 pi = {0u, 0u};
  auto pool_issue = [&](int tile, int hf = 0) {
    const int b = tile / per_img, t2 = tile % per_img;
    const int py = (t2 / tiles_x) * (THv / 2) + (TWv == 32 ? 0 : NPR * hf) + p_pr;
    const int px = (t2 % tiles_x) * (TWv / 2) + (TWv == 32 ? NPC * hf : 0) + p_pc;
    const int off = ((b * Ho + py) * Wo + px) * K + NKB * C64 * wg_kz + 32 * p_plane + 8 * p_piece;
    if (py < Ho && px < Wo) {
      pg = *reinterpret_cast<const u32x4*>(gz + off);
      pi = *reinterpret_cast<const uint2*>(pidx + off);
    } else {
      pg = u32x4{0u, 0u, 0u, 0u};
      pi = uint2{0u, 0u};
    }
  };
  auto pool_write = [&](int buf) {
    unsigned short* dst = lds + buf * WBUF + 2 * XPLANE + p_plane * GPLANE +
                          (2 * p_pr * SW + 2 * p_pc) * WPL + 8 * p_piece;
    const UnpoolFlags fl = unpool_flags(pi.x, pi.y);
#pragma unroll
    for (int pos = 0; pos < 4; ++pos)
      *reinterpret_cast<u32x4*>(dst + ((pos >> 1) * SW + (pos & 1)) * WPL) = unpool8(pg, fl, pos);
  };

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = zero16();
  // Bias gradient on the side: the B fragment of a step is 8 pixels of gz channel r of this
  // wave's n-tile — summed into one register per lane (v_dot2c_f32_bf16 against (1, 1): four
  // instructions per nine MFMAs), behind a wave-uniform branch in the waves that write theirs
  // out: mt == 0 of the workgroups cb == 0.
  float bsum = 0.f;
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const bool bias_wave = __builtin_amdgcn_readfirstlane((bslabs && wg_cb == 0 && mt == 0) ? 1 : 0) != 0;

  // The wave's 72 (step, tap) products of a tile run as ONE software pipeline: the window-row
  // fragment a product opens is requested six products earlier (an LDS transposed read returns
  // long after one 32-cycle MFMA), the B operand of the next step while the current one runs.
  // The tiles alternate between two LDS buffers: the DMA of tile n + 1 runs under the whole
  // of tile n; one barrier per tile (it drains the DMA: hipcc waits vmcnt(0) there).
  //
  // SCHED 1 — the two waves of a SIMD half a tile apart.  With SCHED 0 every barrier puts the eight
  // waves back in phase: both waves of a SIMD run their DMA-laden steps 0-3 together and their clean
  // steps 4-7 together, matrix beside matrix, and the older one then idles at the barrier while the
  // younger one finishes alone.  Here the staged unit is a HALF tile (steps 0-3 or 4-7: disjoint
  // pixels, the shared halo staged twice) in a ring of four slots, and interval n — the time between
  // two barriers — runs
  //   waves 0-3: the 36 products of half n           (slot n & 3)
  //   waves 4-7: the 36 products of half n - 1       (slot (n - 1) & 3)
  //   staging:   all chunks of half n + 2            (slot (n + 2) & 3: half n - 2 lived there, and
  //              its last reader, a wave 4-7 in interval n - 1, left it before the barrier)
  // so every wave issues exactly the products of SCHED 0, in the same order, into the same
  // accumulators — the results are the same bit for bit — only the barrier a product runs against
  // moves.  Half n + 2 is staged by the four waves that are in steps 0-3 of their own tile (waves
  // 0-3 the even halves, waves 4-7 the odd ones; the pooled form builds its gz half there too): of a
  // SIMD's two waves one issues DMA and the other does not.  A wave waits for its chunks at the end
  // of its steps 4-7, one barrier before the first reader.  (All eight waves staging in every
  // interval, four chunks each, was measured too: 3-14 % slower than SCHED 0 on every layer.)
  // Waves 4-7 sit out interval 0, waves 0-3 the last one: every wave of a workgroup passes
  // 2 * tiles + 2 barriers, however many tiles it walks.
  //
  // kDbgStamps (scl_debug_set_variant(2004 / 2006 / 2008)): wave 0 of every workgroup writes s_memtime
  // stamps of its first four tiles to bslabs (no bias partials then): [workgroup][tile][8] —
  //   SCHED 0: 0 tile start, 1 staging issued, 2 first step done, 3 fourth step done, 4 last product
  //            issued, 5 own DMA landed, 6 barrier passed;
  //   SCHED 1: 0 tile start, 1 first step done, 2 fourth step done, 3 own DMA landed, 4 mid-tile
  //            barrier passed, 5 last product issued, 6 own DMA landed, 7 barrier passed — and wave 4
  //            writes the same record of ITS tiles behind the slabs in use (the workspace holds two
  //            slabs per workgroup, [64 c] x [128 k] blocks write one).
  uint64_t stamp[8];
#define WRW_STAMP(k)                                                     \
  do {                                                                   \
    if (DBG & kDbgStamps) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[k])::"memory"); \
  } while (0)
  // The NSTEP * 9 products of one staged unit out of buffer `buf`, the wave's chunks of unit `stg`
  // on their way into buffer `sbuf` in between.
  auto products = [&](auto stage_, int buf, const TilePos& stg, int sbuf, auto&& stamp_at) __attribute__((always_inline)) {
    constexpr bool STAGE = decltype(stage_)::value;
    const unsigned short* xl =
        lds + buf * WBUF + mt * XPLANE + (lrow * WCv + lcol) * WPL + ch0;
    const unsigned short* gl =
        lds + buf * WBUF + 2 * XPLANE + nt * GPLANE + (lrow * SW + lcol) * WPL + ch0;
    // product i = 9 * s + t: step s of this wave's eight (first pixel (ry, cx)), tap t = 3 kh + kw.
    // A lane's A operand is 8 consecutive pixels of a window row for its channel; the three kw
    // taps of a row are the same pixels shifted by 0 / 1 / 2 — three fragments of 8 pixels (two
    // transposed reads each), read at pixel offsets 0 / 1 / 2 of the window row: the shift is an
    // address, and every product multiplies exactly the pixel pairs it always did (the results do
    // not change by a bit against the fragment that was shifted inside the lane with four
    // v_alignbit for kw = 1 and four register moves for kw = 2).  A window row serves the kh taps
    // of three tile rows (wide tiles) / two steps (tall tiles): its fragments are read once and
    // stay in registers.  LDS reads per wave and tile: 72 (102 tall) + 16 for B instead of 144 + 16
    // for nine separate taps, which kept the LDS pipe busy for more cycles than the MFMAs take.
    auto x_frag = [&](int wrow, int cx, int kw) {
      return tr_pair(xl + (wrow * WCv + cx + kw) * WPL, 4 * WPL);
    };
    // window row (relative to the wave's first) and column slot of step s_, tap row kh
    // Wide tiles walk the left 16 columns of the wave's four rows, then the right ones (steps
    // 0-3, 4-7): three window rows of ONE column half are live at a time.  (SCHED 1: the unit IS one
    // half — four steps, one column slot.)
    constexpr int NS = Cfg::NSTEP;
    constexpr int NFR = TWv == 32 ? 6 : 2 * NS + 2, NFC = TWv == 32 && !SCHED ? 2 : 1;
    auto f_row = [](int s_, int kh) { return TWv == 32 ? (s_ & 3) + kh : 2 * s_ + kh; };
    auto f_col = [](int s_) { return TWv == 32 && !SCHED ? (s_ >> 2) : 0; };
    // is (s_, kh) the first product that touches its fragment?
    auto f_first = [](int s_, int kh) { return TWv == 32 ? ((s_ & 3) == 0 || kh == 2) : (s_ == 0 || kh >= 1); };
    const int row_w = TWv == 32 ? 4 * ph : 16 * ph;        // the wave's first window row
    u32x4 fr[NFR][NFC][3];
    auto f_load = [&](int i) {                            // the fragment product i opens
      const int s_ = i / 9, kh = (i % 9) / 3, kw = i % 3;
      fr[f_row(s_, kh)][f_col(s_)][kw] = x_frag(row_w + f_row(s_, kh), 16 * f_col(s_), kw);
    };
    auto b_of = [&](int s_) {
      const int ry = TWv == 32 ? 4 * ph + (s_ & 3) : 16 * ph + 2 * s_;
      return tr_pair(gl + (ry * SW + 16 * f_col(s_)) * WPL, 4 * WPL);
    };
    constexpr int LEAD = 6;                                // products between a read and its first use
    constexpr int STG = SCHED ? 4 : 5;                     // products between two staging chunks
    // (SCHED 1 waits for its chunks one interval later)
    static_assert(STG * NI <= 9 * NS - (SCHED ? 0 : 12), "the last chunk needs time to land");
    u32x4 bf[2];
#pragma unroll
    for (int i = 0; i < LEAD; ++i)
      if (f_first(i / 9, (i % 9) / 3)) f_load(i);
    bf[0] = b_of(0);
#pragma unroll
    for (int i = 0; i < 9 * NS; ++i) {
      const int s_ = i / 9, kh = (i % 9) / 3, kw = i % 3;
      if (i + LEAD < 9 * NS && f_first((i + LEAD) / 9, ((i + LEAD) % 9) / 3)) f_load(i + LEAD);
      if (i % 9 == 2 && s_ + 1 < NS) bf[(s_ + 1) & 1] = b_of(s_ + 1);
      if (STAGE && !(DBG & kDbgNoRestage) && i % STG == 0 && i / STG < NI) stage_chunk(stg, sbuf, i / STG);
      __builtin_amdgcn_sched_barrier(0);
      const u32x4 a = fr[f_row(s_, kh)][f_col(s_)][kw];
      if constexpr ((DBG & kDbgMfma16) != 0) {
        // timing ablation (RESULTS MEANINGLESS): the same FLOPs, operand registers and accumulator
        // registers on v_mfma_f32_16x16x32_bf16 — what would the other MFMA shape be worth here?
        f32x16& c_ = acc[i % 9];
        const int o_ = 8 * (i & 1);
        f32x4 q0 = {c_[o_], c_[o_ + 1], c_[o_ + 2], c_[o_ + 3]};
        f32x4 q1 = {c_[o_ + 4], c_[o_ + 5], c_[o_ + 6], c_[o_ + 7]};
        q0 = mfma16b(a, bf[s_ & 1], q0);
        q1 = mfma16b(a, bf[s_ & 1], q1);
        c_[o_] = q0[0]; c_[o_ + 1] = q0[1]; c_[o_ + 2] = q0[2]; c_[o_ + 3] = q0[3];
        c_[o_ + 4] = q1[0]; c_[o_ + 5] = q1[1]; c_[o_ + 6] = q1[2]; c_[o_ + 7] = q1[3];
      } else {
        acc[i % 9] = mfma32b(a, bf[s_ & 1], acc[i % 9]);
      }
      stamp_at(i);
      if (i % 9 == 4 && bias_wave) {
        const u32x4 bw = bf[s_ & 1];
        const bf16x2 one2 = __builtin_bit_cast(bf16x2, 0x3f803f80u);
        // (element by element: indexing the vector in a loop made hipcc feed word 0 four times)
        const unsigned w0 = bw.x, w1 = bw.y, w2 = bw.z, w3 = bw.w;
        bsum = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w0), one2, bsum, false);
        bsum = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w1), one2, bsum, false);
        bsum = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w2), one2, bsum, false);
        bsum = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, w3), one2, bsum, false);
      }
    }
  };
  // the stamps of wave `wv`'s tile number tcount (of its first four) go to `o`
  auto stamps_out = [&](uint64_t* o, int wv, int tcount) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (threadIdx.x == 64 * wv && tcount < 4) {
      o += ((int64_t)((int)blockIdx.x) * 4 + tcount) * 8;
#pragma unroll
      for (int k = 0; k < (SCHED ? 8 : 7); ++k) o[k] = stamp[k];
    }
  };

  if constexpr (SCHED == 0) {
    int tile = wg_p;
    if (tile < ntiles) {
      stage_issue(tile, 0);
      if (PL) {
        pool_issue(tile);
        pool_write(0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0, tcount = 0;
    for (; tile < ntiles; tile += n_p) {
      WRW_STAMP(0);
      const int next = (DBG & kDbgNoRestage) ? ntiles : tile + n_p;
      // (after the last tile the current one is staged again, into the buffer nobody reads: the
      // product loop stays free of branches)
      const TilePos stg = tile_pos(next < ntiles ? next : tile);
      if (PL && next < ntiles) pool_issue(next);
      WRW_STAMP(1);
      products(std::true_type{}, buf, stg, buf ^ 1, [&](int i) {
        if (i == 8) WRW_STAMP(2);
        if (i == 35) WRW_STAMP(3);
        if (i == 71) WRW_STAMP(4);
      });
      if (PL && next < ntiles) pool_write(buf ^ 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMA chunks have landed
      WRW_STAMP(5);
      __syncthreads();
      WRW_STAMP(6);
      if (DBG & kDbgStamps) stamps_out(reinterpret_cast<uint64_t*>(bslabs), 0, tcount++);
      buf ^= 1;
    }
  } else {
    // (wave-uniform, scalar: the barriers below sit behind branches on it)
    const int lag = wid_s >> 2;
    const int nh = wg_p < ntiles ? 2 * ((ntiles - wg_p + n_p - 1) / n_p) : 0;   // this workgroup's halves
    auto tile_of = [&](int g) { return wg_p + (g >> 1) * n_p; };
    if (nh > 0) {
      stage_issue(tile_of(0), 0, 0);
      stage_issue(tile_of(1), 1, 1);
      if (PL) {
        pool_issue(tile_of(lag), lag);
        pool_write(lag);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (lag) __syncthreads();                               // interval 0 of waves 4-7
    for (int g = 0; g < nh; g += 2) {                       // the wave's halves g, g + 1 in intervals g + lag ..
      WRW_STAMP(0);
      const int hs = g + 2 + lag;
      // (past the last half the current one is staged again, into the slot nobody reads: the product
      // loop stays free of branches)
      const TilePos stg = hs < nh ? tile_pos(tile_of(hs), hs & 1) : tile_pos(tile_of(g), 0);
      const bool pool_now = PL && hs < nh;
      if (pool_now) pool_issue(tile_of(hs), hs & 1);
      products(std::true_type{}, g & 3, stg, hs & 3, [&](int i) {
        if (i == 8) WRW_STAMP(1);
        if (i == 35) WRW_STAMP(2);
      });
      if (pool_now) pool_write(hs & 3);
      WRW_STAMP(3);
      __syncthreads();
      WRW_STAMP(4);
      products(std::false_type{}, (g + 1) & 3, stg, 0, [&](int i) {
        if (i == 35) WRW_STAMP(5);
      });
      // the chunks of half hs have landed: its first reader passes the barrier after this one
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      WRW_STAMP(6);
      __syncthreads();
      WRW_STAMP(7);
      if (DBG & kDbgStamps) {
        // (wave 4: behind the gridDim.x slabs of [2][9][64][64] floats that this launch writes)
        uint64_t* lag_o = reinterpret_cast<uint64_t*>(slabs + (int64_t)gridDim.x * 2 * 9 * C64 * C64);
        stamps_out(lag ? lag_o : reinterpret_cast<uint64_t*>(bslabs), 4 * lag, g >> 1);
      }
    }
    if (!lag) __syncthreads();                              // the last interval of waves 0-3
  }
#undef WRW_STAMP

  // slab[s][cb][kb][tap][c][k] with 64 x 64 blocks (cb, kb): s = 2 p + ph (NKB = 1) or p, kb =
  // the workgroup's block or its pair 2 z + nt / 2; accumulator register qq <-> c = 32 mt +
  // acc_row(qq, h), lane r <-> k
  const int slab = NKB == 1 ? 2 * wg_p + ph : wg_p;
  const int kb = NKB == 1 ? wg_kz : 2 * wg_kz + (nt >> 1);
  float* out = slabs + (((int64_t)slab * n_cb + wg_cb) * (NKB * n_kz) + kb) * 9 * C64 * C64;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int qq = 0; qq < 16; ++qq)
      out[(t * C64 + 32 * mt + acc_row(qq, h)) * C64 + 32 * (nt & 1) + r] = acc[t][qq];
  // bias partials [slab][K]: the two pixel halves h of a step combined in a fixed order
  const float bs = bsum + __shfl_xor(bsum, 32);
  if (bslabs && !(DBG & kDbgStamps) && wg_cb == 0 && mt == 0 && h == 0)
    bslabs[(int64_t)slab * K + C64 * kb + 32 * (nt & 1) + r] = bs;
}

// dW element (k, c, kh, kw) = sum over the pixel-split slabs of its (cb, kb) block, written
// at the weight's strides (bf16 or float32).  grid (9*64*64/256, CB * KB), block 64 x RG: thread
// (j, g) sums the slabs p = g, g + RG, ... of the FOUR elements 4 (64 * blockIdx.x + j) .. + 3
// (16-byte loads); the RG partials are combined in a fixed order.  RG = 4, or 16 where few
// (cb, kb) blocks face many slabs (conv1_2 / conv2_1: 256 and 128 slabs for 1 and 2 blocks —
// with four groups the 37 MB took 75 us).
template <int RG>
__global__ __launch_bounds__(64 * RG) void wrw64_reduce_kernel(const float* __restrict__ slabs,
                                                              int nsplit, int KB, int64_t sk,
                                                              int64_t sc, int64_t sh, int64_t sw,
                                                              void* __restrict__ gw, int gw_f32,
                                                              const float* __restrict__ bslabs,
                                                              float* __restrict__ gb) {
  __shared__ f32x4 red[RG][64];
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int idx = 4 * (blockIdx.x * 64 + j);           // over 9 * 64 * 64, k fastest
  const int blk = blockIdx.y, nblk = gridDim.y;        // blk = cb * KB + kb
  const int64_t stride = (int64_t)nblk * 9 * C64 * C64;
  const float* base = slabs + (int64_t)blk * 9 * C64 * C64 + idx;
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
  int i = g;
  for (; i + RG < nsplit; i += 2 * RG) {
    s0 += *reinterpret_cast<const f32x4*>(base + (int64_t)i * stride);
    s1 += *reinterpret_cast<const f32x4*>(base + (int64_t)(i + RG) * stride);
  }
  if (i < nsplit) s0 += *reinterpret_cast<const f32x4*>(base + (int64_t)i * stride);
  red[g][j] = s0 + s1;
  __syncthreads();
  if (g == 0) {
    f32x4 s = red[0][j];
#pragma unroll
    for (int q = 1; q < RG; ++q) s += red[q][j];
    const int c = 64 * (blk / KB) + ((idx >> 6) & 63), t = idx >> 12;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = 64 * (blk % KB) + ((idx + e) & 63);
      store_weight_grad(gw, k * sk + c * sc + (t / 3) * sh + (t % 3) * sw, s[e], gw_f32);
    }
  }
  // bias gradient: the blocks (0, cb = 0, kb) add up the partials of their 64 channels — slab
  // groups g, g + RG, ... in parallel, the RG partial sums combined in a fixed order (one wave
  // walking all slabs alone took 64 us of conv2_1's 70 us reduce: a dependent load per slab)
  if (gb && blockIdx.x == 0 && blk / KB == 0) {       // block-uniform
    const int K = 64 * KB, k = 64 * (blk % KB) + j;
    float acc_b = 0.f;
#pragma unroll 4
    for (int sl = g; sl < nsplit; sl += RG) acc_b += bslabs[(int64_t)sl * K + k];
    __syncthreads();                                   // red[] is free again
    reinterpret_cast<float*>(red)[g * 64 + j] = acc_b;
    __syncthreads();
    if (g == 0) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < RG; ++q) t += reinterpret_cast<float*>(red)[q * 64 + j];
      gb[k] = t;
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------
// Host side (the file's header lists the entry points and what each launches).

// A call of the weight gradient (wrw3x3_run), the entry points' arguments in scl_wrw3x3_pooled's order.
// pidx != nullptr: gz is the pooled gradient [B][H/2][W/2][kout], pidx its window positions.
struct WrwCall {
  const void *x, *gz;
  const unsigned char* pidx;
  int B, H, W, cin, kout;
  void* gw;
  int64_t sk, sc, sh, sw;       // strides of gw (elements)
  int gw_f32;
  float* grad_bias;             // [kout], or none
  void* workspace;              // scl_wrw3x3_workspace_bytes(cin, kout), 256-byte aligned
  hipStream_t stream;
};

#ifdef SCL_DIAG
// the diagnostic variants (conv_wrw_diag.hip): true when the variant owns the call, its status in *rc
static bool wrw3x3_diag(const WrwCall& c, int* rc);
#endif

// The workspace: two slabs [9][64][64] per workgroup — at most (kSclMaxConvCus CUs rounded up to whole
// (cb, kb) block sets) workgroups — then the bias partials [slab][kout] of scl_wrw3x3_bias.  Over a
// null workspace it only measures (`bytes`).
struct WrwSpace { float *slabs, *bslabs; size_t bytes; };
static WrwSpace wrw_space(void* workspace, int cin, int kout) {
  const size_t blocks = (size_t)(cin / 64) * (kout / 64);
  const size_t p = (kSclMaxConvCus + blocks - 1) / blocks;
  Carver cv(workspace);
  WrwSpace s;
  s.slabs = cv.take(2 * p * blocks * 9 * 64 * 64);
  s.bslabs = cv.take((2 * p + 2) * (size_t)kout);
  s.bytes = cv.off;
  return s;
}

extern "C" size_t scl_wrw3x3_workspace_bytes(int cin, int kout) {
  if (cin < 64 || kout < 64 || cin % 64 || kout % 64 || cin > 1024 || kout > 1024) return 0;
  return wrw_space(nullptr, cin, kout).bytes;
}

static int wrw_splits(int C, int K, int tiles, int cus) {
  const int blocks = (C / 64) * (K / 64);
  int p = (cus + blocks - 1) / blocks;                 // about one workgroup per CU
  if (p > tiles) p = tiles;
  if (p > 1024) p = 1024;
  return p < 1 ? 1 : p;
}

// How one weight gradient is cut: [64 c] x [64 nkb k] blocks, each over `splits` pixel ranges of
// `tiles` tiles — wide (8 or 4 rows x 32), or tall (32 or 16 x 8) where that pads the map less — into
// `nslab` slabs per 64 x 64 block of the `nblk`.
struct WrwPlan {
  int nkb;
  bool tall;
  int tiles, splits, nslab, nblk;
  float *slabs, *bslabs;          // bslabs: none without grad_bias
};
static WrwPlan wrw_plan(const WrwCall& c, int nkb, bool may_be_tall = true) {
  WrwPlan p;
  p.nkb = nkb;
  const int th_w = nkb == 1 ? 8 : 4, th_t = nkb == 1 ? 32 : 16;
  const int tiles_wide = c.B * ((c.H + th_w - 1) / th_w) * ((c.W + 31) / 32);
  const int tiles_tall = c.B * ((c.H + th_t - 1) / th_t) * ((c.W + 7) / 8);
  p.tall = tiles_tall < tiles_wide && may_be_tall;
  p.tiles = p.tall ? tiles_tall : tiles_wide;
  p.splits = wrw_splits(c.cin, c.kout / nkb, p.tiles, scl_conv_cus());
  p.nslab = nkb == 1 ? 2 * p.splits : p.splits;
  p.nblk = (c.cin / 64) * (c.kout / 64);
  const WrwSpace s = wrw_space(c.workspace, c.cin, c.kout);
  p.slabs = s.slabs;
  p.bslabs = c.grad_bias ? s.bslabs : nullptr;
  return p;
}

template <int DBG, int TWv, int NKB, int PL, int SCHED = 0>
void wrw_launch(const WrwPlan& p, const WrwCall& c) {
  using Cfg = WrwCfg<TWv, NKB, SCHED>;
  scl_lds_limit<&wrw64_kernel<DBG, TWv, NKB, PL, SCHED>>((int)Cfg::LDS);
  SCL_LAUNCH(PL ? "wrw64_kernel<pooled>" : "wrw64_kernel", (wrw64_kernel<DBG, TWv, NKB, PL, SCHED>),
             dim3(p.splits * (c.cin / 64) * (c.kout / (64 * NKB))), dim3(512), (Cfg::LDS), c.stream,
             (const unsigned short*)c.x, (const unsigned short*)c.gz, c.B, c.H, c.W, c.cin, c.kout, p.slabs,
             p.bslabs, c.pidx);
}
// The schedule of an instantiation (WrwCfg).  Whole tiles everywhere: in the same-box A/B of
// profiles/wrw_stagger the half-tile schedule gained on no instantiation (wide tiles equal within the
// spread, tall ones 2-8 % slower), so the product library does not contain it; the diagnostic library
// reaches it through scl_debug_set_variant(2404), and tests/test_gpu_wrw_stagger.py keeps it bit-equal.
constexpr int wrw_sched(int twv, int nkb, int pl) { return 0; }
// f(TWv, NKB, PL, SCHED), each a std::integral_constant<int, .>: wrw64_kernel takes the tile width (32
// wide, 8 tall), the k blocks, the pooled form and the schedule as template arguments
template <class F>
void for_wrw_shape(const WrwPlan& p, bool pooled, F&& f) {
  using std::integral_constant;
  auto sched = [&](auto t, auto n, auto pl) {
    f(t, n, pl, integral_constant<int, wrw_sched(decltype(t)::value, decltype(n)::value, decltype(pl)::value)>{});
  };
  auto form = [&](auto t, auto n) {
    if (!pooled) sched(t, n, integral_constant<int, 0>{}); else sched(t, n, integral_constant<int, 1>{});
  };
  auto blocks = [&](auto t) {
    if (p.nkb == 1) form(t, integral_constant<int, 1>{}); else form(t, integral_constant<int, 2>{});
  };
  if (!p.tall) blocks(integral_constant<int, 32>{}); else blocks(integral_constant<int, 8>{});
}
// the product's kernel for the plan
static void wrw_launch_planned(const WrwPlan& p, const WrwCall& c) {
  for_wrw_shape(p, c.pidx != nullptr, [&](auto t, auto n, auto pl, auto sc) {
    wrw_launch<0, decltype(t)::value, decltype(n)::value, decltype(pl)::value, decltype(sc)::value>(p, c);
  });
}

template <int RG>
void wrw_reduce_launch(const WrwPlan& p, const WrwCall& c) {
  SCL_LAUNCH("wrw64_reduce_kernel", wrw64_reduce_kernel<RG>, dim3(9 * 64 * 64 / 256, p.nblk), dim3(64 * RG), 0,
             c.stream, (const float*)p.slabs, p.nslab, c.kout / 64, c.sk, c.sc, c.sh, c.sw, c.gw,
             c.gw_f32 ? 1 : 0, (const float*)p.bslabs, c.grad_bias);
}
// slabs -> gw (+ grad_bias); 16 slab groups per element where few blocks meet many slabs
static void wrw_reduce(const WrwPlan& p, const WrwCall& c) {
  if (p.nblk <= 4 && p.nslab >= 32) wrw_reduce_launch<16>(p, c); else wrw_reduce_launch<4>(p, c);
}

static int wrw3x3_run(const WrwCall& c, size_t workspace_bytes) {
  if (!c.x || !c.gz || !c.gw || !c.workspace) return SCL_E_NULL;
  if (c.pidx && ((c.H | c.W) & 1 || (uintptr_t)c.pidx % 8)) return SCL_E_SHAPE;
  const size_t need = scl_wrw3x3_workspace_bytes(c.cin, c.kout);
  if (need == 0 || c.B < 1 || c.H < 1 || c.W < 1 || (int64_t)c.B * c.H * c.W > (int64_t)1 << 30)
    return SCL_E_SHAPE;
  if ((int64_t)c.B * c.H * c.W * (c.cin > c.kout ? c.cin : c.kout) >= (int64_t)1 << 31)
    return SCL_E_SHAPE;                                 // 32-bit element offsets in the kernel
  if (((uintptr_t)c.x % 16) || ((uintptr_t)c.gz % 16)) return SCL_E_SHAPE;
  if (!scl_aligned256(c.workspace) || workspace_bytes < need) return SCL_E_WORKSPACE;
#ifdef SCL_DIAG
  if (int rc; wrw3x3_diag(c, &rc)) return rc;
#endif
  // [64 c] x [128 k] blocks wherever the output channels allow (scl_debug_set_variant(2100)
  // pins the 64 x 64 variant)
  const int nkb = (c.kout % 128 == 0 && scl_variant() != 2100) ? 2 : 1;
  const WrwPlan p = wrw_plan(c, nkb);
  wrw_launch_planned(p, c);
  wrw_reduce(p, c);
  return scl_launch_status();
}

extern "C" int scl_wrw3x3_bias(const void* x, const void* gz, int B, int H, int W, int cin, int kout, void* gw,
    int64_t w_stride_k, int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w, int gw_f32, float* grad_bias,
    void* workspace, size_t workspace_bytes, void* stream) {
  return wrw3x3_run(WrwCall{x, gz, nullptr, B, H, W, cin, kout, gw, w_stride_k, w_stride_c, w_stride_h,
                            w_stride_w, gw_f32, grad_bias, workspace, (hipStream_t)stream}, workspace_bytes);
}

extern "C" int scl_wrw3x3_pooled(const void* x, const void* g_pooled, const void* pool_idx, int B, int H, int W,
    int cin, int kout, void* gw, int64_t w_stride_k, int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w,
    int gw_f32, float* grad_bias, void* workspace, size_t workspace_bytes, void* stream) {
  if (!pool_idx) return SCL_E_NULL;
  return wrw3x3_run(WrwCall{x, g_pooled, (const unsigned char*)pool_idx, B, H, W, cin, kout, gw, w_stride_k,
                            w_stride_c, w_stride_h, w_stride_w, gw_f32, grad_bias, workspace, (hipStream_t)stream},
                    workspace_bytes);
}

extern "C" int scl_wrw3x3_ex(const void* x, const void* gz, int B, int H, int W, int cin, int kout, void* gw,
    int64_t w_stride_k, int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w, int gw_f32, void* workspace,
    size_t workspace_bytes, void* stream) {
  return scl_wrw3x3_bias(x, gz, B, H, W, cin, kout, gw, w_stride_k, w_stride_c, w_stride_h,
                         w_stride_w, gw_f32, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int scl_wrw3x3(const void* x, const void* gz, int B, int H, int W, int cin, int kout, void* gw,
    int64_t w_stride_k, int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w, void* workspace,
    size_t workspace_bytes, void* stream) {
  return scl_wrw3x3_bias(x, gz, B, H, W, cin, kout, gw, w_stride_k, w_stride_c, w_stride_h,
                         w_stride_w, 0, nullptr, workspace, workspace_bytes, stream);
}

extern "C" size_t scl_wrw64_workspace_bytes(void) { return scl_wrw3x3_workspace_bytes(64, 64); }

extern "C" int scl_wrw64(const void* x, const void* gz, int B, int H, int W, void* gw, int64_t w_stride_k,
    int64_t w_stride_c, int64_t w_stride_h, int64_t w_stride_w, void* workspace, size_t workspace_bytes,
    void* stream) {
  return scl_wrw3x3_bias(x, gz, B, H, W, 64, 64, gw, w_stride_k, w_stride_c, w_stride_h, w_stride_w,
                         0, nullptr, workspace, workspace_bytes, stream);
}
