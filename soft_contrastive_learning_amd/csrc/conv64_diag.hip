// 3x3 convolutions of the first VGG block, DIAGNOSTIC BUILD ONLY (csrc/Makefile: libscl_hip_diag.so,
// -DSCL_DIAG): the kernel instantiations the product dispatch in conv64.hip never launches, reachable
// through scl_debug_set_variant or SCL_CONV64_TWO_WG for same-box A/B timing and ablations.
//   SCL_CONV64_TWO_WG=1   conv1_2 with two 4-wave workgroups per CU (conv3x3_kernel GEO 1)
//   2001 .. 2003          wrw64_kernel timing diagnostics (DBG 2), 64 x 64 blocks, wide tiles
//   2004, 2006            wrw64_kernel clock stamps (DBG 4; 2006: DBG 6, no staging after the first tile)
//   2200                  round 4's staging without the buffer path (DBG 8): A/B partner, correct results
//   2300                  16x16x32 timing ablation (DBG 16): RESULTS MEANINGLESS
// conv64.hip calls conv3x3_diag / wrw3x3_diag after its argument checks; they return false for every
// other variant, and the product dispatch runs.
#include "conv64.hip"

// conv1_2 with two 4-wave workgroups per CU (ConvCfg GEO 1) — SCL_CONV64_TWO_WG=1.
// Round 6 measured it (scripts/conv12_geo_ab.py, profiles/r06/conv12_two_workgroups_per_cu.txt):
// bit-identical, forward 488 -> 478 us, backward-data with the un-pooling window 555 -> 686 us,
// bias + ReLU forward 510 -> 510.  Taking the tile barrier out from between the two waves of a
// SIMD does not speed the K loop up: the 8,100 cycles per tile are not the phase lock DESIGN.md
// section 7 suspected, so the product keeps the one 8-wave workgroup.
static bool conv64_two_wg() {
  static const bool on = [] {
    const char* e = getenv("SCL_CONV64_TWO_WG");
    return e && e[0] == '1';
  }();
  return on;
}


static bool conv3x3_diag(const void* x, const void* w, int64_t sk, int64_t sc, int64_t sh, int64_t sw,
                         int transposed, int B, int H, int W, int cin, int kout, void* out, const float* bias,
                         int relu, void* pooled, const void* mask, void* pidx, const void* uidx, void* workspace,
                         hipStream_t st, int* rc) {
  if (cin != 64 || kout != 64 || !conv64_two_wg()) return false;
  *rc = launch_conv3x3<64, 64, 1>(x, w, sk, sc, sh, sw, transposed, B, H, W, out, bias, relu ? 1 : 0, pooled,
                                  mask, pidx, uidx, workspace, st);
  return true;
}

// wrw3x3_run's geometry and reduction around the diagnostic instantiations of wrw64_kernel
static bool wrw3x3_diag(const void* x, const void* gz, const unsigned char* pidx, int B, int H, int W, int cin,
                        int kout, void* gw, int64_t w_stride_k, int64_t w_stride_c, int64_t w_stride_h,
                        int64_t w_stride_w, int gw_f32, float* grad_bias, void* workspace, size_t need,
                        void* stream, int* rc) {
  const int v = scl_variant();
  const int dbg = v / 1000 == 2 ? v & 3 : 0;
  const bool stamps = (v == 2004 || v == 2006) && kout % 128 == 0;   // (needs >= 64 KB of bias slabs)
  const bool ab = kout % 128 == 0 && dbg == 0 && (v == 2200 || v == 2300);
  if (dbg == 0 && !stamps && !ab) return false;
  static SclDeviceOnce once;
  scl_call_once(once, [] {
#define SCL_WRW_ATTR(D, T, N, PL)                                                              \
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&wrw64_kernel<D, T, N, PL>),         \
                            hipFuncAttributeMaxDynamicSharedMemorySize,                        \
                            (int)WrwCfg<T, N>::LDS);
    SCL_WRW_ATTR(2, 32, 1, 0)
    SCL_WRW_ATTR(4, 32, 2, 0) SCL_WRW_ATTR(4, 8, 2, 0) SCL_WRW_ATTR(4, 32, 2, 1) SCL_WRW_ATTR(4, 8, 2, 1)
    SCL_WRW_ATTR(6, 32, 2, 0) SCL_WRW_ATTR(6, 8, 2, 0)
    SCL_WRW_ATTR(8, 32, 2, 0) SCL_WRW_ATTR(8, 8, 2, 0) SCL_WRW_ATTR(8, 32, 2, 1) SCL_WRW_ATTR(8, 8, 2, 1)
    SCL_WRW_ATTR(16, 32, 2, 0) SCL_WRW_ATTR(16, 8, 2, 0) SCL_WRW_ATTR(16, 32, 2, 1) SCL_WRW_ATTR(16, 8, 2, 1)
#undef SCL_WRW_ATTR
  });
  const int cus = scl_conv_cus();
  const int nkb = kout % 128 == 0 && dbg == 0 ? 2 : 1;   // (dbg != 0: 64 x 64 blocks and wide tiles)
  const int th_w = nkb == 1 ? 8 : 4, th_t = nkb == 1 ? 32 : 16;
  const int tiles_wide = B * ((H + th_w - 1) / th_w) * ((W + 31) / 32);
  const int tiles_tall = B * ((H + th_t - 1) / th_t) * ((W + 7) / 8);
  const bool tall = tiles_tall < tiles_wide && dbg == 0;
  const int tiles = tall ? tiles_tall : tiles_wide;
  hipStream_t st = (hipStream_t)stream;
#define SCL_WRW_LAUNCH(D, T, N, PL)                                                            \
  SCL_LAUNCH(PL ? "wrw64_kernel<pooled>" : "wrw64_kernel", (wrw64_kernel<D, T, N, PL>),        \
             dim3(PP * (cin / 64) * (kout / (64 * N))), dim3(512), (WrwCfg<T, N>::LDS), st,    \
             (const unsigned short*)x, (const unsigned short*)gz, B, H, W, cin, kout,          \
             (float*)workspace, bslabs, pidx)
  float* bslabs = grad_bias ? (float*)((char*)workspace + wrw_bias_slab_offset(cin, kout)) : nullptr;
  int PP = wrw_splits(cin, kout, tiles, cus);
  if (stamps) {
    PP = wrw_splits(cin, kout / 2, tiles, cus);
    bslabs = (float*)((char*)workspace + wrw_bias_slab_offset(cin, kout));
    if ((size_t)PP * (cin / 64) * (kout / 128) * 256 > need - wrw_bias_slab_offset(cin, kout)) {
      *rc = SCL_E_WORKSPACE;
      return true;
    }
    if (v == 2006) {                    // ... without staging after the first tile
      if (tall) SCL_WRW_LAUNCH(6, 8, 2, 0); else SCL_WRW_LAUNCH(6, 32, 2, 0);
    } else if (pidx) {
      if (tall) SCL_WRW_LAUNCH(4, 8, 2, 1); else SCL_WRW_LAUNCH(4, 32, 2, 1);
    } else {
      if (tall) SCL_WRW_LAUNCH(4, 8, 2, 0); else SCL_WRW_LAUNCH(4, 32, 2, 0);
    }
    *rc = scl_launch_status();
    return true;
  }
  if (v == 2200) {                      // round 4's staging (no buffer path): A/B partner, CORRECT results
    PP = wrw_splits(cin, kout / 2, tiles, cus);
    if (pidx) {
      if (tall) SCL_WRW_LAUNCH(8, 8, 2, 1); else SCL_WRW_LAUNCH(8, 32, 2, 1);
    } else {
      if (tall) SCL_WRW_LAUNCH(8, 8, 2, 0); else SCL_WRW_LAUNCH(8, 32, 2, 0);
    }
  } else if (v == 2300) {               // 16x16x32 timing ablation: RESULTS MEANINGLESS
    PP = wrw_splits(cin, kout / 2, tiles, cus);
    if (pidx) {
      if (tall) SCL_WRW_LAUNCH(16, 8, 2, 1); else SCL_WRW_LAUNCH(16, 32, 2, 1);
    } else {
      if (tall) SCL_WRW_LAUNCH(16, 8, 2, 0); else SCL_WRW_LAUNCH(16, 32, 2, 0);
    }
  } else if (pidx) {                    // dbg != 0: the product kernel of the pooled form
    SCL_WRW_LAUNCH(0, 32, 1, 1);
  } else {
    SCL_WRW_LAUNCH(2, 32, 1, 0);
  }
#undef SCL_WRW_LAUNCH
  const int nslab = nkb == 1 ? 2 * PP : PP, nblk = (cin / 64) * (kout / 64);
#define SCL_WRW_REDUCE(RG)                                                                     \
  SCL_LAUNCH("wrw64_reduce_kernel", wrw64_reduce_kernel<RG>, dim3(9 * 64 * 64 / 256, nblk),    \
             dim3(64 * RG), 0, st, (const float*)workspace, nslab, kout / 64, w_stride_k,      \
             w_stride_c, w_stride_h, w_stride_w, gw, gw_f32 ? 1 : 0, (const float*)bslabs,     \
             grad_bias)
  if (nblk <= 4 && nslab >= 32) SCL_WRW_REDUCE(16); else SCL_WRW_REDUCE(4);
#undef SCL_WRW_REDUCE
  *rc = scl_launch_status();
  return true;
}
