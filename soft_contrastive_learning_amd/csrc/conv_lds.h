// Between the front door of the LDS-weights 3x3 convolution (conv_lds.hip) and its two kernels
// (convh.hip, convg.hip): one validated call, its launchers, and the persistent grid both use.
#pragma once
#include "scl_common.h"

// A call that passed conv_lds.hip's checks.  Contract of scl_convg / scl_convg_masked /
// scl_convg_pool_idx (include/scl_hip.h): at most one of mask and pidx is set, pidx comes with bias.
// The first twelve fields are the entry points' leading arguments in their order (conv_lds.hip
// initialises those by position and every later field by name: new fields go to the END).
struct LdsConvCall {
  const void *x, *w;
  int64_t sk, sc, sh, sw;       // weight strides (elements)
  int flags;                    // SCL_CONV_TRANSPOSED | SCL_W_F32 | SCL_W_PACKED
  int B, H, W, cin, kout;
  void* out;                    // [B,H,W,kout], or the pooled map [B,H/2,W/2,kout] with pidx
  const float* bias;
  int relu;
  const void* mask;
  void *pidx, *workspace;       // workspace: scl_convg_workspace_bytes(cin, kout), 256-aligned
  int dv;                       // diagnostic variant, the kernel pin stripped (0 in the product)
  hipStream_t stream;
};

#define SCL_LOCAL __attribute__((visibility("hidden")))   // internal to the library: not exported
SCL_LOCAL int convh_launch(const LdsConvCall& c);   // v_mfma_f32_16x16x32_bf16, cin % 64 == 0 (convh.hip)
SCL_LOCAL int convg_launch(const LdsConvCall& c);   // v_mfma_f32_32x32x16_bf16, cin % 32 == 0 (convg.hip)

// bf16 per packed weight row of a 32-channel chunk in convg.hip's image (80-byte LDS rows);
// convh.hip's rows are dense, so the one workspace size serves both
constexpr int LDS_CONV_ROW = 40;

// PERSISTENT workgroups, one per usable CU (150-160 KB of LDS each): block v of a virtual grid of
// `vblocks` goes to workgroup v % gsize.  XCD-aware order: workgroups go to the 8 XCDs round-robin
// by linear id, and the kb = kout / 128 output blocks of a pixel block read the same windows — so
// they get virtual ids 8 apart (pixel blocks padded to a multiple of 8, gsize a multiple of 8 kb):
// same XCD, same moment, and their window fetches meet in that XCD's L2 instead of going out to
// the Infinity Cache once per output block.  scl_debug_set_variant(3100 + g) pins g + 1 groups of
// 8 kb (tests: several tiles per workgroup on small shapes), 3099 one tile per workgroup (A/B).
struct LdsConvGrid { int vblocks; unsigned gsize; };
static inline LdsConvGrid lds_conv_grid(int64_t pblocks, int kb, int cus, int dv) {
  const int vblocks = (int)(((pblocks + 7) / 8) * 8 * kb);
  int groups = cus / (8 * kb) > 0 ? cus / (8 * kb) : 1;
  if (dv >= 3100 && dv < 3200) groups = dv - 3100 + 1;
  int gsize = groups * 8 * kb;
  if (gsize > vblocks || dv == 3099) gsize = vblocks;
  return LdsConvGrid{vblocks, (unsigned)gsize};
}
