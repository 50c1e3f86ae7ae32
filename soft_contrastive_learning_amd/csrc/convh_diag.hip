// LDS-weights 3x3 convolution on the 16x16x32 MFMA, DIAGNOSTIC BUILD ONLY (csrc/Makefile:
// libscl_hip_diag.so, -DSCL_DIAG): the kernel instantiations the product launcher in convh.hip never
// launches, reachable through scl_debug_set_variant (50000 + v pins this kernel for any v):
//   3012          12-row blocks cut 4 x 2 waves (HCfg<12>), the A/B partner of the product's 2 x 4
//   3024 .. 3031  clock stamps of wave v - 3024, 2 x 4 cut (bias + ReLU forward on 12-row blocks;
//   3032 .. 3039  ... of wave v - 3032, 4 x 2 cut      scripts/convh_stamps.py, STAMP in convh.hip)
// convh_launch calls convh_diag once the block height and the grid are known; it returns false for
// every other variant, and the product launch runs.
#include "convh.hip"

static bool convh_diag(const LdsConvCall& c, const HGeom& g, int* rc) {
  const int dv = c.dv;
  const bool stamps = dv >= 3024 && dv < 3040 && c.bias && !c.mask && !c.pidx && g.bh == 12;
  if (dv != 3012 && !stamps) return false;
  if (dv == 3012)
    convh_epilogue<12>(c, g, 0);
  else if (dv < 3032)
    convh_run<1, 24, true>(c, g, (c.relu ? 1 : 0) | ((dv - 3024) << 4));
  else
    convh_run<1, 12, true>(c, g, (c.relu ? 1 : 0) | ((dv - 3032) << 4));
  *rc = scl_launch_status();
  return true;
}
