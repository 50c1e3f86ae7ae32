// 3x3 convolutions of the first VGG block, DIAGNOSTIC BUILD ONLY (csrc/Makefile: libscl_hip_diag.so,
// -DSCL_DIAG): the kernel instantiation the product dispatch in conv64.hip never launches, reachable
// through SCL_CONV64_TWO_WG for same-box A/B timing.
//   SCL_CONV64_TWO_WG=1   conv1_2 with two 4-wave workgroups per CU (conv3x3_kernel GEO 1)
// conv64.hip calls conv3x3_diag after its argument checks; it returns false unless the switch is set,
// and the product dispatch runs.  It launches through the product's helper (launch_conv3x3): what stays
// here is the choice of instantiation.  (The weight gradient's variants: conv_wrw_diag.hip.)
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

static bool conv3x3_diag(const RegConvCall& c, int* rc) {
  if (c.cin != 64 || c.kout != 64 || !conv64_two_wg()) return false;
  *rc = launch_conv3x3<64, 64, 1>(c);
  return true;
}
