// 3x3 convolutions of the first VGG block, DIAGNOSTIC BUILD ONLY (csrc/Makefile: libscl_hip_diag.so,
// -DSCL_DIAG): the kernel instantiations the product dispatch in conv64.hip never launches, reachable
// through scl_debug_set_variant or SCL_CONV64_TWO_WG for same-box A/B timing and ablations.
//   SCL_CONV64_TWO_WG=1   conv1_2 with two 4-wave workgroups per CU (conv3x3_kernel GEO 1)
//   2001 .. 2003          wrw64_kernel timing diagnostics (DBG 2), 64 x 64 blocks, wide tiles
//   2004, 2006            wrw64_kernel clock stamps (DBG 4; 2006: DBG 6, no staging after the first tile),
//                         whole-tile schedule (SCHED 0)
//   2008                  the clock stamps of the half-tile schedule (SCHED 1), waves 0 and 4
//   2200                  round 4's staging without the buffer path (DBG 8): A/B partner, correct results
//   2300                  16x16x32 timing ablation (DBG 16): RESULTS MEANINGLESS
//   2400, 2404            [64 c] x [128 k] blocks on the whole-tile schedule (SCHED 0: the schedule before
//                         the half-tile one) / on the half-tile schedule (SCHED 1) whatever wrw_sched
//                         picks: A/B partners, CORRECT results, bit-identical to the product's
// conv64.hip calls conv3x3_diag / wrw3x3_diag after its argument checks; they return false for every
// other variant, and the product dispatch runs.  Both launch through the product's helpers
// (launch_conv3x3; wrw_plan, wrw_launch, wrw_reduce): what stays here is the choice of instantiation.
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

static bool wrw3x3_diag(const WrwCall& c, int* rc) {
  const int v = scl_variant();
  const int dbg = v / 1000 == 2 ? v & 3 : 0;
  const bool stamps = (v == 2004 || v == 2006 || v == 2008) && c.kout % 128 == 0;   // (needs >= 64 KB of bias slabs)
  const bool ab = c.kout % 128 == 0 && dbg == 0 && (v == 2200 || v == 2300 || v == 2400 || v == 2404);
  if (dbg == 0 && !stamps && !ab) return false;
  // (dbg != 0: 64 x 64 blocks and wide tiles)
  WrwPlan p = wrw_plan(c, c.kout % 128 == 0 && dbg == 0 ? 2 : 1, dbg == 0);
  const bool pooled = c.pidx != nullptr;
  // wrw64_kernel<DBG> on [64 c] x [128 k] blocks, tile width and pooled form as planned
  auto blocks128 = [&](auto d, auto sc) {
    for_wrw_shape(p, pooled, [&](auto t, auto, auto pl, auto) {
      wrw_launch<decltype(d)::value, decltype(t)::value, 2, decltype(pl)::value, decltype(sc)::value>(p, c);
    });
  };
  const std::integral_constant<int, 0> whole;
  const std::integral_constant<int, 1> halves;
  if (dbg != 0 && !stamps) {            // timing diagnostics (pooled form: the product kernel)
    if (!pooled) wrw_launch<2, 32, 1, 0>(p, c); else wrw_launch_planned(p, c);
  } else if (stamps) {                  // the stamps go where the bias slabs are; nothing is reduced.  (2006 has
                                        // dbg = 2: its split count is over the wide tiles of 64 x 64 blocks.)
    const WrwSpace s = wrw_space(c.workspace, c.cin, c.kout);
    p.splits = wrw_splits(c.cin, c.kout / 2, p.tiles, scl_conv_cus());
    p.bslabs = s.bslabs;
    if ((size_t)p.splits * (c.cin / 64) * (c.kout / 128) * 256 > s.bytes - (size_t)((char*)s.bslabs - (char*)s.slabs))
      *rc = SCL_E_WORKSPACE;
    else {
      if (v == 2004) blocks128(std::integral_constant<int, 4>{}, whole);
      else if (v == 2008) blocks128(std::integral_constant<int, 4>{}, halves);
      else if (!p.tall) wrw_launch<6, 32, 2, 0>(p, c);     // ... without staging after the first tile
      else wrw_launch<6, 8, 2, 0>(p, c);
      *rc = scl_launch_status();
    }
    return true;
  } else if (v == 2200) {               // round 4's staging (no buffer path): A/B partner, CORRECT results
    blocks128(std::integral_constant<int, 8>{}, whole);
  } else if (v == 2400) {               // the whole-tile schedule
    blocks128(std::integral_constant<int, 0>{}, whole);
  } else if (v == 2404) {               // the half-tile schedule
    blocks128(std::integral_constant<int, 0>{}, halves);
  } else {                              // 2300, the 16x16x32 timing ablation: RESULTS MEANINGLESS
    blocks128(std::integral_constant<int, 16>{}, whole);
  }
  wrw_reduce(p, c);
  *rc = scl_launch_status();
  return true;
}
