// Weight gradient of the 3x3 convolutions, DIAGNOSTIC BUILD ONLY (csrc/Makefile: libscl_hip_diag.so,
// -DSCL_DIAG): the wrw64_kernel instantiations the product dispatch in conv_wrw.hip never launches,
// reachable through scl_debug_set_variant for same-box A/B timing, ablations and clock stamps.
//   2001 .. 2003          timing diagnostics (kDbgNoRestage), 64 x 64 blocks, wide tiles: WRONG results
//   2004, 2006            clock stamps (kDbgStamps; 2006: no staging after the first tile either, full-size
//                         gradients only), whole-tile schedule (SCHED 0)
//   2008                  the clock stamps of the half-tile schedule (SCHED 1), waves 0 and 4
//   2200                  round 4's staging without the buffer path (kDbgLaneBorders): A/B partner, correct
//                         results
//   2300                  16x16x32 timing ablation (kDbgMfma16): RESULTS MEANINGLESS
//   2400, 2404            [64 c] x [128 k] blocks on the whole-tile schedule (SCHED 0: the schedule before
//                         the half-tile one) / on the half-tile schedule (SCHED 1) whatever wrw_sched
//                         picks: A/B partners, CORRECT results, bit-identical to the product's
// (2100, the product kernel pinned to 64 x 64 blocks, is a knob of wrw3x3_run itself.)
// conv_wrw.hip calls wrw3x3_diag after its argument checks; it returns false for every other variant,
// and the product dispatch runs.  It launches through the product's helpers (wrw_plan, wrw_launch,
// for_wrw_shape, wrw_reduce): what stays here is the choice of instantiation.
#include "conv_wrw.hip"

// wrw64_kernel<DBG, ., 2, ., SCHED>: [64 c] x [128 k] blocks, tile width and pooled form as planned
template <int DBG, int SCHED>
void wrw_diag_blocks128(const WrwPlan& p, const WrwCall& c) {
  for_wrw_shape(p, c.pidx != nullptr, [&](auto t, auto, auto pl, auto) {
    wrw_launch<DBG, decltype(t)::value, 2, decltype(pl)::value, SCHED>(p, c);
  });
}
// 2001 .. 2003 (the pooled form: the product kernel)
static void wrw_diag_no_restage(const WrwPlan& p, const WrwCall& c) {
  if (!c.pidx) wrw_launch<kDbgNoRestage, 32, 1, 0>(p, c); else wrw_launch_planned(p, c);
}
// 2006: the full-size form on [64 c] x [128 k] blocks, whatever the call
static void wrw_diag_stamps_no_restage(const WrwPlan& p, const WrwCall& c) {
  constexpr int D = kDbgStamps | kDbgNoRestage;
  if (!p.tall) wrw_launch<D, 32, 2, 0>(p, c); else wrw_launch<D, 8, 2, 0>(p, c);
}

// One row per variant: the launcher — with wrw64_kernel's DBG bits and its schedule — the block width the
// plan is made for, whether the slabs are reduced into gw, and whether the stamps need their area.
struct WrwVariant {
  int v;
  void (*launch)(const WrwPlan&, const WrwCall&);
  int plan_nkb;       // 2: [64 c] x [128 k] blocks — kout a multiple of 128, or the product runs — on wide
                      // or tall tiles; 1: 64 x 64 blocks on wide tiles
  bool reduce, stamps;
};
static const WrwVariant kWrwVariants[] = {
    {2001, wrw_diag_no_restage, 1, true, false},
    {2002, wrw_diag_no_restage, 1, true, false},
    {2003, wrw_diag_no_restage, 1, true, false},
    {2004, wrw_diag_blocks128<kDbgStamps, 0>, 2, false, true},
    // (tiles and split count of 64 x 64 blocks on wide tiles, for a kernel of [64 c] x [128 k] blocks)
    {2006, wrw_diag_stamps_no_restage, 1, false, true},
    {2008, wrw_diag_blocks128<kDbgStamps, 1>, 2, false, true},
    {2200, wrw_diag_blocks128<kDbgLaneBorders, 0>, 2, true, false},
    {2300, wrw_diag_blocks128<kDbgMfma16, 0>, 2, true, false},
    {2400, wrw_diag_blocks128<0, 0>, 2, true, false},
    {2404, wrw_diag_blocks128<0, 1>, 2, true, false},
};

static bool wrw3x3_diag(const WrwCall& c, int* rc) {
  const WrwVariant* row = nullptr;
  for (const WrwVariant& r : kWrwVariants)
    if (r.v == scl_variant()) row = &r;
  // (every kernel that writes stamps has [64 c] x [128 k] blocks)
  if (!row || ((row->plan_nkb == 2 || row->stamps) && c.kout % 128 != 0)) return false;
  WrwPlan p = wrw_plan(c, row->plan_nkb, row->plan_nkb == 2);
  if (row->stamps) {
    // the stamps go where the bias slabs are: [workgroup][4 tiles][8] uint64, one workgroup per split
    // and block of 128 output channels
    const WrwSpace s = wrw_space(c.workspace, c.cin, c.kout);
    p.splits = wrw_splits(c.cin, c.kout / 2, p.tiles, scl_conv_cus());
    p.bslabs = s.bslabs;
    if ((size_t)p.splits * (c.cin / 64) * (c.kout / 128) * 256 > s.bytes - (size_t)((char*)s.bslabs - (char*)s.slabs)) {
      *rc = SCL_E_WORKSPACE;
      return true;
    }
  }
  row->launch(p, c);
  if (row->reduce) wrw_reduce(p, c);
  *rc = scl_launch_status();
  return true;
}
