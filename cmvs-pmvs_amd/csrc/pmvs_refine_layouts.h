// pmvs_refine_layouts.h -- the refine kernel layouts this build instantiates, in one table: what a
// PMVS_REFINE_CONFIG / PMVS_REFINE_LARGE_CONFIG / PMVS_REFINE_SMALL_CONFIG number means (parse) and which
// layout a batch runs once the scene's wsize and tau are known (resolve).  No kernels and nothing of
// HIP: the launchers (pmvs_kernels.hip, pmvs_refine_split.hip, pmvs_refine_lane.hip) expand their
// switches from the lists below, and tests/csrc/refine_layouts_test.cpp checks the table on the host.
//
// The numbering:
//   wavefront form (refine_v2_kernel)    TSLOTS * 100 + NC
//       TSLOTS texture slots per objective chunk, NC optimizer chains per wavefront
//   split form (refine_split_kernel)     200000 + LP * 10000 + G * 1000 + CG
//       LP lanes per texture in the evaluators (0 reads as 1), G optimizer wavefronts of the 8,
//       CG chains per optimizer wavefront; wsize 5 and 7 only
//   lane form (refine_lane_kernel)       300000 + LP
//       LP lanes per texture (4: up to 16 textures per request, 8: up to 8); 300000 itself is no
//       layout but "LP from the scene's tau"
// Every split layout has a bit-exact GPU case (tests/refine_configs.py; tests/test_refine_layouts.py
// compares that list with this table), so a layout cannot be instantiated without one.
#pragma once

namespace pmvsdev {

#define PMVS_WAVE_LAYOUTS(X) X(12, 6) X(24, 8)
// The chains a CU holds (G * CG) are bounded by LDS alone: 1512 B of BqHot and 142 B of tables per
// chain allow 96 (6 x 16, 5 x 19, 7 x 13).
#define PMVS_SPLIT_LAYOUTS(X)                                                                               \
  X(0, 2, 32) X(2, 4, 16) X(2, 5, 16) X(2, 5, 19) X(2, 6, 14) X(2, 6, 15) X(2, 6, 16) X(2, 7, 12) X(2, 7, 13) \
  X(2, 8, 10) X(4, 5, 16) X(4, 6, 14) X(4, 8, 10)
#define PMVS_LANE_LAYOUTS(X) X(8) X(4)

constexpr int wave_config(int tslots, int nc) { return tslots * 100 + nc; }
constexpr int split_config(int lp, int g, int cg) { return 200000 + lp * 10000 + g * 1000 + cg; }
constexpr int lane_config(int lp) { return 300000 + lp; }
constexpr int kLaneAuto = lane_config(0);  // lanes per texture from tau

enum class RefineForm { Wave, Split, Lane };
struct RefineLayout {
  RefineForm form = RefineForm::Wave;
  int config = 0;  // the layout's number
  int tslots = 0;  // wavefront form
  int nc = 0;      // wavefront form: chains per wavefront
  int lp = 0;      // split and lane forms: lanes per texture (split: as encoded, 0 reads as 1; lane: 0 = from tau)
  int g = 0;       // split form: optimizer wavefronts
  int cg = 0;      // split form: chains per optimizer wavefront
  int grid_div = 1;  // resolve: the wavefront form's persistent grid is divided by this
};

constexpr RefineLayout wave_layout(int tslots, int nc) {
  return {RefineForm::Wave, wave_config(tslots, nc), tslots, nc, 0, 0, 0, 1};
}
constexpr RefineLayout split_layout(int lp, int g, int cg) {
  return {RefineForm::Split, split_config(lp, g, cg), 0, 0, lp, g, cg, 1};
}
constexpr RefineLayout lane_layout(int lp) { return {RefineForm::Lane, lane_config(lp), 0, 0, lp, 0, 0, 1}; }

constexpr RefineLayout kWaveDefault = wave_layout(12, 6);  // 19.5 KB LDS: 8 wavefronts per CU
constexpr RefineLayout kWaveWide = wave_layout(24, 8);     // 39 KB LDS: 4 per CU; holds any tau <= 16

// Exactly the listed configs (and kLaneAuto); false leaves `out` alone.
inline bool parse(int config, RefineLayout& out) {
  switch (config) {
#define PMVS_CASE(TS, NC) \
  case wave_config(TS, NC): out = wave_layout(TS, NC); return true;
    PMVS_WAVE_LAYOUTS(PMVS_CASE)
#undef PMVS_CASE
#define PMVS_CASE(LP, G, CG) \
  case split_config(LP, G, CG): out = split_layout(LP, G, CG); return true;
    PMVS_SPLIT_LAYOUTS(PMVS_CASE)
#undef PMVS_CASE
#define PMVS_CASE(LP) \
  case lane_config(LP): out = lane_layout(LP); return true;
    PMVS_LANE_LAYOUTS(PMVS_CASE)
#undef PMVS_CASE
    case kLaneAuto: out = lane_layout(0); return true;
    default: return false;
  }
}

// The layout a batch runs, from the one asked for and the scene's wsize and tau (<= 16):
//   * lane form: 300000 takes 8 lanes per texture up to tau = 8 and 4 above; 8 lanes per texture hold 8
//     textures, so 300008 at tau > 8 runs with 4;
//   * split form at wsize 9 (a texture's 3 * 81 samples exceed the evaluator's registers): the wavefront
//     form's default 1206;
//   * wavefront form whose TSLOTS < tau (a request's textures must fit one chunk), the 1206 of the rule
//     above included: 2408 on half the persistent grid (at least one workgroup).
inline RefineLayout resolve(RefineLayout l, int wsize, int tau) {
  if (l.form == RefineForm::Lane) {
    int lp = l.lp ? l.lp : (tau <= 8 ? 8 : 4);
    if (64 / lp < tau) lp = 4;
    return lane_layout(lp);
  }
  if (l.form == RefineForm::Split && wsize > 7) l = kWaveDefault;
  if (l.form == RefineForm::Wave && l.tslots < tau) {
    l = kWaveWide;
    l.grid_div = 2;
  }
  return l;
}

}  // namespace pmvsdev
