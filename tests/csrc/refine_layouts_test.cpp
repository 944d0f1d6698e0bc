// Stand-alone check of the refine layout table (cmvs-pmvs_amd/csrc/pmvs_refine_layouts.h): what parse
// accepts and decodes, what it rejects, and the layout resolve picks for every wsize and tau.
// tests/test_refine_layouts.py builds and runs it and compares the printed "accepted:" line with the
// configs that have a bit-exact GPU case (tests/refine_configs.py).
// With arguments "CONFIG:WSIZE:TAU" it prints, per argument, what a scene of that wsize and tau runs when
// that number is asked for: "CONFIG WSIZE TAU -> RESOLVED GRID_DIV" (a number that names no layout is
// asked as 1206, as pmvs_scene_create reads PMVS_REFINE_CONFIG); the same test maps its GPU cases to the
// kernels they launch with it.
#include "pmvs_refine_layouts.h"

#include <climits>
#include <cstdio>
#include <cstdlib>

using namespace pmvsdev;

static int g_fail = 0;
#define CHECK(c, ...)                                                       \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "refine_layouts_test:%d: %s  [", __LINE__, #c);      \
      fprintf(stderr, __VA_ARGS__);                                         \
      fprintf(stderr, "]\n");                                               \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

// Every config the build instantiates and what its number encodes, written out by hand.
struct Want {
  int config;
  RefineForm form;
  int tslots, nc, lp, g, cg;
};
static const Want kAccepted[] = {
    {1206, RefineForm::Wave, 12, 6, 0, 0, 0},     {2408, RefineForm::Wave, 24, 8, 0, 0, 0},
    {202032, RefineForm::Split, 0, 0, 0, 2, 32},  {224016, RefineForm::Split, 0, 0, 2, 4, 16},
    {225016, RefineForm::Split, 0, 0, 2, 5, 16},  {225019, RefineForm::Split, 0, 0, 2, 5, 19},
    {226014, RefineForm::Split, 0, 0, 2, 6, 14},  {226015, RefineForm::Split, 0, 0, 2, 6, 15},
    {226016, RefineForm::Split, 0, 0, 2, 6, 16},  {227012, RefineForm::Split, 0, 0, 2, 7, 12},
    {227013, RefineForm::Split, 0, 0, 2, 7, 13},  {228010, RefineForm::Split, 0, 0, 2, 8, 10},
    {245016, RefineForm::Split, 0, 0, 4, 5, 16},  {246014, RefineForm::Split, 0, 0, 4, 6, 14},
    {248010, RefineForm::Split, 0, 0, 4, 8, 10},  {300000, RefineForm::Lane, 0, 0, 0, 0, 0},
    {300004, RefineForm::Lane, 0, 0, 4, 0, 0},    {300008, RefineForm::Lane, 0, 0, 8, 0, 0},
};
static const int kNumAccepted = sizeof(kAccepted) / sizeof(kAccepted[0]);

// Numbers earlier builds accepted: the retired wavefront layouts, the workgroup form, the
// private-state experiment's layouts, the split layouts no test pinned and the 256-thread split build's.
static const int kRetired[] = {
    804,    807,    808,    1201,   1202,   1203,   1204,   1608,                          //
    164011, 164021, 164041, 148041, 132022, 132042, 116042,                                //
    1264,   2464,   1232,   2432,   1216,   2448,   3232,   3248,   3264,   4832,   4864,  //
    226012, 236014, 247012, 288010, 204016,                                                //
    224020, 244020, 284020, 222040, 243024,
};

static bool accepted(int config) {
  for (const Want& w : kAccepted)
    if (w.config == config) return true;
  return false;
}

static void test_parse() {
  for (const Want& w : kAccepted) {
    RefineLayout l;
    CHECK(parse(w.config, l), "%d", w.config);
    CHECK(l.config == w.config && l.form == w.form && l.tslots == w.tslots && l.nc == w.nc && l.lp == w.lp &&
              l.g == w.g && l.cg == w.cg && l.grid_div == 1,
          "%d", w.config);
    for (int d = -1; d <= 1; d += 2)  // its off-by-one neighbours, unless they are layouts themselves
      if (!accepted(w.config + d)) {
        RefineLayout n = wave_layout(99, 9);
        CHECK(!parse(w.config + d, n), "%d", w.config + d);
        CHECK(n.config == wave_config(99, 9), "%d: a rejected number leaves the layout alone", w.config + d);
      }
  }
  RefineLayout l;
  for (int c : kRetired) CHECK(!parse(c, l), "%d", c);
  const int never[] = {0, -1, -1206, -225019, INT_MIN, INT_MAX, 100000, 200000, 299999, 400000};
  for (int c : never) CHECK(!parse(c, l), "%d", c);
}

// The fallback rules, written out per requested config (not through resolve's own decisions):
//   lane form: 300004 always 4 lanes per texture; 300000 and 300008 run 8 up to tau = 8 and 4 above;
//   split form: itself at wsize 5 and 7; at wsize 9 what 1206 gives;
//   1206: itself up to tau = 12, above that 2408 on half the grid;  2408: itself (tau <= 16).
static void expect(int config, int wsize, int tau, int* want_config, int* want_div) {
  *want_div = 1;
  if (config >= 300000) {
    *want_config = (config == 300004 || tau > 8) ? 300004 : 300008;
    return;
  }
  if (config >= 200000 && wsize != 9) {
    *want_config = config;
    return;
  }
  if (config == 2408) {
    *want_config = 2408;
    return;
  }
  // 1206, or a split config at wsize 9
  *want_config = tau <= 12 ? 1206 : 2408;
  *want_div = tau <= 12 ? 1 : 2;
}

static void test_resolve() {
  const int wsizes[] = {5, 7, 9};
  for (const Want& w : kAccepted)
    for (int wsize : wsizes)
      for (int tau = 1; tau <= 16; ++tau) {
        RefineLayout asked;
        if (!parse(w.config, asked)) continue;  // (reported by test_parse)
        int want_config = 0, want_div = 0;
        expect(w.config, wsize, tau, &want_config, &want_div);
        const RefineLayout got = resolve(asked, wsize, tau);
        CHECK(got.config == want_config && got.grid_div == want_div, "%d wsize %d tau %d: %d / %d, expected %d / %d",
              w.config, wsize, tau, got.config, got.grid_div, want_config, want_div);
        // what the launchers rely on: the result is a layout of the table with its own parameters, it
        // holds tau textures, and the split form never runs at wsize 9
        RefineLayout again;
        CHECK(got.config != kLaneAuto && parse(got.config, again), "%d wsize %d tau %d", w.config, wsize, tau);
        CHECK(again.form == got.form && again.tslots == got.tslots && again.nc == got.nc && again.lp == got.lp &&
                  again.g == got.g && again.cg == got.cg,
              "%d wsize %d tau %d", w.config, wsize, tau);
        if (got.form == RefineForm::Wave) CHECK(got.tslots >= tau && got.nc > 0, "%d tau %d", w.config, tau);
        if (got.form == RefineForm::Lane) CHECK(got.lp > 0 && 64 / got.lp >= tau, "%d tau %d", w.config, tau);
        if (got.form == RefineForm::Split) CHECK(wsize <= 7 && got.g > 0 && got.cg > 0, "%d wsize %d", w.config, wsize);
      }
}

// "CONFIG:WSIZE:TAU" -> one line; false for anything else, or a wsize or tau no scene has
static bool print_resolved(const char* arg) {
  char* end = nullptr;
  long v[3] = {0, 0, 0};
  for (int i = 0; i < 3; ++i) {
    v[i] = strtol(arg, &end, 10);
    if (end == arg || *end != (i < 2 ? ':' : '\0') || v[i] < 0 || v[i] > 999999) return false;
    arg = end + 1;
  }
  const int config = (int)v[0], wsize = (int)v[1], tau = (int)v[2];
  if ((wsize != 5 && wsize != 7 && wsize != 9) || tau < 1 || tau > 16) return false;
  RefineLayout asked = kWaveDefault;
  (void)parse(config, asked);
  const RefineLayout got = resolve(asked, wsize, tau);
  printf("%d %d %d -> %d %d\n", config, wsize, tau, got.config, got.grid_div);
  return true;
}

int main(int argc, char** argv) {
  test_parse();
  test_resolve();
  if (g_fail) return 1;
  if (argc > 1) {
    for (int i = 1; i < argc; ++i)
      if (!print_resolved(argv[i])) {
        fprintf(stderr, "refine_layouts_test: bad triple '%s' (CONFIG:WSIZE:TAU, wsize 5/7/9, tau 1-16)\n", argv[i]);
        return 2;
      }
    return 0;
  }
  // the accepted set as the table itself lists it (not kAccepted): every number below 400000 that parses
  printf("accepted:");
  RefineLayout l;
  for (int c = 0; c < 400000; ++c)
    if (parse(c, l)) printf(" %d", c);
  printf("\n");
  return 0;
}
