// tests/csrc/bq_split_host.cpp -- host build of bobyqa_dev.h's state machine in the two layouts of its
// state: one BqState per chain (the wavefront / workgroup forms, bq_host.cpp), and the split-form
// refine kernel's, the hot part (BqHot) and the cold part (BqCold) in separate allocations of exactly
// their sizes.  Both record every evaluation point and value (tests/test_bobyqa_split_state.py).
// With -DBQ_SPLIT_MAIN it is a stand-alone program that runs both layouts over a grid of starts and
// compares them -- the form the address and undefined-behaviour sanitizers are run on.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bobyqa_dev.h"
#include "bq_objectives.h"

using namespace pmvsdev;

namespace {
const double kLb[3] = {-HUGE_VAL, -23.99999, -23.99999}, kUb[3] = {HUGE_VAL, 23.99999, 23.99999};

struct Rec {
  double* pts;  // [maxrec][3] evaluation points
  double* f;    // [maxrec] values
  int maxrec, cnt;
  double eval(int kind, const double* xe) {
    const double v = bq_objective(kind, xe);
    if (cnt < maxrec) {
      for (int i = 0; i < 3; ++i) pts[3 * cnt + i] = xe[i];
      f[cnt] = v;
    }
    cnt++;
    return v;
  }
};
}  // namespace

extern "C" int bq_embed_run(int kind, const double* x0, int maxeval, double* xout, double* fout, double* pts,
                            double* frec, int maxrec, int* nrec) {
  BqState st;
  Rec R = {pts, frec, maxrec, 0};
  bq_begin(st, x0, kLb, kUb, 1e-7, maxeval);
  double f = 0.0;
  while (bq_step(st, f) == BQ_NEED_F) f = R.eval(kind, st.xeval);
  for (int i = 0; i < 3; ++i) xout[i] = st.xout[i];
  *fout = st.minf;
  *nrec = R.cnt;
  return st.rc;
}

extern "C" int bq_split_run(int kind, const double* x0, int maxeval, double* xout, double* fout, double* pts,
                            double* frec, int maxrec, int* nrec) {
  BqHot* hot = (BqHot*)malloc(sizeof(BqHot));
  BqCold* cold = (BqCold*)malloc(sizeof(BqCold));
  // nothing of either part may be read before the optimizer wrote it: the kernel's LDS and its cold
  // slots are not cleared either
  memset(hot, 0xA5, sizeof(BqHot));
  memset(cold, 0x5A, sizeof(BqCold));
  Rec R = {pts, frec, maxrec, 0};
  bq_begin(*hot, *cold, x0, kLb, kUb, 1e-7, maxeval);
  double f = 0.0;
  while (bq_step(*hot, cold, f) == BQ_NEED_F) f = R.eval(kind, hot->xeval);
  for (int i = 0; i < 3; ++i) xout[i] = cold->xout[i];
  *fout = cold->minf;
  *nrec = R.cnt;
  const int rc = hot->rc;
  free(cold);
  free(hot);
  return rc;
}

#if defined(BQ_SPLIT_MAIN)
int main() {
  enum { MAXREC = 1024 };
  static double pa[3 * MAXREC], fa[MAXREC], pb[3 * MAXREC], fb[MAXREC];
  unsigned long long rng = 0x2545F4914F6CDD1Dull;
  auto uni = [&]() {  // xorshift64*, [-1, 1)
    rng ^= rng >> 12; rng ^= rng << 25; rng ^= rng >> 27;
    return (double)((rng * 0x2545F4914F6CDD1Dull) >> 11) * (2.0 / 9007199254740992.0) - 1.0;
  };
  const int maxevals[3] = {1000, 40, 13};
  long long runs = 0, evals = 0;
  for (int kind = 0; kind < 10; ++kind)
    for (int m = 0; m < 3; ++m)
      for (int s = 0; s < 12; ++s) {
        double x0[3] = {0.0, 0.0, 0.0};
        if (s) { x0[0] = 6.0 * uni(); x0[1] = 23.99999 * uni(); x0[2] = 23.99999 * uni(); }
        double xa[3], xb[3], ma, mb;
        int na, nb;
        const int ra = bq_embed_run(kind, x0, maxevals[m], xa, &ma, pa, fa, MAXREC, &na);
        const int rb = bq_split_run(kind, x0, maxevals[m], xb, &mb, pb, fb, MAXREC, &nb);
        const int n = na < MAXREC ? na : MAXREC;
        if (ra != rb || na != nb || memcmp(xa, xb, sizeof(xa)) || memcmp(&ma, &mb, sizeof(ma)) ||
            memcmp(pa, pb, 3 * n * sizeof(double)) || memcmp(fa, fb, n * sizeof(double))) {
          fprintf(stderr, "layouts differ: kind %d maxeval %d start %d (rc %d / %d, evals %d / %d)\n", kind, maxevals[m], s,
                  ra, rb, na, nb);
          return 1;
        }
        runs++;
        evals += na;
      }
  printf("bq_split_host: %lld runs, %lld evaluations, layouts equal\n", runs, evals);
  return 0;
}
#endif
