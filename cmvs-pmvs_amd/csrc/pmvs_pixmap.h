// pmvs_pixmap.h -- the per-pixel maps' definition (include/pmvs_amd.h, pmvs_loop_pixel_maps), stated
// once as host + device inline functions: the footprint of a projected patch and the depth it gives
// one pixel.  All arithmetic is f64 from the f32 inputs, unfused (-ffp-contract=off), in the order
// written here; tests/test_gpu_pixel_maps.py restates the same operations in numpy.
#pragma once
#include "pmvs_layout.h"

namespace pmvspix {

// The footprint of a patch projected to (x, y) (CCamera::project's f32 values) in a W x H image: the
// pixels [x0, x1] x [y0, y1], and the centre pixel (cx, cy).  Compared in double, so project's
// clamped values (+-2^31, -65535 behind the camera) cannot wrap and a NaN gives no footprint.
struct Footprint {
  int cx, cy, x0, x1, y0, y1;
};
PMVS_HD inline double pix_floor(double v) { return __builtin_floor(v); }
PMVS_HD inline bool footprint(float x, float y, int W, int H, int R, Footprint* f) {
  const double cx = pix_floor((double)x + 0.5), cy = pix_floor((double)y + 0.5);
  if (!(cx + (double)R >= 0.0 && cx - (double)R <= (double)W - 1.0)) return false;
  if (!(cy + (double)R >= 0.0 && cy - (double)R <= (double)H - 1.0)) return false;
  // here cx is in [-R, W - 1 + R] and cy in [-R, H - 1 + R]: exact as ints
  f->cx = (int)cx;
  f->cy = (int)cy;
  f->x0 = f->cx - R < 0 ? 0 : f->cx - R;
  f->x1 = f->cx + R > W - 1 ? W - 1 : f->cx + R;
  f->y0 = f->cy - R < 0 ? 0 : f->cy - R;
  f->y1 = f->cy + R > H - 1 ? H - 1 : f->cy + R;
  return f->x0 <= f->x1 && f->y0 <= f->y1;
}

PMVS_HD inline bool pix_finite(float d) { return d - d == 0.0f; }

// The depth a patch (centre X, normal N, flat depth z = OpticalAxis * X) gives pixel (u, v) of the view
// with projection P (3 x 4, row-major, at the maps' level), optical centre `centre` and optical axis
// `oaxis`: where the patch faces the camera within ~75.5 degrees, OpticalAxis * S for the point S in
// which the pixel's ray meets the patch's plane; otherwise, or when that is not a finite positive
// number, z.
PMVS_HD inline float pixel_depth(const float* P, const float* centre, const float* oaxis, const float* X,
                                 const float* N, int u, int v, float z) {
  const double n0 = N[0], n1 = N[1], n2 = N[2];
  const double x0 = X[0], x1 = X[1], x2 = X[2];
  const double v0 = (double)centre[0] - x0, v1 = (double)centre[1] - x1, v2 = (double)centre[2] - x2;
  const double nv = n0 * v0 + n1 * v1 + n2 * v2;
  const double nn = n0 * n0 + n1 * n1 + n2 * n2;
  const double vv = v0 * v0 + v1 * v1 + v2 * v2;
  if (!(nv > 0.0 && nv * nv >= 0.0625 * (nn * vv))) return z;
  // the ray of pixel (u, v): a . (S, 1) = 0 and b . (S, 1) = 0
  const double du = (double)u, dv = (double)v;
  const double a0 = (double)P[0] - du * (double)P[8], a1 = (double)P[1] - du * (double)P[9];
  const double a2 = (double)P[2] - du * (double)P[10], aw = (double)P[3] - du * (double)P[11];
  const double b0 = (double)P[4] - dv * (double)P[8], b1 = (double)P[5] - dv * (double)P[9];
  const double b2 = (double)P[6] - dv * (double)P[10], bw = (double)P[7] - dv * (double)P[11];
  // [a; b; N] S = (-aw, -bw, N . X) by Cramer's rule
  const double bn0 = b1 * n2 - b2 * n1, bn1 = b2 * n0 - b0 * n2, bn2 = b0 * n1 - b1 * n0;  // b x N
  const double na0 = n1 * a2 - n2 * a1, na1 = n2 * a0 - n0 * a2, na2 = n0 * a1 - n1 * a0;  // N x a
  const double ab0 = a1 * b2 - a2 * b1, ab1 = a2 * b0 - a0 * b2, ab2 = a0 * b1 - a1 * b0;  // a x b
  const double det = a0 * bn0 + a1 * bn1 + a2 * bn2;
  const double r0 = -aw, r1 = -bw, r2 = n0 * x0 + n1 * x1 + n2 * x2;
  const double s0 = (r0 * bn0 + r1 * na0 + r2 * ab0) / det;
  const double s1 = (r0 * bn1 + r1 * na1 + r2 * ab1) / det;
  const double s2 = (r0 * bn2 + r1 * na2 + r2 * ab2) / det;
  const float d = (float)((double)oaxis[0] * s0 + (double)oaxis[1] * s1 + (double)oaxis[2] * s2 + (double)oaxis[3]);
  return (pix_finite(d) && d > 0.0f) ? d : z;
}

}  // namespace pmvspix
