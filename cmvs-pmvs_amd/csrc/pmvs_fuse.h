// pmvs_fuse.h -- the fusion's definition (include/pmvs_amd.h, pmvs_loop_fuse), stated once as host +
// device inline functions: the point a filled pixel stands for, the pixel that point falls on in another
// target, and the depth and normal tests between the two.  All arithmetic is f64 from the f32 inputs,
// unfused (-ffp-contract=off), in the order written here; tests/test_gpu_fuse.py restates the same
// operations in numpy.  The projection itself is pmvs_device.h's f32 project / depth_of.
#pragma once
#include "pmvs_layout.h"
#include "pmvs_pixmap.h"

namespace pmvsfuse {

// The point S on the ray of pixel (u, v) of the view with projection P (3 x 4, row-major, at the maps'
// level) and optical axis `oaxis` whose depth OpticalAxis * (S, 1) is d, rounded to f32: the operations of
// pmvspix::pixel_depth's solve with the optical axis in the normal's place.  False when a component is
// not finite (the pixel is then not valid).
PMVS_HD inline bool pixel_point(const float* P, const float* oaxis, int u, int v, float d, float* Sf) {
  const double du = (double)u, dv = (double)v;
  const double a0 = (double)P[0] - du * (double)P[8], a1 = (double)P[1] - du * (double)P[9];
  const double a2 = (double)P[2] - du * (double)P[10], aw = (double)P[3] - du * (double)P[11];
  const double b0 = (double)P[4] - dv * (double)P[8], b1 = (double)P[5] - dv * (double)P[9];
  const double b2 = (double)P[6] - dv * (double)P[10], bw = (double)P[7] - dv * (double)P[11];
  const double c0 = oaxis[0], c1 = oaxis[1], c2 = oaxis[2];
  // [a; b; c] S = (-aw, -bw, d - oaxis3) by Cramer's rule
  const double bc0 = b1 * c2 - b2 * c1, bc1 = b2 * c0 - b0 * c2, bc2 = b0 * c1 - b1 * c0;  // b x c
  const double ca0 = c1 * a2 - c2 * a1, ca1 = c2 * a0 - c0 * a2, ca2 = c0 * a1 - c1 * a0;  // c x a
  const double ab0 = a1 * b2 - a2 * b1, ab1 = a2 * b0 - a0 * b2, ab2 = a0 * b1 - a1 * b0;  // a x b
  const double det = a0 * bc0 + a1 * bc1 + a2 * bc2;
  const double r0 = -aw, r1 = -bw, r2 = (double)d - (double)oaxis[3];
  Sf[0] = (float)((r0 * bc0 + r1 * ca0 + r2 * ab0) / det);
  Sf[1] = (float)((r0 * bc1 + r1 * ca1 + r2 * ab1) / det);
  Sf[2] = (float)((r0 * bc2 + r1 * ca2 + r2 * ab2) / det);
  return pmvspix::pix_finite(Sf[0]) && pmvspix::pix_finite(Sf[1]) && pmvspix::pix_finite(Sf[2]);
}

// The pixel of a W x H image the projection (x, y) (CCamera::project's f32 values) falls on.  Compared in
// double, so project's clamped values cannot wrap and a NaN gives no pixel.
PMVS_HD inline bool pixel_at(float x, float y, int W, int H, int* px, int* py) {
  const double cx = pmvspix::pix_floor((double)x + 0.5), cy = pmvspix::pix_floor((double)y + 0.5);
  if (!(cx >= 0.0 && cx <= (double)W - 1.0 && cy >= 0.0 && cy <= (double)H - 1.0)) return false;
  *px = (int)cx;
  *py = (int)cy;
  return true;
}

// ds: the depth stored at the pixel, zs: the point's own depth in that view.
PMVS_HD inline bool depth_consistent(float ds, float zs, float depth_rel) {
  return zs > 0.0f && __builtin_fabs((double)ds - (double)zs) <= (double)depth_rel * (double)zs;
}

// The two normals as stored (no normalisation).
PMVS_HD inline bool normal_consistent(const float* n, const float* m, float normal_cos) {
  return (double)n[0] * (double)m[0] + (double)n[1] * (double)m[1] + (double)n[2] * (double)m[2] >= (double)normal_cos;
}

}  // namespace pmvsfuse
