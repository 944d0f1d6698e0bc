// pmvs_texmesh.h -- the mesh raster's and the view selection's definition (include/pmvs_amd.h,
// pmvs_mesh_raster / pmvs_mesh_texture / pmvs_write_ply_texmesh_binary), stated once as host + device
// inline functions: when a projected face is drawn, the pixels of its clipped box, the coverage and the
// depth of one pixel, the front-facing test, a corner's visibility, the score, and the writer's texture
// coordinates.  All arithmetic is f64 from the f32 inputs, unfused (-ffp-contract=off), sums left to
// right in the order written here; tests/test_gpu_mesh_raster.py restates the same operations in numpy.
// The projection itself is pmvs_device.h's f32 project / depth_of.
#pragma once
#include "pmvs_layout.h"
#include "pmvs_pixmap.h"

namespace pmvstex {

// One corner of a face in one target: project's (x, y) at the scene's level and depth_of's z.
struct Corner {
  float x, y, z;
};

PMVS_HD inline bool tex_finite(double d) { return d - d == 0.0; }

// A.1: the face is drawn iff the three depths are finite and positive, the six coordinates finite and
// the doubled signed area A finite and not zero.  *A is set whenever the corners pass.
PMVS_HD inline bool face_drawn(const Corner* c, double* A) {
  for (int k = 0; k < 3; ++k)
    if (!(pmvspix::pix_finite(c[k].z) && c[k].z > 0.0f && pmvspix::pix_finite(c[k].x) && pmvspix::pix_finite(c[k].y))) return false;
  const double a = ((double)c[1].x - (double)c[0].x) * ((double)c[2].y - (double)c[0].y) -
                   ((double)c[1].y - (double)c[0].y) * ((double)c[2].x - (double)c[0].x);
  *A = a;
  return tex_finite(a) && a != 0.0;
}

// A.2: the integer pixels [u0, u1] x [v0, v1] of a drawn face's bounding box clipped to the W x H image;
// false when it is empty.  Compared in double, so project's clamped +-2^31 cannot wrap.
struct Box {
  int u0, u1, v0, v1;
};
PMVS_HD inline bool face_box(const Corner* c, int W, int H, Box* b) {
  double xlo = c[0].x, xhi = c[0].x, ylo = c[0].y, yhi = c[0].y;
  for (int k = 1; k < 3; ++k) {
    const double x = c[k].x, y = c[k].y;
    xlo = x < xlo ? x : xlo, xhi = x > xhi ? x : xhi;
    ylo = y < ylo ? y : ylo, yhi = y > yhi ? y : yhi;
  }
  double u0 = __builtin_ceil(xlo), u1 = __builtin_floor(xhi), v0 = __builtin_ceil(ylo), v1 = __builtin_floor(yhi);
  u0 = u0 < 0.0 ? 0.0 : u0, v0 = v0 < 0.0 ? 0.0 : v0;
  u1 = u1 > (double)W - 1.0 ? (double)W - 1.0 : u1, v1 = v1 > (double)H - 1.0 ? (double)H - 1.0 : v1;
  if (!(u0 <= u1 && v0 <= v1)) return false;
  // here all four lie in [0, W - 1] or [0, H - 1]: exact as ints
  b->u0 = (int)u0, b->u1 = (int)u1, b->v0 = (int)v0, b->v1 = (int)v1;
  return true;
}
PMVS_HD inline long long box_pixels(const Box& b) { return (long long)(b.u1 - b.u0 + 1) * (long long)(b.v1 - b.v0 + 1); }

// A.3 and A.4: whether the face covers integer pixel (u, v), and the depth it gives it.  False when the
// pixel is not covered or the depth is not a finite positive number.
PMVS_HD inline bool face_pixel_depth(const Corner* c, double A, int u, int v, float* d) {
  const double du = (double)u, dv = (double)v;
  const double x0 = c[0].x, y0 = c[0].y, x1 = c[1].x, y1 = c[1].y, x2 = c[2].x, y2 = c[2].y;
  const double w0 = (x2 - x1) * (dv - y1) - (y2 - y1) * (du - x1);
  const double w1 = (x0 - x2) * (dv - y2) - (y0 - y2) * (du - x2);
  const double w2 = (x1 - x0) * (dv - y0) - (y1 - y0) * (du - x0);
  const bool covered = A > 0.0 ? (w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0) : (w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0);
  if (!covered) return false;
  const double l0 = w0 / A, l1 = w1 / A, l2 = w2 / A;
  const double inv = l0 / (double)c[0].z + l1 / (double)c[1].z + l2 / (double)c[2].z;
  const float r = (float)(1.0 / inv);
  *d = r;
  return pmvspix::pix_finite(r) && r > 0.0f;
}

// B.2: N = (V1 - V0) x (V2 - V0), and N . (centre - V0) > 0.
PMVS_HD inline bool face_front(const float* V0, const float* V1, const float* V2, const float* centre) {
  const double a0 = (double)V1[0] - (double)V0[0], a1 = (double)V1[1] - (double)V0[1], a2 = (double)V1[2] - (double)V0[2];
  const double b0 = (double)V2[0] - (double)V0[0], b1 = (double)V2[1] - (double)V0[1], b2 = (double)V2[2] - (double)V0[2];
  const double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
  const double c0 = (double)centre[0] - (double)V0[0], c1 = (double)centre[1] - (double)V0[1], c2 = (double)centre[2] - (double)V0[2];
  return n0 * c0 + n1 * c1 + n2 * c2 > 0.0;
}

// B.3: a corner of depth z against the raster's pixel it falls on (empty, or filled at depth dq).
PMVS_HD inline bool corner_visible(float z, bool empty, float dq, float depth_rel) {
  return empty || (double)z - (double)dq <= (double)depth_rel * (double)z;
}

// B.4: the projected area in pixels^2.
PMVS_HD inline float face_score(double A) { return (float)(0.5 * __builtin_fabs(A)); }

// C: the texture coordinates of pixel position (x, y) in a W0 x H0 image: pixel centres at integers, V up.
PMVS_HD inline float tex_clamp01(double t) { return (float)(t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t)); }
PMVS_HD inline float tex_u(float x, int W0) { return tex_clamp01(((double)x + 0.5) / (double)W0); }
PMVS_HD inline float tex_v(float y, int H0) { return tex_clamp01(1.0 - ((double)y + 0.5) / (double)H0); }

}  // namespace pmvstex
