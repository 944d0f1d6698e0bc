// pmvs_atlas.h -- the texture atlas's definition (include/pmvs_amd.h, pmvs_mesh_atlas /
// pmvs_atlas_layout_from_counts), stated once as host + device inline functions: when a face is placed, the
// side of its triangle, the bands of the classes, the texel -> (rank in its class, half, barycentric
// weights) map, the triangles' corners, the surface point of a texel and the sample's clamp and rounding.
// All arithmetic is f64 from the f32 inputs, unfused (-ffp-contract=off), sums left to right in the order
// written here; tests/test_gpu_mesh_atlas.py restates the same operations in numpy.  The projection and the
// bilinear fetch themselves are pmvs_device.h's f32 project / get_color.
#pragma once
#include "pmvs_layout.h"

namespace pmvsatlas {

constexpr int kGutter = 5;  // c = n + 5: one gutter texel on each outer side, and three on the diagonal

PMVS_HD inline bool atlas_finite(double d) { return d - d == 0.0; }

// 1: the corners (x, y, w) of a face whose view is >= 0 place it iff the three w > 0 and the six
// coordinates are finite.
PMVS_HD inline bool corners_placed(const float ic[3][3]) {
  for (int k = 0; k < 3; ++k)
    if (!(ic[k][2] > 0.0f && atlas_finite(ic[k][0]) && atlas_finite(ic[k][1]))) return false;
  return true;
}

// 2: the side n of a placed face: the Chebyshev length of its longest edge in level-0 pixels, scaled.
PMVS_HD inline int face_side(const float ic[3][3], float scale, int M) {
  double e = 0.0;
  for (int a = 0; a < 3; ++a) {
    const int b = a == 2 ? 0 : a + 1;
    const double dx = __builtin_fabs((double)ic[a][0] - (double)ic[b][0]);
    const double dy = __builtin_fabs((double)ic[a][1] - (double)ic[b][1]);
    e = dx > e ? dx : e;
    e = dy > e ? dy : e;
  }
  const double s = (double)scale * e;
  if (s <= 1.0) return 1;
  if (s >= (double)M) return M;
  return (int)__builtin_ceil(s);
}

// 4: the cells per row and the rows of a class of `count` faces in an atlas W texels wide (W >= n + 5).
PMVS_HD inline int cells_per_row(int W, int n) { return W / (n + kGutter); }
PMVS_HD inline long long class_slots(long long count) { return (count >> 1) + (count & 1); }  // (count + 1) >> 1, for any count
PMVS_HD inline long long class_rows(long long count, int W, int n) {
  const long long k = cells_per_row(W, n), slots = class_slots(count);
  return slots / k + (slots % k != 0 ? 1 : 0);
}

// One non-empty class as the render kernel finds it: its first atlas row, its side, its faces and the
// position of its first face in the (class, face id) order.  The table is in layout order: n descending,
// y0 ascending.
struct Band {
  int y0, n, count, base;
};
// The band that holds atlas row J (0 <= J < H; nb >= 1): the last one that starts at or above it.
PMVS_HD inline int band_of_row(const Band* bands, int nb, int J) {
  int lo = 0, hi = nb - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bands[mid].y0 <= J) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// 5 and 6: texel (I, Jrel) of a band (Jrel = J - y0 >= 0, below the band's rows): the rank 2 * slot + half of
// its face within the class and the weights l1, l2; false when the texel is EMPTY.  Everything fits an int:
// the atlas height does, and slots * 2 <= count + 1.
struct Texel {
  int rank, half;
  double l1, l2;
};
PMVS_HD inline bool texel_of(int W, int n, int count, int I, int Jrel, Texel* t) {
  const int c = n + kGutter, k = W / c;
  const int col = I / c, i = I - col * c;
  const int crow = Jrel / c, j = Jrel - crow * c;
  if (col >= k) return false;
  const long long slot = (long long)crow * k + col;
  if (slot >= class_slots(count)) return false;
  const int half = (i + j <= n + 3) ? 0 : 1;
  const long long rank = 2 * slot + half;
  if (rank >= count) return false;  // the last slot of an odd class has no second face
  t->rank = (int)rank, t->half = half;
  if (half == 0) {
    t->l1 = (double)(i - 1) / (double)n;
    t->l2 = (double)(j - 1) / (double)n;
  } else {
    t->l1 = (double)(c - 2 - i) / (double)n;
    t->l2 = (double)(c - 2 - j) / (double)n;
  }
  return true;
}

// 4 and 5: corner k of the face of rank r in a class of side n whose band starts at row y0, in atlas texels.
PMVS_HD inline void face_corner(int W, int n, int y0, int r, int k, long long* x, long long* y) {
  const int c = n + kGutter, per_row = W / c, slot = r >> 1, half = r & 1;
  const long long ox = (long long)(slot % per_row) * c, oy = (long long)y0 + (long long)(slot / per_row) * c;
  int tx, ty;
  if (half == 0) {
    tx = k == 1 ? 1 + n : 1, ty = k == 2 ? 1 + n : 1;
  } else {
    tx = k == 1 ? c - 2 - n : c - 2, ty = k == 2 ? c - 2 - n : c - 2;
  }
  *x = ox + tx, *y = oy + ty;
}

// 6: the surface point of weights (l1, l2) on the face's plane.
PMVS_HD inline void surface_point(const float* V0, const float* V1, const float* V2, double l1, double l2, float* X) {
  const double l0 = 1.0 - l1 - l2;
  for (int a = 0; a < 3; ++a) X[a] = (float)(l0 * (double)V0[a] + l1 * (double)V1[a] + l2 * (double)V2[a]);
  X[3] = 1.0f;
}

// 6: whether the projected (x, y, w) is sampled at all, and the sample's coordinate in an image `size` wide
// or high (size >= 2): clamped to [0, size - 2] so that get_color's four texels exist.
PMVS_HD inline bool sample_ok(const float* ic) { return ic[2] > 0.0f && atlas_finite(ic[0]) && atlas_finite(ic[1]); }
PMVS_HD inline float sample_clamp(float x, int size) {
  const float hi = (float)(size - 2);
  return (double)x < 0.0 ? 0.0f : ((double)x > (double)hi ? hi : x);
}
// 6: pmvs_patch_colors' rounding of one channel.
PMVS_HD inline unsigned char color_byte(float c) {
  const int q = (int)__builtin_floor((double)(c + 0.5f));
  return (unsigned char)(q < 255 ? q : 255);
}

}  // namespace pmvsatlas
