// pmvs_brick.h -- the sparse volume's definition (include/pmvs_amd.h, pmvs_loop_brick_tsdf /
// pmvs_brick_tsdf_mesh), stated once as host + device inline functions: the voxel a fused point falls in,
// the clipped box of voxels around it, the brick grid of a volume, a brick's key and a stored voxel's
// array index.  All arithmetic is f64 from the f32 inputs, unfused (-ffp-contract=off);
// tests/test_gpu_brick_tsdf.py restates the same operations in numpy.
#pragma once
#include "pmvs_layout.h"
#include "pmvs_pixmap.h"

namespace pmvsbrick {

enum { kEdge = 8, kShift = 3, kVoxels = 512 };  // PMVS_BRICK, its log2, voxels per brick

// Selection step 2: the voxel coordinate (a whole number, as a double) of the point's component S.
PMVS_HD inline double grid_coord(float S, float origin, float voxel) {
  return pmvspix::pix_floor(((double)S - (double)origin) / (double)voxel);
}

// Selection steps 3 and 4 on one axis: false when the box [g - margin, g + margin] misses [0, dim - 1]
// (compared in double, so no g can wrap), else the clipped box.
PMVS_HD inline bool clipped_box(double g, int margin, int dim, int* lo, int* hi) {
  const double l = g - (double)margin, h = g + (double)margin, last = (double)dim - 1.0;
  if (!(h >= 0.0 && l <= last)) return false;
  *lo = l > 0.0 ? (int)l : 0;
  *hi = h < last ? (int)h : dim - 1;
  return true;
}

// The brick grid of a volume: ceil(dims / 8) per axis.
struct Grid {
  int bx, by, bz;
  PMVS_HD long long bricks() const { return (long long)bx * by * bz; }
  PMVS_HD long long key(int bi, int bj, int bk) const { return ((long long)bk * by + bj) * bx + bi; }
  PMVS_HD void brick_of(long long key, int* bi, int* bj, int* bk) const {
    *bi = (int)(key % bx), *bj = (int)((key / bx) % by), *bk = (int)(key / ((long long)bx * by));
  }
};
PMVS_HD inline int bricks_along(int dim) { return (dim + kEdge - 1) >> kShift; }
PMVS_HD inline Grid grid_of(const int* dims) { return Grid{bricks_along(dims[0]), bricks_along(dims[1]), bricks_along(dims[2])}; }

// The array index of the voxel at (li, lj, lk) in [0, 8)^3 of stored brick number `slot`.
PMVS_HD inline int local_index(int li, int lj, int lk) { return (lk * kEdge + lj) * kEdge + li; }
PMVS_HD inline long long slot_voxel(long long slot, int li, int lj, int lk) { return slot * kVoxels + local_index(li, lj, lk); }

}  // namespace pmvsbrick
