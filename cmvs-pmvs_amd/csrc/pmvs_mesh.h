// pmvs_mesh.h -- the meshing's definition (include/pmvs_amd.h, pmvs_loop_tsdf / pmvs_tsdf_mesh), stated
// once as host + device inline functions: a voxel's centre, one target's observation of it, and the
// vertex, normal and colour naive surface nets gives an active cell.  All arithmetic is f64 from the f32
// inputs, unfused (-ffp-contract=off), sums left to right in the order written here;
// tests/test_gpu_tsdf.py and tests/test_gpu_mesh.py restate the same operations in numpy.
#pragma once
#include "pmvs_layout.h"

namespace pmvsmesh {

// Coordinate `a` of the point at (idx + 0.5 + m) voxels from the origin: a voxel's centre with m = 0, a
// cell's vertex with m = the mean crossing point in cell units.
PMVS_HD inline float voxel_coord(float origin, float voxel, int idx, double m) {
  return (float)((double)origin + ((double)idx + 0.5 + m) * (double)voxel);
}
PMVS_HD inline float voxel_centre(float origin, float voxel, int idx) {
  return (float)((double)origin + ((double)idx + 0.5) * (double)voxel);
}

// One voxel's sums over the targets that observe it.
struct VoxelSums {
  double sum = 0.0;
  int n = 0, nc = 0;
  int c[3] = {0, 0, 0};
};

// The signed distance s = d - z along the ray (d: the depth stored at the pixel, z: the voxel's own):
// whether the target observes the voxel at all (not hidden behind the surface by more than trunc) ...
PMVS_HD inline bool observes(float d, float z, float trunc, double* s) {
  *s = (double)d - (double)z;
  return *s >= -(double)trunc;
}
// ... the value it contributes, and whether the voxel lies in the band, where it takes the pixel's colour.
PMVS_HD inline double tsdf_value(double s, float trunc) { return s >= (double)trunc ? 1.0 : s / (double)trunc; }
PMVS_HD inline bool in_band(double s, float trunc) { return s < (double)trunc; }

PMVS_HD inline float tsdf_of(const VoxelSums& v) { return v.n ? (float)(v.sum / (double)v.n) : 1.0f; }
PMVS_HD inline unsigned char obs_of(const VoxelSums& v) { return (unsigned char)(v.n < 255 ? v.n : 255); }
PMVS_HD inline unsigned char colour_of(const VoxelSums& v, int ch) { return (unsigned char)((v.c[ch] + v.nc / 2) / v.nc); }

// ---- naive surface nets.  A cell's corner c is the voxel at offsets (c & 1, (c >> 1) & 1, c >> 2); its
// 12 edges are axis a = e / 4 with the offsets (e & 1, (e >> 1) & 1) along the next two axes of the
// cyclic order (x, y, z), from the lower corner to the upper one.
PMVS_HD inline int edge_lower_corner(int e) {
  const int a = e >> 2, b = (a + 1) % 3, c = (a + 2) % 3;
  return ((e & 1) << b) | (((e >> 1) & 1) << c);
}

PMVS_HD inline bool cell_active(const bool* observed, const bool* inside) {
  bool all = true, any_in = false, any_out = false;
  for (int c = 0; c < 8; ++c) {
    all = all && observed[c];
    any_in = any_in || inside[c];
    any_out = any_out || !inside[c];
  }
  return all && any_in && any_out;
}

// The mean crossing point m (cell units) and the unit gradient of an active cell with corner values v[8].
PMVS_HD inline void cell_vertex(const float* v, double* m, float* normal) {
  double sum[3] = {0.0, 0.0, 0.0}, g[3];
  int count = 0;
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    double ga = 0.0;
    for (int k = 0; k < 4; ++k) {
      const int lo = edge_lower_corner(4 * a + k), hi = lo | (1 << a);
      const double v0 = v[lo], v1 = v[hi];
      ga = k ? ga + (v1 - v0) : v1 - v0;
      if ((v[lo] < 0.0f) != (v[hi] < 0.0f)) {
        double p[3];
        p[a] = v0 / (v0 - v1);
        p[b] = (double)(k & 1);
        p[c] = (double)((k >> 1) & 1);
        sum[0] += p[0], sum[1] += p[1], sum[2] += p[2];
        ++count;
      }
    }
    g[a] = ga;
  }
  for (int a = 0; a < 3; ++a) m[a] = sum[a] / (double)count;
  const double len = __builtin_sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  const bool ok = len > 0.0 && len - len == 0.0;
  for (int a = 0; a < 3; ++a) normal[a] = ok ? (float)(g[a] / len) : 0.0f;
}

// The rounded mean of the corners that have a colour (A = 255), RGBA per corner.
PMVS_HD inline void cell_colour(const unsigned char (*rgba)[4], unsigned char* out) {
  int s[3] = {0, 0, 0}, m = 0;
  for (int c = 0; c < 8; ++c)
    if (rgba[c][3] == 255) {
      s[0] += rgba[c][0], s[1] += rgba[c][1], s[2] += rgba[c][2];
      ++m;
    }
  for (int ch = 0; ch < 3; ++ch) out[ch] = (unsigned char)(m ? (s[ch] + m / 2) / m : 0);
}

}  // namespace pmvsmesh
