// pmvs_tsdf_voxel.h -- one voxel of the TSDF integration on the device (include/pmvs_amd.h, INTEGRATION
// steps 1-3), shared by the dense kernel (pmvs_mesh.hip, one thread per voxel of the box) and the brick
// kernel (pmvs_brick.hip, one workgroup per stored brick): both call tsdf_voxel and tsdf_store, so a voxel's
// bytes do not depend on which of the two wrote it.
#pragma once
#include <hip/hip_runtime.h>

#include "pmvs_device.h"
#include "pmvs_fuse.h"
#include "pmvs_launch.h"
#include "pmvs_mesh.h"

namespace pmvsdev {

struct TsdfMapsView {     // the range's depth map and pass flags, by value to the kernel
  const float* depth;
  const unsigned char* pass;
  const long long* off;   // count + 1: the first pixel of each target's map
  int first, count;       // views [first, first + count)
};

// The sums of voxel (i, j, k) over the range's targets.  The loop is wave-uniform: the view is read
// through scalar loads.
__device__ __forceinline__ pmvsmesh::VoxelSums tsdf_voxel(const DScene& s, const TsdfMapsView& m, const pmvs_volume& vol, float trunc,
                                                          int i, int j, int k) {
  const float C4[4] = {pmvsmesh::voxel_centre(vol.origin[0], vol.voxel, i), pmvsmesh::voxel_centre(vol.origin[1], vol.voxel, j),
                       pmvsmesh::voxel_centre(vol.origin[2], vol.voxel, k), 1.0f};
  pmvsmesh::VoxelSums v;
  for (int t = 0; t < m.count; ++t) {
    const DView& vw = s.views[m.first + t];
    const int W = vw.w[s.level], H = vw.h[s.level];
    float ic[3];
    project(vw, C4, s.level, ic);
    int px, py;
    if (!pmvsfuse::pixel_at(ic[0], ic[1], W, H, &px, &py)) continue;  // the guard of every index below
    const long long p = (long long)py * W + px;
    const long long q = m.off[t] + p;
    if (!m.pass[q]) continue;
    const float z = depth_of(vw, C4);
    double sd;
    if (!(z > 0.0f) || !pmvsmesh::observes(m.depth[q], z, trunc, &sd)) continue;
    v.sum += pmvsmesh::tsdf_value(sd, trunc);
    ++v.n;
    if (pmvsmesh::in_band(sd, trunc)) {
      const uint32_t w = s.pyr[vw.pyr_off[s.level] + p];
      v.c[0] += (int)(w & 0xff), v.c[1] += (int)((w >> 8) & 0xff), v.c[2] += (int)((w >> 16) & 0xff);
      ++v.nc;
    }
  }
  return v;
}

// Step 3 into the requested arrays at element `idx`.  Sums that observed nothing give (1.0f, 0, 0).
__device__ __forceinline__ void tsdf_store(const TsdfArrays& out, long long idx, const pmvsmesh::VoxelSums& v) {
  if (out.tsdf) out.tsdf[idx] = pmvsmesh::tsdf_of(v);
  if (out.obs) out.obs[idx] = pmvsmesh::obs_of(v);
  if (out.color) {
    uchar4 c = make_uchar4(0, 0, 0, 0);
    if (v.nc) c = make_uchar4(pmvsmesh::colour_of(v, 0), pmvsmesh::colour_of(v, 1), pmvsmesh::colour_of(v, 2), 255);
    reinterpret_cast<uchar4*>(out.color)[idx] = c;
  }
}

}  // namespace pmvsdev
