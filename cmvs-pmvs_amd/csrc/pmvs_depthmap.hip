// pmvs_depthmap.hip -- the model's per-target depth maps, produced on the device
// (pmvs_loop_depth_maps / pmvs_depth_maps_patches, include/pmvs_amd.h).
//
// CFilter::setDepthMaps (filter.cpp:667-732) over a list of records, in the order the caller chose
// (model order, or the writers' order from export_order), as three steps:
//   depthmap_pack_kernel     per row: the record's coordinate as a float4 and, when normals or ncc are
//                            wanted, (normal x, y, z, ncc) as a second float4, both in row order -- the
//                            other kernels never touch the 1608-byte records
//   depthmap_build_kernel    one thread per (group of kTargetsPerThread targets, row): project, the up
//                            to four cells {floor, ceil}(x / csize) x {floor, ceil}(y / csize), and per
//                            cell in the grid a 64-bit atomicMin of (depth_bits(depth) << 32) | row.
//                            The smaller depth wins and, at equal depths, the smaller row: the
//                            reference replaces a cell's patch only when `depth < dtmp`, so its earlier
//                            patch stays.  The minimum does not depend on the order of the atomics.
//   depthmap_resolve_kernel  one thread per cell: every wanted output written once (empty cells too)
// The loop's own depth_map_kernel (pmvs_filter.hip) is the same computation over the filter's collect
// order into the filter's buffers; this file leaves it alone.
// Plain HIP: a scatter of atomics and two streaming kernels.
#include <hip/hip_runtime.h>

#include <climits>

#include "pmvs_device.h"
#include "pmvs_launch.h"

namespace pmvsdev {
namespace {

#define DCHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

constexpr int kTargetsPerThread = 4;  // the row's coordinate is read once for them (as the loop's kernel)
constexpr unsigned long long kEmpty = ~0ull;  // no row: depth_bits of a row's key never has all 64 bits set (row < 2^31)

__global__ __launch_bounds__(256) void depthmap_pack_kernel(const pmvs_patch* __restrict__ P, const int* __restrict__ src,
                                                            int n, float4* __restrict__ coordc, float4* __restrict__ attrc) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const pmvs_patch* q = P + (src ? src[r] : r);
  coordc[r] = make_float4(q->coord[0], q->coord[1], q->coord[2], q->coord[3]);
  if (attrc) attrc[r] = make_float4(q->normal[0], q->normal[1], q->normal[2], q->ncc);
}

// setDepthMapsThread (filter.cpp:687-732).  project clamps its result to the int range and sends a
// point behind the camera to -65535, so xs / ys are defined ints; the in-grid test guards every
// access to the maps.
__global__ __launch_bounds__(256) void depthmap_build_kernel(DScene s, const float4* __restrict__ coordc, int n,
                                                             const long long* __restrict__ off,
                                                             unsigned long long* __restrict__ keys) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int ngrp = (s.tnum + kTargetsPerThread - 1) / kTargetsPerThread;
  if (g >= (long long)n * ngrp) return;
  const int jg = (int)(g / n), r = (int)(g - (long long)jg * n);  // target-major: neighbouring threads, neighbouring rows
  const float4 c4 = coordc[r];
  const float coord[4] = {c4.x, c4.y, c4.z, c4.w};
  for (int u = 0; u < kTargetsPerThread; ++u) {
    const int t = jg * kTargetsPerThread + u;
    if (t >= s.tnum) break;
    const DView& v = s.views[t];
    float ic[3];
    project(v, coord, s.level, ic);
    const float fx = __fdiv_rn(ic[0], (float)s.csize), fy = __fdiv_rn(ic[1], (float)s.csize);
    const int xs[2] = {(int)floor((double)fx), (int)ceil((double)fx)};
    const int ys[2] = {(int)floor((double)fy), (int)ceil((double)fy)};
    const unsigned long long key = ((unsigned long long)depth_bits(depth_of(v, coord)) << 32) | (unsigned)r;
    const int gw = gwidth(s, t), gh = gheight(s, t);
    for (int y = 0; y < 2; ++y)
      for (int x = 0; x < 2; ++x) {
        if (xs[x] < 0 || gw <= xs[x] || ys[y] < 0 || gh <= ys[y]) continue;
        unsigned long long* cell = &keys[off[t] + (long long)ys[y] * gw + xs[x]];
        // the stored minimum only decreases, so a (possibly stale) value <= key means the atomic
        // could not change the cell: skip it
        if (key < *cell) atomicMin(cell, key);
      }
  }
}

// depth_from_bits: the winner's depth as the build kernel computed it, not a second evaluation.
__global__ __launch_bounds__(256) void depthmap_resolve_kernel(const unsigned long long* __restrict__ keys, long long cells,
                                                               const float4* __restrict__ attrc, int* __restrict__ patch,
                                                               float* __restrict__ depth, float* __restrict__ normal,
                                                               float* __restrict__ ncc) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cells) return;
  const unsigned long long key = keys[c];
  const bool filled = key != kEmpty;
  const int r = filled ? (int)(key & 0xffffffffull) : -1;
  if (patch) patch[c] = r;
  if (depth) depth[c] = filled ? depth_from_bits((unsigned int)(key >> 32)) : 0.0f;
  if (normal || ncc) {
    const float4 a = filled ? attrc[r] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (normal) {
      normal[3 * c] = a.x;
      normal[3 * c + 1] = a.y;
      normal[3 * c + 2] = a.z;
    }
    if (ncc) ncc[c] = a.w;
  }
}

inline hipError_t blocks_for(long long items, unsigned* blocks) {
  const long long g = (items + 255) / 256;
  if (g > INT_MAX) return hipErrorInvalidValue;
  *blocks = (unsigned)(g < 1 ? 1 : g);
  return hipSuccess;
}

}  // namespace

hipError_t depth_map_pack(const pmvs_patch* P, const int* src, int n, float4* coordc, float4* attrc, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  unsigned nb = 0;
  DCHK(blocks_for(n, &nb));
  hipLaunchKernelGGL(depthmap_pack_kernel, dim3(nb), dim3(256), 0, st, P, src, n, coordc, attrc);
  return hipGetLastError();
}

hipError_t depth_map_pass(const DScene& s, const pmvs_patch* P, int n, const int* src, const long long* d_off,
                          long long cells, const DepthMapArrays& out, hipStream_t st) {
  if (cells <= 0 || !(out.patch || out.depth || out.normal || out.ncc)) return hipSuccess;
  const bool attr = out.normal || out.ncc;
  DevBuf<unsigned long long> keys;
  DevBuf<float4> coordc, attrc;
  unsigned nb = 0;
  DCHK(keys.alloc((size_t)cells));
  DCHK(hipMemsetAsync(keys.p, 0xff, (size_t)cells * sizeof(unsigned long long), st));
  if (n > 0) {
    DCHK(coordc.alloc((size_t)n));
    if (attr) DCHK(attrc.alloc((size_t)n));
    DCHK(depth_map_pack(P, src, n, coordc.p, attrc.p, st));
    const int ngrp = (s.tnum + kTargetsPerThread - 1) / kTargetsPerThread;
    DCHK(blocks_for((long long)n * ngrp, &nb));
    hipLaunchKernelGGL(depthmap_build_kernel, dim3(nb), dim3(256), 0, st, s, coordc.p, n, d_off, keys.p);
    DCHK(hipGetLastError());
  }
  DCHK(blocks_for(cells, &nb));
  hipLaunchKernelGGL(depthmap_resolve_kernel, dim3(nb), dim3(256), 0, st, keys.p, cells, attrc.p, out.patch, out.depth,
                     out.normal, out.ncc);
  DCHK(hipGetLastError());
  // the scratch above is freed on return: the work that reads it must have finished
  return hipStreamSynchronize(st);
}

}  // namespace pmvsdev
