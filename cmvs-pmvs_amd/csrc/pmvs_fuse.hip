// pmvs_fuse.hip -- the per-pixel maps fused into a cross-view-checked point cloud on the device
// (pmvs_loop_fuse / pmvs_fuse_patches, include/pmvs_amd.h; the definition is pmvs_fuse.h).
//
// The first consumer of the per-pixel maps (pmvs_pixmap.hip), which it renders into scratch by the maps'
// own pass.  Every kernel takes one thread per pixel and its target from blockIdx.y, so that the pixel's
// own view is wave-uniform; the loop over the range's other targets is wave-uniform too, so each of
// their projections and optical axes is a scalar load:
//   fuse_support_kernel   an empty pixel writes 0 and leaves; a filled one back-projects once
//                         (pixel_point) and per other target s projects the point, gathers patch / depth /
//                         normal at the pixel it falls on and counts the consistent s: the support map and
//                         one pass flag per pixel
//   fuse_emit_kernel      a second launch (it reads the finished pass flags of lower targets): the same
//                         walk over s < t only, until a consistent passing pixel suppresses this one; the
//                         emit flag as a 64-bit 0 / 1
//   hipcub InclusiveSum   in place over those flags: a point's index is its sum - 1, the last sum the count
//   fuse_gather_kernel    the emitted pixels below `cap` write the requested point arrays; the colour is
//                         the pixel's RGBA8 pyramid word
// Nothing depends on the order of the work, so the cloud is deterministic.
// fuse_maps_pass is the first half (the maps and fuse_support_kernel) on its own: the TSDF integration
// (pmvs_mesh.hip) starts from the same maps and pass flags.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <vector>

#include "pmvs_device.h"
#include "pmvs_fuse.h"
#include "pmvs_launch.h"

namespace pmvsdev {
namespace {

#define FCHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

struct FuseMapsView {    // the range's maps, by value to the kernels
  const int* patch;
  const float *depth, *normal;
  const long long* off;  // count + 1: the first pixel of each target's map
  int first, count;      // views [first, first + count)
};

// The pixel of the range's target j (wave-uniform) that the point S4 = (Sf, 1) with normal n is consistent
// with, or -1.  Every index is guarded by pixel_at: q lies in target j's map.
__device__ __forceinline__ long long consistent_pixel(const DScene& s, const FuseMapsView& m, int j, const float* S4, const float* n,
                                                      const pmvs_fuse_params& prm) {
  const DView& vs = s.views[m.first + j];
  const int W = vs.w[s.level], H = vs.h[s.level];
  float ic[3];
  project(vs, S4, s.level, ic);
  int px, py;
  if (!pmvsfuse::pixel_at(ic[0], ic[1], W, H, &px, &py)) return -1;
  const long long q = m.off[j] + (long long)py * W + px;
  if (m.patch[q] < 0) return -1;
  if (!pmvsfuse::depth_consistent(m.depth[q], depth_of(vs, S4), prm.depth_rel)) return -1;
  const float mn[3] = {m.normal[3 * q], m.normal[3 * q + 1], m.normal[3 * q + 2]};
  return pmvsfuse::normal_consistent(n, mn, prm.normal_cos) ? q : -1;
}

// This thread's pixel: c = its index in the range's arrays, (u, v) in target j; false past the image.
__device__ __forceinline__ bool own_pixel(const DScene& s, const FuseMapsView& m, int* j, int* u, int* v, long long* c) {
  *j = blockIdx.y;
  if (*j >= m.count) return false;
  const DView& vw = s.views[m.first + *j];
  const int W = vw.w[s.level], H = vw.h[s.level];
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long long)W * H) return false;
  *u = (int)(p % W), *v = (int)(p / W);
  *c = m.off[*j] + p;
  return true;
}

__global__ __launch_bounds__(256) void fuse_support_kernel(DScene s, FuseMapsView m, pmvs_fuse_params prm,
                                                           unsigned char* __restrict__ support,
                                                           unsigned char* __restrict__ pass) {
  int j, u, v;
  long long c;
  if (!own_pixel(s, m, &j, &u, &v, &c)) return;
  const DView& vw = s.views[m.first + j];
  float S4[4];
  S4[3] = 1.0f;
  if (m.patch[c] < 0 || !pmvsfuse::pixel_point(vw.P[s.level], vw.oaxis, u, v, m.depth[c], S4)) {
    support[c] = 0;
    pass[c] = 0;
    return;
  }
  const float n[3] = {m.normal[3 * c], m.normal[3 * c + 1], m.normal[3 * c + 2]};
  int cnt = 0;
  for (int k = 0; k < m.count; ++k)
    if (k != j && consistent_pixel(s, m, k, S4, n, prm) >= 0) ++cnt;
  support[c] = (unsigned char)cnt;  // at most PMVS_MAX_TARGETS - 1
  pass[c] = cnt >= prm.min_support;
}

__global__ __launch_bounds__(256) void fuse_emit_kernel(DScene s, FuseMapsView m, pmvs_fuse_params prm,
                                                        const unsigned char* __restrict__ pass, long long* __restrict__ pos) {
  int j, u, v;
  long long c;
  if (!own_pixel(s, m, &j, &u, &v, &c)) return;
  if (!pass[c]) {
    pos[c] = 0;
    return;
  }
  const DView& vw = s.views[m.first + j];
  float S4[4];
  S4[3] = 1.0f;
  pmvsfuse::pixel_point(vw.P[s.level], vw.oaxis, u, v, m.depth[c], S4);  // valid: the pixel passes
  const float n[3] = {m.normal[3 * c], m.normal[3 * c + 1], m.normal[3 * c + 2]};
  bool emit = true;
  for (int k = 0; k < j && emit; ++k) {
    const long long q = consistent_pixel(s, m, k, S4, n, prm);
    if (q >= 0 && pass[q]) emit = false;
  }
  pos[c] = emit;
}

// pos: the inclusive sums of the emit flags.
__global__ __launch_bounds__(256) void fuse_gather_kernel(DScene s, FuseMapsView m, const unsigned char* __restrict__ support,
                                                          const long long* __restrict__ pos, long long cap, FuseArrays out) {
  int j, u, v;
  long long c;
  if (!own_pixel(s, m, &j, &u, &v, &c)) return;
  const long long i = pos[c] - 1;
  if (pos[c] == (c ? pos[c - 1] : 0) || i >= cap) return;
  const DView& vw = s.views[m.first + j];
  if (out.coord) {
    float S[3];
    pmvsfuse::pixel_point(vw.P[s.level], vw.oaxis, u, v, m.depth[c], S);
    out.coord[3 * i] = S[0], out.coord[3 * i + 1] = S[1], out.coord[3 * i + 2] = S[2];
  }
  if (out.normal) {
    out.normal[3 * i] = m.normal[3 * c];
    out.normal[3 * i + 1] = m.normal[3 * c + 1];
    out.normal[3 * i + 2] = m.normal[3 * c + 2];
  }
  if (out.color) {
    const uint32_t w = s.pyr[vw.pyr_off[s.level] + (long long)v * vw.w[s.level] + u];
    out.color[3 * i] = (unsigned char)(w & 0xff);
    out.color[3 * i + 1] = (unsigned char)((w >> 8) & 0xff);
    out.color[3 * i + 2] = (unsigned char)((w >> 16) & 0xff);
  }
  if (out.support) out.support[i] = support[c];
  if (out.pixel) out.pixel[i] = c;
  if (out.patch) out.patch[i] = m.patch[c];
}

}  // namespace

hipError_t fuse_maps_pass(const DScene& s, const DView* hviews, const pmvs_patch* P, int n, const int* src, int first, int count,
                          const pmvs_fuse_params& prm, unsigned char* support_map, FuseMaps& f, hipStream_t st) {
  std::vector<long long>& off = f.host_off;  // it outlives the asynchronous upload below
  off.assign((size_t)count + 1, 0);
  long long pixels = 0, widest = 0;
  for (int j = 0; j < count; ++j) {
    const long long wh = (long long)hviews[first + j].w[s.level] * hviews[first + j].h[s.level];
    off[(size_t)j] = pixels;
    pixels += wh;
    widest = wh > widest ? wh : widest;
  }
  off[(size_t)count] = pixels;
  const long long rb = (widest + 255) / 256;
  if (rb > INT_MAX) return hipErrorInvalidValue;
  f.pixels = pixels;
  f.row_blocks = (unsigned)(rb < 1 ? 1 : rb);
  const dim3 grid(f.row_blocks, (unsigned)count);

  FCHK(f.patch.alloc((size_t)pixels));
  FCHK(f.depth.alloc((size_t)pixels));
  FCHK(f.normal.alloc((size_t)pixels * 3));
  FCHK(f.pass.alloc((size_t)pixels));
  FCHK(f.off.alloc(off.size()));
  f.support_map = support_map;
  if (!f.support_map) {
    FCHK(f.support.alloc((size_t)pixels));
    f.support_map = f.support.p;
  }

  // the maps, by the maps' own pass: the bytes pmvs_loop_pixel_maps gives in device mode
  DepthMapArrays maps;
  maps.patch = f.patch.p, maps.depth = f.depth.p, maps.normal = f.normal.p;
  FCHK(pixel_map_pass(s, hviews, P, n, src, first, count, prm.radius, maps, st));

  FCHK(hipMemcpyAsync(f.off.p, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st));
  const FuseMapsView m{f.patch.p, f.depth.p, f.normal.p, f.off.p, first, count};
  hipLaunchKernelGGL(fuse_support_kernel, grid, dim3(256), 0, st, s, m, prm, f.support_map, f.pass.p);
  return hipGetLastError();
}

hipError_t fuse_pass(const DScene& s, const DView* hviews, const pmvs_patch* P, int n, const int* src, int first, int count,
                     const pmvs_fuse_params& prm, long long cap, const FuseArrays& out, long long* total, hipStream_t st) {
  FuseMaps f;
  DevBuf<long long> pos;
  DevBuf<char> temp;
  FCHK(fuse_maps_pass(s, hviews, P, n, src, first, count, prm, out.support_map, f, st));
  const long long pixels = f.pixels;
  const dim3 grid(f.row_blocks, (unsigned)count);
  unsigned char* d_support = f.support_map;
  const FuseMapsView m{f.patch.p, f.depth.p, f.normal.p, f.off.p, first, count};
  FCHK(pos.alloc((size_t)pixels));
  size_t tb = 0;
  FCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tb, pos.p, pos.p, pixels, st));
  FCHK(temp.alloc(tb));

  hipLaunchKernelGGL(fuse_emit_kernel, grid, dim3(256), 0, st, s, m, prm, f.pass.p, pos.p);
  FCHK(hipGetLastError());
  FCHK(hipcub::DeviceScan::InclusiveSum(temp.p, tb, pos.p, pos.p, pixels, st));
  long long cnt = 0;
  FCHK(hipMemcpyAsync(&cnt, pos.p + (pixels - 1), sizeof(cnt), hipMemcpyDeviceToHost, st));
  if (cap > 0 && (out.coord || out.normal || out.color || out.support || out.pixel || out.patch)) {
    hipLaunchKernelGGL(fuse_gather_kernel, grid, dim3(256), 0, st, s, m, d_support, pos.p, cap, out);
    FCHK(hipGetLastError());
  }
  // the scratch above is freed on return: the work that reads it must have finished
  FCHK(hipStreamSynchronize(st));
  *total = cnt;
  return hipSuccess;
}

}  // namespace pmvsdev
