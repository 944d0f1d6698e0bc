// pmvs_pixmap.hip -- the model's per-pixel depth and normal maps, rendered on the device
// (pmvs_loop_pixel_maps / pmvs_pixel_maps_patches, include/pmvs_amd.h; the definition is pmvs_pixmap.h).
//
// The depth maps' shape (pmvs_depthmap.hip) at image resolution.  The rows' float4 arrays are the
// depth maps' own (depth_map_pack); the targets of a call are taken in groups of kGroupTargets, so
// that the keys -- 8 bytes per pixel, the only scratch that grows with the images -- stay bounded:
//   pixmap_scatter_kernel   one thread per (target of the group, row), the target from blockIdx.y so
//                           that its view is wave-uniform: project, the footprint, and per footprint
//                           pixel pixel_depth and a 64-bit atomicMin of (depth_bits(d) << 32) | row
//                           into the group's keys, behind a plain read that skips it when the stored
//                           key is already smaller
//   pixmap_resolve_kernel   one thread per pixel of the group: every wanted output written once
//                           (empty pixels too)
// The minimum does not depend on the order of the atomics, so the maps are deterministic.
// A tile-binned form (bin entries per 32 x 32-pixel tile, a radix sort by tile, one workgroup per tile
// with its keys in LDS and the resolve fused) gave the same bytes and measured 2.7 times slower on the
// C3 model; DESIGN.md section 4h has its design and times.
#include <hip/hip_runtime.h>

#include <climits>

#include "pmvs_device.h"
#include "pmvs_launch.h"
#include "pmvs_pixmap.h"

namespace pmvsdev {
namespace {

#define PCHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

constexpr int kGroupTargets = 8;              // targets rendered together
constexpr unsigned long long kEmpty = ~0ull;  // no row: a row's key never has all 64 bits set (row < 2^31)

struct PixGroup {                  // one group of targets, by value to the kernel
  int first, count, radius;        // views [first, first + count)
  long long off[kGroupTargets];    // first pixel of each target's map in the group's keys
};

__global__ __launch_bounds__(256) void pixmap_scatter_kernel(DScene s, PixGroup g, const float4* __restrict__ coordc,
                                                             const float4* __restrict__ attrc, int n,
                                                             unsigned long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y;
  if (i >= n || j >= g.count) return;
  const int r = (int)i;
  const DView& vw = s.views[g.first + j];
  const int W = vw.w[s.level], H = vw.h[s.level];
  const float4 c4 = coordc[r];
  const float coord[4] = {c4.x, c4.y, c4.z, c4.w};
  float ic[3];
  project(vw, coord, s.level, ic);
  pmvspix::Footprint f;
  if (!pmvspix::footprint(ic[0], ic[1], W, H, g.radius, &f)) return;
  const float4 a4 = attrc[r];
  const float normal[3] = {a4.x, a4.y, a4.z};
  const float z = depth_of(vw, coord);
  const long long base = g.off[j];
  // the footprint is clipped to [0, W) x [0, H): the guard of every index below
  for (int v = f.y0; v <= f.y1; ++v)
    for (int u = f.x0; u <= f.x1; ++u) {
      const float d = pmvspix::pixel_depth(vw.P[s.level], vw.center, vw.oaxis, coord, normal, u, v, z);
      const unsigned long long key = ((unsigned long long)depth_bits(d) << 32) | (unsigned)r;
      unsigned long long* cell = &keys[base + (long long)v * W + u];
      // the stored minimum only decreases, so a (possibly stale) value <= key means the atomic
      // could not change the pixel: skip it
      if (key < *cell) atomicMin(cell, key);
    }
}

// `first`: the group's first pixel in the call's arrays.  depth_from_bits: the winner's depth as the
// scatter kernel computed it, not a second evaluation.
__global__ __launch_bounds__(256) void pixmap_resolve_kernel(const unsigned long long* __restrict__ keys, long long pixels,
                                                             long long first, const float4* __restrict__ attrc,
                                                             DepthMapArrays out) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pixels) return;
  const unsigned long long key = keys[p];
  const bool filled = key != kEmpty;
  const int r = filled ? (int)(key & 0xffffffffull) : -1;
  const long long c = first + p;
  if (out.patch) out.patch[c] = r;
  if (out.depth) out.depth[c] = filled ? depth_from_bits((unsigned int)(key >> 32)) : 0.0f;
  if (out.normal || out.ncc) {
    const float4 a = filled ? attrc[r] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (out.normal) {
      out.normal[3 * c] = a.x;
      out.normal[3 * c + 1] = a.y;
      out.normal[3 * c + 2] = a.z;
    }
    if (out.ncc) out.ncc[c] = a.w;
  }
}

}  // namespace

hipError_t pixel_map_pass(const DScene& s, const DView* hviews, const pmvs_patch* P, int n, const int* src, int first,
                          int count, int radius, const DepthMapArrays& out, hipStream_t st) {
  if (count <= 0 || !(out.patch || out.depth || out.normal || out.ncc)) return hipSuccess;
  DevBuf<float4> coordc, attrc;
  DevBuf<unsigned long long> keys;
  if (n > 0) {
    PCHK(coordc.alloc((size_t)n));
    PCHK(attrc.alloc((size_t)n));
    PCHK(depth_map_pack(P, src, n, coordc.p, attrc.p, st));
  }
  long long off = 0;  // the group's first pixel in the call's arrays
  for (int t0 = first; t0 < first + count; t0 += kGroupTargets) {
    PixGroup g{};
    g.first = t0, g.radius = radius;
    g.count = first + count - t0 < kGroupTargets ? first + count - t0 : kGroupTargets;
    long long pixels = 0;
    for (int j = 0; j < g.count; ++j) {
      g.off[j] = pixels;
      pixels += (long long)hviews[t0 + j].w[s.level] * hviews[t0 + j].h[s.level];
    }
    const long long rb = (pixels + 255) / 256;
    if (rb > INT_MAX) return hipErrorInvalidValue;
    PCHK(keys.grow((size_t)pixels));
    PCHK(memset_big(keys.p, 0xff, (size_t)pixels * sizeof(unsigned long long), st));
    if (n > 0) {
      hipLaunchKernelGGL(pixmap_scatter_kernel, dim3((unsigned)(((long long)n + 255) / 256), (unsigned)g.count), dim3(256), 0, st, s, g,
                         coordc.p, attrc.p, n, keys.p);
      PCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(pixmap_resolve_kernel, dim3((unsigned)(rb < 1 ? 1 : rb)), dim3(256), 0, st, keys.p, pixels, off,
                       attrc.p, out);
    PCHK(hipGetLastError());
    off += pixels;
  }
  // the scratch above is freed on return: the work that reads it must have finished
  return hipStreamSynchronize(st);
}

}  // namespace pmvsdev
