// pmvs_texmesh.hip -- a triangle mesh rasterised into the target images and one target chosen per face
// (pmvs_mesh_raster / pmvs_mesh_texture, include/pmvs_amd.h; the definition is pmvs_texmesh.h).
//
// The per-pixel maps' shape (pmvs_pixmap.hip) with faces in the place of patches.  The targets of a call are
// taken in groups of kGroupTargets, so that the keys -- 8 bytes per pixel, the only scratch that grows with
// the images -- stay bounded:
//   texmesh_ids_check_kernel  a caller's device face ids: one flag, read back before any id is an index
//   texmesh_scatter_kernel    one thread per (target of the group, face), the target from blockIdx.y so that
//                             its view is wave-uniform: the three corners projected, the drawn test, the
//                             clipped box.  A box of at most kThreadBox pixels is walked by the thread: per
//                             covered pixel a 64-bit atomicMin of (depth_bits(d) << 32) | face into the
//                             group's keys, behind a plain read that skips it when the stored key is already
//                             smaller.  A larger box is only counted (one wave-aggregated add per wave).
//   texmesh_bigfaces_kernel   only when the count is not zero: the same classification again, the large
//                             boxes' (face, target) pairs appended to a list of exactly that size by a
//                             wave-aggregated append (count-then-fill; the list's order does not matter,
//                             the result is a minimum)
//   texmesh_wave_kernel       one wavefront per list entry, its 64 lanes striding the box: a face of a
//                             whole 3840 x 2160 target costs its pixels, and no thread loops over a box
//                             larger than kThreadBox
//   texmesh_resolve_kernel    pmvs_mesh_raster: one thread per pixel of the group, face and depth written once
//   texmesh_select_kernel     pmvs_mesh_texture: one thread per face, the group's targets in ascending order
//                             inside the thread: drawn, front, the three corners against the keys, the
//                             score; a strict > replaces the running best (score, view), which lives in the
//                             output arrays between the groups
//   texmesh_uv_kernel         one thread per face: the winner's corners projected at level 0
// The corners are projected again by every kernel that needs them, not stored per (target, vertex): the
// 12-byte projected corner is as large as the 12-byte vertex it would replace, so a table saves arithmetic
// and no gather traffic, and costs 12 bytes per vertex and target of scratch and a pass that writes it
// (DESIGN.md section 4m).  No float atomics and no atomics besides the key minimum and the list counter.
#include <hip/hip_runtime.h>

#include <climits>

#include "pmvs_device.h"
#include "pmvs_fuse.h"
#include "pmvs_launch.h"
#include "pmvs_texmesh.h"

namespace pmvsdev {
namespace {

#define XCHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

constexpr int kGroupTargets = 8;              // targets rendered together
constexpr int kThreadBox = 64;                // pixels of the largest box one thread walks
constexpr unsigned long long kEmpty = ~0ull;  // no face: a face's key never has all 64 bits set (face < 2^31)

struct TexGroup {                  // one group of targets, by value to the kernels
  int first, count;                // views [first, first + count)
  long long off[kGroupTargets];    // first pixel of each target's map in the group's keys
};

__device__ __forceinline__ void project_face(const DView& vw, int level, const float V[3][4], pmvstex::Corner* c) {
  for (int k = 0; k < 3; ++k) {
    float ic[3];
    project(vw, V[k], level, ic);
    c[k].x = ic[0], c[k].y = ic[1], c[k].z = depth_of(vw, V[k]);
  }
}

// Face f of the mesh in view vw: drawn with a non-empty clipped box.
__device__ __forceinline__ bool face_in_view(const DView& vw, int level, const MeshView& m, int f, pmvstex::Corner* c, double* A,
                                             pmvstex::Box* b) {
  float V[3][4];
  load_face(m, f, V);
  project_face(vw, level, V, c);
  return pmvstex::face_drawn(c, A) && pmvstex::face_box(c, vw.w[level], vw.h[level], b);
}

__device__ __forceinline__ void put_pixel(const pmvstex::Corner* c, double A, int u, int v, int f, unsigned long long* __restrict__ row) {
  float d;
  if (!pmvstex::face_pixel_depth(c, A, u, v, &d)) return;
  const unsigned long long key = ((unsigned long long)depth_bits(d) << 32) | (unsigned)f;
  unsigned long long* cell = &row[u];
  // the stored minimum only decreases, so a (possibly stale) value <= key means the atomic could not
  // change the pixel: skip it
  if (key < *cell) atomicMin(cell, key);
}

__global__ __launch_bounds__(256) void texmesh_ids_check_kernel(const int* __restrict__ face, long long ids, int nv,
                                                                int* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ids) return;
  const int v = face[i];
  if (v < 0 || v >= nv) *bad = 1;  // every writer stores the same
}

// The lanes of a wave for which `big` holds take consecutive slots from *counter (one atomic per wave);
// returns the lane's slot, or -1.  Every lane of the wave calls it.
__device__ __forceinline__ long long wave_append(bool big, unsigned long long* counter) {
  const unsigned long long mask = __ballot(big);
  if (!mask) return -1;
  const int lane = (int)(threadIdx.x & 63), leader = __ffsll((long long)mask) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
  base = __shfl(base, leader);
  return big ? (long long)(base + __popcll(mask & ((1ull << lane) - 1ull))) : -1;
}

__global__ __launch_bounds__(256) void texmesh_scatter_kernel(DScene s, TexGroup g, MeshView m, unsigned long long* __restrict__ keys,
                                                              unsigned long long* __restrict__ nbig) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y;  // < g.count: the grid's y extent
  bool big = false;
  if (i < m.nf) {
    const DView& vw = s.views[g.first + j];
    pmvstex::Corner c[3];
    pmvstex::Box b;
    double A;
    if (face_in_view(vw, s.level, m, (int)i, c, &A, &b)) {
      big = pmvstex::box_pixels(b) > kThreadBox;
      if (!big) {
        const int W = vw.w[s.level];
        // the box is clipped to [0, W) x [0, H): the guard of every index below
        for (int v = b.v0; v <= b.v1; ++v)
          for (int u = b.u0; u <= b.u1; ++u) put_pixel(c, A, u, v, (int)i, keys + g.off[j] + (long long)v * W);
      }
    }
  }
  const unsigned long long mask = __ballot(big);
  if (mask && (int)(threadIdx.x & 63) == __ffsll((long long)mask) - 1) atomicAdd(nbig, (unsigned long long)__popcll(mask));
}

// entry = (face << 3) | target of the group; `cap` = the count the scatter kernel found.
__global__ __launch_bounds__(256) void texmesh_bigfaces_kernel(DScene s, TexGroup g, MeshView m, unsigned long long* __restrict__ counter,
                                                               long long cap, long long* __restrict__ list) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int j = blockIdx.y;
  bool big = false;
  if (i < m.nf) {
    pmvstex::Corner c[3];
    pmvstex::Box b;
    double A;
    big = face_in_view(s.views[g.first + j], s.level, m, (int)i, c, &A, &b) && pmvstex::box_pixels(b) > kThreadBox;
  }
  const long long slot = wave_append(big, counter);
  if (slot >= 0 && slot < cap) list[slot] = (i << 3) | j;
}

__global__ __launch_bounds__(256) void texmesh_wave_kernel(DScene s, TexGroup g, MeshView m, const long long* __restrict__ list,
                                                           long long entries, unsigned long long* __restrict__ keys) {
  const long long e = (long long)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (e >= entries) return;
  const long long entry = list[e];
  const int f = (int)(entry >> 3), j = (int)(entry & 7);
  if (f < 0 || f >= m.nf || j >= g.count) return;  // the list holds what the kernel above wrote
  const DView& vw = s.views[g.first + j];
  pmvstex::Corner c[3];
  pmvstex::Box b;
  double A;
  if (!face_in_view(vw, s.level, m, f, c, &A, &b)) return;
  const int W = vw.w[s.level], bw = b.u1 - b.u0 + 1, bh = b.v1 - b.v0 + 1;
  // lane l takes box pixels l, l + 64, ... in row-major order; (du, dv) follows without a division
  int lane = (int)(threadIdx.x & 63), du = lane % bw, dv = lane / bw;
  while (dv < bh) {
    put_pixel(c, A, b.u0 + du, b.v0 + dv, f, keys + g.off[j] + (long long)(b.v0 + dv) * W);
    du += 64;
    if (du >= bw) {
      dv += du / bw;
      du %= bw;
    }
  }
}

// `first`: the group's first pixel in the call's arrays.
__global__ __launch_bounds__(256) void texmesh_resolve_kernel(const unsigned long long* __restrict__ keys, long long pixels,
                                                              long long first, RasterArrays out) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pixels) return;
  const unsigned long long key = keys[p];
  const bool filled = key != kEmpty;
  if (out.face) out.face[first + p] = filled ? (int)(key & 0xffffffffull) : -1;
  if (out.depth) out.depth[first + p] = filled ? depth_from_bits((unsigned int)(key >> 32)) : 0.0f;
}

__global__ __launch_bounds__(256) void texmesh_init_kernel(int nf, int* __restrict__ view, float* __restrict__ score) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nf) return;
  view[f] = -1;
  score[f] = 0.0f;
}

__global__ __launch_bounds__(256) void texmesh_select_kernel(DScene s, TexGroup g, MeshView m, const unsigned long long* __restrict__ keys,
                                                             float depth_rel, float min_area, int* __restrict__ view,
                                                             float* __restrict__ score) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m.nf) return;
  float V[3][4];
  load_face(m, (int)i, V);
  int best_view = view[i];
  float best = score[i];
  for (int j = 0; j < g.count; ++j) {  // wave-uniform: the view's loads are scalar
    const DView& vw = s.views[g.first + j];
    const int W = vw.w[s.level], H = vw.h[s.level];
    pmvstex::Corner c[3];
    double A;
    project_face(vw, s.level, V, c);
    if (!pmvstex::face_drawn(c, &A) || !pmvstex::face_front(V[0], V[1], V[2], vw.center)) continue;
    bool visible = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // no early exit: the corners stay in registers
      int px, py;
      if (visible && pmvsfuse::pixel_at(c[k].x, c[k].y, W, H, &px, &py)) {
        const unsigned long long key = keys[g.off[j] + (long long)py * W + px];  // inside the image: pixel_at
        visible = pmvstex::corner_visible(c[k].z, key == kEmpty, depth_from_bits((unsigned int)(key >> 32)), depth_rel);
      } else {
        visible = false;
      }
    }
    if (!visible) continue;
    const float sc = pmvstex::face_score(A);
    if (!(sc >= min_area)) continue;
    if (best_view < 0 || sc > best) best = sc, best_view = g.first + j;
  }
  view[i] = best_view;
  score[i] = best;
}

__global__ __launch_bounds__(256) void texmesh_uv_kernel(DScene s, MeshView m, const int* __restrict__ view, float* __restrict__ uv) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m.nf) return;
  const int t = view[i];
  float out[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (t >= 0) {
    float V[3][4];
    load_face(m, (int)i, V);
    for (int k = 0; k < 3; ++k) {
      float ic[3];
      project(s.views[t], V[k], 0, ic);
      out[2 * k] = ic[0], out[2 * k + 1] = ic[1];
    }
  }
  for (int k = 0; k < 6; ++k) uv[6 * i + k] = out[k];
}

unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256 < 1 ? 1 : (n + 255) / 256); }

// The group of targets from t0 on and its pixel count.
TexGroup group_of(const DScene& s, const DView* hviews, int t0, int end, long long* pixels) {
  TexGroup g{};
  g.first = t0;
  g.count = end - t0 < kGroupTargets ? end - t0 : kGroupTargets;
  *pixels = 0;
  for (int j = 0; j < g.count; ++j) {
    g.off[j] = *pixels;
    *pixels += (long long)hviews[t0 + j].w[s.level] * hviews[t0 + j].h[s.level];
  }
  return g;
}

// The keys of one group: cleared, then every face's minimum.  `work` = the counter (2 x 8 bytes); the list
// of large boxes is allocated here at its exact size and lives until the next group or the caller's sync.
hipError_t render_group(const DScene& s, const TexGroup& g, const MeshView& m, long long pixels, DevBuf<unsigned long long>& keys,
                        unsigned long long* work, DevBuf<long long>& list, hipStream_t st) {
  if ((pixels + 255) / 256 > INT_MAX) return hipErrorInvalidValue;
  XCHK(keys.grow((size_t)pixels));
  XCHK(memset_big(keys.p, 0xff, (size_t)pixels * sizeof(unsigned long long), st));
  if (m.nf < 1) return hipSuccess;
  const dim3 grid(blocks_of(m.nf), (unsigned)g.count);
  unsigned long long nbig = 0;
  XCHK(hipMemsetAsync(work, 0, 2 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(texmesh_scatter_kernel, grid, dim3(256), 0, st, s, g, m, keys.p, work);
  XCHK(hipGetLastError());
  XCHK(hipMemcpyAsync(&nbig, work, sizeof(nbig), hipMemcpyDeviceToHost, st));
  XCHK(hipStreamSynchronize(st));  // also: the previous group's list is no longer read
  if (nbig == 0) return hipSuccess;
  if ((nbig + 3) / 4 > (unsigned long long)INT_MAX) return hipErrorInvalidValue;
  XCHK(list.grow((size_t)nbig));
  hipLaunchKernelGGL(texmesh_bigfaces_kernel, grid, dim3(256), 0, st, s, g, m, work + 1, (long long)nbig, list.p);
  XCHK(hipGetLastError());
  hipLaunchKernelGGL(texmesh_wave_kernel, dim3((unsigned)((nbig + 3) / 4)), dim3(256), 0, st, s, g, m, list.p, (long long)nbig, keys.p);
  return hipGetLastError();
}

}  // namespace

hipError_t mesh_ids_check(const int* face, long long nf, long long nv, bool* ok, hipStream_t st) {
  *ok = true;
  if (nf < 1) return hipSuccess;
  DevBuf<int> bad;
  int host_bad = 0;
  XCHK(bad.alloc(1));
  XCHK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(texmesh_ids_check_kernel, dim3(blocks_of(3 * nf)), dim3(256), 0, st, face, 3 * nf, (int)nv, bad.p);
  XCHK(hipGetLastError());
  XCHK(hipMemcpyAsync(&host_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  XCHK(hipStreamSynchronize(st));
  *ok = host_bad == 0;
  return hipSuccess;
}

hipError_t mesh_raster_pass(const DScene& s, const DView* hviews, int first, int count, const float* vertex, long long nf,
                            const int* face, const RasterArrays& out, hipStream_t st) {
  if (count <= 0 || !(out.face || out.depth)) return hipSuccess;
  const MeshView m{vertex, face, (int)nf};
  DevBuf<unsigned long long> keys, work;
  DevBuf<long long> list;
  XCHK(work.alloc(2));
  long long off = 0;  // the group's first pixel in the call's arrays
  for (int t0 = first; t0 < first + count; t0 += kGroupTargets) {
    long long pixels = 0;
    const TexGroup g = group_of(s, hviews, t0, first + count, &pixels);
    XCHK(render_group(s, g, m, pixels, keys, work.p, list, st));
    hipLaunchKernelGGL(texmesh_resolve_kernel, dim3(blocks_of(pixels)), dim3(256), 0, st, keys.p, pixels, off, out);
    XCHK(hipGetLastError());
    off += pixels;
  }
  // the scratch above is freed on return: the work that reads it must have finished
  return hipStreamSynchronize(st);
}

hipError_t mesh_texture_pass(const DScene& s, const DView* hviews, int first, int count, const pmvs_texture_params& prm,
                             const float* vertex, long long nf, const int* face, const TextureArrays& out, hipStream_t st) {
  if (count <= 0 || nf < 1 || !(out.view || out.uv || out.score)) return hipSuccess;
  const MeshView m{vertex, face, (int)nf};
  DevBuf<unsigned long long> keys, work;
  DevBuf<long long> list;
  DevBuf<int> own_view;
  DevBuf<float> own_score;
  int* view = out.view;
  float* score = out.score;
  if (!view) {  // the running best lives in the output arrays: the ones the caller did not ask for are scratch
    XCHK(own_view.alloc((size_t)nf));
    view = own_view.p;
  }
  if (!score) {
    XCHK(own_score.alloc((size_t)nf));
    score = own_score.p;
  }
  XCHK(work.alloc(2));
  hipLaunchKernelGGL(texmesh_init_kernel, dim3(blocks_of(nf)), dim3(256), 0, st, (int)nf, view, score);
  XCHK(hipGetLastError());
  for (int t0 = first; t0 < first + count; t0 += kGroupTargets) {
    long long pixels = 0;
    const TexGroup g = group_of(s, hviews, t0, first + count, &pixels);
    XCHK(render_group(s, g, m, pixels, keys, work.p, list, st));
    hipLaunchKernelGGL(texmesh_select_kernel, dim3(blocks_of(nf)), dim3(256), 0, st, s, g, m, keys.p, prm.depth_rel, prm.min_area,
                       view, score);
    XCHK(hipGetLastError());
  }
  if (out.uv) {
    hipLaunchKernelGGL(texmesh_uv_kernel, dim3(blocks_of(nf)), dim3(256), 0, st, s, m, view, out.uv);
    XCHK(hipGetLastError());
  }
  // the scratch above is freed on return: the work that reads it must have finished
  return hipStreamSynchronize(st);
}

}  // namespace pmvsdev
