// pmvs_mesh.hip -- the fused maps meshed on the device: a TSDF volume integrated from the per-pixel maps
// and the fusion's pass flags, and a triangle mesh extracted from a volume by naive surface nets
// (pmvs_loop_tsdf / pmvs_tsdf_mesh / pmvs_loop_mesh, include/pmvs_amd.h; the definition is pmvs_mesh.h).
//
//   tsdf_integrate_kernel  one thread per voxel, x fastest, so a wave's 64 voxels project to neighbouring
//                          pixels of every target.  The loop over the range's targets runs inside the
//                          thread and is wave-uniform: each target's projection, optical axis, image size
//                          and map offset is a scalar load, sum / n / the colour sums stay in registers,
//                          and the voxel's 9 bytes are written once.  No atomics, no pass per target.
//                          The per-voxel body is pmvs_tsdf_voxel.h's, shared with the brick kernel.
//   mesh_cells_kernel      one thread per cell: the active flag (a byte) from the 8 corners
//   mesh_faces_kernel      one thread per voxel: one bit per axis whose +a edge emits a quad, from the two
//                          endpoints and the four cells' active flags
//   rocprim exclusive_scan the active flags to vertex ids (int, 4 bytes per cell) and the voxels' quad
//                          counts to quad offsets (64-bit: a volume can hold more than 2^31 triangles)
//   mesh_vertex_kernel     one thread per cell: an active cell below `vcap` writes vertex, normal, colour
//   mesh_face_kernel       one thread per voxel: its quads' two triangles each, below `fcap`
// The corner reads of neighbouring cells overlap eightfold; they are left to L2 (a row of cells reads two
// rows of two planes, which one workgroup's 256 consecutive cells share), not staged in LDS: nothing has
// been measured that says a tile pays.  Nothing depends on the order of the work, so the mesh is
// deterministic.
#include <hip/hip_runtime.h>

#include <cstring>  // before rocprim, whose texture iterator calls memset without including it

#include <rocprim/rocprim.hpp>

#include "pmvs_device.h"
#include "pmvs_fuse.h"
#include "pmvs_launch.h"
#include "pmvs_mesh.h"
#include "pmvs_tsdf_voxel.h"

namespace pmvsdev {
namespace {

#define MCHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

struct Dims {
  int nx, ny, nz;
  __host__ __device__ long long voxels() const { return (long long)nx * ny * nz; }
  __host__ __device__ long long cells() const { return (long long)(nx - 1) * (ny - 1) * (nz - 1); }
};

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(DScene s, TsdfMapsView m, pmvs_volume vol, float trunc,
                                                             TsdfArrays out) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int nx = vol.dims[0], ny = vol.dims[1], nz = vol.dims[2];
  if (idx >= (long long)nx * ny * nz) return;
  const int i = (int)(idx % nx), j = (int)((idx / nx) % ny), k = (int)(idx / ((long long)nx * ny));
  tsdf_store(out, idx, tsdf_voxel(s, m, vol, trunc, i, j, k));
}

struct VolumeView {
  Dims d;
  int min_obs;
  const float* tsdf;
  const unsigned char *obs, *color;  // color may be null
  __device__ long long voxel(int i, int j, int k) const { return ((long long)k * d.ny + j) * d.nx + i; }
  __device__ long long cell(int i, int j, int k) const { return ((long long)k * (d.ny - 1) + j) * (d.nx - 1) + i; }
};

// Cell index -> (i, j, k); false past the cells.
__device__ __forceinline__ bool own_cell(const Dims& d, int* i, int* j, int* k, long long* c) {
  *c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (*c >= d.cells()) return false;
  const int cx = d.nx - 1, cy = d.ny - 1;
  *i = (int)(*c % cx), *j = (int)((*c / cx) % cy), *k = (int)(*c / ((long long)cx * cy));
  return true;
}
__device__ __forceinline__ bool own_voxel(const Dims& d, int* i, int* j, int* k, long long* v) {
  *v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (*v >= d.voxels()) return false;
  *i = (int)(*v % d.nx), *j = (int)((*v / d.nx) % d.ny), *k = (int)(*v / ((long long)d.nx * d.ny));
  return true;
}

__global__ __launch_bounds__(256) void mesh_cells_kernel(VolumeView vol, unsigned char* __restrict__ active) {
  int i, j, k;
  long long c;
  if (!own_cell(vol.d, &i, &j, &k, &c)) return;
  bool observed[8], inside[8];
  for (int n = 0; n < 8; ++n) {  // corners lie in [0, nx) x [0, ny) x [0, nz): i <= nx - 2 and so on
    const long long v = vol.voxel(i + (n & 1), j + ((n >> 1) & 1), k + (n >> 2));
    observed[n] = vol.obs[v] >= vol.min_obs;
    inside[n] = vol.tsdf[v] < 0.0f;
  }
  active[c] = pmvsmesh::cell_active(observed, inside);
}

// Bit a of quads[v]: the edge from voxel v to its +a neighbour emits a quad.
__global__ __launch_bounds__(256) void mesh_faces_kernel(VolumeView vol, const unsigned char* __restrict__ active,
                                                         unsigned char* __restrict__ quads) {
  int idx[3];
  long long v;
  if (!own_voxel(vol.d, &idx[0], &idx[1], &idx[2], &v)) return;
  const int n[3] = {vol.d.nx, vol.d.ny, vol.d.nz};
  const long long stride[3] = {1, vol.d.nx, (long long)vol.d.nx * vol.d.ny};
  const bool obs0 = vol.obs[v] >= vol.min_obs, in0 = vol.tsdf[v] < 0.0f;
  unsigned bits = 0;
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    if (!obs0 || idx[a] + 1 >= n[a] || idx[b] < 1 || idx[b] > n[b] - 2 || idx[c] < 1 || idx[c] > n[c] - 2) continue;
    const long long w = v + stride[a];  // inside: idx[a] + 1 < n[a]
    if (!(vol.obs[w] >= vol.min_obs) || (vol.tsdf[w] < 0.0f) == in0) continue;
    // the four cells: a-coordinate idx[a] <= n[a] - 2, (b, c) in [idx - 1, idx] within [0, n - 2]
    bool all = true;
    for (int q = 0; q < 4; ++q) {
      int cc[3];
      cc[a] = idx[a], cc[b] = idx[b] - (q & 1), cc[c] = idx[c] - (q >> 1);
      all = all && active[vol.cell(cc[0], cc[1], cc[2])];
    }
    if (all) bits |= 1u << a;
  }
  quads[v] = (unsigned char)bits;
}

__global__ __launch_bounds__(256) void mesh_vertex_kernel(VolumeView vol, pmvs_volume box, const unsigned char* __restrict__ active,
                                                          const int* __restrict__ vid, long long vcap, MeshArrays out) {
  int idx[3];
  long long c;
  if (!own_cell(vol.d, &idx[0], &idx[1], &idx[2], &c)) return;
  if (!active[c]) return;
  const long long o = vid[c];
  if (o >= vcap) return;
  float val[8];
  unsigned char rgba[8][4];
  for (int n = 0; n < 8; ++n) {
    const long long v = vol.voxel(idx[0] + (n & 1), idx[1] + ((n >> 1) & 1), idx[2] + (n >> 2));
    val[n] = vol.tsdf[v];
    const uchar4 w = vol.color ? reinterpret_cast<const uchar4*>(vol.color)[v] : make_uchar4(0, 0, 0, 0);
    rgba[n][0] = w.x, rgba[n][1] = w.y, rgba[n][2] = w.z, rgba[n][3] = w.w;
  }
  double m[3];
  float nrm[3];
  pmvsmesh::cell_vertex(val, m, nrm);
  if (out.vertex)
    for (int a = 0; a < 3; ++a) out.vertex[3 * o + a] = pmvsmesh::voxel_coord(box.origin[a], box.voxel, idx[a], m[a]);
  if (out.normal)
    for (int a = 0; a < 3; ++a) out.normal[3 * o + a] = nrm[a];
  if (out.color) pmvsmesh::cell_colour(rgba, out.color + 3 * o);
}

__global__ __launch_bounds__(256) void mesh_face_kernel(VolumeView vol, const unsigned char* __restrict__ quads,
                                                        const long long* __restrict__ qpos, const int* __restrict__ vid,
                                                        long long fcap, int* __restrict__ face) {
  int idx[3];
  long long v;
  if (!own_voxel(vol.d, &idx[0], &idx[1], &idx[2], &v)) return;
  const unsigned bits = quads[v];
  if (!bits) return;
  const bool in0 = vol.tsdf[v] < 0.0f;
  long long f = 2 * qpos[v];
  for (int a = 0; a < 3; ++a) {
    if (!(bits & (1u << a))) continue;
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    int Q[4];  // Q0 = (b-1, c-1), Q1 = (b, c-1), Q2 = (b, c), Q3 = (b-1, c): the cells mesh_faces_kernel found active
    const int db[4] = {1, 0, 0, 1}, dc[4] = {1, 1, 0, 0};
    for (int q = 0; q < 4; ++q) {
      int cc[3];
      cc[a] = idx[a], cc[b] = idx[b] - db[q], cc[c] = idx[c] - dc[q];
      Q[q] = vid[vol.cell(cc[0], cc[1], cc[2])];
    }
    const int tri[2][3] = {{Q[0], in0 ? Q[1] : Q[2], in0 ? Q[2] : Q[1]}, {Q[0], in0 ? Q[2] : Q[3], in0 ? Q[3] : Q[2]}};
    for (int t = 0; t < 2; ++t, ++f)
      if (f < fcap) face[3 * f] = tri[t][0], face[3 * f + 1] = tri[t][1], face[3 * f + 2] = tri[t][2];
  }
}

struct QuadCount {  // the quads of a voxel's flag byte
  __host__ __device__ long long operator()(unsigned char b) const { return (long long)((b & 1) + ((b >> 1) & 1) + ((b >> 2) & 1)); }
};

unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t tsdf_integrate(const DScene& s, const FuseMaps& f, int first, int count, const pmvs_volume& vol, float trunc,
                          const TsdfArrays& out, hipStream_t st) {
  if (!out.tsdf && !out.obs && !out.color) return hipSuccess;
  const long long voxels = (long long)vol.dims[0] * vol.dims[1] * vol.dims[2];  // <= INT_MAX: the API checked
  const TsdfMapsView m{f.depth.p, f.pass.p, f.off.p, first, count};
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(blocks_of(voxels)), dim3(256), 0, st, s, m, vol, trunc, out);
  return hipGetLastError();
}

hipError_t tsdf_mesh_pass(const pmvs_volume& box, int min_obs, const float* tsdf, const unsigned char* obs,
                          const unsigned char* color, long long vcap, long long fcap, const MeshArrays& out, long long* nverts,
                          long long* nfaces, hipStream_t st) {
  const Dims d{box.dims[0], box.dims[1], box.dims[2]};
  *nverts = *nfaces = 0;
  if (d.nx < 2 || d.ny < 2 || d.nz < 2) return hipSuccess;  // no cells
  const long long voxels = d.voxels(), cells = d.cells();
  const VolumeView vol{d, min_obs, tsdf, obs, color};

  DevBuf<unsigned char> active, quads;
  DevBuf<int> vid;
  DevBuf<long long> qpos;
  DevBuf<char> temp;
  MCHK(active.alloc((size_t)cells));
  MCHK(vid.alloc((size_t)cells));
  MCHK(quads.alloc((size_t)voxels));
  MCHK(qpos.alloc((size_t)voxels));
  const auto quad_counts = rocprim::make_transform_iterator(quads.p, QuadCount());
  size_t tb_v = 0, tb_q = 0;
  MCHK(rocprim::exclusive_scan(nullptr, tb_v, active.p, vid.p, 0, (size_t)cells, rocprim::plus<int>(), st));
  MCHK(rocprim::exclusive_scan(nullptr, tb_q, quad_counts, qpos.p, 0LL, (size_t)voxels, rocprim::plus<long long>(), st));
  MCHK(temp.alloc(tb_v > tb_q ? tb_v : tb_q));

  hipLaunchKernelGGL(mesh_cells_kernel, dim3(blocks_of(cells)), dim3(256), 0, st, vol, active.p);
  MCHK(hipGetLastError());
  hipLaunchKernelGGL(mesh_faces_kernel, dim3(blocks_of(voxels)), dim3(256), 0, st, vol, active.p, quads.p);
  MCHK(hipGetLastError());
  MCHK(rocprim::exclusive_scan(temp.p, tb_v, active.p, vid.p, 0, (size_t)cells, rocprim::plus<int>(), st));
  MCHK(rocprim::exclusive_scan(temp.p, tb_q, quad_counts, qpos.p, 0LL, (size_t)voxels, rocprim::plus<long long>(), st));
  // the counts: the last offset plus the last element's own
  int last_vid = 0;
  unsigned char last_active = 0, last_quads = 0;
  long long last_qpos = 0;
  MCHK(hipMemcpyAsync(&last_vid, vid.p + (cells - 1), sizeof(int), hipMemcpyDeviceToHost, st));
  MCHK(hipMemcpyAsync(&last_active, active.p + (cells - 1), 1, hipMemcpyDeviceToHost, st));
  MCHK(hipMemcpyAsync(&last_qpos, qpos.p + (voxels - 1), sizeof(long long), hipMemcpyDeviceToHost, st));
  MCHK(hipMemcpyAsync(&last_quads, quads.p + (voxels - 1), 1, hipMemcpyDeviceToHost, st));
  if (vcap > 0 && (out.vertex || out.normal || out.color)) {
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3(blocks_of(cells)), dim3(256), 0, st, vol, box, active.p, vid.p, vcap, out);
    MCHK(hipGetLastError());
  }
  if (fcap > 0 && out.face) {
    hipLaunchKernelGGL(mesh_face_kernel, dim3(blocks_of(voxels)), dim3(256), 0, st, vol, quads.p, qpos.p, vid.p, fcap, out.face);
    MCHK(hipGetLastError());
  }
  // the scratch above is freed on return: the work that reads it must have finished
  MCHK(hipStreamSynchronize(st));
  *nverts = (long long)last_vid + (last_active ? 1 : 0);
  *nfaces = 2 * (last_qpos + QuadCount()(last_quads));
  return hipSuccess;
}

}  // namespace pmvsdev
