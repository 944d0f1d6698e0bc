// pmvs_brick.hip -- the sparse volume of 8 x 8 x 8-voxel bricks on the device: the bricks near the fused
// points selected, integrated and meshed (pmvs_loop_brick_tsdf / pmvs_brick_tsdf_mesh / pmvs_loop_brick_mesh,
// include/pmvs_amd.h; the definition is pmvs_brick.h on top of pmvs_mesh.h).  A voxel's bytes and the mesh
// are those of the dense calls (pmvs_mesh.hip); only where the volume exists differs.
//
//   brick_mark_kernel       one thread per pixel of the range, its target from blockIdx.y: a passing pixel
//                           back-projects (pixel_point) and stores the byte 1 into the grid's flag array for
//                           every brick of its clipped box.  Every writer stores the same value: plain stores.
//   rocprim exclusive_scan  the flags to the slot of every grid brick (int): the direct-index brick -> slot
//                           map of every later kernel.  No hash table, no search.
//   brick_keys_kernel       one thread per grid brick: a stored brick writes its key at its slot, every
//                           other brick's slot becomes -1
//   brick_integrate_kernel  one workgroup of 512 per stored brick, a wave per 8 x 8 slab (x fastest), so a
//                           wave's voxels project to neighbouring pixels; the target loop is wave-uniform
//                           and the per-voxel body is pmvs_tsdf_voxel.h's, the dense kernel's.  A brick's
//                           512 values per array are written contiguously; an overhang voxel gets (1, 0, 0).
//   brick_classify_kernel   one workgroup per stored brick: stages the two predicates (observed, inside)
//                           of the 10^3 halo, voxels -1..8 per axis, as one byte each in LDS (1000 B) -- the
//                           neighbours' through the slot map, absent bricks and voxels outside the dims as
//                           unobserved -- then the active flags of the 9^3 cells -1..7 (729 B), then per
//                           voxel its own cell's flag and its 3 quad bits.  Classification reads nothing of
//                           a voxel but the two predicates, so the tile holds those and not the 4-byte
//                           values.  Bytes at strides 1 / 10 / 100: the 64 lanes of a slab read 20
//                           consecutive dwords (lanes of one dword broadcast), no bank is hit twice.
//   order                   the scans of the flags give counts and compaction offsets (64-bit); the active
//                           cells are compacted as (virtual cell index, stored voxel index) pairs and
//                           rocprim::radix_sort_pairs'ed on the bits the largest index needs: the rank is
//                           the vertex id, scattered into an int per stored voxel.  The same for the quads
//                           with the key virtual voxel index * 4 + axis.  Keys are unique.
//   brick_vertex_kernel     one thread per rank below vcap: the 8 corners through the slot map, then
//                           pmvsmesh::cell_vertex / cell_colour / voxel_coord as mesh_vertex_kernel
//   brick_face_kernel       one thread per quad rank below ceil(fcap / 2): the four cells' vertex ids through
//                           the slot map, mesh_face_kernel's winding
// Every virtual or stored index is 64-bit where it is formed; each kernel's guard stands at that place.
// Nothing depends on the order of the work.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>  // before rocprim, whose texture iterator calls memset without including it

#include <rocprim/rocprim.hpp>

#include "pmvs_brick.h"
#include "pmvs_device.h"
#include "pmvs_fuse.h"
#include "pmvs_launch.h"
#include "pmvs_mesh.h"
#include "pmvs_tsdf_voxel.h"

namespace pmvsdev {
namespace {

#define BCHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

using pmvsbrick::Grid;
enum { kBrick = pmvsbrick::kVoxels };

__global__ __launch_bounds__(256) void brick_mark_kernel(DScene s, TsdfMapsView m, pmvs_volume vol, int margin, Grid g,
                                                         unsigned char* __restrict__ flag) {
  const int j = blockIdx.y;
  if (j >= m.count) return;
  const DView& vw = s.views[m.first + j];
  const int W = vw.w[s.level], H = vw.h[s.level];
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long long)W * H) return;
  const long long c = m.off[j] + p;
  if (!m.pass[c]) return;
  float Sf[3];
  pmvsfuse::pixel_point(vw.P[s.level], vw.oaxis, (int)(p % W), (int)(p / W), m.depth[c], Sf);  // valid: the pixel passes
  int lo[3], hi[3];
  for (int a = 0; a < 3; ++a)
    if (!pmvsbrick::clipped_box(pmvsbrick::grid_coord(Sf[a], vol.origin[a], vol.voxel), margin, vol.dims[a], &lo[a], &hi[a])) return;
  // 0 <= lo <= hi <= dims - 1, so every brick below lies in the grid
  for (int bk = lo[2] >> 3; bk <= hi[2] >> 3; ++bk)
    for (int bj = lo[1] >> 3; bj <= hi[1] >> 3; ++bj)
      for (int bi = lo[0] >> 3; bi <= hi[0] >> 3; ++bi) flag[g.key(bi, bj, bk)] = 1;
}

// slot: the exclusive sums of the flags.  The first `stored` selected bricks keep their slot and write their
// key there; every other brick of the grid reads -1 from here on.
__global__ __launch_bounds__(256) void brick_keys_kernel(long long bricks, long long stored, const unsigned char* __restrict__ flag,
                                                         int* __restrict__ slot, long long* __restrict__ key) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= bricks) return;
  const int sl = slot[b];
  if (flag[b] && sl < stored)
    key[sl] = b;
  else
    slot[b] = -1;
}

__global__ __launch_bounds__(512) void brick_integrate_kernel(DScene s, TsdfMapsView m, pmvs_volume vol, float trunc, Grid g,
                                                              const long long* __restrict__ key, TsdfArrays out) {
  const long long sl = blockIdx.x;  // below the stored count: the grid is that size
  int bi, bj, bk;
  g.brick_of(key[sl], &bi, &bj, &bk);
  const int t = threadIdx.x;  // = local_index(li, lj, lk)
  const int i = 8 * bi + (t & 7), j = 8 * bj + ((t >> 3) & 7), k = 8 * bk + (t >> 6);
  // An edge brick runs the target loop with its overhang lanes masked off: the trip count and every view
  // load stay wave-uniform, only the exec mask differs.
  pmvsmesh::VoxelSums v;  // an overhang voxel keeps these: (1.0f, 0, 0)
  if (i < vol.dims[0] && j < vol.dims[1] && k < vol.dims[2]) v = tsdf_voxel(s, m, vol, trunc, i, j, k);
  tsdf_store(out, sl * kBrick + t, v);
}

// A caller's key list: strictly ascending and inside the grid, else *bad = 1 (every writer stores the same).
__global__ __launch_bounds__(256) void brick_keys_check_kernel(const long long* __restrict__ key, long long nb, long long bricks,
                                                               int* __restrict__ bad) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nb) return;
  const long long k = key[s];
  if (k < 0 || k >= bricks || (s > 0 && key[s - 1] >= k)) *bad = 1;
}
// After the check passed: every key lies in the grid.
__global__ __launch_bounds__(256) void brick_slot_scatter_kernel(const long long* __restrict__ key, long long nb, int* __restrict__ slot) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < nb) slot[key[s]] = (int)s;
}

struct BrickView {  // the virtual volume, by value to the extraction's kernels
  int n[3];
  Grid g;
  int min_obs;
  const int* slot;
  const float* tsdf;
  const unsigned char *obs, *color;  // color may be null
  // The array index of virtual voxel (i, j, k), or -1: outside the dims or in no stored brick.
  __device__ long long stored(int i, int j, int k) const {
    if (i < 0 || j < 0 || k < 0 || i >= n[0] || j >= n[1] || k >= n[2]) return -1;
    const int sl = slot[g.key(i >> 3, j >> 3, k >> 3)];
    return sl < 0 ? -1 : pmvsbrick::slot_voxel(sl, i & 7, j & 7, k & 7);
  }
  __device__ long long voxel(int i, int j, int k) const { return ((long long)k * n[1] + j) * n[0] + i; }
  __device__ long long cell(int i, int j, int k) const { return ((long long)k * (n[1] - 1) + j) * (n[0] - 1) + i; }
};

// This thread's voxel of the workgroup's brick.
__device__ __forceinline__ void own_voxel(const Grid& g, long long key, int* idx) {
  int bi, bj, bk;
  g.brick_of(key, &bi, &bj, &bk);
  const int t = threadIdx.x;
  idx[0] = 8 * bi + (t & 7), idx[1] = 8 * bj + ((t >> 3) & 7), idx[2] = 8 * bk + (t >> 6);
}

// active[v]: the cell whose lower corner is stored voxel v is active; bit a of quads[v]: the edge from v to
// its +a neighbour emits a quad.
__global__ __launch_bounds__(512) void brick_classify_kernel(BrickView b, const long long* __restrict__ key,
                                                             unsigned char* __restrict__ active, unsigned char* __restrict__ quads) {
  __shared__ unsigned char halo[1000];  // voxels -1..8: bit 0 observed, bit 1 inside
  __shared__ unsigned char cell[729];   // cells -1..7
  const long long sl = blockIdx.x;
  const int t = threadIdx.x;
  int bi, bj, bk;
  b.g.brick_of(key[sl], &bi, &bj, &bk);
  for (int e = t; e < 1000; e += 512) {
    const long long v = b.stored(8 * bi - 1 + e % 10, 8 * bj - 1 + (e / 10) % 10, 8 * bk - 1 + e / 100);
    halo[e] = v < 0 ? 0 : (unsigned char)((b.obs[v] >= b.min_obs ? 1 : 0) | (b.tsdf[v] < 0.0f ? 2 : 0));
  }
  __syncthreads();
  for (int e = t; e < 729; e += 512) {
    const int cx = e % 9, cy = (e / 9) % 9, cz = e / 81;
    bool observed[8], inside[8];
    for (int n = 0; n < 8; ++n) {
      const unsigned h = halo[((cz + (n >> 2)) * 10 + cy + ((n >> 1) & 1)) * 10 + cx + (n & 1)];
      observed[n] = h & 1, inside[n] = (h >> 1) & 1;
    }
    cell[e] = pmvsmesh::cell_active(observed, inside);  // a corner outside the dims is unobserved: no cell past nx - 2
  }
  __syncthreads();
  const int l[3] = {t & 7, (t >> 3) & 7, t >> 6};
  const int idx[3] = {8 * bi + l[0], 8 * bj + l[1], 8 * bk + l[2]};
  const int hs[3] = {1, 10, 100}, cs[3] = {1, 9, 81};
  const int h0 = ((l[2] + 1) * 10 + l[1] + 1) * 10 + l[0] + 1, c0 = ((l[2] + 1) * 9 + l[1] + 1) * 9 + l[0] + 1;
  const unsigned own = halo[h0];
  unsigned bits = 0;
  for (int a = 0; a < 3; ++a) {
    const int p = (a + 1) % 3, q = (a + 2) % 3;
    if (!(own & 1) || idx[a] + 1 >= b.n[a] || idx[p] < 1 || idx[p] > b.n[p] - 2 || idx[q] < 1 || idx[q] > b.n[q] - 2) continue;
    const unsigned w = halo[h0 + hs[a]];
    if (!(w & 1) || ((w >> 1) & 1) == ((own >> 1) & 1)) continue;
    const bool all = cell[c0] && cell[c0 - cs[p]] && cell[c0 - cs[q]] && cell[c0 - cs[p] - cs[q]];
    if (all) bits |= 1u << a;
  }
  const long long v = sl * kBrick + t;
  active[v] = cell[c0];
  quads[v] = (unsigned char)bits;
}

// pos: the exclusive sums of the active flags.
__global__ __launch_bounds__(512) void brick_cell_pairs_kernel(BrickView b, const long long* __restrict__ key,
                                                               const unsigned char* __restrict__ active, const long long* __restrict__ pos,
                                                               unsigned long long* __restrict__ ckey, long long* __restrict__ cval) {
  const long long v = (long long)blockIdx.x * kBrick + threadIdx.x;
  if (!active[v]) return;
  int idx[3];
  own_voxel(b.g, key[blockIdx.x], idx);
  const long long o = pos[v];  // below the count of active cells: the arrays are that size
  ckey[o] = (unsigned long long)b.cell(idx[0], idx[1], idx[2]);  // an active cell: idx <= n - 2
  cval[o] = v;
}

// pos: the exclusive sums of the voxels' quad counts.
__global__ __launch_bounds__(512) void brick_quad_pairs_kernel(BrickView b, const long long* __restrict__ key,
                                                               const unsigned char* __restrict__ quads, const long long* __restrict__ pos,
                                                               unsigned long long* __restrict__ qkey, long long* __restrict__ qval) {
  const long long v = (long long)blockIdx.x * kBrick + threadIdx.x;
  const unsigned bits = quads[v];
  if (!bits) return;
  int idx[3];
  own_voxel(b.g, key[blockIdx.x], idx);
  long long o = pos[v];
  const unsigned long long base = (unsigned long long)b.voxel(idx[0], idx[1], idx[2]) * 4;  // < 2^62: dims <= 2^20
  for (int a = 0; a < 3; ++a)
    if (bits & (1u << a)) {
      qkey[o] = base + a;
      qval[o++] = v;
    }
}

__global__ __launch_bounds__(256) void brick_rank_kernel(const long long* __restrict__ cval, long long n, int* __restrict__ vid) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n) vid[cval[r]] = (int)r;  // n <= INT_MAX: the pass checked
}

__global__ __launch_bounds__(256) void brick_vertex_kernel(BrickView b, pmvs_volume box, const unsigned long long* __restrict__ ckey,
                                                           long long n, MeshArrays out) {
  const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= n) return;  // n = min(vertices, vcap)
  const long long c = (long long)ckey[o];
  const long long cx = b.n[0] - 1, cy = b.n[1] - 1;
  const int idx[3] = {(int)(c % cx), (int)((c / cx) % cy), (int)(c / (cx * cy))};
  float val[8];
  unsigned char rgba[8][4];
  for (int k = 0; k < 8; ++k) {
    const long long v = b.stored(idx[0] + (k & 1), idx[1] + ((k >> 1) & 1), idx[2] + (k >> 2));  // stored: the cell is active
    val[k] = v < 0 ? 1.0f : b.tsdf[v];
    const uchar4 w = (b.color && v >= 0) ? reinterpret_cast<const uchar4*>(b.color)[v] : make_uchar4(0, 0, 0, 0);
    rgba[k][0] = w.x, rgba[k][1] = w.y, rgba[k][2] = w.z, rgba[k][3] = w.w;
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

__global__ __launch_bounds__(256) void brick_face_kernel(BrickView b, const unsigned long long* __restrict__ qkey,
                                                         const long long* __restrict__ qval, const int* __restrict__ vid, long long n,
                                                         long long fcap, int* __restrict__ face) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;  // n = min(quads, ceil(fcap / 2))
  const int a = (int)(qkey[r] & 3), p = (a + 1) % 3, q = (a + 2) % 3;
  const long long v = (long long)(qkey[r] >> 2);
  const int idx[3] = {(int)(v % b.n[0]), (int)((v / b.n[0]) % b.n[1]), (int)(v / ((long long)b.n[0] * b.n[1]))};
  const bool in0 = b.tsdf[qval[r]] < 0.0f;
  int Q[4];  // Q0 = (p-1, q-1), Q1 = (p, q-1), Q2 = (p, q), Q3 = (p-1, q): the cells the classification found active
  const int dp[4] = {1, 0, 0, 1}, dq[4] = {1, 1, 0, 0};
  for (int k = 0; k < 4; ++k) {
    int cc[3];
    cc[a] = idx[a], cc[p] = idx[p] - dp[k], cc[q] = idx[q] - dq[k];
    const long long c = b.stored(cc[0], cc[1], cc[2]);  // a cell is owned by its lower-corner voxel, stored: it is active
    Q[k] = c < 0 ? 0 : vid[c];
  }
  const int tri[2][3] = {{Q[0], in0 ? Q[1] : Q[2], in0 ? Q[2] : Q[1]}, {Q[0], in0 ? Q[2] : Q[3], in0 ? Q[3] : Q[2]}};
  long long f = 2 * r;
  for (int k = 0; k < 2; ++k, ++f)
    if (f < fcap) face[3 * f] = tri[k][0], face[3 * f + 1] = tri[k][1], face[3 * f + 2] = tri[k][2];
}

struct ByteCount {  // a 0 / 1 flag byte as a 64-bit count
  __host__ __device__ long long operator()(unsigned char b) const { return (long long)b; }
};
struct QuadCount {  // the quads of a voxel's flag byte
  __host__ __device__ long long operator()(unsigned char b) const { return (long long)((b & 1) + ((b >> 1) & 1) + ((b >> 2) & 1)); }
};

unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }
unsigned bits_of(unsigned long long largest) {  // the bits a key up to `largest` needs
  unsigned b = 1;
  while (b < 64 && (largest >> b)) ++b;
  return b;
}

BrickView view_of(const pmvs_volume& vol, int min_obs, const int* slot, const float* tsdf, const unsigned char* obs,
                  const unsigned char* color) {
  return BrickView{{vol.dims[0], vol.dims[1], vol.dims[2]}, pmvsbrick::grid_of(vol.dims), min_obs, slot, tsdf, obs, color};
}

// n (key, value) pairs sorted by the low `bits` bits of the key; the sorted arrays are *skey / *sval.
struct SortedPairs {
  DevBuf<unsigned long long> key[2];
  DevBuf<long long> val[2];
  DevBuf<char> temp;
  size_t temp_bytes = 0;
  unsigned bits = 64;
  hipError_t alloc(long long n, unsigned key_bits, hipStream_t st) {
    bits = key_bits;
    for (int h = 0; h < 2; ++h) {
      BCHK(key[h].alloc((size_t)n));
      BCHK(val[h].alloc((size_t)n));
    }
    BCHK(rocprim::radix_sort_pairs(nullptr, temp_bytes, key[0].p, key[1].p, val[0].p, val[1].p, (size_t)n, 0, bits, st));
    return temp.alloc(temp_bytes);
  }
  hipError_t sort(long long n, hipStream_t st) {
    return rocprim::radix_sort_pairs(temp.p, temp_bytes, key[0].p, key[1].p, val[0].p, val[1].p, (size_t)n, 0, bits, st);
  }
};

}  // namespace

hipError_t brick_select(const DScene& s, const FuseMaps& f, int first, int count, const pmvs_volume& vol, int margin,
                        BrickSelection& sel, hipStream_t st) {
  const Grid g = pmvsbrick::grid_of(vol.dims);
  const long long bricks = g.bricks();  // <= INT_MAX: the API checked
  sel.bricks = bricks;
  BCHK(sel.flag.alloc((size_t)bricks));
  BCHK(sel.slot.alloc((size_t)bricks));
  DevBuf<char> temp;
  size_t tb = 0;
  BCHK(rocprim::exclusive_scan(nullptr, tb, sel.flag.p, sel.slot.p, 0, (size_t)bricks, rocprim::plus<int>(), st));
  BCHK(temp.alloc(tb));
  BCHK(hipMemsetAsync(sel.flag.p, 0, (size_t)bricks, st));
  const TsdfMapsView m{f.depth.p, f.pass.p, f.off.p, first, count};
  hipLaunchKernelGGL(brick_mark_kernel, dim3(f.row_blocks, (unsigned)count), dim3(256), 0, st, s, m, vol, margin, g, sel.flag.p);
  BCHK(hipGetLastError());
  BCHK(rocprim::exclusive_scan(temp.p, tb, sel.flag.p, sel.slot.p, 0, (size_t)bricks, rocprim::plus<int>(), st));
  int last_slot = 0;
  unsigned char last_flag = 0;
  BCHK(hipMemcpyAsync(&last_slot, sel.slot.p + (bricks - 1), sizeof(int), hipMemcpyDeviceToHost, st));
  BCHK(hipMemcpyAsync(&last_flag, sel.flag.p + (bricks - 1), 1, hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));  // and the scan's storage is freed on return
  sel.total = (long long)last_slot + (last_flag ? 1 : 0);
  return hipSuccess;
}

hipError_t brick_keys(BrickSelection& sel, long long stored, long long* key, hipStream_t st) {
  hipLaunchKernelGGL(brick_keys_kernel, dim3(blocks_of(sel.bricks)), dim3(256), 0, st, sel.bricks, stored, sel.flag.p, sel.slot.p, key);
  return hipGetLastError();
}

hipError_t brick_integrate(const DScene& s, const FuseMaps& f, int first, int count, const pmvs_volume& vol, float trunc,
                           const long long* key, long long stored, const TsdfArrays& out, hipStream_t st) {
  if (stored < 1 || (!out.tsdf && !out.obs && !out.color)) return hipSuccess;
  const TsdfMapsView m{f.depth.p, f.pass.p, f.off.p, first, count};
  hipLaunchKernelGGL(brick_integrate_kernel, dim3((unsigned)stored), dim3(512), 0, st, s, m, vol, trunc, pmvsbrick::grid_of(vol.dims), key,
                     out);
  return hipGetLastError();
}

hipError_t brick_slots_from_keys(const pmvs_volume& vol, const long long* key, long long nb, DevBuf<int>& slot, bool* ok,
                                 hipStream_t st) {
  const long long bricks = pmvsbrick::grid_of(vol.dims).bricks();
  *ok = nb <= bricks;
  if (!*ok) return hipSuccess;
  BCHK(slot.alloc((size_t)bricks));
  BCHK(hipMemsetAsync(slot.p, 0xff, (size_t)bricks * sizeof(int), st));  // -1: in no stored brick
  if (nb < 1) return hipSuccess;
  DevBuf<int> bad;
  int host_bad = 0;
  BCHK(bad.alloc(1));
  BCHK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(brick_keys_check_kernel, dim3(blocks_of(nb)), dim3(256), 0, st, key, nb, bricks, bad.p);
  BCHK(hipGetLastError());
  BCHK(hipMemcpyAsync(&host_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  BCHK(hipStreamSynchronize(st));
  *ok = host_bad == 0;
  if (!*ok) return hipSuccess;  // nothing is scattered through keys that failed the check
  hipLaunchKernelGGL(brick_slot_scatter_kernel, dim3(blocks_of(nb)), dim3(256), 0, st, key, nb, slot.p);
  return hipGetLastError();
}

hipError_t brick_mesh_pass(const pmvs_volume& box, int min_obs, long long nb, const long long* key, const int* slot, const float* tsdf,
                           const unsigned char* obs, const unsigned char* color, long long vcap, long long fcap, const MeshArrays& out,
                           long long* nverts, long long* nfaces, hipStream_t st) {
  *nverts = *nfaces = 0;
  if (nb < 1 || box.dims[0] < 2 || box.dims[1] < 2 || box.dims[2] < 2) return hipSuccess;  // no cells
  const BrickView b = view_of(box, min_obs, slot, tsdf, obs, color);
  const long long voxels = nb * kBrick;  // stored
  const unsigned grid = (unsigned)nb;    // <= INT_MAX bricks

  // One 8-byte offset array serves both compactions, for memory: the quad counts are scanned once for the
  // total and again when the faces are written (a third scan over the stored voxels, in the filling call
  // only) rather than held in a second array of 8 bytes per stored voxel beside the cells' offsets.
  DevBuf<unsigned char> active, quads;
  DevBuf<long long> pos;
  DevBuf<int> vid;
  BCHK(active.alloc((size_t)voxels));
  BCHK(quads.alloc((size_t)voxels));
  BCHK(pos.alloc((size_t)voxels));
  const auto cell_counts = rocprim::make_transform_iterator(active.p, ByteCount());
  const auto quad_counts = rocprim::make_transform_iterator(quads.p, QuadCount());
  long long nv = 0, nq = 0;
  {
    DevBuf<char> temp;
    size_t tb_v = 0, tb_q = 0;
    BCHK(rocprim::exclusive_scan(nullptr, tb_v, cell_counts, pos.p, 0LL, (size_t)voxels, rocprim::plus<long long>(), st));
    BCHK(rocprim::exclusive_scan(nullptr, tb_q, quad_counts, pos.p, 0LL, (size_t)voxels, rocprim::plus<long long>(), st));
    BCHK(temp.alloc(tb_v > tb_q ? tb_v : tb_q));
    hipLaunchKernelGGL(brick_classify_kernel, dim3(grid), dim3(512), 0, st, b, key, active.p, quads.p);
    BCHK(hipGetLastError());
    // the counts: the last offset plus the last element's own
    unsigned char last_active = 0, last_quads = 0;
    long long last_pos = 0;
    BCHK(hipMemcpyAsync(&last_active, active.p + (voxels - 1), 1, hipMemcpyDeviceToHost, st));
    BCHK(hipMemcpyAsync(&last_quads, quads.p + (voxels - 1), 1, hipMemcpyDeviceToHost, st));
    BCHK(rocprim::exclusive_scan(temp.p, tb_q, quad_counts, pos.p, 0LL, (size_t)voxels, rocprim::plus<long long>(), st));
    BCHK(hipMemcpyAsync(&last_pos, pos.p + (voxels - 1), sizeof(long long), hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    nq = last_pos + QuadCount()(last_quads);
    // pos is left holding the cells' offsets, which are needed first
    BCHK(rocprim::exclusive_scan(temp.p, tb_v, cell_counts, pos.p, 0LL, (size_t)voxels, rocprim::plus<long long>(), st));
    BCHK(hipMemcpyAsync(&last_pos, pos.p + (voxels - 1), sizeof(long long), hipMemcpyDeviceToHost, st));
    BCHK(hipStreamSynchronize(st));
    nv = last_pos + (last_active ? 1 : 0);
  }
  *nverts = nv;
  *nfaces = 2 * nq;
  if (nv > INT_MAX) return hipSuccess;  // face ids are int: the API reports it
  const bool want_verts = vcap > 0 && nv > 0 && (out.vertex || out.normal || out.color);
  const bool want_faces = fcap > 0 && nq > 0 && out.face;
  if (!want_verts && !want_faces) return hipSuccess;  // the counting call sorts nothing

  const unsigned long long last_cell = (unsigned long long)((long long)(box.dims[0] - 1) * (box.dims[1] - 1) * (box.dims[2] - 1) - 1);
  const unsigned long long last_quad = (unsigned long long)box.dims[0] * box.dims[1] * box.dims[2] * 4;
  {
    SortedPairs sp;
    BCHK(sp.alloc(nv, bits_of(last_cell), st));
    hipLaunchKernelGGL(brick_cell_pairs_kernel, dim3(grid), dim3(512), 0, st, b, key, active.p, pos.p, sp.key[0].p, sp.val[0].p);
    BCHK(hipGetLastError());
    BCHK(sp.sort(nv, st));
    if (want_faces) {
      BCHK(vid.alloc((size_t)voxels));
      hipLaunchKernelGGL(brick_rank_kernel, dim3(blocks_of(nv)), dim3(256), 0, st, sp.val[1].p, nv, vid.p);
      BCHK(hipGetLastError());
    }
    if (want_verts) {
      const long long n = nv < vcap ? nv : vcap;
      hipLaunchKernelGGL(brick_vertex_kernel, dim3(blocks_of(n)), dim3(256), 0, st, b, box, sp.key[1].p, n, out);
      BCHK(hipGetLastError());
    }
    BCHK(hipStreamSynchronize(st));  // the pairs are freed here
  }
  if (want_faces) {
    active.release();
    SortedPairs sp;
    DevBuf<char> temp;
    size_t tb = 0;
    BCHK(sp.alloc(nq, bits_of(last_quad), st));
    BCHK(rocprim::exclusive_scan(nullptr, tb, quad_counts, pos.p, 0LL, (size_t)voxels, rocprim::plus<long long>(), st));
    BCHK(temp.alloc(tb));
    BCHK(rocprim::exclusive_scan(temp.p, tb, quad_counts, pos.p, 0LL, (size_t)voxels, rocprim::plus<long long>(), st));
    hipLaunchKernelGGL(brick_quad_pairs_kernel, dim3(grid), dim3(512), 0, st, b, key, quads.p, pos.p, sp.key[0].p, sp.val[0].p);
    BCHK(hipGetLastError());
    BCHK(sp.sort(nq, st));
    const long long half = (fcap + 1) / 2, n = nq < half ? nq : half;
    hipLaunchKernelGGL(brick_face_kernel, dim3(blocks_of(n)), dim3(256), 0, st, b, sp.key[1].p, sp.val[1].p, vid.p, n, fcap, out.face);
    BCHK(hipGetLastError());
    BCHK(hipStreamSynchronize(st));
  }
  return hipSuccess;
}

}  // namespace pmvsdev
