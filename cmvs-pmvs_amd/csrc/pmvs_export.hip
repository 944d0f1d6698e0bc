// pmvs_export.hip -- the model as compact, writer-ordered arrays, produced on the device
// (pmvs_loop_export / pmvs_export_patches, include/pmvs_amd.h).
//
// What pmvs2 did on the host after fetching every 1608-byte record -- the collectPatches(1) order
// (patchOrganizerS.cpp:207-236), the gather of the writers' fields and image lists, and writePLY's
// colours (patchOrganizerS.cpp:716-731) -- as three steps on the records where they lie:
//   export_key_kernel     per record: the order key, num_images, num_vimages (header + the first
//                         num_images list entries only)
//   hipcub SortPairs      (key, model index), stable, over the key bits in use; DeviceScan over the
//                         permuted counts gives the two 64-bit offset arrays
//   export_gather_kernel  one wavefront per output row: fields, both lists (lanes take entries, so
//                         the int16 loads and the id stores are coalesced) and the colour
// Plain HIP: the kernels are bandwidth-bound gathers.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>

#include "pmvs_device.h"
#include "pmvs_launch.h"

namespace pmvsdev {
namespace {

#define XCHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

constexpr int kKeyLanes = 16;  // lanes sharing one record in export_key_kernel

__device__ __forceinline__ int clamp_count(int c) { return c < 0 ? 0 : (c > PMVS_MAX_IMAGES ? PMVS_MAX_IMAGES : c); }

// Sum of num_images / num_vimages over the records (u64 adds: exact and order-free).
__global__ __launch_bounds__(256) void export_sizes_kernel(const pmvs_patch* __restrict__ P, int n,
                                                           unsigned long long* __restrict__ tot) {
  unsigned long long a = 0, b = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    a += (unsigned long long)clamp_count(P[i].num_images);
    b += (unsigned long long)clamp_count(P[i].num_vimages);
  }
  for (int d = 32; d >= 1; d >>= 1) {
    a += __shfl_xor(a, d);
    b += __shfl_xor(b, d);
  }
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(tot, a);
    if (b) atomicAdd(tot + 1, b);
  }
}

// The collectPatches(1) order key of every record (pmvs2 wrote patches in it): bt = the lowest view
// index below tnum in images, at its first position k0; key = (bt << cell_bits) + cell + bias with
// cell = grids[k0][1] * gwidth(bt) + grids[k0][0].  bias = 32768 * (widest target grid + 1) keeps the
// cell term non-negative for any int16 grid entry and 2^cell_bits exceeds it, so the keys order as
// (bt, cell) does; a record without a target image gets tnum << cell_bits and sorts last.
// kKeyLanes lanes share a record: they read its images entries side by side and reduce
// (index << 8 | position) with a minimum.  keys may be null (model order: counts only), and so may the
// two count arrays (export_order for a caller that wants the order alone).
__global__ __launch_bounds__(256) void export_key_kernel(DScene s, const pmvs_patch* __restrict__ P, int n, int cell_bits,
                                                         long long bias, unsigned long long* __restrict__ keys,
                                                         int* __restrict__ cnt_i, int* __restrict__ cnt_v) {
  const int sub = threadIdx.x & (kKeyLanes - 1);
  const long long stride = (long long)gridDim.x * (blockDim.x / kKeyLanes);
  const long long last = ((long long)n + stride - 1) / stride * stride;  // every lane of a wavefront runs the same trips
  for (long long i = (long long)blockIdx.x * (blockDim.x / kKeyLanes) + threadIdx.x / kKeyLanes; i < last; i += stride) {
    const bool live = i < n;
    const pmvs_patch* q = P + (live ? i : 0);
    const int ni = live ? clamp_count(q->num_images) : 0;
    int best = INT_MAX;
    if (keys)
      for (int k = sub; k < ni; k += kKeyLanes) {
        const int v = q->images[k];
        if (v >= 0 && v < s.tnum) {
          const int c = (v << 8) | k;
          best = c < best ? c : best;
        }
      }
    for (int d = kKeyLanes / 2; d >= 1; d >>= 1) {
      const int o = __shfl_xor(best, d);
      best = o < best ? o : best;
    }
    if (live && sub == 0) {
      if (cnt_i) cnt_i[i] = ni;
      if (cnt_v) cnt_v[i] = clamp_count(q->num_vimages);
      if (keys && best == INT_MAX) {
        keys[i] = (unsigned long long)s.tnum << cell_bits;
      } else if (keys) {
        const int bt = best >> 8, k0 = best & 0xff;
        const DView& v = s.views[bt];
        const long long gw = (v.w[s.level] + s.csize - 1) / s.csize;
        const long long cell = (long long)q->grids[k0][1] * gw + (long long)q->grids[k0][0];
        keys[i] = ((unsigned long long)bt << cell_bits) + (unsigned long long)(cell + bias);
      }
    }
  }
}

// Row r of the output is record src[r] (src null: r).  The rows' list lengths as 64-bit scan inputs,
// n + 1 entries (the last 0, so the exclusive sums end with the totals).
__global__ void export_counts_kernel(const int* __restrict__ src, const int* __restrict__ cnt_i, const int* __restrict__ cnt_v,
                                     int n, long long* __restrict__ out_i, long long* __restrict__ out_v) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n) return;
  const long long m = r == n ? 0 : (src ? src[r] : r);
  out_i[r] = r == n ? 0 : cnt_i[m];
  out_v[r] = r == n ? 0 : cnt_v[m];
}

__global__ void export_iota_kernel(int* __restrict__ a, int n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = (int)i;
}

// One wavefront per output row.  The record's first 11 floats are the writers' fields (coord, normal,
// ncc, dscale, ascale) and go out through lanes 0-10; lanes take list entries k, k + 64.  Colour
// (writePLY mode 0, as patch_colors_kernel): one project + get_color per lane, then the three sums in
// list order k = 0 .. n-1 in f32 -- every lane adds the same __shfl'ed values in that order, so the sum
// is the sequential one -- and __fdiv_rn, floor(m + 0.5f), the clamp to 255.  Out-of-image projections
// are clamped to the border texel as there.  Any output pointer may be null.
__global__ __launch_bounds__(256) void export_gather_kernel(DScene s, const pmvs_patch* __restrict__ P, int n,
                                                            const int* __restrict__ src, const int* __restrict__ tab,
                                                            const long long* __restrict__ ioff,
                                                            const long long* __restrict__ voff, float* __restrict__ fields,
                                                            int* __restrict__ colors, int* __restrict__ image_ids,
                                                            int* __restrict__ image_idx, int* __restrict__ vimage_ids) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * (blockDim.x / 64);
  for (long long r = (long long)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64; r < n; r += stride) {
    const pmvs_patch* q = P + (src ? src[r] : r);
    const long long io = ioff[r], vo = voff[r];
    const int ni = (int)(ioff[r + 1] - io), nv = (int)(voff[r + 1] - vo);
    if (fields && lane < 11) fields[r * 11 + lane] = reinterpret_cast<const float*>(q)[lane];
    const float c[4] = {q->coord[0], q->coord[1], q->coord[2], q->coord[3]};
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int base = 0; base < ni; base += 64) {
      const int k = base + lane;
      float rgb[3] = {0.0f, 0.0f, 0.0f};
      if (k < ni) {
        const int view = q->images[k];
        if (image_idx) image_idx[io + k] = view;
        if (image_ids) image_ids[io + k] = tab ? tab[view] : view;
        if (colors) {
          const DView& v = s.views[view];
          float ic[3];
          project(v, c, s.level, ic);
          const float mx = (float)(v.w[s.level] - 2), my = (float)(v.h[s.level] - 2);
          const float x = ic[0] < 0.0f ? 0.0f : (ic[0] > mx ? mx : ic[0]);
          const float y = ic[1] < 0.0f ? 0.0f : (ic[1] > my ? my : ic[1]);
          get_color(s, v, x, y, s.level, rgb);
        }
      }
      if (colors) {
        const int m = ni - base < 64 ? ni - base : 64;
        for (int j = 0; j < m; ++j) {
          acc[0] += __shfl(rgb[0], j);
          acc[1] += __shfl(rgb[1], j);
          acc[2] += __shfl(rgb[2], j);
        }
      }
    }
    if (colors && lane < 3) {
      int out = 0;  // a record without images has no colour (the writers never see one)
      if (ni > 0) {
        const float a = lane == 0 ? acc[0] : (lane == 1 ? acc[1] : acc[2]);
        const float m = __fdiv_rn(a, (float)ni);
        const int qv = (int)floor((double)(m + 0.5f));
        out = qv < 255 ? qv : 255;
      }
      colors[r * 3 + lane] = out;
    }
    if (vimage_ids)
      for (int k = lane; k < nv; k += 64) {
        const int view = q->vimages[k];
        vimage_ids[vo + k] = tab ? tab[view] : view;
      }
  }
}

inline int grid_for(long long items, int per_block) {
  const long long g = (items + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > (1 << 20) ? (1 << 20) : g));
}

}  // namespace

hipError_t export_sizes(const pmvs_patch* P, int n, unsigned long long* d_tot, hipStream_t st) {
  XCHK(hipMemsetAsync(d_tot, 0, 2 * sizeof(unsigned long long), st));
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(export_sizes_kernel, dim3(grid_for(n, 256 * 8)), dim3(256), 0, st, P, n, d_tot);
  return hipGetLastError();
}

// The writer order of the records (the one place it is computed: export_pass and depth_map_pass call
// this): export_key_kernel, then a stable radix sort of (key, model index) over the key bits in use.
hipError_t export_order(const DScene& s, const pmvs_patch* P, int n, int max_gwidth, int* sorted, int* cnt_i, int* cnt_v,
                        hipStream_t st) {
  if (n <= 0) return hipSuccess;
  // key layout (export_key_kernel): cell + bias below 2^cell_bits, the target index above
  const long long bias = 32768LL * (max_gwidth + 1);
  int cell_bits = 1, end_bit;
  while ((1LL << cell_bits) < 2 * bias) ++cell_bits;
  for (end_bit = cell_bits; ((long long)s.tnum >> (end_bit - cell_bits)) != 0; ++end_bit) {}
  DevBuf<unsigned long long> keys, keys2;
  DevBuf<int> idx;
  DevBuf<char> temp;
  size_t tb_sort = 0;
  XCHK(keys.alloc(n));
  XCHK(keys2.alloc(n));
  XCHK(idx.alloc(n));
  XCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, keys.p, keys2.p, idx.p, sorted, n, 0, end_bit, st));
  XCHK(temp.alloc(tb_sort));
  hipLaunchKernelGGL(export_key_kernel, dim3(grid_for(n, 256 / kKeyLanes)), dim3(256), 0, st, s, P, n, cell_bits, bias, keys.p,
                     cnt_i, cnt_v);
  XCHK(hipGetLastError());
  hipLaunchKernelGGL(export_iota_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, idx.p, n);
  XCHK(hipGetLastError());
  XCHK(hipcub::DeviceRadixSort::SortPairs(temp.p, tb_sort, keys.p, keys2.p, idx.p, sorted, n, 0, end_bit, st));
  // the scratch above is freed on return: the work that reads it must have finished
  return hipStreamSynchronize(st);
}

hipError_t export_pass(const DScene& s, const pmvs_patch* P, int n, bool writer_order, int max_gwidth, const int* d_tab,
                       const ExportArrays& out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const size_t n1 = (size_t)n + 1;
  DevBuf<int> cnt_i, cnt_v, idx2;
  DevBuf<long long> c64_i, c64_v, off_i, off_v;
  DevBuf<char> temp;
  XCHK(cnt_i.alloc(n));
  XCHK(cnt_v.alloc(n));
  XCHK(c64_i.alloc(n1));
  XCHK(c64_v.alloc(n1));
  long long *ioff = out.image_off, *voff = out.vimage_off;
  if (!ioff) {
    XCHK(off_i.alloc(n1));
    ioff = off_i.p;
  }
  if (!voff) {
    XCHK(off_v.alloc(n1));
    voff = off_v.p;
  }
  size_t tb_scan = 0;
  const int* src = nullptr;
  XCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan, c64_i.p, ioff, (int)n1, st));
  XCHK(temp.alloc(tb_scan));
  if (writer_order) {
    int* sorted = out.source;
    if (!sorted) {
      XCHK(idx2.alloc(n));
      sorted = idx2.p;
    }
    XCHK(export_order(s, P, n, max_gwidth, sorted, cnt_i.p, cnt_v.p, st));
    src = sorted;
  } else {  // model order: the counts only
    hipLaunchKernelGGL(export_key_kernel, dim3(grid_for(n, 256 / kKeyLanes)), dim3(256), 0, st, s, P, n, 0, 0LL,
                       (unsigned long long*)nullptr, cnt_i.p, cnt_v.p);
    XCHK(hipGetLastError());
    if (out.source) {
      hipLaunchKernelGGL(export_iota_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, out.source, n);
      XCHK(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(export_counts_kernel, dim3(grid_for((long long)n1, 256)), dim3(256), 0, st, src, cnt_i.p, cnt_v.p, n,
                     c64_i.p, c64_v.p);
  XCHK(hipGetLastError());
  XCHK(hipcub::DeviceScan::ExclusiveSum(temp.p, tb_scan, c64_i.p, ioff, (int)n1, st));
  XCHK(hipcub::DeviceScan::ExclusiveSum(temp.p, tb_scan, c64_v.p, voff, (int)n1, st));
  if (out.fields || out.colors || out.image_ids || out.image_idx || out.vimage_ids) {
    hipLaunchKernelGGL(export_gather_kernel, dim3(grid_for(n, 4)), dim3(256), 0, st, s, P, n, src, d_tab, ioff, voff,
                       out.fields, out.colors, out.image_ids, out.image_idx, out.vimage_ids);
    XCHK(hipGetLastError());
  }
  // the scratch above is freed on return: the work that reads it must have finished
  return hipStreamSynchronize(st);
}

}  // namespace pmvsdev
