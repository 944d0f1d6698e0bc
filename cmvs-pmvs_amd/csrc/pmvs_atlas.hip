// pmvs_atlas.hip -- a textured mesh baked into one atlas image (pmvs_mesh_atlas, include/pmvs_amd.h; the
// definition is pmvs_atlas.h): every face gets a right triangle of side n texels, two to a square cell, the
// cells of one side in one band of rows, and every atlas texel the colour of the surface point it stands for
// in its face's view.
//   atlas_ids_check_kernel  a caller's device face ids and views: one flag, read back before any is an index
//   atlas_classify_kernel   one thread per face: the three corners projected at level 0, the placed test, the
//                           side n as a class byte (0 = not placed) and the face's own id as the sort's value;
//                           a 256-bin histogram per workgroup in LDS, then one integer atomic per non-empty bin.
//                           The histogram's read-back sizes everything: the call's one synchronisation besides
//                           the validity flag's.
//   rocprim radix_sort_pairs  (class byte, face id) on 8 bits: stable, so the faces of a class are in ascending
//                           face id.  A class's faces start at the sum of the smaller classes' counts.
//   atlas_uv_kernel         one thread per sorted position: rank -> cell -> the three corners, scattered to the
//                           face's uv and atlas_view
//   atlas_render_kernel     one workgroup per 256 texels of one atlas row, so that the row, its band and the
//                           band's c, k and y0 are uniform (the band table, at most 251 entries, is searched
//                           with scalar loads).  Per texel: the cell's face through the sorted order, the
//                           barycentric point in f64, one projection, one bilinear fetch of four RGBA8 words.
//                           The 768 colour bytes of the workgroup go through LDS and leave as dwords (bytes only
//                           up to the first and after the last aligned dword of the segment).
// No float atomics; the only atomics are the histogram's integer adds.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>  // before rocprim, whose texture iterator calls memset without including it

#include <rocprim/rocprim.hpp>

#include "pmvs_atlas.h"
#include "pmvs_device.h"
#include "pmvs_launch.h"

namespace pmvsdev {
namespace {

#define ACHK(expr)                        \
  do {                                    \
    const hipError_t e_ = (expr);         \
    if (e_ != hipSuccess) return e_;      \
  } while (0)

constexpr int kClasses = PMVS_ATLAS_MAX_SIDE + 1;  // class 0 = not placed
constexpr int kSegment = 256;                      // texels of a row one workgroup renders

__global__ __launch_bounds__(256) void atlas_ids_check_kernel(const int* __restrict__ face, long long ids, int nv,
                                                              const int* __restrict__ view, int tnum, int* __restrict__ bad) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ids) return;
  const int v = face[i];
  bool wrong = v < 0 || v >= nv;
  if (i % 3 == 0) {
    const int t = view[i / 3];
    wrong = wrong || t < -1 || t >= tnum;
  }
  if (wrong) *bad = 1;  // every writer stores the same
}

// Face f's corners in its view at level 0.
__device__ __forceinline__ void project_corners(const DScene& s, int t, const float V[3][4], float ic[3][3]) {
  for (int k = 0; k < 3; ++k) project(s.views[t], V[k], 0, ic[k]);
}

__global__ __launch_bounds__(256) void atlas_classify_kernel(DScene s, MeshView m, const int* __restrict__ view, float scale, int M,
                                                             unsigned char* __restrict__ cls, int* __restrict__ ids,
                                                             unsigned int* __restrict__ hist) {
  __shared__ unsigned int h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f < m.nf) {
    const int t = view[f];
    int n = 0;
    if (t >= 0) {
      float V[3][4], ic[3][3];
      load_face(m, (int)f, V);
      project_corners(s, t, V, ic);
      if (pmvsatlas::corners_placed(ic)) n = pmvsatlas::face_side(ic, scale, M);  // 1 <= n <= M <= 251
    }
    cls[f] = (unsigned char)n;
    ids[f] = (int)f;
    atomicAdd(&h[n], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kClasses && h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// tab[n] = (base, y0) of class n: the position of its first face in the order, its band's first row.
__global__ __launch_bounds__(256) void atlas_uv_kernel(int nf, int W, const int* __restrict__ order,
                                                       const unsigned char* __restrict__ cls_sorted, const int2* __restrict__ tab,
                                                       float* __restrict__ uv, int* __restrict__ atlas_view) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nf) return;
  const long long f = order[p];  // a permutation of [0, nf): the sort's values
  const int n = cls_sorted[p];
  float out[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (n > 0) {
    const int2 e = tab[n];  // n <= 251: the table has kClasses entries
    for (int k = 0; k < 3; ++k) {
      long long x, y;
      pmvsatlas::face_corner(W, n, e.y, (int)(p - e.x), k, &x, &y);
      out[2 * k] = (float)x, out[2 * k + 1] = (float)y;
    }
  }
  if (uv)
    for (int k = 0; k < 6; ++k) uv[6 * f + k] = out[k];
  if (atlas_view) atlas_view[f] = n > 0 ? 0 : -1;
}

// Rows [row0, row0 + gridDim.x / segs) of the atlas, all below min(H, height_cap); segs = the 256-texel segments
// of a row.
__global__ __launch_bounds__(256) void atlas_render_kernel(DScene s, MeshView m, const int* __restrict__ view,
                                                           const int* __restrict__ order, const pmvsatlas::Band* __restrict__ bands,
                                                           int nb, int W, int row0, int segs, unsigned char* __restrict__ rgb,
                                                           int* __restrict__ texel_face) {
  __shared__ unsigned char stage[3 * kSegment];
  const int tid = threadIdx.x;
  const int row = row0 + (int)(blockIdx.x / (unsigned)segs), I0 = (int)(blockIdx.x % (unsigned)segs) * kSegment;  // uniform
  const pmvsatlas::Band b = bands[pmvsatlas::band_of_row(bands, nb, row)];
  const int I = I0 + tid;
  int f = -1;
  unsigned char px[3] = {0, 0, 0};
  pmvsatlas::Texel tx;
  if (I < W && pmvsatlas::texel_of(W, b.n, b.count, I, row - b.y0, &tx)) {
    f = order[b.base + tx.rank];  // rank < count: inside the class's part of the order; f in [0, nf)
    const int t = view[f];        // >= 0: the face is placed
    float V[3][4], X[4], ic[3];
    load_face(m, f, V);
    pmvsatlas::surface_point(V[0], V[1], V[2], tx.l1, tx.l2, X);
    const DView& vw = s.views[t];
    project(vw, X, 0, ic);
    if (pmvsatlas::sample_ok(ic)) {
      float c[3];
      // clamped to [0, w - 2] x [0, h - 2]: get_color's four texels lie inside the level-0 image
      get_color(s, vw, pmvsatlas::sample_clamp(ic[0], vw.w[0]), pmvsatlas::sample_clamp(ic[1], vw.h[0]), 0, c);
      for (int a = 0; a < 3; ++a) px[a] = pmvsatlas::color_byte(c[a]);
    }
  }
  if (texel_face && I < W) texel_face[(long long)row * W + I] = f;
  if (!rgb) return;  // uniform
  for (int a = 0; a < 3; ++a) stage[3 * tid + a] = px[a];
  __syncthreads();
  // the segment's bytes [0, nbytes) go to dst: bytes up to the first aligned dword, dwords, bytes after the last
  const int nbytes = 3 * (W - I0 < kSegment ? W - I0 : kSegment);
  unsigned char* dst = rgb + 3 * ((long long)row * W + I0);
  int head = (int)((4u - (unsigned)((unsigned long long)dst & 3u)) & 3u);
  head = head < nbytes ? head : nbytes;
  const int nd = (nbytes - head) >> 2, tail0 = head + 4 * nd;
  if (tid < nd) {
    const unsigned char* q = stage + head + 4 * tid;
    *reinterpret_cast<unsigned int*>(dst + head + 4 * tid) =
        (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16) | ((unsigned)q[3] << 24);
  } else if (tid >= 248) {  // nd <= 192: these lanes are free
    const int o = tid - 248;  // 0 .. 7: the head's (at most 3) then the tail's (at most 3) bytes
    if (o < head) dst[o] = stage[o];
    else if (o >= 4 && tail0 + (o - 4) < nbytes) dst[tail0 + (o - 4)] = stage[tail0 + (o - 4)];
  }
}

unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256 < 1 ? 1 : (n + 255) / 256); }

}  // namespace

hipError_t atlas_ids_check(const int* face, const int* view, long long nf, long long nv, int tnum, bool* ok, hipStream_t st) {
  *ok = true;
  if (nf < 1) return hipSuccess;
  DevBuf<int> bad;
  int host_bad = 0;
  ACHK(bad.alloc(1));
  ACHK(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  hipLaunchKernelGGL(atlas_ids_check_kernel, dim3(blocks_of(3 * nf)), dim3(256), 0, st, face, 3 * nf, (int)nv, view, tnum, bad.p);
  ACHK(hipGetLastError());
  ACHK(hipMemcpyAsync(&host_bad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  ACHK(hipStreamSynchronize(st));
  *ok = host_bad == 0;
  return hipSuccess;
}

hipError_t atlas_classify(const DScene& s, const pmvs_atlas_params& prm, const float* vertex, long long nf, const int* face,
                          const int* view, AtlasWork& w, long long* counts, hipStream_t st) {
  for (int n = 0; n < kClasses; ++n) counts[n] = 0;
  if (nf < 1) return hipSuccess;
  DevBuf<unsigned int> hist;
  unsigned int host_hist[256];
  ACHK(hist.alloc(256));
  ACHK(w.cls.alloc((size_t)nf));
  ACHK(w.ids.alloc((size_t)nf));
  ACHK(hipMemsetAsync(hist.p, 0, sizeof(host_hist), st));
  const MeshView m{vertex, face, (int)nf};
  hipLaunchKernelGGL(atlas_classify_kernel, dim3(blocks_of(nf)), dim3(256), 0, st, s, m, view, prm.scale, prm.max_side, w.cls.p,
                     w.ids.p, hist.p);
  ACHK(hipGetLastError());
  ACHK(hipMemcpyAsync(host_hist, hist.p, sizeof(host_hist), hipMemcpyDeviceToHost, st));
  ACHK(hipStreamSynchronize(st));
  for (int n = 0; n < kClasses; ++n) counts[n] = host_hist[n];
  return hipSuccess;
}

hipError_t atlas_render_pass(const DScene& s, const pmvs_atlas_params& prm, const float* vertex, long long nf, const int* face,
                             const int* view, AtlasWork& w, const long long* counts, const long long* band_y, long long rows,
                             const AtlasArrays& out, hipStream_t st) {
  const bool images = rows > 0 && (out.rgb || out.texel_face);
  if (nf < 1 || !(images || out.uv || out.atlas_view)) return hipSuccess;
  const int W = prm.width;
  // the (class, face id) order
  DevBuf<char> temp;
  size_t temp_bytes = 0;
  ACHK(w.cls_sorted.alloc((size_t)nf));
  ACHK(w.order.alloc((size_t)nf));
  ACHK(rocprim::radix_sort_pairs(nullptr, temp_bytes, w.cls.p, w.cls_sorted.p, w.ids.p, w.order.p, (size_t)nf, 0, 8, st));
  ACHK(temp.alloc(temp_bytes));
  ACHK(rocprim::radix_sort_pairs(temp.p, temp_bytes, w.cls.p, w.cls_sorted.p, w.ids.p, w.order.p, (size_t)nf, 0, 8, st));
  // the classes' tables: (base, y0) per class for the uv kernel, the non-empty bands in layout order for the render
  int2 tab[kClasses];
  pmvsatlas::Band bands[kClasses];
  int nb = 0;
  long long base = 0;
  for (int n = 0; n < kClasses; ++n) {
    tab[n] = make_int2((int)base, n > 0 && n <= prm.max_side ? (int)band_y[n] : 0);
    base += counts[n];
  }
  for (int n = prm.max_side; n >= 1; --n)
    if (counts[n] > 0) bands[nb++] = pmvsatlas::Band{(int)band_y[n], n, (int)counts[n], tab[n].x};
  DevBuf<int2> d_tab;
  DevBuf<pmvsatlas::Band> d_bands;
  ACHK(d_tab.alloc(kClasses));
  ACHK(d_bands.alloc((size_t)kClasses));
  ACHK(hipMemcpyAsync(d_tab.p, tab, sizeof(tab), hipMemcpyHostToDevice, st));
  if (nb) ACHK(hipMemcpyAsync(d_bands.p, bands, sizeof(pmvsatlas::Band) * (size_t)nb, hipMemcpyHostToDevice, st));
  if (out.uv || out.atlas_view) {
    hipLaunchKernelGGL(atlas_uv_kernel, dim3(blocks_of(nf)), dim3(256), 0, st, (int)nf, W, w.order.p, w.cls_sorted.p, d_tab.p, out.uv,
                       out.atlas_view);
    ACHK(hipGetLastError());
  }
  if (images && nb > 0) {
    const MeshView m{vertex, face, (int)nf};
    const int segs = (W + kSegment - 1) / kSegment;
    const long long per_launch = (long long)(INT_MAX / 2) / segs;  // rows of one grid
    for (long long row0 = 0; row0 < rows; row0 += per_launch) {
      const long long r = rows - row0 < per_launch ? rows - row0 : per_launch;
      hipLaunchKernelGGL(atlas_render_kernel, dim3((unsigned)(r * segs)), dim3(256), 0, st, s, m, view, w.order.p, d_bands.p, nb, W,
                         (int)row0, segs, out.rgb, out.texel_face);
      ACHK(hipGetLastError());
    }
  }
  // the scratch above and the host tables are released on return: the work that reads them must have finished
  return hipStreamSynchronize(st);
}

}  // namespace pmvsdev
