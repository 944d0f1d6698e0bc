// pmvs_api.cpp -- the C-ABI (include/pmvs_amd.h) on top of the HIP kernels.
//
// Host responsibilities (C++, no torch types): scene validation, camera setup restated from
// the reference's CCamera (camera.cpp:56-173) and COptim::setAxesScales (optim.cpp:43-64),
// device allocation of the pyramid / camera / visibility tables, kernel launches on one HIP
// stream per scene, HIP-event timing, and error mapping (never exit(); PMVS_EDEVICE + message).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/pmvs_amd.h"
#include "pmvs_atlas.h"
#include "pmvs_brick.h"
#include "pmvs_features.h"
#include "pmvs_fmt.h"
#include "pmvs_launch.h"

using namespace pmvsdev;

namespace {

thread_local std::string g_err = "";

pmvs_status fail(pmvs_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return st;
}

}  // namespace

pmvs_status pmvs_io_fail(pmvs_status st, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return st;
}

namespace {

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (expr);                                                                       \
    if (e_ != hipSuccess) return fail(PMVS_EDEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// ---- host restatement of the reference camera setup (CONTOUR projection given as 12 floats)
static inline float dot4f(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }
static inline float dot3f(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static inline void cross3f(const float* u, const float* v, float* o) {
  o[0] = u[1] * v[2] - v[1] * u[2];
  o[1] = -u[0] * v[2] + v[0] * u[2];
  o[2] = u[0] * v[1] - v[0] * u[1];
}
static inline void unitize3f(float* v) {
  const float l = dot3f(v, v);
  if (l != 1.0 && l != 0.0) {
    const float d = (float)std::sqrt((double)l);
    v[0] /= d; v[1] /= d; v[2] /= d;
  }
}

// CCamera::updateProjection / updateCamera / getOpticalCenter (camera.cpp:56-173), txtType 0.
void setup_camera(DView& v, const float* p12, int maxLevel) {
  for (int i = 0; i < 12; ++i) v.P[0][i] = p12[i];
  for (int level = 1; level < maxLevel; ++level) {
    for (int i = 0; i < 12; ++i) v.P[level][i] = v.P[level - 1][i];
    for (int x = 0; x < 4; ++x) {
      v.P[level][x] /= 2.0f;
      v.P[level][4 + x] /= 2.0f;
    }
  }
  for (int level = maxLevel; level < MAXL; ++level) std::memcpy(v.P[level], v.P[maxLevel - 1], sizeof(v.P[0]));
  float oa[4] = {v.P[0][8], v.P[0][9], v.P[0][10], 0.0f};
  const float ftmp = (float)std::sqrt((double)dot4f(oa, oa));
  oa[3] = v.P[0][11];
  for (int i = 0; i < 4; ++i) oa[i] /= ftmp;
  for (int i = 0; i < 4; ++i) v.oaxis[i] = oa[i];
  if (v.P[0][8] == 0.0 && v.P[0][9] == 0.0 && v.P[0][10] == 0.0) {
    float a[3] = {v.P[0][0], v.P[0][1], v.P[0][2]}, b[3] = {v.P[0][4], v.P[0][5], v.P[0][6]}, c[3];
    cross3f(a, b, c);
    unitize3f(c);
    v.center[0] = c[0]; v.center[1] = c[1]; v.center[2] = c[2]; v.center[3] = 0.0f;
  } else {
    double A[3][3], b[3];
    for (int y = 0; y < 3; ++y) {
      for (int x = 0; x < 3; ++x) A[y][x] = v.P[0][4 * y + x];
      b[y] = -(double)v.P[0][4 * y + 3];
    }
    auto cr = [](const double* u, const double* w, double* o) {
      o[0] = u[1] * w[2] - w[1] * u[2];
      o[1] = -u[0] * w[2] + w[0] * u[2];
      o[2] = u[0] * w[1] - w[0] * u[1];
    };
    double ad[3][3];
    cr(A[1], A[2], ad[0]);
    cr(A[2], A[0], ad[1]);
    cr(A[0], A[1], ad[2]);
    const double det = ad[0][0] * A[0][0] + ad[0][1] * A[0][1] + ad[0][2] * A[0][2];
    double inv[3][3] = {{0}};
    if (det != 0.0)
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) inv[r][c] = ad[c][r] / det;
    for (int r = 0; r < 3; ++r) v.center[r] = (float)(inv[r][0] * b[0] + inv[r][1] * b[1] + inv[r][2] * b[2]);
    v.center[3] = 1.0f;
  }
  // COptim::setAxesScales (optim.cpp:43-64)
  float z[3] = {oa[0], oa[1], oa[2]}, x[3] = {v.P[0][0], v.P[0][1], v.P[0][2]}, y[3];
  cross3f(z, x, y);
  unitize3f(y);
  cross3f(y, z, x);
  for (int i = 0; i < 3; ++i) { v.xaxis[i] = x[i]; v.yaxis[i] = y[i]; v.zaxis[i] = z[i]; }
  const float xa[4] = {x[0], x[1], x[2], 0.0f}, ya[4] = {y[0], y[1], y[2], 0.0f};
  const float p0[4] = {v.P[0][0], v.P[0][1], v.P[0][2], v.P[0][3]}, p1[4] = {v.P[0][4], v.P[0][5], v.P[0][6], v.P[0][7]};
  const float fx = dot4f(xa, p0), fy = dot4f(ya, p1);
  v.ipscale = fx + fy;
}

// CImage::buildMask / buildEdge (image.cpp:327-405) on the host (binary maps are optional).
void build_binary(std::vector<uint8_t>* pyr, const int* w, const int* h, int maxLevel) {
  for (int level = 1; level < maxLevel; ++level) {
    pyr[level].assign((size_t)w[level] * h[level], 0);
    for (int y = 0; y < h[level]; ++y) {
      const int ys[2] = {2 * y, std::min(h[level - 1] - 1, 2 * y + 1)};
      for (int x = 0; x < w[level]; ++x) {
        const int xs[2] = {2 * x, std::min(w[level - 1] - 1, 2 * x + 1)};
        int in = 0;
        for (int j = 0; j < 2; ++j)
          for (int i = 0; i < 2; ++i)
            if (pyr[level - 1][ys[j] * w[level - 1] + xs[i]]) in++;
        pyr[level][y * w[level] + x] = (0 < in) ? 255 : 0;
      }
    }
  }
}

}  // namespace

struct pmvs_scene {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t kev[4] = {nullptr, nullptr, nullptr, nullptr};  // around pre / refine / post kernels
  bool last_refine = false;
  DScene ds{};
  int maxLevel = 0;
  std::vector<DView> hviews;
  DevBuf<DView> views;
  DevBuf<uint32_t> pyr;
  DevBuf<uint8_t> masks, edges;
  DevBuf<int> vis_off, vis, bindexes;
  DevBuf<float> scratch;
  DevBuf<DevStats> stats;
  DevBuf<RefineJob> jobs;
  FilterBuffers fbuf;
  ExpandBuffers xbuf;
  DevBuf<pmvs_patch> fpatches;
  DevBuf<int> fkeep;
  DevBuf<unsigned long long> digest;  // pmvs_loop_hash
  int grid = 0, refine_grid = 0;
  RefineLayout layout = split_layout(2, 5, 19);  // pmvs_refine_layouts.h
  // batches below small_n candidates run the lane form, one candidate per wavefront with its BOBYQA
  // state over the lanes (layout_small, pmvs_refine_lane.hip): their length is one chain's latency,
  // not the chip's throughput (the C3 loop, gpurun r06d: small launches 1029 -> 687 ms
  // per step against the retired workgroup form, split point 7000 against 5000 / 10000)
  RefineLayout layout_small = lane_layout(0);
  int small_n = 7000;
  const RefineLayout& refine_cfg(int n) const { return n < small_n ? layout_small : layout; }
  // expansion sharding (pmvs_scene_set_shard) and the kept result of pmvs_expand_run(out = NULL)
  int shard_rank = 0, shard_world = 1;
  pmvs_allgather_fn shard_fn = nullptr;
  void* shard_ctx = nullptr;
  pmvs_rccl* shard_rccl = nullptr;  // set: the records go device to device (pmvs_scene_set_shard_rccl)
  // cluster boundary exchange (pmvs_scene_set_cluster)
  int cl_rank = 0, cl_world = 1;
  pmvs_allgather_fn cl_fn = nullptr;
  void* cl_ctx = nullptr;
  pmvs_rccl* cl_rccl = nullptr;
  DevBuf<unsigned char> cl_shared;
  DevBuf<int> cl_ids, cl_id2idx;
  int cl_maxid = -1;
  ClusterBuffers cbuf;
  RefineHost rhost;             // host libm step of every refine batch (launch_refine)
  int xkept = -1, lkept = -1;   // models kept on the device for pmvs_expand_fetch / pmvs_loop_fetch
  std::vector<pmvs_patch> skept; // seeds kept for pmvs_seed_fetch (pmvs_seed_run with out = NULL, cap = 0)
  bool seeds_kept = false;
  std::vector<int> xalive;
  DevBuf<pmvs_patch> fpatches2;   // compaction target of pmvs_run_loop
  FeatBuffers feat;             // feature-detection scratch (pmvs_detect_features)
  // host copies the seed phase's control logic reads (canAdd masks, collectImages inputs)
  std::vector<std::vector<uint8_t>> hmask_level;  // per view, the binary mask at the scene level (empty = none)
  std::vector<int> hvis_off, hvis;
  int sequence = -1;
  // staging for host-pointer calls
  DevBuf<pmvs_candidate> cand;
  DevBuf<pmvs_refined> res;
  DevBuf<pmvs_eval_query> evq;
  DevBuf<double> evout;
  DevBuf<pmvs_tex_query> tq;
  DevBuf<float> tout;
  DevBuf<int> tvalid;
  ~pmvs_scene() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    for (hipEvent_t e : kev)
      if (e) (void)hipEventDestroy(e);
    if (stream) d2h_stage_release(stream);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

namespace {
template <class T>
pmvs_status ensure(DevBuf<T>& b, size_t n) {
  if (b.cap >= n) return PMVS_OK;
  hipError_t e = b.alloc(n);
  if (e != hipSuccess) return fail(PMVS_ENOMEM, "hipMalloc(%zu bytes): %s", n * sizeof(T), hipGetErrorString(e));
  return PMVS_OK;
}
int grow_alive(pmvs_scene* sc, int n) {
  return sc->xbuf.alive.grow((size_t)n) != hipSuccess;
}
}  // namespace

extern "C" {

const char* pmvs_last_error(void) { return g_err.c_str(); }

int32_t pmvs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

pmvs_status pmvs_scene_create(const pmvs_scene_desc* d, int32_t device, pmvs_scene** out) {
  if (!d || !out) return fail(PMVS_EINVAL, "null argument");
  *out = nullptr;
  if (d->num_views < 1 || d->num_targets < 1 || d->num_targets > d->num_views)
    return fail(PMVS_EINVAL, "num_views=%d num_targets=%d", d->num_views, d->num_targets);
  if (d->level < 0 || d->level > PMVS_MAX_LEVEL) return fail(PMVS_EUNSUPPORTED, "level %d outside 0..%d", d->level, PMVS_MAX_LEVEL);
  if (d->wsize != 5 && d->wsize != 7 && d->wsize != 9) return fail(PMVS_EUNSUPPORTED, "wsize %d (supported: 5, 7, 9)", d->wsize);
  if (d->csize < 1) return fail(PMVS_EINVAL, "csize %d", d->csize);
  if (d->min_image_num < 1) return fail(PMVS_EINVAL, "minImageNum %d", d->min_image_num);
  const int tau = std::min(d->min_image_num * 2, d->num_views);
  if (tau > PMVS_MAX_TAU) return fail(PMVS_EUNSUPPORTED, "tau = min(2*minImageNum, num) = %d > %d", tau, PMVS_MAX_TAU);
  if (!d->views || !d->visdata2_offsets) return fail(PMVS_EINVAL, "views / visdata2 missing");
  {  // the organizer and commit records index target cells (pgrids) with 32-bit ints
    long long cells = 0;
    for (int t = 0; t < d->num_targets; ++t) {
      long long w = d->views[t].width, h = d->views[t].height;
      for (int l = 0; l < d->level; ++l) { w /= 2; h /= 2; }
      const long long gw = (w + d->csize - 1) / d->csize, gh = (h + d->csize - 1) / d->csize;
      // pmvs_patch keeps cell coordinates as int16 (include/pmvs_amd.h)
      if (gw > 32767 || gh > 32767) return fail(PMVS_EUNSUPPORTED, "view %d: %lld x %lld cells (at most 32767 a side)", t, gw, gh);
      cells += gw * gh;
    }
    if (cells > INT_MAX) return fail(PMVS_EUNSUPPORTED, "%lld target cells at level %d exceed 2^31 - 1", cells, d->level);
  }
  if (d->num_views > 32767) return fail(PMVS_EUNSUPPORTED, "%d views (pmvs_patch image indexes are 16-bit)", d->num_views);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PMVS_EDEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(PMVS_EINVAL, "device %d of %d", device, ndev);
  HIPCHK(hipSetDevice(device));

  (void)hipGetLastError();  // launches below are checked with hipGetLastError: start from a clean slate
  pmvs_scene* sc = new pmvs_scene();
  sc->device = device;
  const int num = d->num_views;
  const int maxLevel = std::max(1, d->level + 3);
  sc->maxLevel = maxLevel;
  auto bail = [&](pmvs_status st) {
    delete sc;
    return st;
  };
  if (hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&sc->ev0) != hipSuccess || hipEventCreate(&sc->ev1) != hipSuccess ||
      hipEventCreate(&sc->kev[0]) != hipSuccess || hipEventCreate(&sc->kev[1]) != hipSuccess ||
      hipEventCreate(&sc->kev[2]) != hipSuccess || hipEventCreate(&sc->kev[3]) != hipSuccess)
    return bail(fail(PMVS_EDEVICE, "stream/event creation failed"));

  // ---- views: sizes, cameras, pyramid offsets
  sc->hviews.assign(num, DView{});
  long long words = 0;
  bool anyMask = false, anyEdge = false;
  for (int i = 0; i < num; ++i) {
    const pmvs_view_desc& vd = d->views[i];
    if (vd.width < 8 || vd.height < 8 || !vd.rgb) return bail(fail(PMVS_EINVAL, "view %d: bad image", i));
    DView& v = sc->hviews[i];
    v.w[0] = vd.width;
    v.h[0] = vd.height;
    for (int l = 1; l < MAXL; ++l) {
      v.w[l] = l < maxLevel ? v.w[l - 1] / 2 : 0;
      v.h[l] = l < maxLevel ? v.h[l - 1] / 2 : 0;
    }
    for (int l = 0; l < MAXL; ++l) {
      v.pyr_off[l] = words;
      if (l < maxLevel) words += (long long)v.w[l] * v.h[l] + 1;  // +1 pad word: bilinear reads lx+1
      v.mask_off[l] = -1;
      v.edge_off[l] = -1;
    }
    setup_camera(v, vd.projection, maxLevel);
    anyMask |= vd.mask != nullptr;
    anyEdge |= vd.edge != nullptr;
  }
  if (hipMalloc((void**)&sc->pyr.p, words * sizeof(uint32_t)) != hipSuccess)
    return bail(fail(PMVS_ENOMEM, "pyramid: %lld words", words));
  sc->pyr.cap = words;
  if (memset_big(sc->pyr.p, 0, words * sizeof(uint32_t), sc->stream) != hipSuccess)
    return bail(fail(PMVS_EDEVICE, "pyramid: clearing %lld words", words));

  // ---- pyramids on device: RGB level chain (CImage::buildImage) then RGBA packing
  {
    size_t maxrgb = 0;
    for (int i = 0; i < num; ++i) maxrgb = std::max(maxrgb, (size_t)d->views[i].width * d->views[i].height * 3);
    uint8_t *a = nullptr, *b = nullptr, *pin = nullptr;
    // host images go up through a pinned bounce buffer, in pieces: a direct pageable copy out of a
    // multi-GB host array (70 views x 8K = 7 GB, sliced per view) failed with "invalid resource
    // handle" (gpurun r03q), and pinned pieces also keep the copy at full PCIe rate
    constexpr size_t kPin = size_t(32) << 20;
    if (hipMalloc((void**)&a, maxrgb) != hipSuccess || hipMalloc((void**)&b, maxrgb) != hipSuccess ||
        hipHostMalloc((void**)&pin, 2 * kPin, hipHostMallocDefault) != hipSuccess) {
      if (a) (void)hipFree(a);
      if (b) (void)hipFree(b);
      return bail(fail(PMVS_ENOMEM, "pyramid staging"));
    }
    hipEvent_t piece_done[2];
    bool ev_ok = hipEventCreate(&piece_done[0]) == hipSuccess;
    ev_ok = hipEventCreate(&piece_done[1]) == hipSuccess && ev_ok;
    // double-buffered: piece k is copied into half k % 2 once that half's previous upload finished
    auto upload = [&](uint8_t* dst, const uint8_t* src, size_t bytes) -> hipError_t {
      if (!ev_ok) return hipErrorOutOfMemory;
      bool used[2] = {false, false};
      for (size_t off = 0, k = 0; off < bytes; off += kPin, ++k) {
        const int h = (int)(k & 1);
        const size_t m = bytes - off < kPin ? bytes - off : kPin;
        if (used[h]) {
          const hipError_t e = hipEventSynchronize(piece_done[h]);
          if (e != hipSuccess) return e;
        }
        std::memcpy(pin + h * kPin, src + off, m);
        hipError_t e = hipMemcpyAsync(dst + off, pin + h * kPin, m, hipMemcpyHostToDevice, sc->stream);
        if (e == hipSuccess) e = hipEventRecord(piece_done[h], sc->stream);
        if (e != hipSuccess) return e;
        used[h] = true;
      }
      return hipSuccess;
    };
    pmvs_status st = PMVS_OK;
    for (int i = 0; i < num && st == PMVS_OK; ++i) {
      const DView& v = sc->hviews[i];
      const size_t bytes0 = (size_t)v.w[0] * v.h[0] * 3;
      const char* step = "upload";
      int lv = 0;
      hipError_t e = upload(a, d->views[i].rgb, bytes0);
      if (e == hipSuccess && (step = "pack")) e = launch_pack_rgba(a, sc->pyr.p + v.pyr_off[0], (long long)v.w[0] * v.h[0], sc->stream);
      uint8_t* src = a;
      uint8_t* dst = b;
      for (int l = 1; l < maxLevel && e == hipSuccess; ++l) {
        lv = l;
        step = "downsample";
        e = launch_build_level(src, v.w[l - 1], v.h[l - 1], dst, v.w[l], v.h[l], sc->stream);
        if (e == hipSuccess && (step = "pack")) e = launch_pack_rgba(dst, sc->pyr.p + v.pyr_off[l], (long long)v.w[l] * v.h[l], sc->stream);
        std::swap(src, dst);
      }
      if (e == hipSuccess && (step = "sync")) e = hipStreamSynchronize(sc->stream);  // staging reused per view
      if (e != hipSuccess)
        st = fail(PMVS_EDEVICE, "pyramid build (view %d, level %d, %s): %s", i, lv, step, hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(sc->stream);
    (void)hipFree(a);
    (void)hipFree(b);
    (void)hipHostFree(pin);
    if (ev_ok) {
      (void)hipEventDestroy(piece_done[0]);
      (void)hipEventDestroy(piece_done[1]);
    }
    if (st != PMVS_OK) return bail(st);
  }

  // ---- optional masks / edges (binary pyramids built on the host)
  auto upload_binary = [&](bool any, bool isMask, DevBuf<uint8_t>& buf) -> pmvs_status {
    if (!any) return PMVS_OK;
    std::vector<uint8_t> all;
    for (int i = 0; i < num; ++i) {
      const pmvs_view_desc& vd = d->views[i];
      const uint8_t* m0 = isMask ? vd.mask : vd.edge;
      DView& v = sc->hviews[i];
      if (!m0) continue;
      std::vector<uint8_t> pyr[MAXL];
      pyr[0].resize((size_t)v.w[0] * v.h[0]);
      for (size_t k = 0; k < pyr[0].size(); ++k)
        pyr[0][k] = isMask ? ((127 < (int)m0[k]) ? 255 : 0) : ((1 < m0[k]) ? 255 : 0);  // image.cpp:159-180
      build_binary(pyr, v.w, v.h, maxLevel);
      if (isMask) sc->hmask_level[i] = pyr[d->level];
      for (int l = 0; l < maxLevel; ++l) {
        (isMask ? v.mask_off[l] : v.edge_off[l]) = (long long)all.size();
        all.insert(all.end(), pyr[l].begin(), pyr[l].end());
      }
    }
    if (buf.alloc(all.size()) != hipSuccess) return fail(PMVS_ENOMEM, "mask/edge upload");
    if (hipMemcpy(buf.p, all.data(), all.size(), hipMemcpyHostToDevice) != hipSuccess)
      return fail(PMVS_EDEVICE, "mask/edge copy");
    return PMVS_OK;
  };
  sc->hmask_level.assign(num, std::vector<uint8_t>());
  pmvs_status st = upload_binary(anyMask, true, sc->masks);
  if (st == PMVS_OK) st = upload_binary(anyEdge, false, sc->edges);
  if (st != PMVS_OK) return bail(st);

  // ---- tables
  std::vector<int> voff(d->visdata2_offsets, d->visdata2_offsets + num + 1);
  const int nvis = voff[num];
  sc->hvis_off = voff;
  sc->hvis.assign(d->visdata2, d->visdata2 + nvis);
  sc->sequence = d->sequence;
  for (int k = 0; k < nvis; ++k)
    if (d->visdata2[k] < 0 || d->visdata2[k] >= num) return bail(fail(PMVS_EINVAL, "visdata2[%d] = %d", k, d->visdata2[k]));
  for (int k = 0; k < d->num_bindexes; ++k)
    if (d->bindexes[k] < 0 || d->bindexes[k] >= num) return bail(fail(PMVS_EINVAL, "bindexes[%d]", k));
  if (sc->views.alloc(num) != hipSuccess || sc->vis_off.alloc(num + 1) != hipSuccess ||
      sc->vis.alloc(std::max(1, nvis)) != hipSuccess || sc->bindexes.alloc(std::max(1, d->num_bindexes)) != hipSuccess ||
      sc->stats.alloc(1) != hipSuccess)
    return bail(fail(PMVS_ENOMEM, "scene tables"));
  if (hipMemcpy(sc->views.p, sc->hviews.data(), num * sizeof(DView), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(sc->vis_off.p, voff.data(), (num + 1) * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      (nvis && hipMemcpy(sc->vis.p, d->visdata2, nvis * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) ||
      (d->num_bindexes && hipMemcpy(sc->bindexes.p, d->bindexes, d->num_bindexes * sizeof(int), hipMemcpyHostToDevice) != hipSuccess))
    return bail(fail(PMVS_EDEVICE, "scene table copy"));

  // ---- persistent grid: enough single-wave workgroups to fill every CU
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bail(fail(PMVS_EDEVICE, "device properties"));
  int gpc = 8;  // persistent single-wave workgroups per CU (pre/post, organizer and filter kernels)
  if (const char* e = getenv("PMVS_GRID_WAVES_PER_CU")) gpc = std::max(1, std::min(32, atoi(e)));
  sc->grid = std::max(1, prop.multiProcessorCount) * gpc;
  // tuning knobs (defaults measured on MI355X): refine wavefronts per CU and the
  // number of texture slots one cooperative objective chunk packs
  int wpc = 8;  // 1206: 19.5 KB LDS, <= 256 registers -> 8 resident per CU
  if (const char* e = getenv("PMVS_REFINE_WAVES_PER_CU")) wpc = std::max(1, std::min(32, atoi(e)));
  if (const char* e = getenv("PMVS_REFINE_CONFIG")) {  // one layout for every batch size
    if (!parse(atoi(e), sc->layout)) sc->layout = kWaveDefault;
    sc->layout_small = sc->layout;
  }
  if (const char* e = getenv("PMVS_REFINE_LARGE_CONFIG")) {  // the layout of the batches >= small_n only
    (void)parse(atoi(e), sc->layout);  // an unsupported number is ignored
  }
  if (const char* e = getenv("PMVS_REFINE_SMALL_CONFIG")) {  // the layout of the batches < small_n only
    (void)parse(atoi(e), sc->layout_small);
  }
  if (const char* e = getenv("PMVS_REFINE_SMALL_N")) sc->small_n = std::max(0, atoi(e));
  sc->refine_grid = std::max(1, prop.multiProcessorCount) * wpc;
  // per-workgroup global scratch: the scene grid, or pre / post's larger grid (prepost_waves)
  const size_t scratch_blocks = (size_t)sc->grid * std::max(2, prepost_waves()) / 2;
  if (sc->scratch.alloc(scratch_blocks * PMVS_MAX_IMAGES * PMVS_MAX_IMAGES) != hipSuccess)
    return bail(fail(PMVS_ENOMEM, "scratch"));

  DScene& s = sc->ds;
  s.views = sc->views.p;
  s.pyr = sc->pyr.p;
  s.masks = sc->masks.p;
  s.edges = sc->edges.p;
  s.vis_off = sc->vis_off.p;
  s.vis = sc->vis.p;
  s.bindexes = sc->bindexes.p;
  s.scratch = sc->scratch.p;
  s.nb = d->num_bindexes;
  s.num = num;
  s.tnum = d->num_targets;
  s.level = d->level;
  s.csize = d->csize;
  s.wsize = d->wsize;
  s.minImageNum = d->min_image_num;
  s.tau = tau;
  s.anyMask = anyMask ? 1 : 0;
  // CFindMatch::init thresholds (findMatch.cpp:92-106)
  s.nccThreshold = d->threshold;
  s.nccThresholdBefore = d->threshold - 0.3f;
  s.maxAngle = d->max_angle;
  const float angle0 = (float)(60.0f * M_PI / 180.0f);
  s.angle1 = (float)(60.0f * M_PI / 180.0f);
  s.athreshold = (float)std::cos((double)angle0);
  s.cosAngle1 = std::cos((double)s.angle1);
  s.sortThreshold = (float)(1.0f - std::cos(10.0 * M_PI / 180.0));
  s.ascale = (float)(M_PI / 48.0f);
  s.log2f = (float)std::log(2.0);
  s.quad = d->quad_threshold;
  s.depth = 0;
  if (hipStreamSynchronize(sc->stream) != hipSuccess) return bail(fail(PMVS_EDEVICE, "scene upload"));
  *out = sc;
  return PMVS_OK;
}

void pmvs_scene_destroy(pmvs_scene* scene) {
  if (!scene) return;
  (void)hipSetDevice(scene->device);
  (void)hipStreamSynchronize(scene->stream);
  delete scene;
}

pmvs_status pmvs_set_thresholds(pmvs_scene* sc, float ncc, float ncc_before, int32_t depth) {
  if (!sc) return fail(PMVS_EINVAL, "null scene");
  if (depth < 0) return fail(PMVS_EINVAL, "depth %d", depth);
  sc->ds.depth = depth;
  sc->ds.nccThreshold = ncc;
  sc->ds.nccThresholdBefore = ncc_before;
  return PMVS_OK;
}

pmvs_status pmvs_scene_get_level(pmvs_scene* sc, int32_t view, int32_t level, uint8_t* out, int32_t* width,
                                 int32_t* height) {
  if (!sc) return fail(PMVS_EINVAL, "null scene");
  if (view < 0 || view >= sc->ds.num || level < 0 || level >= sc->maxLevel) return fail(PMVS_EINVAL, "view/level");
  const DView& v = sc->hviews[view];
  if (width) *width = v.w[level];
  if (height) *height = v.h[level];
  if (!out) return PMVS_OK;
  HIPCHK(hipSetDevice(sc->device));
  const long long npix = (long long)v.w[level] * v.h[level];
  uint8_t* tmp = nullptr;
  HIPCHK(hipMalloc((void**)&tmp, npix * 3));
  hipError_t e = launch_unpack_rgba(sc->pyr.p + v.pyr_off[level], tmp, npix, sc->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, npix * 3, hipMemcpyDeviceToHost, sc->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(sc->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) return fail(PMVS_EDEVICE, "get_level: %s", hipGetErrorString(e));
  return PMVS_OK;
}

// ---- feature detection (CDetectFeatures::run, detectFeatures.cpp:47-124)
namespace {

// CDetector::setGaussI (detector.cpp:29-49): float weights, exp() of a float argument evaluated
// by the double C exp (unqualified exp(float) in that TU; probed), float normalisation.
FeatFilter gauss_i(float sigma) {
  FeatFilter f{};
  const int m = (int)std::ceil((double)(2 * sigma));
  f.n = 2 * m + 1;
  float denom = 0.0f;
  for (int x = 0; x < f.n; ++x) {
    const int xt = x - m;
    const float arg = (float)(-(xt * xt)) / (2 * sigma * sigma);
    const float d = (float)std::exp((double)arg);
    f.w[x] = d;
    denom += d;
  }
  for (int x = 0; x < f.n; ++x) f.w[x] /= denom;
  return f;
}

// The result multisets of one detector (harris.cpp:251-261 / dog.cpp:192-202) read from the
// largest element (detectFeatures.cpp:84-88, 103-107): blocks are inserted in raster order, each
// block's points in ascending order, so equal responses come out in reverse insertion order.
void order_points(const FeatPoint* pts, const int* cnt, int nb, int type, std::vector<pmvs_point>& out) {
  struct Item { float r; int64_t seq; float x, y; };
  std::vector<Item> v;
  int64_t seq = 0;
  for (int b = 0; b < nb; ++b)
    for (int k = 0; k < cnt[b]; ++k) {
      const FeatPoint& p = pts[4 * b + k];
      v.push_back({p.response, seq++, p.x, p.y});
    }
  std::sort(v.begin(), v.end(), [](const Item& a, const Item& b) {
    if (a.r != b.r) return a.r > b.r;
    return a.seq > b.seq;
  });
  for (const Item& it : v) out.push_back(pmvs_point{it.x, it.y, it.r, type});
}

}  // namespace

pmvs_status pmvs_detect_features(pmvs_scene* sc, int32_t view, int32_t fcsize, pmvs_point* out, int32_t cap,
                                 int32_t* n_out) {
  if (!sc || !n_out || (cap > 0 && !out)) return fail(PMVS_EINVAL, "null argument");
  if (view < 0 || view >= sc->ds.num) return fail(PMVS_EINVAL, "view %d", view);
  if (fcsize < 1) return fail(PMVS_EINVAL, "fcsize %d", fcsize);
  HIPCHK(hipSetDevice(sc->device));
  const int level = sc->ds.level;
  const DView& v = sc->hviews[view];
  FeatJob j{};
  j.W = v.w[level];
  j.H = v.h[level];
  j.pyr = sc->pyr.p + v.pyr_off[level];
  j.mask = v.mask_off[level] >= 0 ? sc->masks.p + v.mask_off[level] : nullptr;
  j.edge = v.edge_off[level] >= 0 ? sc->edges.p + v.edge_off[level] : nullptr;
  // CHarris::run: gridsize = gspeedup * 2 (harris.cpp:216-221), gspeedup = fcsize (16 in findMatch.cpp:81)
  j.gsize = fcsize * 2;
  j.bw = (j.W + j.gsize - 1) / j.gsize;
  j.bh = (j.H + j.gsize - 1) / j.gsize;
  const float sigma = 4.0f;  // detectFeatures.cpp:73
  j.harris_margin = ((2 * (int)std::ceil((double)(2 * sigma)) + 1)) / 2;  // (int)_gaussD.size() / 2
  j.dfilter.n = 3;
  j.dfilter.w[0] = -0.5f; j.dfilter.w[1] = 0.0f; j.dfilter.w[2] = 0.5f;  // harris.cpp:151
  j.ifilter.n = 3;
  j.ifilter.w[0] = j.ifilter.w[1] = j.ifilter.w[2] = (float)(1.0 / 3.0);  // harris.cpp:153
  j.gaussI = gauss_i(sigma);
  // CDifferenceOfGaussians::run (dog.cpp:130-160), firstScale 1, lastScale 3 (detectFeatures.cpp:75-76)
  const float first = 1.0f, last = 3.0f;
  const float step = (float)std::pow(2.0, 0.5);  // pow(2.0f, 1 / 2.0f): the double C pow
  const int steps = std::max(4, (int)std::ceil(std::log((double)(last / first)) / std::log((double)step)));
  if (steps != 4) return fail(PMVS_EUNSUPPORTED, "DoG with %d steps", steps);
  const float scales[5] = {first, first * step, first * step * step, (float)(first * std::pow((double)step, 3.0)),
                           (float)(first * std::pow((double)step, 4.0))};
  for (int k = 0; k < 5; ++k) j.dog_gauss[k] = gauss_i(scales[k]);
  for (int k = 0; k < 2; ++k) j.dog_margin[k] = (int)std::ceil((double)(2 * scales[3 + k]));
  for (const FeatFilter* f : {&j.gaussI, &j.dog_gauss[4]})
    if (f->n > 32) return fail(PMVS_EUNSUPPORTED, "filter with %d taps", f->n);
  HIPCHK(detect_features(j, sc->feat, sc->stream));
  const int nb = j.bw * j.bh;
  std::vector<FeatPoint> pts((size_t)nb * 8);
  std::vector<int> cnt((size_t)nb * 2);
  HIPCHK(hipMemcpyAsync(pts.data(), sc->feat.pts, pts.size() * sizeof(FeatPoint), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipMemcpyAsync(cnt.data(), sc->feat.cnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipStreamSynchronize(sc->stream));
  std::vector<pmvs_point> all;
  order_points(pts.data(), cnt.data(), nb, 0, all);
  order_points(pts.data() + 4 * (size_t)nb, cnt.data() + nb, nb, 1, all);
  *n_out = (int32_t)all.size();
  if (out) std::memcpy(out, all.data(), std::min<size_t>(all.size(), (size_t)std::max(cap, 0)) * sizeof(pmvs_point));
  return PMVS_OK;
}

pmvs_status pmvs_seed_run(pmvs_scene* sc, const pmvs_point* points, const int32_t* num_points, int32_t batch,
                          pmvs_patch* out, int32_t cap, int32_t* n_out, pmvs_seed_stats* stats) {
  if (!sc || !num_points || !n_out || cap < 0 || (cap > 0 && !out)) return fail(PMVS_EINVAL, "null argument");
  const bool keep = !out && cap == 0;  // the scene keeps the seeds; pmvs_seed_fetch copies them out
  sc->seeds_kept = false;
  std::vector<pmvs_patch>().swap(sc->skept);
  if (sc->ds.depth != 0) return fail(PMVS_EINVAL, "the seed phase runs at depth 0 (scene depth %d)", sc->ds.depth);
  long long np = 0;
  for (int i = 0; i < sc->ds.num; ++i) {
    if (num_points[i] < 0) return fail(PMVS_EINVAL, "num_points[%d] = %d", i, num_points[i]);
    np += num_points[i];
  }
  if (np > 0 && !points) return fail(PMVS_EINVAL, "null points");
  for (long long k = 0; k < np; ++k)
    if (!(points[k].x >= 0.0f && points[k].y >= 0.0f)) return fail(PMVS_EINVAL, "point %lld outside the image", k);
  *n_out = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  HIPCHK(hipSetDevice(sc->device));
  SeedInput in;
  in.points = points;
  in.npts = num_points;
  in.vis_off = sc->hvis_off.data();
  in.vis = sc->hvis.data();
  in.sequence = sc->sequence;
  in.angle0 = (float)(60.0f * M_PI / 180.0f);  // findMatch.cpp:92
  for (int i = 0; i < sc->ds.num; ++i) in.mask_level.push_back(sc->hmask_level[i].empty() ? nullptr : sc->hmask_level[i].data());
  in.batch = batch > 0 ? batch : 16384;
  in.per_cell = 4;
  if (const char* e = getenv("PMVS_SEED_PER_CELL")) in.per_cell = std::max(1, atoi(e));
  in.lookahead = 1;  // speculation into the next images: measured no fewer rounds
  if (const char* e = getenv("PMVS_SEED_LOOKAHEAD")) in.lookahead = std::max(1, atoi(e));
  in.spec_near = 2048;
  if (const char* e = getenv("PMVS_SEED_NEAR")) in.spec_near = std::max(1, atoi(e));
  HIPCHK(hipMemsetAsync(sc->stats.p, 0, sizeof(DevStats), sc->stream));
  sc->rhost.prof = false;
  RefineFn refine = [&](const pmvs_candidate* d_in, int m, pmvs_refined* d_out) -> hipError_t {
    if (ensure(sc->jobs, m)) return hipErrorOutOfMemory;
    hipError_t e = hipMemsetAsync(&sc->stats.p->queue, 0, 3 * sizeof(unsigned long long), sc->stream);
    if (e != hipSuccess) return e;
    return launch_refine(sc->ds, d_in, sc->jobs.p, d_out, m, sc->stats.p, sc->grid, sc->refine_grid, sc->refine_cfg(m),
                         sc->stream, sc->kev, sc->rhost);
  };
  SeedOutput so;
  const hipError_t e = seed_pass(sc->ds, sc->hviews, in, sc->stream, refine, so);
  if (e == hipErrorOutOfMemory) return fail(PMVS_ENOMEM, "seed phase: device memory");
  if (e == hipErrorNotSupported)
    return fail(PMVS_EUNSUPPORTED, "seed phase: a candidate's image list exceeds %d entries", PMVS_MAX_IMAGES);
  HIPCHK(e);
  sc->last_refine = false;
  const int ns = (int)so.seeds.size();
  *n_out = ns;
  if (stats) {
    stats->trial = so.stats[0]; stats->pass = so.stats[1]; stats->fail0 = so.stats[2]; stats->fail1 = so.stats[3];
    stats->refined = so.stats[4]; stats->rounds = so.stats[5]; stats->candidates = so.stats[6];
    stats->wall_ms = so.wall_ms; stats->gen_ms = so.gen_ms; stats->refine_ms = so.refine_ms;
  }
  if (keep) {
    sc->skept.swap(so.seeds);
    sc->seeds_kept = true;
    return PMVS_OK;
  }
  if (ns > cap) return fail(PMVS_EINVAL, "seed phase: %d seeds, capacity %d", ns, cap);
  if (ns) std::memcpy(out, so.seeds.data(), (size_t)ns * sizeof(pmvs_patch));
  return PMVS_OK;
}

pmvs_status pmvs_seed_fetch(pmvs_scene* sc, pmvs_patch* out, int32_t n) {
  if (!sc || n < 0 || (n > 0 && !out)) return fail(PMVS_EINVAL, "invalid argument");
  if (!sc->seeds_kept || (size_t)n != sc->skept.size())
    return fail(PMVS_EINVAL, "seed_fetch: %d seeds kept, %d asked", sc->seeds_kept ? (int)sc->skept.size() : -1, n);
  if (n) std::memcpy(out, sc->skept.data(), (size_t)n * sizeof(pmvs_patch));
  sc->seeds_kept = false;
  std::vector<pmvs_patch>().swap(sc->skept);
  return PMVS_OK;
}

pmvs_status pmvs_grab_tex(pmvs_scene* sc, const pmvs_tex_query* q, int32_t n, float* out_tex, int32_t* out_valid) {
  if (!sc || (n > 0 && (!q || !out_tex || !out_valid))) return fail(PMVS_EINVAL, "null argument");
  if (n <= 0) return PMVS_OK;
  for (int i = 0; i < n; ++i)
    if (q[i].view < 0 || q[i].view >= sc->ds.num) return fail(PMVS_EINVAL, "query %d: view %d", i, q[i].view);
  HIPCHK(hipSetDevice(sc->device));
  const int len = 3 * sc->ds.wsize * sc->ds.wsize;
  pmvs_status st;
  if ((st = ensure(sc->tq, n)) || (st = ensure(sc->tout, (size_t)n * len)) || (st = ensure(sc->tvalid, n))) return st;
  HIPCHK(hipMemcpyAsync(sc->tq.p, q, n * sizeof(pmvs_tex_query), hipMemcpyHostToDevice, sc->stream));
  HIPCHK(launch_grab_tex(sc->ds, sc->tq.p, n, sc->tout.p, sc->tvalid.p, sc->stream));
  HIPCHK(hipMemcpyAsync(out_tex, sc->tout.p, (size_t)n * len * sizeof(float), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipMemcpyAsync(out_valid, sc->tvalid.p, n * sizeof(int), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipStreamSynchronize(sc->stream));
  return PMVS_OK;
}

static void fill_stats(const DevStats& d, int64_t n, float ms, pmvs_stats* st) {
  if (!st) return;
  st->candidates = n;
  st->accepted = (int64_t)d.accepted;
  st->fail_pre = (int64_t)d.fail_pre;
  st->fail_post = (int64_t)d.fail_post;
  st->refine_failed = (int64_t)d.refine_failed;
  st->evals = (int64_t)d.evals;
  st->tex_valid = (int64_t)d.tex_valid;
  st->tex_grabs = (int64_t)d.tex_grabs;
  st->kernel_ms = ms;
  st->opt_cycles = (int64_t)d.cyc_opt;
  st->objective_cycles = (int64_t)d.cyc_eval;
  st->rounds = (int64_t)d.rounds;
  st->chunks = (int64_t)d.chunks;
  for (int i = 0; i < 8; ++i) st->prof[i] = (int64_t)d.prof[i];
}

pmvs_status pmvs_incc_eval(pmvs_scene* sc, const pmvs_eval_query* q, int32_t n, double* out_f, pmvs_stats* stats) {
  if (!sc || (n > 0 && (!q || !out_f))) return fail(PMVS_EINVAL, "null argument");
  if (n <= 0) return PMVS_OK;
  for (int i = 0; i < n; ++i) {
    if (q[i].num_images < 1 || q[i].num_images > PMVS_MAX_TAU) return fail(PMVS_EINVAL, "query %d: num_images", i);
    for (int k = 0; k < q[i].num_images; ++k)
      if (q[i].images[k] < 0 || q[i].images[k] >= sc->ds.num) return fail(PMVS_EINVAL, "query %d: image", i);
  }
  HIPCHK(hipSetDevice(sc->device));
  pmvs_status st;
  if ((st = ensure(sc->evq, n)) || (st = ensure(sc->evout, n))) return st;
  HIPCHK(hipMemcpyAsync(sc->evq.p, q, n * sizeof(pmvs_eval_query), hipMemcpyHostToDevice, sc->stream));
  HIPCHK(hipMemsetAsync(sc->stats.p, 0, sizeof(DevStats), sc->stream));
  HIPCHK(hipEventRecord(sc->ev0, sc->stream));
  HIPCHK(launch_incc_eval(sc->ds, sc->evq.p, n, sc->evout.p, sc->stats.p, sc->stream));
  HIPCHK(hipEventRecord(sc->ev1, sc->stream));
  HIPCHK(hipMemcpyAsync(out_f, sc->evout.p, n * sizeof(double), hipMemcpyDeviceToHost, sc->stream));
  DevStats ds{};
  HIPCHK(hipMemcpyAsync(&ds, sc->stats.p, sizeof(DevStats), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipStreamSynchronize(sc->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, sc->ev0, sc->ev1));
  fill_stats(ds, n, ms, stats);
  return PMVS_OK;
}

static pmvs_status check_candidates(const pmvs_scene* sc, const pmvs_candidate* in, int n) {
  for (int i = 0; i < n; ++i) {
    if (in[i].num_images < 1 || in[i].num_images > PMVS_MAX_IMAGES) return fail(PMVS_EINVAL, "candidate %d: num_images %d", i, in[i].num_images);
    for (int k = 0; k < in[i].num_images; ++k)
      if (in[i].images[k] < 0 || in[i].images[k] >= sc->ds.num) return fail(PMVS_EINVAL, "candidate %d: image %d", i, in[i].images[k]);
  }
  return PMVS_OK;
}

pmvs_status pmvs_refine_batch_device(pmvs_scene* sc, const pmvs_candidate* d_in, int32_t n, pmvs_refined* d_out) {
  if (!sc || (n > 0 && (!d_in || !d_out))) return fail(PMVS_EINVAL, "null argument");
  if (sc->ds.depth != 0)
    return fail(PMVS_EUNSUPPORTED, "refine at depth %d: the depth >= 1 postProcess steps (setVImagesVGrids, check) "
                "are not part of pmvs_refine_batch in this release", sc->ds.depth);
  if (n <= 0) return PMVS_OK;
  HIPCHK(hipSetDevice(sc->device));
  pmvs_status st;
  if ((st = ensure(sc->jobs, n))) return st;
  HIPCHK(hipMemsetAsync(sc->stats.p, 0, sizeof(DevStats), sc->stream));
  HIPCHK(hipEventRecord(sc->ev0, sc->stream));
  HIPCHK(launch_refine(sc->ds, d_in, sc->jobs.p, d_out, n, sc->stats.p, sc->grid, sc->refine_grid, sc->refine_cfg(n), sc->stream,
                       sc->kev, sc->rhost));
  HIPCHK(hipEventRecord(sc->ev1, sc->stream));
  sc->last_refine = true;
  return PMVS_OK;
}

pmvs_status pmvs_scene_sync(pmvs_scene* sc, pmvs_stats* stats) {
  if (!sc) return fail(PMVS_EINVAL, "null scene");
  HIPCHK(hipSetDevice(sc->device));
  DevStats ds{};
  HIPCHK(hipMemcpyAsync(&ds, sc->stats.p, sizeof(DevStats), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipStreamSynchronize(sc->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, sc->ev0, sc->ev1) != hipSuccess) ms = 0;
  fill_stats(ds, (int64_t)(ds.queue > 0 ? ds.queue : 0), ms, stats);
  if (stats && sc->last_refine) {
    float a = 0, b = 0, c = 0;
    if (hipEventElapsedTime(&a, sc->kev[0], sc->kev[1]) == hipSuccess) stats->pre_ms = a;
    if (hipEventElapsedTime(&b, sc->kev[1], sc->kev[2]) == hipSuccess) stats->refine_ms = b;
    if (hipEventElapsedTime(&c, sc->kev[2], sc->kev[3]) == hipSuccess) stats->post_ms = c;
  }
  if (stats) {
    // queue overshoots by one dequeue per workgroup: the candidate count is recorded by the caller
    stats->candidates = (int64_t)(ds.accepted + ds.fail_pre + ds.fail_post);
  }
  return PMVS_OK;
}

pmvs_status pmvs_refine_batch(pmvs_scene* sc, const pmvs_candidate* in, int32_t n, pmvs_refined* out,
                              pmvs_stats* stats) {
  if (!sc || (n > 0 && (!in || !out))) return fail(PMVS_EINVAL, "null argument");
  if (n <= 0) {
    if (stats) std::memset(stats, 0, sizeof(*stats));
    return PMVS_OK;
  }
  pmvs_status st = check_candidates(sc, in, n);
  if (st) return st;
  HIPCHK(hipSetDevice(sc->device));
  if ((st = ensure(sc->cand, n)) || (st = ensure(sc->res, n))) return st;
  HIPCHK(hipMemcpyAsync(sc->cand.p, in, n * sizeof(pmvs_candidate), hipMemcpyHostToDevice, sc->stream));
  if ((st = pmvs_refine_batch_device(sc, sc->cand.p, n, sc->res.p))) return st;
  HIPCHK(hipMemcpyAsync(out, sc->res.p, n * sizeof(pmvs_refined), hipMemcpyDeviceToHost, sc->stream));
  return pmvs_scene_sync(sc, stats);
}

pmvs_status pmvs_selftest_math(int32_t device, int32_t op, const double* in, double* out, int32_t n) {
  if (!in || !out || n <= 0) return fail(PMVS_EINVAL, "null argument");
  HIPCHK(hipSetDevice(device));
  double *di = nullptr, *dout = nullptr;
  HIPCHK(hipMalloc((void**)&di, n * sizeof(double)));
  hipError_t e = hipMalloc((void**)&dout, n * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(di, in, n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_math_selftest(op, di, dout, n, nullptr);
  if (e == hipSuccess) e = hipMemcpy(out, dout, n * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(di);
  if (dout) (void)hipFree(dout);
  if (e != hipSuccess) return fail(PMVS_EDEVICE, "math selftest: %s", hipGetErrorString(e));
  return PMVS_OK;
}

pmvs_status pmvs_selftest_lls(int32_t device, const float* A, const float* b, const int32_t* offsets, int32_t nsys,
                              float* x) {
  if (!A || !b || !offsets || !x || nsys <= 0) return fail(PMVS_EINVAL, "null argument");
  for (int k = 0; k < nsys; ++k)
    if (offsets[k + 1] - offsets[k] < 5) return fail(PMVS_EINVAL, "system %d has fewer than 5 rows", k);
  HIPCHK(hipSetDevice(device));
  HIPCHK(lls_selftest(A, b, offsets, nsys, offsets[nsys], x));
  return PMVS_OK;
}

pmvs_status pmvs_selftest_bobyqa(int32_t device, int32_t mode, int32_t kind, const double* x0, int32_t n,
                                 int32_t maxeval, double* out, double* ms) {
  if (!x0 || !out || n <= 0) return fail(PMVS_EINVAL, "null argument");
  HIPCHK(hipSetDevice(device));
  double *dx = nullptr, *dout = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(hipMalloc((void**)&dx, 3 * n * sizeof(double)));
  hipError_t e = hipMalloc((void**)&dout, 6 * n * sizeof(double));
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  if (e == hipSuccess) e = hipMemcpy(dx, x0, 3 * n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
  if (e == hipSuccess) e = launch_bobyqa_selftest(mode, kind, dx, n, maxeval, dout, nullptr);
  if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
  if (e == hipSuccess) e = hipMemcpy(out, dout, 6 * n * sizeof(double), hipMemcpyDeviceToHost);
  float t = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
  if (ms) *ms = t;
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(dx);
  if (dout) (void)hipFree(dout);
  if (e != hipSuccess) return fail(PMVS_EDEVICE, "bobyqa selftest: %s", hipGetErrorString(e));
  return PMVS_OK;
}

}  // extern "C"

pmvs_status pmvs_patch_colors(pmvs_scene* sc, int32_t n, const float* coords4, const int32_t* nimg,
                              const int32_t* images_flat, int32_t* colors_out) {
  if (!sc || n < 0 || (n > 0 && (!coords4 || !nimg || !images_flat || !colors_out))) return fail(PMVS_EINVAL, "null argument");
  if (n == 0) return PMVS_OK;
  std::vector<int> off(n + 1, 0);
  for (int i = 0; i < n; ++i) {
    if (nimg[i] < 1) return fail(PMVS_EINVAL, "patch %d: no images", i);
    off[i + 1] = off[i] + nimg[i];
  }
  for (int k = 0; k < off[n]; ++k)
    if (images_flat[k] < 0 || images_flat[k] >= sc->ds.num) return fail(PMVS_EINVAL, "image index %d", images_flat[k]);
  HIPCHK(hipSetDevice(sc->device));
  float* dc = nullptr;
  int *doff = nullptr, *dimg = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc((void**)&dc, (size_t)n * 4 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&doff, (size_t)(n + 1) * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&dimg, (size_t)off[n] * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&dout, (size_t)n * 3 * sizeof(int));
  if (e == hipSuccess) e = hipMemcpyAsync(dc, coords4, (size_t)n * 4 * sizeof(float), hipMemcpyHostToDevice, sc->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(doff, off.data(), (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice, sc->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dimg, images_flat, (size_t)off[n] * sizeof(int), hipMemcpyHostToDevice, sc->stream);
  if (e == hipSuccess) e = launch_patch_colors(sc->ds, n, dc, doff, dimg, dout, sc->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(colors_out, dout, (size_t)n * 3 * sizeof(int), hipMemcpyDeviceToHost, sc->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(sc->stream);
  (void)hipFree(dc);
  (void)hipFree(doff);
  (void)hipFree(dimg);
  (void)hipFree(dout);
  if (e != hipSuccess) return fail(PMVS_EDEVICE, "patch colours: %s", hipGetErrorString(e));
  return PMVS_OK;
}

pmvs_status pmvs_filter_run(pmvs_scene* sc, pmvs_patch* patches, int32_t n, int32_t* keep, pmvs_filter_stats* stats) {
  if (!sc || n < 0 || (n > 0 && (!patches || !keep))) return fail(PMVS_EINVAL, "null argument");
  if (sc->ds.tnum > PMVS_MAX_TARGETS) return fail(PMVS_EUNSUPPORTED, "filter pass: more than %d target images", PMVS_MAX_TARGETS);
  for (int i = 0; i < n; ++i) {
    const pmvs_patch& p = patches[i];
    if (p.num_images < 1 || p.num_images > PMVS_MAX_IMAGES || p.num_vimages < 0 || p.num_vimages > PMVS_MAX_IMAGES)
      return fail(PMVS_EINVAL, "patch %d: image counts", i);
    for (int k = 0; k < p.num_images; ++k)
      if (p.images[k] < 0 || p.images[k] >= sc->ds.num) return fail(PMVS_EINVAL, "patch %d: image %d", i, p.images[k]);
    for (int k = 0; k < p.num_vimages; ++k)
      if (p.vimages[k] < 0 || p.vimages[k] >= sc->ds.tnum) return fail(PMVS_EINVAL, "patch %d: vimage", i);
  }
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return PMVS_OK;
  HIPCHK(hipSetDevice(sc->device));
  pmvs_status st;
  if ((st = ensure(sc->fpatches, n)) || (st = ensure(sc->fkeep, n))) return st;
  std::vector<long long> tgoff(sc->ds.tnum + 1, 0);
  for (int t = 0; t < sc->ds.tnum; ++t) {
    const DView& v = sc->hviews[t];
    const long long gw = (v.w[sc->ds.level] + sc->ds.csize - 1) / sc->ds.csize;
    const long long gh = (v.h[sc->ds.level] + sc->ds.csize - 1) / sc->ds.csize;
    tgoff[t + 1] = tgoff[t] + gw * gh;
  }
  HIPCHK(hipMemcpyAsync(sc->fpatches.p, patches, (size_t)n * sizeof(pmvs_patch), hipMemcpyHostToDevice, sc->stream));
  HIPCHK(hipEventRecord(sc->ev0, sc->stream));
  int counts[4], overflow = 0;
  const hipError_t fe = filter_pass(sc->ds, sc->fbuf, sc->fpatches.p, n, tgoff[sc->ds.tnum], tgoff.data(), sc->grid,
                                    sc->stream, counts, &overflow, sc->fkeep.p);
  if (fe == hipErrorNotSupported)
    return fail(PMVS_EUNSUPPORTED, "filter pass: a patch is visible in more than %d target images", PMVS_MAX_IMAGES);
  HIPCHK(fe);
  HIPCHK(hipEventRecord(sc->ev1, sc->stream));
  HIPCHK(hipMemcpyAsync(patches, sc->fpatches.p, (size_t)n * sizeof(pmvs_patch), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipMemcpyAsync(keep, sc->fkeep.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipStreamSynchronize(sc->stream));
  if (overflow) return fail(PMVS_EUNSUPPORTED, "filterNeighbor: %d patches with more than 16384 neighbours", overflow);
  if (stats) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, sc->ev0, sc->ev1);
    stats->input = n;
    stats->removed_outside = counts[0];
    stats->removed_exact = counts[1];
    stats->removed_neighbor = counts[2];
    stats->removed_groups = counts[3];
    int64_t k = 0;
    for (int i = 0; i < n; ++i) k += keep[i];
    stats->kept = k;
    stats->kernel_ms = ms;
  }
  sc->last_refine = false;
  return PMVS_OK;
}

namespace {

// validation of a caller's patch set (image counts and indexes)
pmvs_status check_patches(const pmvs_scene* sc, const pmvs_patch* patches, int n) {
  for (int i = 0; i < n; ++i) {
    const pmvs_patch& p = patches[i];
    if (p.num_images < 1 || p.num_images > PMVS_MAX_IMAGES || p.num_vimages < 0 || p.num_vimages > PMVS_MAX_IMAGES)
      return fail(PMVS_EINVAL, "patch %d: image counts", i);
    for (int k = 0; k < p.num_images; ++k)
      if (p.images[k] < 0 || p.images[k] >= sc->ds.num) return fail(PMVS_EINVAL, "patch %d: image %d", i, p.images[k]);
    for (int k = 0; k < p.num_vimages; ++k)
      if (p.vimages[k] < 0 || p.vimages[k] >= sc->ds.tnum) return fail(PMVS_EINVAL, "patch %d: vimage", i);
  }
  return PMVS_OK;
}

// The scene's shard (pmvs_scene_set_shard / _rccl) as the organizer code takes it.
Shard make_shard(const pmvs_scene* sc) {
  Shard sh;
  if (sc->shard_fn && sc->shard_world > 1) {
    sh.rank = sc->shard_rank;
    sh.world = sc->shard_world;
    pmvs_allgather_fn fn = sc->shard_fn;
    void* ctx = sc->shard_ctx;
    sh.exchange = [fn, ctx](const void* send, size_t bytes, void* recv) { return fn(ctx, send, (int64_t)bytes, recv); };
    if (pmvs_rccl* comm = sc->shard_rccl)
      sh.exchange_dev = [comm](const void* dsend, size_t bytes, void* drecv, hipStream_t st) {
        return pmvs_rccl_allgather_device(comm, dsend, (int64_t)bytes, drecv, st);
      };
  }
  return sh;
}

// The scene's cluster exchange channel (pmvs_scene_set_cluster / _rccl).
Shard make_cluster_shard(const pmvs_scene* sc) {
  Shard sh;
  if (sc->cl_fn && sc->cl_world > 1) {
    sh.rank = sc->cl_rank;
    sh.world = sc->cl_world;
    pmvs_allgather_fn fn = sc->cl_fn;
    void* ctx = sc->cl_ctx;
    sh.exchange = [fn, ctx](const void* send, size_t bytes, void* recv) { return fn(ctx, send, (int64_t)bytes, recv); };
    if (pmvs_rccl* comm = sc->cl_rccl)
      sh.exchange_dev = [comm](const void* dsend, size_t bytes, void* drecv, hipStream_t st) {
        return pmvs_rccl_allgather_device(comm, dsend, (int64_t)bytes, drecv, st);
      };
  }
  return sh;
}

// Loop-level 8-byte header {error, 0} of the sharded loop: a rank that fails outside the
// expansion's / filter's own exchanges sends it once (its peers receive it in place of their next
// expansion batch header), and every rank sends {0} when the loop ends.  Returns 0 = every rank
// OK, 1 = some rank failed, -1 = the exchange itself failed.
int loop_header(const Shard& sh, int err) {
  int h[2] = {err, 0};
  std::vector<int> all(2 * (size_t)sh.world, 0);
  if (sh.exchange(h, sizeof(h), all.data()) != 0) return -1;
  for (int r = 0; r < sh.world; ++r)
    if (all[2 * r] != 0) return 1;
  return 0;
}

std::vector<long long> target_cells(pmvs_scene* sc) {
  std::vector<long long> tgoff(sc->ds.tnum + 1, 0);
  sc->xbuf.gw.assign(sc->ds.tnum, 0);
  sc->xbuf.gh.assign(sc->ds.tnum, 0);
  for (int t = 0; t < sc->ds.tnum; ++t) {
    const DView& v = sc->hviews[t];
    sc->xbuf.gw[t] = (v.w[sc->ds.level] + sc->ds.csize - 1) / sc->ds.csize;
    sc->xbuf.gh[t] = (v.h[sc->ds.level] + sc->ds.csize - 1) / sc->ds.csize;
    tgoff[t + 1] = tgoff[t] + (long long)sc->xbuf.gw[t] * sc->xbuf.gh[t];
  }
  return tgoff;
}

// One expansion run on the device-resident model sc->fpatches[0, n0) with alive flags
// sc->xbuf.alive; *n_out patches afterwards.
// Test hook (tests/test_gpu_expand.py): PMVS_TEST_SHARD_FAIL="rank:0:x" (after the expansion's last
// exchange) or "rank:0:s" (after the filter pass's last exchange) makes that rank fail locally there,
// as an asynchronous kernel fault surfacing at the stream synchronisation would.
bool test_local_fail(const pmvs_scene* sc, char where) {
  const char* e = getenv("PMVS_TEST_SHARD_FAIL");
  int r = -1, w = -1;
  char c = 0;
  if (!e || sscanf(e, "%d:%d:%c", &r, &w, &c) != 3 || c != where) return false;
  return (sc->shard_world > 1 && r == sc->shard_rank) || (sc->cl_world > 1 && r == sc->cl_rank);
}

// *handled (sharded loop): whether the peers already know of a failure returned here -- true only
// for failures expand_pass reported through its own header exchanges.
pmvs_status expand_device(pmvs_scene* sc, int n0, int wave, int min_cands, int cthr, int flags, int cap, int* n_out,
                          pmvs_expand_stats* stats, bool* handled = nullptr) {
  if (handled) *handled = false;
  const std::vector<long long> tgoff = target_cells(sc);
  // refine-work accounting: device counters accumulate over the run (only the work-queue heads
  // are reset per launch); the refine-kernel time of each launch is read at the next one, when
  // the host has synchronised in between.
  double refine_ms = 0.0, refine_ms_small = 0.0;
  int64_t refined = 0, launches = 0, launches_small = 0;
  bool pending = false, pending_small = false;
  auto take_time = [&]() {
    if (!pending) return;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, sc->kev[1], sc->kev[2]) == hipSuccess) {
      refine_ms += ms;
      if (pending_small) refine_ms_small += ms;
    }
    pending = false;
  };
  HIPCHK(hipMemsetAsync(sc->stats.p, 0, sizeof(DevStats), sc->stream));
  sc->rhost.prof = getenv("PMVS_EXPAND_PROFILE") != nullptr;
  sc->rhost.trip_ms = 0.0;
  sc->rhost.trips = 0;
  RefineFn refine = [&](const pmvs_candidate* d_in, int m, pmvs_refined* d_out) -> hipError_t {
    if (ensure(sc->jobs, m)) return hipErrorOutOfMemory;
    take_time();
    hipError_t e = hipMemsetAsync(&sc->stats.p->queue, 0, 3 * sizeof(unsigned long long), sc->stream);
    if (e != hipSuccess) return e;
    refined += m;
    ++launches;
    pending = true;
    const RefineLayout& cfg = sc->refine_cfg(m);
    pending_small = m < sc->small_n;  // the small batches (refine_cfg: layout_small)
    launches_small += pending_small ? 1 : 0;
    return launch_refine(sc->ds, d_in, sc->jobs.p, d_out, m, sc->stats.p, sc->grid, sc->refine_grid, cfg, sc->stream,
                         sc->kev, sc->rhost);
  };
  const Shard sh = make_shard(sc);
  long long sv[8];
  const auto t0 = std::chrono::steady_clock::now();
  const hipError_t e = expand_pass(sc->ds, sc->fbuf, sc->xbuf, sc->fpatches.p, sc->fpatches.cap, n0, sc->xbuf.alive, cap,
                                   tgoff[sc->ds.tnum], tgoff.data(), wave, cthr, flags, sc->grid, sc->stream, refine, sh,
                                   sv, n_out, min_cands);
  if (handled) *handled = e != hipSuccess;  // expand_pass ends every failure with a header all ranks see
  if (e == kCapacityOverflow)
    return fail(PMVS_EUNSUPPORTED,
                "expansion: capacity %d exceeded, a patch has more than 16384 neighbours, or a patch's image / "
                "visible-target list exceeds %d entries", cap, PMVS_MAX_IMAGES);
  if (e == hipErrorOutOfMemory) return fail(PMVS_ENOMEM, "expansion: device memory");
  if (e == hipErrorUnknown && sh.world > 1) return fail(PMVS_EDEVICE, "expansion: the shard exchange or another rank failed");
  HIPCHK(e);
  if (handled) *handled = false;  // from here on a failure is this rank's alone
  if (test_local_fail(sc, 'x')) return fail(PMVS_EDEVICE, "expansion: injected local failure (test)");
  HIPCHK(hipStreamSynchronize(sc->stream));
  take_time();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  DevStats ds{};
  HIPCHK(hipMemcpy(&ds, sc->stats.p, sizeof(DevStats), hipMemcpyDeviceToHost));
  if (sc->rhost.prof)
    fprintf(stderr, "[refine round trip] batches=%lld device_ms=%.1f (pre_kernel end -> refine start: start points "
                    "down, host libm asin/acos, angles up)\n", sc->rhost.trips, sc->rhost.trip_ms);
  if (getenv("PMVS_REFINE_TAIL"))  // diagnostics: the refine launches' tails (s_memrealtime: 100 MHz)
    for (int f = 0; f < 2; ++f)
      if (ds.tail_launches[f])
        fprintf(stderr, "[refine tail] form=%s launches=%llu span_ms=%.2f tail_ms=%.2f tail_frac=%.3f\n",
                f ? "workgroup" : "wavefront", ds.tail_launches[f], ds.span_t[f] / 1e5, ds.tail_t[f] / 1e5,
                ds.span_t[f] ? (double)ds.tail_t[f] / (double)ds.span_t[f] : 0.0);
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->parents = sv[0]; stats->candidates = sv[1]; stats->fail_prep = sv[2]; stats->fail_pre = sv[3];
    stats->fail_post = sv[4]; stats->fail_commit = sv[5]; stats->added = sv[6]; stats->waves = sv[7];
    stats->wall_ms = ms;
    stats->refined = refined;
    stats->evals = (int64_t)ds.evals;
    stats->tex_valid = (int64_t)ds.tex_valid;
    stats->refine_ms = refine_ms;
    stats->refine_launches = launches;
    stats->tex_valid_small = (int64_t)ds.tex_valid_wg;
    stats->refine_ms_small = refine_ms_small;
    stats->refine_launches_small = launches_small;
  }
  sc->last_refine = false;
  return PMVS_OK;
}

// One filter pass on the device-resident model sc->fpatches[0, n); keep flags in sc->fkeep.
// *handled (sharded loop): whether the peers already know of a failure returned here.
pmvs_status filter_device(pmvs_scene* sc, int n, pmvs_filter_stats* stats, bool* handled = nullptr) {
  if (handled) *handled = false;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (n == 0) return PMVS_OK;
  pmvs_status st;
  if ((st = ensure(sc->fkeep, n))) return st;
  std::vector<long long> tgoff = target_cells(sc);
  HIPCHK(hipEventRecord(sc->ev0, sc->stream));
  int counts[4], overflow = 0;
  const Shard sh = make_shard(sc);
  bool fh = true;
  const hipError_t fe = filter_pass(sc->ds, sc->fbuf, sc->fpatches.p, n, tgoff[sc->ds.tnum], tgoff.data(), sc->grid,
                                    sc->stream, counts, &overflow, sc->fkeep.p, &sh, &fh);
  if (fe != hipSuccess) {
    if (handled) *handled = fh;
    if (fe == hipErrorNotSupported)
      return fail(PMVS_EUNSUPPORTED, "filter pass: a patch is visible in more than %d target images", PMVS_MAX_IMAGES);
    return fail(PMVS_EDEVICE, "filter pass: %s", hipGetErrorString(fe));
  }
  // kernels launched after the pass's last exchange (small groups, collect, keep) fault only at
  // this synchronisation, on this rank alone: *handled stays false so the loop announces it
  HIPCHK(hipEventRecord(sc->ev1, sc->stream));
  if (test_local_fail(sc, 's')) return fail(PMVS_EDEVICE, "filter pass: injected local failure (test)");
  HIPCHK(hipStreamSynchronize(sc->stream));
  if (handled) *handled = true;  // overflow is all-gathered: every rank returns it together
  if (overflow) return fail(PMVS_EUNSUPPORTED, "filterNeighbor: %d patches with more than 16384 neighbours", overflow);
  if (stats) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, sc->ev0, sc->ev1);
    stats->input = n;
    stats->removed_outside = counts[0];
    stats->removed_exact = counts[1];
    stats->removed_neighbor = counts[2];
    stats->removed_groups = counts[3];
    stats->kept = n - counts[0] - counts[1] - counts[2] - counts[3];
    stats->kernel_ms = ms;
  }
  sc->last_refine = false;
  return PMVS_OK;
}

}  // namespace

pmvs_status pmvs_expand_run(pmvs_scene* sc, const pmvs_patch* patches, const int32_t* alive, int32_t n, int32_t wave,
                            int32_t min_candidates, int32_t count_threshold, int32_t flags, pmvs_patch* out, int32_t* alive_out, int32_t cap,
                            int32_t* n_out, pmvs_expand_stats* stats) {
  const bool keep = !out && !alive_out;
  if (!sc || n < 0 || (n > 0 && (!patches || !alive)) || (!keep && (!out || !alive_out)) || !n_out || cap < n)
    return fail(PMVS_EINVAL, "invalid argument");
  if (wave < 1 || wave > kMaxWave) return fail(PMVS_EINVAL, "wave must be in [1, %d]", kMaxWave);
  if (sc->ds.tnum > PMVS_MAX_TARGETS) return fail(PMVS_EUNSUPPORTED, "expansion: more than %d target images", PMVS_MAX_TARGETS);
  pmvs_status st;
  if ((st = check_patches(sc, patches, n))) return st;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  *n_out = 0;
  sc->xkept = keep ? 0 : -1;
  sc->xalive.clear();
  if (n == 0) return PMVS_OK;
  HIPCHK(hipSetDevice(sc->device));
  if ((st = ensure(sc->fpatches, n))) return st;
  if (grow_alive(sc, n)) return fail(PMVS_ENOMEM, "alive flags");
  HIPCHK(hipMemcpyAsync(sc->fpatches.p, patches, (size_t)n * sizeof(pmvs_patch), hipMemcpyHostToDevice, sc->stream));
  HIPCHK(hipMemcpyAsync(sc->xbuf.alive, alive, (size_t)n * sizeof(int), hipMemcpyHostToDevice, sc->stream));
  int nn = 0;
  if (min_candidates < 0) return fail(PMVS_EINVAL, "min_candidates %d", min_candidates);
  if ((st = expand_device(sc, n, wave, min_candidates, count_threshold, flags, cap, &nn, stats))) return st;
  *n_out = nn;
  std::vector<int> al(alive, alive + n);
  al.resize(nn, 1);
  if (keep) {
    sc->xkept = nn;
    sc->xalive.swap(al);
    return PMVS_OK;
  }
  HIPCHK(hipMemcpy(out, sc->fpatches.p, (size_t)nn * sizeof(pmvs_patch), hipMemcpyDeviceToHost));
  std::memcpy(alive_out, al.data(), (size_t)nn * sizeof(int));
  return PMVS_OK;
}

pmvs_status pmvs_expand_fetch(pmvs_scene* sc, pmvs_patch* out, int32_t* alive_out, int32_t n) {
  if (!sc || n < 0 || (n > 0 && (!out || !alive_out))) return fail(PMVS_EINVAL, "invalid argument");
  if (n != sc->xkept) return fail(PMVS_EINVAL, "expand_fetch: %d patches kept, %d asked", sc->xkept, n);
  if (n) {
    HIPCHK(hipSetDevice(sc->device));
    HIPCHK(hipMemcpy(out, sc->fpatches.p, (size_t)n * sizeof(pmvs_patch), hipMemcpyDeviceToHost));
    if (alive_out) std::memcpy(alive_out, sc->xalive.data(), (size_t)n * sizeof(int));
  }
  sc->xkept = -1;
  std::vector<int>().swap(sc->xalive);
  return PMVS_OK;
}

pmvs_status pmvs_run_loop(pmvs_scene* sc, const pmvs_patch* seeds, int32_t n, float threshold, int32_t iterations,
                          int32_t wave, int32_t min_candidates, int32_t flags, int32_t cap, int32_t* n_out, pmvs_loop_iter* iters) {
  if (!sc || n < 0 || (n > 0 && !seeds) || !n_out || iterations < 0 || cap < n || min_candidates < 0)
    return fail(PMVS_EINVAL, "invalid argument");
  if (wave < 1 || wave > kMaxWave) return fail(PMVS_EINVAL, "wave must be in [1, %d]", kMaxWave);
  if (sc->ds.tnum > PMVS_MAX_TARGETS) return fail(PMVS_EUNSUPPORTED, "expansion: more than %d target images", PMVS_MAX_TARGETS);
  pmvs_status st;
  if ((st = check_patches(sc, seeds, n))) return st;
  *n_out = 0;
  sc->lkept = -1;
  if (iters) std::memset(iters, 0, sizeof(pmvs_loop_iter) * (size_t)iterations);
  HIPCHK(hipSetDevice(sc->device));
  if ((st = ensure(sc->fpatches, std::max(n, 1)))) return st;
  if (n) HIPCHK(hipMemcpyAsync(sc->fpatches.p, seeds, (size_t)n * sizeof(pmvs_patch), hipMemcpyHostToDevice, sc->stream));
  // CFindMatch::run after the seed phase (findMatch.cpp:196-217); updateThreshold in float
  // (findMatch.cpp:23-28): before = threshold - 0.3f (findMatch.cpp:104)
  float ncc = threshold, before = threshold - 0.3f;
  int cthr = 4, depth = 1, cur = n;
  // Sharded: a failure the peers have not seen is announced with one loop header (loop_header).
  const Shard lsh = make_shard(sc);
  const Shard csh = make_cluster_shard(sc);  // cluster boundary exchange (pmvs_scene_set_cluster)
  if (lsh.world > 1 && csh.world > 1) return fail(PMVS_EINVAL, "a scene is either sharded or a cluster, not both");
  const Shard& hsh = (csh.world > 1) ? csh : lsh;  // the channel of the loop's error headers
  auto fail_loop = [&](pmvs_status s0, bool peers_know) {
    if (hsh.world > 1 && !peers_know) (void)loop_header(hsh, 1);
    return s0;
  };
  // Compaction targets (fpatches2) are sized by the kept records: the source's capacity (the
  // expansion's, up to twice its model) would hold two full-size models at once -- at C5 scale
  // (50 M patches of 1608 B after one expansion) more than the GPU has.  The source buffer is
  // released after the swap when it is much larger than the model.
  bool dst_oom = false;
  auto dst_for = [&](int k, pmvs_patch** d) -> hipError_t {
    if (sc->fpatches2.cap > 2 * (size_t)std::max(k, 1)) sc->fpatches2.release();
    if (ensure(sc->fpatches2, std::max(k, 1))) {
      dst_oom = true;
      return hipErrorOutOfMemory;
    }
    *d = sc->fpatches2.p;
    return hipSuccess;
  };
  auto swap_models = [&](int kept) {
    std::swap(sc->fpatches, sc->fpatches2);
    if (sc->fpatches2.cap > 2 * (size_t)std::max(kept, 1)) sc->fpatches2.release();
  };
  // the model without foreign patches, compacted through fpatches2
  auto drop = [&](int n, int* kept) -> pmvs_status {
    if (n == 0) { *kept = 0; return PMVS_OK; }
    if (drop_foreign(sc->fbuf, sc->fpatches.p, n, dst_for, kept, sc->stream) != hipSuccess)
      return dst_oom ? fail(PMVS_ENOMEM, "model (%d patches)", *kept) : fail(PMVS_EDEVICE, "foreign patches");
    swap_models(*kept);
    return PMVS_OK;
  };
  for (int it = 0; it < iterations; ++it) {
    sc->ds.depth = depth;
    sc->ds.nccThreshold = ncc;
    sc->ds.nccThresholdBefore = before;
    if (grow_alive(sc, std::max(cur, 1))) return fail_loop(fail(PMVS_ENOMEM, "alive flags"), false);
    if (fill_int(sc->xbuf.alive, cur, 1, sc->stream) != hipSuccess) return fail_loop(fail(PMVS_EDEVICE, "alive flags"), false);
    pmvs_loop_iter li{};
    li.depth = depth;
    int nn = cur;
    // expand_device / filter_device report failures their own exchanges announced (*handled); those
    // exchanges run on the shard channel, so in a cluster scene (loop headers on the cluster
    // channel) no peer has seen them and the loop header must carry them
    bool xhandled = true;
    const int xflags = (flags & ~PMVS_EXPAND_AFTER_SEEDS) | ((it == 0 && (flags & PMVS_EXPAND_AFTER_SEEDS)) ? 1 : 0);
    if (cur > 0 && (st = expand_device(sc, cur, wave, min_candidates, cthr, xflags, cap, &nn, &li.expand, &xhandled)))
      return fail_loop(st, xhandled && &hsh == &lsh);
    bool handled = true;
    if ((st = filter_device(sc, nn, &li.filter, &handled))) return fail_loop(st, handled && &hsh == &lsh);
    int kept = 0;
    if (nn > 0) {
      if (compact_model(sc->fbuf, sc->fpatches.p, nn, sc->fkeep.p, dst_for, &kept, sc->stream) != hipSuccess)
        return fail_loop(dst_oom ? fail(PMVS_ENOMEM, "model (%d patches)", kept) : fail(PMVS_EDEVICE, "model compaction"),
                         false);
      swap_models(kept);
    }
    cur = kept;
    li.patches = kept;
    if (csh.world > 1 && it + 1 < iterations) {  // cluster boundary exchange before the next iteration
      int own = 0;
      if ((st = drop(cur, &own))) return fail_loop(st, false);
      li.patches = own;
      // PMVS_LOOP_LEAN=1: the pass buffers go back to the device while this rank waits for its peers
      // (several 8K clusters sharing one GPU, tests/test_gpu_c5_exchange.py); the next pass reserves
      // them again
      if (getenv("PMVS_LOOP_LEAN")) {
        if (hipStreamSynchronize(sc->stream) != hipSuccess) return fail_loop(fail(PMVS_EDEVICE, "loop synchronisation"), false);
        sc->fbuf.release();
        sc->xbuf.release();
      }
      const ClusterMaps cm{sc->cl_shared.p, sc->cl_ids.p, sc->cl_id2idx.p, sc->cl_maxid};
      long long xs[3] = {0, 0, 0};
      bool agreed = false;
      int nn2 = own;
      const hipError_t xe = cluster_exchange(sc->ds, sc->cbuf, cm, sc->fpatches.p, own, sc->fpatches.p, sc->fpatches.cap, &nn2,
                                             csh, sc->stream, xs, agreed);
      if (xe != hipSuccess) return fail_loop(fail(PMVS_EDEVICE, "cluster exchange: %s", hipGetErrorString(xe)), agreed);
      cur = nn2;
      li.boundary_sent = xs[0];
      li.boundary_received = xs[1];
      li.boundary_inserted = xs[2];
    }
    if (iters) iters[it] = li;
    ncc -= 0.05f;
    before -= 0.05f;
    cthr = 2;
    ++depth;
  }
  if (csh.world > 1) {  // the cluster's own patches only
    int own = 0;
    if ((st = drop(cur, &own))) return fail_loop(st, false);
    cur = own;
  }
  if (hipStreamSynchronize(sc->stream) != hipSuccess) return fail_loop(fail(PMVS_EDEVICE, "loop synchronisation"), false);
  if (hsh.world > 1 && loop_header(hsh, 0) != 0) return fail(PMVS_EDEVICE, "sharded loop: another rank failed");
  *n_out = cur;
  sc->lkept = cur;
  return PMVS_OK;
}

pmvs_status pmvs_loop_fetch(pmvs_scene* sc, pmvs_patch* out, int32_t n) {
  if (!sc || n < 0 || (n > 0 && !out)) return fail(PMVS_EINVAL, "invalid argument");
  if (n != sc->lkept) return fail(PMVS_EINVAL, "loop_fetch: %d patches kept, %d asked", sc->lkept, n);
  if (n) {
    HIPCHK(hipSetDevice(sc->device));
    HIPCHK(hipMemcpy(out, sc->fpatches.p, (size_t)n * sizeof(pmvs_patch), hipMemcpyDeviceToHost));
  }
  sc->lkept = -1;
  return PMVS_OK;
}

pmvs_status pmvs_loop_hash(pmvs_scene* sc, uint64_t* hash) {
  if (!sc || !hash) return fail(PMVS_EINVAL, "invalid argument");
  if (sc->lkept < 0) return fail(PMVS_EINVAL, "loop_hash: no loop result on the device");
  HIPCHK(hipSetDevice(sc->device));
  if (ensure(sc->digest, 1)) return fail(PMVS_ENOMEM, "digest");
  HIPCHK(hipMemsetAsync(sc->digest.p, 0, sizeof(unsigned long long), sc->stream));
  static_assert(sizeof(pmvs_patch) % 4 == 0, "record words");
  HIPCHK(launch_model_digest(sc->fpatches.p, sc->lkept, (int)sizeof(pmvs_patch), sc->digest.p, sc->stream));
  unsigned long long h = 0;
  HIPCHK(hipMemcpyAsync(&h, sc->digest.p, sizeof(h), hipMemcpyDeviceToHost, sc->stream));
  HIPCHK(hipStreamSynchronize(sc->stream));
  *hash = h ^ (unsigned long long)sc->lkept;
  return PMVS_OK;
}

// ---- the model-output calls: what every stage below shares
namespace {
static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "output array types");

pmvs_status export_status(hipError_t e, const char* what) {
  if (e == hipErrorOutOfMemory) return fail(PMVS_ENOMEM, "%s: %s", what, hipGetErrorString(e));
  return fail(PMVS_EDEVICE, "%s: %s", what, hipGetErrorString(e));
}
#define EXPCHK(expr)                                         \
  do {                                                       \
    const hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) return export_status(e_, #expr);   \
  } while (0)

bool flags_ok(int32_t flags, int32_t allowed = PMVS_EXPORT_WRITER_ORDER | PMVS_EXPORT_DEVICE) { return !(flags & ~allowed); }
bool records_ok(const pmvs_patch* patches, int32_t n) { return n >= 0 && (n == 0 || patches); }

// Target t's cell grid and the maps' cell offsets (tnum + 1 entries); returns the widest grid.
int depth_map_layout(const pmvs_scene* sc, int32_t* dims, int64_t* offsets) {
  int64_t off = 0;
  int max_gwidth = 1;
  for (int t = 0; t < sc->ds.tnum; ++t) {
    const int gw = (sc->hviews[t].w[sc->ds.level] + sc->ds.csize - 1) / sc->ds.csize;
    const int gh = (sc->hviews[t].h[sc->ds.level] + sc->ds.csize - 1) / sc->ds.csize;
    if (dims) { dims[2 * t] = gw; dims[2 * t + 1] = gh; }
    if (offsets) offsets[t] = off;
    off += (int64_t)gw * gh;
    max_gwidth = std::max(max_gwidth, gw);
  }
  if (offsets) offsets[sc->ds.tnum] = off;
  return max_gwidth;
}

pmvs_status check_export_patches(const pmvs_scene* sc, const pmvs_patch* patches, int32_t n, pmvs_export_sizes* sizes) {
  long long ni = 0, nv = 0;
  for (int i = 0; i < n; ++i) {
    const pmvs_patch& p = patches[i];
    if (p.num_images < 1 || p.num_images > PMVS_MAX_IMAGES || p.num_vimages < 0 || p.num_vimages > PMVS_MAX_IMAGES)
      return fail(PMVS_EINVAL, "patch %d: image counts", i);
    for (int k = 0; k < p.num_images; ++k)
      if (p.images[k] < 0 || p.images[k] >= sc->ds.num) return fail(PMVS_EINVAL, "patch %d: image %d", i, p.images[k]);
    for (int k = 0; k < p.num_vimages; ++k)
      if (p.vimages[k] < 0 || p.vimages[k] >= sc->ds.tnum) return fail(PMVS_EINVAL, "patch %d: vimage", i);
    ni += p.num_images;
    nv += p.num_vimages;
  }
  if (sizes) *sizes = pmvs_export_sizes{n, 0, ni, nv};
  return PMVS_OK;
}

// The records of a loop_* call: the loop result where it lies (`call` names the entry point in the message).
pmvs_status loop_records(pmvs_scene* sc, const char* call, const pmvs_patch** dP, int32_t* n) {
  if (sc->lkept < 0) return fail(PMVS_EINVAL, "%s: no loop result on the device", call);
  HIPCHK(hipSetDevice(sc->device));
  *dP = sc->fpatches.p;
  *n = sc->lkept;
  return PMVS_OK;
}

// The records of a *_patches call: validated (sizes = their totals, or null) and uploaded into a buffer of
// the call's own (sc->fpatches may hold a loop result).
pmvs_status upload_records(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, pmvs_export_sizes* sizes, CallArena& arena,
                           const pmvs_patch** dP) {
  *dP = nullptr;
  if (pmvs_status st = check_export_patches(sc, patches, n, sizes)) return st;
  HIPCHK(hipSetDevice(sc->device));
  if (n) {
    pmvs_patch* up = nullptr;
    EXPCHK(arena.alloc(&up, (size_t)n));
    EXPCHK(hipMemcpyAsync(up, patches, (size_t)n * sizeof(pmvs_patch), hipMemcpyHostToDevice, sc->stream));
    *dP = up;
  }
  return PMVS_OK;
}

// Row r of a writer-ordered call is record d_src[r]: the export's order, from the export's code.  Null in
// model order and without records.
pmvs_status writer_order_source(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, CallArena& arena, int** d_src) {
  *d_src = nullptr;
  if ((flags & PMVS_EXPORT_WRITER_ORDER) && n > 0) {
    EXPCHK(arena.alloc(d_src, (size_t)n));
    EXPCHK(export_order(sc->ds, dP, n, depth_map_layout(sc, nullptr, nullptr), *d_src, nullptr, nullptr, sc->stream));
  }
  return PMVS_OK;
}

// index2image on the device, or null (identity).
pmvs_status upload_index2image(pmvs_scene* sc, const int32_t* index2image, CallArena& arena, int** d_tab) {
  *d_tab = nullptr;
  if (index2image) {
    EXPCHK(arena.alloc(d_tab, (size_t)sc->ds.num));
    EXPCHK(hipMemcpyAsync(*d_tab, index2image, (size_t)sc->ds.num * sizeof(int), hipMemcpyHostToDevice, sc->stream));
  }
  return PMVS_OK;
}
}  // namespace

// ---- model export (pmvs_export.hip)
namespace {
pmvs_status device_export_sizes(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, pmvs_export_sizes* sizes) {
  CallArena arena;
  unsigned long long* d_tot = nullptr;
  unsigned long long tot[2] = {0, 0};
  EXPCHK(arena.alloc(&d_tot, 2));
  EXPCHK(export_sizes(dP, n, d_tot, sc->stream));
  EXPCHK(hipMemcpyAsync(tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, sc->stream));
  EXPCHK(hipStreamSynchronize(sc->stream));
  *sizes = pmvs_export_sizes{n, 0, (int64_t)tot[0], (int64_t)tot[1]};
  return PMVS_OK;
}

// The export of the device records dP[0, n); sz = their totals.
pmvs_status export_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, const pmvs_export_sizes& sz, int32_t flags,
                           const int32_t* index2image, const pmvs_export_buffers* b) {
  const bool dev = (flags & PMVS_EXPORT_DEVICE) != 0;
  if (n == 0) {  // offsets {0}
    int64_t* const offs[2] = {b->image_off, b->vimage_off};
    for (int64_t* off : offs) {
      if (off && dev) EXPCHK(hipMemsetAsync(off, 0, sizeof(int64_t), sc->stream));
      if (off && !dev) *off = 0;
    }
    if (dev) EXPCHK(hipStreamSynchronize(sc->stream));
    return PMVS_OK;
  }
  CallArena arena;
  Staging stg(arena, dev);
  int* d_tab = nullptr;
  if (pmvs_status st = upload_index2image(sc, index2image, arena, &d_tab)) return st;
  const size_t np = (size_t)n, ne = (size_t)sz.image_entries, nve = (size_t)sz.vimage_entries;
  ExportArrays a;
  EXPCHK(stg.fixed(&a.fields, b->fields, np * 11));
  EXPCHK(stg.fixed(&a.colors, b->colors, np * 3));
  EXPCHK(stg.fixed(&a.image_off, b->image_off, np + 1));
  EXPCHK(stg.fixed(&a.image_ids, b->image_ids, ne));
  EXPCHK(stg.fixed(&a.image_idx, b->image_idx, ne));
  EXPCHK(stg.fixed(&a.vimage_off, b->vimage_off, np + 1));
  EXPCHK(stg.fixed(&a.vimage_ids, b->vimage_ids, nve));
  EXPCHK(stg.fixed(&a.source, b->source, np));
  EXPCHK(export_pass(sc->ds, dP, n, (flags & PMVS_EXPORT_WRITER_ORDER) != 0, depth_map_layout(sc, nullptr, nullptr), d_tab, a,
                     sc->stream));
  EXPCHK(stg.finish(sc->stream));
  return PMVS_OK;
}
}  // namespace

pmvs_status pmvs_loop_export_sizes(pmvs_scene* sc, pmvs_export_sizes* sizes) {
  if (!sc || !sizes) return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_export_sizes", &dP, &n)) return st;
  return device_export_sizes(sc, dP, n, sizes);
}

pmvs_status pmvs_loop_export(pmvs_scene* sc, int32_t flags, const int32_t* index2image, const pmvs_export_buffers* buffers) {
  if (!sc || !buffers || !flags_ok(flags)) return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_export", &dP, &n)) return st;
  pmvs_export_sizes sz{};
  if (pmvs_status st = device_export_sizes(sc, dP, n, &sz)) return st;
  return export_records(sc, dP, n, sz, flags, index2image, buffers);
}

pmvs_status pmvs_export_patches_sizes(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, pmvs_export_sizes* sizes) {
  if (!sc || !sizes || !records_ok(patches, n)) return fail(PMVS_EINVAL, "invalid argument");
  return check_export_patches(sc, patches, n, sizes);
}

pmvs_status pmvs_export_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t flags,
                                const int32_t* index2image, const pmvs_export_buffers* buffers) {
  if (!sc || !buffers || !records_ok(patches, n) || !flags_ok(flags)) return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  pmvs_export_sizes sz{};
  if (pmvs_status st = upload_records(sc, patches, n, &sz, arena, &dP)) return st;
  return export_records(sc, dP, n, sz, flags, index2image, buffers);
}

// ---- per-target depth maps (pmvs_depthmap.hip)
namespace {
bool wants_maps(const pmvs_depthmap_buffers* b) { return b->patch || b->depth || b->normal || b->ncc; }

// The four maps of `elems` cells or pixels each (the normals three floats per element).
hipError_t stage_maps(Staging& stg, const pmvs_depthmap_buffers* b, size_t elems, DepthMapArrays* a) {
  hipError_t e = stg.fixed(&a->patch, b->patch, elems);
  if (e == hipSuccess) e = stg.fixed(&a->depth, b->depth, elems);
  if (e == hipSuccess) e = stg.fixed(&a->normal, b->normal, elems * 3);
  if (e == hipSuccess) e = stg.fixed(&a->ncc, b->ncc, elems);
  return e;
}

// The depth maps of the device records dP[0, n).
pmvs_status depth_maps_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, const pmvs_depthmap_buffers* b) {
  if (!wants_maps(b)) return PMVS_OK;
  std::vector<int64_t> off((size_t)sc->ds.tnum + 1);
  depth_map_layout(sc, nullptr, off.data());
  const size_t cells = (size_t)off.back();
  CallArena arena;
  Staging stg(arena, (flags & PMVS_EXPORT_DEVICE) != 0);
  long long* d_off = nullptr;
  int* d_src = nullptr;
  EXPCHK(arena.alloc(&d_off, off.size()));
  EXPCHK(hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, sc->stream));
  if (pmvs_status st = writer_order_source(sc, dP, n, flags, arena, &d_src)) return st;
  DepthMapArrays a;
  EXPCHK(stage_maps(stg, b, cells, &a));
  EXPCHK(depth_map_pass(sc->ds, dP, n, d_src, d_off, (long long)cells, a, sc->stream));
  EXPCHK(stg.finish(sc->stream));
  return PMVS_OK;
}
}  // namespace

pmvs_status pmvs_depth_map_layout(pmvs_scene* sc, int32_t* dims, int64_t* offsets) {
  if (!sc) return fail(PMVS_EINVAL, "invalid argument");
  depth_map_layout(sc, dims, offsets);
  return PMVS_OK;
}

pmvs_status pmvs_loop_depth_maps(pmvs_scene* sc, int32_t flags, const pmvs_depthmap_buffers* buffers) {
  if (!sc || !buffers || !flags_ok(flags)) return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_depth_maps", &dP, &n)) return st;
  return depth_maps_records(sc, dP, n, flags, buffers);
}

pmvs_status pmvs_depth_maps_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t flags,
                                    const pmvs_depthmap_buffers* buffers) {
  if (!sc || !buffers || !records_ok(patches, n) || !flags_ok(flags)) return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  if (pmvs_status st = upload_records(sc, patches, n, nullptr, arena, &dP)) return st;
  return depth_maps_records(sc, dP, n, flags, buffers);
}

// ---- per-pixel maps (pmvs_pixmap.hip)
namespace {
bool target_range_ok(const pmvs_scene* sc, int32_t first, int32_t num) {
  return first >= 0 && num > 0 && (int64_t)first + num <= sc->ds.tnum;
}
bool radius_ok(int32_t radius) { return radius >= 0 && radius <= PMVS_PIXEL_MAX_RADIUS; }
// What every call over a target range checks of the scene.  The validators below look at the scene last: a
// call with a null argument fails before the handle is touched (the *_abi tests pass a handle that is not one).
bool range_call_ok(const pmvs_scene* sc, int32_t flags, int32_t first, int32_t num) {
  return sc && flags_ok(flags) && target_range_ok(sc, first, num);
}

// The images of targets [first, first + num) at the scene's level and their pixel offsets; returns the total.
int64_t pixel_map_layout(const pmvs_scene* sc, int32_t first, int32_t num, int32_t* dims, int64_t* offsets) {
  int64_t off = 0;
  for (int j = 0; j < num; ++j) {
    const DView& v = sc->hviews[first + j];
    if (dims) { dims[2 * j] = v.w[sc->ds.level]; dims[2 * j + 1] = v.h[sc->ds.level]; }
    if (offsets) offsets[j] = off;
    off += (int64_t)v.w[sc->ds.level] * v.h[sc->ds.level];
  }
  if (offsets) offsets[num] = off;
  return off;
}

// The pixel maps of the device records dP[0, n).
pmvs_status pixel_maps_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, int32_t first, int32_t num,
                               int32_t radius, const pmvs_depthmap_buffers* b) {
  if (!wants_maps(b)) return PMVS_OK;
  const size_t pixels = (size_t)pixel_map_layout(sc, first, num, nullptr, nullptr);
  CallArena arena;
  Staging stg(arena, (flags & PMVS_EXPORT_DEVICE) != 0);
  int* d_src = nullptr;
  if (pmvs_status st = writer_order_source(sc, dP, n, flags, arena, &d_src)) return st;
  DepthMapArrays a;
  EXPCHK(stage_maps(stg, b, pixels, &a));
  EXPCHK(pixel_map_pass(sc->ds, sc->hviews.data(), dP, n, d_src, first, num, radius, a, sc->stream));
  EXPCHK(stg.finish(sc->stream));
  return PMVS_OK;
}

bool pixel_args_ok(const pmvs_scene* sc, int32_t flags, int32_t first, int32_t num, int32_t radius,
                   const pmvs_depthmap_buffers* b) {
  return b && radius_ok(radius) && range_call_ok(sc, flags, first, num);
}
}  // namespace

pmvs_status pmvs_pixel_map_layout(pmvs_scene* sc, int32_t first_target, int32_t num_targets, int32_t* dims, int64_t* offsets) {
  if (!sc || !target_range_ok(sc, first_target, num_targets)) return fail(PMVS_EINVAL, "invalid argument");
  pixel_map_layout(sc, first_target, num_targets, dims, offsets);
  return PMVS_OK;
}

pmvs_status pmvs_loop_pixel_maps(pmvs_scene* sc, int32_t flags, int32_t first_target, int32_t num_targets, int32_t radius,
                                 const pmvs_depthmap_buffers* buffers) {
  if (!pixel_args_ok(sc, flags, first_target, num_targets, radius, buffers)) return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_pixel_maps", &dP, &n)) return st;
  return pixel_maps_records(sc, dP, n, flags, first_target, num_targets, radius, buffers);
}

pmvs_status pmvs_pixel_maps_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t flags, int32_t first_target,
                                    int32_t num_targets, int32_t radius, const pmvs_depthmap_buffers* buffers) {
  if (!pixel_args_ok(sc, flags, first_target, num_targets, radius, buffers) || !records_ok(patches, n))
    return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  if (pmvs_status st = upload_records(sc, patches, n, nullptr, arena, &dP)) return st;
  return pixel_maps_records(sc, dP, n, flags, first_target, num_targets, radius, buffers);
}

// ---- fusion of the per-pixel maps (pmvs_fuse.hip)
namespace {
bool fuse_params_ok(const pmvs_fuse_params* p) {
  return p && radius_ok(p->radius) && p->min_support >= 0 && p->min_support <= 255 && std::isfinite(p->depth_rel) &&
         p->depth_rel >= 0.0f && !std::isnan(p->normal_cos);
}
bool fuse_args_ok(const pmvs_scene* sc, int32_t flags, int32_t first, int32_t num, const pmvs_fuse_params* p, int64_t cap,
                  const pmvs_fuse_buffers* b, const int64_t* count) {
  return b && count && cap >= 0 && fuse_params_ok(p) && range_call_ok(sc, flags, first, num);
}

enum { kPoints = 1, kVertices = 1, kFaces = 2 };  // Staging parts: the capped arrays that share a written count

// The fusion of the device records dP[0, n).
pmvs_status fuse_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, int32_t first, int32_t num,
                         const pmvs_fuse_params* prm, int64_t cap, const pmvs_fuse_buffers* b, int64_t* count) {
  const size_t pixels = (size_t)pixel_map_layout(sc, first, num, nullptr, nullptr);
  CallArena arena;
  Staging stg(arena, (flags & PMVS_EXPORT_DEVICE) != 0);
  int* d_src = nullptr;
  if (pmvs_status st = writer_order_source(sc, dP, n, flags, arena, &d_src)) return st;
  // no more points than pixels can be emitted: the staging is sized by that, whatever the caller's cap
  const size_t pts = (size_t)std::min<int64_t>(cap, (int64_t)pixels);
  FuseArrays a;
  EXPCHK(stg.fixed(&a.support_map, b->support_map, pixels));
  EXPCHK(stg.capped(&a.coord, b->coord, pts, 3, kPoints));
  EXPCHK(stg.capped(&a.normal, b->normal, pts, 3, kPoints));
  EXPCHK(stg.capped(&a.color, b->color, pts, 3, kPoints));
  EXPCHK(stg.capped(&a.support, b->support, pts, 1, kPoints));
  EXPCHK(stg.capped(&a.pixel, b->pixel, pts, 1, kPoints));
  EXPCHK(stg.capped(&a.patch, b->patch, pts, 1, kPoints));
  long long total = 0;
  EXPCHK(fuse_pass(sc->ds, sc->hviews.data(), dP, n, d_src, first, num, *prm, (long long)pts, a, &total, sc->stream));
  *count = total;
  stg.wrote(kPoints, (size_t)total);
  EXPCHK(stg.finish(sc->stream));
  return PMVS_OK;
}
}  // namespace

pmvs_status pmvs_loop_fuse(pmvs_scene* sc, int32_t flags, int32_t first_target, int32_t num_targets,
                           const pmvs_fuse_params* params, int64_t cap, const pmvs_fuse_buffers* buffers, int64_t* count) {
  if (!fuse_args_ok(sc, flags, first_target, num_targets, params, cap, buffers, count)) return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_fuse", &dP, &n)) return st;
  return fuse_records(sc, dP, n, flags, first_target, num_targets, params, cap, buffers, count);
}

pmvs_status pmvs_fuse_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t flags, int32_t first_target,
                              int32_t num_targets, const pmvs_fuse_params* params, int64_t cap, const pmvs_fuse_buffers* buffers,
                              int64_t* count) {
  if (!fuse_args_ok(sc, flags, first_target, num_targets, params, cap, buffers, count) || !records_ok(patches, n))
    return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  if (pmvs_status st = upload_records(sc, patches, n, nullptr, arena, &dP)) return st;
  return fuse_records(sc, dP, n, flags, first_target, num_targets, params, cap, buffers, count);
}

// ---- meshing of the fused maps (pmvs_mesh.hip)
namespace {
bool volume_ok(const pmvs_volume* v) {
  if (!v || !std::isfinite(v->origin[0]) || !std::isfinite(v->origin[1]) || !std::isfinite(v->origin[2])) return false;
  if (!std::isfinite(v->voxel) || !(v->voxel > 0.0f)) return false;
  if (v->dims[0] < 1 || v->dims[1] < 1 || v->dims[2] < 1) return false;
  return (int64_t)v->dims[0] * v->dims[1] <= INT32_MAX && (int64_t)v->dims[0] * v->dims[1] * v->dims[2] <= INT32_MAX;
}

bool tsdf_params_ok(const pmvs_tsdf_params* p) {
  return p && fuse_params_ok(&p->fuse) && std::isfinite(p->trunc) && p->trunc > 0.0f;
}

bool tsdf_args_ok(const pmvs_scene* sc, int32_t flags, int32_t first, int32_t num, const pmvs_tsdf_params* p,
                  const pmvs_volume* v) {
  return tsdf_params_ok(p) && volume_ok(v) && range_call_ok(sc, flags, first, num);
}

bool mesh_args_ok(int32_t min_obs, int64_t vcap, int64_t fcap, const pmvs_mesh_buffers* b, const int64_t* nverts,
                  const int64_t* nfaces) {
  return b && nverts && nfaces && min_obs >= 1 && min_obs <= 255 && vcap >= 0 && fcap >= 0;
}

size_t volume_voxels(const pmvs_volume& v) { return (size_t)v.dims[0] * v.dims[1] * v.dims[2]; }

// The fusion's maps and pass flags of the device records dP[0, n) into `f`, enqueued on the scene's stream.
pmvs_status tsdf_maps(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, int32_t first, int32_t num,
                      const pmvs_fuse_params& prm, CallArena& arena, FuseMaps& f) {
  int* d_src = nullptr;
  if (pmvs_status st = writer_order_source(sc, dP, n, flags, arena, &d_src)) return st;
  EXPCHK(fuse_maps_pass(sc->ds, sc->hviews.data(), dP, n, d_src, first, num, prm, nullptr, f, sc->stream));
  return PMVS_OK;
}

// The TSDF of the device records dP[0, n).
pmvs_status tsdf_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, int32_t first, int32_t num,
                         const pmvs_tsdf_params* prm, const pmvs_volume* vol, const pmvs_tsdf_buffers* b) {
  if (!b->tsdf && !b->obs && !b->color) return PMVS_OK;
  const size_t voxels = volume_voxels(*vol);
  CallArena arena;
  Staging stg(arena, (flags & PMVS_EXPORT_DEVICE) != 0);
  FuseMaps f;
  TsdfArrays a;
  EXPCHK(stg.fixed(&a.tsdf, b->tsdf, voxels));
  EXPCHK(stg.fixed(&a.obs, b->obs, voxels));
  EXPCHK(stg.fixed(&a.color, b->color, voxels * 4));
  if (pmvs_status st = tsdf_maps(sc, dP, n, flags, first, num, prm->fuse, arena, f)) return st;
  EXPCHK(tsdf_integrate(sc->ds, f, first, num, *vol, prm->trunc, a, sc->stream));
  EXPCHK(stg.finish(sc->stream, true));  // in device mode too: the maps are freed on return
  return PMVS_OK;
}

// Surface nets over device volume arrays into the caller's buffers (device mode) or through staging.
pmvs_status mesh_device_volume(pmvs_scene* sc, bool dev, const pmvs_volume* vol, int32_t min_obs, const float* d_tsdf,
                               const uint8_t* d_obs, const uint8_t* d_color, int64_t vcap, int64_t fcap,
                               const pmvs_mesh_buffers* b, int64_t* nverts, int64_t* nfaces) {
  const size_t voxels = volume_voxels(*vol);
  const size_t cells = (size_t)(vol->dims[0] - 1) * (vol->dims[1] - 1) * (vol->dims[2] - 1);
  // no more vertices than cells and no more faces than 6 per voxel exist: the staging is sized by that
  const size_t nv = (size_t)std::min<int64_t>(vcap, (int64_t)cells), nf = (size_t)std::min<int64_t>(fcap, (int64_t)voxels * 6);
  CallArena arena;
  Staging stg(arena, dev);
  MeshArrays a;
  EXPCHK(stg.capped(&a.vertex, b->vertex, nv, 3, kVertices));
  EXPCHK(stg.capped(&a.normal, b->normal, nv, 3, kVertices));
  EXPCHK(stg.capped(&a.color, b->color, nv, 3, kVertices));
  EXPCHK(stg.capped(&a.face, b->face, nf, 3, kFaces));
  long long tv = 0, tf = 0;
  EXPCHK(tsdf_mesh_pass(*vol, min_obs, d_tsdf, d_obs, d_color, (long long)nv, (long long)nf, a, &tv, &tf, sc->stream));
  *nverts = tv;
  *nfaces = tf;
  stg.wrote(kVertices, (size_t)tv);
  stg.wrote(kFaces, (size_t)tf);
  EXPCHK(stg.finish(sc->stream));
  return PMVS_OK;
}

// Integration then extraction of the device records dP[0, n): the volume stays on the device.
pmvs_status mesh_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, int32_t first, int32_t num,
                         const pmvs_tsdf_params* prm, const pmvs_volume* vol, int32_t min_obs, int64_t vcap, int64_t fcap,
                         const pmvs_mesh_buffers* b, int64_t* nverts, int64_t* nfaces) {
  const size_t voxels = volume_voxels(*vol);
  CallArena arena;
  TsdfArrays a;
  EXPCHK(arena.alloc(&a.tsdf, voxels));
  EXPCHK(arena.alloc(&a.obs, voxels));
  EXPCHK(arena.alloc(&a.color, voxels * 4));
  {
    FuseMaps f;
    if (pmvs_status st = tsdf_maps(sc, dP, n, flags, first, num, prm->fuse, arena, f)) return st;
    EXPCHK(tsdf_integrate(sc->ds, f, first, num, *vol, prm->trunc, a, sc->stream));
    EXPCHK(hipStreamSynchronize(sc->stream));  // the maps are freed here, before the extraction's scratch
  }
  return mesh_device_volume(sc, (flags & PMVS_EXPORT_DEVICE) != 0, vol, min_obs, a.tsdf, a.obs, a.color, vcap, fcap, b, nverts,
                            nfaces);
}
}  // namespace

pmvs_status pmvs_loop_tsdf(pmvs_scene* sc, int32_t flags, int32_t first_target, int32_t num_targets,
                           const pmvs_tsdf_params* params, const pmvs_volume* volume, const pmvs_tsdf_buffers* buffers) {
  if (!buffers || !tsdf_args_ok(sc, flags, first_target, num_targets, params, volume)) return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_tsdf", &dP, &n)) return st;
  return tsdf_records(sc, dP, n, flags, first_target, num_targets, params, volume, buffers);
}

pmvs_status pmvs_tsdf_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t flags, int32_t first_target,
                              int32_t num_targets, const pmvs_tsdf_params* params, const pmvs_volume* volume,
                              const pmvs_tsdf_buffers* buffers) {
  if (!buffers || !tsdf_args_ok(sc, flags, first_target, num_targets, params, volume) || !records_ok(patches, n))
    return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  if (pmvs_status st = upload_records(sc, patches, n, nullptr, arena, &dP)) return st;
  return tsdf_records(sc, dP, n, flags, first_target, num_targets, params, volume, buffers);
}

pmvs_status pmvs_tsdf_mesh(pmvs_scene* sc, int32_t flags, const pmvs_volume* volume, int32_t min_obs, const float* tsdf,
                           const uint8_t* obs, const uint8_t* color, int64_t vcap, int64_t fcap, const pmvs_mesh_buffers* buffers,
                           int64_t* nverts, int64_t* nfaces) {
  if (!sc || !flags_ok(flags, PMVS_EXPORT_DEVICE) || !volume_ok(volume) || !tsdf || !obs ||
      !mesh_args_ok(min_obs, vcap, fcap, buffers, nverts, nfaces))
    return fail(PMVS_EINVAL, "invalid argument");
  HIPCHK(hipSetDevice(sc->device));
  const bool dev = (flags & PMVS_EXPORT_DEVICE) != 0;
  CallArena arena;
  if (!dev) {  // the volume goes up
    const size_t voxels = volume_voxels(*volume);
    float* d_tsdf = nullptr;
    uint8_t *d_obs = nullptr, *d_color = nullptr;
    EXPCHK(arena.alloc(&d_tsdf, voxels));
    EXPCHK(arena.alloc(&d_obs, voxels));
    EXPCHK(hipMemcpyAsync(d_tsdf, tsdf, voxels * sizeof(float), hipMemcpyHostToDevice, sc->stream));
    EXPCHK(hipMemcpyAsync(d_obs, obs, voxels, hipMemcpyHostToDevice, sc->stream));
    if (color) {
      EXPCHK(arena.alloc(&d_color, voxels * 4));
      EXPCHK(hipMemcpyAsync(d_color, color, voxels * 4, hipMemcpyHostToDevice, sc->stream));
    }
    tsdf = d_tsdf, obs = d_obs, color = d_color;
  }
  if (pmvs_status st = mesh_device_volume(sc, dev, volume, min_obs, tsdf, obs, color, vcap, fcap, buffers, nverts, nfaces)) return st;
  if (!dev) EXPCHK(hipStreamSynchronize(sc->stream));  // the uploads too, when there were no cells
  return PMVS_OK;
}

pmvs_status pmvs_loop_mesh(pmvs_scene* sc, int32_t flags, int32_t first_target, int32_t num_targets,
                           const pmvs_tsdf_params* params, const pmvs_volume* volume, int32_t min_obs, int64_t vcap, int64_t fcap,
                           const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces) {
  if (!mesh_args_ok(min_obs, vcap, fcap, buffers, nverts, nfaces) ||
      !tsdf_args_ok(sc, flags, first_target, num_targets, params, volume))
    return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_mesh", &dP, &n)) return st;
  return mesh_records(sc, dP, n, flags, first_target, num_targets, params, volume, min_obs, vcap, fcap, buffers, nverts, nfaces);
}

pmvs_status pmvs_mesh_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t flags, int32_t first_target,
                              int32_t num_targets, const pmvs_tsdf_params* params, const pmvs_volume* volume, int32_t min_obs,
                              int64_t vcap, int64_t fcap, const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces) {
  if (!mesh_args_ok(min_obs, vcap, fcap, buffers, nverts, nfaces) || !records_ok(patches, n) ||
      !tsdf_args_ok(sc, flags, first_target, num_targets, params, volume))
    return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  if (pmvs_status st = upload_records(sc, patches, n, nullptr, arena, &dP)) return st;
  return mesh_records(sc, dP, n, flags, first_target, num_targets, params, volume, min_obs, vcap, fcap, buffers, nverts, nfaces);
}

// ---- the sparse brick volume (pmvs_brick.hip)
namespace {
bool brick_volume_ok(const pmvs_volume* v) {
  if (!v || !std::isfinite(v->origin[0]) || !std::isfinite(v->origin[1]) || !std::isfinite(v->origin[2])) return false;
  if (!std::isfinite(v->voxel) || !(v->voxel > 0.0f)) return false;
  for (int a = 0; a < 3; ++a)
    if (v->dims[a] < 1 || v->dims[a] > PMVS_BRICK_MAX_DIM) return false;
  return pmvsbrick::grid_of(v->dims).bricks() <= INT32_MAX;  // at most 2^51: no overflow
}

bool brick_args_ok(const pmvs_scene* sc, int32_t flags, int32_t first, int32_t num, const pmvs_brick_params* p,
                   const pmvs_volume* v) {
  return p && tsdf_params_ok(&p->tsdf) && p->margin >= 0 && p->margin <= PMVS_BRICK_MAX_MARGIN && brick_volume_ok(v) &&
         range_call_ok(sc, flags, first, num);
}

enum { kBricks = 1 };  // Staging part: the brick arrays share the stored count

// The bricks of the device records dP[0, n): selection, then the first min(count, bcap) integrated.
pmvs_status brick_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, int32_t first, int32_t num,
                          const pmvs_brick_params* prm, const pmvs_volume* vol, int64_t bcap, const pmvs_brick_buffers* b,
                          int64_t* nbricks) {
  CallArena arena;
  Staging stg(arena, (flags & PMVS_EXPORT_DEVICE) != 0);
  FuseMaps f;
  BrickSelection sel;
  if (pmvs_status st = tsdf_maps(sc, dP, n, flags, first, num, prm->tsdf.fuse, arena, f)) return st;
  EXPCHK(brick_select(sc->ds, f, first, num, *vol, prm->margin, sel, sc->stream));
  *nbricks = sel.total;
  const size_t stored = (size_t)std::min<int64_t>(bcap, sel.total);  // the staging is sized by what exists
  long long* keys = nullptr;
  TsdfArrays a;
  EXPCHK(stg.capped(&keys, b->brick, stored, 1, kBricks));
  EXPCHK(stg.capped(&a.tsdf, b->tsdf, stored, PMVS_BRICK * PMVS_BRICK * PMVS_BRICK, kBricks));
  EXPCHK(stg.capped(&a.obs, b->obs, stored, PMVS_BRICK * PMVS_BRICK * PMVS_BRICK, kBricks));
  EXPCHK(stg.capped(&a.color, b->color, stored, PMVS_BRICK * PMVS_BRICK * PMVS_BRICK * 4, kBricks));
  if (stored > 0 && (keys || a.tsdf || a.obs || a.color)) {
    if (!keys) EXPCHK(arena.alloc(&keys, stored));  // the integration reads the list, wanted or not
    EXPCHK(brick_keys(sel, (long long)stored, keys, sc->stream));
    EXPCHK(brick_integrate(sc->ds, f, first, num, *vol, prm->tsdf.trunc, keys, (long long)stored, a, sc->stream));
  }
  stg.wrote(kBricks, stored);
  EXPCHK(stg.finish(sc->stream, true));  // in device mode too: the maps and the selection are freed on return
  return PMVS_OK;
}

// Surface nets over device bricks into the caller's buffers (device mode) or through staging.
pmvs_status brick_mesh_device(pmvs_scene* sc, bool dev, const pmvs_volume* vol, int32_t min_obs, int64_t nb, const long long* d_key,
                              const int* d_slot, const float* d_tsdf, const uint8_t* d_obs, const uint8_t* d_color, int64_t vcap,
                              int64_t fcap, const pmvs_mesh_buffers* b, int64_t* nverts, int64_t* nfaces) {
  const int64_t voxels = nb * (PMVS_BRICK * PMVS_BRICK * PMVS_BRICK);  // stored: < 2^40
  // no more vertices than stored voxels and no more faces than 6 per stored voxel exist
  const size_t nv = (size_t)std::min<int64_t>(vcap, voxels), nf = (size_t)std::min<int64_t>(fcap, voxels * 6);
  CallArena arena;
  Staging stg(arena, dev);
  MeshArrays a;
  EXPCHK(stg.capped(&a.vertex, b->vertex, nv, 3, kVertices));
  EXPCHK(stg.capped(&a.normal, b->normal, nv, 3, kVertices));
  EXPCHK(stg.capped(&a.color, b->color, nv, 3, kVertices));
  EXPCHK(stg.capped(&a.face, b->face, nf, 3, kFaces));
  long long tv = 0, tf = 0;
  EXPCHK(brick_mesh_pass(*vol, min_obs, nb, d_key, d_slot, d_tsdf, d_obs, d_color, (long long)nv, (long long)nf, a, &tv, &tf,
                         sc->stream));
  *nverts = tv;
  *nfaces = tf;
  if (tv > INT32_MAX) return fail(PMVS_EUNSUPPORTED, "brick mesh: %lld vertices do not fit the int32 face ids", tv);
  stg.wrote(kVertices, (size_t)tv);
  stg.wrote(kFaces, (size_t)tf);
  EXPCHK(stg.finish(sc->stream));
  return PMVS_OK;
}

// Selection, integration, then extraction of the device records dP[0, n): the bricks stay on the device.
pmvs_status brick_mesh_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, int32_t flags, int32_t first, int32_t num,
                               const pmvs_brick_params* prm, const pmvs_volume* vol, int32_t min_obs, int64_t vcap, int64_t fcap,
                               const pmvs_mesh_buffers* b, int64_t* nverts, int64_t* nfaces) {
  CallArena arena;
  BrickSelection sel;
  long long* keys = nullptr;
  TsdfArrays a;
  {
    FuseMaps f;
    if (pmvs_status st = tsdf_maps(sc, dP, n, flags, first, num, prm->tsdf.fuse, arena, f)) return st;
    EXPCHK(brick_select(sc->ds, f, first, num, *vol, prm->margin, sel, sc->stream));
    const size_t voxels = (size_t)sel.total * (PMVS_BRICK * PMVS_BRICK * PMVS_BRICK);
    EXPCHK(arena.alloc(&keys, (size_t)sel.total));
    EXPCHK(arena.alloc(&a.tsdf, voxels));
    EXPCHK(arena.alloc(&a.obs, voxels));
    EXPCHK(arena.alloc(&a.color, voxels * 4));
    EXPCHK(brick_keys(sel, sel.total, keys, sc->stream));
    EXPCHK(brick_integrate(sc->ds, f, first, num, *vol, prm->tsdf.trunc, keys, sel.total, a, sc->stream));
    EXPCHK(hipStreamSynchronize(sc->stream));  // the maps are freed here, before the extraction's scratch
  }
  sel.flag.release();
  return brick_mesh_device(sc, (flags & PMVS_EXPORT_DEVICE) != 0, vol, min_obs, sel.total, keys, sel.slot.p, a.tsdf, a.obs, a.color,
                           vcap, fcap, b, nverts, nfaces);
}
}  // namespace

pmvs_status pmvs_loop_brick_tsdf(pmvs_scene* sc, int32_t flags, int32_t first_target, int32_t num_targets,
                                 const pmvs_brick_params* params, const pmvs_volume* volume, int64_t bcap,
                                 const pmvs_brick_buffers* buffers, int64_t* nbricks) {
  if (!buffers || !nbricks || bcap < 0 || !brick_args_ok(sc, flags, first_target, num_targets, params, volume))
    return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_brick_tsdf", &dP, &n)) return st;
  return brick_records(sc, dP, n, flags, first_target, num_targets, params, volume, bcap, buffers, nbricks);
}

pmvs_status pmvs_brick_tsdf_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t flags, int32_t first_target,
                                    int32_t num_targets, const pmvs_brick_params* params, const pmvs_volume* volume, int64_t bcap,
                                    const pmvs_brick_buffers* buffers, int64_t* nbricks) {
  if (!buffers || !nbricks || bcap < 0 || !records_ok(patches, n) ||
      !brick_args_ok(sc, flags, first_target, num_targets, params, volume))
    return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  if (pmvs_status st = upload_records(sc, patches, n, nullptr, arena, &dP)) return st;
  return brick_records(sc, dP, n, flags, first_target, num_targets, params, volume, bcap, buffers, nbricks);
}

pmvs_status pmvs_brick_tsdf_mesh(pmvs_scene* sc, int32_t flags, const pmvs_volume* volume, int32_t min_obs, int64_t nbricks,
                                 const int64_t* brick, const float* tsdf, const uint8_t* obs, const uint8_t* color, int64_t vcap,
                                 int64_t fcap, const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces) {
  if (!sc || !flags_ok(flags, PMVS_EXPORT_DEVICE) || !brick_volume_ok(volume) || nbricks < 0 ||
      (nbricks > 0 && (!brick || !tsdf || !obs)) || !mesh_args_ok(min_obs, vcap, fcap, buffers, nverts, nfaces))
    return fail(PMVS_EINVAL, "invalid argument");
  const bool dev = (flags & PMVS_EXPORT_DEVICE) != 0;
  const int64_t grid = pmvsbrick::grid_of(volume->dims).bricks();
  if (nbricks > grid) return fail(PMVS_EINVAL, "brick_tsdf_mesh: more bricks than the grid holds");
  if (!dev)  // host keys are checked here, before the scene is touched; device keys by a kernel below
    for (int64_t s = 0; s < nbricks; ++s)
      if (brick[s] < 0 || brick[s] >= grid || (s > 0 && brick[s - 1] >= brick[s]))
        return fail(PMVS_EINVAL, "brick_tsdf_mesh: key %lld is outside the grid or not ascending", (long long)s);
  *nverts = *nfaces = 0;
  if (nbricks == 0) return PMVS_OK;  // an empty volume: an empty mesh
  HIPCHK(hipSetDevice(sc->device));
  CallArena arena;
  const long long* d_key = reinterpret_cast<const long long*>(brick);
  if (!dev) {  // the bricks go up
    const size_t nb = (size_t)nbricks, voxels = nb * (PMVS_BRICK * PMVS_BRICK * PMVS_BRICK);
    long long* u_key = nullptr;
    float* d_tsdf = nullptr;
    uint8_t *d_obs = nullptr, *d_color = nullptr;
    EXPCHK(arena.alloc(&u_key, nb));
    EXPCHK(arena.alloc(&d_tsdf, voxels));
    EXPCHK(arena.alloc(&d_obs, voxels));
    EXPCHK(hipMemcpyAsync(u_key, brick, nb * sizeof(int64_t), hipMemcpyHostToDevice, sc->stream));
    EXPCHK(hipMemcpyAsync(d_tsdf, tsdf, voxels * sizeof(float), hipMemcpyHostToDevice, sc->stream));
    EXPCHK(hipMemcpyAsync(d_obs, obs, voxels, hipMemcpyHostToDevice, sc->stream));
    if (color) {
      EXPCHK(arena.alloc(&d_color, voxels * 4));
      EXPCHK(hipMemcpyAsync(d_color, color, voxels * 4, hipMemcpyHostToDevice, sc->stream));
    }
    d_key = u_key, tsdf = d_tsdf, obs = d_obs, color = d_color;
  }
  DevBuf<int> slot;
  bool keys_ok = false;
  EXPCHK(brick_slots_from_keys(*volume, d_key, nbricks, slot, &keys_ok, sc->stream));
  if (!keys_ok) {
    EXPCHK(hipStreamSynchronize(sc->stream));
    return fail(PMVS_EINVAL, "brick_tsdf_mesh: the keys are not strictly ascending inside the grid");
  }
  if (pmvs_status st = brick_mesh_device(sc, dev, volume, min_obs, nbricks, d_key, slot.p, tsdf, obs, color, vcap, fcap, buffers,
                                         nverts, nfaces))
    return st;
  EXPCHK(hipStreamSynchronize(sc->stream));  // the uploads and the slot map too, when there were no cells
  return PMVS_OK;
}

pmvs_status pmvs_loop_brick_mesh(pmvs_scene* sc, int32_t flags, int32_t first_target, int32_t num_targets,
                                 const pmvs_brick_params* params, const pmvs_volume* volume, int32_t min_obs, int64_t vcap,
                                 int64_t fcap, const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces) {
  if (!mesh_args_ok(min_obs, vcap, fcap, buffers, nverts, nfaces) ||
      !brick_args_ok(sc, flags, first_target, num_targets, params, volume))
    return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_brick_mesh", &dP, &n)) return st;
  return brick_mesh_records(sc, dP, n, flags, first_target, num_targets, params, volume, min_obs, vcap, fcap, buffers, nverts,
                            nfaces);
}

pmvs_status pmvs_brick_mesh_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t flags, int32_t first_target,
                                    int32_t num_targets, const pmvs_brick_params* params, const pmvs_volume* volume, int32_t min_obs,
                                    int64_t vcap, int64_t fcap, const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces) {
  if (!mesh_args_ok(min_obs, vcap, fcap, buffers, nverts, nfaces) || !records_ok(patches, n) ||
      !brick_args_ok(sc, flags, first_target, num_targets, params, volume))
    return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  if (pmvs_status st = upload_records(sc, patches, n, nullptr, arena, &dP)) return st;
  return brick_mesh_records(sc, dP, n, flags, first_target, num_targets, params, volume, min_obs, vcap, fcap, buffers, nverts,
                            nfaces);
}

// ---- the mesh rasterised into the targets and a view per face (pmvs_texmesh.hip)
namespace {
bool texture_params_ok(const pmvs_texture_params* p) {
  return p && std::isfinite(p->depth_rel) && p->depth_rel >= 0.0f && std::isfinite(p->min_area) && p->min_area >= 0.0f;
}

// What both calls check of the mesh and the scene; the scene last (range_call_ok).
bool texmesh_args_ok(const pmvs_scene* sc, int32_t flags, int32_t first, int32_t num, int64_t nv, const float* vertex, int64_t nf,
                     const int32_t* face) {
  return nv >= 0 && nv <= INT32_MAX && nf >= 0 && nf <= INT32_MAX && (nv == 0 || vertex) && (nf == 0 || face) &&
         flags_ok(flags, PMVS_EXPORT_DEVICE) && range_call_ok(sc, flags, first, num);
}

// The mesh on the device: the caller's pointers in device mode, uploaded into the arena otherwise.  Host ids
// are checked here before the scene is touched, device ids by a kernel before any of them is an index.
pmvs_status texmesh_device_mesh(pmvs_scene* sc, bool dev, const char* call, int64_t nv, const float* vertex, int64_t nf,
                                const int32_t* face, CallArena& arena, const float** d_vertex, const int** d_face) {
  *d_vertex = vertex, *d_face = face;
  if (!dev)
    for (int64_t i = 0; i < 3 * nf; ++i)
      if (face[i] < 0 || face[i] >= nv) return fail(PMVS_EINVAL, "%s: face %lld has a vertex id outside [0, nv)", call, (long long)(i / 3));
  HIPCHK(hipSetDevice(sc->device));
  if (!dev) {
    float* uv = nullptr;
    int* uf = nullptr;
    EXPCHK(arena.alloc(&uv, (size_t)nv * 3));
    EXPCHK(arena.alloc(&uf, (size_t)nf * 3));
    if (nv) EXPCHK(hipMemcpyAsync(uv, vertex, (size_t)nv * 3 * sizeof(float), hipMemcpyHostToDevice, sc->stream));
    if (nf) EXPCHK(hipMemcpyAsync(uf, face, (size_t)nf * 3 * sizeof(int), hipMemcpyHostToDevice, sc->stream));
    *d_vertex = uv, *d_face = uf;
  } else {
    bool ids_ok = true;
    EXPCHK(mesh_ids_check(face, nf, nv, &ids_ok, sc->stream));
    if (!ids_ok) return fail(PMVS_EINVAL, "%s: a face has a vertex id outside [0, nv)", call);
  }
  return PMVS_OK;
}
}  // namespace

pmvs_status pmvs_mesh_raster(pmvs_scene* sc, int32_t flags, int32_t first_target, int32_t num_targets, int64_t nv,
                             const float* vertex, int64_t nf, const int32_t* face, const pmvs_raster_buffers* buffers) {
  if (!buffers || !texmesh_args_ok(sc, flags, first_target, num_targets, nv, vertex, nf, face))
    return fail(PMVS_EINVAL, "invalid argument");
  const bool dev = (flags & PMVS_EXPORT_DEVICE) != 0;
  CallArena arena;
  const float* d_vertex = nullptr;
  const int* d_face = nullptr;
  if (pmvs_status st = texmesh_device_mesh(sc, dev, "mesh_raster", nv, vertex, nf, face, arena, &d_vertex, &d_face)) return st;
  const size_t pixels = (size_t)pixel_map_layout(sc, first_target, num_targets, nullptr, nullptr);
  Staging stg(arena, dev);
  RasterArrays a;
  EXPCHK(stg.fixed(&a.face, buffers->face, pixels));
  EXPCHK(stg.fixed(&a.depth, buffers->depth, pixels));
  EXPCHK(mesh_raster_pass(sc->ds, sc->hviews.data(), first_target, num_targets, d_vertex, nf, d_face, a, sc->stream));
  EXPCHK(stg.finish(sc->stream, true));  // in device mode too: the uploads' arena is freed on return
  return PMVS_OK;
}

pmvs_status pmvs_mesh_texture(pmvs_scene* sc, int32_t flags, int32_t first_target, int32_t num_targets,
                              const pmvs_texture_params* params, int64_t nv, const float* vertex, int64_t nf,
                              const int32_t* face, const pmvs_texture_buffers* buffers) {
  if (!buffers || !texture_params_ok(params) || !texmesh_args_ok(sc, flags, first_target, num_targets, nv, vertex, nf, face))
    return fail(PMVS_EINVAL, "invalid argument");
  if (nf == 0) return PMVS_OK;  // no face: nothing is written
  const bool dev = (flags & PMVS_EXPORT_DEVICE) != 0;
  CallArena arena;
  const float* d_vertex = nullptr;
  const int* d_face = nullptr;
  if (pmvs_status st = texmesh_device_mesh(sc, dev, "mesh_texture", nv, vertex, nf, face, arena, &d_vertex, &d_face)) return st;
  Staging stg(arena, dev);
  TextureArrays a;
  EXPCHK(stg.fixed(&a.view, buffers->view, (size_t)nf));
  EXPCHK(stg.fixed(&a.uv, buffers->uv, (size_t)nf * 6));
  EXPCHK(stg.fixed(&a.score, buffers->score, (size_t)nf));
  EXPCHK(mesh_texture_pass(sc->ds, sc->hviews.data(), first_target, num_targets, *params, d_vertex, nf, d_face, a, sc->stream));
  EXPCHK(stg.finish(sc->stream, true));
  return PMVS_OK;
}

// ---- the textured mesh baked into one atlas image (pmvs_atlas.hip)
namespace {
bool atlas_params_ok(const pmvs_atlas_params* p) {
  return p && p->max_side >= 1 && p->max_side <= PMVS_ATLAS_MAX_SIDE && p->width >= p->max_side + 5 &&
         p->width <= PMVS_ATLAS_MAX_WIDTH && std::isfinite(p->scale) && p->scale > 0.0f;
}

enum { kAtlasRows = 1 };  // Staging part: the two images share the written rows
}  // namespace

pmvs_status pmvs_atlas_layout_from_counts(const pmvs_atlas_params* params, const int64_t* counts, pmvs_atlas_layout* layout,
                                          int64_t* band_y) {
  if (!atlas_params_ok(params) || !counts || !layout) return fail(PMVS_EINVAL, "invalid argument");
  for (int n = 1; n <= params->max_side; ++n)
    if (counts[n] < 0) return fail(PMVS_EINVAL, "atlas_layout_from_counts: class %d has a negative count", n);
  // 251 classes of up to 2^63 faces: summed in 128 bits and reported saturated, so that nothing wraps
  __int128 y = 0, placed = 0, cells = 0;
  const auto sat = [](__int128 v) { return v > INT64_MAX ? INT64_MAX : (int64_t)v; };
  for (int n = params->max_side; n >= 1; --n) {
    if (band_y) band_y[n] = sat(y);
    y += (__int128)pmvsatlas::class_rows(counts[n], params->width, n) * (n + 5);
    placed += counts[n];
    cells += pmvsatlas::class_slots(counts[n]);
  }
  if (band_y) band_y[0] = sat(y);
  *layout = pmvs_atlas_layout{params->width, sat(y), sat(placed), sat(cells)};
  if (y > INT32_MAX) return fail(PMVS_EUNSUPPORTED, "atlas_layout_from_counts: the atlas height %lld exceeds 2^31-1", (long long)sat(y));
  return PMVS_OK;
}

pmvs_status pmvs_mesh_atlas(pmvs_scene* sc, int32_t flags, const pmvs_atlas_params* params, int64_t nv, const float* vertex,
                            int64_t nf, const int32_t* face, const int32_t* view, int64_t height_cap,
                            const pmvs_atlas_buffers* buffers, pmvs_atlas_layout* layout) {
  if (!atlas_params_ok(params) || !layout || !flags_ok(flags, PMVS_EXPORT_DEVICE) || nv < 0 || nv > INT32_MAX || nf < 0 ||
      nf > INT32_MAX || (nv > 0 && !vertex) || (nf > 0 && (!face || !view)) || height_cap < 0 || !sc)
    return fail(PMVS_EINVAL, "invalid argument");
  const bool dev = (flags & PMVS_EXPORT_DEVICE) != 0;
  const int tnum = sc->ds.tnum;
  for (int t = 0; t < tnum; ++t)
    if (sc->hviews[t].w[0] < 2 || sc->hviews[t].h[0] < 2)
      return fail(PMVS_EINVAL, "mesh_atlas: target %d is smaller than 2 x 2 pixels at level 0", t);
  if (!dev)
    for (int64_t f = 0; f < nf; ++f)
      if (view[f] < -1 || view[f] >= tnum) return fail(PMVS_EINVAL, "mesh_atlas: face %lld has a view outside [-1, num_targets)", (long long)f);
  const pmvs_atlas_buffers none{};
  const pmvs_atlas_buffers& b = buffers ? *buffers : none;
  CallArena arena;
  const float* d_vertex = nullptr;
  const int* d_face = nullptr;
  const int* d_view = view;
  if (!dev) {  // the host ids are checked, then the mesh goes up
    if (pmvs_status st = texmesh_device_mesh(sc, false, "mesh_atlas", nv, vertex, nf, face, arena, &d_vertex, &d_face)) return st;
    int* uview = nullptr;
    EXPCHK(arena.alloc(&uview, (size_t)nf));
    if (nf) EXPCHK(hipMemcpyAsync(uview, view, (size_t)nf * sizeof(int), hipMemcpyHostToDevice, sc->stream));
    d_view = uview;
  } else {
    HIPCHK(hipSetDevice(sc->device));
    d_vertex = vertex, d_face = face;
    bool ids_ok = true;
    EXPCHK(atlas_ids_check(face, view, nf, nv, tnum, &ids_ok, sc->stream));
    if (!ids_ok) return fail(PMVS_EINVAL, "mesh_atlas: a face has a vertex id outside [0, nv) or a view outside [-1, num_targets)");
  }
  AtlasWork work;
  long long counts[PMVS_ATLAS_MAX_SIDE + 1];
  EXPCHK(atlas_classify(sc->ds, *params, d_vertex, nf, d_face, d_view, work, counts, sc->stream));
  int64_t counts64[PMVS_ATLAS_MAX_SIDE + 1], band_y[PMVS_ATLAS_MAX_SIDE + 1];
  for (int n = 0; n <= PMVS_ATLAS_MAX_SIDE; ++n) counts64[n] = counts[n];
  if (pmvs_status st = pmvs_atlas_layout_from_counts(params, counts64, layout, band_y)) {
    if (!dev) EXPCHK(hipStreamSynchronize(sc->stream));  // the uploads' arena is freed on return
    return st;
  }
  const size_t rows = (size_t)std::min<int64_t>(layout->height, height_cap), W = (size_t)params->width;
  Staging stg(arena, dev);
  AtlasArrays a;
  EXPCHK(stg.capped(&a.rgb, b.rgb, rows, W * 3, kAtlasRows));
  EXPCHK(stg.capped(&a.texel_face, b.texel_face, rows, W, kAtlasRows));
  EXPCHK(stg.fixed(&a.uv, b.uv, (size_t)nf * 6));
  EXPCHK(stg.fixed(&a.atlas_view, b.atlas_view, (size_t)nf));
  long long band_ll[PMVS_ATLAS_MAX_SIDE + 1];
  for (int n = 0; n <= PMVS_ATLAS_MAX_SIDE; ++n) band_ll[n] = n <= params->max_side ? band_y[n] : 0;
  EXPCHK(atlas_render_pass(sc->ds, *params, d_vertex, nf, d_face, d_view, work, counts, band_ll, (long long)rows, a, sc->stream));
  EXPCHK(stg.finish(sc->stream, true));  // in device mode too: the uploads' arena is freed on return
  return PMVS_OK;
}

// ---- text files (pmvs_text.hip)
namespace {
bool text_args_ok(const pmvs_scene* sc, int32_t kind, int32_t flags, const char* out, int64_t cap, const int64_t* bytes) {
  return sc && bytes && (kind == PMVS_TEXT_PLY || kind == PMVS_TEXT_PATCH || kind == PMVS_TEXT_PSET) && flags_ok(flags) &&
         cap >= 0 && (out || cap == 0);
}

// The header of a `kind` file of n patches (pmvs_io.cpp's writers).
std::string text_header(int32_t kind, int32_t n) {
  if (kind == PMVS_TEXT_PLY)
    return "ply\nformat ascii 1.0\nelement vertex " + std::to_string(n) +
           "\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\n"
           "property float nz\nproperty uchar diffuse_red\nproperty uchar diffuse_green\n"
           "property uchar diffuse_blue\nproperty float quality\nend_header\n";
  if (kind == PMVS_TEXT_PATCH) return "PATCHES\n" + std::to_string(n) + "\n";
  return std::string();
}

// The text of the device records dP[0, n); sz = their totals.
pmvs_status text_records(pmvs_scene* sc, const pmvs_patch* dP, int32_t n, const pmvs_export_sizes& sz, int32_t kind,
                         int32_t flags, const int32_t* index2image, char* out, int64_t cap, int64_t* bytes) {
  const bool dev = (flags & PMVS_EXPORT_DEVICE) != 0;
  const std::string header = text_header(kind, n);
  CallArena arena;
  Staging stg(arena, dev);
  TextArrays t;
  long long* d_off = nullptr;
  int64_t total = (int64_t)header.size();
  if (n > 0) {
    // the export's arrays this kind reads, into call-scoped scratch
    const size_t np = (size_t)n;
    ExportArrays a;
    EXPCHK(arena.alloc(&a.fields, np * 11));
    if (kind == PMVS_TEXT_PLY) EXPCHK(arena.alloc(&a.colors, np * 3));
    if (kind == PMVS_TEXT_PATCH) {
      EXPCHK(arena.alloc(&a.image_off, np + 1));
      EXPCHK(arena.alloc(&a.image_ids, (size_t)sz.image_entries));
      EXPCHK(arena.alloc(&a.vimage_off, np + 1));
      EXPCHK(arena.alloc(&a.vimage_ids, (size_t)sz.vimage_entries));
    }
    int* d_tab = nullptr;
    if (pmvs_status st = upload_index2image(sc, kind == PMVS_TEXT_PATCH ? index2image : nullptr, arena, &d_tab)) return st;
    const int max_gwidth = depth_map_layout(sc, nullptr, nullptr);
    EXPCHK(export_pass(sc->ds, dP, n, (flags & PMVS_EXPORT_WRITER_ORDER) != 0, max_gwidth, d_tab, a, sc->stream));
    t.fields = a.fields; t.colors = a.colors; t.image_off = a.image_off; t.image_ids = a.image_ids;
    t.vimage_off = a.vimage_off; t.vimage_ids = a.vimage_ids;
    EXPCHK(arena.alloc(&d_off, np + 1));
    EXPCHK(text_offsets(kind, t, n, (long long)header.size(), d_off, sc->stream));
    long long end = 0;
    EXPCHK(hipMemcpyAsync(&end, d_off + n, sizeof(end), hipMemcpyDeviceToHost, sc->stream));
    EXPCHK(hipStreamSynchronize(sc->stream));
    total = end;
  }
  *bytes = total;
  if (!out && cap == 0) return PMVS_OK;  // the size query
  if (cap < total) return fail(PMVS_EINVAL, "text: the buffer holds %lld bytes, the text has %lld", (long long)cap, (long long)total);
  if (total == 0) return PMVS_OK;
  if (!dev && n == 0) {
    std::memcpy(out, header.data(), header.size());
    return PMVS_OK;
  }
  char* d_out = nullptr;
  EXPCHK(stg.fixed(&d_out, out, (size_t)total));
  if (!header.empty()) EXPCHK(hipMemcpyAsync(d_out, header.data(), header.size(), hipMemcpyHostToDevice, sc->stream));
  EXPCHK(text_write(kind, t, n, d_off, d_out, sc->stream));
  // in device mode too: the scratch and the header are freed on return, the work that reads them must have finished
  EXPCHK(stg.finish(sc->stream, true));
  return PMVS_OK;
}
}  // namespace

pmvs_status pmvs_loop_text(pmvs_scene* sc, int32_t kind, int32_t flags, const int32_t* index2image, char* out,
                           int64_t cap, int64_t* bytes) {
  if (!text_args_ok(sc, kind, flags, out, cap, bytes)) return fail(PMVS_EINVAL, "invalid argument");
  const pmvs_patch* dP = nullptr;
  int32_t n = 0;
  if (pmvs_status st = loop_records(sc, "loop_text", &dP, &n)) return st;
  pmvs_export_sizes sz{};
  if (pmvs_status st = device_export_sizes(sc, dP, n, &sz)) return st;
  return text_records(sc, dP, n, sz, kind, flags, index2image, out, cap, bytes);
}

pmvs_status pmvs_text_patches(pmvs_scene* sc, const pmvs_patch* patches, int32_t n, int32_t kind, int32_t flags,
                              const int32_t* index2image, char* out, int64_t cap, int64_t* bytes) {
  if (!text_args_ok(sc, kind, flags, out, cap, bytes) || !records_ok(patches, n)) return fail(PMVS_EINVAL, "invalid argument");
  CallArena arena;
  const pmvs_patch* dP = nullptr;
  pmvs_export_sizes sz{};
  if (pmvs_status st = upload_records(sc, patches, n, &sz, arena, &dP)) return st;
  return text_records(sc, dP, n, sz, kind, flags, index2image, out, cap, bytes);
}

pmvs_status pmvs_selftest_format(int32_t device, int32_t precision, const float* in, int32_t n, char* out, int32_t* len) {
  if (!in || !out || !len || n <= 0 || (precision != 6 && precision != 17)) return fail(PMVS_EINVAL, "invalid argument");
  if (device == -1) {  // the same source on the host
    std::memset(out, 0, (size_t)n * 24);
    for (int i = 0; i < n; ++i) len[i] = pmvsfmt::fmt_g(in[i], precision, out + (size_t)i * 24);
    return PMVS_OK;
  }
  HIPCHK(hipSetDevice(device));
  CallArena arena;
  float* d_in = nullptr;
  char* d_out = nullptr;
  int* d_len = nullptr;
  EXPCHK(arena.alloc(&d_in, (size_t)n));
  EXPCHK(arena.alloc(&d_out, (size_t)n * 24));
  EXPCHK(arena.alloc(&d_len, (size_t)n));
  EXPCHK(hipMemcpy(d_in, in, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
  EXPCHK(hipMemset(d_out, 0, (size_t)n * 24));
  EXPCHK(launch_format_selftest(precision, d_in, n, d_out, d_len, nullptr));
  EXPCHK(hipMemcpy(out, d_out, (size_t)n * 24, hipMemcpyDeviceToHost));
  EXPCHK(hipMemcpy(len, d_len, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  return PMVS_OK;
}

pmvs_status pmvs_selftest_labels(int32_t device, int32_t n, const int32_t* edge_off, const int32_t* edges, int32_t* lab_out,
                                 int32_t* stats_out) {
  if (n <= 0 || !edge_off || !lab_out || !stats_out || edge_off[0] != 0) return fail(PMVS_EINVAL, "invalid argument");
  for (int i = 0; i < n; ++i)
    if (edge_off[i + 1] < edge_off[i]) return fail(PMVS_EINVAL, "edge_off decreases at %d", i);
  if (edge_off[n] > 0 && !edges) return fail(PMVS_EINVAL, "invalid argument");
  for (int e = 0; e < edge_off[n]; ++e)
    if (edges[e] < 0 || edges[e] >= n) return fail(PMVS_EINVAL, "edge %d leaves the graph", e);
  HIPCHK(hipSetDevice(device));
  const hipError_t e = labels_selftest(edge_off, edges, n, lab_out, stats_out);
  if (e != hipSuccess) return fail(PMVS_EDEVICE, "labels selftest: %s", hipGetErrorString(e));
  return PMVS_OK;
}

pmvs_status pmvs_scene_set_shard(pmvs_scene* sc, int32_t rank, int32_t world, pmvs_allgather_fn fn, void* ctx) {
  if (!sc || world < 1 || rank < 0 || rank >= world || (world > 1 && !fn)) return fail(PMVS_EINVAL, "invalid shard");
  sc->shard_rank = rank;
  sc->shard_world = world;
  sc->shard_fn = fn;
  sc->shard_ctx = ctx;
  sc->shard_rccl = nullptr;
  return PMVS_OK;
}

pmvs_status pmvs_scene_set_cluster(pmvs_scene* sc, int32_t rank, int32_t world, const int32_t* image_ids,
                                   pmvs_allgather_fn fn, void* ctx) {
  if (!sc || world < 1 || rank < 0 || rank >= world || (world > 1 && (!fn || !image_ids)))
    return fail(PMVS_EINVAL, "invalid cluster");
  sc->cl_world = 1;
  sc->cl_fn = nullptr;
  sc->cl_rccl = nullptr;
  if (world == 1) return PMVS_OK;
  const int num = sc->ds.num, tnum = sc->ds.tnum;
  // Local validation first; its outcome travels in the all-gather (mine[0] < 0), so a rank with a
  // bad argument fails together with its peers instead of leaving them in the collective.
  pmvs_status bad = PMVS_OK;
  int maxid = -1;
  std::vector<int> id2idx;
  if (tnum > PMVS_MAX_TARGETS) bad = fail(PMVS_EUNSUPPORTED, "cluster: more than %d target images", PMVS_MAX_TARGETS);
  for (int i = 0; i < num && !bad; ++i) {
    if (image_ids[i] < 0) bad = fail(PMVS_EINVAL, "image_ids[%d] = %d", i, image_ids[i]);
    maxid = std::max(maxid, image_ids[i]);
  }
  if (!bad && maxid > (1 << 26)) bad = fail(PMVS_EUNSUPPORTED, "image number %d", maxid);
  if (!bad) {
    id2idx.assign((size_t)maxid + 1, -1);
    for (int i = 0; i < num && !bad; ++i) {
      if (id2idx[image_ids[i]] >= 0) bad = fail(PMVS_EINVAL, "image number %d appears twice", image_ids[i]);
      id2idx[image_ids[i]] = i;
    }
  }
  // all-gather of the target image numbers (collective): a target is shared when another cluster
  // has it as a target too
  std::vector<int> mine(1 + PMVS_MAX_TARGETS, -1), all((size_t)(1 + PMVS_MAX_TARGETS) * world, -1);
  mine[0] = bad ? -1 : tnum;
  for (int t = 0; t < tnum && !bad; ++t) mine[1 + t] = image_ids[t];
  if (fn(ctx, mine.data(), (int64_t)(mine.size() * sizeof(int)), all.data()) != 0)
    return fail(PMVS_EDEVICE, "cluster setup: the all-gather failed");
  if (bad) return bad;
  for (int r = 0; r < world; ++r)
    if (all[(size_t)r * (1 + PMVS_MAX_TARGETS)] < 0) return fail(PMVS_EINVAL, "cluster setup: rank %d failed its validation", r);
  std::vector<unsigned char> shared(std::max(tnum, 1), 0);
  for (int r = 0; r < world; ++r) {
    if (r == rank) continue;
    const int* o = all.data() + (size_t)r * (1 + PMVS_MAX_TARGETS);
    for (int k = 0; k < std::min(o[0], PMVS_MAX_TARGETS); ++k) {
      const int id = o[1 + k];
      if (0 <= id && id <= maxid && id2idx[id] >= 0 && id2idx[id] < tnum) shared[id2idx[id]] = 1;
    }
  }
  HIPCHK(hipSetDevice(sc->device));
  pmvs_status st;
  if ((st = ensure(sc->cl_shared, shared.size())) || (st = ensure(sc->cl_ids, (size_t)num)) ||
      (st = ensure(sc->cl_id2idx, id2idx.size())))
    return st;
  HIPCHK(hipMemcpy(sc->cl_shared.p, shared.data(), shared.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(sc->cl_ids.p, image_ids, (size_t)num * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(sc->cl_id2idx.p, id2idx.data(), id2idx.size() * sizeof(int), hipMemcpyHostToDevice));
  sc->cl_maxid = maxid;
  sc->cl_rank = rank;
  sc->cl_world = world;
  sc->cl_fn = fn;
  sc->cl_ctx = ctx;
  return PMVS_OK;
}

pmvs_status pmvs_scene_set_cluster_rccl(pmvs_scene* sc, int32_t rank, int32_t world, const int32_t* image_ids,
                                        pmvs_rccl* comm) {
  if (!sc || !comm) return fail(PMVS_EINVAL, "invalid cluster");
  const pmvs_status st = pmvs_scene_set_cluster(sc, rank, world, image_ids, &pmvs_rccl_allgather, comm);
  if (st == PMVS_OK && world > 1) sc->cl_rccl = comm;
  return st;
}

pmvs_status pmvs_scene_set_shard_rccl(pmvs_scene* sc, int32_t rank, int32_t world, pmvs_rccl* comm) {
  if (!sc || !comm || world < 1 || rank < 0 || rank >= world) return fail(PMVS_EINVAL, "invalid shard");
  const pmvs_status st = pmvs_scene_set_shard(sc, rank, world, &pmvs_rccl_allgather, comm);
  if (st == PMVS_OK) sc->shard_rccl = comm;
  return st;
}

// ---- in-process all-gather among threads (generation-counted barrier)
struct pmvs_thread_exchange {
  int world = 1;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0, leaving = 0;
  long long gen = 0;
  std::vector<const void*> send;
  int64_t bytes = -1;
  bool bad = false;
  std::vector<std::pair<pmvs_thread_exchange*, int>> ctx;
};

pmvs_thread_exchange* pmvs_thread_exchange_create(int32_t world) {
  if (world < 1) return nullptr;
  auto* g = new pmvs_thread_exchange();
  g->world = world;
  g->send.assign(world, nullptr);
  for (int r = 0; r < world; ++r) g->ctx.push_back({g, r});
  return g;
}

void* pmvs_thread_exchange_ctx(pmvs_thread_exchange* g, int32_t rank) {
  if (!g || rank < 0 || rank >= g->world) return nullptr;
  return &g->ctx[rank];
}

int pmvs_thread_allgather(void* ctx, const void* send, int64_t bytes, void* recv) {
  auto* c = static_cast<std::pair<pmvs_thread_exchange*, int>*>(ctx);
  if (!c) return -1;
  pmvs_thread_exchange* g = c->first;
  const int r = c->second;
  std::unique_lock<std::mutex> lk(g->mu);
  g->cv.wait(lk, [&] { return g->leaving == 0; });  // the previous round has fully drained
  if (g->arrived == 0) { g->bytes = bytes; g->bad = false; }
  if (bytes != g->bytes) g->bad = true;
  g->send[r] = send;
  const long long my = g->gen;
  if (++g->arrived == g->world) {
    g->leaving = g->world;
    g->arrived = 0;
    ++g->gen;
    g->cv.notify_all();
  } else {
    g->cv.wait(lk, [&] { return g->gen != my; });
  }
  const bool bad = g->bad;
  if (!bad)
    for (int k = 0; k < g->world; ++k) std::memcpy((char*)recv + (size_t)k * bytes, g->send[k], (size_t)bytes);
  if (--g->leaving == 0) g->cv.notify_all();  // nobody returns before every copy is done
  else g->cv.wait(lk, [&] { return g->leaving == 0; });
  return bad ? -1 : 0;
}

void pmvs_thread_exchange_destroy(pmvs_thread_exchange* g) { delete g; }
