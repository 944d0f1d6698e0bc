// export_timing_host.cpp -- the way pmvs2 turned a loop result into writer-ready host arrays before
// pmvs_loop_export: pmvs_loop_fetch of every record, the collectPatches(1) key and std::stable_sort on
// the host, the single-threaded gather of fields and lists, and pmvs_patch_colors (coordinates and
// lists uploaded again).  tools/export_timing.py builds this file (g++ -O2 -shared) and times it
// against the device export, from "loop finished" to "arrays on the host".
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <vector>

#include "../include/pmvs_amd.h"

namespace {
std::vector<float> g_fields;
std::vector<int32_t> g_nimg, g_nvimg, g_ids, g_vids, g_idx, g_colors;
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}  // namespace

typedef pmvs_status (*fetch_fn)(pmvs_scene*, pmvs_patch*, int32_t);
typedef pmvs_status (*colors_fn)(pmvs_scene*, int32_t, const float*, const int32_t*, const int32_t*, int32_t*);

// gwidth: per view, the cell-grid width; images: index2image.  seconds: fetch, host ordering and
// gather, colours.  entries: image / vimage list entries.  Returns the first failing status.
extern "C" int host_path(pmvs_scene* sc, int nmodel, int tnum, const int* gwidth, const int* images, fetch_fn fetch,
                         colors_fn patch_colors, double seconds[3], long long entries[2]) {
  const double t0 = now_s();
  std::vector<pmvs_patch> model(std::max(nmodel, 1));
  if (int st = fetch(sc, model.data(), nmodel)) return st;
  model.resize(nmodel);
  const double t1 = now_s();
  std::vector<long long> key(nmodel);
  for (int p = 0; p < nmodel; ++p) {
    const pmvs_patch& q = model[p];
    int bt = INT_MAX, k0 = -1;
    for (int k = 0; k < q.num_images; ++k)
      if (q.images[k] < tnum && q.images[k] < bt) { bt = q.images[k]; k0 = k; }
    key[p] = k0 < 0 ? LLONG_MAX
                    : ((long long)bt << 40) + (long long)q.grids[k0][1] * gwidth[bt] + q.grids[k0][0];
  }
  std::vector<int> order(nmodel);
  for (int p = 0; p < nmodel; ++p) order[p] = p;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
  std::vector<float> fields((size_t)nmodel * 11);
  std::vector<int32_t> nimg(nmodel), nvimg(nmodel), ids, vids, idx;
  for (int r = 0; r < nmodel; ++r) {
    const pmvs_patch& q = model[order[r]];
    float* f = fields.data() + (size_t)r * 11;
    for (int k = 0; k < 4; ++k) { f[k] = q.coord[k]; f[4 + k] = q.normal[k]; }
    f[8] = q.ncc; f[9] = q.dscale; f[10] = q.ascale;
    nimg[r] = q.num_images;
    nvimg[r] = q.num_vimages;
    for (int k = 0; k < q.num_images; ++k) {
      ids.push_back(images[q.images[k]]);  // index2image
      idx.push_back(q.images[k]);
    }
    for (int k = 0; k < q.num_vimages; ++k) vids.push_back(images[q.vimages[k]]);
  }
  std::vector<float> coords((size_t)std::max(nmodel, 1) * 4);
  for (int r = 0; r < nmodel; ++r)
    for (int k = 0; k < 4; ++k) coords[(size_t)4 * r + k] = fields[(size_t)r * 11 + k];
  const double t2 = now_s();
  std::vector<int32_t> colors((size_t)std::max(nmodel, 1) * 3);
  if (nmodel)
    if (int st = patch_colors(sc, nmodel, coords.data(), nimg.data(), idx.data(), colors.data())) return st;
  const double t3 = now_s();
  seconds[0] = t1 - t0; seconds[1] = t2 - t1; seconds[2] = t3 - t2;
  entries[0] = (long long)ids.size(); entries[1] = (long long)vids.size();
  g_fields.swap(fields); g_nimg.swap(nimg); g_nvimg.swap(nvimg); g_ids.swap(ids); g_vids.swap(vids); g_idx.swap(idx);
  g_colors.swap(colors);
  return 0;
}

// The arrays of the last host_path call (for the comparison with the device export), then released.
extern "C" void host_path_take(float* fields, int32_t* colors, int32_t* nimg, int32_t* ids, int32_t* nvimg, int32_t* vids) {
  std::copy(g_fields.begin(), g_fields.end(), fields);
  std::copy(g_colors.begin(), g_colors.begin() + g_nimg.size() * 3, colors);
  std::copy(g_nimg.begin(), g_nimg.end(), nimg);
  std::copy(g_ids.begin(), g_ids.end(), ids);
  std::copy(g_nvimg.begin(), g_nvimg.end(), nvimg);
  std::copy(g_vids.begin(), g_vids.end(), vids);
  for (auto* v : {&g_nimg, &g_nvimg, &g_ids, &g_vids, &g_idx, &g_colors}) std::vector<int32_t>().swap(*v);
  std::vector<float>().swap(g_fields);
}
