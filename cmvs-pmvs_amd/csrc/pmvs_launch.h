// pmvs_launch.h -- host-side launchers of the kernels in pmvs_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include "pmvs_device.h"
#include "pmvs_devbuf.h"
#include "pmvs_refine_layouts.h"
#include <functional>
#include <memory>
#include <utility>
#include <vector>

namespace pmvsdev {

// hipMemsetAsync in pieces of at most 1 GiB: the C5-scale buffers (a 70-view 8K pyramid is 12 GB,
// its cell tables 2-5 GB) exceed what one fill launch takes (a 12 GB pyramid clear failed with
// "invalid resource handle", gpurun r03p).
inline hipError_t memset_big(void* p, int value, size_t bytes, hipStream_t st) {
  constexpr size_t kPiece = size_t(1) << 30;
  char* c = static_cast<char*>(p);
  for (size_t off = 0; off < bytes; off += kPiece) {
    const hipError_t e = hipMemsetAsync(c + off, value, bytes - off < kPiece ? bytes - off : kPiece, st);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// Page-locked host staging (hipHostMalloc), grown on demand with 25 % headroom: the large per-pass
// downloads (filterSmallGroups' edge lists, the expansion queue's initial order) and the refine batches'
// start points at full PCIe rate.
struct PinnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {  // o leaves with the old buffer and frees it
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t c = bytes + bytes / 4 + 4096;
    const hipError_t e = hipHostMalloc(&p, c, hipHostMallocDefault);
    if (e == hipSuccess) cap = c;
    return e;
  }
  template <class T>
  T* as(size_t offset_bytes = 0) const { return reinterpret_cast<T*>(static_cast<char*>(p) + offset_bytes); }
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
};
// Host staging of the refine batches' start-point angles (encode_angles_host, pmvs_kernels.hip).
struct RefineHost {
  DevBuf<float4> d_enc;
  DevBuf<double2> d_ang;
  PinnedBuf h_enc, h_ang;
  DevBuf<unsigned char> bq_cold;  // the split-form refine kernel's cold optimizer state (launch_refine_split)
  // PMVS_EXPAND_PROFILE: the round trip's share of the device timeline (pre_kernel's end to the
  // refine kernel's start: start points down, host libm, angles up), summed over the batches
  bool prof = false;
  hipEvent_t ev_pre = nullptr;
  double trip_ms = 0.0;
  long long trips = 0;
  hipError_t ensure(size_t n);
  ~RefineHost();
};
// Waves per SIMD pre_kernel / post_kernel / filter_refimage_kernel are built for (PMVS_PREPOST_WPE, default 3:
// pmvs_kernels.hip); their persistent grid is the scene grid x this / 2, and the per-workgroup global scratch is
// sized for it.
int prepost_waves();
// pre, the angle round trip, the refine kernel of resolve(layout, wsize, tau) (pmvs_refine_layouts.h), post
hipError_t launch_refine(const DScene& s, const pmvs_candidate* d_in, RefineJob* d_jobs, pmvs_refined* d_out, int n,
                         DevStats* d_st, int grid, int refine_grid, const RefineLayout& layout, hipStream_t stream,
                         hipEvent_t* ev, RefineHost& rh);
// split-form refine kernel alone (pmvs_refine_split.hip), wsize 5 or 7.  `cold`: the chains' cold optimizer
// state (bobyqa_dev.h BqCold), grown here to one slot per chain of a full grid; it carries nothing from
// one launch to the next
hipError_t launch_refine_split(const RefineLayout& l, const DScene& s, RefineJob* d_jobs, int n, DevStats* d_st,
                               hipStream_t stream, DevBuf<unsigned char>& cold);
// lane-form refine kernel alone (pmvs_refine_lane.hip): one candidate per wavefront, BOBYQA state spread
// over the lanes; a resolved layout (4 or 8 lanes per texture)
hipError_t launch_refine_lane(const RefineLayout& l, const DScene& s, RefineJob* d_jobs, int n, DevStats* d_st,
                              hipStream_t stream);
hipError_t launch_incc_eval(const DScene& s, const pmvs_eval_query* d_q, int n, double* d_out, DevStats* d_st,
                            hipStream_t stream);
hipError_t launch_grab_tex(const DScene& s, const pmvs_tex_query* d_q, int n, float* d_out, int* d_valid,
                           hipStream_t stream);
hipError_t launch_build_level(const uint8_t* d_src, int Wp, int Hp, uint8_t* d_dst, int W, int H, hipStream_t stream);
hipError_t launch_pack_rgba(const uint8_t* d_rgb, uint32_t* d_out, long long npix, hipStream_t stream);
hipError_t launch_unpack_rgba(const uint32_t* d_in, uint8_t* d_rgb, long long npix, hipStream_t stream);
hipError_t launch_math_selftest(int op, const double* d_in, double* d_out, int n, hipStream_t stream);
hipError_t launch_bobyqa_selftest(int mode, int kind, const double* d_x0, int n, int maxeval, double* d_out,
                                  hipStream_t stream);
hipError_t launch_model_digest(const void* recs, int n, int record_bytes, unsigned long long* d_out, hipStream_t stream);
hipError_t launch_patch_colors(const DScene& s, int n, const float* coords, const int* off, const int* images, int* out,
                               hipStream_t stream);

// ---- model export (pmvs_export.hip)
// Device pointers of the arrays of pmvs_export_buffers (include/pmvs_amd.h); null = not wanted.
struct ExportArrays {
  float* fields = nullptr;
  int* colors = nullptr;
  long long* image_off = nullptr;
  int *image_ids = nullptr, *image_idx = nullptr;
  long long* vimage_off = nullptr;
  int *vimage_ids = nullptr, *source = nullptr;
};
// d_tot[0] / d_tot[1] = the records' num_images / num_vimages summed (queued on st).
hipError_t export_sizes(const pmvs_patch* P, int n, unsigned long long* d_tot, hipStream_t st);
// The records P[0, n) as the arrays of `out`, rows in collectPatches(1) order (writer_order) or model
// order; max_gwidth = the widest target cell grid (sizes the sort key), d_tab = index2image on the
// device or null (identity).  Returns after the stream has finished the work; hipErrorOutOfMemory when
// its scratch cannot be allocated.
hipError_t export_pass(const DScene& s, const pmvs_patch* P, int n, bool writer_order, int max_gwidth, const int* d_tab,
                       const ExportArrays& out, hipStream_t st);
// The writer order alone: sorted[r] = the model index of row r in collectPatches(1) order (n device
// ints).  cnt_i / cnt_v (n device ints each, or null) receive the records' clamped list lengths.
// Returns after the stream has finished the work.
hipError_t export_order(const DScene& s, const pmvs_patch* P, int n, int max_gwidth, int* sorted, int* cnt_i, int* cnt_v,
                        hipStream_t st);

// ---- text files (pmvs_text.hip)
// The export's device arrays a text kind reads: fields always, colors for .ply, the lists for .patch.
struct TextArrays {
  const float* fields = nullptr;
  const int* colors = nullptr;
  const long long *image_off = nullptr, *vimage_off = nullptr;
  const int *image_ids = nullptr, *vimage_ids = nullptr;
};
// The byte offset of every row of the PMVS_TEXT_* `kind` file in d_off (n + 1 device entries: the first
// is header_bytes, the last the file's size).  Returns after the stream has finished the work.
hipError_t text_offsets(int kind, const TextArrays& in, int n, long long header_bytes, long long* d_off, hipStream_t st);
// Formats the n rows at their offsets in d_out (queued on the stream).
hipError_t text_write(int kind, const TextArrays& in, int n, const long long* d_off, char* d_out, hipStream_t st);
// pmvsfmt::fmt_g of n floats as a kernel: d_out n x 24 bytes, d_len n.
hipError_t launch_format_selftest(int precision, const float* d_in, int n, char* d_out, int* d_len, hipStream_t st);

// ---- per-target depth maps (pmvs_depthmap.hip)
// Device pointers of the arrays of pmvs_depthmap_buffers (include/pmvs_amd.h); null = not wanted.
struct DepthMapArrays {
  int* patch = nullptr;
  float *depth = nullptr, *normal = nullptr, *ncc = nullptr;
};
// setDepthMaps over the records P[0, n) in model order (src null) or with row r = record src[r]:
// d_off = the tnum + 1 cell offsets of the targets' maps on the device, cells = their total.  Returns
// after the stream has finished the work; hipErrorOutOfMemory when its scratch cannot be allocated.
hipError_t depth_map_pass(const DScene& s, const pmvs_patch* P, int n, const int* src, const long long* d_off,
                          long long cells, const DepthMapArrays& out, hipStream_t st);
// The rows' float4 arrays both map passes read instead of the 1608-byte records (queued on the stream):
// coordc[r] = the coordinate of row r (record src[r], or r when src is null) and, when attrc is not
// null, attrc[r] = (normal x, y, z, ncc).
hipError_t depth_map_pack(const pmvs_patch* P, const int* src, int n, float4* coordc, float4* attrc, hipStream_t st);

// ---- per-pixel maps (pmvs_pixmap.hip; the definition is csrc/pmvs_pixmap.h)
// The maps of targets [first, first + count) at `radius` over the records P[0, n) in model order (src
// null) or with row r = record src[r], into the arrays of `out` (device pointers, pixel offsets
// relative to target `first`).  Returns after the stream has finished the work; its scratch (32 bytes
// per row, 8 per pixel of one group of at most eight targets) is freed by then.
hipError_t pixel_map_pass(const DScene& s, const DView* hviews, const pmvs_patch* P, int n, const int* src, int first,
                          int count, int radius, const DepthMapArrays& out, hipStream_t st);

// ---- fusion of the per-pixel maps (pmvs_fuse.hip; the definition is csrc/pmvs_fuse.h)
// Device pointers of the arrays of pmvs_fuse_buffers (include/pmvs_amd.h); null = not wanted.
struct FuseArrays {
  unsigned char* support_map = nullptr;
  float *coord = nullptr, *normal = nullptr;
  unsigned char *color = nullptr, *support = nullptr;
  long long* pixel = nullptr;
  int* patch = nullptr;
};
// The fusion of targets [first, first + count) over the records P[0, n) (rows as pixel_map_pass takes
// them): the support map and the first min(*total, cap) points into `out`, *total = the points emitted.
// Returns after the stream has finished the work; its scratch (30 bytes per pixel of the range and the
// maps' own) is freed by then.
hipError_t fuse_pass(const DScene& s, const DView* hviews, const pmvs_patch* P, int n, const int* src, int first, int count,
                     const pmvs_fuse_params& prm, long long cap, const FuseArrays& out, long long* total, hipStream_t st);
// Fuse steps 1-4 alone, for the consumers of the maps and the pass flags (fuse_pass itself, the TSDF
// integration): the range's patch, depth and normal maps, the support map (into `support_map` when the
// caller has one, else into `support`) and one pass flag per pixel, with the pixel offset of every target.
// The work is enqueued on `st`, not waited for; `f` owns the arrays.
struct FuseMaps {
  DevBuf<int> patch;
  DevBuf<float> depth, normal;
  DevBuf<unsigned char> support, pass;
  DevBuf<long long> off;            // count + 1
  std::vector<long long> host_off;  // the same on the host
  unsigned char* support_map = nullptr;
  long long pixels = 0;
  unsigned row_blocks = 1;          // blocks of 256 pixels that cover the largest image
};
hipError_t fuse_maps_pass(const DScene& s, const DView* hviews, const pmvs_patch* P, int n, const int* src, int first, int count,
                          const pmvs_fuse_params& prm, unsigned char* support_map, FuseMaps& f, hipStream_t st);

// ---- meshing of the fused maps (pmvs_mesh.hip; the definition is csrc/pmvs_mesh.h)
// Device pointers of pmvs_tsdf_buffers / pmvs_mesh_buffers (include/pmvs_amd.h); null = not wanted.
struct TsdfArrays {
  float* tsdf = nullptr;
  unsigned char *obs = nullptr, *color = nullptr;
};
struct MeshArrays {
  float *vertex = nullptr, *normal = nullptr;
  unsigned char* color = nullptr;
  int* face = nullptr;
};
// The TSDF of `vol` integrated from the maps and pass flags `f` of targets [first, first + count), on `st`
// (not waited for).
hipError_t tsdf_integrate(const DScene& s, const FuseMaps& f, int first, int count, const pmvs_volume& vol, float trunc,
                          const TsdfArrays& out, hipStream_t st);
// Naive surface nets over the device volume arrays (color may be null): the first min(*nverts, vcap)
// vertices and min(*nfaces, fcap) faces into `out`.  Returns after the stream has finished the work; its
// scratch (5 bytes per cell, 9 per voxel) is freed by then.
hipError_t tsdf_mesh_pass(const pmvs_volume& vol, int min_obs, const float* tsdf, const unsigned char* obs,
                          const unsigned char* color, long long vcap, long long fcap, const MeshArrays& out, long long* nverts,
                          long long* nfaces, hipStream_t st);

// ---- the sparse volume of 8^3-voxel bricks (pmvs_brick.hip; the definition is csrc/pmvs_brick.h)
// The bricks the passing pixels of `f` select: one flag byte and one slot (the exclusive sums of the
// flags) per brick of the grid, and the selected count.  Returns after the stream has finished.
struct BrickSelection {
  DevBuf<unsigned char> flag;
  DevBuf<int> slot;
  long long bricks = 0, total = 0;  // of the grid, selected
};
hipError_t brick_select(const DScene& s, const FuseMaps& f, int first, int count, const pmvs_volume& vol, int margin,
                        BrickSelection& sel, hipStream_t st);
// The keys of the first `stored` selected bricks into key[0, stored), ascending; sel.slot becomes the
// brick -> slot map of those, -1 for every other brick of the grid.  Enqueued on `st`.
hipError_t brick_keys(BrickSelection& sel, long long stored, long long* key, hipStream_t st);
// The TSDF of the stored bricks key[0, stored): 512 values per brick and array.  Enqueued on `st`.
hipError_t brick_integrate(const DScene& s, const FuseMaps& f, int first, int count, const pmvs_volume& vol, float trunc,
                           const long long* key, long long stored, const TsdfArrays& out, hipStream_t st);
// The brick -> slot map of a caller's device key list; *ok = strictly ascending and inside the grid
// (checked by a kernel before anything is written through a key).
hipError_t brick_slots_from_keys(const pmvs_volume& vol, const long long* key, long long nb, DevBuf<int>& slot, bool* ok,
                                 hipStream_t st);
// tsdf_mesh_pass over the virtual volume of the stored bricks (arrays of nb x 512, color may be null).  With
// more than INT_MAX vertices it writes nothing and reports the counts.  Returns after the stream has
// finished; its scratch (per stored voxel: flags 2, offset 8, vertex id 4; per vertex and per quad the
// sort's 32 bytes and storage) is freed by then.
hipError_t brick_mesh_pass(const pmvs_volume& vol, int min_obs, long long nb, const long long* key, const int* slot, const float* tsdf,
                           const unsigned char* obs, const unsigned char* color, long long vcap, long long fcap, const MeshArrays& out,
                           long long* nverts, long long* nfaces, hipStream_t st);

// ---- the mesh rasterised into the targets and a view per face (pmvs_texmesh.hip; the definition is
// csrc/pmvs_texmesh.h)
// Device pointers of pmvs_raster_buffers / pmvs_texture_buffers (include/pmvs_amd.h); null = not wanted.
struct RasterArrays {
  int* face = nullptr;
  float* depth = nullptr;
};
struct TextureArrays {
  int* view = nullptr;
  float *uv = nullptr, *score = nullptr;
};
// *ok = every one of the 3 * nf device face ids lies in [0, nv) (a kernel's one flag, read back).
hipError_t mesh_ids_check(const int* face, long long nf, long long nv, bool* ok, hipStream_t st);
// The nearest face and its depth per pixel of targets [first, first + count) (pixel offsets relative to
// target `first`) of the device mesh, whose ids were checked.  Returns after the stream has finished the
// work; its scratch (8 bytes per pixel of one group of at most eight targets, 8 bytes per (face, target of
// the group) whose clipped box exceeds 64 pixels) is freed by then.
hipError_t mesh_raster_pass(const DScene& s, const DView* hviews, int first, int count, const float* vertex, long long nf,
                            const int* face, const RasterArrays& out, hipStream_t st);
// The best target of the range per face, with the same raster rendered group by group inside the call; also
// 8 bytes per face for the view and score the caller did not ask for.  nf < 1 writes nothing.
hipError_t mesh_texture_pass(const DScene& s, const DView* hviews, int first, int count, const pmvs_texture_params& prm,
                             const float* vertex, long long nf, const int* face, const TextureArrays& out, hipStream_t st);

// ---- the textured mesh baked into one atlas image (pmvs_atlas.hip; the definition is csrc/pmvs_atlas.h)
// Device pointers of pmvs_atlas_buffers (include/pmvs_amd.h); null = not wanted.
struct AtlasArrays {
  unsigned char* rgb = nullptr;
  int* texel_face = nullptr;
  float* uv = nullptr;
  int* atlas_view = nullptr;
};
// *ok = every one of the 3 * nf device face ids lies in [0, nv) and every one of the nf device views in
// [-1, tnum) (a kernel's one flag, read back).
hipError_t atlas_ids_check(const int* face, const int* view, long long nf, long long nv, int tnum, bool* ok, hipStream_t st);
// The classes of a call's faces, between its two steps; owns the per-face scratch (10 bytes per face and
// the sort's temporary storage).
struct AtlasWork {
  DevBuf<unsigned char> cls, cls_sorted;
  DevBuf<int> ids, order;
};
// Step 1-2: the class byte of every face (0 = not placed) and the faces per class in counts[0, 252).
// Returns after the stream has finished the work.
hipError_t atlas_classify(const DScene& s, const pmvs_atlas_params& prm, const float* vertex, long long nf, const int* face,
                          const int* view, AtlasWork& w, long long* counts, hipStream_t st);
// Steps 3-7 for the layout those counts give (band_y[n] = the first row of class n, H = the atlas height):
// uv and atlas_view of every face and the first `rows` rows of the two images.  Returns after the stream
// has finished the work.
hipError_t atlas_render_pass(const DScene& s, const pmvs_atlas_params& prm, const float* vertex, long long nf, const int* face,
                             const int* view, AtlasWork& w, const long long* counts, const long long* band_y, long long rows,
                             const AtlasArrays& out, hipStream_t st);

// ---- filter pass (pmvs_filter.hip)
// The fields of a patch that neighbour and visibility tests read from OTHER patches (isNeighbor,
// computeGain, isVisible), one 64-B line per patch instead of 2-3 lines of its 1.6-KB record;
// rebuilt by every collect and written by the expansion's commit (coord / normal / dscale / ncc
// never change after a patch is created; unit0 = getUnit(images[0], coord) follows setRefImage).
struct alignas(64) PHot {
  float coord[4];
  float normal[4];
  float dscale, ncc, unit0, pad[5];
};
// Buffers sized by reserve() share the logical capacities cap_n / cap_cells / cap_grid / cap_e; the
// others grow on demand and their DevBuf holds their capacity.
struct FilterBuffers {
  PinnedBuf pin;  // host staging of the small-groups BFS inputs
  DevBuf<Reg> preg, vreg, safe;  // per patch: registered / filterExact-safe list entries
  DevBuf<unsigned long long> keys, keys2, dpkey;
  DevBuf<long long> tgoff;
  DevBuf<int> cnt, off, cellcnt, pg_off, pg_items, vp_off, vp_items, order, rank, flags, need, list, counters, edge_off,
      edges;
  DevBuf<PHot> hot;
  DevBuf<double> scratch;
  DevBuf<char> temp;        // hipcub temp storage, sized by reserve / ensure_entries for every sort and scan here
  DevBuf<unsigned> rbits;   // sharded filterNeighbor: packed reject flags
  DevBuf<float4> coordc;    // collected patches' coordinates in collect order (depth maps)
  // setVImagesVGrids' visibility rows (target-major bits), the collected patches' normals and used
  // targets; owner-partitioned pass (world > 1): setRefImage outcomes and the all-gathered payloads
  DevBuf<unsigned long long> vrows, used;
  DevBuf<float4> normalc;
  DevBuf<int> refpos;
  DevBuf<int> lparent;  // filterSmallGroups: the union-find parents, then the supernodes' labels (label_stage)
  DevBuf<char> xr;
  // filterNeighbor's deferred quadric fits (pmvs_filter.hip QuadJobs)
  DevBuf<float> qf;
  DevBuf<double> qrows;
  DevBuf<int4> qjobs;
  DevBuf<unsigned long long> qctr;  // [0] rows used, [1] low 32 bits: jobs, [2] low 32 bits: quad_split_kernel's kb
  DevBuf<unsigned long long> qkeys, qkeys2;  // jobs by descending row count
  DevBuf<int> qcrows, qoff;                  // per 64-job chunk: pool rows, offsets
  size_t cap_qrows = 0;  // rows of qf (qrows holds 64 x NB_CAP more)
  // the neighbour walks' NB_CAP_BIG re-walks (pmvs_filter.hip NbOverflow): overflowed work items
  // and the big form's global scratch
  DevBuf<int> ovf_items;
  DevBuf<double> scratch_big;
  int cap_n = 0, cap_grid = 0;
  long long cap_cells = 0;
  size_t cap_e = 0;  // entries keys / keys2 are sized for (pg_items, vp_items: grown to their lists' size)
  hipError_t reserve(int n, long long ncells, int tnum, int grid);
  hipError_t ensure_entries(size_t e, int vis);
  void release() { *this = FilterBuffers(); }  // frees every buffer; the next pass reserves again (PMVS_LOOP_LEAN)
};

// setRefImage + setGrids for the patches list[0, m) (filterExact); with refpos, only the entries whose
// reference image rank owns (of world) are evaluated, their outcomes written to refpos (see the kernel)
hipError_t launch_filter_refimage(const DScene& s, pmvs_patch* P, const int* list, int m, int grid, hipStream_t stream,
                                  int* refpos = nullptr, int rank = 0, int world = 1);
hipError_t launch_apply_refpos(const DScene& s, pmvs_patch* P, const int* list, int m, const int* allpos, int world,
                               hipStream_t stream);

// ---- expansion run (pmvs_filter.hip)
constexpr int kMaxWave = 65536;  // parents per expansion wave (device slot arrays are sized by it)
struct CommitWork;  // device commit scratch (pmvs_filter.hip)
struct CommitWorkDelete {
  void operator()(CommitWork* w) const;
};
// Pinned staging of the per-wave host -> device index lists, with the event of its last copy
// (recorded on the scene's stream; owned by the scene, so never waited on after that stream is gone)
struct H2DStage {
  PinnedBuf pin;
  hipEvent_t done = nullptr;
  bool pending = false;
  H2DStage() = default;
  H2DStage(H2DStage&& o) noexcept : pin(std::move(o.pin)), done(o.done), pending(o.pending) { o.done = nullptr; }
  H2DStage& operator=(H2DStage&& o) noexcept {  // o leaves with the old buffer and event and frees them
    pin = std::move(o.pin);
    std::swap(done, o.done);
    std::swap(pending, o.pending);
    return *this;
  }
  ~H2DStage() {
    if (done) (void)hipEventDestroy(done);
  }
};
// The expansion's logical capacity overflows (more than NB_CAP_BIG neighbours, a list past
// PMVS_MAX_IMAGES, the model cap) return this code, so the API tells them from a device allocation
// that failed (hipErrorOutOfMemory: PMVS_ENOMEM).
constexpr hipError_t kCapacityOverflow = hipErrorNotSupported;

// Every buffer grows on demand to what a wave needs (exactly; the three the chunks of a wave append
// to, parents / cand_coord / cand_ok, and the entry pool d_ent keep their contents).
struct ExpandBuffers {
  std::unique_ptr<CommitWork, CommitWorkDelete> cm;
  long long ncells = 0;  // target cells of the pass (the commit sorts only the cell bits of its keys)
  // (the initial queue run is built on the device: qkeep / qpos / qitems)
  H2DStage h2d;
  DevBuf<unsigned char> occ;  // per target cell: pgrids holds a patch (device commit)
  DevBuf<int> parents, cand_ok, status, slots, ostatus, alive;
  DevBuf<float> cand_coord;
  DevBuf<pmvs_candidate> cand, cand2;
  DevBuf<pmvs_patch> prep, prep2, outp;
  DevBuf<pmvs_refined> res;
  DevBuf<unsigned char> counts;
  // registrations committed during the run: per-cell chain heads + entry pool (FilterDev delta)
  // d_ent: the pool, {item, next} per entry (one 8-B load per chain step; round 6, separate item / next
  // arrays made every step touch two cache lines)
  DevBuf<int> pg_head, vp_head;
  DevBuf<int2> d_ent;
  DevBuf<float> qtmp;         // _tmp of the collected patches (queue)
  DevBuf<float> qkey;         // the initial queue sorted on the device: keys, collect ranks, temp
  DevBuf<int> qrank, qrank2;
  DevBuf<int> qkeep, qpos;    // the initial run built on the device (queue_items_kernel)
  DevBuf<int> sflag, spos, slot2;  // survivor compaction (surv_*_kernel)
  DevBuf<char> qitems;
  DevBuf<char> qsort_tmp;     // hipcub temp storage of the expansion's sorts and scans
  DevBuf<char> xsd, xrd;      // device payload of the sharded exchange (send, all ranks)
  DevBuf<int> cidx;           // wave slot -> compact index of its free direction (candidate / prep records)
  DevBuf<int> crec, acc;      // commit records; committed record indexes
  DevBuf<int2> dupd;          // (parent, failed-direction bits) of a wave
  size_t pool_host = 0;
  std::vector<int> gw, gh;  // grid sizes of the target images
  void release() { *this = ExpandBuffers(); }  // frees every buffer; the next pass grows them again (PMVS_LOOP_LEAN)
};
using RefineFn = std::function<hipError_t(const pmvs_candidate* d_in, int n, pmvs_refined* d_out)>;
// All-gather of `bytes` per rank into recv (world * bytes, rank order); 0 = OK.
using ExchangeFn = std::function<int(const void* send, size_t bytes, void* recv)>;
// Device all-gather on the given stream (RCCL); empty = the payload goes through `exchange`.
using ExchangeDevFn = std::function<int(const void* dsend, size_t bytes, void* drecv, hipStream_t st)>;
struct Shard {
  int rank = 0, world = 1;
  ExchangeFn exchange;
  ExchangeDevFn exchange_dev;
};
// dP[0, n0): the device-resident model (grown in place, contents kept); d_alive[0, n0) marks the
// patches the organizer holds; cap bounds the result size *n_out.
// One CFilter::run pass on the device model; sharded (sh->world > 1) filterNeighbor runs on the
// patches this rank owns and the flags are all-gathered (one exchange per pass).
hipError_t filter_pass(const DScene& s, FilterBuffers& B, pmvs_patch* dP, int n, long long ncells, const long long* h_tgoff,
                       int grid, hipStream_t st, int counts[4], int* overflow, int* keep_dev, const Shard* sh = nullptr,
                       bool* handled = nullptr);
hipError_t expand_pass(const DScene& s, FilterBuffers& B, ExpandBuffers& X, pmvs_patch*& dP, size_t& dP_cap, int n0,
                       const int* d_alive, int cap, long long ncells, const long long* h_tgoff, int wave, int cthr,
                       int flags, int grid, hipStream_t st, const RefineFn& refine, const Shard& sh, long long stats[8],
                       int* n_out, int min_cands = 0);
// dst_for(kept, &dst) supplies the target once the number of kept records is known
using CompactDst = std::function<hipError_t(int, pmvs_patch**)>;
hipError_t compact_model(FilterBuffers& B, const pmvs_patch* src, int n, const int* keep, const CompactDst& dst_for,
                         int* nkept, hipStream_t st);
hipError_t fill_int(int* a, int n, int v, hipStream_t st);
// filterSmallGroups' label stage, as filter_pass runs it, on a host CSR graph of n vertices (edges in
// [0, n)): h_lab[j] = the smallest vertex from which j is reachable; stats = supernodes, residual
// vertices, sweeps.
hipError_t labels_selftest(const int* h_eoff, const int* h_edges, int n, int* h_lab, int stats[3]);
// frees the device-to-host staging buffers of a scene's stream (pmvs_scene_destroy)
void d2h_stage_release(hipStream_t st);

// ---- CMVS cluster boundary exchange (pmvs_scene_set_cluster)
struct ClusterMaps {              // device tables of one cluster scene
  const unsigned char* shared_t;  // per local target index: its image is a target of another cluster too
  const int* ids;                 // per local view index: the global image number
  const int* id2idx;              // global image number (0 .. maxid) -> local view index, or -1
  int maxid;
};
struct ClusterBuffers {
  DevBuf<BRec> send, recv;
  DevBuf<pmvs_patch> ins;
  DevBuf<int> flags, pos, cnts;
  DevBuf<char> temp;  // hipcub temp storage
};
// The model without other clusters' boundary patches (fix != PMVS_FIX_FOREIGN), compacted into dst.
hipError_t drop_foreign(FilterBuffers& B, const pmvs_patch* src, int n, const CompactDst& dst_for, int* n_out,
                        hipStream_t st);
// One boundary exchange: src[0, n) is this rank's model without foreign patches.  Its boundary
// patches (registered in a target image another cluster also has as a target) are all-gathered
// (header {error, count} first, the "visibility counts"; then the records), and every other rank's
// records whose reference image is one of this scene's views and that project into one of its
// targets are appended to dst (= src's contents + the inserted patches; grown as needed) as fixed,
// never-expanded patches (fix = PMVS_FIX_FOREIGN), with grids from CPatchOrganizerS::setGrids.
// xstats: [0] own boundary patches, [1] records received, [2] inserted.  agreed: the failure (if
// any) was seen by every rank.
hipError_t cluster_exchange(const DScene& s, ClusterBuffers& CB, const ClusterMaps& cm, const pmvs_patch* src, int n,
                            pmvs_patch*& dst, size_t& dst_cap, int* n_out, const Shard& sh, hipStream_t st,
                            long long xstats[3], bool& agreed);
hipError_t lls_selftest(const float* A, const float* b, const int* off, int nsys, int total, float* x);

// ---- seed phase (pmvs_seed.hip)
struct SeedInput {
  const pmvs_point* points;  // every view's feature points, view 0 first
  const int* npts;           // per view
  const int* vis_off;        // visdata2 CSR (host)
  const int* vis;
  int sequence;
  float angle0;              // _angleThreshold0
  std::vector<const uint8_t*> mask_level;  // per view: binary mask at the scene level (host), or null
  int batch, per_cell;       // speculative refine batch size / unknown candidates requested per cell
  int lookahead;             // images (current + next) the speculation may request candidates of
  int spec_near;             // cells from the replay cursor every speculation walk re-visits
};
struct SeedOutput {
  std::vector<pmvs_patch> seeds;  // addPatch order
  long long stats[8];             // trial, pass, fail0, fail1, refined, rounds, candidates
  double gen_ms = 0, refine_ms = 0, wall_ms = 0;
};
hipError_t seed_pass(const DScene& s, const std::vector<DView>& hv, const SeedInput& in, hipStream_t st,
                     const RefineFn& refine, SeedOutput& out);
}  // namespace pmvsdev
