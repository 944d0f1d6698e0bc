/*
 * pmvs_amd.h -- C-ABI of the MI355X-native PMVS2 dense-matching core.
 *
 * The reference (robjermy/CMVS-PMVS) has no plugin/FFI surface for its hot path: the stages
 * share one CFindMatch& (reference include/pmvs/findMatch.hpp:150-163).  This ABI is the
 * boundary SURVEY.md §8(b) defines; each entry point names the reference interface it
 * replaces.  Plain pointers and sizes only; no exceptions cross it; errors are status codes
 * with a message from pmvs_last_error().  Never calls exit().
 *
 * Index convention: every image number below is an *index* into the scene's view list
 * (targets first, then other images), exactly like the reference's internal _images
 * (CPatchOrganizerS::image2index / index2image, patchOrganizerS.cpp:16-52).
 *
 * Ownership: all input/output arrays belong to the caller (host memory); a scene owns its
 * device memory.  Threading: calls on one scene are serialised on that scene's HIP stream;
 * different scenes (one per GPU) may be driven from different host threads.
 */
#ifndef PMVS_AMD_H
#define PMVS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Capacity of one patch's image list and of its visible-target list (reference: unbounded
 * std::vector, patch.hpp:38,42).  A patch's images are distinct views and its vimages distinct
 * targets, so both lists always fit for scenes of up to PMVS_MAX_IMAGES views; larger scenes are
 * supported, and a list that would overflow fails the call with PMVS_EUNSUPPORTED (never a clamp). */
#define PMVS_MAX_IMAGES 128
#define PMVS_MAX_TARGETS 256 /* target images (timages) per scene: a C5 cluster is maximage 70 plus overlap */
#define PMVS_MAX_TAU 16    /* max textures in the objective: tau = min(2*minImageNum, num) */
#define PMVS_MAX_LEVEL 4   /* reference MyPow2 table limits level to <= 4 (optim.cpp:808-811) */
/* Unique neighbours one findNeighbors walk may hold (filterNeighbor, findEmptyBlocks, the depth >= 2
 * check; reference: unbounded std::vector).  Walks past 1024 are redone with a 16384-entry form;
 * beyond this the call fails with PMVS_EUNSUPPORTED. */
#define PMVS_MAX_NEIGHBOURS 16384

typedef enum pmvs_status {
  PMVS_OK = 0,
  PMVS_EINVAL = 1,      /* invalid argument */
  PMVS_EDEVICE = 2,     /* HIP runtime error */
  PMVS_ENOMEM = 3,      /* allocation failure */
  PMVS_EUNSUPPORTED = 4 /* configuration outside the supported envelope */
} pmvs_status;

/* Outcome of one candidate in pmvs_refine_batch (CSeed::initialMatchSub seed.cpp:387-414,
 * CExpand::expandSub expand.cpp:225-237: preProcess -> refinePatch -> postProcess). */
typedef enum pmvs_candidate_status {
  PMVS_ACCEPTED = 0,      /* postProcess returned 0 */
  PMVS_FAIL_PRE = 1,      /* COptim::preProcess returned 1 */
  PMVS_FAIL_POST = 2,     /* COptim::postProcess returned 1 */
  PMVS_FAIL_OVERFLOW = 3  /* image list exceeded PMVS_MAX_IMAGES (not a reference outcome; the loop entry
                             points turn it into a PMVS_EUNSUPPORTED error) */
} pmvs_candidate_status;

/* One view: CPhoto = CImage (pyramid) + CCamera (projection), reference include/image/photo.hpp. */
typedef struct pmvs_view_desc {
  int32_t width, height;    /* level-0 size */
  const uint8_t* rgb;       /* width*height*3 interleaved RGB8, row-major (CImage::_images[0]) */
  const uint8_t* mask;      /* optional width*height, 0 = outside; NULL = no mask */
  const uint8_t* edge;      /* optional width*height; NULL = no edge map */
  float projection[12];     /* level-0 3x4 projection, row-major (txt/%08d.txt, CCamera::init) */
} pmvs_view_desc;

/* Scene: SOption (option.cpp:10-28,30-158) + CFindMatch::init (findMatch.cpp:30-107). */
typedef struct pmvs_scene_desc {
  int32_t num_views;          /* _num = |timages| + |oimages| */
  int32_t num_targets;        /* _tnum = |timages| */
  int32_t level;              /* option level (0..PMVS_MAX_LEVEL) */
  int32_t csize;              /* option csize */
  int32_t wsize;              /* option wsize (odd) */
  int32_t min_image_num;      /* option minImageNum */
  float threshold;            /* option threshold (initial _nccThreshold) */
  float max_angle;            /* SOption::_maxAngleThreshold in radians (maxAngle * M_PI/180) */
  float quad_threshold;       /* option quad */
  int32_t sequence;           /* option sequence (-1 = off) */
  const int32_t* visdata2_offsets; /* CSR row starts, num_views+1 entries (SOption::_visdata2) */
  const int32_t* visdata2;         /* CSR column indexes */
  int32_t num_bindexes;            /* SOption::_bindexes (useBound) */
  const int32_t* bindexes;
  const pmvs_view_desc* views;     /* num_views entries */
} pmvs_scene_desc;

/* A patch candidate before preProcess (Patch::CPatch, reference include/pmvs/patch.hpp:10-77). */
typedef struct pmvs_candidate {
  float coord[4];  /* _coord, w = 1 */
  float normal[4]; /* _normal, w = 0 */
  float dscale;    /* initial _dscale (0 for a freshly constructed CPatch) */
  int32_t num_images;
  int32_t images[PMVS_MAX_IMAGES]; /* _images (indexes); [0] is the reference image */
} pmvs_candidate;

/* A candidate after preProcess -> refinePatch -> postProcess. */
typedef struct pmvs_refined {
  int32_t status;      /* pmvs_candidate_status */
  int32_t refine_code; /* optimizer result, NLopt numbering (4 = XTOL_REACHED, 5 = MAXEVAL, -4 = ROUNDOFF) */
  int32_t evals;       /* objective evaluations (COptim::my_f calls) in refinePatch */
  int32_t num_images;
  float coord[4];
  float normal[4];
  float ncc;           /* _ncc (stays -1 if refinement failed, as in the reference) */
  float dscale;
  float ascale;
  float tmp;           /* _tmp = score2(nccThreshold) */
  int32_t timages;
  int32_t reserved;
  int32_t images[PMVS_MAX_IMAGES];
  int32_t grids[PMVS_MAX_IMAGES][2]; /* _grids (cell x, cell y) per image */
} pmvs_refined;

/* Objective query: the refine state of refinePatchBFGS (optim.cpp:580-599) for a patch, and
 * an optimizer point x at which COptim::my_f (optim.cpp:507-578) is evaluated. */
typedef struct pmvs_eval_query {
  float coord[4];
  float normal[4];
  float dscale;
  int32_t num_images;
  int32_t images[PMVS_MAX_TAU]; /* first min(tau, num_images) are used */
  double x[3];
} pmvs_eval_query;

/* One texture grab: COptim::grabTex (optim.cpp:815-863) followed by COptim::normalize
 * (optim.cpp:1031-1067) when valid. */
typedef struct pmvs_tex_query {
  float coord[4];
  float pxaxis[4];
  float pyaxis[4];
  float normal[4];
  int32_t view;
  int32_t normalize; /* 1 = apply normalize() to a valid texture */
} pmvs_tex_query;

typedef struct pmvs_stats {
  int64_t candidates;
  int64_t accepted;
  int64_t fail_pre;
  int64_t fail_post;
  int64_t refine_failed;  /* optimizer result not in {SUCCESS, STOPVAL, FTOL, XTOL} */
  int64_t evals;          /* my_f evaluations inside refinePatch */
  int64_t tex_valid;      /* sum over those evaluations of valid textures (algorithmic bytes = 588*this for wsize 7) */
  int64_t tex_grabs;      /* every grabTex executed (incl. pre/post-processing) */
  double kernel_ms;       /* device time of the last call's kernels (HIP events on the scene stream) */
  /* refine-kernel phase profile (diagnostics; summed over wavefronts, shader clock cycles) */
  int64_t opt_cycles;       /* BOBYQA steps, refill and request publication */
  int64_t objective_cycles; /* cooperative my_f / computeINCC evaluation */
  int64_t rounds;           /* optimizer rounds (all lanes step once) */
  int64_t chunks;           /* cooperative objective chunks */
  int64_t prof[8];          /* cycles: refill, optimizer step, publish, chunk setup, gather, normalize, dot, reduce */
  double pre_ms, refine_ms, post_ms; /* per-kernel device time of the last refine batch (HIP events) */
} pmvs_stats;

typedef struct pmvs_scene pmvs_scene;

/* Last error message of the calling thread (never NULL). */
const char* pmvs_last_error(void);

/* Number of visible HIP devices (0 if none). */
int32_t pmvs_device_count(void);

/* Replaces CFindMatch::init's image/camera setup (findMatch.cpp:30-107): CPhotoSetS::init
 * (photoSetS.cpp:12-80) + CImage::buildImage pyramids (image.cpp:228-325, built ON DEVICE),
 * CCamera::updateCamera (camera.cpp:109-138), COptim::setAxesScales (optim.cpp:43-64) and the
 * threshold defaults (findMatch.cpp:92-106).  Copies everything to device `device`. */
pmvs_status pmvs_scene_create(const pmvs_scene_desc* desc, int32_t device, pmvs_scene** out);

void pmvs_scene_destroy(pmvs_scene* scene);

/* CFindMatch::updateThreshold semantics (findMatch.cpp:23-28) made explicit, plus _depth. */
pmvs_status pmvs_set_thresholds(pmvs_scene* scene, float ncc, float ncc_before, int32_t depth);

/* Read back one pyramid level of one view (parity of CImage::buildImage). */
pmvs_status pmvs_scene_get_level(pmvs_scene* scene, int32_t view, int32_t level, uint8_t* out,
                                 int32_t* width, int32_t* height);

/* A feature point (PMVS3::CPoint, point.hpp): image coordinates at the option level, detector
 * response, type 0 = Harris, 1 = DoG. */
typedef struct pmvs_point {
  float x, y, response;
  int32_t type;
} pmvs_point;

/* PMVS3::CDetectFeatures::run for one view (detectFeatures.cpp:47-124; the caller is
 * CFindMatch::init, findMatch.cpp:79-82 with fcsize 16): CHarris (sigma 4) then
 * CDifferenceOfGaussians (scales 1..3) on the view's pyramid at the scene level with its mask and
 * edge images, at most 4 points per 2*fcsize block, computed on the device.  Points come in the
 * reference's order: Harris points by decreasing response, then DoG points by decreasing response
 * (each detector's std::multiset read from its end).  *n_out = the number of points; at most cap
 * are written (call with cap = 0 to size the array). */
pmvs_status pmvs_detect_features(pmvs_scene* scene, int32_t view, int32_t fcsize, pmvs_point* out, int32_t cap,
                                 int32_t* n_out);

/* Batched COptim::grabTex + normalize: out_tex is n * 3*wsize*wsize floats, out_valid n ints
 * (1 = texture grabbed, 0 = grabTex returned 1 / empty texture). */
pmvs_status pmvs_grab_tex(pmvs_scene* scene, const pmvs_tex_query* q, int32_t n, float* out_tex,
                          int32_t* out_valid);

/* Batched COptim::my_f: out_f[i] = my_f(q[i].x) after the refinePatchBFGS setup of q[i]. */
pmvs_status pmvs_incc_eval(pmvs_scene* scene, const pmvs_eval_query* q, int32_t n, double* out_f,
                           pmvs_stats* stats);

/* Batched preProcess -> refinePatch -> postProcess (optim.cpp:95-190, 496-658) for n candidates
 * at the scene's current thresholds, as the seed phase calls them (CSeed at _depth 0,
 * findMatch.cpp:187-194; seed.cpp:385-395).  The expansion's calls (expand.cpp:225-237, _depth >= 1)
 * also run postProcess's organizer steps (setVImagesVGrids, check(); optim.cpp:178-188) against the
 * model, so they run inside pmvs_expand_run / pmvs_run_loop, where the organizer lives on the
 * device; this call returns PMVS_EUNSUPPORTED when the scene's depth is >= 1. */
pmvs_status pmvs_refine_batch(pmvs_scene* scene, const pmvs_candidate* in, int32_t n,
                              pmvs_refined* out, pmvs_stats* stats);

/* Device-resident variant for benchmarking: candidates/results already on the device
 * (pointers from hipMalloc / torch).  Runs on the scene stream and waits once mid-call (after
 * preProcess, for the start points' angles, which the host's libm computes as the reference's
 * encode does); returns with the refine and postProcess kernels queued: call pmvs_scene_sync()
 * and read stats afterwards. */
pmvs_status pmvs_refine_batch_device(pmvs_scene* scene, const pmvs_candidate* d_in, int32_t n,
                                     pmvs_refined* d_out);
pmvs_status pmvs_scene_sync(pmvs_scene* scene, pmvs_stats* stats);


/* Self-test: evaluates the device libm function `op` (0 sqrt, 1 sin, 2 cos, 3 asin, 4 acos,
 * 5 atan, 6 log, 7 f32 sqrt, 8 f32 divide in[i]/in[i+1], 9 floor) on n doubles. */
pmvs_status pmvs_selftest_math(int32_t device, int32_t op, const double* in, double* out, int32_t n);

/* Self-test: the device Cmylapack::lls (filterQuad's least squares, Eigen JacobiSVD semantics) on
 * nsys n_k x 5 systems: rows offsets[k] .. offsets[k+1]-1 of A (5 floats per row) and b; x: 5 floats
 * per system. */
pmvs_status pmvs_selftest_lls(int32_t device, const float* A, const float* b, const int32_t* offsets, int32_t nsys,
                              float* x);

/* Self-test: device BOBYQA on analytic objective `kind` (0 quadratic, 1 Rosenbrock-3, 2 bound
 * active) from n start points x0 (3 doubles each).  mode 0 = one problem per lane, 1 = one per
 * wavefront.  out: 6 doubles per problem (x[3], minf, nevals, result code); *ms kernel time. */
pmvs_status pmvs_selftest_bobyqa(int32_t device, int32_t mode, int32_t kind, const double* x0, int32_t n,
                                 int32_t maxeval, double* out, double* ms);

/* ---------------------------------------------------------------------------------------
 * Filter pass over a patch set (PMVS3::CFilter::run, filter.cpp:13-27): the cell organizer
 * (CPatchOrganizerS pgrids / vpgrids / depth maps) is built on the device from the patch
 * array; insertion order = array index.  Runs at the scene's thresholds and depth
 * (pmvs_set_thresholds; the reference runs filters at depth >= 1).
 * The model record (CPatch, patch.hpp:10-77) keeps its lists as 16-bit view indexes and 16-bit
 * cell coordinates (scenes of < 32768 views, cell grids < 32768 wide and high: checked by
 * pmvs_scene_create), so 128-entry lists cost the bytes 64 32-bit entries did. */
typedef struct pmvs_patch {
  float coord[4], normal[4];
  float ncc, dscale, ascale, tmp;
  int32_t timages, flag, fix, num_images, num_vimages, dflag; /* dflag: CPatch::_dflag (failed expansion directions) */
  int16_t images[PMVS_MAX_IMAGES];
  int16_t grids[PMVS_MAX_IMAGES][2];
  int16_t vimages[PMVS_MAX_IMAGES];
  int16_t vgrids[PMVS_MAX_IMAGES][2];
} pmvs_patch;

/* pmvs_patch.fix: 0 = a patch of this scene, 1 = fixed (CPatch::_fix, patchOrganizerS.cpp:175-197: never
 * filtered), PMVS_FIX_FOREIGN = another cluster's boundary patch inserted by the cluster exchange
 * (pmvs_scene_set_cluster): fixed, and never expanded or returned by this scene. */
#define PMVS_FIX_FOREIGN 2

typedef struct pmvs_filter_stats {
  int64_t input, removed_outside, removed_exact, removed_neighbor, removed_groups, kept;
  double kernel_ms;
} pmvs_filter_stats;

/* patches are updated in place (images/grids/timages/vimages/vgrids as the reference leaves
 * them); keep[i] = 1 when patch i is still in the organizer (the model) after the pass. */
pmvs_status pmvs_filter_run(pmvs_scene* scene, pmvs_patch* patches, int32_t n, int32_t* keep,
                            pmvs_filter_stats* stats);

/* One expansion run (PMVS3::CExpand::run, expand.cpp:17-406) on a model = patches[i] with
 * alive[i] (the state a filter pass leaves: pgrids/vpgrids/depth maps are rebuilt from it).  The
 * max-_tmp queue is expanded in waves of `wave` parents (1 = the reference's single-thread
 * schedule), candidates are refined with preProcess -> refinePatch ->
 * postProcess including the depth >= 1 steps (setVImagesVGrids; check() at depth >= 2) and
 * committed in (parent priority, direction) order; with min_candidates > 0 (and wave > 1) a wave
 * takes further chunks of `wave` parents until its parents have that many free directions
 * (findEmptyBlocks against the start-of-wave model).  count_threshold = _countThreshold1 (4 at the
 * first expansion, 2 after updateThreshold).  The result is the old patches (with updated
 * _flag/_dflag) followed by the new ones, at most `cap` in all; *n_out is their number.
 * out/alive_out receive it when non-NULL; with out == alive_out == NULL the scene keeps it and
 * pmvs_expand_fetch copies it out (so the caller can size its arrays after the run).
 * With a shard set (pmvs_scene_set_shard) the call is collective: every rank passes the same
 * model and arguments and gets the same result. */
#define PMVS_EXPAND_AFTER_SEEDS 1 /* model straight from the seed phase: no depth maps yet (findMatch.cpp:193-202) */
/* flags bits 8..31: stop after that many waves (0 = run until the queue is empty).  Not a reference
 * behaviour: it bounds full-size parity samples against the CPU oracle, which has the same bound. */
#define PMVS_EXPAND_MAX_WAVES(n) ((int32_t)((uint32_t)(n) << 8))
typedef struct pmvs_expand_stats {
  int64_t parents, candidates, fail_prep, fail_pre, fail_post, fail_commit, added, waves;
  double wall_ms;
  /* this rank's refine work (preProcess -> refinePatch -> postProcess of its candidate share):
   * candidates refined, my_f + computeINCC evaluations, valid textures over them, summed
   * refine-kernel time (HIP events) */
  int64_t refined, evals, tex_valid;
  double refine_ms;
  int64_t refine_launches;
  /* the part of tex_valid / refine_ms / refine_launches that ran the small-batch refine layout
   * (batches below the scene's small-batch size: the workgroup-form kernel) */
  int64_t tex_valid_small;
  double refine_ms_small;
  int64_t refine_launches_small;
} pmvs_expand_stats;
pmvs_status pmvs_expand_run(pmvs_scene* scene, const pmvs_patch* patches, const int32_t* alive, int32_t n,
                            int32_t wave, int32_t min_candidates, int32_t count_threshold, int32_t flags, pmvs_patch* out, int32_t* alive_out,
                            int32_t cap, int32_t* n_out, pmvs_expand_stats* stats);
/* Copies the result the last pmvs_expand_run kept (out == NULL) and releases it; n = *n_out. */
pmvs_status pmvs_expand_fetch(pmvs_scene* scene, pmvs_patch* out, int32_t* alive_out, int32_t n);

/* The dense-matching loop after the seed phase, PMVS3::CFindMatch::run (findMatch.cpp:196-217):
 * `iterations` x (CExpand::run, CFilter::run, updateThreshold) from the seed patches, with the
 * model resident in HBM between the passes (only the final model crosses PCIe).  Thresholds as
 * the reference: depth 1 upwards, ncc = threshold and before = threshold - 0.3f, both -= 0.05f
 * and _countThreshold1 4 -> 2 after each iteration (findMatch.cpp:23-28, 104).  flags:
 * PMVS_EXPAND_AFTER_SEEDS for the first expansion; PMVS_EXPAND_MAX_WAVES(n) bounds every
 * iteration's expansion to n waves (not a reference behaviour: full-size parity samples of the
 * whole loop against the CPU oracle, which has the same bound).  cap bounds the model size.  *n_out = the final
 * model's size; pmvs_loop_fetch copies it out.  iters (may be NULL) receives per-iteration stats.
 * Collective when a shard is set. */
typedef struct pmvs_loop_iter {
  int32_t depth, patches; /* patches kept after the filter pass */
  pmvs_expand_stats expand;
  pmvs_filter_stats filter;
  /* cluster exchange after this iteration (pmvs_scene_set_cluster; 0 otherwise): this rank's boundary
   * patches sent, the other ranks' records received, the records inserted as foreign patches */
  int64_t boundary_sent, boundary_received, boundary_inserted;
} pmvs_loop_iter;
pmvs_status pmvs_run_loop(pmvs_scene* scene, const pmvs_patch* seeds, int32_t n, float threshold, int32_t iterations,
                          int32_t wave, int32_t min_candidates, int32_t flags, int32_t cap, int32_t* n_out, pmvs_loop_iter* iters);
pmvs_status pmvs_loop_fetch(pmvs_scene* scene, pmvs_patch* out, int32_t n);
/* (new) A 64-bit digest of pmvs_run_loop's result while it is still on the device (no PCIe
 * transfer): every record's bytes mixed with its position, so equal models give equal digests
 * (identical-repetition checks of a device-resident pipeline).  pmvs_loop_fetch still works after it. */
pmvs_status pmvs_loop_hash(pmvs_scene* scene, uint64_t* hash);

/* The model as the compact arrays the writers (pmvs_write_ply / _patches / _pset) and a downstream
 * GPU stage read, produced on the device from the records where they lie: about 76 bytes per patch
 * plus 4 per list entry of each list array cross PCIe instead of the 1608-byte record (and nothing in
 * device mode).  Replaces CPatchOrganizerS::collectPatches(1) (patchOrganizerS.cpp:207-236: target images in
 * order, their cells in raster order, each cell's list in insertion = model order, every patch at its
 * first registration), the field and list gathers of writePatches2 (patchOrganizerS.cpp:89-132) and
 * writePLY's colour mode 0 (patchOrganizerS.cpp:716-731).  Writer order: rows sorted by (lowest target
 * index bt in images, cell grids[k0][1] * gwidth(bt) + grids[k0][0] at bt's first position k0), a patch
 * without a target image last, equal keys in model order (a stable sort). */
#define PMVS_EXPORT_WRITER_ORDER 1 /* rows in CPatchOrganizerS::collectPatches(1) order (what pmvs2 writes);
                                      without it: model order, row i = record i of pmvs_loop_fetch */
#define PMVS_EXPORT_DEVICE       2 /* every pointer in pmvs_export_buffers is a device pointer on the scene's device */

typedef struct pmvs_export_sizes { int32_t patches, reserved; int64_t image_entries, vimage_entries; } pmvs_export_sizes;

typedef struct pmvs_export_buffers {   /* any pointer may be NULL: that array is skipped */
  float*   fields;      /* patches x 11: coord[4], normal[4], ncc, dscale, ascale (the writers' layout) */
  int32_t* colors;      /* patches x 3: writePLY colour mode 0, exactly pmvs_patch_colors' values */
  int64_t* image_off;   /* patches + 1 */
  int32_t* image_ids;   /* image_entries: _images with index2image applied (identity when index2image == NULL) */
  int32_t* image_idx;   /* image_entries: _images as view indexes */
  int64_t* vimage_off;  /* patches + 1 */
  int32_t* vimage_ids;  /* vimage_entries: _vimages with index2image applied */
  int32_t* source;      /* patches: the model index of each output row */
} pmvs_export_buffers;

/* The pmvs_loop_* pair reads the result pmvs_run_loop left on the device (PMVS_EINVAL when there is
 * none, as pmvs_loop_hash) and does not consume it: pmvs_loop_hash and pmvs_loop_fetch still work
 * afterwards.  index2image: num_views image numbers on the host, or NULL.  Offsets are 64-bit (a
 * C5-size model times its list lengths passes 2^31); zero patches give offsets {0}.  The work is queued
 * on the scene's stream and the call returns after it has finished, so device-mode buffers are ready for
 * any other stream.  A device-mode buffer has the size pmvs_*_export_sizes reported. */
pmvs_status pmvs_loop_export_sizes(pmvs_scene* scene, pmvs_export_sizes* sizes);
pmvs_status pmvs_loop_export(pmvs_scene* scene, int32_t flags, const int32_t* index2image,
                             const pmvs_export_buffers* buffers);
/* The same export of caller-supplied records (results of pmvs_filter_run / pmvs_expand_run, or hand-made
 * ones): uploaded once; list counts (1..PMVS_MAX_IMAGES images, 0..PMVS_MAX_IMAGES vimages) and view
 * indexes are validated as pmvs_filter_run does (PMVS_EINVAL). */
pmvs_status pmvs_export_patches_sizes(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, pmvs_export_sizes* sizes);
pmvs_status pmvs_export_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t flags,
                                const int32_t* index2image, const pmvs_export_buffers* buffers);

/* What each target image sees of the model: CFilter::setDepthMaps (filter.cpp:667-732) over the rows of
 * an export, produced on the device.  Every row is projected into every target image at the scene's
 * level and touches the up to four cells {floor, ceil}(x / csize) x {floor, ceil}(y / csize) that lie
 * in the target's gwidth x gheight cell grid; a cell keeps the row with the smallest depth
 * (OpticalAxis * coord, the f32 value setDepthMapsThread compares) and, at equal depths, the earlier
 * row (the reference replaces only when `depth < dtmp`).  One cell per csize x csize pixels is the
 * density PMVS reconstructs at.
 * Layout: target t's map is row-major, gheight(t) rows of gwidth(t) cells, and starts at cell
 * offsets[t] of every array; targets in index order; offsets[num_targets] cells in all.
 * Rows: flags are PMVS_EXPORT_WRITER_ORDER and PMVS_EXPORT_DEVICE and no other bit (PMVS_EINVAL).
 * Without WRITER_ORDER row i is record i (model order); with it the rows are those of
 * pmvs_loop_export / pmvs_export_patches(PMVS_EXPORT_WRITER_ORDER) of the same records -- the order comes
 * from the same code -- so `patch` indexes that export's arrays, and the maps are what the reference's
 * setDepthMaps computes over the model it writes.  With PMVS_EXPORT_DEVICE every pointer is a device
 * pointer on the scene's device. */
typedef struct pmvs_depthmap_buffers {  /* any pointer may be NULL: that array is skipped */
  int32_t* patch;   /* cells: row of the winning patch, -1 = empty cell */
  float*   depth;   /* cells: OpticalAxis * coord of the winner (the value setDepthMaps compares); 0 = empty */
  float*   normal;  /* cells x 3: the winner's normal x, y, z; 0 = empty */
  float*   ncc;     /* cells: the winner's ncc; 0 = empty */
} pmvs_depthmap_buffers;

/* dims: num_targets x 2 (gwidth, gheight); offsets: num_targets + 1 (first cell of each target's map;
 * the last entry is the total).  Host arrays; either may be NULL.  Depends on the scene only. */
pmvs_status pmvs_depth_map_layout(pmvs_scene* scene, int32_t* dims, int64_t* offsets);
/* The maps of the result pmvs_run_loop left on the device (PMVS_EINVAL when there is none).  Reads it
 * where it lies and does not consume it: pmvs_loop_hash, pmvs_loop_fetch and pmvs_loop_export still
 * work afterwards.  Scratch (8 bytes per cell, 16 or 32 per row) is allocated for the call and freed on
 * return.  The work is queued on the scene's stream and the call returns after it has finished, so
 * device-mode buffers are ready for any other stream. */
pmvs_status pmvs_loop_depth_maps(pmvs_scene* scene, int32_t flags, const pmvs_depthmap_buffers* buffers);
/* The same for caller-supplied records: uploaded once and validated as pmvs_export_patches validates
 * them (PMVS_EINVAL).  n = 0 gives all-empty maps. */
pmvs_status pmvs_depth_maps_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t flags,
                                    const pmvs_depthmap_buffers* buffers);

/* The model rendered into the target images: one depth and one normal per pixel at the scene's level,
 * every patch taken as the oriented plane element its centre and normal are.  The depth maps above hold
 * one flat value per csize x csize cell (what visibility tests want); these maps are what depth-map
 * fusion, meshing and texturing want.  The definition (csrc/pmvs_pixmap.h implements it once, for host
 * and device), for target t with W x H = its image at the scene's level, and row r with f32 coord X and
 * normal N:
 *  1. (x, y) = CCamera::project(view t, X, level) and z = OpticalAxis(t) * X, the f32 values of the
 *     depth maps.
 *  2. Footprint: cx = floor((double)x + 0.5), cy likewise; the integer pixels cx-R <= u <= cx+R,
 *     cy-R <= v <= cy+R that lie in [0, W) x [0, H), R = the call's radius.  Compared in double: project's
 *     clamped values cannot wrap, a NaN fails.  A row with an empty footprint contributes nothing.
 *  3. The depth d at pixel (u, v), in f64 from the f32 inputs, unfused, sums left to right:
 *     V = centre(t) - X, nv = N.V, nn = N.N, vv = V.V (3 components).  If nv > 0 and
 *     nv*nv >= 0.0625*(nn*vv) (the patch faces the camera within ~75.5 degrees): with P the target's 3x4
 *     projection at the level, a = P0 - u*P2, b = P1 - v*P2 (4-vectors; a3, b3 their first three
 *     components), solve [a3; b3; N] S = (-a_w, -b_w, N.X) by Cramer's rule: det = a3.(b3 x N),
 *     S = ((-a_w)*(b3 x N) + (-b_w)*(N x a3) + (N.X)*(a3 x b3)) / det, and
 *     d = (float)(oaxis0*S0 + oaxis1*S1 + oaxis2*S2 + oaxis3): OpticalAxis * (the point where the
 *     pixel's ray meets the patch's plane).  Otherwise, or when that d is not finite or <= 0: d = z.
 *  4. A pixel keeps the minimum key (depth_bits(d) << 32) | r: the smallest depth and, at equal depths,
 *     the earlier row (the depth maps' rule).  The minimum does not depend on the order of arrival.
 *  5. Per pixel, the arrays of pmvs_depthmap_buffers: patch (the row, -1 = empty), depth (the key's d),
 *     normal x 3 and ncc of the winner; empty pixels -1 / +0.0.  Any pointer may be NULL.
 * Layout: the maps of targets [first_target, first_target + num_targets), each row-major H rows of W
 * pixels, target first_target + j at pixel offsets[j] of every array (64-bit: a C5 cluster passes 2^31
 * pixels).  The range bounds memory: a buffer holds 4 (normal: 12) bytes per pixel of the range.
 * flags, rows, record validation and the use of the loop's result are those of the depth-map calls.
 * PMVS_EINVAL: a NULL scene or buffers, another flag bit, an empty range or one outside the scene's
 * targets, a radius outside 0..PMVS_PIXEL_MAX_RADIUS, no loop result.  Scratch (32 bytes per row, 8 per
 * pixel of at most eight targets at a time, and in host mode the maps) is allocated for the call and
 * freed on return; the call returns after its work has finished. */
#define PMVS_PIXEL_MAX_RADIUS 16
/* dims: num_targets x 2 (width, height at the scene's level); offsets: num_targets + 1 pixels, relative to
 * first_target (the last entry is the total).  Host arrays; either may be NULL. */
pmvs_status pmvs_pixel_map_layout(pmvs_scene* scene, int32_t first_target, int32_t num_targets, int32_t* dims,
                                  int64_t* offsets);
pmvs_status pmvs_loop_pixel_maps(pmvs_scene* scene, int32_t flags, int32_t first_target, int32_t num_targets,
                                 int32_t radius, const pmvs_depthmap_buffers* buffers);
/* The same for caller-supplied records, as pmvs_depth_maps_patches.  n = 0 gives all-empty maps. */
pmvs_status pmvs_pixel_maps_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t flags,
                                    int32_t first_target, int32_t num_targets, int32_t radius,
                                    const pmvs_depthmap_buffers* buffers);

/* The per-pixel maps fused into one dense, cross-view-checked point cloud on the device: per pixel the
 * number of other targets that see the same surface point (the support map, the signal of
 * view-dependent filtering), and one oriented, coloured point per supported pixel, emitted once per
 * surface point and not once per view.  There is no reference for this; the definition below is the
 * contract (csrc/pmvs_fuse.h implements it once, for host and device).  All f64 arithmetic is unfused,
 * sums left to right, as for the maps.
 * The fusion is over the targets of the range [first_target, first_target + num_targets) ONLY, as if the
 * scene had no other targets: that bounds memory and makes a range call well defined.  A range call is
 * therefore NOT a slice of the call over all targets: supports count fewer views and other pixels emit.
 *  1. Maps: the patch, depth and normal maps of pmvs_loop_pixel_maps for the range, params->radius and
 *     the flags (the same code renders them, so the same bytes).
 *  2. The point of a filled pixel (t, u, v) with depth d: P and oaxis = view t's projection at the level
 *     and its optical axis, f64 from f32; a = P0 - u*P2, b = P1 - v*P2, c3 = oaxis[0..2]; solve
 *     [a3; b3; c3] S = (-a_w, -b_w, d - oaxis[3]) by Cramer's rule in the maps' operation order:
 *     det = a3.(b3 x c3), S = ((-a_w)*(b3 x c3) + (-b_w)*(c3 x a3) + (d - oaxis3)*(a3 x b3)) / det;
 *     Sf = (float)S.  The pixel is valid iff the three components of Sf are finite.
 *  3. A valid pixel p = (t, u, v) is consistent with target s != t of the range iff, with
 *     (x, y) = CCamera::project(view s, (Sf, 1.0f), level) and zs = OpticalAxis(s) * (Sf, 1.0f) in f32,
 *     px = floor((double)x + 0.5), py likewise: q = (s, px, py) lies in [0, Ws) x [0, Hs) (compared in
 *     double: a NaN fails, clamped values cannot wrap); q is filled; with ds the depth at q, zs > 0 and
 *     fabs((double)ds - (double)zs) <= (double)depth_rel * (double)zs; and with n, m the normals stored at
 *     p and q, (double)n0*m0 + (double)n1*m1 + (double)n2*m2 >= (double)normal_cos (no normalisation).
 *  4. support(p) = the number of consistent s; 0 for empty or invalid pixels (at most 255: a byte).
 *     pass(p) = filled and valid and support(p) >= min_support.
 *  5. emit(p) = pass(p) and there is no s < t in the range with p consistent with s and pass(q(p, s)).
 *     A suppressed pixel so has a passing consistent pixel in a lower target, and that chain ends at an
 *     emitted one: no supported surface point is lost.  Nothing depends on the order of the work.
 *  6. The points: the emitted pixels in ascending pixel index of the range (target, row, column); per
 *     point coord = Sf, normal = the pixel's, color = the three bytes of pixel (u, v) of target t's image
 *     at the scene's level as pmvs_scene_get_level returns them, support, pixel = its index in the layout
 *     of pmvs_pixel_map_layout for the range, patch = the row.
 * flags, rows, record validation and the use of the loop's result are those of the pixel-map calls.
 * *count receives the number of emitted points, which may exceed cap; only the first min(*count, cap)
 * points are written and nothing past cap; cap = 0 with NULL point arrays is the counting call.  With
 * PMVS_EXPORT_DEVICE every pointer of the buffers is a device pointer on the scene's device.
 * PMVS_EINVAL: a NULL scene, params, buffers or count; another flag bit; an empty range or one outside the
 * scene's targets; a parameter outside the ranges below; cap < 0; no loop result.  PMVS_ENOMEM when the
 * device cannot hold the scratch: 21 bytes per pixel of the RANGE (patch 4, depth 4, normal 12, support 1;
 * the support map is the caller's when given in device mode), the pixel maps' own scratch, and 9 bytes per
 * pixel for the pass flags and the compaction (and in host mode the requested arrays, for min(cap, pixels
 * of the range) points: no more can be emitted, so a generous cap costs nothing).  All of it is
 * allocated for the call and freed on return; the call returns after its work has finished. */
typedef struct pmvs_fuse_params {
  int32_t radius;       /* the maps' radius, 0..PMVS_PIXEL_MAX_RADIUS */
  int32_t min_support;  /* 0..255: other targets of the range that must agree */
  float   depth_rel;    /* finite, >= 0: relative depth tolerance */
  float   normal_cos;   /* not NaN: least dot product of the two stored normals */
} pmvs_fuse_params;

typedef struct pmvs_fuse_buffers {   /* any pointer may be NULL: that array is skipped */
  uint8_t* support_map;  /* pixels of the range */
  float*   coord;        /* cap x 3 */
  float*   normal;       /* cap x 3 */
  uint8_t* color;        /* cap x 3 */
  uint8_t* support;      /* cap */
  int64_t* pixel;        /* cap */
  int32_t* patch;        /* cap */
} pmvs_fuse_buffers;

/* Reads the result pmvs_run_loop left on the device where it lies and does not consume it (the digest of
 * pmvs_loop_hash is the same before and after). */
pmvs_status pmvs_loop_fuse(pmvs_scene* scene, int32_t flags, int32_t first_target, int32_t num_targets,
                           const pmvs_fuse_params* params, int64_t cap, const pmvs_fuse_buffers* buffers,
                           int64_t* count);
/* The same for caller-supplied records, validated and uploaded as pmvs_pixel_maps_patches does.  n = 0 gives
 * a zero support map and *count = 0. */
pmvs_status pmvs_fuse_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t flags,
                              int32_t first_target, int32_t num_targets, const pmvs_fuse_params* params,
                              int64_t cap, const pmvs_fuse_buffers* buffers, int64_t* count);
/* A point cloud as one binary PLY: the header `format binary_little_endian 1.0`, `element vertex n`,
 * float x y z nx ny nz, uchar diffuse_red diffuse_green diffuse_blue, uchar support; then n 28-byte
 * records.  Host arrays (coord and normal n x 3 floats, color n x 3 bytes, support n bytes).  PMVS_EINVAL
 * for a NULL path, n < 0, a NULL array with n > 0, or a file that cannot be written. */
pmvs_status pmvs_write_ply_binary(const char* path, int64_t n, const float* coord, const float* normal,
                                  const uint8_t* color, const uint8_t* support);

/* The fused maps meshed on the device, in two stages: a truncated signed distance (TSDF) volume integrated
 * from the per-pixel maps and the fusion's pass flags, and a triangle mesh extracted from a volume by naive
 * surface nets (no case table; a closed manifold wherever the volume is closed).  There is no reference
 * for this; the definition below is the contract (csrc/pmvs_mesh.h implements it once, for host and
 * device).  All f64 arithmetic is unfused, sums left to right in the stated order, as for the maps.
 *
 * The volume is an axis-aligned box of nx x ny x nz voxels of edge `voxel` from `origin`; voxel (i, j, k)
 * has index ((k*ny)+j)*nx + i (x fastest).
 *
 * INTEGRATION (pmvs_loop_tsdf, pmvs_tsdf_patches).  The inputs are the range's patch, depth and normal maps
 * and the fusion's pass(p) flags (pmvs_loop_fuse step 4) for params->fuse: the code pmvs_loop_fuse runs
 * computes them, so they are the same bytes.  For voxel (i, j, k):
 *  1. Cf[a] = (float)((double)origin[a] + ((double)idx_a + 0.5) * (double)voxel).
 *  2. For each target t of the range, ascending: (x, y) = CCamera::project(view t, (Cf, 1.0f), level) and
 *     z = OpticalAxis(t) * (Cf, 1.0f) in f32; px = floor((double)x + 0.5), py likewise, the inside test in
 *     double (fuse step 3).  t observes the voxel iff q = (t, px, py) is inside the image, pass(q), z > 0,
 *     and with d the depth at q, s = (double)d - (double)z >= -(double)trunc.  Then
 *     v = s >= (double)trunc ? 1.0 : s / (double)trunc, sum += v, n += 1; and if s < (double)trunc the
 *     three bytes of pixel q of target t's level image are added to three integer sums and nc += 1.
 *  3. tsdf = n ? (float)(sum / (double)n) : 1.0f; obs = min(n, 255);
 *     color = nc ? ((sum_c + nc/2) / nc per channel, 255) : (0, 0, 0, 0), integer division.
 * The TSDF is positive outside the surface.  Nothing depends on the order of the work.
 *
 * EXTRACTION (pmvs_tsdf_mesh).  observed = obs >= min_obs, inside = tsdf < 0.
 *  Cells: cell (i, j, k), 0 <= i < nx-1 and likewise j, k, has index ((k*(ny-1))+j)*(nx-1) + i; its corner c
 *   is the voxel (i + (c&1), j + ((c>>1)&1), k + (c>>2)).  A cell is active iff all 8 corners are observed
 *   and their inside flags are not all equal.
 *  Edges: a cell's 12 edges in order: the four x-edges with (y, z) offsets 00, 10, 01, 11, the four y-edges
 *   with (z, x) offsets in that pattern, the four z-edges with (x, y) offsets; each from the lower corner
 *   (value v0) to the upper (v1).  An edge crosses when its two inside flags differ; then
 *   t = (double)v0 / ((double)v0 - (double)v1) and its crossing point in cell units is the lower corner's
 *   offset plus t along the edge's axis.
 *  Vertex of an active cell: m = the sum of the crossing points (per component, in edge order) divided by
 *   their count; vertex[a] = (float)((double)origin[a] + ((double)idx_a + 0.5 + m_a) * (double)voxel).
 *  Normal: g_a = the sum of ((double)v1 - (double)v0) over axis a's four edges in edge order,
 *   len = sqrt(gx*gx + gy*gy + gz*gz), normal[a] = (float)(g_a / len); zero when len is 0 or not finite.
 *   It points outward.
 *  Colour: per channel (sum + m/2) / m over the m corners whose A byte is 255, integer division; 0 when
 *   m = 0 or color is NULL.
 *  Vertices are emitted in ascending cell index.
 *  Faces: for every voxel (i, j, k) in ascending index and every axis a in x, y, z order, with (a, b, c) the
 *   cyclic permutation of (x, y, z) that starts at a: the edge to the +a neighbour is considered iff that
 *   neighbour exists, 1 <= idx_b <= n_b-2 and 1 <= idx_c <= n_c-2; it emits iff both endpoints are
 *   observed, their inside flags differ, and the four cells with a-coordinate idx_a and (b, c) coordinates
 *   Q0 = (idx_b-1, idx_c-1), Q1 = (idx_b, idx_c-1), Q2 = (idx_b, idx_c), Q3 = (idx_b-1, idx_c) are all
 *   active.  If the lower endpoint is inside it emits the two consecutive triangles (Q0, Q1, Q2),
 *   (Q0, Q2, Q3) as vertex ids, otherwise (Q0, Q2, Q1), (Q0, Q3, Q2): either way they face outward.
 *  *nverts and *nfaces receive the full counts; only the first min(count, cap) entries are written and
 *  nothing past a cap; caps 0 with NULL arrays is the counting call.  A volume with a dim of 1 has no cells
 *  and gives an empty mesh.
 *
 * flags, the target range, record validation, the use of the loop's result and device / host mode are
 * those of the fuse calls; with PMVS_EXPORT_DEVICE every array pointer is a device pointer on the scene's
 * device.  pmvs_tsdf_mesh takes only the device and stream from the scene, and of the flags only
 * PMVS_EXPORT_DEVICE.  pmvs_loop_mesh / pmvs_mesh_patches integrate and extract in one call; the volume
 * never leaves the device.
 * PMVS_EINVAL: a NULL scene, volume, params, buffers or count pointer (pmvs_tsdf_mesh: a NULL tsdf or obs);
 * another flag bit; the fuse calls' range and parameter checks; a non-finite origin; voxel or trunc not
 * finite or <= 0; a dim < 1 or nx*ny*nz > 2^31-1; min_obs outside 1..255; a negative cap; no loop result.
 * PMVS_ENOMEM when the device cannot hold the scratch.  Integration: 22 bytes per pixel of the RANGE (patch
 * 4, depth 4, normal 12, support 1, pass 1) and the pixel maps' own scratch; nothing per voxel but the
 * outputs (in host mode the requested ones staged on the device, at most 9 bytes per voxel; the combined
 * calls always hold all 9).  Extraction: 5 bytes per cell (active flag 1, vertex id 4), 9 bytes per voxel
 * (face flags 1, face offset 8) and the scan's temporary storage; in host mode also the volume (9 bytes
 * per voxel) and the requested mesh arrays for min(cap, cells) vertices and min(cap, 6 * voxels) faces.
 * All of it is allocated for the call and freed on return; the calls return after their work has finished. */
typedef struct pmvs_volume {
  float   origin[3];  /* finite: the corner of voxel (0, 0, 0) */
  float   voxel;      /* finite, > 0: the voxels' edge */
  int32_t dims[3];    /* nx, ny, nz >= 1, nx*ny*nz <= 2^31-1 */
} pmvs_volume;

typedef struct pmvs_tsdf_params {
  pmvs_fuse_params fuse;  /* the maps and pass flags integrated */
  float            trunc; /* finite, > 0: the truncation distance, in the scene's units */
} pmvs_tsdf_params;

typedef struct pmvs_tsdf_buffers {  /* any pointer may be NULL: that array is skipped */
  float*   tsdf;   /* voxels */
  uint8_t* obs;    /* voxels */
  uint8_t* color;  /* voxels x 4: RGBA, A = 255 iff the voxel has a colour; a device pointer is 4-byte aligned */
} pmvs_tsdf_buffers;

typedef struct pmvs_mesh_buffers {  /* any pointer may be NULL: that array is skipped */
  float*   vertex;  /* vcap x 3 */
  float*   normal;  /* vcap x 3 */
  uint8_t* color;   /* vcap x 3 */
  int32_t* face;    /* fcap x 3: vertex ids */
} pmvs_mesh_buffers;

/* Reads the result pmvs_run_loop left on the device and does not consume it. */
pmvs_status pmvs_loop_tsdf(pmvs_scene* scene, int32_t flags, int32_t first_target, int32_t num_targets,
                           const pmvs_tsdf_params* params, const pmvs_volume* volume, const pmvs_tsdf_buffers* buffers);
/* The same for caller-supplied records, validated and uploaded as pmvs_fuse_patches does. */
pmvs_status pmvs_tsdf_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t flags,
                              int32_t first_target, int32_t num_targets, const pmvs_tsdf_params* params,
                              const pmvs_volume* volume, const pmvs_tsdf_buffers* buffers);
/* The mesh of caller-supplied volume arrays (tsdf and obs one value per voxel, color 4 bytes per voxel or
 * NULL; a device color pointer is 4-byte aligned). */
pmvs_status pmvs_tsdf_mesh(pmvs_scene* scene, int32_t flags, const pmvs_volume* volume, int32_t min_obs,
                           const float* tsdf, const uint8_t* obs, const uint8_t* color, int64_t vcap, int64_t fcap,
                           const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces);
/* Integration then extraction. */
pmvs_status pmvs_loop_mesh(pmvs_scene* scene, int32_t flags, int32_t first_target, int32_t num_targets,
                           const pmvs_tsdf_params* params, const pmvs_volume* volume, int32_t min_obs, int64_t vcap,
                           int64_t fcap, const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces);
pmvs_status pmvs_mesh_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t flags,
                              int32_t first_target, int32_t num_targets, const pmvs_tsdf_params* params,
                              const pmvs_volume* volume, int32_t min_obs, int64_t vcap, int64_t fcap,
                              const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces);
/* The volume `pmvs2 ... MESH` uses for a point cloud (host coord, n x 3): with lo, hi the cloud's bounding
 * box, voxel = (float)(max_a((double)hi[a] - (double)lo[a]) / (double)cells), origin[a] =
 * (float)((double)lo[a] - (double)pad * (double)voxel) and dims[a] = max(1, ceil(((double)hi[a] -
 * (double)lo[a]) / (double)voxel)) + 2 * pad.  PMVS_EINVAL for a NULL pointer, n < 1, cells < 1, pad < 0, a
 * point that is not finite, a box of no extent, or a volume past the limits above. */
pmvs_status pmvs_volume_from_points(int64_t n, const float* coord, int32_t cells, int32_t pad, pmvs_volume* volume);
/* A mesh as one binary PLY: the header `format binary_little_endian 1.0`, `element vertex nv`, float x y z
 * nx ny nz, uchar diffuse_red diffuse_green diffuse_blue, `element face nf`, `property list uchar int
 * vertex_indices`; then nv 27-byte vertex records and nf 13-byte face records (the count 3 and three ids).
 * Host arrays.  PMVS_EINVAL for a NULL path, a negative count, a NULL array with a positive count, or a
 * file that cannot be written. */
pmvs_status pmvs_write_ply_mesh_binary(const char* path, int64_t nv, const float* vertex, const float* normal,
                                       const uint8_t* color, int64_t nf, const int32_t* face);

/* The same meshing in a SPARSE volume: the volume exists only in 8 x 8 x 8-voxel bricks near the fused
 * points, so its resolution is bounded by the surface's area and not by the box's volume.  A voxel's values
 * and the mesh keep the definitions above exactly; what follows defines where the volume exists
 * (csrc/pmvs_brick.h implements it once, for host and device).
 *
 * THE VIRTUAL VOLUME is a pmvs_volume with limits of its own: every dim in 1..PMVS_BRICK_MAX_DIM, and the
 * brick grid Ba = ceil(dims[a] / 8) with Bx*By*Bz <= 2^31-1; the dense nx*ny*nz limit does not apply.  The
 * key of brick (bi, bj, bk) is (bk*By + bj)*Bx + bi.  The stored bricks are listed by ascending key; voxel
 * (8bi+li, 8bj+lj, 8bk+lk) of stored brick number s (its position in that list) is at array index
 * s*512 + (lk*8 + lj)*8 + li.
 *
 * SELECTION (which bricks exist).
 *  1. For every pixel p of the range with pass(p) (fuse step 4): Sf from fuse step 2.
 *  2. g_a = floor(((double)Sf[a] - (double)origin[a]) / (double)voxel) per axis, in double.
 *  3. The pixel is skipped if, compared in double, g_a + margin < 0 or g_a - margin > dims[a] - 1 for any a.
 *  4. Otherwise lo_a = max(0, g_a - margin), hi_a = min(dims[a] - 1, g_a + margin).
 *  5. Every brick with lo_a >> 3 <= b_a <= hi_a >> 3 on all three axes is selected.
 * The brick list is the selected keys in ascending order.  Nothing depends on the order of the work.
 *
 * INTEGRATION (pmvs_loop_brick_tsdf, pmvs_brick_tsdf_patches).  A stored voxel inside dims gets steps 1-3
 * of the INTEGRATION above, by the same code: the bytes pmvs_loop_tsdf writes for that voxel whenever the
 * dense call accepts the volume.  A stored voxel outside dims (the overhang of an edge brick) is tsdf 1.0f,
 * obs 0, colour (0, 0, 0, 0).  *nbricks receives the full count; only the first min(count, bcap) bricks are
 * written and nothing past them; bcap 0 with NULL arrays is the counting call.
 *
 * EXTRACTION (pmvs_brick_tsdf_mesh).  The EXTRACTION above applied to the virtual volume, in which a voxel
 * of no stored brick reads as obs 0, tsdf 1.0f, colour 0: the same cells, edges, vertex, normal, colour and
 * face rules and the same orders, vertices by ascending virtual cell index ((k*(ny-1))+j)*(nx-1) + i and
 * faces by ascending (virtual voxel index, axis).  So for any volume the dense calls accept, the output is
 * byte for byte that of pmvs_tsdf_mesh on the dense arrays obtained by scattering the bricks into a volume
 * pre-filled with (1.0f, 0, 0).  Keys are caller-supplied here: strictly ascending and inside the grid.
 * More than 2^31-1 vertices: PMVS_EUNSUPPORTED (face ids are int32).
 *
 * MARGIN is the caller's knob, not a guarantee: a cell that is active in the dense volume but has a corner
 * in no stored brick drops out, and the surface opens a boundary there -- the rule for unobserved regions.
 * A margin of ceil(trunc / voxel) + 2 keeps the band around every fused point; `pmvs2 ... FINEMESH` uses it.
 *
 * flags, the target range, record validation, the loop's result and device / host mode are those of the
 * dense calls; pmvs_brick_tsdf_mesh takes of the flags only PMVS_EXPORT_DEVICE.  pmvs_loop_brick_mesh /
 * pmvs_brick_mesh_patches select, integrate and extract in one call and the bricks never leave the device.
 * As in the dense calls, a counting call does the whole selection (and the mesh calls the integration)
 * again: no volume is kept between calls.
 * PMVS_EINVAL: the dense calls' checks with the volume limits above in place of theirs; a margin outside
 * 0..PMVS_BRICK_MAX_MARGIN; a negative cap or nbricks; pmvs_brick_tsdf_mesh: a NULL brick, tsdf or obs with
 * nbricks > 0, keys not strictly ascending or outside the grid (device mode: checked by a kernel before a
 * key is used).  PMVS_ENOMEM when the device cannot hold the scratch: the integration's 22 bytes per pixel
 * of the range; 5 bytes per brick of the GRID (flag 1, slot 4; pmvs_brick_tsdf_mesh: 4) and the scan's
 * storage; the bricks themselves (8 + 512 * 9 bytes each: the combined calls hold all of them, the others
 * the requested arrays in host mode); for the extraction 10 bytes per stored voxel (cell flag 1, face flags
 * 1, offset 8), 4 more (vertex id) when faces are written, and 32 bytes per vertex, then per quad, for the
 * sort's (key, value) pairs in and out plus rocprim's radix sort storage; in host mode the requested mesh
 * arrays.  All of it is allocated for the call and freed on return. */
#define PMVS_BRICK 8              /* voxels per brick edge; 512 per brick */
#define PMVS_BRICK_MAX_MARGIN 64
#define PMVS_BRICK_MAX_DIM (1 << 20)

typedef struct pmvs_brick_params {
  pmvs_tsdf_params tsdf;    /* the maps integrated and the truncation distance */
  int32_t          margin;  /* 0..PMVS_BRICK_MAX_MARGIN: voxels around each fused point's voxel */
} pmvs_brick_params;

typedef struct pmvs_brick_buffers {  /* any pointer may be NULL: that array is skipped */
  int64_t* brick;   /* bcap: brick keys, strictly ascending */
  float*   tsdf;    /* bcap x 512 */
  uint8_t* obs;     /* bcap x 512 */
  uint8_t* color;   /* bcap x 512 x 4: RGBA as pmvs_tsdf_buffers; a device pointer is 4-byte aligned */
} pmvs_brick_buffers;

/* Reads the result pmvs_run_loop left on the device and does not consume it. */
pmvs_status pmvs_loop_brick_tsdf(pmvs_scene* scene, int32_t flags, int32_t first_target, int32_t num_targets,
                                 const pmvs_brick_params* params, const pmvs_volume* volume, int64_t bcap,
                                 const pmvs_brick_buffers* buffers, int64_t* nbricks);
/* The same for caller-supplied records. */
pmvs_status pmvs_brick_tsdf_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t flags,
                                    int32_t first_target, int32_t num_targets, const pmvs_brick_params* params,
                                    const pmvs_volume* volume, int64_t bcap, const pmvs_brick_buffers* buffers,
                                    int64_t* nbricks);
/* The mesh of caller-supplied bricks (brick nbricks keys, tsdf and obs nbricks x 512, color nbricks x 512 x 4
 * or NULL; a device color pointer is 4-byte aligned). */
pmvs_status pmvs_brick_tsdf_mesh(pmvs_scene* scene, int32_t flags, const pmvs_volume* volume, int32_t min_obs,
                                 int64_t nbricks, const int64_t* brick, const float* tsdf, const uint8_t* obs,
                                 const uint8_t* color, int64_t vcap, int64_t fcap, const pmvs_mesh_buffers* buffers,
                                 int64_t* nverts, int64_t* nfaces);
/* Selection, integration, then extraction. */
pmvs_status pmvs_loop_brick_mesh(pmvs_scene* scene, int32_t flags, int32_t first_target, int32_t num_targets,
                                 const pmvs_brick_params* params, const pmvs_volume* volume, int32_t min_obs,
                                 int64_t vcap, int64_t fcap, const pmvs_mesh_buffers* buffers, int64_t* nverts,
                                 int64_t* nfaces);
pmvs_status pmvs_brick_mesh_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t flags,
                                    int32_t first_target, int32_t num_targets, const pmvs_brick_params* params,
                                    const pmvs_volume* volume, int32_t min_obs, int64_t vcap, int64_t fcap,
                                    const pmvs_mesh_buffers* buffers, int64_t* nverts, int64_t* nfaces);
/* pmvs_volume_from_points' formulas within the brick volume's limits (a dim past PMVS_BRICK_MAX_DIM or a
 * brick grid past 2^31-1 is PMVS_EINVAL): the volume `pmvs2 ... FINEMESH` uses. */
pmvs_status pmvs_brick_volume_from_points(int64_t n, const float* coord, int32_t cells, int32_t pad, pmvs_volume* volume);

/* TEXTURING without an atlas: the textures are the target images themselves.  A triangle mesh (vertex nv x 3
 * f32, face nf x 3 int32 vertex ids; from pmvs_tsdf_mesh, pmvs_brick_tsdf_mesh or the caller's own) is
 * rasterised into the targets [first_target, first_target + num_targets) at the scene's level L, and every
 * face gets the target that sees it best and unoccluded and its corners' positions in that image.  Only the
 * device, the stream and the views are taken from the scene; no loop result is needed.  There is no
 * reference for this; csrc/pmvs_texmesh.h implements what follows once, for host and device.  All f64
 * arithmetic is unfused, from the f32 inputs, sums left to right in the order written.
 *
 * Per vertex i and target t (W x H its image at level L): (x_i, y_i) = CCamera::project(view t, (V_i, 1.0f), L)
 * and z_i = OpticalAxis(t) . (V_i, 1.0f), all f32.
 *
 * A. THE RASTER (pmvs_mesh_raster): per pixel of every target of the range, the nearest face and its depth.
 *  1. Face f = (i0, i1, i2) is DRAWN in t iff the three z are finite and > 0, the six coordinates are finite,
 *     and A = (x1-x0)*(y2-y0) - (y1-y0)*(x2-x0) (differences and products in f64) is finite and != 0.  Both
 *     windings are drawn: a back face occludes too.
 *  2. Its box: u0 = max(0, ceil(min x)), u1 = min(W-1, floor(max x)), v0 and v1 likewise from y and H, in
 *     double (project's clamped +-2^31 cannot wrap).  An empty box draws nothing.
 *  3. Integer pixel (u, v) of the box is covered iff, with
 *       w0 = (x2-x1)*(v-y1) - (y2-y1)*(u-x1), w1 = (x0-x2)*(v-y2) - (y0-y2)*(u-x2),
 *       w2 = (x1-x0)*(v-y0) - (y1-y0)*(u-x0),
 *     all wk >= 0 when A > 0, all wk <= 0 when A < 0.  A shared edge is covered from both sides; step 5 makes
 *     that harmless, and no fill rule is needed.
 *  4. Its depth there: lk = wk / A, inv = l0/(double)z0 + l1/(double)z1 + l2/(double)z2, d = (float)(1.0 / inv)
 *     (1/z is affine in the image: the optical axis is the projection's third row scaled).  The pixel takes
 *     the face iff d is finite and > 0.
 *  5. A pixel keeps the minimum key (depth_bits(d) << 32) | f: the smallest depth and, at equal depths, the
 *     lower face id -- the maps' rule, so nothing depends on the order of the work.
 *  6. face: int32 per pixel, -1 where empty; depth: f32 per pixel, +0.0 where empty; laid out as
 *     pmvs_pixel_map_layout gives for the range.  Either pointer may be NULL.  nf = 0: every pixel is empty.
 *
 * B. VIEW SELECTION (pmvs_mesh_texture).  Face f is ELIGIBLE in target t of the range iff
 *  1. it is drawn in t (A.1);
 *  2. it is seen from its front: N = (V1-V0) x (V2-V0) in f64 and N . (centre(t) - V0) > 0 (the extraction
 *     winds faces outward);
 *  3. every corner k is visible: the pixel q = (floor((double)xk + 0.5), floor((double)yk + 0.5)) lies in the
 *     image (the fusion's pixel_at), and with (fq, dq) the raster of A at q either fq == -1 (an empty pixel
 *     occludes nothing) or (double)zk - (double)dq <= (double)depth_rel * (double)zk.  All three corners
 *     inside the image puts the whole face inside;
 *  4. its score s = (float)(0.5 * fabs(A)), the projected area in pixels^2, is >= min_area.
 *  view(f) = the eligible t with the greatest s, the lowest t on ties, as a scene target index; -1 if none.
 *  score(f) = the winner's s, 0 with view -1.  uv(f) = six f32, (x, y) of the three corners from
 *  project(view, (Vk, 1.0f), 0): LEVEL-0 pixels, so they address the image file whatever the scene's level;
 *  0 with view -1.  Any pointer may be NULL.  nf = 0 writes nothing.
 *  The raster B reads is A's, rendered inside the call by the same code.
 *
 * C. THE FILE (pmvs_write_ply_texmesh_binary; host arrays).  The header is exactly
 *     ply\nformat binary_little_endian 1.0\n
 *     comment TextureFile <tex_files[0]>\n ... comment TextureFile <tex_files[ntex-1]>\n
 *     element vertex <nv>\nproperty float x\nproperty float y\nproperty float z\nproperty float nx\n
 *     property float ny\nproperty float nz\nproperty uchar diffuse_red\nproperty uchar diffuse_green\n
 *     property uchar diffuse_blue\nelement face <nf>\nproperty list uchar int vertex_indices\n
 *     property list uchar float texcoord\nproperty int texnumber\nend_header\n
 *  then nv 27-byte vertex records as pmvs_write_ply_mesh_binary writes them and nf 42-byte face records: the
 *  count 3 and three ids (13 bytes), the count 6 and u0 v0 u1 v1 u2 v2 (25 bytes), texnumber = view (4 bytes).
 *  With (W0, H0) = tex_dims[2 * view], tex_dims[2 * view + 1] and (x, y) a corner's uv:
 *  u = (float)clamp(((double)x + 0.5) / W0, 0, 1), v = (float)clamp(1.0 - ((double)y + 0.5) / H0, 0, 1): pixel
 *  centres at integers, the V axis up.  A face with view -1 gets six zeros.
 *
 * flags: only PMVS_EXPORT_DEVICE; with it every array pointer (vertex, face and the buffers') is a device
 * pointer on the scene's device.  PMVS_EINVAL: a NULL scene, params or buffers; another flag bit; an empty
 * range or one outside the scene's targets; nv or nf negative or above 2^31-1; a NULL array with a positive
 * count; depth_rel or min_area not finite or < 0; a face id outside [0, nv) (host ids are checked before the
 * scene is touched, device ids by a kernel whose one flag is read back before any id is used as an index);
 * the writer: a NULL path, a view outside -1..ntex-1, a texture dim < 1, a NULL name, a file that cannot be
 * written.  PMVS_ENOMEM when the device cannot hold the scratch: 8 bytes per pixel of one group of at most
 * eight targets (the keys); nothing per vertex; per face 8 bytes for each (face, target of the group) whose
 * clipped box exceeds 64 pixels (at most 64 bytes per face, none for a mesh at image resolution) and, in
 * pmvs_mesh_texture, 8 bytes for the running view and score where the caller did not ask for them; in host
 * mode also the mesh (12 bytes per vertex and per face) and the requested outputs (8 bytes per pixel of the
 * range; 32 bytes per face).  All of it is allocated for the call and freed on return; the calls return after
 * their work has finished. */
typedef struct pmvs_raster_buffers {  /* either pointer may be NULL: that array is skipped */
  int32_t* face;   /* pixels of the range: the nearest face, -1 = empty */
  float*   depth;  /* pixels of the range: its depth, +0.0 = empty */
} pmvs_raster_buffers;

typedef struct pmvs_texture_params {
  float depth_rel;  /* finite, >= 0: a corner may lie this fraction of its depth behind the raster */
  float min_area;   /* finite, >= 0: the smallest projected area, in pixels^2 at the scene's level */
} pmvs_texture_params;

typedef struct pmvs_texture_buffers {  /* any pointer may be NULL: that array is skipped */
  int32_t* view;   /* nf: the chosen target, -1 = none */
  float*   uv;     /* nf x 6: the corners in level-0 pixels of that target */
  float*   score;  /* nf: the winner's projected area */
} pmvs_texture_buffers;

pmvs_status pmvs_mesh_raster(pmvs_scene* scene, int32_t flags, int32_t first_target, int32_t num_targets, int64_t nv,
                             const float* vertex, int64_t nf, const int32_t* face, const pmvs_raster_buffers* buffers);
pmvs_status pmvs_mesh_texture(pmvs_scene* scene, int32_t flags, int32_t first_target, int32_t num_targets,
                              const pmvs_texture_params* params, int64_t nv, const float* vertex, int64_t nf,
                              const int32_t* face, const pmvs_texture_buffers* buffers);
/* tex_files: ntex names, written as given; tex_dims: ntex x 2, the (width, height) the uv are scaled by. */
pmvs_status pmvs_write_ply_texmesh_binary(const char* path, int64_t nv, const float* vertex, const float* normal,
                                          const uint8_t* color, int64_t nf, const int32_t* face, const int32_t* view,
                                          const float* uv, int32_t ntex, const char* const* tex_files,
                                          const int32_t* tex_dims);

/* THE ATLAS: the textured mesh baked into one image.  pmvs_mesh_atlas cuts every face's texels out of the view
 * pmvs_mesh_texture chose for it and packs them into one W-texel-wide RGB image, so that the model travels
 * with one texture instead of its input images.  Only the device, the stream, the views and the level-0 images
 * are taken from the scene.  There is no reference for this; csrc/pmvs_atlas.h implements what follows once,
 * for host and device.  All f64 arithmetic is unfused, from the f32 inputs, sums left to right in the order
 * written.
 *
 * Inputs: the mesh (vertex nv x 3 f32, face nf x 3 int32), view (nf int32, as pmvs_mesh_texture returns it: a
 * scene target index in [0, num_targets) or -1) and the parameters width W, max_side M and scale.
 *  1. CORNERS.  For face f with view(f) = t >= 0 and corner k: (x_k, y_k, w_k) = CCamera::project(view t,
 *     (V_k, 1.0f), 0): level-0 pixels, pmvs_mesh_texture's uv.  f is PLACED iff t >= 0, the three w_k > 0 and
 *     the six coordinates are finite.
 *  2. SIDE.  e = the greatest of |x_a - x_b| and |y_a - y_b| over the three edges (differences in f64; a
 *     Chebyshev length, no square root), s = (double)scale * e, n(f) = 1 if s <= 1, M if s >= M, else
 *     (int)ceil(s).
 *  3. ORDER.  The placed faces of side n, by ascending face id, have ranks r = 0, 1, ... within their class;
 *     slot = r >> 1, half = r & 1: two faces share one square cell.
 *  4. BANDS.  Classes are laid out from n = M down to 1.  For class n: c = n + 5, k = W / c cells per row,
 *     slots = (count_n + 1) >> 1, rows = ceil(slots / k), y_n = the sum over the classes m > n of
 *     rows_m * (m + 5); slot s has the cell origin (ox, oy) = ((s % k) * c, y_n + (s / k) * c).  The atlas
 *     height H = the sum over all classes of rows_n * (n + 5); 0 if nothing is placed.
 *  5. TRIANGLES.  Texel centres are at integers (uv's convention, so pmvs_write_ply_texmesh_binary applies
 *     unchanged).  Relative to the cell origin, half 0 has the corners T0 = (1, 1), T1 = (1 + n, 1),
 *     T2 = (1, 1 + n); half 1 has T0 = (c - 2, c - 2), T1 = (c - 2 - n, c - 2), T2 = (c - 2, c - 2 - n).
 *     Texel (i, j) of the cell belongs to half 0 iff i + j <= n + 3, otherwise to half 1.  A bilinear fetch
 *     at any point of a triangle then touches, with non-zero weight, only texels of its own half of its own
 *     cell; column and row 0 are pure gutter of half 0, column and row c - 1 of half 1.
 *  6. TEXEL -> COLOUR.  Texel (I, J) of the atlas: the band that contains row J, the cell row (J - y_n) / c,
 *     the column I / c, hence the slot and (i, j) = (I - ox, J - oy) and the half.  The texel is EMPTY when
 *     I / c >= k, when the slot is >= slots, when its half holds no face (the last slot of a class with an
 *     odd count), or when J >= H: texel_face = -1, colour (0, 0, 0).  Otherwise f is its face and, for half 0,
 *     l1 = (double)(i - 1) / n, l2 = (double)(j - 1) / n; for half 1, l1 = (double)(c - 2 - i) / n,
 *     l2 = (double)(c - 2 - j) / n; l0 = 1.0 - l1 - l2; X_a = (float)(l0 * V0_a + l1 * V1_a + l2 * V2_a);
 *     (x, y, w) = project(view(f), (X, 1.0f), 0): through the face's plane, so perspective-correct; gutter
 *     texels extrapolate on the same plane.  If w <= 0 or x or y is not finite the colour is (0, 0, 0).
 *     Otherwise xs = x clamped to [0, W0 - 2], ys = y clamped to [0, H0 - 2] (compared in double, the bounds
 *     as f32; W0 x H0 = view(f)'s level-0 image), rgb = CImage::getColor's bilinear arithmetic
 *     (image.hpp:435-476) on that image at (xs, ys), and each byte = min(255, floor(c + 0.5f)),
 *     pmvs_patch_colors' rounding.  The clamp gives up at most the last column and row of a source image.
 *  7. OUTPUTS.  rgb: H x W x 3 bytes, top row first.  texel_face: H x W int32.  uv: nf x 6 f32, for a placed
 *     face the three corners (float)(ox + T_k.x), (float)(oy + T_k.y), zeros for any other face.  atlas_view:
 *     nf int32, 0 for a placed face and -1 otherwise: what pmvs_write_ply_texmesh_binary takes as `view` with
 *     ntex = 1 and tex_dims = {W, H}.  Any pointer may be NULL (and buffers itself: nothing is wanted).  Only
 *     the first min(H, height_cap) rows of the two images are written and nothing past them; height_cap = 0
 *     with NULL image pointers is the sizing call.  *layout = {W, H, placed faces, cells (the sum of slots)}.
 *     Nothing depends on the order of the work.
 *
 * flags: only PMVS_EXPORT_DEVICE; with it every array pointer (vertex, face, view and the buffers') is a device
 * pointer on the scene's device.  PMVS_EINVAL: a NULL scene, params or layout; another flag bit; max_side
 * outside 1..PMVS_ATLAS_MAX_SIDE; width outside [max_side + 5, PMVS_ATLAS_MAX_WIDTH]; scale not finite or
 * <= 0; nv or nf negative or above 2^31-1; a NULL array with a positive count; a negative height_cap; a source
 * image narrower or lower than 2 pixels at level 0; a face id outside [0, nv) or a view outside
 * [-1, num_targets) (host arrays are checked before the device is touched, device arrays by a kernel whose one
 * flag is read back before any value is used as an index).  PMVS_EUNSUPPORTED when H exceeds 2^31-1 (*layout is
 * still filled, its fields saturated at 2^63-1).  PMVS_ENOMEM when the device cannot hold the scratch: per face 10 bytes (two class bytes, the
 * face id and its place in the class order) and the radix sort's temporary storage (about 5 more); nothing per
 * texel; in host mode also the mesh (12 bytes per vertex, 16 per face) and the requested outputs (7 bytes per
 * written texel, 28 per face).  All of it is allocated for the call and freed on return; the call returns
 * after its work has finished.
 *
 * pmvs_atlas_layout_from_counts is step 4 alone, on the host: counts[n], n = 1..max_side, = the placed faces
 * of side n (counts[0] is not read); band_y (max_side + 1 entries, may be NULL) receives y_n, band_y[0] = H.
 * PMVS_EINVAL for a NULL params, counts or layout, the parameters' ranges above, a negative count;
 * PMVS_EUNSUPPORTED when H exceeds 2^31-1.  pmvs_mesh_atlas calls it on its histogram. */
#define PMVS_ATLAS_MAX_SIDE  251    /* so that a cell is at most 256 texels */
#define PMVS_ATLAS_MAX_WIDTH 65536
typedef struct pmvs_atlas_params {
  int32_t width;     /* W: max_side + 5 .. PMVS_ATLAS_MAX_WIDTH texels */
  int32_t max_side;  /* M: 1 .. PMVS_ATLAS_MAX_SIDE */
  float   scale;     /* finite, > 0: atlas texels per level-0 pixel of a face's longest edge */
} pmvs_atlas_params;

typedef struct pmvs_atlas_layout {
  int64_t width;   /* W */
  int64_t height;  /* H */
  int64_t placed;  /* faces with a triangle in the atlas */
  int64_t cells;   /* square cells in use */
} pmvs_atlas_layout;

typedef struct pmvs_atlas_buffers {  /* any pointer may be NULL: that array is skipped */
  uint8_t* rgb;         /* min(H, height_cap) x W x 3 */
  int32_t* texel_face;  /* min(H, height_cap) x W: the texel's face, -1 = EMPTY */
  float*   uv;          /* nf x 6: the corners in atlas texels */
  int32_t* atlas_view;  /* nf: 0 = placed, -1 = not */
} pmvs_atlas_buffers;

pmvs_status pmvs_mesh_atlas(pmvs_scene* scene, int32_t flags, const pmvs_atlas_params* params, int64_t nv,
                            const float* vertex, int64_t nf, const int32_t* face, const int32_t* view,
                            int64_t height_cap, const pmvs_atlas_buffers* buffers, pmvs_atlas_layout* layout);
pmvs_status pmvs_atlas_layout_from_counts(const pmvs_atlas_params* params, const int64_t* counts,
                                          pmvs_atlas_layout* layout, int64_t* band_y);

/* The .ply / .patch / .pset text of the model, formatted on the device: the bytes pmvs_write_ply /
 * pmvs_write_patches / pmvs_write_pset write from the export of the same records and flags
 * (CPatchOrganizerS::writePLY patchOrganizerS.cpp:687-776, writePatches2 :89-132 with Patch::operator<<
 * patch.cpp:31-48; `ostream << float` at precision 17, the .pset at 6), as one contiguous buffer that the
 * caller writes with one call.  The rows, index2image and the colours come from the export's code; every
 * row is formatted independently, a 64-bit scan of the rows' byte counts places them.
 * flags: PMVS_EXPORT_WRITER_ORDER and PMVS_EXPORT_DEVICE (then `out` is a device pointer on the scene's
 * device) and no other bit.  *bytes receives the text's size; out == NULL with cap == 0 is the size query
 * and writes nothing else.  PMVS_EINVAL: cap smaller than the size (*bytes is set), a kind that is not
 * PMVS_TEXT_*, another flag bit, a NULL scene or a NULL bytes.  Zero patches give the header alone (the
 * .pset has none).  Scratch (the export's arrays, 16 bytes per row and, in host mode, the text) is
 * allocated for the call and freed on return; the work is queued on the scene's stream and the call
 * returns after it has finished. */
#define PMVS_TEXT_PLY 0
#define PMVS_TEXT_PATCH 1
#define PMVS_TEXT_PSET 2
/* Reads the result pmvs_run_loop left on the device (PMVS_EINVAL when there is none) and does not consume
 * it: pmvs_loop_hash, pmvs_loop_fetch, pmvs_loop_export and pmvs_loop_depth_maps still work afterwards. */
pmvs_status pmvs_loop_text(pmvs_scene* scene, int32_t kind, int32_t flags, const int32_t* index2image,
                           char* out, int64_t cap, int64_t* bytes);
/* The same for caller-supplied records: uploaded once and validated as pmvs_export_patches validates
 * them (PMVS_EINVAL). */
pmvs_status pmvs_text_patches(pmvs_scene* scene, const pmvs_patch* patches, int32_t n, int32_t kind, int32_t flags,
                              const int32_t* index2image, char* out, int64_t cap, int64_t* bytes);
/* Self-test of the number formatter the text kernels use (csrc/pmvs_fmt.h): the bytes of
 * printf("%.{precision}g", (double)in[i]) in out + 24 * i (zero-filled behind them) and their number in
 * len[i].  device == -1 runs it on the host, otherwise as a kernel on that device.  precision is 6 or 17
 * (PMVS_EINVAL otherwise). */
pmvs_status pmvs_selftest_format(int32_t device, int32_t precision, const float* in, int32_t n,
                                 char* out /* n x 24 */, int32_t* len /* n */);
/* Self-test of filterSmallGroups' label stage, exactly as the filter pass runs it, on a caller's directed
 * graph in CSR form: the edges of vertex i are i -> edges[e], e in [edge_off[i], edge_off[i + 1]), with
 * edge_off[0] = 0 and every target in [0, n) (PMVS_EINVAL otherwise).  lab_out[j] = the smallest vertex
 * from which j is reachable (j itself included).  stats_out: the number of sets left after contracting
 * the mutual edge pairs, the number of vertices with an edge into another set, and the number of
 * sweeps of the contracted fixpoint. */
pmvs_status pmvs_selftest_labels(int32_t device, int32_t n, const int32_t* edge_off, const int32_t* edges,
                                 int32_t* lab_out /* n */, int32_t* stats_out /* 3 */);

/* The seed phase, PMVS3::CSeed::init + run (seed.cpp:11-107) at CPU 1: target images in the
 * reference's std::shuffle(mt19937(42)) order, cells in raster order, the feature points of every
 * view (points: num_points[0] of view 0, then view 1, ..., as pmvs_detect_features returns them)
 * matched along epipolar lines on the device, and the candidates of a point refined in order of
 * _response (the reference sorts them by heap address, seed.cpp:322: documented deviation) until
 * two succeed (preProcess -> refinePatch -> postProcess, seed.cpp:387-414).  Refinement is batched
 * and speculative; the result equals the sequential one for any batch size.  Runs at depth 0 with
 * the scene's current thresholds (CFindMatch::init values).  Writes the seed patches in addPatch
 * order (at most cap; *n_out = their number) -- the `seeds` input of pmvs_run_loop.  With out = NULL
 * and cap = 0 the scene keeps the seeds and pmvs_seed_fetch copies them out (size the array from
 * *n_out first). */
typedef struct pmvs_seed_stats {
  int64_t trial, pass, fail0, fail1; /* initialMatchSub calls and outcomes (seed.cpp:94-100) */
  int64_t refined;                   /* candidates refined on the device (incl. speculative ones) */
  int64_t rounds;                    /* refine launches */
  int64_t candidates;                /* epipolar candidates collected */
  int64_t reserved;
  double wall_ms, gen_ms, refine_ms; /* whole call, candidate generation, refine batches (wall) */
} pmvs_seed_stats;
pmvs_status pmvs_seed_run(pmvs_scene* scene, const pmvs_point* points, const int32_t* num_points, int32_t batch,
                          pmvs_patch* out, int32_t cap, int32_t* n_out, pmvs_seed_stats* stats);
/* Copies the seeds the last pmvs_seed_run kept (out = NULL, cap = 0) and releases them; n = *n_out. */
pmvs_status pmvs_seed_fetch(pmvs_scene* scene, pmvs_patch* out, int32_t n);

/* Multi-GPU sharding of the expansion: one scene per GPU/rank, all holding the
 * same model.  Each wave's candidates are split into contiguous rank ranges for the refine and
 * the per-candidate results are all-gathered through `fn` before the (replicated) commit.
 * fn(ctx, send, bytes, recv): all-gather of `bytes` from every rank into recv (world * bytes, in
 * rank order), host memory, returns 0 on success; it is called from the thread that called
 * pmvs_expand_run.  world = 1 (or fn = NULL) turns sharding off. */
typedef int (*pmvs_allgather_fn)(void* ctx, const void* send, int64_t bytes, void* recv);
pmvs_status pmvs_scene_set_shard(pmvs_scene* scene, int32_t rank, int32_t world, pmvs_allgather_fn fn, void* ctx);

/* Native RCCL communicator (one process per GPU; librccl.so.1 opened at run time).  Rank 0 calls
 * pmvs_rccl_unique_id and shares the 128 bytes with every rank (any channel); each rank calls
 * pmvs_rccl_create on its device, then pmvs_scene_set_shard_rccl: the expansion's per-wave
 * records are then all-gathered device to device on the scene's stream (ncclAllGather), and the
 * 8-byte error headers through pmvs_rccl_allgather (a pmvs_allgather_fn on host buffers). */
typedef struct pmvs_rccl pmvs_rccl;
pmvs_status pmvs_rccl_unique_id(uint8_t* id128);
pmvs_status pmvs_rccl_create(int32_t device, int32_t rank, int32_t world, const uint8_t* id128, pmvs_rccl** out);
void pmvs_rccl_destroy(pmvs_rccl* comm);
int pmvs_rccl_allgather(void* comm, const void* send, int64_t bytes, void* recv);
int pmvs_rccl_allgather_device(void* comm, const void* dsend, int64_t bytes, void* drecv, void* hip_stream);
pmvs_status pmvs_scene_set_shard_rccl(pmvs_scene* scene, int32_t rank, int32_t world, pmvs_rccl* comm);

/* CMVS cluster per GPU with a boundary exchange.  The reference runs one
 * pmvs2 per cluster option file (genOption.cpp:73-108) and CMVS clusters overlap in their target images
 * (bundle.cpp:1003-1160, ske.dat).  With a cluster set, pmvs_run_loop on this scene (one rank of
 * `world`, one scene per GPU) all-gathers after every iteration but the last, through `fn` (or the
 * native RCCL communicator, device to device), the patches it holds in target images that another
 * rank also has as targets -- a {error, record count} header per rank first, then the records with
 * image NUMBERS.  (CExpand's per-cell _counts are not exchanged: every expansion run starts by clearing
 * them, expand.cpp:32, and the exchange happens between runs; the inserted patches carry the cell
 * occupancy the next run's checkCounts reads.)  Every rank inserts the other ranks' records whose reference
 * image is one of its views as the reference's readPatches inserts another run's patches
 * (patchOrganizerS.cpp:133-197: image numbers mapped to indexes, _vimages cleared, setGrids, addPatch),
 * as fixed patches that are never expanded (fix = PMVS_FIX_FOREIGN): they fill their cells, so the
 * rank does not reconstruct the surface the others already hold there, and they take part in the
 * filters' visibility tests.  Foreign patches are never returned: the final model is this cluster's
 * own patches, and the merged reconstruction is the concatenation of the ranks' models (as the
 * reference's per-cluster .ply files are merged).  image_ids: num_views global image numbers of the
 * scene's views (the option file's timages then oimages).  Collective: every rank calls it (it
 * all-gathers the target lists once).  world = 1 turns it off.  Not combined with a shard. */
pmvs_status pmvs_scene_set_cluster(pmvs_scene* scene, int32_t rank, int32_t world, const int32_t* image_ids,
                                   pmvs_allgather_fn fn, void* ctx);
pmvs_status pmvs_scene_set_cluster_rccl(pmvs_scene* scene, int32_t rank, int32_t world, const int32_t* image_ids,
                                        pmvs_rccl* comm);

/* A host all-gather over TCP among `world` processes (pmvs_hostcomm.cpp): rank 0 listens on addr:port,
 * the other ranks connect (retrying until timeout_ms); pmvs_tcp_allgather is a pmvs_allgather_fn with
 * ctx = the pmvs_tcp.  The multi-rank pmvs2 job's bootstrap (the RCCL unique id travels on it) and its
 * exchange channel when the ranks share one GPU (PMVS_EXCHANGE=tcp).  A rank that exits closes its
 * connection, so its peers' exchanges fail instead of blocking. */
typedef struct pmvs_tcp pmvs_tcp;
pmvs_status pmvs_tcp_create(int32_t rank, int32_t world, const char* addr, int32_t port, int32_t timeout_ms,
                            pmvs_tcp** out);
int pmvs_tcp_allgather(void* ctx, const void* send, int64_t bytes, void* recv);
void pmvs_tcp_destroy(pmvs_tcp* comm);

/* An in-process all-gather among `world` threads (one scene per thread, e.g. several scenes on
 * one GPU): pmvs_thread_allgather with ctx = pmvs_thread_exchange_ctx(group, rank). */
typedef struct pmvs_thread_exchange pmvs_thread_exchange;
pmvs_thread_exchange* pmvs_thread_exchange_create(int32_t world);
void* pmvs_thread_exchange_ctx(pmvs_thread_exchange* group, int32_t rank);
int pmvs_thread_allgather(void* ctx, const void* send, int64_t bytes, void* recv);
void pmvs_thread_exchange_destroy(pmvs_thread_exchange* group);

/* ---------------------------------------------------------------------------------------
 * pmvs2 input / output surface (SURVEY.md §8(b) external boundary, §8 row a19).  Host code;
 * errors are status codes (the reference exits). */

/* Image::CCamera::init + setProjection (camera.cpp:13-54, 256-360): reads a CONTOUR /
 * CONTOUR2 / CONTOUR3 txt file and writes the level-0 3x4 projection (row-major). */
pmvs_status pmvs_camera_load(const char* txt_path, float projection[12]);

/* Binary 8-bit PPM (P6) reader: the PNM path of CImage::readAnyImage (image.cpp:473-506).
 * rgb may be NULL to query the size; otherwise width*height*3 bytes are written. */
pmvs_status pmvs_ppm_load(const char* path, int32_t* width, int32_t* height, uint8_t* rgb);

/* CImage::readAnyImage (image.cpp:473-506) by extension: binary PPM, or JPEG decoded with the
 * image's libjpeg (loaded at run time, as CImg's cimg_use_jpeg path).  rgb may be NULL (size query). */
pmvs_status pmvs_image_load(const char* path, int32_t* width, int32_t* height, uint8_t* rgb);

/* CImage::readPGMImage / readPBMImage (image.cpp:508-670): binary P5 / P4 mask or edge image, raw
 * bytes (P4 bits: 1 -> 0, 0 -> 255).  out may be NULL (size query). */
pmvs_status pmvs_pnm_mask_load(const char* path, int32_t* width, int32_t* height, uint8_t* out);

/* CImage::setEdge (image.cpp:407-460): the edge map the option `setEdge threshold` derives from the
 * level-0 image (width*height bytes, 0/255). */
pmvs_status pmvs_set_edge(const uint8_t* rgb, int32_t width, int32_t height, float threshold, uint8_t* edge_out);

/* PMVS3::SOption (option.cpp:10-307): option file keys and defaults, timages/oimages
 * (enumeration, -1 range, -2 from vis.dat, -3 none), useVisData (vis.dat), useBound
 * (bimages.dat).  Image lists are image NUMBERS; visdata2 is CSR over view indexes
 * (timages first, then oimages); bindexes are target indexes. */
typedef struct pmvs_options {
  int32_t level, csize, wsize, min_image_num, cpu, use_bound, use_vis_data, sequence, tflag, oflag;
  float threshold, set_edge, max_angle /* radians */, quad;
  int32_t num_timages, num_oimages, num_bindexes;
  const int32_t* timages;
  const int32_t* oimages;
  const int32_t* bindexes;
  const int32_t* visdata2_offsets; /* num_timages + num_oimages + 1 */
  const int32_t* visdata2;
} pmvs_options;
pmvs_status pmvs_options_load(const char* prefix, const char* option_file, pmvs_options** out);
void pmvs_options_free(pmvs_options* options);

/* Patch fields for the writers: 11 floats per patch = coord[4], normal[4], ncc, dscale, ascale. */
/* .patch text exactly as CPatchOrganizerS::writePatches2 + Patch::operator<< (patchOrganizerS.cpp:98-116,
 * patch.cpp:31-48); ids/vids are image numbers (index2image applied by the caller). */
pmvs_status pmvs_write_patches(const char* path, int32_t n, const float* fields, const int32_t* nimg,
                               const int32_t* ids, const int32_t* nvimg, const int32_t* vids);
/* .pset text (patchOrganizerS.cpp:118-131). */
pmvs_status pmvs_write_pset(const char* path, int32_t n, const float* fields);
/* ASCII .ply with colour and quality (CPatchOrganizerS::writePLY, patchOrganizerS.cpp:687-776). */
pmvs_status pmvs_write_ply(const char* path, int32_t n, const float* fields, const int32_t* colors);
/* A one-channel PFM image of width x height floats given top row first (one target's `depth` map of
 * pmvs_loop_depth_maps, width = gwidth, height = gheight): the header "Pf\n<width> <height>\n-1.0\n",
 * then the rows from the bottom one to the top one as little-endian float32.  PMVS_EINVAL for a NULL
 * argument, a non-positive size or a file that cannot be written. */
pmvs_status pmvs_write_pfm(const char* path, int32_t width, int32_t height, const float* data);
/* A binary 8-bit PPM of width x height RGB pixels given top row first (pmvs_mesh_atlas's rgb): the header
 * "P6\n<width> <height>\n255\n", then the bytes as given; what pmvs_ppm_load reads back.  PMVS_EINVAL for a
 * NULL argument, a non-positive size or a file that cannot be written. */
pmvs_status pmvs_write_ppm(const char* path, int32_t width, int32_t height, const uint8_t* rgb);
/* writePLY colour mode 0 on the device: mean of CPhotoSetS::getColor over the patch's images at
 * the scene level, floor(c + 0.5) clamped to 255.  images_flat holds nimg[i] view indexes per patch. */
pmvs_status pmvs_patch_colors(pmvs_scene* scene, int32_t n, const float* coords4, const int32_t* nimg,
                              const int32_t* images_flat, int32_t* colors_out);

/* ---------------------------------------------------------------------------------------
 * Synthetic workload generator (NOT a reference interface: the reference ships no data).
 * Textured unit sphere seen by a ring of pinhole cameras. */
typedef struct pmvs_synth_params {
  int32_t num_views;     /* ring cameras */
  int32_t num_targets;   /* candidate reference images are drawn from the first num_targets */
  int32_t width, height; /* level-0 image size */
  int32_t supersample;   /* per-axis supersampling (1..4) */
  int32_t level;         /* option level the candidates are meant for (depth perturbation scale) */
  uint64_t seed;         /* texture seed */
  double ring_radius;    /* camera distance from the sphere centre (4.0) */
  double height_offset;  /* alternating camera height (0.3) */
  double focal_scale;    /* f = focal_scale * width */
  double arc_step_deg;   /* angular spacing of the cameras on the ring (0 = 360/num_views) */
  /* photometrically hard mode (all 0 = the plain scene): per-view gain N(1, gain_sigma) and bias
   * N(0, bias_sigma), per-pixel sensor noise of std noise_sigma (intensities in [0, 1]), low-texture
   * regions where a low-frequency noise field is below `lowtex` (texture contrast x 0.05), and a
   * textured occluding sphere of radius occluder_radius between the ring and the main sphere. */
  double gain_sigma, bias_sigma, noise_sigma, lowtex, occluder_radius;
  /* render only the render_count views render_first, render_first + 1, ... (mod num_views) into rgb
   * (count 0 = all views); projections are written for every view */
  int32_t render_first, render_count;
} pmvs_synth_params;

/* Renders num_views RGB8 images (rgb: num_views*width*height*3 bytes, may be NULL to get only
 * the projections) and writes num_views 3x4 projections (proj: 12 floats per view). */
pmvs_status pmvs_synth_ring(const pmvs_synth_params* p, uint8_t* rgb, float* proj, int32_t nthreads);

/* n seed-path candidates (images = [most frontal target, next most frontal view]). */
pmvs_status pmvs_synth_candidates(const pmvs_synth_params* p, const float* proj, int32_t n, uint64_t seed,
                                  float depth_sigma_px, float max_tilt_deg, pmvs_candidate* out);

#ifdef __cplusplus
}
#endif
#endif /* PMVS_AMD_H */
