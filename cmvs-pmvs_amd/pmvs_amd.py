"""pmvs_amd.py -- host-side Python mirror of the C-ABI in include/pmvs_amd.h (ctypes).

This is the test/bench-facing mirror of the boundary: numpy record dtypes with the exact C
layout of pmvs_candidate / pmvs_refined / pmvs_eval_query / pmvs_tex_query, a Scene wrapper
over pmvs_scene_create/destroy, and the batch entry points.  It never falls back to a CPU
path: if libpmvs_amd.so is missing or a HIP device is absent the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PMVS_AMD_LIB", os.path.join(HERE, "libpmvs_amd.so"))

MAX_IMAGES = 128
MAX_TAU = 16

ACCEPTED, FAIL_PRE, FAIL_POST, FAIL_OVERFLOW = 0, 1, 2, 3
FIX_FOREIGN = 2  # pmvs_patch.fix of another cluster's boundary patch (PMVS_FIX_FOREIGN)

CANDIDATE_DTYPE = np.dtype(
    [("coord", "<f4", 4), ("normal", "<f4", 4), ("dscale", "<f4"), ("num_images", "<i4"),
     ("images", "<i4", MAX_IMAGES)], align=True)
REFINED_DTYPE = np.dtype(
    [("status", "<i4"), ("refine_code", "<i4"), ("evals", "<i4"), ("num_images", "<i4"),
     ("coord", "<f4", 4), ("normal", "<f4", 4), ("ncc", "<f4"), ("dscale", "<f4"), ("ascale", "<f4"),
     ("tmp", "<f4"), ("timages", "<i4"), ("reserved", "<i4"), ("images", "<i4", MAX_IMAGES),
     ("grids", "<i4", (MAX_IMAGES, 2))], align=True)
EVAL_QUERY_DTYPE = np.dtype(
    [("coord", "<f4", 4), ("normal", "<f4", 4), ("dscale", "<f4"), ("num_images", "<i4"),
     ("images", "<i4", MAX_TAU), ("x", "<f8", 3)], align=True)
PATCH_DTYPE = np.dtype(
    [("coord", "<f4", 4), ("normal", "<f4", 4), ("ncc", "<f4"), ("dscale", "<f4"), ("ascale", "<f4"),
     ("tmp", "<f4"), ("timages", "<i4"), ("flag", "<i4"), ("fix", "<i4"), ("num_images", "<i4"),
     ("num_vimages", "<i4"), ("dflag", "<i4"), ("images", "<i2", MAX_IMAGES), ("grids", "<i2", (MAX_IMAGES, 2)),
     ("vimages", "<i2", MAX_IMAGES), ("vgrids", "<i2", (MAX_IMAGES, 2))], align=True)
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("type", "<i4")])  # pmvs_point
TEX_QUERY_DTYPE = np.dtype(
    [("coord", "<f4", 4), ("pxaxis", "<f4", 4), ("pyaxis", "<f4", 4), ("normal", "<f4", 4),
     ("view", "<i4"), ("normalize", "<i4")], align=True)


class ViewDesc(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.c_void_p), ("mask", C.c_void_p),
                ("edge", C.c_void_p), ("projection", C.c_float * 12)]


class SceneDesc(C.Structure):
    _fields_ = [("num_views", C.c_int32), ("num_targets", C.c_int32), ("level", C.c_int32),
                ("csize", C.c_int32), ("wsize", C.c_int32), ("min_image_num", C.c_int32),
                ("threshold", C.c_float), ("max_angle", C.c_float), ("quad_threshold", C.c_float),
                ("sequence", C.c_int32), ("visdata2_offsets", C.c_void_p), ("visdata2", C.c_void_p),
                ("num_bindexes", C.c_int32), ("bindexes", C.c_void_p), ("views", C.POINTER(ViewDesc))]


class Stats(C.Structure):
    _fields_ = [("candidates", C.c_int64), ("accepted", C.c_int64), ("fail_pre", C.c_int64),
                ("fail_post", C.c_int64), ("refine_failed", C.c_int64), ("evals", C.c_int64),
                ("tex_valid", C.c_int64), ("tex_grabs", C.c_int64), ("kernel_ms", C.c_double),
                ("opt_cycles", C.c_int64), ("objective_cycles", C.c_int64), ("rounds", C.c_int64),
                ("chunks", C.c_int64), ("prof", C.c_int64 * 8), ("pre_ms", C.c_double),
                ("refine_ms", C.c_double), ("post_ms", C.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "prof" else getattr(self, k)) for k, _ in self._fields_}


class FilterStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("input", "removed_outside", "removed_exact", "removed_neighbor",
                                          "removed_groups", "kept")] + [("kernel_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ExpandStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("parents", "candidates", "fail_prep", "fail_pre", "fail_post",
                                          "fail_commit", "added", "waves")] + [("wall_ms", C.c_double)] + \
               [(k, C.c_int64) for k in ("refined", "evals", "tex_valid")] + [("refine_ms", C.c_double)] + \
               [("refine_launches", C.c_int64), ("tex_valid_small", C.c_int64), ("refine_ms_small", C.c_double),
                ("refine_launches_small", C.c_int64)]

    WORK = ("wall_ms", "refined", "evals", "tex_valid", "refine_ms", "refine_launches", "tex_valid_small",
            "refine_ms_small", "refine_launches_small")  # timing / per-rank work fields

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LoopIter(C.Structure):
    _fields_ = [("depth", C.c_int32), ("patches", C.c_int32), ("expand", ExpandStats), ("filter", FilterStats),
                ("boundary_sent", C.c_int64), ("boundary_received", C.c_int64), ("boundary_inserted", C.c_int64)]

    def as_dict(self):
        return {"depth": self.depth, "expand": self.expand.as_dict(), "filter": self.filter.as_dict(),
                "patches": self.patches, "boundary": {"sent": self.boundary_sent, "received": self.boundary_received,
                                                      "inserted": self.boundary_inserted}}


class ExportSizes(C.Structure):  # pmvs_export_sizes
    _fields_ = [("patches", C.c_int32), ("reserved", C.c_int32), ("image_entries", C.c_int64),
                ("vimage_entries", C.c_int64)]


class ExportBuffers(C.Structure):  # pmvs_export_buffers
    _fields_ = [(k, C.c_void_p) for k in ("fields", "colors", "image_off", "image_ids", "image_idx", "vimage_off",
                                          "vimage_ids", "source")]


EXPORT_WRITER_ORDER, EXPORT_DEVICE = 1, 2
PIXEL_MAX_RADIUS = 16  # PMVS_PIXEL_MAX_RADIUS
TEXT_PLY, TEXT_PATCH, TEXT_PSET = 0, 1, 2  # PMVS_TEXT_*: the kinds of pmvs_loop_text / pmvs_text_patches


class DepthMapBuffers(C.Structure):  # pmvs_depthmap_buffers
    _fields_ = [(k, C.c_void_p) for k in ("patch", "depth", "normal", "ncc")]


class FuseParams(C.Structure):  # pmvs_fuse_params
    _fields_ = [("radius", C.c_int32), ("min_support", C.c_int32), ("depth_rel", C.c_float), ("normal_cos", C.c_float)]


class FuseBuffers(C.Structure):  # pmvs_fuse_buffers
    _fields_ = [(k, C.c_void_p) for k in ("support_map", "coord", "normal", "color", "support", "pixel", "patch")]


class Volume(C.Structure):  # pmvs_volume
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("dims", C.c_int32 * 3)]


class TsdfParams(C.Structure):  # pmvs_tsdf_params
    _fields_ = [("fuse", FuseParams), ("trunc", C.c_float)]


class TsdfBuffers(C.Structure):  # pmvs_tsdf_buffers
    _fields_ = [(k, C.c_void_p) for k in ("tsdf", "obs", "color")]


class MeshBuffers(C.Structure):  # pmvs_mesh_buffers
    _fields_ = [(k, C.c_void_p) for k in ("vertex", "normal", "color", "face")]


class BrickParams(C.Structure):  # pmvs_brick_params
    _fields_ = [("tsdf", TsdfParams), ("margin", C.c_int32)]


class BrickBuffers(C.Structure):  # pmvs_brick_buffers
    _fields_ = [(k, C.c_void_p) for k in ("brick", "tsdf", "obs", "color")]


class RasterBuffers(C.Structure):  # pmvs_raster_buffers
    _fields_ = [(k, C.c_void_p) for k in ("face", "depth")]


class TextureParams(C.Structure):  # pmvs_texture_params
    _fields_ = [("depth_rel", C.c_float), ("min_area", C.c_float)]


class TextureBuffers(C.Structure):  # pmvs_texture_buffers
    _fields_ = [(k, C.c_void_p) for k in ("view", "uv", "score")]


class AtlasParams(C.Structure):  # pmvs_atlas_params
    _fields_ = [("width", C.c_int32), ("max_side", C.c_int32), ("scale", C.c_float)]


class AtlasLayout(C.Structure):  # pmvs_atlas_layout
    _fields_ = [(k, C.c_int64) for k in ("width", "height", "placed", "cells")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AtlasBuffers(C.Structure):  # pmvs_atlas_buffers
    _fields_ = [(k, C.c_void_p) for k in ("rgb", "texel_face", "uv", "atlas_view")]


ATLAS_MAX_SIDE = 251
ATLAS_MAX_WIDTH = 65536


class SeedStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("trial", "pass_", "fail0", "fail1", "refined", "rounds", "candidates",
                                          "reserved")] + [(k, C.c_double) for k in ("wall_ms", "gen_ms", "refine_ms")]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["pass"] = d.pop("pass_")
        return d


class Options(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("level", "csize", "wsize", "min_image_num", "cpu", "use_bound",
                                          "use_vis_data", "sequence", "tflag", "oflag")] + \
               [(k, C.c_float) for k in ("threshold", "set_edge", "max_angle", "quad")] + \
               [(k, C.c_int32) for k in ("num_timages", "num_oimages", "num_bindexes")] + \
               [(k, C.POINTER(C.c_int32)) for k in ("timages", "oimages", "bindexes", "visdata2_offsets",
                                                      "visdata2")]


class SynthParams(C.Structure):
    _fields_ = [("num_views", C.c_int32), ("num_targets", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("supersample", C.c_int32), ("level", C.c_int32),
                ("seed", C.c_uint64), ("ring_radius", C.c_double), ("height_offset", C.c_double),
                ("focal_scale", C.c_double), ("arc_step_deg", C.c_double), ("gain_sigma", C.c_double),
                ("bias_sigma", C.c_double), ("noise_sigma", C.c_double), ("lowtex", C.c_double),
                ("occluder_radius", C.c_double), ("render_first", C.c_int32), ("render_count", C.c_int32)]


# the photometrically hard synthetic mode (pmvs_synth_params): per-view gain / bias, sensor noise,
# low-texture regions and an occluder, so final NCCs spread over ~0.4-1 and image selection
# (constraintImages, optim.cpp:192-206) and filterOutside gains (filter.cpp:62-71) see values near
# their thresholds
HARD = dict(gain_sigma=0.15, bias_sigma=0.04, noise_sigma=0.08, lowtex=0.5, occluder_radius=0.3)


EXPORTS = ["pmvs_last_error", "pmvs_device_count", "pmvs_scene_create", "pmvs_scene_destroy",
           "pmvs_set_thresholds", "pmvs_scene_get_level", "pmvs_grab_tex", "pmvs_incc_eval",
           "pmvs_refine_batch", "pmvs_refine_batch_device", "pmvs_scene_sync", "pmvs_synth_ring",
           "pmvs_synth_candidates", "pmvs_selftest_math", "pmvs_selftest_bobyqa", "pmvs_camera_load",
           "pmvs_ppm_load", "pmvs_options_load", "pmvs_options_free", "pmvs_write_patches", "pmvs_write_pset",
           "pmvs_write_ply", "pmvs_patch_colors", "pmvs_filter_run",
           "pmvs_expand_run", "pmvs_expand_fetch", "pmvs_run_loop", "pmvs_loop_fetch", "pmvs_loop_hash",
           "pmvs_loop_export_sizes", "pmvs_loop_export", "pmvs_export_patches_sizes", "pmvs_export_patches",
           "pmvs_depth_map_layout", "pmvs_loop_depth_maps", "pmvs_depth_maps_patches", "pmvs_write_pfm",
           "pmvs_pixel_map_layout", "pmvs_loop_pixel_maps", "pmvs_pixel_maps_patches",
           "pmvs_loop_fuse", "pmvs_fuse_patches", "pmvs_write_ply_binary",
           "pmvs_loop_tsdf", "pmvs_tsdf_patches", "pmvs_tsdf_mesh", "pmvs_loop_mesh", "pmvs_mesh_patches",
           "pmvs_volume_from_points", "pmvs_write_ply_mesh_binary",
           "pmvs_loop_brick_tsdf", "pmvs_brick_tsdf_patches", "pmvs_brick_tsdf_mesh", "pmvs_loop_brick_mesh",
           "pmvs_brick_mesh_patches", "pmvs_brick_volume_from_points",
           "pmvs_mesh_raster", "pmvs_mesh_texture", "pmvs_write_ply_texmesh_binary",
           "pmvs_mesh_atlas", "pmvs_atlas_layout_from_counts", "pmvs_write_ppm",
           "pmvs_loop_text", "pmvs_text_patches", "pmvs_selftest_format", "pmvs_selftest_labels",
           "pmvs_scene_set_shard", "pmvs_scene_set_shard_rccl", "pmvs_scene_set_cluster",
           "pmvs_scene_set_cluster_rccl", "pmvs_rccl_unique_id",
           "pmvs_rccl_create", "pmvs_rccl_destroy", "pmvs_rccl_allgather", "pmvs_rccl_allgather_device",
           "pmvs_tcp_create", "pmvs_tcp_allgather", "pmvs_tcp_destroy", "pmvs_thread_exchange_create",
           "pmvs_thread_exchange_ctx", "pmvs_thread_allgather", "pmvs_thread_exchange_destroy", "pmvs_detect_features",
           "pmvs_seed_run", "pmvs_seed_fetch", "pmvs_selftest_lls", "pmvs_image_load", "pmvs_pnm_mask_load", "pmvs_set_edge"]

# int fn(void* ctx, const void* send, int64_t bytes, void* recv): all-gather (pmvs_allgather_fn)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)

_lib = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load libpmvs_amd.so (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not built: run `make -C cmvs-pmvs_amd` (no CPU fallback exists)")
    lib = C.CDLL(path)
    lib.pmvs_last_error.restype = C.c_char_p
    lib.pmvs_device_count.restype = C.c_int32
    lib.pmvs_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int32, C.POINTER(C.c_void_p)]
    lib.pmvs_scene_destroy.argtypes = [C.c_void_p]
    lib.pmvs_scene_destroy.restype = None
    lib.pmvs_set_thresholds.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_int32]
    lib.pmvs_scene_get_level.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.pmvs_grab_tex.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.pmvs_detect_features.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                         C.POINTER(C.c_int32)]
    lib.pmvs_seed_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                  C.POINTER(C.c_int32), C.POINTER(SeedStats)]
    lib.pmvs_seed_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.pmvs_incc_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(Stats)]
    lib.pmvs_refine_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(Stats)]
    lib.pmvs_refine_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.pmvs_scene_sync.argtypes = [C.c_void_p, C.POINTER(Stats)]
    lib.pmvs_synth_ring.argtypes = [C.POINTER(SynthParams), C.c_void_p, C.c_void_p, C.c_int32]
    lib.pmvs_synth_candidates.argtypes = [C.POINTER(SynthParams), C.c_void_p, C.c_int32, C.c_uint64,
                                          C.c_float, C.c_float, C.c_void_p]
    lib.pmvs_selftest_bobyqa.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_void_p, C.POINTER(C.c_double)]
    lib.pmvs_selftest_lls.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.pmvs_selftest_math.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    lib.pmvs_camera_load.argtypes = [C.c_char_p, C.c_void_p]
    lib.pmvs_image_load.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    lib.pmvs_pnm_mask_load.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    lib.pmvs_set_edge.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    lib.pmvs_ppm_load.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
    lib.pmvs_options_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.POINTER(Options))]
    lib.pmvs_options_free.argtypes = [C.POINTER(Options)]
    lib.pmvs_options_free.restype = None
    lib.pmvs_write_patches.argtypes = [C.c_char_p, C.c_int32] + [C.c_void_p] * 5
    lib.pmvs_write_pset.argtypes = [C.c_char_p, C.c_int32, C.c_void_p]
    lib.pmvs_write_ply.argtypes = [C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.pmvs_patch_colors.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    lib.pmvs_filter_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(FilterStats)]
    lib.pmvs_expand_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(ExpandStats)]
    lib.pmvs_expand_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.pmvs_run_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    lib.pmvs_loop_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.pmvs_loop_hash.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    lib.pmvs_loop_export_sizes.argtypes = [C.c_void_p, C.POINTER(ExportSizes)]
    lib.pmvs_loop_export.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(ExportBuffers)]
    lib.pmvs_export_patches_sizes.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(ExportSizes)]
    lib.pmvs_export_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.POINTER(ExportBuffers)]
    lib.pmvs_depth_map_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pmvs_loop_depth_maps.argtypes = [C.c_void_p, C.c_int32, C.POINTER(DepthMapBuffers)]
    lib.pmvs_depth_maps_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(DepthMapBuffers)]
    lib.pmvs_write_pfm.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.pmvs_pixel_map_layout.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.pmvs_loop_pixel_maps.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DepthMapBuffers)]
    lib.pmvs_pixel_maps_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.POINTER(DepthMapBuffers)]
    lib.pmvs_loop_fuse.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FuseParams), C.c_int64,
                                   C.POINTER(FuseBuffers), C.POINTER(C.c_int64)]
    lib.pmvs_fuse_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(FuseParams),
                                      C.c_int64, C.POINTER(FuseBuffers), C.POINTER(C.c_int64)]
    lib.pmvs_write_ply_binary.argtypes = [C.c_char_p, C.c_int64] + [C.c_void_p] * 4
    tsdf_tail = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(TsdfParams), C.POINTER(Volume)]  # flags, range, params, volume
    mesh_tail = [C.c_int32, C.c_int64, C.c_int64, C.POINTER(MeshBuffers), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.pmvs_loop_tsdf.argtypes = [C.c_void_p] + tsdf_tail + [C.POINTER(TsdfBuffers)]
    lib.pmvs_tsdf_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + tsdf_tail + [C.POINTER(TsdfBuffers)]
    lib.pmvs_tsdf_mesh.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Volume), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_int64, C.POINTER(MeshBuffers), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.pmvs_loop_mesh.argtypes = [C.c_void_p] + tsdf_tail + mesh_tail
    lib.pmvs_mesh_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + tsdf_tail + mesh_tail
    lib.pmvs_volume_from_points.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Volume)]
    brick_tail = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(BrickParams), C.POINTER(Volume)]  # flags, range, params, volume
    brick_caps = [C.c_int64, C.POINTER(BrickBuffers), C.POINTER(C.c_int64)]
    lib.pmvs_loop_brick_tsdf.argtypes = [C.c_void_p] + brick_tail + brick_caps
    lib.pmvs_brick_tsdf_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + brick_tail + brick_caps
    lib.pmvs_brick_tsdf_mesh.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Volume), C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p] + mesh_tail[1:]
    lib.pmvs_loop_brick_mesh.argtypes = [C.c_void_p] + brick_tail + mesh_tail
    lib.pmvs_brick_mesh_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + brick_tail + mesh_tail
    lib.pmvs_brick_volume_from_points.argtypes = [C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Volume)]
    lib.pmvs_write_ply_mesh_binary.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    texmesh_tail = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]  # nv, vertex, nf, face
    lib.pmvs_mesh_raster.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + texmesh_tail + [C.POINTER(RasterBuffers)]
    lib.pmvs_mesh_texture.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(TextureParams)] + texmesh_tail + \
                                     [C.POINTER(TextureBuffers)]
    lib.pmvs_write_ply_texmesh_binary.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p),
                                                  C.c_void_p]
    lib.pmvs_mesh_atlas.argtypes = [C.c_void_p, C.c_int32, C.POINTER(AtlasParams)] + texmesh_tail + \
                                   [C.c_void_p, C.c_int64, C.POINTER(AtlasBuffers), C.POINTER(AtlasLayout)]
    lib.pmvs_atlas_layout_from_counts.argtypes = [C.POINTER(AtlasParams), C.c_void_p, C.POINTER(AtlasLayout), C.c_void_p]
    lib.pmvs_write_ppm.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.pmvs_loop_text.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.POINTER(C.c_int64)]
    lib.pmvs_text_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.POINTER(C.c_int64)]
    lib.pmvs_selftest_format.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.pmvs_selftest_labels.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pmvs_scene_set_shard.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.pmvs_scene_set_cluster.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pmvs_scene_set_cluster_rccl.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.pmvs_rccl_unique_id.argtypes = [C.c_void_p]
    lib.pmvs_rccl_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.pmvs_rccl_destroy.argtypes = [C.c_void_p]
    lib.pmvs_rccl_destroy.restype = None
    lib.pmvs_rccl_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.pmvs_rccl_allgather.restype = C.c_int
    lib.pmvs_scene_set_shard_rccl.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.pmvs_tcp_create.argtypes = [C.c_int32, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    lib.pmvs_tcp_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.pmvs_tcp_destroy.argtypes = [C.c_void_p]
    lib.pmvs_tcp_destroy.restype = None
    lib.pmvs_thread_exchange_create.argtypes = [C.c_int32]
    lib.pmvs_thread_exchange_create.restype = C.c_void_p
    lib.pmvs_thread_exchange_ctx.argtypes = [C.c_void_p, C.c_int32]
    lib.pmvs_thread_exchange_ctx.restype = C.c_void_p
    lib.pmvs_thread_allgather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.pmvs_thread_exchange_destroy.argtypes = [C.c_void_p]
    lib.pmvs_thread_exchange_destroy.restype = None
    for fn in EXPORTS:
        getattr(lib, fn).restype = getattr(lib, fn).restype or C.c_int
    lib.pmvs_last_error.restype = C.c_char_p
    lib.pmvs_device_count.restype = C.c_int32
    lib.pmvs_scene_destroy.restype = None
    lib.pmvs_options_free.restype = None
    lib.pmvs_thread_exchange_create.restype = C.c_void_p
    lib.pmvs_thread_exchange_ctx.restype = C.c_void_p
    lib.pmvs_thread_exchange_destroy.restype = None
    lib.pmvs_tcp_destroy.restype = None
    _lib = lib
    return lib


class PmvsError(RuntimeError):
    pass


def _check(status: int):
    if status != 0:
        msg = load_library().pmvs_last_error().decode(errors="replace")
        raise PmvsError(f"pmvs status {status}: {msg}")


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------------- scene
@dataclass
class SceneInputs:
    """Everything pmvs_scene_create needs (SOption + image/camera set), as numpy arrays."""
    images: List[np.ndarray]             # per view uint8 [H, W, 3]
    projections: np.ndarray              # float32 [V, 3, 4] (level 0)
    num_targets: int
    level: int = 1
    csize: int = 2
    wsize: int = 7
    min_image_num: int = 3
    threshold: float = 0.7
    max_angle_deg: Optional[float] = None   # None = SOption default (option.cpp:25)
    quad: float = 2.5
    sequence: int = -1
    visdata2: Optional[List[List[int]]] = None   # None = all-pairs (useVisData 0, option.cpp:204-220)
    bindexes: Sequence[int] = ()
    masks: Optional[List[Optional[np.ndarray]]] = None
    edges: Optional[List[Optional[np.ndarray]]] = None
    _keep: list = field(default_factory=list, repr=False)

    def vis_csr(self):
        V = len(self.images)
        vis = self.visdata2
        if vis is None:
            vis = [[x for x in range(V) if x != y] for y in range(V)]
        off = np.zeros(V + 1, np.int32)
        for i, row in enumerate(vis):
            off[i + 1] = off[i] + len(row)
        flat = np.array([x for row in vis for x in row] or [0], np.int32)
        return off, flat

    def max_angle_rad(self) -> float:
        if self.max_angle_deg is None:
            # SOption(): _maxAngleThreshold = 10.0f * M_PI / 180.0f  (evaluated in double)
            return float(np.float32(np.float64(np.float32(10.0)) * np.pi / np.float64(np.float32(180.0))))
        # SOption::init "maxAngle": _maxAngleThreshold *= M_PI / 180.0f  (float *= double)
        return float(np.float32(np.float64(np.float32(self.max_angle_deg)) * (np.pi / np.float64(np.float32(180.0)))))

    def build_desc(self) -> SceneDesc:
        V = len(self.images)
        self._keep = []
        views = (ViewDesc * V)()
        for i, img in enumerate(self.images):
            img = np.ascontiguousarray(img, dtype=np.uint8)
            assert img.ndim == 3 and img.shape[2] == 3
            self._keep.append(img)
            views[i].width = img.shape[1]
            views[i].height = img.shape[0]
            views[i].rgb = img.ctypes.data
            m = None if self.masks is None else self.masks[i]
            e = None if self.edges is None else self.edges[i]
            if m is not None:
                m = np.ascontiguousarray(m, np.uint8)
                self._keep.append(m)
                views[i].mask = m.ctypes.data
            if e is not None:
                e = np.ascontiguousarray(e, np.uint8)
                self._keep.append(e)
                views[i].edge = e.ctypes.data
            p = np.asarray(self.projections[i], np.float32).reshape(12)
            for k in range(12):
                views[i].projection[k] = float(p[k])
        off, flat = self.vis_csr()
        bidx = np.array(list(self.bindexes) or [0], np.int32)
        self._keep += [off, flat, bidx, views]
        d = SceneDesc()
        d.num_views = V
        d.num_targets = self.num_targets
        d.level = self.level
        d.csize = self.csize
        d.wsize = self.wsize
        d.min_image_num = self.min_image_num
        d.threshold = self.threshold
        d.max_angle = self.max_angle_rad()
        d.quad_threshold = self.quad
        d.sequence = self.sequence
        d.visdata2_offsets = off.ctypes.data
        d.visdata2 = flat.ctypes.data
        d.num_bindexes = len(self.bindexes)
        d.bindexes = bidx.ctypes.data
        d.views = C.cast(views, C.POINTER(ViewDesc))
        return d


class Scene:
    """A device-resident scene on one GPU (pmvs_scene_create)."""

    def __init__(self, inputs: SceneInputs, device: int = 0):
        self.lib = load_library()
        self.inputs = inputs
        self.desc = inputs.build_desc()
        h = C.c_void_p()
        _check(self.lib.pmvs_scene_create(C.byref(self.desc), device, C.byref(h)))
        self.handle = h
        self.device = device
        self.wsize = inputs.wsize

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pmvs_scene_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_thresholds(self, ncc: float, ncc_before: float, depth: int = 0):
        _check(self.lib.pmvs_set_thresholds(self.handle, ncc, ncc_before, depth))

    def get_level(self, view: int, level: int) -> np.ndarray:
        w, h = C.c_int32(), C.c_int32()
        _check(self.lib.pmvs_scene_get_level(self.handle, view, level, None, C.byref(w), C.byref(h)))
        out = np.empty((h.value, w.value, 3), np.uint8)
        _check(self.lib.pmvs_scene_get_level(self.handle, view, level, _ptr(out), C.byref(w), C.byref(h)))
        return out

    def detect_features(self, view: int, fcsize: int = 16) -> np.ndarray:
        """CDetectFeatures::run for one view on the device (pmvs_detect_features): POINT_DTYPE
        records, Harris then DoG, each by decreasing response (the reference's order)."""
        n = C.c_int32(0)
        _check(self.lib.pmvs_detect_features(self.handle, view, fcsize, None, 0, C.byref(n)))
        out = np.zeros(n.value, POINT_DTYPE)
        _check(self.lib.pmvs_detect_features(self.handle, view, fcsize, _ptr(out), n.value, C.byref(n)))
        return out

    def seed_run(self, points, batch: int = 0, cap=None):
        """CSeed::run on the device (pmvs_seed_run) from per-view feature points (POINT_DTYPE arrays,
        or float [n, 4] = x, y, response, type): (seed patches in addPatch order, stats)."""
        flat, npts = points_flat(points)
        n = C.c_int32(0)
        st = SeedStats()
        if cap is None:  # the scene keeps the seeds; fetch exactly their number
            _check(self.lib.pmvs_seed_run(self.handle, _ptr(flat), _ptr(npts), int(batch), None, 0, C.byref(n),
                                          C.byref(st)))
            out = np.zeros(n.value, PATCH_DTYPE)
            _check(self.lib.pmvs_seed_fetch(self.handle, _ptr(out), n.value))
            return out, st.as_dict()
        out = np.zeros(int(cap), PATCH_DTYPE)
        _check(self.lib.pmvs_seed_run(self.handle, _ptr(flat), _ptr(npts), int(batch), _ptr(out), int(cap), C.byref(n),
                                      C.byref(st)))
        return out[:n.value].copy(), st.as_dict()

    def grab_tex(self, q: np.ndarray):
        q = np.ascontiguousarray(q, TEX_QUERY_DTYPE)
        n = len(q)
        out = np.zeros((n, 3 * self.wsize * self.wsize), np.float32)
        valid = np.zeros(n, np.int32)
        _check(self.lib.pmvs_grab_tex(self.handle, _ptr(q), n, _ptr(out), _ptr(valid)))
        return out, valid

    def incc_eval(self, q: np.ndarray):
        q = np.ascontiguousarray(q, EVAL_QUERY_DTYPE)
        n = len(q)
        out = np.zeros(n, np.float64)
        st = Stats()
        _check(self.lib.pmvs_incc_eval(self.handle, _ptr(q), n, _ptr(out), C.byref(st)))
        return out, st.as_dict()

    def refine_batch(self, cands: np.ndarray):
        cands = np.ascontiguousarray(cands, CANDIDATE_DTYPE)
        n = len(cands)
        out = np.zeros(n, REFINED_DTYPE)
        st = Stats()
        _check(self.lib.pmvs_refine_batch(self.handle, _ptr(cands), n, _ptr(out), C.byref(st)))
        return out, st.as_dict()

    def refine_batch_device(self, d_in_ptr: int, n: int, d_out_ptr: int):
        _check(self.lib.pmvs_refine_batch_device(self.handle, C.c_void_p(d_in_ptr), n, C.c_void_p(d_out_ptr)))

    def filter_run(self, patches: np.ndarray):
        """One CFilter::run pass on the device: returns (patches_out, keep, stats)."""
        pa = np.ascontiguousarray(patches, PATCH_DTYPE).copy()
        keep = np.zeros(len(pa), np.int32)
        st = FilterStats()
        _check(self.lib.pmvs_filter_run(self.handle, _ptr(pa), len(pa), _ptr(keep), C.byref(st)))
        return pa, keep, st.as_dict()

    def expand_run(self, patches: np.ndarray, alive=None, wave: int = 1, count_threshold: int = 4, cap=None,
                   after_seeds: bool = False, min_candidates: int = 0, max_waves: int = 0):
        """One CExpand::run on the device (expand.cpp:17-406): returns (patches, alive, stats).

        The result holds the input patches (flags updated) followed by the new ones; `cap` bounds
        its size (default: 2^30).  max_waves > 0 stops after that many waves (bounded parity
        samples; PMVS_EXPAND_MAX_WAVES).  Collective when a shard is set (set_shard)."""
        pa = np.ascontiguousarray(patches, PATCH_DTYPE)
        al = np.ones(len(pa), np.int32) if alive is None else np.ascontiguousarray(alive, np.int32)
        cap = int(cap or (1 << 30))
        n_out = C.c_int32(0)
        st = ExpandStats()
        _check(self.lib.pmvs_expand_run(self.handle, _ptr(pa), _ptr(al), len(pa), wave, min_candidates, count_threshold,
                                        int(after_seeds) | (int(max_waves) << 8), None, None, cap, C.byref(n_out),
                                        C.byref(st)))
        out = np.empty(n_out.value, PATCH_DTYPE)
        aout = np.empty(n_out.value, np.int32)
        _check(self.lib.pmvs_expand_fetch(self.handle, _ptr(out), _ptr(aout), n_out.value))
        return out, aout, st.as_dict()

    def set_shard(self, rank: int, world: int, fn=None, ctx=None):
        """Shard the expansion over `world` ranks (pmvs_scene_set_shard); fn is a C function
        pointer (pmvs_allgather_fn: the library's pmvs_thread_allgather, or an ALLGATHER_FN
        callback such as DistExchange's).  The callback object must outlive the scene's use."""
        self._shard_keep = fn
        ptr = None if fn is None else (fn if isinstance(fn, int) else C.cast(fn, C.c_void_p).value)
        _check(self.lib.pmvs_scene_set_shard(self.handle, rank, world, ptr, ctx))

    def set_cluster(self, rank: int, world: int, image_ids, fn=None, ctx=None):
        """One CMVS cluster of `world` (pmvs_scene_set_cluster): run_loop then exchanges boundary
        patches with the other ranks after every iteration.  image_ids: the global image number of
        each view.  fn: a pmvs_allgather_fn (ThreadExchange.endpoint / DistExchange.fn).  Collective."""
        ids = np.ascontiguousarray(image_ids, np.int32)
        assert len(ids) == len(self.inputs.images)
        self._cluster_keep = (fn, ids)
        ptr = None if fn is None else (fn if isinstance(fn, int) else C.cast(fn, C.c_void_p).value)
        _check(self.lib.pmvs_scene_set_cluster(self.handle, rank, world, _ptr(ids), ptr, ctx))

    def run_loop(self, seeds: np.ndarray, threshold: float, iterations: int = 3, wave: int = 4096, cap=None,
                 after_seeds: bool = True, native: bool = True, min_candidates: int = 0, max_waves: int = 0,
                 fetch: bool = True):
        """CFindMatch::run after the seed phase (findMatch.cpp:196-217): depth 1, then `iterations` x
        (CExpand::run, CFilter::run, updateThreshold, ++depth).  Thresholds follow the reference's
        float arithmetic: before = threshold - 0.3f (findMatch.cpp:104), -= 0.05f per iteration and
        _countThreshold1 4 -> 2 (findMatch.cpp:23-28).  native=True runs the whole loop in the
        library with the model resident in HBM (pmvs_run_loop); native=False composes expand_run
        and filter_run through host memory (same result).  max_waves > 0 bounds every iteration's
        expansion to that many waves (PMVS_EXPAND_MAX_WAVES: bounded full-size parity samples).
        Returns (patches, per-iteration stats).  fetch=False (native only) leaves the result on the
        device and returns (its size, stats): loop_hash() / loop_fetch(n) then read it."""
        model = np.ascontiguousarray(seeds, PATCH_DTYPE)
        if native:
            iters = (LoopIter * max(1, iterations))()
            n_out = C.c_int32(0)
            _check(self.lib.pmvs_run_loop(self.handle, _ptr(model), len(model), float(np.float32(threshold)),
                                          iterations, wave, min_candidates,
                                          (1 if after_seeds else 0) | (int(max_waves) << 8), int(cap or (1 << 30)),
                                          C.byref(n_out), iters))
            log = [iters[t].as_dict() for t in range(iterations)]
            if not fetch:
                return n_out.value, log
            return self.loop_fetch(n_out.value), log
        ncc = np.float32(threshold)
        before = np.float32(ncc - np.float32(0.3))
        cthr, depth = 4, 1
        log = []
        for t in range(iterations):
            self.set_thresholds(float(ncc), float(before), depth)
            model, alive, st_e = self.expand_run(model, wave=wave, count_threshold=cthr, cap=cap,
                                                 after_seeds=after_seeds and t == 0, min_candidates=min_candidates,
                                                 max_waves=max_waves)
            model, keep, st_f = self.filter_run(model)
            model = model[keep == 1]
            log.append({"depth": depth, "expand": st_e, "filter": st_f, "patches": len(model)})
            ncc = np.float32(ncc - np.float32(0.05))
            before = np.float32(before - np.float32(0.05))
            cthr = 2
            depth += 1
        return model, log

    def loop_fetch(self, n: int) -> np.ndarray:
        """pmvs_loop_fetch: the n-patch result of the last run_loop(fetch=False), device to host."""
        out = np.empty(n, PATCH_DTYPE)
        _check(self.lib.pmvs_loop_fetch(self.handle, _ptr(out), n))
        return out

    def loop_hash(self) -> int:
        """pmvs_loop_hash: 64-bit digest of the last run_loop result still on the device."""
        h = C.c_uint64(0)
        _check(self.lib.pmvs_loop_hash(self.handle, C.byref(h)))
        return int(h.value)

    # The arrays of the model-output calls, keyed and ordered as the fields of the C struct that points at
    # them: name -> (dtype, shape); a name in a shape is a size the call supplies to _new_arrays.
    # pmvs_export_buffers: n patches (n1 = n + 1), e image entries, v vimage entries
    EXPORT_ARRAYS = {"fields": ("float32", ("n", 11)), "colors": ("int32", ("n", 3)), "image_off": ("int64", ("n1",)),
                     "image_ids": ("int32", ("e",)), "image_idx": ("int32", ("e",)), "vimage_off": ("int64", ("n1",)),
                     "vimage_ids": ("int32", ("v",)), "source": ("int32", ("n",))}
    # pmvs_depthmap_buffers: c cells (depth maps) or pixels (pixel maps)
    DEPTH_MAP_ARRAYS = {"patch": ("int32", ("c",)), "depth": ("float32", ("c",)), "normal": ("float32", ("c", 3)),
                        "ncc": ("float32", ("c",))}
    # pmvs_fuse_buffers: px pixels of the range, n points
    FUSE_ARRAYS = {"support_map": ("uint8", ("px",)), "coord": ("float32", ("n", 3)), "normal": ("float32", ("n", 3)),
                   "color": ("uint8", ("n", 3)), "support": ("uint8", ("n",)), "pixel": ("int64", ("n",)),
                   "patch": ("int32", ("n",))}
    # pmvs_tsdf_buffers: the volume's nx x ny x nz voxels; pmvs_mesh_buffers: v vertices, f faces
    TSDF_ARRAYS = {"tsdf": ("float32", ("nz", "ny", "nx")), "obs": ("uint8", ("nz", "ny", "nx")),
                   "color": ("uint8", ("nz", "ny", "nx", 4))}
    # pmvs_brick_buffers: b stored bricks of 8 x 8 x 8 voxels, [lk, lj, li]
    BRICK_ARRAYS = {"brick": ("int64", ("b",)), "tsdf": ("float32", ("b", 8, 8, 8)), "obs": ("uint8", ("b", 8, 8, 8)),
                    "color": ("uint8", ("b", 8, 8, 8, 4))}
    MESH_ARRAYS = {"vertex": ("float32", ("v", 3)), "normal": ("float32", ("v", 3)), "color": ("uint8", ("v", 3)),
                   "face": ("int32", ("f", 3))}

    def _new_arrays(self, Buffers, spec, names, device, **sizes):
        """The arrays `names` (None = all) of `spec` (one of the tables above) as numpy arrays or torch
        tensors on the scene's device, and the C struct that points at them (an empty array, and every
        name not asked for, as NULL)."""
        out, buf = {}, Buffers()
        for k in (spec if names is None else names):
            dt, shape = spec[k]
            shape = tuple(sizes[d] if isinstance(d, str) else d for d in shape)
            if device:
                import torch
                out[k] = torch.empty(shape, dtype=getattr(torch, dt), device=torch.device("cuda", self.device))
                setattr(buf, k, out[k].data_ptr() if out[k].numel() else None)
            else:
                out[k] = np.empty(shape, dt)
                setattr(buf, k, out[k].ctypes.data if out[k].size else None)
        return out, buf

    @staticmethod
    def _flags(writer_order: bool, device: bool) -> int:
        return (EXPORT_WRITER_ORDER if writer_order else 0) | (EXPORT_DEVICE if device else 0)

    @staticmethod
    def _records(patches) -> np.ndarray:
        return np.ascontiguousarray(patches, PATCH_DTYPE)

    @staticmethod
    def _index2image(index2image):
        return None if index2image is None else np.ascontiguousarray(index2image, np.int32)

    def _range(self, first_target, num_targets, radius=None):
        """(num_targets, radius) with their defaults: all targets from first_target on, csize."""
        return (self.desc.num_targets - first_target if num_targets is None else num_targets,
                self.desc.csize if radius is None else radius)

    def loop_export_sizes(self) -> dict:
        """pmvs_loop_export_sizes: patches and list entries of the loop result on the device."""
        sz = ExportSizes()
        _check(self.lib.pmvs_loop_export_sizes(self.handle, C.byref(sz)))
        return {"patches": sz.patches, "image_entries": sz.image_entries, "vimage_entries": sz.vimage_entries}

    def _export_call(self, sizes_call, call, writer_order, index2image, device, arrays):
        """sizes_call(byref(sizes)), the arrays they ask for, then call(flags, index2image, byref(buffers))."""
        sz = ExportSizes()
        _check(sizes_call(C.byref(sz)))
        out, buf = self._new_arrays(ExportBuffers, self.EXPORT_ARRAYS, arrays, device, n=sz.patches, n1=sz.patches + 1,
                                    e=sz.image_entries, v=sz.vimage_entries)
        tab = self._index2image(index2image)
        _check(call(self._flags(writer_order, device), _ptr(tab), C.byref(buf)))
        return out

    def loop_export(self, writer_order: bool = True, index2image=None, device: bool = False, arrays=None) -> dict:
        """pmvs_loop_export: the last run_loop(fetch=False) result as compact arrays, keyed by the
        fields of pmvs_export_buffers (fields [n, 11], colors [n, 3], image_off [n + 1], image_ids,
        image_idx, vimage_off [n + 1], vimage_ids, source [n]); rows in the order pmvs2 writes
        (writer_order) or in model order.  Does not consume the result.  index2image: the image number
        of every view (None = the view indexes).  device=True: torch tensors allocated on the scene's
        device and written there (no host copy; import torch before the first Scene when torch ships
        its own HIP runtime, as bench.py does).  arrays: the names wanted (None = all)."""
        return self._export_call(lambda *a: self.lib.pmvs_loop_export_sizes(self.handle, *a),
                                 lambda *a: self.lib.pmvs_loop_export(self.handle, *a), writer_order, index2image, device, arrays)

    def export_patches(self, patches: np.ndarray, writer_order: bool = True, index2image=None, device: bool = False,
                       arrays=None) -> dict:
        """pmvs_export_patches: loop_export's arrays for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        return self._export_call(lambda *a: self.lib.pmvs_export_patches_sizes(self.handle, _ptr(pa), len(pa), *a),
                                 lambda *a: self.lib.pmvs_export_patches(self.handle, _ptr(pa), len(pa), *a), writer_order,
                                 index2image, device, arrays)

    def depth_map_layout(self):
        """pmvs_depth_map_layout: (dims [T, 2] int32 = every target's (gwidth, gheight), offsets [T + 1]
        int64 = the first cell of every target's map, the last entry the total)."""
        tnum = self.desc.num_targets
        dims, off = np.zeros((tnum, 2), np.int32), np.zeros(tnum + 1, np.int64)
        _check(self.lib.pmvs_depth_map_layout(self.handle, _ptr(dims), _ptr(off)))
        return dims, off

    def _depth_map_call(self, call, writer_order, device, arrays):
        out, buf = self._new_arrays(DepthMapBuffers, self.DEPTH_MAP_ARRAYS, arrays, device, c=int(self.depth_map_layout()[1][-1]))
        _check(call(self._flags(writer_order, device), C.byref(buf)))
        return out

    def loop_depth_maps(self, writer_order: bool = True, device: bool = False, arrays=None) -> dict:
        """pmvs_loop_depth_maps: what every target image sees of the last run_loop(fetch=False) result
        (CFilter::setDepthMaps over it), keyed by the fields of pmvs_depthmap_buffers: patch [cells]
        (-1 = empty), depth [cells], normal [cells, 3], ncc [cells]; depth_map_layout() gives the
        cells of each target and depth_map_view one target's image.  `patch` indexes the rows of
        loop_export(writer_order=...) (model order: the records of loop_fetch).  Does not consume the
        result.  device=True: torch tensors on the scene's device, written there.  arrays: the names
        wanted (None = all)."""
        return self._depth_map_call(lambda *a: self.lib.pmvs_loop_depth_maps(self.handle, *a), writer_order, device, arrays)

    def depth_maps_patches(self, patches: np.ndarray, writer_order: bool = True, device: bool = False,
                           arrays=None) -> dict:
        """pmvs_depth_maps_patches: loop_depth_maps' arrays for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        return self._depth_map_call(lambda *a: self.lib.pmvs_depth_maps_patches(self.handle, _ptr(pa), len(pa), *a),
                                    writer_order, device, arrays)

    def pixel_map_layout(self, first_target: int = 0, num_targets=None):
        """pmvs_pixel_map_layout: (dims [n, 2] int32 = the (width, height) of targets [first_target,
        first_target + num_targets) at the scene's level, offsets [n + 1] int64 = the first pixel of each
        target's map relative to the first, the last entry the total).  num_targets None: all from
        first_target on."""
        num, _ = self._range(first_target, num_targets)
        dims, off = np.zeros((max(num, 0), 2), np.int32), np.zeros(max(num, 0) + 1, np.int64)
        _check(self.lib.pmvs_pixel_map_layout(self.handle, first_target, num, _ptr(dims), _ptr(off)))
        return dims, off

    def _pixel_map_call(self, call, writer_order, device, arrays, first_target, num_targets, radius):
        num, radius = self._range(first_target, num_targets, radius)
        out, buf = self._new_arrays(DepthMapBuffers, self.DEPTH_MAP_ARRAYS, arrays, device,
                                    c=int(self.pixel_map_layout(first_target, num)[1][-1]))
        _check(call(self._flags(writer_order, device), first_target, num, radius, C.byref(buf)))
        return out

    def loop_pixel_maps(self, writer_order: bool = True, device: bool = False, arrays=None, first_target: int = 0,
                        num_targets=None, radius=None) -> dict:
        """pmvs_loop_pixel_maps: the last run_loop(fetch=False) result rendered into targets
        [first_target, first_target + num_targets) (None: all from first_target on), one value per pixel
        at the scene's level, every patch a plane element of `radius` pixels (None: csize) around its
        projection; keyed as loop_depth_maps: patch [pixels] (-1 = empty), depth [pixels], normal
        [pixels, 3], ncc [pixels].  pixel_map_layout() of the same range gives each target's pixels and
        depth_map_view one target's image.  Does not consume the result.  device=True: torch tensors on
        the scene's device, written there.  arrays: the names wanted (None = all)."""
        return self._pixel_map_call(lambda *a: self.lib.pmvs_loop_pixel_maps(self.handle, *a), writer_order, device,
                                    arrays, first_target, num_targets, radius)

    def pixel_maps_patches(self, patches: np.ndarray, writer_order: bool = True, device: bool = False, arrays=None,
                           first_target: int = 0, num_targets=None, radius=None) -> dict:
        """pmvs_pixel_maps_patches: loop_pixel_maps' arrays for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        return self._pixel_map_call(lambda *a: self.lib.pmvs_pixel_maps_patches(self.handle, _ptr(pa), len(pa), *a),
                                    writer_order, device, arrays, first_target, num_targets, radius)

    def _fuse_call(self, call, writer_order, device, arrays, first_target, num_targets, radius, min_support, depth_rel,
                   normal_cos):
        num, radius = self._range(first_target, num_targets, radius)
        prm = FuseParams(radius, min_support, depth_rel, normal_cos)
        flags = self._flags(writer_order, device)
        count = C.c_int64(0)
        _check(call(flags, first_target, num, C.byref(prm), 0, C.byref(FuseBuffers()), C.byref(count)))  # the counting call
        n = int(count.value)
        out, buf = self._new_arrays(FuseBuffers, self.FUSE_ARRAYS, arrays, device,
                                    px=int(self.pixel_map_layout(first_target, num)[1][-1]), n=n)
        _check(call(flags, first_target, num, C.byref(prm), n, C.byref(buf), C.byref(count)))
        if int(count.value) != n:
            raise PmvsError(f"the fusion emitted {count.value} points after counting {n}")
        return out

    def loop_fuse(self, writer_order: bool = True, device: bool = False, arrays=None, first_target: int = 0, num_targets=None,
                  radius=None, min_support: int = 2, depth_rel: float = 0.01, normal_cos: float = 0.5) -> dict:
        """pmvs_loop_fuse: the per-pixel maps of the last run_loop(fetch=False) result over targets
        [first_target, first_target + num_targets) (None: all from first_target on) fused into one point
        cloud, keyed by the fields of pmvs_fuse_buffers: support_map [pixels] uint8 (how many other
        targets of the range see each pixel's surface point consistently), and per emitted point coord
        [n, 3], normal [n, 3], color [n, 3] uint8, support [n] uint8, pixel [n] int64 (its index in
        pixel_map_layout() of the range), patch [n] int32.  The arrays are sized by a counting call
        first.  radius None: csize.  A range is fused as if the scene had no other targets, so it is
        not a slice of the full call.  Does not consume the result.  device=True: torch tensors on the
        scene's device, written there.  arrays: the names wanted (None = all)."""
        return self._fuse_call(lambda *a: self.lib.pmvs_loop_fuse(self.handle, *a), writer_order, device, arrays,
                               first_target, num_targets, radius, min_support, depth_rel, normal_cos)

    def fuse_patches(self, patches: np.ndarray, writer_order: bool = True, device: bool = False, arrays=None,
                     first_target: int = 0, num_targets=None, radius=None, min_support: int = 2, depth_rel: float = 0.01,
                     normal_cos: float = 0.5) -> dict:
        """pmvs_fuse_patches: loop_fuse's arrays for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        return self._fuse_call(lambda *a: self.lib.pmvs_fuse_patches(self.handle, _ptr(pa), len(pa), *a), writer_order,
                               device, arrays, first_target, num_targets, radius, min_support, depth_rel, normal_cos)

    def _tsdf_params(self, volume, trunc, writer_order, device, first_target, num_targets, radius, min_support, depth_rel,
                     normal_cos):
        """(flags, first, num, byref(params), byref(volume)): the arguments the TSDF and mesh calls share."""
        num, radius = self._range(first_target, num_targets, radius)
        prm = TsdfParams(FuseParams(radius, min_support, depth_rel, normal_cos), trunc)
        return self._flags(writer_order, device), first_target, num, C.byref(prm), C.byref(volume)

    def _tsdf_call(self, call, volume, device, arrays, shared):
        nx, ny, nz = volume.dims
        out, buf = self._new_arrays(TsdfBuffers, self.TSDF_ARRAYS, arrays, device, nx=nx, ny=ny, nz=nz)
        _check(call(*shared, C.byref(buf)))
        return out

    def loop_tsdf(self, volume: Volume, trunc: float, writer_order: bool = True, device: bool = False, arrays=None,
                  first_target: int = 0, num_targets=None, radius=None, min_support: int = 2, depth_rel: float = 0.01,
                  normal_cos: float = 0.5) -> dict:
        """pmvs_loop_tsdf: the TSDF of `volume` (P.volume(origin, voxel, dims)) integrated from the per-pixel
        maps and the fusion's pass flags of the last run_loop(fetch=False) result over a target range,
        keyed by the fields of pmvs_tsdf_buffers: tsdf [nz, ny, nx] float32 (positive outside, 1 where
        unobserved), obs [nz, ny, nx] uint8 (the targets that observe the voxel), color [nz, ny, nx, 4]
        uint8 (RGBA, A = 255 iff the voxel has a colour).  The other parameters are loop_fuse's.  Does
        not consume the result.  device=True: torch tensors on the scene's device, written there."""
        shared = self._tsdf_params(volume, trunc, writer_order, device, first_target, num_targets, radius, min_support,
                                   depth_rel, normal_cos)
        return self._tsdf_call(lambda *a: self.lib.pmvs_loop_tsdf(self.handle, *a), volume, device, arrays, shared)

    def tsdf_patches(self, patches: np.ndarray, volume: Volume, trunc: float, writer_order: bool = True, device: bool = False,
                     arrays=None, first_target: int = 0, num_targets=None, radius=None, min_support: int = 2,
                     depth_rel: float = 0.01, normal_cos: float = 0.5) -> dict:
        """pmvs_tsdf_patches: loop_tsdf's arrays for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        shared = self._tsdf_params(volume, trunc, writer_order, device, first_target, num_targets, radius, min_support,
                                   depth_rel, normal_cos)
        return self._tsdf_call(lambda *a: self.lib.pmvs_tsdf_patches(self.handle, _ptr(pa), len(pa), *a), volume, device,
                               arrays, shared)

    def _mesh_call(self, call, device, arrays):
        """call(vcap, fcap, byref(buffers), byref(nverts), byref(nfaces)): a counting call, then the arrays."""
        nv, nf = C.c_int64(0), C.c_int64(0)
        _check(call(0, 0, C.byref(MeshBuffers()), C.byref(nv), C.byref(nf)))
        v, f = int(nv.value), int(nf.value)
        out, buf = self._new_arrays(MeshBuffers, self.MESH_ARRAYS, arrays, device, v=v, f=f)
        _check(call(v, f, C.byref(buf), C.byref(nv), C.byref(nf)))
        if (int(nv.value), int(nf.value)) != (v, f):
            raise PmvsError(f"the mesh has {nv.value} vertices and {nf.value} faces after counting {v} and {f}")
        return out

    def tsdf_mesh(self, volume: Volume, tsdf, obs, color=None, min_obs: int = 1, device: bool = False, arrays=None) -> dict:
        """pmvs_tsdf_mesh: the naive-surface-nets mesh of a volume (tsdf and obs [nz, ny, nx], color
        [nz, ny, nx, 4] or None), keyed by the fields of pmvs_mesh_buffers: vertex [nv, 3] and normal
        [nv, 3] float32, color [nv, 3] uint8, face [nf, 3] int32 (vertex ids, outward facing).  A voxel
        counts as observed from min_obs observations on.  The arrays are sized by a counting call first.
        device=True: the volume arrays are torch tensors on the scene's device and so is the mesh."""
        voxels = volume.dims[0] * volume.dims[1] * volume.dims[2]
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            ins = [torch.as_tensor(a, dtype=dt, device=dev).contiguous() if a is not None else None
                   for a, dt in ((tsdf, torch.float32), (obs, torch.uint8), (color, torch.uint8))]
            sizes, ptrs = [0 if a is None else a.numel() for a in ins], [None if a is None else a.data_ptr() for a in ins]
        else:
            ins = [np.ascontiguousarray(a, dt) if a is not None else None
                   for a, dt in ((tsdf, np.float32), (obs, np.uint8), (color, np.uint8))]
            sizes, ptrs = [0 if a is None else a.size for a in ins], [_ptr(a) for a in ins]
        if sizes[:2] != [voxels, voxels] or sizes[2] not in (0, 4 * voxels):
            raise ValueError("tsdf_mesh: the arrays do not have the volume's size")
        flags = self._flags(False, device)
        return self._mesh_call(lambda *a: self.lib.pmvs_tsdf_mesh(self.handle, flags, C.byref(volume), min_obs, *ptrs, *a),
                               device, arrays)

    def loop_mesh(self, volume: Volume, trunc: float, min_obs: int = 1, writer_order: bool = True, device: bool = False,
                  arrays=None, first_target: int = 0, num_targets=None, radius=None, min_support: int = 2,
                  depth_rel: float = 0.01, normal_cos: float = 0.5) -> dict:
        """pmvs_loop_mesh: loop_tsdf then tsdf_mesh in one call, the volume never leaving the device;
        tsdf_mesh's arrays.  The counting call integrates too, so the integration runs twice."""
        shared = self._tsdf_params(volume, trunc, writer_order, device, first_target, num_targets, radius, min_support,
                                   depth_rel, normal_cos)
        return self._mesh_call(lambda *a: self.lib.pmvs_loop_mesh(self.handle, *shared, min_obs, *a), device, arrays)

    def mesh_patches(self, patches: np.ndarray, volume: Volume, trunc: float, min_obs: int = 1, writer_order: bool = True,
                     device: bool = False, arrays=None, first_target: int = 0, num_targets=None, radius=None,
                     min_support: int = 2, depth_rel: float = 0.01, normal_cos: float = 0.5) -> dict:
        """pmvs_mesh_patches: loop_mesh's arrays for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        shared = self._tsdf_params(volume, trunc, writer_order, device, first_target, num_targets, radius, min_support,
                                   depth_rel, normal_cos)
        return self._mesh_call(lambda *a: self.lib.pmvs_mesh_patches(self.handle, _ptr(pa), len(pa), *shared, min_obs, *a),
                               device, arrays)

    def _brick_params(self, volume, trunc, margin, writer_order, device, first_target, num_targets, radius, min_support,
                      depth_rel, normal_cos):
        """(flags, first, num, byref(params), byref(volume)): the arguments the brick calls share."""
        num, radius = self._range(first_target, num_targets, radius)
        prm = BrickParams(TsdfParams(FuseParams(radius, min_support, depth_rel, normal_cos), trunc), margin)
        return self._flags(writer_order, device), first_target, num, C.byref(prm), C.byref(volume)

    def _brick_call(self, call, device, arrays):
        """call(bcap, byref(buffers), byref(nbricks)): a counting call, then the arrays."""
        nb = C.c_int64(0)
        _check(call(0, C.byref(BrickBuffers()), C.byref(nb)))
        b = int(nb.value)
        out, buf = self._new_arrays(BrickBuffers, self.BRICK_ARRAYS, arrays, device, b=b)
        _check(call(b, C.byref(buf), C.byref(nb)))
        if int(nb.value) != b:
            raise PmvsError(f"the volume has {nb.value} bricks after counting {b}")
        return out

    def loop_brick_tsdf(self, volume: Volume, trunc: float, margin: int, writer_order: bool = True, device: bool = False,
                        arrays=None, first_target: int = 0, num_targets=None, radius=None, min_support: int = 2,
                        depth_rel: float = 0.01, normal_cos: float = 0.5) -> dict:
        """pmvs_loop_brick_tsdf: loop_tsdf in a sparse volume of 8 x 8 x 8-voxel bricks: only the bricks within
        `margin` voxels of a fused point's voxel exist.  Keyed by the fields of pmvs_brick_buffers: brick [b]
        int64 (the keys (bk * By + bj) * Bx + bi of the stored bricks, ascending), tsdf and obs [b, 8, 8, 8]
        ([lk, lj, li]; loop_tsdf's values for the voxels inside the volume, (1, 0) for an edge brick's
        overhang), color [b, 8, 8, 8, 4].  `volume` may exceed loop_tsdf's 2^31-1 voxels.  The arrays are
        sized by a counting call first, which selects the bricks too."""
        shared = self._brick_params(volume, trunc, margin, writer_order, device, first_target, num_targets, radius,
                                    min_support, depth_rel, normal_cos)
        return self._brick_call(lambda *a: self.lib.pmvs_loop_brick_tsdf(self.handle, *shared, *a), device, arrays)

    def brick_tsdf_patches(self, patches: np.ndarray, volume: Volume, trunc: float, margin: int, writer_order: bool = True,
                           device: bool = False, arrays=None, first_target: int = 0, num_targets=None, radius=None,
                           min_support: int = 2, depth_rel: float = 0.01, normal_cos: float = 0.5) -> dict:
        """pmvs_brick_tsdf_patches: loop_brick_tsdf's arrays for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        shared = self._brick_params(volume, trunc, margin, writer_order, device, first_target, num_targets, radius,
                                    min_support, depth_rel, normal_cos)
        return self._brick_call(lambda *a: self.lib.pmvs_brick_tsdf_patches(self.handle, _ptr(pa), len(pa), *shared, *a),
                                device, arrays)

    def brick_tsdf_mesh(self, volume: Volume, brick, tsdf, obs, color=None, min_obs: int = 1, device: bool = False,
                        arrays=None) -> dict:
        """pmvs_brick_tsdf_mesh: tsdf_mesh of the virtual volume made of the bricks `brick` (keys, strictly
        ascending; tsdf and obs [b, 8, 8, 8], color [b, 8, 8, 8, 4] or None), in which a voxel of no brick is
        unobserved: tsdf_mesh's arrays, byte for byte those of the bricks scattered into a dense volume.
        device=True: the brick arrays are torch tensors on the scene's device and so is the mesh."""
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            ins = [torch.as_tensor(a, dtype=dt, device=dev).contiguous() if a is not None else None
                   for a, dt in ((brick, torch.int64), (tsdf, torch.float32), (obs, torch.uint8), (color, torch.uint8))]
            sizes = [0 if a is None else a.numel() for a in ins]
            ptrs = [None if a is None or not a.numel() else a.data_ptr() for a in ins]
        else:
            ins = [np.ascontiguousarray(a, dt) if a is not None else None
                   for a, dt in ((brick, np.int64), (tsdf, np.float32), (obs, np.uint8), (color, np.uint8))]
            sizes, ptrs = [0 if a is None else a.size for a in ins], [_ptr(a) for a in ins]
        b = sizes[0]
        if sizes[1:3] != [512 * b, 512 * b] or sizes[3] not in (0, 2048 * b):
            raise ValueError("brick_tsdf_mesh: the arrays do not have the bricks' size")
        flags = self._flags(False, device)
        return self._mesh_call(lambda *a: self.lib.pmvs_brick_tsdf_mesh(self.handle, flags, C.byref(volume), min_obs, b, *ptrs, *a),
                               device, arrays)

    def loop_brick_mesh(self, volume: Volume, trunc: float, margin: int, min_obs: int = 1, writer_order: bool = True,
                        device: bool = False, arrays=None, first_target: int = 0, num_targets=None, radius=None,
                        min_support: int = 2, depth_rel: float = 0.01, normal_cos: float = 0.5) -> dict:
        """pmvs_loop_brick_mesh: loop_brick_tsdf then brick_tsdf_mesh in one call, the bricks never leaving
        the device; tsdf_mesh's arrays.  The counting call selects and integrates too, so both run twice."""
        shared = self._brick_params(volume, trunc, margin, writer_order, device, first_target, num_targets, radius,
                                    min_support, depth_rel, normal_cos)
        return self._mesh_call(lambda *a: self.lib.pmvs_loop_brick_mesh(self.handle, *shared, min_obs, *a), device, arrays)

    def brick_mesh_patches(self, patches: np.ndarray, volume: Volume, trunc: float, margin: int, min_obs: int = 1,
                           writer_order: bool = True, device: bool = False, arrays=None, first_target: int = 0, num_targets=None,
                           radius=None, min_support: int = 2, depth_rel: float = 0.01, normal_cos: float = 0.5) -> dict:
        """pmvs_brick_mesh_patches: loop_brick_mesh's arrays for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        shared = self._brick_params(volume, trunc, margin, writer_order, device, first_target, num_targets, radius,
                                    min_support, depth_rel, normal_cos)
        return self._mesh_call(lambda *a: self.lib.pmvs_brick_mesh_patches(self.handle, _ptr(pa), len(pa), *shared, min_obs, *a),
                               device, arrays)

    # pmvs_raster_buffers: px pixels of the range; pmvs_texture_buffers: f faces
    RASTER_ARRAYS = {"face": ("int32", ("px",)), "depth": ("float32", ("px",))}
    TEXTURE_ARRAYS = {"view": ("int32", ("f",)), "uv": ("float32", ("f", 6)), "score": ("float32", ("f",))}

    def _mesh_inputs(self, vertex, face, device):
        """(nv, vertex pointer, nf, face pointer) of a mesh and the arrays that keep the pointers alive: numpy
        in host mode, torch tensors on the scene's device in device mode (device tensors are taken as they are)."""
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            v = torch.as_tensor(vertex, dtype=torch.float32, device=dev).contiguous().reshape(-1, 3)
            f = torch.as_tensor(face, dtype=torch.int32, device=dev).contiguous().reshape(-1, 3)
            ptrs = [a.data_ptr() if a.numel() else None for a in (v, f)]
        else:
            if hasattr(vertex, "cpu"):
                vertex, face = vertex.cpu().numpy(), face.cpu().numpy()
            v = np.ascontiguousarray(vertex, np.float32).reshape(-1, 3)
            f = np.ascontiguousarray(face, np.int32).reshape(-1, 3)
            ptrs = [_ptr(a) if a.size else None for a in (v, f)]
        return (len(v), ptrs[0], len(f), ptrs[1]), (v, f)

    def mesh_raster(self, vertex, face, device: bool = False, arrays=None, first_target: int = 0, num_targets=None) -> dict:
        """pmvs_mesh_raster: the mesh (vertex [nv, 3] float32, face [nf, 3] int32 vertex ids) rasterised into
        targets [first_target, first_target + num_targets) (None: all from first_target on) at the scene's
        level, keyed by the fields of pmvs_raster_buffers: face [pixels] int32 (the nearest face, -1 = empty)
        and depth [pixels] float32 (its depth, 0 = empty); pixel_map_layout() of the same range gives each
        target's pixels.  Needs no loop result.  device=True: the mesh and the maps are torch tensors on the
        scene's device.  arrays: the names wanted (None = all)."""
        num, _ = self._range(first_target, num_targets)
        mesh, keep = self._mesh_inputs(vertex, face, device)
        out, buf = self._new_arrays(RasterBuffers, self.RASTER_ARRAYS, arrays, device,
                                    px=int(self.pixel_map_layout(first_target, num)[1][-1]))
        _check(self.lib.pmvs_mesh_raster(self.handle, self._flags(False, device), first_target, num, *mesh, C.byref(buf)))
        del keep
        return out

    def mesh_texture(self, vertex, face, depth_rel: float = 0.01, min_area: float = 0.0, device: bool = False, arrays=None,
                     first_target: int = 0, num_targets=None) -> dict:
        """pmvs_mesh_texture: per face of the mesh the target of the range that sees it best -- front-facing,
        its three corners inside the image and not more than depth_rel of their depth behind the mesh's own
        raster, with the largest projected area, at least min_area pixels^2 -- keyed by the fields of
        pmvs_texture_buffers: view [nf] int32 (a scene target index, -1 = none), uv [nf, 6] float32 (the
        corners' (x, y) in level-0 pixels of that target, 0 without one) and score [nf] float32 (the area).
        Needs no loop result.  device=True: the mesh and the arrays are torch tensors on the scene's device.
        arrays: the names wanted (None = all)."""
        num, _ = self._range(first_target, num_targets)
        mesh, keep = self._mesh_inputs(vertex, face, device)
        out, buf = self._new_arrays(TextureBuffers, self.TEXTURE_ARRAYS, arrays, device, f=mesh[2])
        prm = TextureParams(depth_rel, min_area)
        _check(self.lib.pmvs_mesh_texture(self.handle, self._flags(False, device), first_target, num, C.byref(prm), *mesh,
                                          C.byref(buf)))
        del keep
        return out

    # pmvs_atlas_buffers: h written rows of w texels; f faces
    ATLAS_ARRAYS = {"rgb": ("uint8", ("h", "w", 3)), "texel_face": ("int32", ("h", "w")), "uv": ("float32", ("f", 6)),
                    "atlas_view": ("int32", ("f",))}

    def mesh_atlas(self, vertex, face, view, width: int = 8192, max_side: int = 64, scale: float = 1.0, device: bool = False,
                   arrays=None, height_cap=None):
        """pmvs_mesh_atlas: the mesh with mesh_texture's `view` [nf] baked into one atlas `width` texels wide:
        every placed face gets a right triangle of side 1 .. max_side texels (`scale` texels per level-0 pixel
        of its longest edge), two to a cell.  Returns (arrays, layout): the arrays keyed by the fields of
        pmvs_atlas_buffers -- rgb [rows, width, 3] uint8, texel_face [rows, width] int32 (-1 = EMPTY), uv
        [nf, 6] float32 (the corners in atlas texels), atlas_view [nf] int32 (0 = placed, -1 = not) -- and
        the layout {width, height, placed, cells}.  rows = min(height, height_cap) (None: the whole atlas);
        a sizing call comes first.  device=True: the mesh, the views and the arrays are torch tensors on the
        scene's device.  arrays: the names wanted (None = all)."""
        mesh, keep = self._mesh_inputs(vertex, face, device)
        if device:
            import torch
            vw = torch.as_tensor(view, dtype=torch.int32, device=torch.device("cuda", self.device)).contiguous().reshape(-1)
            vptr = vw.data_ptr() if vw.numel() else None
        else:
            vw = np.ascontiguousarray(view.cpu().numpy() if hasattr(view, "cpu") else view, np.int32).reshape(-1)
            vptr = _ptr(vw) if vw.size else None
        if len(vw) != mesh[2]:
            raise ValueError("mesh_atlas takes one view per face")
        prm, layout = AtlasParams(width, max_side, scale), AtlasLayout()
        flags = self._flags(False, device)
        _check(self.lib.pmvs_mesh_atlas(self.handle, flags, C.byref(prm), *mesh, vptr, 0, None, C.byref(layout)))
        rows = int(layout.height) if height_cap is None else min(int(layout.height), int(height_cap))
        out, buf = self._new_arrays(AtlasBuffers, self.ATLAS_ARRAYS, arrays, device, h=rows, w=width, f=mesh[2])
        _check(self.lib.pmvs_mesh_atlas(self.handle, flags, C.byref(prm), *mesh, vptr, rows, C.byref(buf), C.byref(layout)))
        del keep, vw
        return out, layout.as_dict()

    def _text(self, call, writer_order, index2image, device: bool, out):
        """call(flags, index2image, out, cap, byref(size)): a size query, the buffer (numpy uint8, or a torch
        uint8 tensor on the scene's device; `out` supplies it) and the call that fills it; returns the
        buffer cut to the text's size."""
        tab = self._index2image(index2image)
        head = (self._flags(writer_order, device), _ptr(tab))
        size = C.c_int64(0)
        _check(call(*head, None, 0, C.byref(size)))
        n = int(size.value)
        if device:
            import torch
            if out is None:
                out = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", self.device))
            cap, ptr = out.numel(), (out.data_ptr() if out.numel() else None)
        else:
            if out is None:
                out = np.empty(n, np.uint8)
            cap, ptr = out.size, (out.ctypes.data if out.size else None)
        if n > cap:
            raise PmvsError(f"the text has {n} bytes, `out` holds {cap}")
        if n:
            _check(call(*head, ptr, cap, C.byref(size)))
        return out[:n]

    def loop_text(self, kind: int, writer_order: bool = True, index2image=None, device: bool = False, out=None):
        """pmvs_loop_text: the .ply / .patch / .pset text (kind = TEXT_PLY / TEXT_PATCH / TEXT_PSET) of
        the last run_loop(fetch=False) result, formatted on the device: the bytes write_ply /
        write_patches / write_pset write from loop_export of the same flags, as a numpy uint8 array
        (device=True: a torch uint8 tensor on the scene's device, nothing crosses PCIe).  Does not
        consume the result.  out: a uint8 buffer of at least the text's size to use."""
        return self._text(lambda *a: self.lib.pmvs_loop_text(self.handle, kind, *a), writer_order, index2image, device, out)

    def text_patches(self, patches: np.ndarray, kind: int, writer_order: bool = True, index2image=None,
                     device: bool = False, out=None):
        """pmvs_text_patches: loop_text's bytes for caller-supplied PATCH_DTYPE records."""
        pa = self._records(patches)
        return self._text(lambda *a: self.lib.pmvs_text_patches(self.handle, _ptr(pa), len(pa), kind, *a), writer_order,
                          index2image, device, out)

    def patch_colors(self, coords: np.ndarray, images) -> np.ndarray:
        """writePLY colour mode 0 for patches (coords [n,4], images: list of view-index lists)."""
        coords = np.ascontiguousarray(coords, np.float32).reshape(-1, 4)
        nimg = np.array([len(x) for x in images], np.int32)
        flat = np.array([v for x in images for v in x] or [0], np.int32)
        out = np.zeros((len(coords), 3), np.int32)
        _check(self.lib.pmvs_patch_colors(self.handle, len(coords), _ptr(coords), _ptr(nimg), _ptr(flat), _ptr(out)))
        return out

    def sync(self):
        st = Stats()
        _check(self.lib.pmvs_scene_sync(self.handle, C.byref(st)))
        return st.as_dict()


def points_flat(points):
    """Per-view feature points -> (flat POINT_DTYPE array, per-view counts)."""
    parts = []
    for pv in points:
        if isinstance(pv, np.ndarray) and pv.dtype == POINT_DTYPE:
            parts.append(pv)
            continue
        a = np.asarray(pv, np.float32).reshape(-1, 4)
        r = np.zeros(len(a), POINT_DTYPE)
        r["x"], r["y"], r["response"], r["type"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3].astype(np.int32)
        parts.append(r)
    npts = np.array([len(p) for p in parts], np.int32)
    flat = np.concatenate(parts) if parts and npts.sum() else np.zeros(1, POINT_DTYPE)
    return np.ascontiguousarray(flat), npts


def selftest_math(op: int, x: np.ndarray, device: int = 0) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    _check(load_library().pmvs_selftest_math(device, op, _ptr(x), _ptr(out), len(x)))
    return out


def selftest_format(precision: int, x: np.ndarray, device: int = 0):
    """pmvs_selftest_format: the text kernels' number formatter (csrc/pmvs_fmt.h) on float32 values, as a
    list of bytes -- what printf("%.{precision}g") prints; device=-1 runs the same source on the host."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.zeros((len(x), 24), np.uint8)
    ln = np.zeros(len(x), np.int32)
    if len(x):
        _check(load_library().pmvs_selftest_format(device, precision, _ptr(x), len(x), _ptr(out), _ptr(ln)))
    raw = out.tobytes()
    return [raw[24 * i:24 * i + int(k)] for i, k in enumerate(ln)]


def selftest_labels(edge_off: np.ndarray, edges: np.ndarray, device: int = 0):
    """pmvs_selftest_labels: filterSmallGroups' label stage on a directed CSR graph (vertex i's targets are
    edges[edge_off[i]:edge_off[i + 1]]).  Returns (labels, stats): labels[j] = the smallest vertex from which
    j is reachable; stats = {"supernodes", "residual", "sweeps"}."""
    edge_off = np.ascontiguousarray(edge_off, np.int32).reshape(-1)
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1)
    n = len(edge_off) - 1
    lab = np.zeros(max(n, 0), np.int32)
    stats = np.zeros(3, np.int32)
    keep = edges if len(edges) else np.zeros(1, np.int32)
    _check(load_library().pmvs_selftest_labels(device, n, _ptr(edge_off), _ptr(keep), _ptr(lab), _ptr(stats)))
    return lab, {"supernodes": int(stats[0]), "residual": int(stats[1]), "sweeps": int(stats[2])}


def selftest_lls(systems, device: int = 0) -> np.ndarray:
    """Device lls (filterQuad's least squares) on a list of (A [n, 5], b [n]) systems: x [k, 5]."""
    A = np.ascontiguousarray(np.concatenate([np.asarray(a, np.float32).reshape(-1, 5) for a, _ in systems]))
    b = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float32).reshape(-1) for _, v in systems]))
    off = np.zeros(len(systems) + 1, np.int32)
    off[1:] = np.cumsum([len(v) for _, v in systems])
    x = np.zeros((len(systems), 5), np.float32)
    _check(load_library().pmvs_selftest_lls(device, _ptr(A), _ptr(b), _ptr(off), len(systems), _ptr(x)))
    return x


def selftest_bobyqa(kind: int, x0: np.ndarray, mode: int = 0, maxeval: int = 1000, device: int = 0):
    x0 = np.ascontiguousarray(x0, np.float64).reshape(-1, 3)
    out = np.zeros((len(x0), 6), np.float64)
    ms = C.c_double()
    _check(load_library().pmvs_selftest_bobyqa(device, mode, kind, _ptr(x0), len(x0), maxeval, _ptr(out), C.byref(ms)))
    return out, ms.value


# ---------------------------------------------------------------------------------- pmvs2 I/O
def camera_load(path: str) -> np.ndarray:
    """CONTOUR/CONTOUR2/CONTOUR3 txt -> level-0 3x4 projection (pmvs_camera_load)."""
    out = np.zeros(12, np.float32)
    _check(load_library().pmvs_camera_load(path.encode(), _ptr(out)))
    return out.reshape(3, 4)


def ppm_load(path: str) -> np.ndarray:
    lib = load_library()
    w, h = C.c_int32(), C.c_int32()
    _check(lib.pmvs_ppm_load(path.encode(), C.byref(w), C.byref(h), None))
    img = np.zeros((h.value, w.value, 3), np.uint8)
    _check(lib.pmvs_ppm_load(path.encode(), C.byref(w), C.byref(h), _ptr(img)))
    return img


def image_load(path: str) -> np.ndarray:
    """CImage::readAnyImage: PPM or JPEG -> uint8 [H, W, 3] (pmvs_image_load)."""
    lib = load_library()
    w, h = C.c_int32(), C.c_int32()
    _check(lib.pmvs_image_load(path.encode(), C.byref(w), C.byref(h), None))
    img = np.zeros((h.value, w.value, 3), np.uint8)
    _check(lib.pmvs_image_load(path.encode(), C.byref(w), C.byref(h), _ptr(img)))
    return img


def mask_load(path: str) -> np.ndarray:
    """Binary PGM (P5) / PBM (P4) mask or edge image -> uint8 [H, W] (pmvs_pnm_mask_load)."""
    lib = load_library()
    w, h = C.c_int32(), C.c_int32()
    _check(lib.pmvs_pnm_mask_load(path.encode(), C.byref(w), C.byref(h), None))
    m = np.zeros((h.value, w.value), np.uint8)
    _check(lib.pmvs_pnm_mask_load(path.encode(), C.byref(w), C.byref(h), _ptr(m)))
    return m


def set_edge(rgb: np.ndarray, threshold: float) -> np.ndarray:
    """CImage::setEdge (option setEdge): edge map of a level-0 image (pmvs_set_edge)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    out = np.zeros(rgb.shape[:2], np.uint8)
    _check(load_library().pmvs_set_edge(_ptr(rgb), rgb.shape[1], rgb.shape[0], float(threshold), _ptr(out)))
    return out


def options_load(prefix: str, option_file: str) -> dict:
    """pmvs2 option file (+ vis.dat / bimages.dat) -> dict (pmvs_options_load)."""
    lib = load_library()
    p = C.POINTER(Options)()
    _check(lib.pmvs_options_load(prefix.encode(), option_file.encode(), C.byref(p)))
    o = p.contents
    d = {k: getattr(o, k) for k, _ in Options._fields_[:17]}
    num = o.num_timages + o.num_oimages
    d["timages"] = [o.timages[i] for i in range(o.num_timages)]
    d["oimages"] = [o.oimages[i] for i in range(o.num_oimages)]
    d["bindexes"] = [o.bindexes[i] for i in range(o.num_bindexes)]
    off = [o.visdata2_offsets[i] for i in range(num + 1)]
    d["visdata2"] = [[o.visdata2[k] for k in range(off[r], off[r + 1])] for r in range(num)]
    lib.pmvs_options_free(p)
    return d


def _patch_arrays(fields, images, vimages):
    fields = np.ascontiguousarray(fields, np.float32).reshape(-1, 11)
    nimg = np.array([len(x) for x in images], np.int32)
    nv = np.array([len(x) for x in vimages], np.int32)
    ids = np.array([v for x in images for v in x] or [0], np.int32)
    vids = np.array([v for x in vimages for v in x] or [0], np.int32)
    return fields, nimg, ids, nv, vids


def write_patches(path: str, fields, images, vimages):
    f, nimg, ids, nv, vids = _patch_arrays(fields, images, vimages)
    _check(load_library().pmvs_write_patches(path.encode(), len(f), _ptr(f), _ptr(nimg), _ptr(ids), _ptr(nv),
                                             _ptr(vids)))


def write_pset(path: str, fields):
    f = np.ascontiguousarray(fields, np.float32).reshape(-1, 11)
    _check(load_library().pmvs_write_pset(path.encode(), len(f), _ptr(f)))


def write_ply(path: str, fields, colors):
    f = np.ascontiguousarray(fields, np.float32).reshape(-1, 11)
    c = np.ascontiguousarray(colors, np.int32).reshape(-1, 3)
    _check(load_library().pmvs_write_ply(path.encode(), len(f), _ptr(f), _ptr(c)))


def write_ply_binary(path: str, coord, normal, color, support):
    """pmvs_write_ply_binary: a fused point cloud (Scene.loop_fuse's coord, normal, color, support) as one
    binary little-endian PLY of 28-byte vertices."""
    c = np.ascontiguousarray(coord, np.float32).reshape(-1, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    col = np.ascontiguousarray(color, np.uint8).reshape(-1, 3)
    sup = np.ascontiguousarray(support, np.uint8).reshape(-1)
    if not len(c) == len(nm) == len(col) == len(sup):
        raise ValueError("write_ply_binary takes arrays of one length")
    _check(load_library().pmvs_write_ply_binary(path.encode(), len(c), _ptr(c), _ptr(nm), _ptr(col), _ptr(sup)))


def volume(origin, voxel: float, dims) -> Volume:
    """A pmvs_volume: nx x ny x nz = dims voxels of edge `voxel` from the corner `origin`; voxel (i, j, k)
    has index (k * ny + j) * nx + i."""
    return Volume((C.c_float * 3)(*[float(x) for x in origin]), float(voxel), (C.c_int32 * 3)(*[int(x) for x in dims]))


def volume_from_points(coord, cells: int = 256, pad: int = 3) -> Volume:
    """pmvs_volume_from_points: the volume `pmvs2 ... MESH` meshes a cloud in: its bounding box padded by
    `pad` voxels on every side, the voxel the box's longest extent / cells."""
    c = np.ascontiguousarray(coord, np.float32).reshape(-1, 3)
    v = Volume()
    _check(load_library().pmvs_volume_from_points(len(c), _ptr(c), cells, pad, C.byref(v)))
    return v


def brick_volume_from_points(coord, cells: int, pad: int = 3) -> Volume:
    """pmvs_brick_volume_from_points: volume_from_points within the brick volume's limits (dims up to 2^20, a
    brick grid up to 2^31-1): the volume `pmvs2 ... FINEMESH` meshes a cloud in."""
    c = np.ascontiguousarray(coord, np.float32).reshape(-1, 3)
    v = Volume()
    _check(load_library().pmvs_brick_volume_from_points(len(c), _ptr(c), cells, pad, C.byref(v)))
    return v


def write_ply_mesh_binary(path: str, vertex, normal, color, face):
    """pmvs_write_ply_mesh_binary: a mesh (Scene.tsdf_mesh's vertex, normal, color, face) as one binary
    little-endian PLY of 27-byte vertices and 13-byte faces."""
    v = np.ascontiguousarray(vertex, np.float32).reshape(-1, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    col = np.ascontiguousarray(color, np.uint8).reshape(-1, 3)
    f = np.ascontiguousarray(face, np.int32).reshape(-1, 3)
    if not len(v) == len(nm) == len(col):
        raise ValueError("write_ply_mesh_binary takes vertex arrays of one length")
    _check(load_library().pmvs_write_ply_mesh_binary(path.encode(), len(v), _ptr(v), _ptr(nm), _ptr(col), len(f), _ptr(f)))


def write_ply_texmesh_binary(path: str, vertex, normal, color, face, view, uv, tex_files, tex_dims):
    """pmvs_write_ply_texmesh_binary: a mesh with Scene.mesh_texture's view [nf] and uv [nf, 6] as one binary
    little-endian PLY of 27-byte vertices and 42-byte faces (ids, texcoord, texnumber), one `comment
    TextureFile` line per name of tex_files; tex_dims [ntex, 2] = the (width, height) of each texture, which
    scale the level-0 pixel uv to [0, 1] with V up."""
    v = np.ascontiguousarray(vertex, np.float32).reshape(-1, 3)
    nm = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    col = np.ascontiguousarray(color, np.uint8).reshape(-1, 3)
    f = np.ascontiguousarray(face, np.int32).reshape(-1, 3)
    vw = np.ascontiguousarray(view, np.int32).reshape(-1)
    tc = np.ascontiguousarray(uv, np.float32).reshape(-1, 6)
    dims = np.ascontiguousarray(tex_dims, np.int32).reshape(-1, 2)
    if not len(v) == len(nm) == len(col) or not len(f) == len(vw) == len(tc) or len(dims) != len(tex_files):
        raise ValueError("write_ply_texmesh_binary takes vertex arrays of one length, face arrays of one length and one "
                         "(width, height) per texture file")
    names = (C.c_char_p * max(len(tex_files), 1))(*[os.fsencode(n) for n in tex_files])
    _check(load_library().pmvs_write_ply_texmesh_binary(path.encode(), len(v), _ptr(v), _ptr(nm), _ptr(col), len(f), _ptr(f),
                                                        _ptr(vw), _ptr(tc), len(tex_files), names, _ptr(dims)))


def write_pfm(path: str, data):
    """pmvs_write_pfm: a [height, width] float32 image (top row first) as a one-channel PFM."""
    a = np.ascontiguousarray(data, np.float32)
    if a.ndim != 2:
        raise ValueError("write_pfm takes a [height, width] array")
    _check(load_library().pmvs_write_pfm(path.encode(), a.shape[1], a.shape[0], _ptr(a)))


def write_ppm(path: str, rgb):
    """pmvs_write_ppm: a [height, width, 3] uint8 image (top row first) as a binary P6 PPM."""
    a = np.ascontiguousarray(rgb, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("write_ppm takes a [height, width, 3] array")
    _check(load_library().pmvs_write_ppm(path.encode(), a.shape[1], a.shape[0], _ptr(a)))


def atlas_layout_from_counts(counts, width: int, max_side: int, scale: float = 1.0):
    """pmvs_atlas_layout_from_counts: (layout dict, band_y [max_side + 1]) of an atlas whose class n holds
    counts[n] faces (counts has max_side + 1 entries; counts[0] is not read); band_y[0] = the height."""
    c = np.ascontiguousarray(counts, np.int64)
    if c.shape != (max_side + 1,):
        raise ValueError("atlas_layout_from_counts takes max_side + 1 counts")
    prm, layout, band_y = AtlasParams(width, max_side, scale), AtlasLayout(), np.zeros(max_side + 1, np.int64)
    _check(load_library().pmvs_atlas_layout_from_counts(C.byref(prm), _ptr(c), C.byref(layout), _ptr(band_y)))
    return layout.as_dict(), band_y


def depth_map_view(array, dims, offsets, t: int):
    """Target t's (gheight, gwidth[, 3]) view of an array of loop_depth_maps / depth_maps_patches
    (numpy or torch), dims and offsets from depth_map_layout()."""
    gw, gh = int(dims[t][0]), int(dims[t][1])
    part = array[int(offsets[t]):int(offsets[t + 1])]
    return part.reshape((gh, gw) + tuple(part.shape[1:]))


def patches_from_refined(refined: np.ndarray) -> np.ndarray:
    """Accepted pmvs_refined records -> pmvs_patch records (the CPatch fields a filter pass reads)."""
    acc = refined[refined["status"] == ACCEPTED]
    p = np.zeros(len(acc), PATCH_DTYPE)
    for f in ("coord", "normal", "ncc", "dscale", "ascale", "tmp", "timages", "num_images", "images"):
        p[f] = acc[f]
    p["grids"] = grid16(acc["grids"])
    return p


def grid16(g):
    """Cell coordinates as pmvs_patch stores them (int16): values outside [-32767, 32767] -- only
    projections far outside the image, so outside every cell grid -- become -32768 (pmvs_layout.h)."""
    g = np.asarray(g, np.int64)
    return np.where((g < -32767) | (g > 32767), -32768, g).astype(np.int16)


def device_count() -> int:
    return int(load_library().pmvs_device_count())


# ---------------------------------------------------------------------------------- synthetic data
def synth_params(num_views: int, width: int, height: int, num_targets: Optional[int] = None,
                 supersample: int = 2, level: int = 1, seed: int = 0x504D5653,
                 ring_radius: float = 4.0, height_offset: float = 0.3, focal_scale: float = 1.16,
                 arc_step_deg: Optional[float] = None, hard: bool = False) -> SynthParams:
    p = SynthParams()
    p.num_views = num_views
    p.num_targets = num_views if num_targets is None else num_targets
    p.width, p.height = width, height
    p.supersample = supersample
    p.level = level
    p.seed = seed
    p.ring_radius, p.height_offset, p.focal_scale = ring_radius, height_offset, focal_scale
    # cameras every min(360/V, 15) degrees: a full ring for V >= 24, an arc otherwise
    p.arc_step_deg = min(360.0 / num_views, 15.0) if arc_step_deg is None else arc_step_deg
    for k, v in (HARD if hard else {}).items():
        setattr(p, k, v)
    return p


def synth_ring(p: SynthParams, nthreads: int = 8, render: bool = True):
    """(rgb of the rendered views -- all, or p.render_count from p.render_first --, every view's projection)."""
    lib = load_library()
    proj = np.zeros((p.num_views, 3, 4), np.float32)
    count = p.render_count if p.render_count > 0 else p.num_views
    rgb = np.zeros((count, p.height, p.width, 3), np.uint8) if render else None
    _check(lib.pmvs_synth_ring(C.byref(p), _ptr(rgb), _ptr(proj), nthreads))
    return rgb, proj


def synth_candidates(p: SynthParams, proj: np.ndarray, n: int, seed: int = 0x5EED,
                     depth_sigma_px: float = 1.0, max_tilt_deg: float = 10.0) -> np.ndarray:
    lib = load_library()
    out = np.zeros(n, CANDIDATE_DTYPE)
    proj = np.ascontiguousarray(proj, np.float32)
    _check(lib.pmvs_synth_candidates(C.byref(p), _ptr(proj), n, seed, depth_sigma_px, max_tilt_deg, _ptr(out)))
    return out


def synth_scene(num_views: int, width: int, height: int, level: int = 1, num_targets: Optional[int] = None,
                supersample: int = 2, nthreads: int = 8, seed: int = 0x504D5653, hard: bool = False,
                arc_step_deg: Optional[float] = None, **opts) -> SceneInputs:
    p = synth_params(num_views, width, height, num_targets=num_targets, supersample=supersample, level=level,
                     seed=seed, hard=hard, arc_step_deg=arc_step_deg)
    rgb, proj = synth_ring(p, nthreads=nthreads)
    return SceneInputs(images=[rgb[i] for i in range(num_views)], projections=proj,
                       num_targets=p.num_targets, level=level, **opts), p


class ThreadExchange:
    """In-process all-gather among `world` threads (pmvs_thread_exchange): scene r of a group uses
    set_shard(r, world, *group.endpoint(r)).  Used to run several sharded scenes on one GPU."""

    def __init__(self, world: int):
        self.lib = load_library()
        self.world = world
        self.handle = self.lib.pmvs_thread_exchange_create(world)
        if not self.handle:
            raise PmvsError("pmvs_thread_exchange_create failed")

    def endpoint(self, rank: int):
        fn = C.cast(self.lib.pmvs_thread_allgather, C.c_void_p).value
        return fn, self.lib.pmvs_thread_exchange_ctx(self.handle, rank)

    def close(self):
        if self.handle:
            self.lib.pmvs_thread_exchange_destroy(self.handle)
            self.handle = None


class RcclExchange:
    """Native RCCL communicator of the sharded expansion (pmvs_rccl_*): one process per GPU; the
    per-wave records go device to device on the scene's stream.  Rank 0 creates the 128-byte id
    (unique_id()) and every rank receives it (e.g. torch.distributed.broadcast_object_list)."""

    def __init__(self, rank: int, world: int, uid: bytes, device: int = 0):
        self.lib = load_library()
        self.rank, self.world = rank, world
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        h = C.c_void_p()
        _check(self.lib.pmvs_rccl_create(device, rank, world, buf, C.byref(h)))
        self.handle = h

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _check(load_library().pmvs_rccl_unique_id(buf))
        return bytes(buf)

    def allgather(self, data: bytes) -> bytes:
        n = len(data)
        out = (C.c_uint8 * (n * self.world))()
        src = (C.c_uint8 * max(1, n)).from_buffer_copy(data if n else b"\0")
        if self.lib.pmvs_rccl_allgather(self.handle, src, n, out) != 0:
            raise PmvsError("pmvs_rccl_allgather failed")
        return bytes(out)

    def attach(self, scene: "Scene"):
        _check(self.lib.pmvs_scene_set_shard_rccl(scene.handle, self.rank, self.world, self.handle))

    def attach_cluster(self, scene: "Scene", image_ids):
        """The scene is this rank's CMVS cluster; its boundary patches go device to device over RCCL."""
        ids = np.ascontiguousarray(image_ids, np.int32)
        scene._cluster_keep = (None, ids)
        _check(self.lib.pmvs_scene_set_cluster_rccl(scene.handle, self.rank, self.world, _ptr(ids), self.handle))

    def close(self):
        if self.handle:
            self.lib.pmvs_rccl_destroy(self.handle)
            self.handle = None


class DistExchange:
    """pmvs_allgather_fn over torch.distributed: one process per GPU (RCCL over xGMI when the
    process group's backend is nccl; gloo on CPUs).  The host buffer of each expansion wave is
    staged through a device tensor for RCCL.  Keep the object alive while the scene uses it."""

    def __init__(self, group=None, device=None):
        import torch
        import torch.distributed as dist
        self.dist, self.torch, self.group = dist, torch, group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        backend = dist.get_backend(group)
        self.device = device if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu"))
        self.error = None
        self.fn = ALLGATHER_FN(self._allgather)

    def _allgather(self, ctx, send, nbytes, recv):
        try:
            torch = self.torch
            src = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(nbytes,))
            t = torch.from_numpy(src.copy()).to(self.device)
            if self.device.type == "cpu":  # gloo: list form
                parts = [torch.empty_like(t) for _ in range(self.world)]
                self.dist.all_gather(parts, t, group=self.group)
                res = torch.cat(parts).numpy()
            else:
                out = torch.empty(nbytes * self.world, dtype=torch.uint8, device=self.device)
                self.dist.all_gather_into_tensor(out, t, group=self.group)
                res = out.cpu().numpy()
            C.memmove(recv, res.ctypes.data, nbytes * self.world)
            return 0
        except Exception as e:  # reported by pmvs_expand_run as a failed exchange
            self.error = e
            return -1

    def attach(self, scene: "Scene"):
        scene.set_shard(self.rank, self.world, self.fn, None)
