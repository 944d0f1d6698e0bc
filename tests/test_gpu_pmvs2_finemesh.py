"""pmvs2's optional FINEMESH export: FUSE's maps meshed in a sparse volume of 8 x 8 x 8-voxel bricks at image
resolution (pmvs_loop_brick_mesh with FUSE's parameters in pmvs_brick_volume_from_points(fused cloud, cells, 3),
cells = min(4096, the largest level-image width or height over the targets), trunc = 3 voxels, margin 5, min_obs 1,
writer order), written as models/<option>.finemesh.ply.  Checked here: that FINEMESH adds exactly that file and
leaves MESH's file and every other unchanged in the same run, and that the file's arrays equal
Scene.loop_brick_mesh of the same loop run through the library with the documented parameters, byte for byte."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_pmvs2 import _load_cluster, make_dataset
from test_gpu_pmvs2_fuse import CSIZE, H, LEVEL, NUMBERS, W, run
from test_mesh_abi import parse_ply_mesh_binary

pytestmark = pytest.mark.gpu


def test_pmvs2_finemesh_export(gpu_available, tmp_path):
    roots = [str(tmp_path / "mesh"), str(tmp_path / "fine")]
    for root in roots:
        make_dataset(root, 3, W, H, LEVEL, CSIZE, 8, numbers=NUMBERS)
    meshed = run(roots[0], "PATCH", "FUSE", "MESH")
    fine = run(roots[1], "PATCH", "FUSE", "MESH", "FINEMESH")
    assert "option-0000.finemesh.ply" not in meshed
    assert sorted(fine) == sorted(list(meshed) + ["option-0000.finemesh.ply"])   # FINEMESH adds exactly this file
    for f in meshed:                                                               # MESH's file included
        assert fine[f] == meshed[f], f
    v, face = parse_ply_mesh_binary(fine["option-0000.finemesh.ply"])
    assert len(v) >= 1 and len(face) >= 1 and face.min() >= 0 and face.max() < len(v)
    assert np.isfinite(v["xyz"]).all() and np.isfinite(v["n"]).all()
    import pmvs_amd as P
    opt, nums, inp = _load_cluster(roots[1], "option-0000")
    g = P.Scene(inp)
    try:
        seeds = g.seed_run([g.detect_features(i) for i in range(len(nums))])[0]
        g.run_loop(seeds, inp.threshold, wave=32768, min_candidates=131072, fetch=False)
        prm = dict(writer_order=True, radius=CSIZE, min_support=2, depth_rel=0.01, normal_cos=0.5)
        cloud = g.loop_fuse(**prm)
        dims = g.pixel_map_layout()[0]
        cells = min(4096, int(np.max(dims)))
        assert cells == max(W, H) >> LEVEL
        vol = P.brick_volume_from_points(cloud["coord"], cells, 3)
        assert max(vol.dims) in (cells + 6, cells + 7)
        trunc = float(np.float32(3.0) * np.float32(vol.voxel))
        h = g.loop_hash()
        m = g.loop_brick_mesh(vol, trunc, 5, min_obs=1, **prm)
        assert g.loop_hash() == h
    finally:
        g.close()
    assert v["xyz"].tobytes() == m["vertex"].tobytes() and v["n"].tobytes() == m["normal"].tobytes()
    assert np.array_equal(v["rgb"], m["color"]) and np.array_equal(face, m["face"])
    # a finer volume than MESH's 256 cells would be at full size; here the images are small, so only that it differs
    assert fine["option-0000.finemesh.ply"] != fine["option-0000.mesh.ply"]
