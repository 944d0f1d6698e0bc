"""pmvs2's optional MESH export: FUSE's maps integrated into a TSDF volume and meshed by naive surface nets
(pmvs_loop_mesh with FUSE's parameters in pmvs_volume_from_points(fused cloud, 256, 3), trunc = 3 voxels,
min_obs 1, writer order), written as models/<option>.mesh.ply.  Checked here: the file, its name, header and
size, that the run without MESH writes no such file and that MESH changes nothing else, and that the file's
arrays equal Scene.loop_mesh of the same loop run through the library (features, seeds and loop as pmvs2 runs
them) with the documented default volume, byte for byte.  The exact values against the definition are the
business of tests/test_gpu_tsdf.py and tests/test_gpu_mesh.py."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_fuse_abi import parse_ply_binary
from test_gpu_pmvs2 import _load_cluster, make_dataset
from test_gpu_pmvs2_fuse import CSIZE, H, LEVEL, NUMBERS, W, run
from test_mesh_abi import parse_ply_mesh_binary

pytestmark = pytest.mark.gpu


def test_pmvs2_mesh_export(gpu_available, tmp_path):
    roots = [str(tmp_path / "fuse"), str(tmp_path / "mesh")]
    for root in roots:
        make_dataset(root, 3, W, H, LEVEL, CSIZE, 8, numbers=NUMBERS)
    fused = run(roots[0], "PATCH", "FUSE")
    meshed = run(roots[1], "PATCH", "FUSE", "MESH")
    assert "option-0000.mesh.ply" not in fused                  # without MESH no such file
    assert sorted(meshed) == sorted(list(fused) + ["option-0000.mesh.ply"])  # MESH adds exactly this file
    for f in fused:                                             # and changes nothing else
        assert meshed[f] == fused[f], f
    v, face = parse_ply_mesh_binary(meshed["option-0000.mesh.ply"])
    assert len(v) >= 1 and len(face) >= 1
    assert np.isfinite(v["xyz"]).all() and np.isfinite(v["n"]).all()
    assert face.min() >= 0 and face.max() < len(v)
    # the same loop through the library, as pmvs2 runs it
    import pmvs_amd as P
    opt, nums, inp = _load_cluster(roots[1], "option-0000")
    g = P.Scene(inp)
    try:
        seeds = g.seed_run([g.detect_features(i) for i in range(len(nums))])[0]
        g.run_loop(seeds, inp.threshold, wave=32768, min_candidates=131072, fetch=False)
        prm = dict(writer_order=True, radius=CSIZE, min_support=2, depth_rel=0.01, normal_cos=0.5)
        cloud = g.loop_fuse(**prm)
        assert parse_ply_binary(meshed["option-0000.fused.ply"])["xyz"].tobytes() == cloud["coord"].tobytes()
        vol = P.volume_from_points(cloud["coord"], 256, 3)      # the documented default volume
        assert max(vol.dims) in (262, 263)
        trunc = float(np.float32(3.0) * np.float32(vol.voxel))
        h = g.loop_hash()
        m = g.loop_mesh(vol, trunc, min_obs=1, **prm)
        # the two stages apart, the volume staying on the device: the same mesh, and the model untouched
        v3 = g.loop_tsdf(vol, trunc, device=True, **prm)
        assert v3["tsdf"].shape == (vol.dims[2], vol.dims[1], vol.dims[0]) and int((v3["obs"] > 0).sum()) > 0
        m2 = g.tsdf_mesh(vol, v3["tsdf"], v3["obs"], v3["color"], min_obs=1, device=True)
        for k in m:
            assert m2[k].cpu().numpy().tobytes() == m[k].tobytes(), k
        assert g.loop_hash() == h
    finally:
        g.close()
    assert v["xyz"].tobytes() == m["vertex"].tobytes() and v["n"].tobytes() == m["normal"].tobytes()
    assert np.array_equal(v["rgb"], m["color"]) and np.array_equal(face, m["face"])
    again = str(tmp_path / "again.ply")
    P.write_ply_mesh_binary(again, m["vertex"], m["normal"], m["color"], m["face"])
    assert open(again, "rb").read() == meshed["option-0000.mesh.ply"]
