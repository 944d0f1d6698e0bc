"""pmvs2's optional TEXMESH export: MESH's mesh (the same volume and parameters, obtained in device mode) with a target
image chosen per face (pmvs_mesh_texture over all targets, depth_rel 0.01, min_area 0), written as
models/<option>.texmesh.ply.  Checked here: that MESH together with TEXMESH writes the .mesh.ply of MESH alone and
adds exactly the one file, that the file parses with the documented header, that its vertices and faces are the
.mesh.ply's, that it names one TextureFile per target image (the files pmvs2 loaded, relative to models/), and
that its texnumber and texcoord equal Scene.mesh_texture followed by the writer's formula on the same loop run
through the library.  The exact values against the definition are the business of tests/test_gpu_mesh_raster.py and
tests/test_gpu_mesh_texture.py."""
import os

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_pmvs2 import _load_cluster, make_dataset
from test_gpu_pmvs2_fuse import CSIZE, H, LEVEL, NUMBERS, W, run
from test_mesh_abi import parse_ply_mesh_binary
from test_texmesh_abi import parse_ply_texmesh_binary, texcoords

pytestmark = pytest.mark.gpu


def test_pmvs2_texmesh_export(gpu_available, tmp_path):
    roots = [str(tmp_path / "mesh"), str(tmp_path / "texmesh")]
    for root in roots:
        make_dataset(root, 3, W, H, LEVEL, CSIZE, 8, numbers=NUMBERS)
    meshed = run(roots[0], "MESH")
    textured = run(roots[1], "MESH", "TEXMESH")
    assert "option-0000.texmesh.ply" not in meshed
    assert sorted(textured) == sorted(list(meshed) + ["option-0000.texmesh.ply"])  # TEXMESH adds exactly this file
    for f in meshed:                                                               # and changes nothing else
        assert textured[f] == meshed[f], f
    v, face = parse_ply_mesh_binary(textured["option-0000.mesh.ply"])
    tex, tv, tf = parse_ply_texmesh_binary(textured["option-0000.texmesh.ply"])
    assert len(v) >= 1 and len(face) >= 1
    assert tv.tobytes() == v.tobytes() and np.array_equal(tf["ids"], face)       # the mesh is MESH's
    # the same loop through the library, as pmvs2 runs it
    import pmvs_amd as P
    opt, nums, inp = _load_cluster(roots[1], "option-0000")
    tnum = inp.num_targets
    files = sorted(os.listdir(os.path.join(roots[1], "visualize")))
    assert tex == ["../visualize/" + next(f for f in files if f.startswith("%08d." % nums[t])) for t in range(tnum)]
    dims = np.array([[inp.images[t].shape[1], inp.images[t].shape[0]] for t in range(tnum)], np.int32)
    assert (dims == (W, H)).all()                                                 # the level-0 sizes
    g = P.Scene(inp)
    try:
        seeds = g.seed_run([g.detect_features(i) for i in range(len(nums))])[0]
        g.run_loop(seeds, inp.threshold, wave=32768, min_candidates=131072, fetch=False)
        prm = dict(writer_order=True, radius=CSIZE, min_support=2, depth_rel=0.01, normal_cos=0.5)
        vol = P.volume_from_points(g.loop_fuse(arrays=("coord",), **prm)["coord"], 256, 3)
        h = g.loop_hash()
        m = g.loop_mesh(vol, float(np.float32(3.0) * np.float32(vol.voxel)), min_obs=1, device=True, **prm)
        t = g.mesh_texture(m["vertex"], m["face"], depth_rel=0.01, min_area=0.0, device=True)
        assert g.loop_hash() == h                                                 # the model is untouched
        m, t = {k: a.cpu().numpy() for k, a in m.items()}, {k: a.cpu().numpy() for k, a in t.items()}
    finally:
        g.close()
    assert v["xyz"].tobytes() == m["vertex"].tobytes() and np.array_equal(face, m["face"])
    assert (t["view"] >= 0).any() and t["view"].max() < tnum
    assert np.array_equal(tf["texnumber"], t["view"])
    assert tf["tex"].tobytes() == texcoords(t["view"], t["uv"], dims).tobytes()
    has = t["view"] >= 0
    assert tf["tex"][has].any() and not tf["tex"][~has].any()
    again = str(tmp_path / "again.ply")
    P.write_ply_texmesh_binary(again, m["vertex"], m["normal"], m["color"], m["face"], t["view"], t["uv"], tex, dims)
    assert open(again, "rb").read() == textured["option-0000.texmesh.ply"]
