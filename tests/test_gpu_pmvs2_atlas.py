"""pmvs2's optional ATLAS export: TEXMESH's mesh and views (the same calls, in device mode) baked by pmvs_mesh_atlas at
the defaults (width 8192, max_side 64, scale 1) into models/<option>.atlas.ppm, with models/<option>.atlas.ply naming
that one texture.  Checked here: that MESH TEXMESH together with ATLAS writes the files of MESH TEXMESH alone, byte for
byte, and adds exactly the two; that the .ppm loads with pmvs_ppm_load at the layout's size and equals the library
call's rgb on the same loop run; that the .ply has exactly one `comment TextureFile` line, the 42-byte face records,
texnumber 0 or -1 only, and the writer's texture coordinates of the library's atlas uv.  The exact values against the
definition are the business of tests/test_gpu_mesh_atlas.py."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_pmvs2 import _load_cluster, make_dataset
from test_gpu_pmvs2_fuse import CSIZE, H, LEVEL, NUMBERS, W, run
from test_texmesh_abi import FACE_DTYPE, parse_ply_texmesh_binary, texcoords

pytestmark = pytest.mark.gpu

ATLAS = dict(width=8192, max_side=64, scale=1.0)


def test_pmvs2_atlas_export(gpu_available, tmp_path):
    roots = [str(tmp_path / "texmesh"), str(tmp_path / "atlas")]
    for root in roots:
        make_dataset(root, 3, W, H, LEVEL, CSIZE, 8, numbers=NUMBERS)
    textured = run(roots[0], "MESH", "TEXMESH")
    baked = run(roots[1], "MESH", "TEXMESH", "ATLAS")
    new = ["option-0000.atlas.ply", "option-0000.atlas.ppm"]
    assert not set(new) & set(textured)
    assert sorted(baked) == sorted(list(textured) + new)                          # ATLAS adds exactly these files
    for f in textured:                                                           # and changes nothing else
        assert baked[f] == textured[f], f
    assert "option-0000.mesh.ply" in textured and "option-0000.texmesh.ply" in textured
    raw = baked["option-0000.atlas.ply"]
    assert raw.count(b"comment TextureFile ") == 1
    tex, av, af = parse_ply_texmesh_binary(raw)
    _, tv, tf = parse_ply_texmesh_binary(baked["option-0000.texmesh.ply"])
    assert tex == ["option-0000.atlas.ppm"] and FACE_DTYPE.itemsize == 42
    assert av.tobytes() == tv.tobytes() and np.array_equal(af["ids"], tf["ids"])  # the mesh is TEXMESH's
    assert set(np.unique(af["texnumber"])) <= {0, -1} and (af["texnumber"] == 0).any()
    assert not (af["texnumber"] == 0)[tf["texnumber"] < 0].any()                  # no texels without an image
    # the same loop through the library, as pmvs2 runs it
    import os
    import pmvs_amd as P
    img = P.ppm_load(os.path.join(roots[1], "models", "option-0000.atlas.ppm"))
    opt, nums, inp = _load_cluster(roots[1], "option-0000")
    g = P.Scene(inp)
    try:
        seeds = g.seed_run([g.detect_features(i) for i in range(len(nums))])[0]
        g.run_loop(seeds, inp.threshold, wave=32768, min_candidates=131072, fetch=False)
        prm = dict(writer_order=True, radius=CSIZE, min_support=2, depth_rel=0.01, normal_cos=0.5)
        vol = P.volume_from_points(g.loop_fuse(arrays=("coord",), **prm)["coord"], 256, 3)
        h = g.loop_hash()
        m = g.loop_mesh(vol, float(np.float32(3.0) * np.float32(vol.voxel)), min_obs=1, device=True, **prm)
        t = g.mesh_texture(m["vertex"], m["face"], depth_rel=0.01, min_area=0.0, device=True)
        a, layout = g.mesh_atlas(m["vertex"], m["face"], t["view"], device=True, **ATLAS)
        assert g.loop_hash() == h                                                 # the model is untouched
        a = {k: x.cpu().numpy() for k, x in a.items()}
        view = t["view"].cpu().numpy()
    finally:
        g.close()
    assert layout["width"] == 8192 and layout["height"] > 0 and 0 < layout["placed"] <= (view >= 0).sum()
    assert img.shape == (layout["height"], layout["width"], 3) and img.tobytes() == a["rgb"].tobytes() and img.any()
    assert np.array_equal(af["texnumber"], a["atlas_view"])
    dims = np.array([[layout["width"], layout["height"]]], np.int32)
    assert af["tex"].tobytes() == texcoords(a["atlas_view"], a["uv"], dims).tobytes()
    has = a["atlas_view"] == 0
    assert af["tex"][has].any() and not af["tex"][~has].any()
