"""pmvs2's optional FUSE export: the written model's per-pixel maps over all target images fused into one
binary PLY (pmvs_loop_fuse at radius csize, min_support 2, depth_rel 0.01, normal_cos 0.5, writer order).
Checked here: the file, its name, header and size, finite contents, that the other outputs do not change,
and that the file equals write_ply_binary of Scene.fuse_patches over the records of the written .patch
model: the .patch rows are in writer order already, so they are fused in model order (the text carries no
grids to sort by, and needs none).  The exact values against the definition are the business of
tests/test_gpu_fuse.py."""
import os
import subprocess

import numpy as np
import pytest

from test_fuse_abi import parse_ply_binary
from test_gpu_pmvs2 import PMVS2, make_dataset

pytestmark = pytest.mark.gpu

NUMBERS = [0, 3, 7]  # image numbers that are not the view indexes
W, H, LEVEL, CSIZE = 640, 480, 2, 4


def run(root, *keywords):
    r = subprocess.run([PMVS2, root + "/", "option-0000", *keywords], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    models = os.path.join(root, "models")
    return {f: open(os.path.join(models, f), "rb").read() for f in sorted(os.listdir(models))}


def patch_records(P, text, numbers):
    """The records of a .patch file (Patch::operator<<: coord, normal, ncc dscale ascale, the image and
    vimage lists by image number), in the file's order."""
    tok = text.split()
    assert tok[0] == b"PATCHES"
    recs = np.zeros(int(tok[1]), P.PATCH_DTYPE)
    k = 2
    for r in recs:
        assert tok[k] == b"PATCHS"
        f = np.array([float(x) for x in tok[k + 1:k + 12]], np.float64).astype(np.float32)
        r["coord"], r["normal"], r["ncc"], r["dscale"], r["ascale"] = f[0:4], f[4:8], f[8], f[9], f[10]
        k += 12
        for cnt, ids in (("num_images", "images"), ("num_vimages", "vimages")):
            n = int(tok[k])
            r[cnt] = n
            r[ids][:n] = [numbers.index(int(x)) for x in tok[k + 1:k + 1 + n]]
            k += 1 + n
    assert k == len(tok)
    return recs


def test_pmvs2_fuse_export(gpu_available, tmp_path):
    roots = [str(tmp_path / "plain"), str(tmp_path / "fuse")]
    for root in roots:
        make_dataset(root, 3, W, H, LEVEL, CSIZE, 8, numbers=NUMBERS)
    plain = run(roots[0], "PATCH")
    fused = run(roots[1], "PATCH", "FUSE")
    assert sorted(plain) == ["option-0000.patch", "option-0000.ply"]
    assert sorted(fused) == sorted(list(plain) + ["option-0000.fused.ply"])  # FUSE adds exactly this file
    for f in plain:  # without FUSE nothing changes, and FUSE changes nothing else
        assert fused[f] == plain[f], f
    v = parse_ply_binary(fused["option-0000.fused.ply"])
    assert len(v) >= 1
    assert np.isfinite(v["xyz"]).all() and np.isfinite(v["n"]).all()
    assert (v["support"] == 2).all()  # three targets, min_support 2: both others agree
    w, h = W >> LEVEL, H >> LEVEL
    assert len(v) <= 3 * w * h
    # the same cloud from the written model, through the library
    import pmvs_amd as P
    inp, _ = P.synth_scene(3, W, H, level=LEVEL, csize=CSIZE, supersample=2)  # make_dataset's scene
    recs = patch_records(P, plain["option-0000.patch"], NUMBERS)
    g = P.Scene(inp)
    try:
        c = g.fuse_patches(recs, writer_order=False, radius=CSIZE, min_support=2, depth_rel=0.01, normal_cos=0.5)
    finally:
        g.close()
    again = str(tmp_path / "again.ply")
    P.write_ply_binary(again, c["coord"], c["normal"], c["color"], c["support"])
    assert open(again, "rb").read() == fused["option-0000.fused.ply"]
