"""pmvs2's optional PIXDEPTH export: one PFM per target image with the depth of the written model
rendered per pixel at the option's level (pmvs_loop_pixel_maps at radius csize, writer order).  Checked
here: the files, their names, header and size, plausible contents, and that the other outputs do not
change.  The exact values are the business of tests/test_gpu_pixel_maps.py."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_pmvs2 import PMVS2, make_dataset

pytestmark = pytest.mark.gpu

NUMBERS = [0, 3, 7]  # image numbers that are not the view indexes
W, H, LEVEL, CSIZE = 640, 480, 2, 4


def run(root, *keywords):
    r = subprocess.run([PMVS2, root + "/", "option-0000", *keywords], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    models = os.path.join(root, "models")
    return {f: open(os.path.join(models, f), "rb").read() for f in sorted(os.listdir(models))}


def test_pmvs2_pixdepth_export(gpu_available, tmp_path):
    roots = [str(tmp_path / "plain"), str(tmp_path / "pixdepth")]
    for root in roots:
        make_dataset(root, 3, W, H, LEVEL, CSIZE, 8, numbers=NUMBERS)
    plain = run(roots[0], "PATCH")
    pix = run(roots[1], "PATCH", "PIXDEPTH")
    assert sorted(plain) == ["option-0000.patch", "option-0000.ply"]
    pfm = ["option-0000.pixdepth.%08d.pfm" % n for n in NUMBERS]
    assert sorted(pix) == sorted(list(plain) + pfm)
    for f in plain:  # without PIXDEPTH nothing changes, and PIXDEPTH changes nothing else
        assert pix[f] == plain[f], f
    patches = int(plain["option-0000.patch"].split(b"\n")[1])
    assert patches > 0
    w, h = W >> LEVEL, H >> LEVEL
    header = b"Pf\n%d %d\n-1.0\n" % (w, h)
    assert header == b"Pf\n160 120\n-1.0\n"
    for f in pfm:
        data = pix[f]
        assert data.startswith(header) and len(data) == len(header) + 4 * w * h, f
        v = np.frombuffer(data[len(header):], "<f4")
        assert np.isfinite(v).all() and (v >= 0).all() and not (v.view(np.uint32) == 0x80000000).any(), f
        assert 1 <= np.count_nonzero(v) <= (2 * CSIZE + 1) ** 2 * patches, f
