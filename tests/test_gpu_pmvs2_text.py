"""pmvs2 writes its .ply / .patch / .pset from the text formatted on the device (pmvs_loop_text); with
PMVS_HOST_WRITERS=1 it keeps the export arrays and the host writers.  On the C1 dataset of
test_gpu_pmvs2.py both runs must leave byte-identical files."""
import os
import subprocess

import pytest

from test_gpu_pmvs2 import PMVS2, make_dataset

pytestmark = pytest.mark.gpu


def test_pmvs2_device_text_equals_host_writers(gpu_available, tmp_path):
    root = str(tmp_path / "pmvs")
    make_dataset(root, 3, 640, 480, 2, 4, 8, masks=True, numbers=[0, 3, 7])
    files = {}
    for mode, env in (("device", {}), ("host", {"PMVS_HOST_WRITERS": "1"})):
        r = subprocess.run([PMVS2, root + "/", "option-0000", "PATCH", "PSET"], capture_output=True, text=True,
                           timeout=300, env=dict(os.environ, **env))
        assert r.returncode == 0, (mode, r.stderr[-2000:])
        assert "write " in r.stderr  # the timing line keeps its fields
        files[mode] = {}
        for ext in (".ply", ".patch", ".pset"):
            path = os.path.join(root, "models", "option-0000" + ext)
            with open(path, "rb") as f:
                files[mode][ext] = f.read()
            os.remove(path)
    for ext in (".ply", ".patch", ".pset"):
        assert len(files["host"][ext]) > 1000, ext
        assert files["device"][ext] == files["host"][ext], ext
