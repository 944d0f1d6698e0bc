"""Uninitialised-memory hunt over the brick volume's calls, by tests/test_gpu_poison.py's scheme: with
PMVS_POISON_ALLOC=<byte> every new device allocation is filled with that byte, so a kernel that reads memory no
kernel wrote changes the result.  brick_tsdf_patches and brick_mesh_patches (host mode, so their staging arrays
are poisoned too) on a small synthetic loop's records must give byte-identical output with two different poison
bytes and without poisoning.  The variable is read once per process, so each run is a child process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import pmvs_amd as P
inp, p = P.synth_scene(6, 320, 240, level=1, supersample=2, hard=True)
g = P.Scene(inp)
cands = P.synth_candidates(p, inp.projections, 300, seed=9)
r, _ = g.refine_batch(cands)
out, log = g.run_loop(P.patches_from_refined(r), inp.threshold, wave=256, min_candidates=512)
def digest(arrays):
    h = hashlib.sha1()
    for k in arrays:
        h.update(arrays[k].tobytes())
    return h.hexdigest()
cloud = g.fuse_patches(out)
vol = P.brick_volume_from_points(cloud["coord"], cells=40)
trunc = 3.0 * vol.voxel
bricks = g.brick_tsdf_patches(out, vol, trunc, 5)
mesh = g.brick_mesh_patches(out, vol, trunc, 5)
print(len(out), len(bricks["brick"]), len(mesh["vertex"]), len(mesh["face"]), digest(bricks), digest(mesh),
      digest(g.brick_mesh_patches(out, vol, trunc, 0, min_obs=2)))
g.close()
"""


def _run(poison):
    env = dict(os.environ)
    env.pop("PMVS_POISON_ALLOC", None)
    if poison is not None:
        env["PMVS_POISON_ALLOC"] = str(poison)
    res = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "cmvs-pmvs_amd")], env=env,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout.split()


@pytest.mark.timeout(400)
def test_poisoned_allocations_do_not_change_brick_results(gpu_available):
    base = _run(None)
    assert int(base[0]) > 100 and int(base[1]) > 0 and int(base[2]) > 0 and int(base[3]) > 0   # a model, bricks, a mesh
    for byte in (0xAB, 0x00):
        assert _run(byte) == base, f"poison byte {byte:#x} changed the result"
