"""pmvs_texmesh.h on the host (CPU test): the definition's functions -- face_drawn, face_box, face_pixel_depth, the
texture coordinates -- compiled into a stand-alone program (tests/csrc/texmesh_host_test.cpp) with
-fsanitize=address,undefined and run on already projected corners, against tests/test_gpu_mesh_raster.py's numpy
restatement of the same definition: the winning key of every pixel, which faces are drawn and boxed, the boxes'
pixel counts and the texture coordinates, byte for byte.  The corners include what project() can return: the
clamped +-2^31, the -65535 of a point behind the camera with its depth -1, NaN and infinite depths, zero areas,
faces far larger than the image and faces between the pixel centres."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_mesh_raster import TargetRaster
from test_texmesh_abi import texcoords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 23


class Projected:
    """An oracle that returns the corners as they are: vertex = (x, y, z), already projected."""
    level = 0

    @staticmethod
    def project(t, level, c4):
        return np.ascontiguousarray(c4[:, :3], np.float32)

    @staticmethod
    def depth(t, c4):
        return np.ascontiguousarray(c4[:, 2], np.float32)


def corners_and_faces():
    rng = np.random.default_rng(77)
    n = 600
    v = np.empty((n, 3), np.float32)
    v[:, 0] = rng.uniform(-10, W + 10, n)
    v[:, 1] = rng.uniform(-10, H + 10, n)
    v[:, 2] = rng.uniform(0.5, 9.0, n)
    v[:40, :2] = np.round(v[:40, :2])                                   # corners on pixel centres: edges through centres
    special = np.array([[2147483648.0, 5, 3], [-2147483648.0, 5, 3], [4, 2147483648.0, 3], [-65535, -65535, -1],
                        [5, 5, np.nan], [6, 7, np.inf], [3, 3, 0.0], [8, 2, -2.0], [-500, -400, 2], [900, -300, 2.5],
                        [10, 1200, 3.5], [12.3, 9.6, 1e-30], [12.9, 9.7, 1e30]], np.float32)
    v = np.concatenate([v, special])
    f = rng.integers(0, n, (1500, 3)).astype(np.int32)
    f[:60] = rng.integers(0, 40, (60, 3))                                # among the integer corners
    near = rng.integers(40, n, 300)
    small = np.stack([near, near, near], axis=1).astype(np.int32)       # sub-pixel faces around a corner
    extra = np.concatenate([v[near] + rng.uniform(-0.6, 0.6, (300, 3)).astype(np.float32) * [1, 1, 0],
                            v[near] + rng.uniform(-0.6, 0.6, (300, 3)).astype(np.float32) * [1, 1, 0]]).astype(np.float32)
    small[:, 1] = len(v) + np.arange(300)
    small[:, 2] = len(v) + 300 + np.arange(300)
    v = np.concatenate([v, extra]).astype(np.float32)
    s = n + np.arange(len(special))
    hand = np.array([[s[8], s[9], s[10]], [s[0], s[1], s[2]], [0, 1, s[3]], [0, 1, s[4]], [2, 3, s[5]], [4, 5, s[6]], [6, 7, s[7]],
                     [7, 7, 8], [9, 10, 9], [s[11], s[12], 11], [s[8], s[10], s[9]], [0, 1, 2], [0, 1, 2]], np.int32)
    return v, np.concatenate([f, small, hand]).astype(np.int32)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("texmesh_host") / "texmesh_host_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cmvs-pmvs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "texmesh_host_test.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_header_matches_restatement(program, tmp_path):
    v, f = corners_and_faces()
    r = TargetRaster(Projected, Projected, W, H, 0, v, f)
    # the branches, on the restatement alone
    assert (~r.drawn).sum() > 5 and (r.drawn & ~r.boxed).sum() > 50 and (r.boxed & (r.covered == 0)).sum() > 10
    assert r.box_pixels.max() == W * H and (r.A[r.drawn] > 0).any() and (r.A[r.drawn] < 0).any()
    assert (r.keys != np.uint64(0xFFFFFFFFFFFFFFFF)).sum() > W * H // 2
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as fh:
        fh.write(np.array([W, H, len(v), len(f)], np.int32).tobytes() + v.tobytes() + f.tobytes())
    subprocess.run([program, str(src), str(dst)], check=True)
    raw = open(dst, "rb").read()
    nf, nv = len(f), len(v)
    keys = np.frombuffer(raw[:8 * W * H], np.uint64)
    flags = np.frombuffer(raw[8 * W * H:8 * W * H + 8 * nf], np.int32).reshape(nf, 2)
    boxes = np.frombuffer(raw[8 * W * H + 8 * nf:8 * W * H + 16 * nf], np.int64)
    tex = np.frombuffer(raw[8 * W * H + 16 * nf:], np.float32).reshape(nv, 2)
    assert keys.tobytes() == r.keys.tobytes()
    assert np.array_equal(flags[:, 0] != 0, r.drawn) and np.array_equal(flags[:, 1] != 0, r.boxed)
    assert np.array_equal(boxes, r.box_pixels)
    # the texture coordinates: the writer's formula on every corner, taken as three corners of one face each
    uv = np.concatenate([v[:, :2]] * 3, axis=1)
    want = texcoords(np.zeros(nv, np.int32), uv, np.array([[W, H]], np.int32))[:, :2]
    ok = np.isfinite(v[:, :2]).all(axis=1)
    assert ok.all() and tex.tobytes() == want.tobytes()
