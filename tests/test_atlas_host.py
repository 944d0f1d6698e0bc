"""pmvs_atlas.h on the host (CPU test): the definition's texel map -- texel_of, face_corner, band_of_row -- compiled
into a stand-alone program (tests/csrc/atlas_host_test.cpp) with -fsanitize=address,undefined and run over every texel
of small layouts (n in {1, 2, 3, 7}, W in {c, 2c + 1}, odd and even counts that wrap to further rows), against the
numpy restatement of steps 3-6 that tests/test_gpu_mesh_atlas.py builds its atlas from.

The ownership property of step 5 is checked on the restatement alone: for a dense set of points of every triangle,
its corners and points of its hypotenuse among them, the bilinear neighbours with a non-zero weight are texels of that
triangle's own half of its own cell."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.dtype([("ok", "<i4"), ("rank", "<i4"), ("half", "<i4"), ("pad", "<i4"), ("l1", "<f8"), ("l2", "<f8")])
SIDES = (1, 2, 3, 7)


def restate_texels(W, n, count, I, Jrel):
    """Steps 5 and 6 for texels (I, Jrel) of the band of a class of `count` faces of side n (integer arrays):
    (ok, rank within the class, half, l1, l2); ok False = EMPTY."""
    I, Jrel = np.asarray(I, np.int64), np.asarray(Jrel, np.int64)
    c, k, slots = n + 5, W // (n + 5), (count + 1) >> 1
    col, i, crow, j = I // c, I % c, Jrel // c, Jrel % c
    slot = crow * k + col
    half = np.where(i + j <= n + 3, 0, 1)
    rank = 2 * slot + half
    ok = (col < k) & (slot < slots) & (rank < count)
    l1 = np.where(half == 0, (i - 1).astype(np.float64), (c - 2 - i).astype(np.float64)) / np.float64(n)
    l2 = np.where(half == 0, (j - 1).astype(np.float64), (c - 2 - j).astype(np.float64)) / np.float64(n)
    return ok, rank, half, l1, l2


def restate_corners(W, n, y0, r):
    """Steps 4 and 5: the three corners [len(r), 3, 2] (int64 atlas texels) of the faces of ranks r."""
    r = np.asarray(r, np.int64)
    c, k, slot, half = n + 5, W // (n + 5), r >> 1, r & 1
    ox, oy = (slot % k) * c, y0 + (slot // k) * c
    t0 = np.where(half == 0, 1, c - 2)
    t1 = np.where(half == 0, 1 + n, c - 2 - n)
    return np.stack([np.stack([ox + t0, oy + t0], 1), np.stack([ox + t1, oy + t0], 1), np.stack([ox + t0, oy + t1], 1)], 1)


def layouts():
    for n in SIDES:
        c = n + 5
        for W in (c, 2 * c + 1):
            k = W // c
            for count in (1, 2 * k, 2 * k + 1, 4 * k + 3 if k > 1 else 5):
                yield W, n, count


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("atlas_host") / "atlas_host_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cmvs-pmvs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "atlas_host_test.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def test_header_matches_restatement(program, tmp_path):
    seen = {"empty_half": 0, "margin": 0, "empty_slot": 0, "wrapped": 0}
    for W, n, count in layouts():
        c, k = n + 5, W // (n + 5)
        rows = -(-((count + 1) >> 1) // k) * c
        y0 = 1000 + n
        dst = tmp_path / "out.bin"
        subprocess.run([program, str(W), str(n), str(count), str(y0), str(dst)], check=True)
        raw = open(dst, "rb").read()
        recs = np.frombuffer(raw[:REC.itemsize * rows * W], REC).reshape(rows, W)
        corners = np.frombuffer(raw[REC.itemsize * rows * W:], np.int64).reshape(count, 3, 2)
        J, I = np.meshgrid(np.arange(rows), np.arange(W), indexing="ij")
        ok, rank, half, l1, l2 = restate_texels(W, n, count, I, J)
        assert np.array_equal(recs["ok"] != 0, ok), (W, n, count)
        for name, want in (("rank", rank), ("half", half), ("l1", l1), ("l2", l2)):
            assert recs[name][ok].tobytes() == want[ok].astype(recs[name].dtype).tobytes(), (W, n, count, name)
        assert np.array_equal(corners, restate_corners(W, n, y0, np.arange(count)))
        # every face owns texels, and its corners are texels of its own
        assert np.array_equal(np.unique(rank[ok]), np.arange(count))
        cr = restate_corners(W, n, 0, np.arange(count))
        for kk in range(3):
            o2, r2 = restate_texels(W, n, count, cr[:, kk, 0], cr[:, kk, 1])[:2]
            assert o2.all() and np.array_equal(r2, np.arange(count))
        seen["empty_half"] += int(count % 2 == 1)
        seen["margin"] += int((~ok[:, k * c:]).all() and W > k * c)
        seen["empty_slot"] += int((((count + 1) >> 1) % k) != 0)
        seen["wrapped"] += int(rows > c)
    assert all(v > 0 for v in seen.values()), seen


def triangle_points(d):
    """The points (a / d, b / d) of the unit right triangle, a + b <= d, as integer arrays (a, b): the corners, the
    hypotenuse (a + b == d) and the interior.  Positions are kept exact as integers over the denominator d."""
    a, b = np.meshgrid(np.arange(d + 1), np.arange(d + 1), indexing="ij")
    keep = a + b <= d
    return a[keep].astype(np.int64), b[keep].astype(np.int64)


def test_bilinear_fetch_stays_in_its_half():
    checked = 0
    for W, n, count in layouts():
        corners = restate_corners(W, n, 0, np.arange(count))
        for d in (1, n, 4 * n + 3, 7):   # the corners alone; the texel centres; two grids between the centres
            a, b = triangle_points(d)
            assert ((a + b) == d).sum() == d + 1 and ((a == 0) & (b == 0)).any()
            for r in range(count):
                T0, T1, T2 = (corners[r, kk] for kk in range(3))
                # the point T0 + (a / d) (T1 - T0) + (b / d) (T2 - T0), times d
                un = T0[0] * d + a * (T1[0] - T0[0]) + b * (T2[0] - T0[0])
                vn = T0[1] * d + a * (T1[1] - T0[1]) + b * (T2[1] - T0[1])
                x0, y0 = un // d, vn // d
                fx, fy = un - x0 * d, vn - y0 * d          # the fractions' numerators: 0 = on a texel centre
                for da, wa in ((0, d - fx), (1, fx)):
                    for db, wb in ((0, d - fy), (1, fy)):
                        live = (wa * wb) != 0               # a neighbour of weight zero is not fetched
                        x, y = (x0 + da)[live], (y0 + db)[live]
                        assert ((x >= 0) & (x < W) & (y >= 0)).all()
                        ok, rank = restate_texels(W, n, count, x, y)[:2]
                        assert ok.all() and (rank == r).all(), (W, n, count, r, d, da, db)
                        checked += int(live.sum())
    assert checked > 10000
