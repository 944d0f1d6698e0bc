"""CPU tests of the atlas's boundary (pmvs_mesh_atlas, pmvs_atlas_layout_from_counts, pmvs_write_ppm): the symbols are
exported, the Python mirror's struct layouts equal the C compiler's, every NULL and out-of-range argument of the
rejection list is refused without a device and leaves the outputs untouched, the PPM writer round-trips through
pmvs_ppm_load with the exact header, and the bands of step 4 equal a ten-line Python restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmvs_mesh_atlas", "pmvs_atlas_layout_from_counts", "pmvs_write_ppm")
EINVAL, EUNSUPPORTED = 1, 4


def restate_layout(counts, W, M):
    """Step 4 of the definition: (H, band_y [M + 1] with band_y[0] = H, placed, cells) from the faces per class."""
    y, band_y, placed, cells = 0, [0] * (M + 1), 0, 0
    for n in range(M, 0, -1):
        c, k, slots = n + 5, W // (n + 5), (int(counts[n]) + 1) >> 1
        band_y[n] = y
        y += -(-slots // k) * c
        placed, cells = placed + int(counts[n]), cells + slots
    band_y[0] = y
    return y, band_y, placed, cells


def test_atlas_symbols_exported(product_lib):
    import pmvs_amd as P
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cmvs-pmvs_amd", "libpmvs_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS:
        assert s in exported and s in P.EXPORTS, s


def test_atlas_layouts_match_c(tmp_path):
    import pmvs_amd as P
    exe = tmp_path / "atlas_layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "csrc", "atlas_layout.c"), "-o", str(exe)], check=True)
    c = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *rest = line.split()
        c[k if rest[0] != "sizeof" else k + ".sizeof"] = int(rest[-1])
    for name, T in (("pmvs_atlas_params", P.AtlasParams), ("pmvs_atlas_layout", P.AtlasLayout),
                    ("pmvs_atlas_buffers", P.AtlasBuffers)):
        assert C.sizeof(T) == c[name + ".sizeof"], name
        for f, _ in T._fields_:
            assert getattr(T, f).offset == c[f"{name}.{f}"], (name, f)
    assert c["PMVS_ATLAS_MAX_SIDE"] == P.ATLAS_MAX_SIDE == 251 and c["PMVS_ATLAS_MAX_WIDTH"] == P.ATLAS_MAX_WIDTH == 65536
    assert len(c) == 3 + 3 + 4 + 4 + 2  # every field of the three structs and the two limits were printed and compared


def test_atlas_arguments_rejected_without_a_device(product_lib):
    """No scene exists here, so every call must fail before it touches a device: with the NULL scene alone, and with
    each other NULL or out-of-range argument of the list beside it; the outputs keep their bytes.
    (tests/test_gpu_mesh_atlas.py repeats the list with a real scene, where the argument itself is what is rejected.)"""
    import pmvs_amd as P
    lib = product_lib
    vertex = np.zeros((3, 3), np.float32)
    face = np.array([[0, 1, 2]], np.int32)
    view = np.zeros(1, np.int32)
    rgb, tf = np.full(64 * 8 * 3, 7, np.uint8), np.full(64 * 8, -7, np.int32)
    uv, av = np.full(6, -7, np.float32), np.full(1, -7, np.int32)
    buf = P.AtlasBuffers(rgb.ctypes.data, tf.ctypes.data, uv.ctypes.data, av.ctypes.data)
    good = P.AtlasParams(64, 8, 1.0)
    layout = P.AtlasLayout(-7, -7, -7, -7)
    nan, inf = float("nan"), float("inf")

    def ref(x):
        return None if x is None else C.byref(x)

    def call(flags=0, prm=good, nv=3, v=vertex.ctypes.data, nf=1, f=face.ctypes.data, vw=view.ctypes.data, cap=8, b=buf, lay=layout):
        return lib.pmvs_mesh_atlas(None, flags, ref(prm), nv, v, nf, f, vw, cap, ref(b), ref(lay))

    assert call() == EINVAL and lib.pmvs_last_error()
    for kw in (dict(lay=None), dict(b=None), dict(flags=1), dict(flags=4), dict(flags=-1), dict(flags=2), dict(nv=-1), dict(nf=-1),
               dict(nv=1 << 31), dict(nf=1 << 31), dict(v=None), dict(f=None), dict(vw=None), dict(nv=2), dict(cap=-1), dict(cap=0),
               dict(nf=0, f=None, vw=None), dict(nv=0, v=None, nf=0, f=None, vw=None)):
        assert call(**kw) == EINVAL, kw
    bad_params = (None, P.AtlasParams(64, 0, 1.0), P.AtlasParams(64, -1, 1.0), P.AtlasParams(300, 252, 1.0), P.AtlasParams(12, 8, 1.0),
                  P.AtlasParams(65537, 8, 1.0), P.AtlasParams(-1, 8, 1.0), P.AtlasParams(64, 8, 0.0), P.AtlasParams(64, 8, -1.0),
                  P.AtlasParams(64, 8, nan), P.AtlasParams(64, 8, inf))
    counts = np.zeros(252, np.int64)
    lay2 = P.AtlasLayout(-7, -7, -7, -7)
    for prm in bad_params:
        assert call(prm=prm) == EINVAL
        assert lib.pmvs_atlas_layout_from_counts(ref(prm), counts.ctypes.data, C.byref(lay2), None) == EINVAL
    assert lib.pmvs_atlas_layout_from_counts(C.byref(good), None, C.byref(lay2), None) == EINVAL
    assert lib.pmvs_atlas_layout_from_counts(C.byref(good), counts.ctypes.data, None, None) == EINVAL
    neg = counts.copy()
    neg[3] = -1
    assert lib.pmvs_atlas_layout_from_counts(C.byref(good), neg.ctypes.data, C.byref(lay2), None) == EINVAL
    for a, v in ((rgb, 7), (tf, -7), (uv, -7), (av, -7)):
        assert (a == v).all()
    for lay in (layout, lay2):
        assert [lay.width, lay.height, lay.placed, lay.cells] == [-7] * 4
    # the limits themselves are accepted: the widest atlas, the largest side, the narrowest atlas of a side
    for prm in (P.AtlasParams(65536, 251, 1.0), P.AtlasParams(256, 251, 0.5), P.AtlasParams(13, 8, 1e-30)):
        assert lib.pmvs_atlas_layout_from_counts(C.byref(prm), counts.ctypes.data, C.byref(lay2), None) == 0
        assert [lay2.width, lay2.height, lay2.placed, lay2.cells] == [prm.width, 0, 0, 0]


def test_write_ppm_round_trip(product_lib, tmp_path):
    import pmvs_amd as P
    lib = product_lib
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (7, 3), (640, 2), (3, 1000)):
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        path = str(tmp_path / f"a{w}x{h}.ppm")
        P.write_ppm(path, img)
        raw = open(path, "rb").read()
        head = f"P6\n{w} {h}\n255\n".encode()
        assert raw[:len(head)] == head and raw[len(head):] == img.tobytes()
        back = P.ppm_load(path)
        assert back.dtype == np.uint8 and back.shape == (h, w, 3) and back.tobytes() == img.tobytes()
    one = np.zeros(3, np.uint8)
    ok = str(tmp_path / "one.ppm").encode()
    assert lib.pmvs_write_ppm(ok, 1, 1, one.ctypes.data) == 0
    # pmvs_write_pfm's rejections: a NULL argument, a non-positive size, a file that cannot be written
    assert lib.pmvs_write_ppm(None, 1, 1, one.ctypes.data) == EINVAL and lib.pmvs_write_ppm(ok, 1, 1, None) == EINVAL
    assert lib.pmvs_write_ppm(ok, 0, 1, one.ctypes.data) == EINVAL and lib.pmvs_write_ppm(ok, 1, 0, one.ctypes.data) == EINVAL
    assert lib.pmvs_write_ppm(ok, -1, 1, one.ctypes.data) == EINVAL and lib.pmvs_write_ppm(ok, 1, -1, one.ctypes.data) == EINVAL
    assert lib.pmvs_write_ppm(b"/nonexistent-dir/x.ppm", 1, 1, one.ctypes.data) == EINVAL
    with pytest.raises(ValueError):
        P.write_ppm(ok.decode(), np.zeros((2, 2), np.uint8))


def layout_cases():
    """(W, M, counts): empty classes between full ones, an odd count, a class that fills exactly one row, one that
    fills one row plus one cell, all zeros, and W = max_side + 5 (one cell per row)."""
    M = 8
    cases = []
    c = np.zeros(M + 1, np.int64)
    cases.append((64, M, c.copy()))                      # all zeros: H = 0
    c[8], c[5], c[2], c[1] = 3, 7, 1, 4                  # classes 7, 6, 4, 3 empty between full ones; odd counts
    c[0] = 99                                             # not read
    cases.append((64, M, c.copy()))
    k5 = 64 // 10
    c[5] = 2 * k5                                         # class 5 fills exactly one row
    cases.append((64, M, c.copy()))
    c[5] = 2 * k5 + 1                                     # one row plus one cell (of one face)
    cases.append((64, M, c.copy()))
    c[5] = 2 * k5 + 2                                     # one row plus one full cell
    cases.append((64, M, c.copy()))
    cases.append((M + 5, M, c.copy()))                   # one cell per row for the largest class
    rng = np.random.default_rng(3)
    big = rng.integers(0, 100000, 252).astype(np.int64)
    big[rng.integers(1, 252, 60)] = 0
    cases.append((8192, 251, big))
    cases.append((256, 251, big))
    return cases


def test_layout_from_counts_matches_restatement(product_lib):
    import pmvs_amd as P
    seen_zero = seen_one_cell = False
    for W, M, counts in layout_cases():
        H, band_y, placed, cells = restate_layout(counts, W, M)
        layout, got_y = P.atlas_layout_from_counts(counts, W, M)
        assert layout == {"width": W, "height": H, "placed": placed, "cells": cells}, (W, M)
        assert got_y.dtype == np.int64 and list(got_y) == band_y
        seen_zero |= H == 0
        seen_one_cell |= W // (M + 5) == 1 and counts[M] > 2
    assert seen_zero and seen_one_cell
    # the cases are what they are said to be, on the restatement alone
    W, M, c = layout_cases()[2]
    assert restate_layout(c, W, M)[1][4] - restate_layout(c, W, M)[1][5] == 10          # exactly one row of cells of 10
    W, M, c = layout_cases()[3]
    assert restate_layout(c, W, M)[1][4] - restate_layout(c, W, M)[1][5] == 20 and c[5] % 2 == 1
    # a height past 2^31-1 is unsupported, and the layout still says what it would be
    lib = product_lib
    prm, lay = P.AtlasParams(256, 251, 1.0), P.AtlasLayout()
    huge = np.zeros(252, np.int64)
    huge[251] = 1 << 25
    assert lib.pmvs_atlas_layout_from_counts(C.byref(prm), huge.ctypes.data, C.byref(lay), None) == EUNSUPPORTED
    assert lay.height == restate_layout(huge, 256, 251)[0] > (1 << 31) - 1
    huge[251] = (1 << 63) - 1
    assert lib.pmvs_atlas_layout_from_counts(C.byref(prm), huge.ctypes.data, C.byref(lay), None) == EUNSUPPORTED
    assert lay.height == (1 << 63) - 1                                                # saturated, not wrapped
