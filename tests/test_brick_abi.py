"""CPU tests of the brick volume's boundary (pmvs_loop_brick_tsdf, pmvs_brick_tsdf_patches, pmvs_brick_tsdf_mesh,
pmvs_loop_brick_mesh, pmvs_brick_mesh_patches, pmvs_brick_volume_from_points): the symbols are declared and
exported, the Python mirror's struct layouts equal the C compiler's, the volume call follows the documented
formulas within the brick limits, and every PMVS_EINVAL is reached without a device."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmvs_loop_brick_tsdf", "pmvs_brick_tsdf_patches", "pmvs_brick_tsdf_mesh", "pmvs_loop_brick_mesh",
           "pmvs_brick_mesh_patches", "pmvs_brick_volume_from_points")
EINVAL = 1


def test_brick_symbols_declared_and_exported(product_lib):
    import pmvs_amd as P
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cmvs-pmvs_amd", "libpmvs_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    header = open(os.path.join(ROOT, "include", "pmvs_amd.h")).read()
    for s in SYMBOLS:
        assert s in exported and s in P.EXPORTS and f"pmvs_status {s}(" in header, s
    for name in ("loop_brick_tsdf", "brick_tsdf_patches", "brick_tsdf_mesh", "loop_brick_mesh", "brick_mesh_patches"):
        assert callable(getattr(P.Scene, name))
    assert callable(P.brick_volume_from_points)


def test_brick_layouts_match_c(tmp_path):
    import pmvs_amd as P
    exe = tmp_path / "brick_layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "csrc", "brick_layout.c"), "-o", str(exe)], check=True)
    c = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *rest = line.split()
        c[k if rest[0] != "sizeof" else k + ".sizeof"] = int(rest[-1])
    for name, T in (("pmvs_brick_params", P.BrickParams), ("pmvs_brick_buffers", P.BrickBuffers)):
        assert C.sizeof(T) == c[name + ".sizeof"], name
        for f, _ in T._fields_:
            assert getattr(T, f).offset == c[f"{name}.{f}"], (name, f)
    assert len(c) == 3 + 5 + 3  # every field of the two structs and the three constants
    assert C.sizeof(P.BrickParams) == C.sizeof(P.TsdfParams) + 4
    assert (c["PMVS_BRICK"], c["PMVS_BRICK_MAX_MARGIN"], c["PMVS_BRICK_MAX_DIM"]) == (8, 64, 1 << 20)
    assert P.Scene.BRICK_ARRAYS["tsdf"][1] == ("b", 8, 8, 8) and list(P.Scene.BRICK_ARRAYS) == [f for f, _ in P.BrickBuffers._fields_]


def test_brick_volume_from_points(product_lib):
    """pmvs_volume_from_points' arithmetic, restated, at a resolution the dense call rejects."""
    import pmvs_amd as P
    rng = np.random.default_rng(11)
    pts = (rng.normal(size=(500, 3)) * [1.0, 0.37, 0.11] + [3, -2, 0.5]).astype(np.float32)
    lib, out = product_lib, P.Volume()
    assert lib.pmvs_volume_from_points(500, pts.ctypes.data, 8192, 3, C.byref(out)) == EINVAL   # past 2^31-1 voxels
    for cells in (256, 8192):
        v = P.brick_volume_from_points(pts, cells, 3)
        lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
        voxel = np.float32((hi - lo).max() / float(cells))
        assert np.float32(v.voxel) == voxel
        assert list(v.origin) == [float(np.float32(lo[a] - 3.0 * np.float64(voxel))) for a in range(3)]
        assert list(v.dims) == [int(max(1.0, np.ceil((hi[a] - lo[a]) / np.float64(voxel)))) + 6 for a in range(3)]
        assert cells + 6 <= v.dims[0] <= cells + 7
    dense = P.volume_from_points(pts, 256, 3)
    same = P.brick_volume_from_points(pts, 256, 3)
    assert bytes(dense) == bytes(same)                      # where both accept, the same volume
    assert v.dims[0] * v.dims[1] * v.dims[2] > 2 ** 31 - 1
    flat = np.zeros((4, 3), np.float32)
    for n, coord, cells, pad, o in ((0, pts, 256, 3, out), (500, None, 256, 3, out), (500, pts, 0, 3, out), (500, pts, 256, -1, out),
                                    (500, pts, 256, 3, None), (4, flat, 256, 3, out)):
        assert lib.pmvs_brick_volume_from_points(n, None if coord is None else coord.ctypes.data, cells, pad,
                                                 None if o is None else C.byref(o)) == EINVAL
    bad = pts.copy()
    bad[7, 1] = np.nan
    assert lib.pmvs_brick_volume_from_points(500, bad.ctypes.data, 256, 3, C.byref(out)) == EINVAL
    assert lib.pmvs_brick_volume_from_points(500, pts.ctypes.data, (1 << 20) - 5, 3, C.byref(out)) == EINVAL  # a dim past 2^20
    cube = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    assert lib.pmvs_brick_volume_from_points(500, cube.ctypes.data, 12000, 3, C.byref(out)) == EINVAL        # 1500^3 bricks > 2^31-1
    assert lib.pmvs_brick_volume_from_points(500, cube.ctypes.data, 8192, 3, C.byref(out)) == 0              # 1025^3 fit


def test_brick_arguments_rejected_without_a_device(product_lib):
    """No scene exists here, so every call must fail before it touches a device: with the NULL scene alone, and
    with each other NULL or out-of-range argument beside it; and with a handle that is no scene, which a call
    may only look at once everything else has passed."""
    import pmvs_amd as P
    lib = product_lib
    tp = P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), 0.1)
    prm = P.BrickParams(tp, 3)
    vol = P.volume((0, 0, 0), 0.1, (12, 9, 4))             # a 2 x 2 x 1 brick grid
    bb, mb, nb, nv, nf = P.BrickBuffers(), P.MeshBuffers(), C.c_int64(-7), C.c_int64(-7), C.c_int64(-7)
    keys = np.array([0, 1, 3], np.int64)
    tsdf, obs = np.ones(3 * 512, np.float32), np.ones(3 * 512, np.uint8)
    nan, inf = float("nan"), float("inf")
    bad_volumes = [None, P.volume((nan, 0, 0), 0.1, (4, 4, 4)), P.volume((0, inf, 0), 0.1, (4, 4, 4)),
                   P.volume((0, 0, 0), 0.0, (4, 4, 4)), P.volume((0, 0, 0), -1.0, (4, 4, 4)), P.volume((0, 0, 0), nan, (4, 4, 4)),
                   P.volume((0, 0, 0), inf, (4, 4, 4)), P.volume((0, 0, 0), 0.1, (0, 4, 4)), P.volume((0, 0, 0), 0.1, (4, 4, -1)),
                   P.volume((0, 0, 0), 0.1, ((1 << 20) + 1, 4, 4)),            # a dim past 2^20
                   P.volume((0, 0, 0), 0.1, (1 << 20, 1 << 17, 8)),            # 2^31 bricks
                   P.volume((0, 0, 0), 0.1, (1 << 20, 1 << 20, 1 << 20))]
    bad_params = [None] + [P.BrickParams(tp, m) for m in (-1, 65, 1 << 30)] + [
        P.BrickParams(P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), t), 3) for t in (0.0, -0.1, nan, inf)] + [
        P.BrickParams(P.TsdfParams(fp, 0.1), 3) for fp in (P.FuseParams(-1, 2, 0.01, 0.5), P.FuseParams(2, 256, 0.01, 0.5),
                                                           P.FuseParams(2, 2, nan, 0.5))]

    def ref(x):
        return None if x is None else C.byref(x)

    def calls(scene=None, p=prm, v=vol, b=bb, m=mb, flags=0, first=0, num=1, bcap=0, cb=nb, min_obs=1, vcap=0, fcap=0, cv=nv, cf=nf,
              k=keys, nbricks=3, which=(0, 1, 2, 3, 4)):
        """The status of the calls `which` (only those are made: the others' arguments may all be valid)."""
        tail = (min_obs, vcap, fcap, ref(m), ref(cv), ref(cf))
        fns = [lambda: lib.pmvs_loop_brick_tsdf(scene, flags, first, num, ref(p), ref(v), bcap, ref(b), ref(cb)),
               lambda: lib.pmvs_brick_tsdf_patches(scene, None, 0, flags, first, num, ref(p), ref(v), bcap, ref(b), ref(cb)),
               lambda: lib.pmvs_brick_tsdf_mesh(scene, flags & ~1, ref(v), min_obs, nbricks, None if k is None else k.ctypes.data,
                                                tsdf.ctypes.data, obs.ctypes.data, None, vcap, fcap, ref(m), ref(cv), ref(cf)),
               lambda: lib.pmvs_loop_brick_mesh(scene, flags, first, num, ref(p), ref(v), *tail),
               lambda: lib.pmvs_brick_mesh_patches(scene, None, 0, flags, first, num, ref(p), ref(v), *tail)]
        return [fns[i]() for i in which]

    assert calls() == [EINVAL] * 5 and lib.pmvs_last_error()
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)   # zeroed, not a scene: reading it would not be noticed, so ...
    for scene in (None, fake):                             # ... the same lists must fail with either
        for v in bad_volumes:
            assert calls(scene, v=v) == [EINVAL] * 5
        for kw in (dict(m=None), dict(cv=None), dict(cf=None), dict(min_obs=0), dict(min_obs=256), dict(vcap=-1), dict(fcap=-1),
                   dict(flags=4), dict(flags=-1)):
            assert calls(scene, which=(2, 3, 4), **kw) == [EINVAL] * 3, kw
        for kw in (dict(b=None), dict(cb=None), dict(bcap=-1), dict(flags=4), dict(flags=-1)):
            assert calls(scene, which=(0, 1), **kw) == [EINVAL] * 2, kw
        for p in bad_params:
            assert calls(scene, p=p, which=(0, 1, 3, 4)) == [EINVAL] * 4
        # the caller's bricks: a negative count, a NULL key list, keys that are unsorted, repeated or outside the grid
        for kw in (dict(nbricks=-1), dict(k=None), dict(k=np.array([1, 0, 3], np.int64)), dict(k=np.array([0, 1, 1], np.int64)),
                   dict(k=np.array([0, 1, 4], np.int64)), dict(k=np.array([-1, 1, 3], np.int64)),
                   dict(k=np.array([0, 1, 2, 3, 4], np.int64), nbricks=5)):
            assert calls(scene, which=(2,), **kw) == [EINVAL], kw
    assert (nb.value, nv.value, nf.value) == (-7, -7, -7)
    # the target range is the scene's to judge: a NULL scene fails there too
    for first, num in ((-1, 1), (0, 0)):
        assert calls(first=first, num=num, which=(0, 1, 3, 4)) == [EINVAL] * 4
