"""pmvs_loop_fuse / pmvs_fuse_patches: the per-pixel maps fused into a cross-view-checked point cloud.
There is no reference for this: the expected arrays are a numpy restatement of the definition in
include/pmvs_amd.h, built from test_gpu_pixel_maps.py's restatement of the maps and from
OracleScene.project, .depth, .camera and .get_level alone: explicit element-wise float64 products and sums in
the definition's order (no `@`, no np.dot), the two float parameters rounded to float32 before they are
widened.  Every array is compared for exact equality of dtype, shape and bytes; nothing is excluded.

The scene is test_gpu_depth_maps.py's crafted one (4 targets at 160 x 120, one cropped to 150 x 100) and the
model a surface defined here: a sphere the targets see consistently, an occluded inner sphere, floaters, and
surface points whose normals are tilted away -- so that every branch of the definition occurs, which the
fixture asserts on the restatement alone."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_depth_maps import crafted_scene, order_keys
from test_gpu_pixel_maps import image_dims, restate

pytestmark = pytest.mark.gpu

NAMES = ("support_map", "coord", "normal", "color", "support", "pixel", "patch")
EINVAL = "pmvs status 1:"
RADIUS = 2
PARAMS = ((0.01, 0.5, 2), (0.002, 0.9, 1), (0.01, 0.5, 3))  # depth_rel, normal_cos, min_support
PIXELS = 72600


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def surface_records(P):
    """1650 records, shuffled: 1200 on the sphere of radius 0.45 about the origin with outward unit normals;
    200 on an inner sphere of radius 0.30 (occluded); 150 floaters uniform in +-0.8 with random unit
    normals; 100 on the outer sphere with normals tilted 70 degrees off the radial direction.  Images and
    grids as test_gpu_depth_maps.py's records have them, so the writer order is a real permutation."""
    rng = np.random.default_rng(20262)
    n = 1650
    r = np.zeros(n, P.PATCH_DTYPE)
    d_out, d_in, d_tilt = unit(rng.normal(size=(1200, 3))), unit(rng.normal(size=(200, 3))), unit(rng.normal(size=(100, 3)))
    side = unit(np.cross(d_tilt, unit(rng.normal(size=(100, 3)))))
    tilt = np.deg2rad(70.0)
    coord = np.concatenate([0.45 * d_out, 0.30 * d_in, rng.uniform(-0.8, 0.8, (150, 3)), 0.45 * d_tilt])
    normal = np.concatenate([d_out, d_in, unit(rng.normal(size=(150, 3))), np.cos(tilt) * d_tilt + np.sin(tilt) * side])
    r["coord"][:, :3] = coord.astype(np.float32)
    r["coord"][:, 3] = 1.0
    r["normal"][:, :3] = normal.astype(np.float32)
    for f in ("ncc", "dscale", "ascale"):
        r[f] = rng.uniform(0, 1, n).astype(np.float32)
    for i in range(n):
        k = int(rng.integers(1, 6))
        r["num_images"][i] = k
        r["images"][i, :k] = rng.integers(0, 6, k)
        r["grids"][i, :k, 0] = rng.integers(0, 75, k)
        r["grids"][i, :k, 1] = rng.integers(0, 50, k)
    return r[rng.permutation(n)]


def cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


class Fusion:
    """The definition over the targets `targets` (as if the scene had no others), from their maps: what
    does not depend on the parameters is computed once (points, validity, the pixel q(p, s) of every pair),
    fuse() applies a parameter set."""

    def __init__(self, o, inp, maps, targets):
        self.maps, self.targets = maps, list(targets)
        dims = [image_dims(inp)[t] for t in targets]
        self.off = np.concatenate([[0], np.cumsum([w * h for w, h in dims])]).astype(np.int64)
        total = int(self.off[-1])
        patch, depth = maps["patch"], maps["depth"]
        assert patch.shape == (total,)
        self.filled = patch >= 0
        self.Sf = np.zeros((total, 3), np.float32)
        self.valid = np.zeros(total, bool)
        self.color = np.zeros((total, 3), np.uint8)
        nt = len(targets)
        # per ordered pair (j, k): q = the pixel of k a valid pixel of j falls on (-1: outside), zs its depth there
        self.q = {(j, k): np.full(total, -1, np.int64) for j in range(nt) for k in range(nt) if j != k}
        self.zs = {jk: np.zeros(total, np.float32) for jk in self.q}
        for j, t in enumerate(targets):
            W, H = dims[j]
            sl = slice(int(self.off[j]), int(self.off[j + 1]))
            self.color[sl] = o.get_level(t, inp.level).reshape(-1, 3)
            idx = np.nonzero(self.filled[sl])[0]
            u, v = (idx % W).astype(np.float64), (idx // W).astype(np.float64)
            cam = o.camera(t, inp.level).astype(np.float64)
            oaxis, Pm = cam[4:8], cam[18:30]
            a = [Pm[k] - u * Pm[8 + k] for k in range(4)]
            b = [Pm[4 + k] - v * Pm[8 + k] for k in range(4)]
            c = [oaxis[0], oaxis[1], oaxis[2]]
            bc, ca, ab = cross(b, c), cross(c, a), cross(a, b)
            det = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2]
            r0, r1, r2 = -a[3], -b[3], depth[sl][idx].astype(np.float64) - oaxis[3]
            with np.errstate(all="ignore"):
                S = np.stack([((r0 * bc[k] + r1 * ca[k] + r2 * ab[k]) / det).astype(np.float32) for k in range(3)], -1)
            ok = np.isfinite(S).all(axis=1)
            g = int(self.off[j]) + idx
            self.Sf[g], self.valid[g] = S, ok
            gv = g[ok]
            c4 = np.concatenate([S[ok], np.ones((len(gv), 1), np.float32)], axis=1)
            for k, s in enumerate(targets):
                if k == j:
                    continue
                Ws, Hs = dims[k]
                xy = o.project(s, inp.level, c4)
                px = np.floor(xy[:, 0].astype(np.float64) + 0.5)
                py = np.floor(xy[:, 1].astype(np.float64) + 0.5)
                with np.errstate(invalid="ignore"):
                    inside = (px >= 0) & (px <= Ws - 1) & (py >= 0) & (py <= Hs - 1)  # in double: a NaN fails
                qq = np.full(len(gv), -1, np.int64)
                qq[inside] = int(self.off[k]) + py[inside].astype(np.int64) * Ws + px[inside].astype(np.int64)
                self.q[j, k][gv] = qq
                self.zs[j, k][gv] = o.depth(s, c4)

    def pair(self, j, k, depth_rel, normal_cos):
        """Per pixel of the range, for target j against k: (the pixels of j, has a pixel q, q is filled,
        the depth test, the normal test)."""
        sl = slice(int(self.off[j]), int(self.off[j + 1]))
        q = self.q[j, k][sl]
        inside = q >= 0
        qc = np.where(inside, q, 0)
        filled = inside & self.filled[qc]
        ds, zs = self.maps["depth"][qc].astype(np.float64), self.zs[j, k][sl].astype(np.float64)
        with np.errstate(invalid="ignore"):
            dok = (self.zs[j, k][sl] > 0) & (np.abs(ds - zs) <= np.float64(np.float32(depth_rel)) * zs)
        n, m = self.maps["normal"][sl].astype(np.float64), self.maps["normal"][qc].astype(np.float64)
        with np.errstate(invalid="ignore"):
            nok = n[:, 0] * m[:, 0] + n[:, 1] * m[:, 1] + n[:, 2] * m[:, 2] >= np.float64(np.float32(normal_cos))
        return sl, q, inside, filled, dok, nok

    def fuse(self, depth_rel, normal_cos, min_support):
        nt, total = len(self.targets), int(self.off[-1])
        cons = {}
        support = np.zeros(total, np.int64)
        stats = {"outside": 0, "empty": 0, "depth_only": 0, "normal_only": 0, "other_row": 0, "same_row": 0}
        for (j, k) in self.q:
            sl, q, inside, filled, dok, nok = self.pair(j, k, depth_rel, normal_cos)
            valid = self.valid[sl]
            cons[j, k] = valid & filled & dok & nok
            support[sl] += cons[j, k]
            stats["outside"] += int((valid & ~inside).sum())
            stats["empty"] += int((valid & inside & ~filled).sum())
            stats["depth_only"] += int((valid & filled & ~dok & nok).sum())
            stats["normal_only"] += int((valid & filled & dok & ~nok).sum())
            same = self.maps["patch"][sl] == self.maps["patch"][np.where(inside, q, 0)]
            stats["other_row"] += int((cons[j, k] & ~same).sum())
            stats["same_row"] += int((cons[j, k] & same).sum())
        assert support.max(initial=0) <= nt - 1
        passing = self.filled & self.valid & (support >= min_support)
        emit = passing.copy()
        for (j, k) in self.q:
            if k < j:
                sl = slice(int(self.off[j]), int(self.off[j + 1]))
                emit[sl] &= ~(cons[j, k] & passing[np.where(self.q[j, k][sl] >= 0, self.q[j, k][sl], 0)])
        pix = np.nonzero(emit)[0].astype(np.int64)
        out = {"support_map": support.astype(np.uint8), "coord": self.Sf[pix], "normal": self.maps["normal"][pix],
               "color": self.color[pix], "support": support[pix].astype(np.uint8), "pixel": pix,
               "patch": self.maps["patch"][pix]}
        return out, {"stats": stats, "cons": cons, "passing": passing, "emit": emit}


def assert_same(got, want, names=NAMES):
    assert set(got) == set(names)
    for k in names:
        a = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        assert a.dtype == want[k].dtype and a.shape == want[k].shape, k
        assert a.tobytes() == want[k].tobytes(), k


def kw(prm):
    return dict(radius=RADIUS, depth_rel=prm[0], normal_cos=prm[1], min_support=prm[2])


@pytest.fixture(scope="module")
def surface(gpu_available, oracle_mod):
    import pmvs_amd as P
    inp = crafted_scene(P)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    recs = surface_records(P)
    order = np.argsort(order_keys(recs, inp), kind="stable")
    assert not np.array_equal(order, np.arange(len(recs)))
    assert image_dims(inp) == [(160, 120), (150, 100), (160, 120), (160, 120)]
    fus, want, aux = {}, {}, {}
    for wo, rows in ((False, np.arange(len(recs))), (True, order)):
        fus[wo] = Fusion(o, inp, restate(o, inp, recs, rows, RADIUS)[0], range(4))
        for prm in PARAMS:
            want[prm, wo], aux[prm, wo] = fus[wo].fuse(*prm)
    # coverage, on the restatement alone
    for wo in (False, True):
        f, (w, a) = fus[wo], (want[PARAMS[0], wo], aux[PARAMS[0], wo])
        assert set(np.unique(w["support_map"][f.filled & f.valid])) == {0, 1, 2, 3}   # every support value
        assert all(a["stats"][k] > 0 for k in a["stats"]), a["stats"]                  # every failure reason, both supporters
        assert (w["pixel"] >= 19200).any()                                             # an emitter in a target > 0
        assert (a["passing"] & ~a["emit"]).any()                                       # a suppressed passing pixel
        assert 0 < len(w["pixel"]) < int(a["passing"].sum())
    yield P, g, o, inp, recs, order, fus, want, aux
    g.close()
    o.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("writer_order", [False, True])
@pytest.mark.parametrize("prm", PARAMS)
def test_fuse_crafted(surface, prm, writer_order, device):
    P, g, o, inp, recs, order, fus, want, aux = surface
    got = g.fuse_patches(recs, writer_order=writer_order, device=device, **kw(prm))
    if device:
        assert all(t.is_cuda and t.device.index == g.device for t in got.values())
    assert_same(got, want[prm, writer_order])


def test_fuse_range_is_not_a_slice(surface):
    """Targets [1, 3) are fused as if the scene had no others: equal to the restatement over those two
    alone, and not the slice of the full call."""
    P, g, o, inp, recs, order, fus, want, aux = surface
    prm = (0.01, 0.5, 1)
    part = Fusion(o, inp, restate(o, inp, recs, order, RADIUS, targets=(1, 2))[0], (1, 2)).fuse(*prm)[0]
    got = g.fuse_patches(recs, writer_order=True, first_target=1, num_targets=2, **kw(prm))
    assert_same(got, part)
    assert len(got["pixel"]) > 0 and got["support_map"].max() == 1
    full = g.fuse_patches(recs, writer_order=True, **kw(prm))
    assert not np.array_equal(full["support_map"][19200:53400], got["support_map"])
    inside = (full["pixel"] >= 19200) & (full["pixel"] < 53400)
    assert not np.array_equal(full["pixel"][inside] - 19200, got["pixel"])


def raw_call(P, g, recs, prm, cap, arrays, flags=0, first=0, num=4):
    """pmvs_fuse_patches through ctypes with caller-made host arrays; returns (status, count)."""
    buf = P.FuseBuffers()
    for k, a in arrays.items():
        setattr(buf, k, a.ctypes.data)
    pa = np.ascontiguousarray(recs, P.PATCH_DTYPE)
    fp = P.FuseParams(RADIUS, prm[2], prm[0], prm[1])
    cnt = C.c_int64(-1)
    st = g.lib.pmvs_fuse_patches(g.handle, pa.ctypes.data, len(pa), flags, first, num, C.byref(fp), cap, C.byref(buf), C.byref(cnt))
    return st, int(cnt.value)


def test_fuse_cap_and_counting_call(surface):
    P, g, o, inp, recs, order, fus, want, aux = surface
    prm = PARAMS[0]
    w = want[prm, False]
    n = len(w["pixel"])
    assert raw_call(P, g, recs, prm, 0, {}) == (0, n)            # the counting call: every pointer NULL
    cap, guard = n // 3, 64
    assert 0 < cap < n
    shapes = {"coord": ((cap + guard, 3), np.float32), "normal": ((cap + guard, 3), np.float32),
              "color": ((cap + guard, 3), np.uint8), "support": ((cap + guard,), np.uint8),
              "pixel": ((cap + guard,), np.int64), "patch": ((cap + guard,), np.int32)}
    arrays = {k: np.full(s, 0x5A, dt) for k, (s, dt) in shapes.items()}
    arrays["support_map"] = np.full(PIXELS + guard, 0x5A, np.uint8)
    assert raw_call(P, g, recs, prm, cap, arrays) == (0, n)      # count is the total, not what was written
    for k in shapes:
        assert arrays[k][:cap].tobytes() == w[k][:cap].tobytes(), k
        assert (arrays[k][cap:] == np.array(0x5A, arrays[k].dtype)).all(), k
    assert arrays["support_map"][:PIXELS].tobytes() == w["support_map"].tobytes()
    assert (arrays["support_map"][PIXELS:] == 0x5A).all()
    # a cap beyond the count writes count points
    big = {"pixel": np.full(n + guard, -3, np.int64)}
    assert raw_call(P, g, recs, prm, n + guard, big) == (0, n)
    assert np.array_equal(big["pixel"][:n], w["pixel"]) and (big["pixel"][n:] == -3).all()
    # and so does any cap, however large: no more points than pixels exist, and the staging is sized by that
    huge = {"pixel": np.full(n + guard, -3, np.int64), "coord": np.full((n + guard, 3), 0x5A, np.float32)}
    assert raw_call(P, g, recs, prm, 2 ** 62, huge) == (0, n)
    assert np.array_equal(huge["pixel"][:n], w["pixel"]) and (huge["pixel"][n:] == -3).all()
    assert huge["coord"][:n].tobytes() == w["coord"].tobytes() and (huge["coord"][n:] == np.float32(0x5A)).all()
    # device mode by hand: the same prefix and guard
    dpix = torch.full((cap + guard,), -3, dtype=torch.int64, device=torch.device("cuda", g.device))
    buf = P.FuseBuffers()
    buf.pixel = dpix.data_ptr()
    pa = np.ascontiguousarray(recs, P.PATCH_DTYPE)
    fp, cnt = P.FuseParams(RADIUS, prm[2], prm[0], prm[1]), C.c_int64(-1)
    assert g.lib.pmvs_fuse_patches(g.handle, pa.ctypes.data, len(pa), P.EXPORT_DEVICE, 0, 4, C.byref(fp), cap, C.byref(buf),
                                   C.byref(cnt)) == 0
    assert cnt.value == n
    dpix = dpix.cpu().numpy()
    assert np.array_equal(dpix[:cap], w["pixel"][:cap]) and (dpix[cap:] == -3).all()


def test_fuse_min_support_zero(surface):
    """Every filled valid pixel passes; a pixel no other target confirms is emitted with support 0."""
    P, g, o, inp, recs, order, fus, want, aux = surface
    w, a = fus[True].fuse(0.01, 0.5, 0)
    assert np.array_equal(a["passing"], fus[True].filled & fus[True].valid) and (w["support"] == 0).any()
    assert (a["passing"] & ~a["emit"]).any()
    assert_same(g.fuse_patches(recs, writer_order=True, **kw((0.01, 0.5, 0))), w)
    assert_same(g.fuse_patches(recs, writer_order=True, arrays=("support", "pixel"), **kw((0.01, 0.5, 0))), w,
                ("support", "pixel"))


def test_fuse_no_records(surface):
    P, g, o, inp, recs, order, fus, want, aux = surface
    for writer_order in (False, True):
        for min_support in (0, 2):
            got = g.fuse_patches(recs[:0], writer_order=writer_order, **kw((0.01, 0.5, min_support)))
            assert got["support_map"].shape == (PIXELS,) and not got["support_map"].any()
            assert got["coord"].shape == (0, 3) and got["pixel"].shape == (0,)
    assert raw_call(P, g, recs[:0], PARAMS[0], 0, {}) == (0, 0)


def test_fuse_suppressed_pixels_have_a_passing_lower_pixel(surface):
    """The device's own output: every passing pixel it did not emit is consistent with a passing pixel of a
    lower target (so following that chain ends at an emitted point)."""
    P, g, o, inp, recs, order, fus, want, aux = surface
    for prm in PARAMS:
        f = fus[False]
        got = g.fuse_patches(recs, writer_order=False, **kw(prm))
        passing = f.filled & f.valid & (got["support_map"] >= prm[2])
        emitted = np.zeros(PIXELS, bool)
        emitted[got["pixel"]] = True
        assert not (emitted & ~passing).any()
        supp = passing & ~emitted
        assert supp.any() and not supp[:19200].any()              # nothing suppresses target 0
        backed = np.zeros(PIXELS, bool)
        for (j, k), c in aux[prm, False]["cons"].items():
            if k < j:
                sl = slice(int(f.off[j]), int(f.off[j + 1]))
                q = f.q[j, k][sl]
                backed[sl] |= c & passing[np.where(q >= 0, q, 0)]
        assert not (supp & ~backed).any()
        assert not (emitted & backed).any()


def test_fuse_errors(surface):
    P, g, o, inp, recs, order, fus, want, aux = surface
    with pytest.raises(P.PmvsError, match=EINVAL):   # no run_loop on this scene
        g.loop_fuse()
    lib, pa = g.lib, np.ascontiguousarray(recs[:4], P.PATCH_DTYPE)
    good, buf, cnt = P.FuseParams(RADIUS, 2, 0.01, 0.5), P.FuseBuffers(), C.c_int64(0)

    def call(flags=0, first=0, num=4, prm=good, cap=0, b=buf, c=cnt, scene=g.handle, patches=pa.ctypes.data, n=4):
        return lib.pmvs_fuse_patches(scene, patches, n, flags, first, num, C.byref(prm) if prm is not None else None, cap,
                                     C.byref(b) if b is not None else None, C.byref(c) if c is not None else None)

    def loop(flags=0, first=0, num=4, prm=good, cap=0, b=buf, c=cnt, scene=g.handle):
        return lib.pmvs_loop_fuse(scene, flags, first, num, C.byref(prm) if prm is not None else None, cap,
                                  C.byref(b) if b is not None else None, C.byref(c) if c is not None else None)

    assert call() == 0
    for f in (call, loop):
        assert f(scene=None) == 1 and f(prm=None) == 1 and f(b=None) == 1 and f(c=None) == 1
        for flags in (4, 8, 1 | 16, -1):                 # any bit beyond WRITER_ORDER | DEVICE
            assert f(flags=flags) == 1
        for first, num in ((-1, 1), (0, 0), (3, 2), (4, 1)):
            assert f(first=first, num=num) == 1
        assert f(cap=-1) == 1
        for bad in (P.FuseParams(-1, 2, 0.01, 0.5), P.FuseParams(P.PIXEL_MAX_RADIUS + 1, 2, 0.01, 0.5),
                    P.FuseParams(RADIUS, -1, 0.01, 0.5), P.FuseParams(RADIUS, 256, 0.01, 0.5),
                    P.FuseParams(RADIUS, 2, -0.01, 0.5), P.FuseParams(RADIUS, 2, float("inf"), 0.5),
                    P.FuseParams(RADIUS, 2, float("nan"), 0.5), P.FuseParams(RADIUS, 2, 0.01, float("nan"))):
            assert f(prm=bad) == 1
    assert loop() == 1                                   # valid arguments, but no loop result
    assert call(n=-1) == 1 and call(patches=None) == 1
    for ok in (P.FuseParams(0, 0, 0.0, float("-inf")), P.FuseParams(P.PIXEL_MAX_RADIUS, 255, 1e30, float("inf"))):
        assert call(prm=ok) == 0                         # the ends of the ranges are inside
    bad = recs[:4].copy()
    bad["num_images"][2] = 0
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.fuse_patches(bad)


def test_loop_fuse_matches_restatement(gpu_available, oracle_mod):
    """A real loop result (test_gpu_pixel_maps.py's `looped` shape): loop_fuse equals fuse_patches of the
    fetched records and the restatement, and changes nothing in the model (the fetch is what consumes
    it, so it comes after the loop form's calls)."""
    import pmvs_amd as P
    inp, p = P.synth_scene(6, 480, 360, level=1, supersample=2, num_targets=4)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    try:
        cands = P.synth_candidates(p, inp.projections, 300, seed=3)
        r, _ = g.refine_batch(cands)
        n, _ = g.run_loop(P.patches_from_refined(r), inp.threshold, iterations=2, wave=256, fetch=False)
        h = g.loop_hash()
        wr = g.loop_fuse(writer_order=True)                      # radius = csize, the CLI's parameters
        dv = g.loop_fuse(writer_order=True, device=True)
        mo = g.loop_fuse(writer_order=False)
        assert g.loop_hash() == h
        # with a loop result on the device the loop form's argument checks are what rejects a call
        buf, cnt = P.FuseBuffers(), C.c_int64(0)

        def loop(flags=0, first=0, num=4, prm=P.FuseParams(inp.csize, 2, 0.01, 0.5), cap=0):
            return g.lib.pmvs_loop_fuse(g.handle, flags, first, num, C.byref(prm), cap, C.byref(buf), C.byref(cnt))

        assert loop() == 0 and cnt.value == len(mo["pixel"])
        assert loop(flags=4) == 1 and loop(first=3, num=2) == 1 and loop(num=0) == 1 and loop(cap=-1) == 1
        assert loop(prm=P.FuseParams(17, 2, 0.01, 0.5)) == 1 and loop(prm=P.FuseParams(2, 256, 0.01, 0.5)) == 1
        assert loop(prm=P.FuseParams(2, 2, -1.0, 0.5)) == 1 and loop(prm=P.FuseParams(2, 2, 0.01, float("nan"))) == 1
        assert g.loop_hash() == h
        src = g.loop_export(writer_order=True, arrays=("source",))["source"]
        model = g.loop_fetch(n)
        assert n > 1000 and len(model) == n
        assert_same(dv, wr)
        assert_same(g.fuse_patches(model, writer_order=True), wr)
        assert_same(g.fuse_patches(model, writer_order=False), mo)
        for rows, got in ((src, wr), (np.arange(n), mo)):
            f = Fusion(o, inp, restate(o, inp, model, rows, inp.csize)[0], range(4))
            want, a = f.fuse(0.01, 0.5, 2)
            assert_same(got, want)
            assert len(want["pixel"]) > 0 and (a["passing"] & ~a["emit"]).any()
    finally:
        g.close()
        o.close()


def test_fuse_filled_but_invalid_pixels(gpu_available, oracle_mod):
    """Filled pixels whose point is not finite in float32: support 0, never passing, never emitted, not even
    at min_support 0 -- what the pass flags carry and the support byte cannot.  Target 0 gets the camera
    [I | 0] at the scene's level (one pixel per unit of x / z) and sees only a patch at depth 3e38 facing
    it, the 3 x 3 pixels its footprint keeps at the image corner; at the five with u = 2 or v = 2 the ray
    meets its plane beyond the largest float.  The other records lie behind that camera and are what the other targets see."""
    import pmvs_amd as P
    inp, _ = P.synth_scene(4, 128, 96, level=1, num_targets=3)
    inp.projections[0] = np.array([[2, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 0]], np.float32)
    recs = surface_records(P)
    recs = recs[recs["coord"][:, 2] < -0.05][:400].copy()
    recs["images"] = np.minimum(recs["images"], 3)
    recs["coord"][0], recs["normal"][0] = (0, 0, 3e38, 1), (0, 0, -1, 0)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    try:
        f = Fusion(o, inp, restate(o, inp, recs, np.arange(len(recs)), RADIUS)[0], range(3))
        bad = f.filled & ~f.valid
        assert np.nonzero(bad)[0].tolist() == [2, 66, 128, 129, 130] and (f.maps["patch"][bad] == 0).all()
        for prm in ((0.01, 0.5, 0), (0.01, 0.5, 1)):
            want, a = f.fuse(*prm)
            assert not a["passing"][bad].any() and not want["support_map"][bad].any()
            assert (want["patch"] == 0).sum() == (4 if prm[2] == 0 else 0)   # its valid pixels pass at 0 only
            assert len(want["pixel"]) > 4 and not np.isin(np.nonzero(bad)[0], want["pixel"]).any()
            for device in (False, True):
                got = g.fuse_patches(recs, writer_order=False, device=device, **kw(prm))
                assert_same(got, want)
    finally:
        g.close()
        o.close()
