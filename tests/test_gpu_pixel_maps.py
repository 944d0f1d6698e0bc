"""pmvs_loop_pixel_maps / pmvs_pixel_maps_patches: the model rendered into the target images, one depth
and one normal per pixel.  The expected maps are a numpy restatement of the definition in
include/pmvs_amd.h, built only from OracleScene.project, .depth and .camera: explicit element-wise
float64 products and sums in the definition's order (no `@`, no np.dot: their summation order is not
defined).  Every array is compared for exact equality of dtype, shape and bytes.

The restatement itself is checked independently: for the winners that took the plane branch,
np.linalg.solve of the same 3 x 3 system gives the f32 depth within 1 ulp -- one f32 rounding of two f64
results that agree to far below half an f32 ulp, because the facing test bounds the system's
conditioning."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_depth_maps import COPIES, crafted_scene, order_keys
from test_gpu_depth_maps import crafted_records as depth_map_records

pytestmark = pytest.mark.gpu

NAMES = ("patch", "depth", "normal", "ncc")
EINVAL = "pmvs status 1:"
RADII = (0, 2, 5)
TILE = 32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def image_dims(inp):
    return [(im.shape[1] >> inp.level, im.shape[0] >> inp.level) for im in inp.images[:inp.num_targets]]


def depth_bits(d):
    u = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def depth_from_bits(b):
    b = b.astype(np.uint32)
    return np.where(b & np.uint32(0x80000000), b & np.uint32(0x7FFFFFFF), ~b).astype(np.uint32).view(np.float32)


def crafted_records(P):
    """test_gpu_depth_maps.py's 1500 records (+-0.5 coordinates, 300 at +-1.6, 3 far outside or behind
    cameras, random normals), with the 40 copies made exact: here a patch's depth depends on its normal
    too, so rows 1300-1339 take the normals of rows 100-139 as well as their coordinates.  Their ncc
    still differs, so a wrong winner of a tie shows."""
    r = depth_map_records(P)
    r["normal"][1300:1340] = r["normal"][100:140]
    assert not np.array_equal(r["ncc"][1300:1340], r["ncc"][100:140])
    return r


def restate_target(o, inp, W, H, t, coords, normals, R):
    """Target t's winning key per pixel and what the coverage conditions and the independent check
    need: per (row, footprint pixel) pair the row, the pixel, the key and whether the plane branch gave
    the depth."""
    xy = o.project(t, inp.level, coords)
    z = o.depth(t, coords)
    cam = o.camera(t, inp.level).astype(np.float64)
    centre, oaxis, Pm = cam[0:4], cam[4:8], cam[18:30]
    cx = np.floor(xy[:, 0].astype(np.float64) + 0.5)
    cy = np.floor(xy[:, 1].astype(np.float64) + 0.5)
    offs = np.arange(-R, R + 1, dtype=np.float64)
    U = cx[:, None, None] + offs[None, None, :] + 0.0 * offs[None, :, None]
    V = cy[:, None, None] + offs[None, :, None] + 0.0 * offs[None, None, :]
    with np.errstate(invalid="ignore"):
        inside = (U >= 0) & (U < W) & (V >= 0) & (V < H)  # in double: a NaN fails
    r = np.nonzero(inside)[0]
    u, v = U[inside], V[inside]
    X = [coords[r, k].astype(np.float64) for k in range(3)]
    N = [normals[r, k].astype(np.float64) for k in range(3)]
    Vc = [centre[k] - X[k] for k in range(3)]
    nv = N[0] * Vc[0] + N[1] * Vc[1] + N[2] * Vc[2]
    nn = N[0] * N[0] + N[1] * N[1] + N[2] * N[2]
    vv = Vc[0] * Vc[0] + Vc[1] * Vc[1] + Vc[2] * Vc[2]
    facing = (nv > 0.0) & (nv * nv >= 0.0625 * (nn * vv))
    a = [Pm[k] - u * Pm[8 + k] for k in range(4)]
    b = [Pm[4 + k] - v * Pm[8 + k] for k in range(4)]

    def cross(p, q):
        return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]

    bn, na, ab = cross(b, N), cross(N, a), cross(a, b)
    det = a[0] * bn[0] + a[1] * bn[1] + a[2] * bn[2]
    r0, r1, r2 = -a[3], -b[3], N[0] * X[0] + N[1] * X[1] + N[2] * X[2]
    with np.errstate(all="ignore"):
        S = [(r0 * bn[k] + r1 * na[k] + r2 * ab[k]) / det for k in range(3)]
        dp = (oaxis[0] * S[0] + oaxis[1] * S[1] + oaxis[2] * S[2] + oaxis[3]).astype(np.float32)
        plane = facing & np.isfinite(dp) & (dp > 0)
    d = np.where(plane, dp, z[r]).astype(np.float32)
    key = (depth_bits(d).astype(np.uint64) << np.uint64(32)) | r.astype(np.uint64)
    pix = v.astype(np.int64) * W + u.astype(np.int64)
    best = np.full(W * H, EMPTY, np.uint64)
    np.minimum.at(best, pix, key)
    # footprints: cut by a border, and the tiles they span
    x0, x1 = np.maximum(cx - R, 0), np.minimum(cx + R, W - 1)
    y0, y1 = np.maximum(cy - R, 0), np.minimum(cy + R, H - 1)
    with np.errstate(invalid="ignore"):
        some = (x0 <= x1) & (y0 <= y1)
        cut = some & ((cx - R < 0) | (cx + R > W - 1) | (cy - R < 0) | (cy + R > H - 1))
        span = np.where(some, np.maximum(x1 // TILE - x0 // TILE, y1 // TILE - y0 // TILE), 0)
    aux = {"rows": r, "pix": pix, "key": key, "plane": plane, "cut": bool(cut.any()), "span": int(span.max(initial=0)),
           "system": (a, b, N, r0, r1, r2, oaxis)}
    return best, aux


def restate(o, inp, recs, rows, R, targets=None):
    """The four arrays for the records taken in the order `rows`, from the definition alone; and the
    per-target auxiliaries."""
    m = recs[rows]
    coords = np.ascontiguousarray(m["coord"], np.float32)
    normals = np.ascontiguousarray(m["normal"][:, :3], np.float32)
    dims = image_dims(inp)
    keys, auxs = [], []
    for t in (range(inp.num_targets) if targets is None else targets):
        best, aux = restate_target(o, inp, dims[t][0], dims[t][1], t, coords, normals, R)
        keys.append(best)
        auxs.append(aux)
    keys = np.concatenate(keys)
    filled = keys != EMPTY
    patch = np.where(filled, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(filled, depth_from_bits(keys >> np.uint64(32)), np.float32(0)).astype(np.float32)
    normal = np.zeros((len(keys), 3), np.float32)
    normal[filled] = normals[patch[filled]]
    ncc = np.zeros(len(keys), np.float32)
    ncc[filled] = m["ncc"][patch[filled]]
    return {"patch": patch, "depth": depth, "normal": normal, "ncc": ncc}, auxs, keys


def winners(aux, best):
    """The (row, pixel) pairs that won their pixel."""
    return best[aux["pix"]] == aux["key"]


def check_plane_winners(aux, best):
    """np.linalg.solve of the plane-branch winners' systems: the f32 depth within 1 ulp."""
    sel = winners(aux, best) & aux["plane"]
    a, b, N, r0, r1, r2, oaxis = aux["system"]
    M = np.stack([np.stack([a[k][sel] for k in range(3)], -1), np.stack([b[k][sel] for k in range(3)], -1),
                  np.stack([N[k][sel] for k in range(3)], -1)], -2)
    rhs = np.stack([r0[sel], r1[sel], r2[sel]], -1)[..., None]
    S = np.linalg.solve(M, rhs)[..., 0]
    d = (oaxis[0] * S[:, 0] + oaxis[1] * S[:, 1] + oaxis[2] * S[:, 2] + oaxis[3]).astype(np.float32)
    got = depth_from_bits(aux["key"][sel] >> np.uint64(32))
    assert (d > 0).all() and (got > 0).all()
    ulp = np.abs(d.view(np.int32).astype(np.int64) - got.view(np.int32).astype(np.int64))
    assert ulp.max(initial=0) <= 1
    return int(sel.sum())


def assert_same(got, want, names=NAMES, sl=slice(None)):
    assert set(got) == set(names)
    for k in names:
        a, w = np.asarray(got[k]), want[k][sl]
        assert a.dtype == w.dtype and a.shape == w.shape, k
        assert a.tobytes() == w.tobytes(), k


def check_empty_pixels(maps):
    e = maps["patch"] < 0
    assert (maps["patch"][e] == -1).all()
    for k in ("depth", "normal", "ncc"):
        assert not maps[k][e].view(np.uint32).any(), k  # +0.0 exactly


@pytest.fixture(scope="module")
def crafted(gpu_available, oracle_mod):
    import pmvs_amd as P
    inp = crafted_scene(P)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    recs = crafted_records(P)
    n = len(recs)
    order = np.argsort(order_keys(recs, inp), kind="stable")
    assert not np.array_equal(order, np.arange(n))
    assert image_dims(inp) == [(160, 120), (150, 100), (160, 120), (160, 120)]
    want = {}
    for R in RADII:
        for wo, rows in ((False, np.arange(n)), (True, order)):
            maps, auxs, keys = restate(o, inp, recs, rows, R)
            want[R, wo] = maps
            # coverage, on the restatement alone
            mo = maps["patch"]
            assert (mo < 0).any() and (mo >= 0).any()
            off, won, plane_won, checked = 0, 0, 0, 0
            for aux, (W, H) in zip(auxs, image_dims(inp)):
                best = keys[off:off + W * H]
                off += W * H
                w = winners(aux, best)
                won += int(w.sum())
                plane_won += int((w & aux["plane"]).sum())
                checked += check_plane_winners(aux, best)
            assert won == int((mo >= 0).sum()) and checked == plane_won
            assert 0.1 * won <= plane_won <= 0.9 * won          # both branches among the winners
            if R > 0:
                assert any(a["cut"] for a in auxs)                # a footprint cut by an image border
                assert max(a["span"] for a in auxs) >= 1          # and one that crosses a tile border
            if not wo:
                assert np.isin(mo, COPIES[0]).any() and not np.isin(mo, COPIES[1]).any()  # ties: the earlier row
                rev = restate(o, inp, recs, np.arange(n)[::-1], R)[0]["patch"]
                rev = np.where(rev >= 0, n - 1 - rev, -1)
                assert (rev != mo).any()                          # the order matters
    yield P, g, o, inp, recs, order, want
    g.close()
    o.close()


@pytest.fixture(scope="module")
def looped(gpu_available, oracle_mod):
    """One loop result left on the device (the shape of test_gpu_depth_maps.py's fixture)."""
    import pmvs_amd as P
    inp, p = P.synth_scene(6, 480, 360, level=1, supersample=2, num_targets=4)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    cands = P.synth_candidates(p, inp.projections, 300, seed=3)
    r, _ = g.refine_batch(cands)
    seeds = P.patches_from_refined(r)
    n, _ = g.run_loop(seeds, inp.threshold, iterations=2, wave=256, fetch=False)
    yield P, g, o, inp, n
    g.close()
    o.close()


def test_pixel_map_layout(crafted):
    P, g, o, inp, recs, order, want = crafted
    dims, off = g.pixel_map_layout()
    assert dims.dtype == np.int32 and off.dtype == np.int64
    assert dims.tolist() == [[160, 120], [150, 100], [160, 120], [160, 120]]
    assert off.tolist() == [0, 19200, 34200, 53400, 72600]
    dims, off = g.pixel_map_layout(1, 2)
    assert dims.tolist() == [[150, 100], [160, 120]] and off.tolist() == [0, 15000, 34200]
    v = P.depth_map_view(want[2, False]["normal"][19200:53400], dims, off, 0)
    assert v.shape == (100, 150, 3) and v.base is not None
    for first, num in ((-1, 1), (0, 0), (3, 2), (4, 1)):
        assert g.lib.pmvs_pixel_map_layout(g.handle, first, num, None, None) == 1


@pytest.mark.parametrize("writer_order", [False, True])
@pytest.mark.parametrize("radius", RADII)
def test_pixel_maps_crafted(crafted, radius, writer_order):
    P, g, o, inp, recs, order, want = crafted
    got = g.pixel_maps_patches(recs, writer_order=writer_order, radius=radius)
    assert_same(got, want[radius, writer_order])
    check_empty_pixels(got)
    part = g.pixel_maps_patches(recs, writer_order=writer_order, radius=radius, first_target=1, num_targets=2)
    assert_same(part, want[radius, writer_order], sl=slice(19200, 53400))


def test_pixel_maps_widest_radius(crafted):
    """Radius 16, the largest: footprints of 1089 pixels, on the 150 x 100 target, where most of them
    are cut by a border."""
    P, g, o, inp, recs, order, want = crafted
    maps, auxs, keys = restate(o, inp, recs, np.arange(len(recs)), P.PIXEL_MAX_RADIUS, targets=(1,))
    assert auxs[0]["span"] == 1 and auxs[0]["cut"] and (maps["patch"] >= 0).any()
    assert check_plane_winners(auxs[0], keys) > 0
    got = g.pixel_maps_patches(recs, writer_order=False, radius=P.PIXEL_MAX_RADIUS, first_target=1, num_targets=1)
    assert_same(got, maps)


def test_pixel_maps_device_mode_and_partial(crafted):
    P, g, o, inp, recs, order, want = crafted
    dv = g.pixel_maps_patches(recs, writer_order=True, device=True, radius=5)
    assert all(t.is_cuda and t.device.index == g.device for t in dv.values())
    assert_same({k: t.cpu().numpy() for k, t in dv.items()}, want[5, True])
    assert_same(g.pixel_maps_patches(recs, writer_order=True, radius=5), want[5, True])  # two calls, the same bytes
    assert_same(g.pixel_maps_patches(recs, writer_order=False, radius=2, arrays=("patch",)), want[2, False], ("patch",))
    # a request for patch alone writes nothing else: the other pointers stay NULL, and buffers the call
    # is not given keep their contents
    buf = P.DepthMapBuffers()
    patch = np.full(72600, 7, np.int32)
    buf.patch = patch.ctypes.data
    pa = np.ascontiguousarray(recs, P.PATCH_DTYPE)
    assert g.lib.pmvs_pixel_maps_patches(g.handle, pa.ctypes.data, len(pa), 0, 0, 4, 2, buf) == 0
    assert np.array_equal(patch, want[2, False]["patch"])
    assert_same(g.pixel_maps_patches(recs, writer_order=True, radius=0, arrays=("depth", "normal")), want[0, True],
                ("depth", "normal"))


def test_pixel_maps_no_records(crafted):
    P, g, o, inp, recs, order, want = crafted
    for writer_order in (False, True):
        got = g.pixel_maps_patches(recs[:0], writer_order=writer_order)
        assert (got["patch"] == -1).all() and got["patch"].shape == (72600,)
        check_empty_pixels(got)


def test_loop_pixel_maps_match_restatement(looped):
    P, g, o, inp, n = looped
    h = g.loop_hash()
    ex = g.loop_export(writer_order=True)
    wr = g.loop_pixel_maps(writer_order=True)      # radius = csize
    mo = g.loop_pixel_maps(writer_order=False)
    dv = g.loop_pixel_maps(writer_order=True, device=True)
    assert g.loop_hash() == h                      # the maps change nothing in the model
    assert_same({k: t.cpu().numpy() for k, t in dv.items()}, wr)
    ex2 = g.loop_export(writer_order=True)         # and do not consume it
    assert set(ex2) == set(ex) and all(ex2[k].tobytes() == ex[k].tobytes() for k in ex)
    model = g.loop_fetch(n)                        # still there (the fetch is what consumes it)
    assert n > 1000 and len(model) == n
    src = ex["source"]
    assert np.array_equal(ex["fields"][:, :4], model["coord"][src])
    assert np.array_equal(ex["fields"][:, 4:8], model["normal"][src])
    assert image_dims(inp) == [(240, 180)] * 4 and wr["patch"].shape == (4 * 240 * 180,)
    assert_same(wr, restate(o, inp, model, src, inp.csize)[0])
    assert_same(mo, restate(o, inp, model, np.arange(n), inp.csize)[0])
    assert (wr["patch"] >= 0).any() and (wr["patch"] < 0).any()
    check_empty_pixels(wr)


def test_pixel_maps_errors(crafted):
    P, g, o, inp, recs, order, want = crafted
    with pytest.raises(P.PmvsError, match=EINVAL):   # no run_loop on this scene yet
        g.loop_pixel_maps()
    buf = P.DepthMapBuffers()
    patch = np.zeros(72600, np.int32)
    buf.patch = patch.ctypes.data
    pa = np.ascontiguousarray(recs[:4], P.PATCH_DTYPE)
    assert g.lib.pmvs_pixel_maps_patches(g.handle, pa.ctypes.data, 4, 0, 0, 4, 2, buf) == 0
    for flags in (4, 8, 1 | 16, -1):                 # any bit beyond WRITER_ORDER | DEVICE
        assert g.lib.pmvs_pixel_maps_patches(g.handle, pa.ctypes.data, 4, flags, 0, 4, 2, buf) == 1
        assert g.lib.pmvs_loop_pixel_maps(g.handle, flags, 0, 4, 2, buf) == 1
    for first, num in ((-1, 1), (0, 0), (3, 2), (4, 1)):
        assert g.lib.pmvs_pixel_maps_patches(g.handle, pa.ctypes.data, 4, 0, first, num, 2, buf) == 1
        assert g.lib.pmvs_loop_pixel_maps(g.handle, 0, first, num, 2, buf) == 1
        with pytest.raises(P.PmvsError, match=EINVAL):
            g.pixel_maps_patches(recs[:4], first_target=first, num_targets=num)
    for radius in (-1, 17):
        assert g.lib.pmvs_pixel_maps_patches(g.handle, pa.ctypes.data, 4, 0, 0, 4, radius, buf) == 1
        with pytest.raises(P.PmvsError, match=EINVAL):
            g.pixel_maps_patches(recs[:4], radius=radius)
    bad = recs[:4].copy()
    bad["num_images"][2] = 0
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.pixel_maps_patches(bad)
