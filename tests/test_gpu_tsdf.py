"""pmvs_loop_tsdf / pmvs_tsdf_patches: the fused maps integrated into a truncated signed distance volume.
There is no reference for this: the expected arrays are a numpy restatement of the integration's definition in
include/pmvs_amd.h, built on test_gpu_fuse.py's Fusion (the maps, the pass flags, the level images) and on
OracleScene.project / .depth alone, in explicit element-wise float64 operations in the definition's order, the
float parameters rounded to float32 before they are widened.  tsdf, obs and color are compared for exact
equality of dtype, shape and bytes; nothing is excluded.

The scene and model are test_gpu_fuse.py's (4 targets at 160 x 120, one cropped; a sphere of radius 0.45 with an
occluded inner sphere, floaters and tilted normals) and the volume is 40 x 36 x 32 voxels of 0.05 whose lowest z
face cuts the sphere and whose far corners project outside the images, the dims unequal so that an index-order
mix-up shows.  The fixture asserts on the restatement alone that every branch of the definition occurs
but one: `z > 0` never decides, since the optical axis is the projection's third row scaled, so a point that
projects into an image has a positive depth there."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_depth_maps import crafted_scene, order_keys
from test_gpu_fuse import RADIUS, Fusion, surface_records
from test_gpu_pixel_maps import image_dims, restate

pytestmark = pytest.mark.gpu

NAMES = ("tsdf", "obs", "color")
PARAMS = ((0.01, 0.5, 2), (0.01, 0.5, 0))  # depth_rel, normal_cos, min_support
ORIGIN, VOXEL, DIMS, TRUNC = (-0.7, -0.9, -0.33), 0.05, (40, 36, 32), 0.15
SUB = (1, 2)  # the sub-range of targets


def voxel_centres(vol):
    """[voxels, 4] float32 (Cf, 1) in voxel-index order, and the (i, j, k) of every voxel."""
    nx, ny, nz = vol.dims
    idx = np.arange(nx * ny * nz, dtype=np.int64)
    ijk = [idx % nx, (idx // nx) % ny, idx // (nx * ny)]
    voxel = np.float64(np.float32(vol.voxel))
    c = [(np.float64(np.float32(vol.origin[a])) + (ijk[a].astype(np.float64) + 0.5) * voxel).astype(np.float32) for a in range(3)]
    return np.stack(c + [np.ones(len(idx), np.float32)], axis=1), ijk


def integrate(o, inp, fus, passing, vol, trunc):
    """The integration's definition over fus.targets, from the maps of `fus` and the pass flags `passing`."""
    c4, _ = voxel_centres(vol)
    nvox = len(c4)
    tr = np.float64(np.float32(trunc))
    total = np.zeros(nvox, np.float64)
    n, nc = np.zeros(nvox, np.int64), np.zeros(nvox, np.int64)
    csum = np.zeros((nvox, 3), np.int64)
    stats = {"outside": 0, "not_passing": 0, "behind_camera": 0, "hidden": 0, "clamped": 0, "band_pos": 0, "band_neg": 0}
    dims = [image_dims(inp)[t] for t in fus.targets]
    for j, t in enumerate(fus.targets):
        W, H = dims[j]
        xy = o.project(t, inp.level, c4)
        px, py = np.floor(xy[:, 0].astype(np.float64) + 0.5), np.floor(xy[:, 1].astype(np.float64) + 0.5)
        with np.errstate(invalid="ignore"):
            inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)  # in double: a NaN fails
        q = np.where(inside, int(fus.off[j]) + np.where(inside, py, 0).astype(np.int64) * W + np.where(inside, px, 0).astype(np.int64), 0)
        ok = inside & passing[q]
        z = o.depth(t, c4)
        front = ok & (z > 0)
        s = fus.maps["depth"][q].astype(np.float64) - z.astype(np.float64)
        with np.errstate(invalid="ignore"):
            seen = front & (s >= -tr)
            v = np.where(s >= tr, 1.0, s / tr)
            band = seen & (s < tr)
        total = total + np.where(seen, v, 0.0)
        n += seen
        csum += np.where(band[:, None], fus.color[q].astype(np.int64), 0)
        nc += band
        stats["outside"] += int((~inside).sum())
        stats["not_passing"] += int((inside & ~ok).sum())
        stats["behind_camera"] += int((ok & ~front).sum())
        stats["hidden"] += int((front & ~seen).sum())
        stats["clamped"] += int((seen & ~band).sum())
        stats["band_pos"] += int((band & (s > 0)).sum())
        stats["band_neg"] += int((band & (s < 0)).sum())
    nx, ny, nz = vol.dims
    with np.errstate(invalid="ignore", divide="ignore"):
        tsdf = np.where(n > 0, (total / n.astype(np.float64)).astype(np.float32), np.float32(1.0)).astype(np.float32)
    color = np.zeros((nvox, 4), np.uint8)
    has = nc > 0
    color[has, :3] = ((csum[has] + (nc[has] // 2)[:, None]) // nc[has][:, None]).astype(np.uint8)
    color[has, 3] = 255
    out = {"tsdf": tsdf.reshape(nz, ny, nx), "obs": np.minimum(n, 255).astype(np.uint8).reshape(nz, ny, nx),
           "color": color.reshape(nz, ny, nx, 4)}
    return out, {"stats": stats, "n": n, "nc": nc}


def assert_same(got, want, names=NAMES):
    assert set(got) == set(names)
    for k in names:
        a = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        assert a.dtype == want[k].dtype and a.shape == want[k].shape, k
        assert a.tobytes() == want[k].tobytes(), k


def kw(prm):
    return dict(radius=RADIUS, depth_rel=prm[0], normal_cos=prm[1], min_support=prm[2])


@pytest.fixture(scope="module")
def volume_case(gpu_available, oracle_mod):
    """Shared with tests/test_gpu_mesh.py: the scene, the records, and per parameter set the restated volume
    over all targets in writer order (and over SUB for the first set)."""
    import pmvs_amd as P
    inp = crafted_scene(P)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    recs = surface_records(P)
    order = np.argsort(order_keys(recs, inp), kind="stable")
    vol = P.volume(ORIGIN, VOXEL, DIMS)
    fus = Fusion(o, inp, restate(o, inp, recs, order, RADIUS)[0], range(4))
    want, aux = {}, {}
    for prm in PARAMS:
        want[prm], aux[prm] = integrate(o, inp, fus, fus.fuse(*prm)[1]["passing"], vol, TRUNC)
    part = Fusion(o, inp, restate(o, inp, recs, order, RADIUS, targets=SUB)[0], SUB)
    want["sub"], aux["sub"] = integrate(o, inp, part, part.fuse(*PARAMS[0])[1]["passing"], vol, TRUNC)
    # coverage, on the restatement alone
    for prm in PARAMS:
        w, a = want[prm], aux[prm]
        st = a["stats"]
        assert (a["n"] == 0).any() and (w["tsdf"].reshape(-1)[a["n"] == 0] == 1.0).all()   # an unobserved voxel
        assert st["clamped"] > 0 and (w["tsdf"] == 1.0).sum() > (a["n"] == 0).sum()         # a voxel clamped at 1
        assert st["band_pos"] > 0 and st["band_neg"] > 0                                    # inside the band, each sign
        assert ((w["tsdf"] > 0) & (w["tsdf"] < 1)).any() and (w["tsdf"] < 0).any()
        assert st["hidden"] > 0                                                             # hidden by more than trunc
        assert ((a["nc"] == 0) & (a["n"] > 0)).any()                                        # observed, no colour
        assert st["outside"] > 0 and st["not_passing"] > 0
        assert set(np.unique(w["obs"])) >= {0, 1, 2}
    assert want[PARAMS[0]]["tsdf"].tobytes() != want[PARAMS[1]]["tsdf"].tobytes()
    assert want[PARAMS[0]]["tsdf"].tobytes() != want["sub"]["tsdf"].tobytes()
    yield P, g, o, inp, recs, vol, want, aux
    g.close()
    o.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("prm", PARAMS)
def test_tsdf_matches_restatement(volume_case, prm, device):
    P, g, o, inp, recs, vol, want, aux = volume_case
    got = g.tsdf_patches(recs, vol, TRUNC, writer_order=True, device=device, **kw(prm))
    if device:
        assert all(t.is_cuda and t.device.index == g.device for t in got.values())
    assert_same(got, want[prm])


def test_tsdf_sub_range(volume_case):
    """Targets [1, 3) alone: the maps, the pass flags and the observations of those two."""
    P, g, o, inp, recs, vol, want, aux = volume_case
    got = g.tsdf_patches(recs, vol, TRUNC, writer_order=True, first_target=SUB[0], num_targets=len(SUB), **kw(PARAMS[0]))
    assert_same(got, want["sub"])
    assert got["obs"].max() <= 2


def test_tsdf_selected_arrays_and_model_order(volume_case):
    """A NULL array is skipped and the others do not change; without the writer order the maps differ where
    two patches tie, so the call only has to succeed with the same shapes."""
    P, g, o, inp, recs, vol, want, aux = volume_case
    got = g.tsdf_patches(recs, vol, TRUNC, writer_order=True, arrays=("obs",), **kw(PARAMS[0]))
    assert_same(got, want[PARAMS[0]], ("obs",))
    got = g.tsdf_patches(recs, vol, TRUNC, writer_order=False, device=True, arrays=("tsdf", "color"), **kw(PARAMS[0]))
    assert got["tsdf"].shape == (32, 36, 40) and got["color"].shape == (32, 36, 40, 4)


def test_tsdf_errors(volume_case):
    P, g, o, inp, recs, vol, want, aux = volume_case
    with pytest.raises(P.PmvsError, match="pmvs status 1:"):   # no run_loop on this scene
        g.loop_tsdf(vol, TRUNC)
    lib, pa = g.lib, np.ascontiguousarray(recs[:4], P.PATCH_DTYPE)
    good, buf = P.TsdfParams(P.FuseParams(RADIUS, 2, 0.01, 0.5), TRUNC), P.TsdfBuffers()
    small = P.volume(ORIGIN, VOXEL, (3, 2, 2))

    def ref(x):
        return None if x is None else C.byref(x)

    def call(flags=0, first=0, num=4, prm=good, v=small, b=buf, scene=g.handle, patches=pa.ctypes.data, n=4):
        return lib.pmvs_tsdf_patches(scene, patches, n, flags, first, num, ref(prm), ref(v), ref(b))

    def loop(flags=0, first=0, num=4, prm=good, v=small, b=buf, scene=g.handle):
        return lib.pmvs_loop_tsdf(scene, flags, first, num, ref(prm), ref(v), ref(b))

    nan, inf = float("nan"), float("inf")
    assert call() == 0
    for f in (call, loop):
        assert f(scene=None) == 1 and f(prm=None) == 1 and f(v=None) == 1 and f(b=None) == 1
        for flags in (4, 8, 1 | 16, -1):
            assert f(flags=flags) == 1
        for first, num in ((-1, 1), (0, 0), (3, 2), (4, 1)):
            assert f(first=first, num=num) == 1
        for trunc in (0.0, -0.1, nan, inf):
            assert f(prm=P.TsdfParams(P.FuseParams(RADIUS, 2, 0.01, 0.5), trunc)) == 1
        for fp in (P.FuseParams(-1, 2, 0.01, 0.5), P.FuseParams(RADIUS, 256, 0.01, 0.5), P.FuseParams(RADIUS, 2, nan, 0.5)):
            assert f(prm=P.TsdfParams(fp, TRUNC)) == 1    # the fuse checks, inherited
        for bad in (P.volume((nan, 0, 0), VOXEL, (3, 2, 2)), P.volume((0, 0, -inf), VOXEL, (3, 2, 2)),
                    P.volume(ORIGIN, 0.0, (3, 2, 2)), P.volume(ORIGIN, -VOXEL, (3, 2, 2)), P.volume(ORIGIN, nan, (3, 2, 2)),
                    P.volume(ORIGIN, inf, (3, 2, 2)), P.volume(ORIGIN, VOXEL, (0, 2, 2)), P.volume(ORIGIN, VOXEL, (3, 2, -2)),
                    P.volume(ORIGIN, VOXEL, (2048, 1024, 1024)), P.volume(ORIGIN, VOXEL, (65536, 65536, 1))):
            assert f(v=bad) == 1
    assert loop() == 1                                    # valid arguments, but no loop result
    assert call(n=-1) == 1 and call(patches=None) == 1
    assert call(v=P.volume(ORIGIN, VOXEL, (1, 1, 1))) == 0  # one voxel is a volume
