"""pmvs_loop_brick_tsdf / pmvs_brick_tsdf_patches: the TSDF in a sparse volume of 8 x 8 x 8-voxel bricks.
Which bricks exist is compared with a numpy restatement of the SELECTION block of include/pmvs_amd.h, from
test_gpu_fuse.py's Fusion (the points Sf and the pass flags) alone, in float64 operations in the block's order.
The stored voxels are compared, byte for byte, with the dense GPU path (tsdf_patches on the same volume) and with
test_gpu_tsdf.py's restated integration; the overhang of the edge bricks must read (1.0f, 0, 0).

The scene and records are test_gpu_tsdf.py's; the volume keeps its origin and voxel with dims (42, 37, 33), no
multiple of 8 on any axis, so every high face has bricks that overhang.  The fixture asserts on the restatement
alone that some grid bricks stay unselected, that a passing pixel is skipped by step 3, that boxes are clipped
at a low and at a high face and that a box spans three bricks on an axis."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_depth_maps import order_keys
from test_gpu_fuse import RADIUS, Fusion
from test_gpu_pixel_maps import restate
from test_gpu_tsdf import ORIGIN, PARAMS, SUB, TRUNC, VOXEL, integrate, kw, volume_case  # noqa: F401 -- volume_case is a fixture

pytestmark = pytest.mark.gpu

NAMES = ("brick", "tsdf", "obs", "color")
BDIMS = (42, 37, 33)
MARGINS = (0, 1, 5)
SUB_PRM = PARAMS[1]  # two targets support a pixel once at most: min_support 2 would pass none


def grid_of(vol):
    return [(int(d) + 7) // 8 for d in vol.dims]


def select(Sf, passing, vol, margin):
    """The selection's definition: the ascending keys and what the boxes did."""
    origin, voxel = [np.float64(np.float32(x)) for x in vol.origin], np.float64(np.float32(vol.voxel))
    last = np.array([int(d) - 1 for d in vol.dims], np.float64)
    S = Sf[passing].astype(np.float64)
    g = np.stack([np.floor((S[:, a] - origin[a]) / voxel) for a in range(3)], 1)
    skip = ((g + margin < 0) | (g - margin > last)).any(1)
    g = g[~skip]
    lo, hi = np.maximum(0.0, g - margin).astype(np.int64), np.minimum(last, g + margin).astype(np.int64)
    B = grid_of(vol)
    chosen = np.zeros((B[2], B[1], B[0]), bool)
    for r in np.unique(np.concatenate([lo >> 3, hi >> 3], 1), axis=0):
        chosen[r[2]:r[5] + 1, r[1]:r[4] + 1, r[0]:r[3] + 1] = True
    stats = {"skipped": int(skip.sum()), "clipped_low": bool((g - margin < 0).any()), "clipped_high": bool((g + margin > last).any()),
             "span3": bool((((hi >> 3) - (lo >> 3)) >= 2).any()), "unselected": int((~chosen).sum())}
    return np.nonzero(chosen.ravel())[0].astype(np.int64), stats


def brick_voxels(keys, vol):
    """The virtual (i, j, k) of every stored voxel, each [b, 8, 8, 8] ([lk, lj, li]), and the inside-dims mask."""
    B = grid_of(vol)
    keys = np.asarray(keys, np.int64)
    b = [keys % B[0], (keys // B[0]) % B[1], keys // (B[0] * B[1])]
    lk, lj, li = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    ijk = [8 * b[a][:, None, None, None] + loc[None] for a, loc in enumerate((li, lj, lk))]
    inside = (ijk[0] < vol.dims[0]) & (ijk[1] < vol.dims[1]) & (ijk[2] < vol.dims[2])
    return ijk, inside


def scatter(vol, bricks):
    """The bricks' voxels inside the dims scattered into dense arrays pre-filled with (1.0f, 0, 0)."""
    nx, ny, nz = vol.dims
    out = {"tsdf": np.ones((nz, ny, nx), np.float32), "obs": np.zeros((nz, ny, nx), np.uint8), "color": np.zeros((nz, ny, nx, 4), np.uint8)}
    (i, j, k), inside = brick_voxels(bricks["brick"], vol)
    for name in out:
        if name in bricks and bricks[name] is not None:
            out[name][k[inside], j[inside], i[inside]] = np.asarray(bricks[name])[inside]
    return out


def host(arrays):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in arrays.items()}


def assert_bricks(got, keys, dense, vol, names=NAMES):
    """`got` holds exactly the bricks `keys`, the dense arrays' bytes inside the dims and (1, 0, 0) in the overhang."""
    got = host(got)
    assert set(got) == set(names)
    b = len(keys)
    shapes = {"brick": ((b,), np.int64), "tsdf": ((b, 8, 8, 8), np.float32), "obs": ((b, 8, 8, 8), np.uint8), "color": ((b, 8, 8, 8, 4), np.uint8)}
    for k in names:
        assert got[k].shape == shapes[k][0] and got[k].dtype == shapes[k][1], k
    if "brick" in names:
        assert got["brick"].tobytes() == keys.tobytes()
    (i, j, k), inside = brick_voxels(keys, vol)
    fill = {"tsdf": np.float32(1.0), "obs": np.uint8(0), "color": np.zeros(4, np.uint8)}
    for name in names:
        if name == "brick":
            continue
        assert got[name][inside].tobytes() == dense[name][k[inside], j[inside], i[inside]].tobytes(), name
        assert (got[name][~inside] == fill[name]).all(), name


@pytest.fixture(scope="module")
def brick_case(volume_case):
    """Shared with tests/test_gpu_brick_mesh.py: volume_case's scene and records, the (42, 37, 33) volume, and per
    parameter set (and for the sub-range) the points, the pass flags, the restated dense volume and the restated
    selection for every margin."""
    P, g, o, inp, recs, vol, want, aux = volume_case
    order = np.argsort(order_keys(recs, inp), kind="stable")
    bvol = P.volume(ORIGIN, VOXEL, BDIMS)
    full = Fusion(o, inp, restate(o, inp, recs, order, RADIUS)[0], range(4))
    part = Fusion(o, inp, restate(o, inp, recs, order, RADIUS, targets=SUB)[0], SUB)
    case = {prm: (full, full.fuse(*prm)[1]["passing"], {}) for prm in PARAMS}
    case["sub"] = (part, part.fuse(*SUB_PRM)[1]["passing"], dict(first_target=SUB[0], num_targets=len(SUB)))
    dense, keys, stats = {}, {}, {}
    for c, (fus, passing, _) in case.items():
        dense[c] = integrate(o, inp, fus, passing, bvol, TRUNC)[0]
        for m in MARGINS:
            keys[c, m], stats[c, m] = select(fus.Sf, passing, bvol, m)
    # coverage, on the restatement alone
    assert all(BDIMS[a] % 8 for a in range(3))                        # every high face has overhanging bricks
    assert all(s["unselected"] > 0 for s in stats.values())           # some grid bricks are never stored
    assert all(len(k) > 0 for k in keys.values())
    assert stats[PARAMS[1], 0]["skipped"] > 0                         # a floater outside the volume, skipped by step 3
    assert any(s["clipped_low"] for s in stats.values()) and any(s["clipped_high"] for s in stats.values())
    assert stats[PARAMS[0], 5]["span3"] and not stats[PARAMS[0], 0]["span3"]
    assert len(keys[PARAMS[0], 0]) < len(keys[PARAMS[0], 1]) < len(keys[PARAMS[0], 5])
    assert keys[PARAMS[0], 1].tobytes() != keys["sub", 1].tobytes()
    return P, g, recs, bvol, case, dense, keys, stats


def prm_of(c):
    return SUB_PRM if c == "sub" else c


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("c", list(PARAMS) + ["sub"])
def test_brick_selection_matches_restatement(brick_case, c, margin):
    P, g, recs, bvol, case, dense, keys, stats = brick_case
    got = g.brick_tsdf_patches(recs, bvol, TRUNC, margin, writer_order=True, arrays=("brick",), **case[c][2], **kw(prm_of(c)))
    assert got["brick"].dtype == np.int64 and got["brick"].tobytes() == keys[c, margin].tobytes()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("prm", PARAMS)
def test_brick_values_match_dense(brick_case, prm, device):
    """Every stored voxel inside the dims: the dense GPU path's bytes and the restated integration's."""
    P, g, recs, bvol, case, dense, keys, stats = brick_case
    got = g.brick_tsdf_patches(recs, bvol, TRUNC, 1, writer_order=True, device=device, **kw(prm))
    if device:
        assert all(t.is_cuda and t.device.index == g.device for t in got.values())
    assert_bricks(got, keys[prm, 1], dense[prm], bvol)
    gpu_dense = g.tsdf_patches(recs, bvol, TRUNC, writer_order=True, **kw(prm))
    assert_bricks(got, keys[prm, 1], gpu_dense, bvol)
    (i, j, k), inside = brick_voxels(keys[prm, 1], bvol)
    assert (~inside).any() and (host(got)["obs"][inside] > 0).any()


def test_brick_sub_range_values(brick_case):
    P, g, recs, bvol, case, dense, keys, stats = brick_case
    got = g.brick_tsdf_patches(recs, bvol, TRUNC, 5, writer_order=True, **case["sub"][2], **kw(SUB_PRM))
    assert_bricks(got, keys["sub", 5], dense["sub"], bvol)


def raw_call(P, g, recs, vol, margin, bcap, arrays, prm=PARAMS[0], flags=1):
    """pmvs_brick_tsdf_patches through ctypes with caller-made host arrays; returns (status, nbricks)."""
    pa = np.ascontiguousarray(recs, P.PATCH_DTYPE)
    buf = P.BrickBuffers()
    for k, a in arrays.items():
        setattr(buf, k, a.ctypes.data)
    bp = P.BrickParams(P.TsdfParams(P.FuseParams(RADIUS, prm[2], prm[0], prm[1]), TRUNC), margin)
    nb = C.c_int64(-1)
    st = g.lib.pmvs_brick_tsdf_patches(g.handle, pa.ctypes.data, len(pa), flags, 0, 4, C.byref(bp), C.byref(vol), bcap, C.byref(buf),
                                       C.byref(nb))
    return st, int(nb.value)


def test_brick_caps_and_counting_call(brick_case):
    P, g, recs, bvol, case, dense, keys, stats = brick_case
    want = keys[PARAMS[0], 1]
    n = len(want)
    assert raw_call(P, g, recs, bvol, 1, 0, {}) == (0, n)            # the counting call: every pointer NULL
    bcap, guard = n // 3, 5
    assert 0 < bcap < n
    shapes = {"brick": ((), np.int64), "tsdf": ((8, 8, 8), np.float32), "obs": ((8, 8, 8), np.uint8), "color": ((8, 8, 8, 4), np.uint8)}
    arrays = {k: np.full((bcap + guard,) + s, 0x5A, dt) for k, (s, dt) in shapes.items()}
    assert raw_call(P, g, recs, bvol, 1, bcap, arrays) == (0, n)     # the count is the total, not what was written
    assert_bricks({k: a[:bcap] for k, a in arrays.items()}, want[:bcap], dense[PARAMS[0]], bvol)
    for k, (s, dt) in shapes.items():
        assert (arrays[k][bcap:] == np.array(0x5A, dt)).all(), k    # nothing past the prefix
    # a cap beyond the count, however large, writes the count
    big = {"brick": np.full(n + guard, -7, np.int64), "obs": np.full((n + guard, 8, 8, 8), 0x5A, np.uint8)}
    assert raw_call(P, g, recs, bvol, 1, 2 ** 62, big) == (0, n)
    assert_bricks({k: a[:n] for k, a in big.items()}, want, dense[PARAMS[0]], bvol, ("brick", "obs"))
    assert (big["brick"][n:] == -7).all() and (big["obs"][n:] == 0x5A).all()
    # selected arrays: a NULL array is skipped, the key list included
    got = g.brick_tsdf_patches(recs, bvol, TRUNC, 1, writer_order=True, arrays=("tsdf", "color"), **kw(PARAMS[0]))
    assert_bricks(got, want, dense[PARAMS[0]], bvol, ("tsdf", "color"))


def test_brick_errors(brick_case):
    P, g, recs, bvol, case, dense, keys, stats = brick_case
    with pytest.raises(P.PmvsError, match="pmvs status 1:"):       # no run_loop on this scene
        g.loop_brick_tsdf(bvol, TRUNC, 1)
    with pytest.raises(P.PmvsError, match="pmvs status 1:"):
        g.loop_brick_mesh(bvol, TRUNC, 1)
    for margin in (-1, 65):
        assert raw_call(P, g, recs, bvol, margin, 0, {}) == (1, -1)
    assert raw_call(P, g, recs, bvol, 64, 0, {})[0] == 0
    assert raw_call(P, g, recs, bvol, 1, -1, {}) == (1, -1)          # a negative cap
    # a dim past 2^20, a dim of 0, and brick grids of 2^37 and of exactly 2^31 bricks
    for dims in ((2 ** 20 + 1, 8, 8), (8, 0, 8), (2 ** 20, 2 ** 20, 64), (2 ** 20, 2 ** 17, 8)):
        assert raw_call(P, g, recs, P.volume(ORIGIN, VOXEL, dims), 1, 0, {}) == (1, -1), dims
