"""pmvs_brick_tsdf_mesh / pmvs_brick_mesh_patches: surface nets over a sparse volume of 8 x 8 x 8-voxel bricks.
The yardstick is the dense path: the brick extraction must give, byte for byte, what tsdf_mesh gives on the
bricks scattered into a dense volume pre-filled with (1.0f, 0, 0) -- and what test_gpu_mesh.py's restatement
extract() gives there -- in vertices, normals, colours, faces and both counts.  The arbitrary-brick case pins the
halo reads, the brick -> slot map and both sorts; the end-to-end cases pin the selection's margin and, with a
65536 x 65536 x 32 virtual volume, every 64-bit index."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_brick_tsdf import brick_case, brick_voxels, grid_of, scatter, select  # noqa: F401 -- brick_case is a fixture
from test_gpu_mesh import NAMES, assert_same, corner, extract
from test_gpu_tsdf import ORIGIN, PARAMS, TRUNC, VOXEL, integrate, kw, volume_case  # noqa: F401 -- volume_case is a fixture

pytestmark = pytest.mark.gpu

A_DIMS = (21, 18, 17)                    # a 3 x 3 x 3 brick grid whose high faces all overhang
S_DIMS = (48, 48, 32)                    # a dense-size volume around the crafted scene
B_DIMS = (65536, 65536, 32)              # the same origin and voxel: 2^37 voxels, 2^28 bricks


def active_cells(vol, v, min_obs):
    """[nz-1, ny-1, nx-1] bool: the dense volume's active cells."""
    nx, ny, nz = vol.dims
    T, O = v["tsdf"].reshape(nz, ny, nx), v["obs"].reshape(nz, ny, nx)
    allobs = np.logical_and.reduce([corner(O >= min_obs, c) for c in range(8)])
    n_in = sum(corner(T < 0, c).astype(np.int64) for c in range(8))
    return allobs & (n_in > 0) & (n_in < 8)


def key_of(b, B):
    return (b[2] * B[1] + b[1]) * B[0] + b[0]


@pytest.fixture(scope="module")
def arbitrary_bricks(volume_case):
    """A seeded subset of A_DIMS' 27 bricks with seeded values, the overhang voxels included (they must not be read)."""
    P, g = volume_case[0], volume_case[1]
    vol = P.volume((0.25, -1.0, 2.0), 0.125, A_DIMS)
    B = grid_of(vol)
    assert B == [3, 3, 3]
    rng = np.random.default_rng(8128)
    corners = [(i, j, k) for k in (0, 2) for j in (0, 2) for i in (0, 2)]
    lonely = (0, 0, 0)                                             # isolated: none of its 26 neighbours is stored
    # A cell across a shared edge or corner needs all the bricks around it, and (1, 1, 1) is never stored: the
    # edge-only and corner-only pairs pin that nothing spurious appears there, the face pairs that cells do.
    face_pair, edge_pair, corner_pair = ((2, 2, 2), (2, 2, 1)), ((2, 0, 2), (1, 1, 2)), ((2, 0, 1), (1, 1, 2))
    forced = set(corners) | set(face_pair) | set(edge_pair) | set(corner_pair) | {(1, 2, 1), (2, 1, 1)}
    # (the last two: an x and a y neighbour of (2, 2, 1); the z = 2 layer is one voxel thick and holds no cell of its own)
    free = [(i, j, k) for k in range(3) for j in range(3) for i in range(3) if (i, j, k) not in forced and max(i, j, k) == 2]
    chosen = forced | {b for b in free if rng.random() < 0.5}
    for a, b in (face_pair, edge_pair, corner_pair):
        assert a in chosen and b in chosen
    assert sorted(abs(p - q) for p, q in zip(*face_pair)) == [0, 0, 1]
    assert sorted(abs(p - q) for p, q in zip(*edge_pair)) == [0, 1, 1]
    assert sorted(abs(p - q) for p, q in zip(*corner_pair)) == [1, 1, 1]
    assert not any(b != lonely and max(abs(p - q) for p, q in zip(b, lonely)) <= 1 for b in chosen)
    assert 13 <= len(chosen) < 27
    keys = np.array(sorted(key_of(b, B) for b in chosen), np.int64)
    n = len(keys)
    bricks = {"brick": keys, "tsdf": rng.uniform(-1, 1, (n, 8, 8, 8)).astype(np.float32),
              "obs": rng.choice(np.arange(4, dtype=np.uint8), (n, 8, 8, 8), p=(0.02, 0.04, 0.47, 0.47)),
              "color": rng.integers(0, 256, (n, 8, 8, 8, 4)).astype(np.uint8)}
    bricks["color"][..., 3] = np.where(rng.random((n, 8, 8, 8)) < 0.7, 255, 0)
    dense = scatter(vol, bricks)
    want = {m: extract(vol, dense["tsdf"], dense["obs"], dense["color"], m) for m in (1, 2)}
    nx, ny, nz = A_DIMS
    for m in (1, 2):
        w = want[m]
        assert len(w["vertex"]) > 100 and len(w["face"]) > 20
        # faces cross brick boundaries on all three axes: a triangle whose cells lie in different bricks along a
        cells = np.nonzero(active_cells(vol, dense, m).ravel())[0]
        cidx = np.stack([cells % (nx - 1), (cells // (nx - 1)) % (ny - 1), cells // ((nx - 1) * (ny - 1))], -1)
        tri = cidx[w["face"]] >> 3                                 # [nf, 3 cells, 3 axes]: the brick of each cell
        for a in range(3):
            assert (tri[:, :, a].min(1) != tri[:, :, a].max(1)).any(), a
    assert len(want[1]["vertex"]) != len(want[2]["vertex"])
    return P, g, vol, bricks, dense, want


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("min_obs", [1, 2])
def test_brick_mesh_equals_dense_on_arbitrary_bricks(arbitrary_bricks, min_obs, device):
    P, g, vol, bricks, dense, want = arbitrary_bricks
    ins = bricks
    if device:
        ins = {k: torch.as_tensor(v, device=torch.device("cuda", g.device)) for k, v in bricks.items()}
    got = g.brick_tsdf_mesh(vol, ins["brick"], ins["tsdf"], ins["obs"], ins["color"], min_obs=min_obs, device=device)
    if device:
        assert all(t.is_cuda for t in got.values())
    assert_same(got, want[min_obs])
    assert_same(g.tsdf_mesh(vol, dense["tsdf"], dense["obs"], dense["color"], min_obs=min_obs), want[min_obs])
    if min_obs == 1 and not device:   # no colour array: the same mesh with colour 0
        nocol = g.brick_tsdf_mesh(vol, bricks["brick"], bricks["tsdf"], bricks["obs"], None)
        assert_same(nocol, dict(want[1], color=np.zeros_like(want[1]["color"])))


@pytest.fixture(scope="module")
def scene_volume(volume_case, brick_case):
    """Volume S around the crafted scene, its restated dense volume and mesh, and the smallest margin at which
    every corner of every dense-active cell lies in a selected brick."""
    P, g, o, inp, recs = volume_case[:5]
    fus, passing, _ = brick_case[4][PARAMS[0]]
    S = P.volume(ORIGIN, VOXEL, S_DIMS)
    dense = integrate(o, inp, fus, passing, S, TRUNC)[0]
    act = active_cells(S, dense, 1)
    B = grid_of(S)
    k, j, i = np.nonzero(act)
    need = np.zeros((B[2], B[1], B[0]), bool)                       # the bricks of the active cells' corners
    for c in range(8):
        need[(k + (c >> 2)) >> 3, (j + ((c >> 1) & 1)) >> 3, (i + (c & 1)) >> 3] = True
    margin = None
    for m in range(0, 65):
        keys, stats = select(fus.Sf, passing, S, m)
        chosen = np.zeros(B[0] * B[1] * B[2], bool)
        chosen[keys] = True
        if chosen[need.ravel()].all():
            margin = m
            break
    assert margin is not None and margin > 0 and stats["unselected"] > 0      # sparse, and margin 0 opens the surface
    # the stored voxels stay clear of S's high x and y faces: in B the same bricks hold the same voxels
    origin, voxel = [np.float64(np.float32(x)) for x in S.origin], np.float64(np.float32(S.voxel))
    gxy = np.stack([np.floor((fus.Sf[passing][:, a].astype(np.float64) - origin[a]) / voxel) for a in range(2)], 1)
    assert (gxy + margin <= np.array(S_DIMS[:2]) - 2).all()         # no box is clipped or skipped there, in S or in B
    b = [keys % B[0], (keys // B[0]) % B[1]]
    assert all(8 * int(b[a].max()) + 7 < S_DIMS[a] - 1 for a in range(2))
    want = extract(S, dense["tsdf"], dense["obs"], dense["color"], 1)
    assert len(want["vertex"]) > 100 and len(want["face"]) > 100
    return P, g, recs, S, dense, want, margin


def test_brick_mesh_end_to_end_equals_dense(scene_volume):
    P, g, recs, S, dense, want, margin = scene_volume
    full = g.mesh_patches(recs, S, TRUNC, writer_order=True, **kw(PARAMS[0]))
    assert_same(full, want)
    assert_same(g.brick_mesh_patches(recs, S, TRUNC, margin, writer_order=True, **kw(PARAMS[0])), want)
    got = g.brick_mesh_patches(recs, S, TRUNC, margin, writer_order=True, device=True, **kw(PARAMS[0]))
    assert all(t.is_cuda for t in got.values())
    assert_same(got, want)
    # margin 0: the mesh of exactly the stored bricks, which opens boundaries the dense mesh does not have
    bricks = g.brick_tsdf_patches(recs, S, TRUNC, 0, writer_order=True, **kw(PARAMS[0]))
    sparse = scatter(S, bricks)
    opened = g.brick_mesh_patches(recs, S, TRUNC, 0, writer_order=True, **kw(PARAMS[0]))
    assert_same(opened, g.tsdf_mesh(S, sparse["tsdf"], sparse["obs"], sparse["color"]))
    assert_same(opened, extract(S, sparse["tsdf"], sparse["obs"], sparse["color"], 1))
    assert 0 < len(opened["vertex"]) < len(want["vertex"])


def test_brick_mesh_in_a_volume_the_dense_calls_reject(scene_volume):
    """B = S's origin and voxel with dims (65536, 65536, 32): 2^37 voxels, which the dense calls reject, and
    virtual voxel indices from 2^32 at k = 1 on (cell indices past 2^31 at k = 1, past 2^32 at k = 2).  The stored bricks are S's, so the mesh must be
    S's byte for byte.  The brick grid is 8192 x 8192 x 4 = 2^28 bricks: 1.34 GB of scratch (flag 1 and
    slot 4 bytes per grid brick) plus the scan's temporary storage, small beside it, for a few hundred stored bricks."""
    P, g, recs, S, dense, want, margin = scene_volume
    Bv = P.volume(ORIGIN, VOXEL, B_DIMS)
    assert B_DIMS[0] * B_DIMS[1] * B_DIMS[2] > 2 ** 31 - 1
    # voxel indices reach 2^32 at k = 1; cell indices pass 2^31 at k = 1 and 2^32 at k = 2
    assert B_DIMS[0] * B_DIMS[1] >= 2 ** 32 and 2 ** 31 < (B_DIMS[0] - 1) * (B_DIMS[1] - 1) < 2 ** 32 < 2 * (B_DIMS[0] - 1) * (B_DIMS[1] - 1)
    with pytest.raises(P.PmvsError, match="pmvs status 1:"):
        g.mesh_patches(recs, Bv, TRUNC, writer_order=True, **kw(PARAMS[0]))
    got = g.brick_mesh_patches(recs, Bv, TRUNC, margin, writer_order=True, **kw(PARAMS[0]))
    assert_same(got, g.brick_mesh_patches(recs, S, TRUNC, margin, writer_order=True, **kw(PARAMS[0])))
    assert_same(got, g.mesh_patches(recs, S, TRUNC, writer_order=True, **kw(PARAMS[0])))
    assert_same(got, want)


def raw_mesh(P, g, vol, bricks, vcap, fcap, arrays, min_obs=1, flags=0, keys=None):
    """pmvs_brick_tsdf_mesh through ctypes with caller-made arrays; returns (status, nverts, nfaces)."""
    buf = P.MeshBuffers()
    for k, a in arrays.items():
        setattr(buf, k, a.ctypes.data)
    keys = bricks["brick"] if keys is None else keys
    nv, nf = C.c_int64(-1), C.c_int64(-1)
    ptr = [a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data for a in (keys, bricks["tsdf"], bricks["obs"], bricks["color"])]
    st = g.lib.pmvs_brick_tsdf_mesh(g.handle, flags, C.byref(vol), min_obs, len(keys), *ptr, vcap, fcap, C.byref(buf), C.byref(nv),
                                    C.byref(nf))
    return st, int(nv.value), int(nf.value)


def test_brick_mesh_caps_and_counting_call(arbitrary_bricks):
    P, g, vol, bricks, dense, want = arbitrary_bricks
    w = want[1]
    nv, nf = len(w["vertex"]), len(w["face"])
    assert raw_mesh(P, g, vol, bricks, 0, 0, {}) == (0, nv, nf)     # the counting call: every pointer NULL
    vcap, fcap, guard = nv // 3, nf // 5 | 1, 64                   # an odd face cap cuts a quad in two
    assert 0 < vcap < nv and 0 < fcap < nf and fcap % 2 == 1
    shapes = {"vertex": (vcap, np.float32), "normal": (vcap, np.float32), "color": (vcap, np.uint8), "face": (fcap, np.int32)}
    arrays = {k: np.full((cap + guard, 3), 0x5A, dt) for k, (cap, dt) in shapes.items()}
    assert raw_mesh(P, g, vol, bricks, vcap, fcap, arrays) == (0, nv, nf)
    for k, (cap, dt) in shapes.items():
        assert arrays[k][:cap].tobytes() == w[k][:cap].tobytes(), k
        assert (arrays[k][cap:] == np.array(0x5A, dt)).all(), k
    big = {"vertex": np.full((nv + guard, 3), 0x5A, np.float32), "face": np.full((nf + guard, 3), -3, np.int32)}
    assert raw_mesh(P, g, vol, bricks, 2 ** 62, 2 ** 62, big) == (0, nv, nf)
    assert big["vertex"][:nv].tobytes() == w["vertex"].tobytes() and (big["vertex"][nv:] == np.float32(0x5A)).all()
    assert np.array_equal(big["face"][:nf], w["face"]) and (big["face"][nf:] == -3).all()
    # faces alone: the vertex ids without a vertex array
    only = {"face": np.full((nf, 3), -3, np.int32)}
    assert raw_mesh(P, g, vol, bricks, 0, nf, only) == (0, nv, nf) and np.array_equal(only["face"], w["face"])


def test_brick_mesh_degenerate_and_bad_keys(arbitrary_bricks, brick_case):
    P, g, vol, bricks, dense, want = arbitrary_bricks
    recs, bvol = brick_case[2], brick_case[3]
    # no records: no passing pixel, no brick, an empty mesh -- not an error
    none = g.brick_tsdf_patches(recs[:0], bvol, TRUNC, 5, **kw(PARAMS[0]))
    assert none["brick"].shape == (0,) and none["tsdf"].shape == (0, 8, 8, 8)
    m = g.brick_mesh_patches(recs[:0], bvol, TRUNC, 5, **kw(PARAMS[0]))
    assert m["vertex"].shape == (0, 3) and m["face"].shape == (0, 3)
    empty = {k: v[:0] for k, v in bricks.items()}
    assert raw_mesh(P, g, vol, empty, 0, 0, {}) == (0, 0, 0)
    # a dim of 1: no cells
    one = {"brick": np.zeros(1, np.int64), "tsdf": np.where(np.arange(512) % 2 == 0, -0.5, 0.5).astype(np.float32).reshape(1, 8, 8, 8),
           "obs": np.ones((1, 8, 8, 8), np.uint8), "color": np.zeros((1, 8, 8, 8, 4), np.uint8)}
    for dims in ((1, 5, 4), (5, 1, 4), (5, 4, 1), (1, 1, 1)):
        assert raw_mesh(P, g, P.volume((0, 0, 0), 1.0, dims), one, 0, 0, {}) == (0, 0, 0)
    # the same brick in a 5 x 4 x 3 volume: every one of its 4 x 3 x 2 cells, and nothing of the overhang
    got = g.brick_tsdf_mesh(P.volume((0, 0, 0), 1.0, (5, 4, 3)), one["brick"], one["tsdf"], one["obs"])
    d = scatter(P.volume((0, 0, 0), 1.0, (5, 4, 3)), one)
    assert_same(got, extract(P.volume((0, 0, 0), 1.0, (5, 4, 3)), d["tsdf"], d["obs"], None, 1))
    assert len(got["vertex"]) == 4 * 3 * 2
    # keys: strictly ascending and inside the 27-brick grid, in host mode and (checked by a kernel) in device mode
    keys = bricks["brick"]
    swapped, twice, outside, negative = keys.copy(), keys.copy(), keys.copy(), keys.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    twice[5] = twice[4]
    outside[-1] = 27
    negative[0] = -1
    dev = torch.device("cuda", g.device)
    on_dev = {k: torch.as_tensor(v, device=dev) for k, v in bricks.items()}
    assert raw_mesh(P, g, vol, on_dev, 0, 0, {}, flags=P.EXPORT_DEVICE) == (0, len(want[1]["vertex"]), len(want[1]["face"]))
    for bad in (swapped, twice, outside, negative):
        assert raw_mesh(P, g, vol, bricks, 0, 0, {}, keys=bad)[0] == 1
        assert raw_mesh(P, g, vol, on_dev, 0, 0, {}, flags=P.EXPORT_DEVICE, keys=torch.as_tensor(bad, device=dev))[0] == 1
    assert raw_mesh(P, g, vol, bricks, 0, 0, {}, flags=1)[0] == 1   # the writer order means nothing to bricks
    assert raw_mesh(P, g, vol, bricks, 0, 0, {}, min_obs=0)[0] == 1 and raw_mesh(P, g, vol, bricks, -1, 0, {})[0] == 1
