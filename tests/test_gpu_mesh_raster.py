"""pmvs_mesh_raster: a triangle mesh rasterised into the target images, the nearest face and its depth per pixel.
There is no reference for this: the expected arrays are a numpy restatement of the definition in
include/pmvs_amd.h (TEXTURING, part A), built on OracleScene.project / .depth alone, in explicit element-wise
float64 operations in the definition's order.  face and depth are compared for exact equality of dtype, shape and
bytes, in host and device mode, over all targets and over a sub-range; nothing is excluded.  Every call goes
through ctypes with canaries behind the output arrays.  (The restatement of part B, the view selection, is here
too: tests/test_gpu_mesh_texture.py uses it on the same meshes.)

Two meshes:
 (a) the real one: test_gpu_tsdf.py's volume in test_gpu_depth_maps.py's scene (4 targets at 160 x 120, one
     cropped), integrated and meshed by the library (those bytes are pinned by test_gpu_tsdf.py and
     test_gpu_mesh.py), with an occluder quad between the sphere and targets 0 and 1 appended;
 (b) a hand-made one in a scene of ten targets at 64 x 48 (more than the eight one group renders together; the
     projections are pmvs_synth_ring's, target 7 a copy of target 2's so that scores tie; the images are black):
     a face whose clipped box is target 0's whole image and which covers all of it but one corner (so that the
     target keeps empty pixels), a face with A = 0, one with a vertex behind a camera, one half outside the
     image, one with a NaN vertex, one face twice (the tie goes to the lower id), a quad whose diagonal runs
     through pixel centres of target 0 (its end points project to integers exactly), and two faces smaller
     than a pixel that cover no centre (one with an empty box, one with a box of one pixel).
The fixtures assert on the restatement alone that each of these branches occurs."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_depth_maps import crafted_scene
from test_gpu_fuse import RADIUS, surface_records
from test_gpu_pixel_maps import depth_bits, depth_from_bits, image_dims
from test_gpu_tsdf import DIMS, ORIGIN, TRUNC, VOXEL

pytestmark = pytest.mark.gpu

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
THREAD_BOX = 64  # pixels of the largest box one thread walks (pmvs_texmesh.hip): larger boxes take the wavefront form
SUB = (1, 2)
CANARY = 64


def homogeneous(vertex):
    return np.concatenate([np.asarray(vertex, np.float32).reshape(-1, 3), np.ones((len(vertex), 1), np.float32)], axis=1)


class TargetRaster:
    """Part A for one target: the winning key per pixel, and per face what the branch asserts and part B need."""

    def __init__(self, o, inp, W, H, t, vertex, face):
        self.W, self.H, self.t = W, H, t
        nf = len(face)
        c4 = homogeneous(vertex)
        xy, z = o.project(t, inp.level, c4), o.depth(t, c4)
        self.x = np.stack([xy[face[:, k], 0] for k in range(3)], axis=1)  # [nf, 3] float32
        self.y = np.stack([xy[face[:, k], 1] for k in range(3)], axis=1)
        self.z = np.stack([z[face[:, k]] for k in range(3)], axis=1)
        X, Y, Z = self.x.astype(np.float64), self.y.astype(np.float64), self.z.astype(np.float64)
        with np.errstate(all="ignore"):
            corners_ok = (np.isfinite(self.z) & (self.z > 0) & np.isfinite(self.x) & np.isfinite(self.y)).all(axis=1)
            A = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (Y[:, 1] - Y[:, 0]) * (X[:, 2] - X[:, 0])
            self.A = A
            self.drawn = corners_ok & np.isfinite(A) & (A != 0)
            u0 = np.maximum(0.0, np.ceil(X.min(axis=1)))
            u1 = np.minimum(W - 1.0, np.floor(X.max(axis=1)))
            v0 = np.maximum(0.0, np.ceil(Y.min(axis=1)))
            v1 = np.minimum(H - 1.0, np.floor(Y.max(axis=1)))
            self.boxed = self.drawn & (u0 <= u1) & (v0 <= v1)
        idx = np.nonzero(self.boxed)[0]
        bw, bh = (u1[idx] - u0[idx] + 1).astype(np.int64), (v1[idx] - v0[idx] + 1).astype(np.int64)
        cnt = bw * bh
        self.box_pixels = np.zeros(nf, np.int64)
        self.box_pixels[idx] = cnt
        fi = np.repeat(idx, cnt)
        local = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        bwr = np.repeat(bw, cnt)
        u = u0[fi] + (local % bwr).astype(np.float64)
        v = v0[fi] + (local // bwr).astype(np.float64)
        x0, y0, x1, y1, x2, y2 = X[fi, 0], Y[fi, 0], X[fi, 1], Y[fi, 1], X[fi, 2], Y[fi, 2]
        w0 = (x2 - x1) * (v - y1) - (y2 - y1) * (u - x1)
        w1 = (x0 - x2) * (v - y2) - (y0 - y2) * (u - x2)
        w2 = (x1 - x0) * (v - y0) - (y1 - y0) * (u - x0)
        Af = A[fi]
        covered = np.where(Af > 0, (w0 >= 0) & (w1 >= 0) & (w2 >= 0), (w0 <= 0) & (w1 <= 0) & (w2 <= 0))
        with np.errstate(all="ignore"):
            inv = (w0 / Af) / Z[fi, 0] + (w1 / Af) / Z[fi, 1] + (w2 / Af) / Z[fi, 2]
            d = (1.0 / inv).astype(np.float32)
            ok = covered & np.isfinite(d) & (d > 0)
        self.pair_face, self.pair_pix = fi[ok], (v[ok].astype(np.int64) * W + u[ok].astype(np.int64))
        self.pair_key = (depth_bits(d[ok]).astype(np.uint64) << np.uint64(32)) | self.pair_face.astype(np.uint64)
        self.covered = np.bincount(self.pair_face, minlength=nf)
        self.keys = np.full(W * H, EMPTY, np.uint64)
        np.minimum.at(self.keys, self.pair_pix, self.pair_key)


def restate_raster(o, inp, vertex, face, targets):
    """({"face", "depth"} over `targets`, the TargetRaster of each)."""
    dims = image_dims(inp)
    rs = [TargetRaster(o, inp, dims[t][0], dims[t][1], t, vertex, face) for t in targets]
    keys = np.concatenate([r.keys for r in rs])
    filled = keys != EMPTY
    out = {"face": np.where(filled, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32),
           "depth": np.where(filled, depth_from_bits(keys >> np.uint64(32)), np.float32(0)).astype(np.float32)}
    return out, rs


def restate_texture(o, inp, vertex, face, rasters, depth_rel, min_area):
    """Part B over the targets of `rasters` (ascending), from their keys: ({"view", "uv", "score"}, aux)."""
    nf = len(face)
    dr, ma = np.float64(np.float32(depth_rel)), np.float32(min_area)
    V = [vertex[face[:, k]].astype(np.float64) for k in range(3)]  # [nf, 3] each
    a, b = [V[1][:, i] - V[0][:, i] for i in range(3)], [V[2][:, i] - V[0][:, i] for i in range(3)]
    N = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    view, best = np.full(nf, -1, np.int32), np.zeros(nf, np.float32)
    per = []
    for r in rasters:
        centre = o.camera(r.t, inp.level)[0:3].astype(np.float64)
        c = [centre[i] - V[0][:, i] for i in range(3)]
        with np.errstate(all="ignore"):
            front = N[0] * c[0] + N[1] * c[1] + N[2] * c[2] > 0
            visible, through_empty = np.ones(nf, bool), np.zeros(nf, bool)
            for k in range(3):
                px, py = np.floor(r.x[:, k].astype(np.float64) + 0.5), np.floor(r.y[:, k].astype(np.float64) + 0.5)
                inside = (px >= 0) & (px <= r.W - 1.0) & (py >= 0) & (py <= r.H - 1.0)
                q = np.where(inside, np.where(inside, py, 0).astype(np.int64) * r.W + np.where(inside, px, 0).astype(np.int64), 0)
                key = r.keys[q]
                empty = key == EMPTY
                dq = depth_from_bits(key >> np.uint64(32)).astype(np.float64)
                zk = r.z[:, k].astype(np.float64)
                visible &= inside & (empty | (zk - dq <= dr * zk))
                through_empty |= inside & empty
            s = (0.5 * np.abs(r.A)).astype(np.float32)
            large = s >= ma
        eligible = r.drawn & front & visible & large
        take = eligible & ((view < 0) | (s > best))
        view[take], best[take] = r.t, s[take]
        per.append({"t": r.t, "drawn": r.drawn, "front": front, "visible": visible, "large": large, "eligible": eligible, "s": s,
                    "through_empty": through_empty})
    uv = np.zeros((nf, 6), np.float32)
    c4 = homogeneous(vertex)
    for t in np.unique(view[view >= 0]):
        xy = o.project(int(t), 0, c4)
        sel = view == t
        for k in range(3):
            uv[sel, 2 * k], uv[sel, 2 * k + 1] = xy[face[sel, k], 0], xy[face[sel, k], 1]
    return {"view": view, "uv": uv, "score": best}, per


def backproject(o, inp, t, u, v, depth):
    """A point that projects near pixel (u, v) of target t at the scene's level, at that depth (float64 solve)."""
    cam = o.camera(t, inp.level).astype(np.float64)
    oaxis, Pm = cam[4:8], cam[18:30].reshape(3, 4)
    M = np.stack([Pm[0, :3] - u * Pm[2, :3], Pm[1, :3] - v * Pm[2, :3], oaxis[:3]])
    rhs = np.array([-(Pm[0, 3] - u * Pm[2, 3]), -(Pm[1, 3] - v * Pm[2, 3]), depth - oaxis[3]])
    return np.linalg.solve(M, rhs).astype(np.float32)


def exact_pixel_point(o, inp, t, u, v, depth):
    """A float32 point whose f32 projection into target t is exactly the integer pixel (u, v): searched among the
    float32 neighbours of the back-projected point."""
    steps = np.arange(-20, 21)
    grid = np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), axis=-1).reshape(-1, 3)
    for i in range(8):  # a few depths: at some, no neighbour hits both coordinates at once
        p = backproject(o, inp, t, u, v, depth + 0.013 * i)
        cand = (p.view(np.int32)[None, :] + grid.astype(np.int32)).astype(np.int32).view(np.float32)
        xy = o.project(t, inp.level, homogeneous(cand))
        hit = np.nonzero((xy[:, 0] == np.float32(u)) & (xy[:, 1] == np.float32(v)))[0]
        if len(hit):
            return cand[hit[0]]
    raise AssertionError("no float32 point projects to the pixel centre exactly")


def occluder_quad():
    """Two faces 1.5 from the origin towards azimuth -5 degrees, 0.6 wide and high, facing outward: in front of the
    sphere's flank as targets 0 and 1 (azimuth 0 and 15 degrees, radius 4) see it, beside it for targets 2 and 3."""
    az = np.deg2rad(-5.0)
    n, side, up = np.array([np.cos(az), np.sin(az), 0.0]), np.array([-np.sin(az), np.cos(az), 0.0]), np.array([0.0, 0.0, 1.0])
    c = 1.5 * n
    v = np.array([c - 0.3 * side - 0.3 * up, c + 0.3 * side - 0.3 * up, c + 0.3 * side + 0.3 * up, c - 0.3 * side + 0.3 * up], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def with_occluder(vertex, face):
    qv, qf = occluder_quad()
    return (np.concatenate([vertex, qv]).astype(np.float32), np.concatenate([face, qf + len(vertex)]).astype(np.int32))


def hand_scene(P):
    """Ten targets (of twelve views) at 64 x 48: level 1 of black 128 x 96 images, pmvs_synth_ring's projections,
    target 7's a copy of target 2's."""
    p = P.synth_params(12, 128, 96, num_targets=10, level=1)
    _, proj = P.synth_ring(p, render=False)
    proj = proj.copy()
    proj[7] = proj[2]
    return P.SceneInputs(images=[np.zeros((96, 128, 3), np.uint8) for _ in range(12)], projections=proj, num_targets=10, level=1)


def hand_mesh(o, inp):
    """(vertex, face, the face ids by name) of mesh (b), built in target 0's pixel coordinates."""
    V, F, names = [], [], {}

    def add(name, pts, tris):
        base = len(V)
        V.extend(np.asarray(p, np.float32) for p in pts)
        names[name] = list(range(len(F), len(F) + len(tris)))
        F.extend([base + i for i in tri] for tri in tris)

    def bp(u, v, depth, t=0):
        return backproject(o, inp, t, u, v, depth)

    centre, oaxis = o.camera(0, inp.level)[0:3].astype(np.float64), o.camera(0, inp.level)[4:7].astype(np.float64)
    add("big", [bp(-5, -5, 5.0), bp(120, -5, 5.0), bp(-5, 90, 5.0)], [(0, 1, 2)])
    add("zero_area", [bp(20, 30, 4.0), bp(26, 36, 4.0)], [(0, 0, 1)])
    add("behind", [bp(30, 10, 3.5), bp(36, 10, 3.5), (centre - 1.0 * oaxis)], [(0, 1, 2)])
    add("half_outside", [bp(58, 20, 3.8), bp(80, 24, 3.8), bp(60, 30, 3.8)], [(0, 1, 2)])
    add("nan", [bp(40, 40, 4.0), bp(44, 40, 4.0), (np.nan, 0.0, 0.0)], [(0, 1, 2)])
    add("twice", [bp(8, 30, 3.9), bp(18, 31, 4.1), bp(10, 42, 4.0)], [(0, 1, 2), (0, 1, 2)])
    add("quad", [exact_pixel_point(o, inp, 0, 40, 8, 3.7), bp(50, 8, 3.7), exact_pixel_point(o, inp, 0, 50, 18, 3.7), bp(40, 18, 3.7)],
        [(0, 1, 2), (0, 2, 3)])
    add("tiny_no_box", [bp(30.55, 30.6, 3.6), bp(30.95, 30.65, 3.6), bp(30.6, 30.95, 3.6)], [(0, 1, 2)])
    add("tiny_one_pixel", [bp(30.8, 36.7, 3.6), bp(31.3, 36.8, 3.6), bp(31.2, 37.2, 3.6)], [(0, 1, 2)])
    add("small", [bp(22, 12, 3.0), bp(25, 12, 3.0), bp(22, 15, 3.0), bp(25, 15, 3.0)], [(0, 1, 2), (1, 3, 2)])
    # parallel to target 2's image (and so to target 7's, its copy), in both windings: one of them is seen from the front
    add("facing_2", [bp(30, 20, 3.2, 2), bp(37, 20, 3.2, 2), bp(30, 27, 3.2, 2)], [(0, 1, 2), (0, 2, 1)])
    return np.stack(V).astype(np.float32), np.asarray(F, np.int32), names


def check_hand_branches(rs, names):
    """On the restatement alone: every branch mesh (b) was made for occurs."""
    r0 = rs[0]
    f = {k: v[0] for k, v in names.items()}
    assert r0.box_pixels[f["big"]] == 64 * 48 and r0.covered[f["big"]] > THREAD_BOX          # the wavefront form
    assert 0 < r0.covered[f["big"]] < 64 * 48
    assert all(r.A[f["zero_area"]] == 0 and not r.drawn[f["zero_area"]] for r in rs)          # A = 0
    assert not (r0.z[f["behind"]] > 0).all() and not r0.drawn[f["behind"]]                     # behind a camera
    assert any(r.drawn[f["behind"]] for r in rs)
    assert r0.boxed[f["half_outside"]] and r0.x[f["half_outside"]].max() > 63 and r0.covered[f["half_outside"]] > 0
    assert not any(r.drawn[f["nan"]] for r in rs)                                             # a NaN vertex
    a, b = names["twice"]                                                                     # the tie: the lower id wins
    both = np.intersect1d(r0.pair_pix[r0.pair_face == a], r0.pair_pix[r0.pair_face == b])
    assert len(both) > 0 and ((r0.keys[both] & np.uint64(0xFFFFFFFF)) != np.uint64(b)).all()
    assert ((r0.keys[both] & np.uint64(0xFFFFFFFF)) == np.uint64(a)).any()
    a, b = names["quad"]                                                                      # the shared diagonal
    assert r0.x[a, 0] == 40 and r0.y[a, 0] == 8 and r0.x[a, 2] == 50 and r0.y[a, 2] == 18
    shared = np.intersect1d(r0.pair_pix[r0.pair_face == a], r0.pair_pix[r0.pair_face == b])
    assert len(shared) >= 9   # (41, 9) .. (49, 17) at least: covered from both sides
    assert r0.drawn[f["tiny_no_box"]] and not r0.boxed[f["tiny_no_box"]]                     # below a pixel: no box
    assert r0.boxed[f["tiny_one_pixel"]] and r0.box_pixels[f["tiny_one_pixel"]] == 1 and r0.covered[f["tiny_one_pixel"]] == 0
    assert 0 < r0.box_pixels[f["small"]] <= THREAD_BOX and r0.covered[f["small"]] > 0        # the thread form
    for r in rs:                                                                              # filled and empty everywhere
        assert (r.keys != EMPTY).any() and (r.keys == EMPTY).any(), r.t


def raster_call(P, g, vertex, face, first, num, device, names=("face", "depth")):
    """pmvs_mesh_raster through ctypes into arrays with CANARY extra elements; the canaries are checked here."""
    pixels = int(g.pixel_map_layout(first, num)[1][-1])
    dt = {"face": (np.int32, torch.int32, -77), "depth": (np.float32, torch.float32, -77.0)}
    buf, arrays = P.RasterBuffers(), {}
    if device:
        dev = torch.device("cuda", g.device)
        v, f = torch.as_tensor(vertex, device=dev).contiguous(), torch.as_tensor(face, device=dev).contiguous()
        ptrs = (v.data_ptr() if v.numel() else None, f.data_ptr() if f.numel() else None)
        for k in names:
            arrays[k] = torch.full((pixels + CANARY,), dt[k][2], dtype=dt[k][1], device=dev)
            setattr(buf, k, arrays[k].data_ptr())
    else:
        v, f = np.ascontiguousarray(vertex, np.float32), np.ascontiguousarray(face, np.int32)
        ptrs = (v.ctypes.data if v.size else None, f.ctypes.data if f.size else None)
        for k in names:
            arrays[k] = np.full(pixels + CANARY, dt[k][2], dt[k][0])
            setattr(buf, k, arrays[k].ctypes.data)
    st = g.lib.pmvs_mesh_raster(g.handle, P.EXPORT_DEVICE if device else 0, first, num, len(vertex), ptrs[0], len(face), ptrs[1],
                                C.byref(buf))
    assert st == 0, g.lib.pmvs_last_error()
    out = {}
    for k in names:
        a = arrays[k].cpu().numpy() if device else arrays[k]
        assert (a[pixels:] == dt[k][2]).all(), k
        out[k] = a[:pixels]
    return out


def assert_same(got, want, names=("face", "depth"), sl=slice(None)):
    assert set(got) == set(names)
    for k in names:
        a = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        w = want[k][sl]
        assert a.dtype == w.dtype and a.shape == w.shape, k
        assert a.tobytes() == w.tobytes(), k


def real_mesh(P, g):
    """Mesh (a): test_gpu_tsdf.py's volume of test_gpu_fuse.py's records, integrated and meshed by the library, plus
    the occluder quad."""
    vol = P.volume(ORIGIN, VOXEL, DIMS)
    t = g.tsdf_patches(surface_records(P), vol, TRUNC, writer_order=True, radius=RADIUS, depth_rel=0.01, normal_cos=0.5,
                       min_support=2)
    m = g.tsdf_mesh(vol, t["tsdf"], t["obs"], t["color"])
    assert len(m["face"]) > 400
    return with_occluder(m["vertex"], m["face"])


@pytest.fixture(scope="module")
def real_case(gpu_available, oracle_mod):
    import pmvs_amd as P
    inp = crafted_scene(P)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    vertex, face = real_mesh(P, g)
    want, rs = restate_raster(o, inp, vertex, face, range(4))
    sub, _ = restate_raster(o, inp, vertex, face, SUB)
    assert image_dims(inp) == [(160, 120), (150, 100), (160, 120), (160, 120)]
    for r in rs:
        assert (r.keys != EMPTY).any() and (r.keys == EMPTY).any()
        assert (r.box_pixels > THREAD_BOX).any() and ((r.box_pixels > 0) & (r.box_pixels <= THREAD_BOX)).any()  # both forms
        assert (r.boxed & (r.covered == 0)).any()          # a face between the pixel centres
    off = np.concatenate([[0], np.cumsum([r.W * r.H for r in rs])])
    assert want["face"][off[1]:off[3]].tobytes() == sub["face"].tobytes()  # a range is a slice: no target sees another
    yield P, g, o, inp, vertex, face, want, sub, rs
    g.close()
    o.close()


@pytest.fixture(scope="module")
def hand_case(gpu_available, oracle_mod):
    import pmvs_amd as P
    inp = hand_scene(P)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    vertex, face, names = hand_mesh(o, inp)
    want, rs = restate_raster(o, inp, vertex, face, range(10))
    assert image_dims(inp) == [(64, 48)] * 10
    check_hand_branches(rs, names)
    yield P, g, o, inp, vertex, face, names, want, rs
    g.close()
    o.close()


@pytest.mark.parametrize("device", [False, True])
def test_raster_real_mesh(real_case, device):
    P, g, o, inp, vertex, face, want, sub, rs = real_case
    assert_same(raster_call(P, g, vertex, face, 0, 4, device), want)
    assert_same(raster_call(P, g, vertex, face, SUB[0], len(SUB), device), sub)


@pytest.mark.parametrize("device", [False, True])
def test_raster_hand_mesh(hand_case, device):
    """Ten targets: two groups, the second of two targets."""
    P, g, o, inp, vertex, face, names, want, rs = hand_case
    assert_same(raster_call(P, g, vertex, face, 0, 10, device), want)
    off = 64 * 48
    assert_same(raster_call(P, g, vertex, face, 7, 3, device), want, sl=slice(7 * off, 10 * off))


def test_raster_python_mirror_and_selected_arrays(hand_case):
    """Scene.mesh_raster: numpy in host mode, torch tensors (also as inputs) in device mode; a NULL array is
    skipped and the other does not change; no face gives empty maps."""
    P, g, o, inp, vertex, face, names, want, rs = hand_case
    assert_same(g.mesh_raster(vertex, face), want)
    dev = torch.device("cuda", g.device)
    got = g.mesh_raster(torch.as_tensor(vertex, device=dev), torch.as_tensor(face, device=dev), device=True)
    assert all(t.is_cuda and t.device.index == g.device for t in got.values())
    assert_same(got, want)
    assert_same(g.mesh_raster(vertex, face, arrays=("depth",), first_target=3, num_targets=1), want, ("depth",),
                slice(3 * 64 * 48, 4 * 64 * 48))
    assert_same(raster_call(P, g, vertex, face, 0, 10, True, names=("face",)), want, ("face",))
    for device in (False, True):
        empty = raster_call(P, g, vertex, face[:0], 0, 10, device)
        assert (empty["face"] == -1).all() and not empty["depth"].view(np.uint32).any()


def test_raster_errors(hand_case):
    """The rejection list with a real scene: the argument itself is what is rejected."""
    P, g, o, inp, vertex, face, names, want, rs = hand_case
    lib, buf = g.lib, P.RasterBuffers()
    nv, nf = len(vertex), len(face)

    def call(flags=0, first=0, num=10, nv=nv, v=vertex.ctypes.data, nf=nf, f=face.ctypes.data, b=buf, scene=g.handle):
        return lib.pmvs_mesh_raster(scene, flags, first, num, nv, v, nf, f, None if b is None else C.byref(b))

    assert call() == 0
    assert call(scene=None) == 1 and call(b=None) == 1
    for flags in (1, 4, 2 | 8, -1):
        assert call(flags=flags) == 1
    for first, num in ((-1, 1), (0, 0), (9, 2), (10, 1), (0, 11)):
        assert call(first=first, num=num) == 1
    assert call(nv=-1) == 1 and call(nf=-1) == 1 and call(nv=1 << 31) == 1 and call(nf=1 << 31) == 1
    assert call(v=None) == 1 and call(f=None) == 1
    assert call(nv=0, v=None, nf=0, f=None) == 0
    for bad in (nv, -1, 1 << 30):
        f = face.copy()
        f[len(f) // 2, 1] = bad
        assert call(f=f.ctypes.data) == 1 and b"vertex id" in lib.pmvs_last_error()
        dev = torch.device("cuda", g.device)
        dv, df = torch.as_tensor(vertex, device=dev), torch.as_tensor(f, device=dev)
        out = torch.full((10 * 64 * 48,), -77, dtype=torch.int32, device=dev)
        b = P.RasterBuffers(face=out.data_ptr())
        assert call(flags=P.EXPORT_DEVICE, v=dv.data_ptr(), f=df.data_ptr(), b=b) == 1 and b"vertex id" in lib.pmvs_last_error()
        assert (out == -77).all()   # rejected before anything was written
    assert call(nv=nv - 1) == 1     # the last vertex is used: now outside
