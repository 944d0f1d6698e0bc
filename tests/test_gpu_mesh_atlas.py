"""pmvs_mesh_atlas: the textured mesh baked into one atlas image.  There is no reference for this: the expected layout,
rgb, texel_face, uv and atlas_view are a numpy restatement of the definition in include/pmvs_amd.h (THE ATLAS, steps
1-7), built on OracleScene.project(view, 0, ...) and OracleScene.get_color(view, 0, ...) alone, in explicit
element-wise float64 operations in the definition's order (the texel map and the bands are tests/test_atlas_host.py's
and tests/test_atlas_abi.py's restatements).  Every output is compared for exact equality of dtype, shape and bytes, in
host and device mode, through ctypes with canaries behind every array; a height_cap below H, the sizing call and NULL
subsets of the buffers are covered.

Two scenes:
 (a) tests/test_gpu_mesh_raster.py's real mesh with the views pmvs_mesh_texture gives it;
 (b) a scene of its own in the shape of that file's hand_scene (ten targets of twelve views, 128 x 96 images at level
     1, so level 0 is not the scene's level) whose images are seeded noise -- black images would hide every sampling
     error -- with a hand-made mesh and a hand-made view array, baked into tiny atlases (W 48 and 61, max_side 8,
     scale 1 and 0.37).
The fixture asserts on the restatement alone that every branch the mesh was made for occurs."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_atlas_abi import restate_layout
from test_atlas_host import restate_corners, restate_texels
from test_gpu_mesh_raster import CANARY, backproject, homogeneous, real_case  # noqa: F401 -- real_case is a fixture

pytestmark = pytest.mark.gpu

NAMES = ("rgb", "texel_face", "uv", "atlas_view")
DT = {"rgb": (np.uint8, torch.uint8, 201), "texel_face": (np.int32, torch.int32, -77), "uv": (np.float32, torch.float32, -77.0),
      "atlas_view": (np.int32, torch.int32, -77)}
HAND_CONFIGS = ((48, 8, 1.0), (61, 8, 0.37))   # W, max_side, scale
REAL_CONFIG = (250, 16, 1.0)
LEVEL0 = SimpleNamespace(level=0)


def restate_atlas(o, inp, vertex, face, view, W, M, scale):
    """Steps 1-7: {"rgb", "texel_face", "uv", "atlas_view"}, the layout and what the branch asserts need."""
    nf = len(face)
    c4 = homogeneous(vertex)
    ic = np.zeros((nf, 3, 3), np.float32)
    for t in np.unique(view[view >= 0]):
        xyw = o.project(int(t), 0, c4)
        ic[view == t] = xyw[face[view == t]]
    with np.errstate(all="ignore"):
        placed = (view >= 0) & (ic[:, :, 2] > 0).all(axis=1) & np.isfinite(ic[:, :, :2]).all(axis=(1, 2))
        X, Y = ic[:, :, 0].astype(np.float64), ic[:, :, 1].astype(np.float64)
        e = np.zeros(nf, np.float64)
        for a, b in ((0, 1), (1, 2), (2, 0)):
            e = np.maximum(e, np.maximum(np.abs(X[:, a] - X[:, b]), np.abs(Y[:, a] - Y[:, b])))
        s = np.float64(np.float32(scale)) * e
        side = np.where(s <= 1.0, 1.0, np.where(s >= M, float(M), np.ceil(s)))
    cls = np.where(placed, side, 0).astype(np.int64)
    counts = np.bincount(cls, minlength=M + 1)
    H, band_y, nplaced, cells = restate_layout(counts, W, M)
    order = np.argsort(cls, kind="stable")               # (class, face id)
    base = np.cumsum(counts) - counts
    rank = np.empty(nf, np.int64)
    rank[order] = np.arange(nf) - base[cls[order]]
    uv, atlas_view = np.zeros((nf, 6), np.float32), np.where(placed, 0, -1).astype(np.int32)
    for n in range(1, M + 1):
        sel = cls == n
        if sel.any():
            uv[sel] = restate_corners(W, n, band_y[n], rank[sel]).reshape(-1, 6).astype(np.float32)
    texel_face = np.full((H, W), -1, np.int32)
    rgb = np.zeros((H, W, 3), np.uint8)
    aux = {"x": np.full((H, W), np.nan), "y": np.full((H, W), np.nan), "sampled": np.zeros((H, W), bool),
           "behind": np.zeros((H, W), bool), "cls": cls, "counts": counts, "band_y": band_y, "rank": rank, "ic": ic}
    for n in range(M, 0, -1):
        if counts[n] == 0:
            continue
        rows = -(-((counts[n] + 1) >> 1) // (W // (n + 5))) * (n + 5)
        J, I = np.meshgrid(np.arange(rows), np.arange(W), indexing="ij")
        ok, r, half, l1, l2 = restate_texels(W, n, int(counts[n]), I, J)
        f = order[base[n] + r[ok]]
        l1, l2 = l1[ok], l2[ok]
        l0 = 1.0 - l1 - l2
        V = [vertex[face[f, k]].astype(np.float64) for k in range(3)]
        Xp = np.stack([(l0 * V[0][:, a] + l1 * V[1][:, a] + l2 * V[2][:, a]).astype(np.float32) for a in range(3)], axis=1)
        col = np.zeros((len(f), 3), np.uint8)
        px, py, sampled, behind = np.full(len(f), np.nan), np.full(len(f), np.nan), np.zeros(len(f), bool), np.zeros(len(f), bool)
        for t in np.unique(view[f]):
            sel = np.nonzero(view[f] == t)[0]
            xyw = o.project(int(t), 0, homogeneous(Xp[sel]))
            x, y, w = xyw[:, 0], xyw[:, 1], xyw[:, 2]
            with np.errstate(all="ignore"):
                good = (w > 0) & np.isfinite(x) & np.isfinite(y)
            behind[sel] = ~(w > 0)
            H0, W0 = inp.images[int(t)].shape[:2]
            hx, hy = np.float32(W0 - 2), np.float32(H0 - 2)
            xd, yd = x.astype(np.float64), y.astype(np.float64)
            xs = np.where(xd < 0.0, np.float32(0), np.where(xd > np.float64(hx), hx, x)).astype(np.float32)
            ys = np.where(yd < 0.0, np.float32(0), np.where(yd > np.float64(hy), hy, y)).astype(np.float32)
            g = np.nonzero(good)[0]
            c = o.get_color(int(t), 0, np.stack([xs[g], ys[g]], axis=1))
            q = np.floor((c + np.float32(0.5)).astype(np.float64))
            col[sel[g]] = np.minimum(q, 255.0).astype(np.uint8)
            px[sel[g]], py[sel[g]], sampled[sel[g]] = xd[g], yd[g], True
        y0 = band_y[n]
        texel_face[y0:y0 + rows][ok] = f
        rgb[y0:y0 + rows][ok] = col
        for k, v in (("x", px), ("y", py), ("sampled", sampled), ("behind", behind)):
            aux[k][y0:y0 + rows][ok] = v
    layout = {"width": W, "height": H, "placed": nplaced, "cells": cells}
    return {"rgb": rgb, "texel_face": texel_face, "uv": uv, "atlas_view": atlas_view}, layout, aux


def noise_scene(P):
    """test_gpu_mesh_raster.py's hand_scene with seeded noise in the place of the black images."""
    p = P.synth_params(12, 128, 96, num_targets=10, level=1)
    _, proj = P.synth_ring(p, render=False)
    rng = np.random.default_rng(4242)
    return P.SceneInputs(images=[rng.integers(0, 256, (96, 128, 3)).astype(np.uint8) for _ in range(12)], projections=proj.copy(),
                         num_targets=10, level=1)


def hand_mesh(o):
    """(vertex, face, view, the face ids by name) of mesh (b), built in the targets' LEVEL-0 pixel coordinates."""
    V, F, VW, names = [], [], [], {}

    def add(name, t, pts, view=None):
        names.setdefault(name, []).append(len(F))
        F.append([len(V) + i for i in range(3)])
        V.extend(np.asarray(p, np.float32) for p in pts)
        VW.append(t if view is None else view)

    def bp(t, u, v, depth):
        return backproject(o, LEVEL0, t, u, v, depth)

    rng = np.random.default_rng(99)
    # right triangles of a given longest extent e (level-0 pixels) somewhere inside target t's 128 x 96 image
    for i, e in enumerate([0.6, 0.9, 2.4, 2.6, 2.2, 4.3, 4.8, 4.1, 4.6, 4.4] + [9.0, 12.0, 30.0, 8.5, 9.5, 10.0, 11.0, 20.0, 15.0]):
        t = i % 4
        u, v = rng.uniform(10, 128 - 40), rng.uniform(10, 96 - 40)
        add("plain", t, [bp(t, u, v, 3.6), bp(t, u + e, v + 0.3 * e, 3.7), bp(t, u + 0.2 * e, v + 0.9 * e, 3.5)])
    add("no_view", 0, [bp(0, 50, 50, 3.6), bp(0, 55, 50, 3.6), bp(0, 50, 55, 3.6)], view=-1)
    cam = o.camera(5, 0)
    centre, oaxis = cam[0:3].astype(np.float64), cam[4:7].astype(np.float64)
    add("behind", 5, [bp(5, 30, 30, 3.5), bp(5, 36, 30, 3.5), centre - 1.0 * oaxis])
    # across each border of target 2's image: samples left of 0, right of W0 - 2, above 0, below H0 - 2
    add("border", 2, [bp(2, -3.0, 40, 3.6), bp(2, 2.5, 41, 3.6), bp(2, -2.0, 45, 3.6)])
    add("border", 2, [bp(2, 124.5, 40, 3.6), bp(2, 130.0, 41, 3.6), bp(2, 125.0, 45, 3.6)])
    add("border", 2, [bp(2, 60, -3.0, 3.6), bp(2, 65, 2.0, 3.6), bp(2, 61, 2.5, 3.6)])
    add("border", 2, [bp(2, 60, 92.5, 3.6), bp(2, 65, 98.0, 3.6), bp(2, 61, 97.5, 3.6)])
    # an edge along target 0's viewing ray: less than a pixel long in the image, and the plane's extrapolation by a
    # gutter texel passes behind the camera
    add("along_ray", 0, [bp(0, 60, 40, 3.0), bp(0, 60, 40, 1.2), bp(0, 60.5, 40.3, 3.0)])
    add("nan", 1, [bp(1, 40, 40, 3.6), bp(1, 44, 40, 3.6), (np.nan, 0.0, 0.0)])
    return np.stack(V).astype(np.float32), np.asarray(F, np.int32), np.asarray(VW, np.int32), names


def check_hand_branches(want, layout, aux, vertex, face, view, names, W, M):
    """On the restatement alone; returns the branches this configuration shows."""
    cls, counts, tf, rgb = aux["cls"], aux["counts"], want["texel_face"], want["rgb"]
    H = layout["height"]
    populated = np.nonzero(counts[1:])[0] + 1
    gaps = [n for n in range(populated.min(), populated.max()) if counts[n] == 0]
    b = {}
    b["three_classes_with_gap"] = len(populated) >= 3 and len(gaps) > 0
    b["odd_class"] = any(counts[n] % 2 == 1 for n in populated)
    b["wrapped_partial"] = any(((counts[n] + 1) >> 1) > W // (n + 5) and ((counts[n] + 1) >> 1) % (W // (n + 5)) != 0 for n in populated)
    margins = [tf[aux["band_y"][n]:aux["band_y"][n] + n + 5, W // (n + 5) * (n + 5):] for n in populated if W % (n + 5)]
    b["right_margin"] = len(margins) > 0 and all(m.size > 0 and (m == -1).all() for m in margins)
    b["clamped_to_1"] = bool((cls[names["plain"][:2]] == 1).all())
    b["clamped_to_max"] = bool((cls[names["plain"][-3:]] == M).all())
    assert view[names["no_view"][0]] == -1 and cls[names["no_view"][0]] == 0
    f = names["behind"][0]
    assert view[f] >= 0 and cls[f] == 0 and not (aux["ic"][f, :, 2] > 0).all()             # not placed: behind its camera
    assert cls[names["nan"][0]] == 0
    sm = aux["sampled"]
    t2 = np.isin(tf, names["border"])
    b["left"], b["right"] = bool((sm & t2 & (aux["x"] < 0)).any()), bool((sm & t2 & (aux["x"] > 126)).any())
    b["top"], b["bottom"] = bool((sm & t2 & (aux["y"] < 0)).any()), bool((sm & t2 & (aux["y"] > 94)).any())
    ar = tf == names["along_ray"][0]
    b["gutter_behind"] = bool((ar & aux["behind"]).any())
    assert not rgb[(tf >= 0) & aux["behind"]].any()                                        # colour 0, the face set
    assert rgb[sm].any() and (tf >= 0).sum() == sm.sum() + ((tf >= 0) & ~sm).sum()
    # two faces with different views in one cell
    mixed = False
    for n in populated:
        fs = np.nonzero(cls == n)[0]
        r = aux["rank"][fs]
        byrank = fs[np.argsort(r)]
        pairs = byrank[:len(byrank) // 2 * 2].reshape(-1, 2)
        mixed |= bool((view[pairs[:, 0]] != view[pairs[:, 1]]).any())
    b["mixed_cell"] = mixed
    assert 40 <= W <= 64 and H > 0 and layout["placed"] == (cls > 0).sum()
    return b


def atlas_call(P, g, vertex, face, view, cfg, cap, device, names=NAMES, alloc_rows=None, expect=0):
    """pmvs_mesh_atlas through ctypes into arrays of alloc_rows (default cap) rows with CANARY extra elements; returns
    (arrays as numpy cut to their size, layout, the raw arrays for the canary checks)."""
    W, M, scale = cfg
    nf = len(face)
    rows = cap if alloc_rows is None else alloc_rows
    size = {"rgb": rows * W * 3, "texel_face": rows * W, "uv": nf * 6, "atlas_view": nf}
    buf, arrays = P.AtlasBuffers(), {}
    if device:
        dev = torch.device("cuda", g.device)
        ins = [torch.as_tensor(a, device=dev).contiguous() for a in (vertex, face, view)]
        ptrs = [a.data_ptr() for a in ins]
        for k in names:
            arrays[k] = torch.full((size[k] + CANARY,), DT[k][2], dtype=DT[k][1], device=dev)
            setattr(buf, k, arrays[k].data_ptr())
    else:
        ins = [np.ascontiguousarray(vertex, np.float32), np.ascontiguousarray(face, np.int32), np.ascontiguousarray(view, np.int32)]
        ptrs = [a.ctypes.data for a in ins]
        for k in names:
            arrays[k] = np.full(size[k] + CANARY, DT[k][2], DT[k][0])
            setattr(buf, k, arrays[k].ctypes.data)
    prm, layout = P.AtlasParams(W, M, scale), P.AtlasLayout(-7, -7, -7, -7)
    st = g.lib.pmvs_mesh_atlas(g.handle, P.EXPORT_DEVICE if device else 0, C.byref(prm), len(vertex), ptrs[0], nf, ptrs[1], ptrs[2],
                               cap, C.byref(buf), C.byref(layout))
    assert st == expect, g.lib.pmvs_last_error()
    raw = {k: (arrays[k].cpu().numpy() if device else arrays[k]) for k in names}
    for k in names:
        assert (raw[k][size[k]:] == DT[k][2]).all(), k
    return {k: raw[k][:size[k]] for k in names}, layout.as_dict(), raw


def assert_same(got, want, rows, W, names=NAMES):
    shapes = {"rgb": (rows, W, 3), "texel_face": (rows, W), "uv": want["uv"].shape, "atlas_view": want["atlas_view"].shape}
    for k in names:
        w = want[k][:rows] if k in ("rgb", "texel_face") else want[k]
        a = got[k].reshape(shapes[k])
        assert a.dtype == w.dtype and a.shape == w.shape, k
        assert a.tobytes() == w.tobytes(), k


@pytest.fixture(scope="module")
def hand_atlas(gpu_available, oracle_mod):
    import pmvs_amd as P
    inp = noise_scene(P)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    vertex, face, view, names = hand_mesh(o)
    wants, seen = {}, {}
    for cfg in HAND_CONFIGS:
        want, layout, aux = restate_atlas(o, inp, vertex, face, view, *cfg)
        wants[cfg] = (want, layout)
        for k, v in check_hand_branches(want, layout, aux, vertex, face, view, names, cfg[0], cfg[1]).items():
            seen[k] = seen.get(k, False) or v
    assert all(seen.values()), seen
    assert wants[HAND_CONFIGS[0]][1] != wants[HAND_CONFIGS[1]][1]      # the scale and the width decide
    yield P, g, o, inp, vertex, face, view, names, wants
    g.close()
    o.close()


@pytest.fixture(scope="module")
def real_atlas(real_case):
    P, g, o, inp, vertex, face, _, _, _ = real_case
    view = g.mesh_texture(vertex, face, arrays=("view",))["view"]
    want, layout, aux = restate_atlas(o, inp, vertex, face, view, *REAL_CONFIG)
    assert set(np.unique(view)) == {-1, 0, 1, 2, 3} and layout["placed"] > 100 and layout["height"] > 2 * (REAL_CONFIG[1] + 5)
    assert len(np.nonzero(aux["counts"][1:])[0]) >= 3 and want["rgb"].any()
    return P, g, vertex, face, view, want, layout


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("cfg", HAND_CONFIGS)
def test_atlas_hand_mesh(hand_atlas, cfg, device):
    P, g, o, inp, vertex, face, view, names, wants = hand_atlas
    want, layout = wants[cfg]
    H, W = layout["height"], cfg[0]
    got, lay, _ = atlas_call(P, g, vertex, face, view, cfg, H, device)
    assert lay == layout
    assert_same(got, want, H, W)
    # a cap past H writes H rows and nothing past them
    got, lay, raw = atlas_call(P, g, vertex, face, view, cfg, H + 5, device)
    assert lay == layout
    assert_same({k: (v[:H * W * 3] if k == "rgb" else v[:H * W] if k == "texel_face" else v) for k, v in got.items()}, want, H, W)
    assert (raw["rgb"][H * W * 3:] == DT["rgb"][2]).all() and (raw["texel_face"][H * W:] == DT["texel_face"][2]).all()
    # a cap below H: only those rows, the rest of an H-row array keeps the canary value
    cap = H // 2 + 1
    got, lay, raw = atlas_call(P, g, vertex, face, view, cfg, cap, device, alloc_rows=H)
    assert lay == layout
    assert_same({k: (v[:cap * W * 3] if k == "rgb" else v[:cap * W] if k == "texel_face" else v) for k, v in got.items()}, want, cap, W)
    assert (raw["rgb"][cap * W * 3:] == DT["rgb"][2]).all() and (raw["texel_face"][cap * W:] == DT["texel_face"][2]).all()


@pytest.mark.parametrize("device", [False, True])
def test_atlas_real_mesh(real_atlas, device):
    P, g, vertex, face, view, want, layout = real_atlas
    H, W = layout["height"], REAL_CONFIG[0]
    got, lay, _ = atlas_call(P, g, vertex, face, view, REAL_CONFIG, H, device)
    assert lay == layout
    assert_same(got, want, H, W)


@pytest.mark.parametrize("device", [False, True])
def test_atlas_sizing_call_and_null_subsets(hand_atlas, device):
    P, g, o, inp, vertex, face, view, names, wants = hand_atlas
    cfg = HAND_CONFIGS[0]
    want, layout = wants[cfg]
    H, W = layout["height"], cfg[0]
    # the sizing call: no buffers at all, and buffers of NULL pointers
    prm, lay = P.AtlasParams(*cfg), P.AtlasLayout()
    if device:
        dev = torch.device("cuda", g.device)
        ins = [torch.as_tensor(a, device=dev).contiguous() for a in (vertex, face, view)]
        ptrs = [a.data_ptr() for a in ins]
    else:
        ptrs = [a.ctypes.data for a in (vertex, face, view)]
    flags = P.EXPORT_DEVICE if device else 0
    for b in (None, C.byref(P.AtlasBuffers())):
        lay = P.AtlasLayout()
        assert g.lib.pmvs_mesh_atlas(g.handle, flags, C.byref(prm), len(vertex), ptrs[0], len(face), ptrs[1], ptrs[2], 0, b, C.byref(lay)) == 0
        assert lay.as_dict() == layout
    got, lay, _ = atlas_call(P, g, vertex, face, view, cfg, 0, device)   # cap 0 with arrays: the per-face ones are written
    assert lay == layout
    assert_same(got, want, 0, W, ("uv", "atlas_view"))
    for sub in (("rgb",), ("texel_face",), ("uv",), ("atlas_view",), ("rgb", "uv"), ("texel_face", "atlas_view")):
        got, lay, _ = atlas_call(P, g, vertex, face, view, cfg, H, device, names=sub)
        assert lay == layout
        assert_same(got, want, H, W, sub)
    # no face: an empty atlas, nothing written
    got, lay, _ = atlas_call(P, g, vertex, face[:0], view[:0], cfg, 4, device, alloc_rows=0)
    assert lay == {"width": W, "height": 0, "placed": 0, "cells": 0}
    # every view -1: the same, and the per-face arrays say so
    got, lay, _ = atlas_call(P, g, vertex, face, np.full_like(view, -1), cfg, 4, device, alloc_rows=0)
    assert lay == {"width": W, "height": 0, "placed": 0, "cells": 0}
    assert (got["atlas_view"] == -1).all() and not got["uv"].any()


def test_atlas_properties(hand_atlas, real_atlas):
    """Without the restatement: every placed face's corners lie inside the atlas, the texel at their rounded centroid is
    the face's, and no texel of a cell names a face of another cell."""
    P, g, o, inp, vertex, face, view, names, wants = hand_atlas
    _, rg, rvertex, rface, rview, _, _ = real_atlas
    for scene, v, f, vw, cfg in ((g, vertex, face, view, HAND_CONFIGS[0]), (g, vertex, face, view, HAND_CONFIGS[1]),
                                 (rg, rvertex, rface, rview, REAL_CONFIG)):
        out, layout = scene.mesh_atlas(v, f, vw, *cfg)
        W, H = layout["width"], layout["height"]
        uv, av, tf = out["uv"].reshape(-1, 3, 2), out["atlas_view"], out["texel_face"]
        placed = np.nonzero(av == 0)[0]
        assert len(placed) == layout["placed"] > 0 and set(np.unique(av)) <= {0, -1} and not uv[av < 0].any()
        x, y = uv[placed, :, 0], uv[placed, :, 1]
        assert (x >= 0).all() and (x < W).all() and (y >= 0).all() and (y < H).all()
        cx, cy = np.floor(x.mean(axis=1) + 0.5).astype(int), np.floor(y.mean(axis=1) + 0.5).astype(int)
        assert np.array_equal(tf[cy, cx], placed)
        # the face's cell from its corners: side n = |x1 - x0|, half 0 iff x1 > x0
        n = np.abs(x[:, 1] - x[:, 0]).astype(int)
        c = n + 5
        half0 = x[:, 1] > x[:, 0]
        ox = np.where(half0, x[:, 0] - 1, x[:, 0] - (c - 2)).astype(int)
        oy = np.where(half0, y[:, 0] - 1, y[:, 0] - (c - 2)).astype(int)
        owners = {}
        for i, fid in enumerate(placed):
            owners.setdefault((ox[i], oy[i], c[i]), []).append(fid)
        assert len(owners) == layout["cells"] and max(len(v) for v in owners.values()) <= 2
        covered = np.zeros((H, W), bool)
        for (x0, y0, cc), ids in owners.items():
            box = tf[y0:y0 + cc, x0:x0 + cc]
            assert box.shape == (cc, cc) and np.isin(box, ids + [-1]).all() and all((box == i).any() for i in ids)
            covered[y0:y0 + cc, x0:x0 + cc] = True
        assert (tf[~covered] == -1).all()


def test_atlas_python_mirror(hand_atlas):
    P, g, o, inp, vertex, face, view, names, wants = hand_atlas
    cfg = HAND_CONFIGS[1]
    want, layout = wants[cfg]
    H, W = layout["height"], cfg[0]
    out, lay = g.mesh_atlas(vertex, face, view, *cfg)
    assert lay == layout
    assert_same(out, want, H, W)
    dev = torch.device("cuda", g.device)
    out, lay = g.mesh_atlas(torch.as_tensor(vertex, device=dev), torch.as_tensor(face, device=dev), torch.as_tensor(view, device=dev),
                            *cfg, device=True)
    assert lay == layout and all(t.is_cuda and t.device.index == g.device for t in out.values())
    assert_same({k: t.cpu().numpy() for k, t in out.items()}, want, H, W)
    out, lay = g.mesh_atlas(vertex, face, view, *cfg, arrays=("rgb",), height_cap=3)
    assert out["rgb"].shape == (3, W, 3) and out["rgb"].tobytes() == want["rgb"][:3].tobytes()


def test_atlas_errors(hand_atlas):
    """The rejection list with a real scene: the argument itself is what is rejected, and nothing is written.  A view
    of num_targets and a face id of nv in DEVICE arrays are invalid inputs the check kernel catches before anything
    is used as an index."""
    P, g, o, inp, vertex, face, view, names, wants = hand_atlas
    lib, nv, nf = g.lib, len(vertex), len(face)
    cfg = HAND_CONFIGS[0]
    H, W = wants[cfg][1]["height"], cfg[0]
    rgb = np.full(H * W * 3, 201, np.uint8)
    av = np.full(nf, -77, np.int32)
    buf, good = P.AtlasBuffers(rgb=rgb.ctypes.data, atlas_view=av.ctypes.data), P.AtlasParams(*cfg)
    lay = P.AtlasLayout()

    def call(flags=0, prm=good, nv=nv, v=vertex.ctypes.data, nf=nf, f=face.ctypes.data, vw=view.ctypes.data, cap=H, b=buf, layout=lay,
             scene=g.handle):
        return lib.pmvs_mesh_atlas(scene, flags, None if prm is None else C.byref(prm), nv, v, nf, f, vw, cap,
                                   None if b is None else C.byref(b), None if layout is None else C.byref(layout))

    assert call() == 0 and (av != -77).all() and rgb.tobytes() == wants[cfg][0]["rgb"].tobytes()
    rgb[:], av[:] = 201, -77
    nan, inf = float("nan"), float("inf")
    assert call(scene=None) == 1 and call(prm=None) == 1 and call(layout=None) == 1
    for flags in (1, 4, 2 | 8, -1):
        assert call(flags=flags) == 1
    for prm in ((48, 0, 1.0), (48, -1, 1.0), (300, 252, 1.0), (12, 8, 1.0), (65537, 8, 1.0), (48, 8, 0.0), (48, 8, -1.0), (48, 8, nan),
                (48, 8, inf)):
        assert call(prm=P.AtlasParams(*prm)) == 1, prm
    assert call(nv=-1) == 1 and call(nf=-1) == 1 and call(nv=1 << 31) == 1 and call(nf=1 << 31) == 1
    assert call(v=None) == 1 and call(f=None) == 1 and call(vw=None) == 1 and call(cap=-1) == 1
    dev = torch.device("cuda", g.device)
    cases = []
    for bad in (nv, -1):
        f2 = face.copy()
        f2[len(f2) // 2, 2] = bad
        cases.append((f2, view))
    for bad in (10, -2):
        v2 = view.copy()
        v2[len(v2) // 2] = bad
        cases.append((face, v2))
    for f2, v2 in cases:
        assert call(f=f2.ctypes.data, vw=v2.ctypes.data) == 1
        assert b"outside" in lib.pmvs_last_error()
        dv, df, dw = (torch.as_tensor(a, device=dev) for a in (vertex, f2, v2))
        out = torch.full((H * W * 3 + CANARY,), 201, dtype=torch.uint8, device=dev)
        oav = torch.full((nf + CANARY,), -77, dtype=torch.int32, device=dev)
        b = P.AtlasBuffers(rgb=out.data_ptr(), atlas_view=oav.data_ptr())
        assert call(flags=P.EXPORT_DEVICE, v=dv.data_ptr(), f=df.data_ptr(), vw=dw.data_ptr(), b=b) == 1
        assert b"outside" in lib.pmvs_last_error()
        assert (out == 201).all() and (oav == -77).all()   # rejected before anything was written
    assert (rgb == 201).all() and (av == -77).all()         # and no rejected call wrote
    assert call(nf=0, f=None, vw=None) == 0 and (rgb == 201).all() and lay.height == 0
