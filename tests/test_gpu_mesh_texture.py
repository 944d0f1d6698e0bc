"""pmvs_mesh_texture: per face of a mesh the target that sees it best, front-facing and unoccluded.  The expected
view, uv and score are test_gpu_mesh_raster.py's numpy restatement of the definition in include/pmvs_amd.h
(TEXTURING, part B, on the restated raster of part A), compared for exact equality of dtype, shape and bytes in host
and device mode, over all targets and over a sub-range, at depth_rel 0 and 0.01 and min_area 0 and 1.5.  The meshes
are that file's two: the real mesh with the occluder quad in front of the sphere as targets 0 and 1 see it, and the
hand-made one in the scene of ten targets, two of which share a projection so that scores tie.

The fixture asserts on the restatement alone that a face is left without a view for each reason (never drawn,
back-facing everywhere, occluded, below min_area), that a tie goes to the lower target, that a face's best-scoring
target is rejected by visibility and another wins, and that a corner passes through an empty pixel.  What the
library returns is also checked without the restatement: a textured face is drawn and front-facing in its view, its
corners at the scene's level lie inside that image, and its score is positive."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_mesh_raster import (CANARY, SUB, hand_case, homogeneous, real_case, restate_raster,  # noqa: F401 -- fixtures
                                  restate_texture)
from test_gpu_pixel_maps import image_dims

pytestmark = pytest.mark.gpu

NAMES = ("view", "uv", "score")
PARAMS = ((0.01, 0.0), (0.0, 0.0), (0.01, 1.5), (0.0, 1.5))  # depth_rel, min_area
HAND_SUB = (2, 6)  # targets 2 .. 7: the tie's two targets, across the groups of the full call


def reasons(per, out):
    """Per face without a view, why: the first of the four conditions no target of the range meets."""
    st = {k: np.stack([p[k] for p in per]) for k in ("drawn", "front", "visible", "large", "eligible")}
    none = out["view"] < 0
    assert (none == ~st["eligible"].any(axis=0)).all()
    never = ~st["drawn"].any(axis=0)
    back = ~never & ~(st["drawn"] & st["front"]).any(axis=0)
    occluded = ~never & ~back & ~(st["drawn"] & st["front"] & st["visible"]).any(axis=0)
    small = none & ~never & ~back & ~occluded
    return {"never": never, "back": back, "occluded": occluded, "small": small}


def rejected_best(per, out):
    """Faces whose best-scoring target among the drawn, front-facing and large enough ones is not visible, and
    which another target wins."""
    s = np.stack([np.where(p["drawn"] & p["front"] & p["large"], p["s"], np.float32(-1)) for p in per])
    top = s.argmax(axis=0)
    cols = np.arange(s.shape[1])
    vis_top = np.stack([p["visible"] for p in per])[top, cols]
    return (out["view"] >= 0) & (s[top, cols] > out["score"]) & ~vis_top


def through_empty(per, out):
    """Faces whose winning target has a corner on an empty pixel of the raster."""
    hit = np.zeros(len(out["view"]), bool)
    for p in per:
        hit |= (out["view"] == p["t"]) & p["through_empty"]
    return hit


def check_real_texture(o, inp, vertex, face, rs):
    """The restated outputs of mesh (a) per parameter set (and over SUB), with the branch asserts."""
    want = {}
    sub_rs = restate_raster(o, inp, vertex, face, SUB)[1]
    for prm in PARAMS:
        out, per = restate_texture(o, inp, vertex, face, rs, *prm)
        want[prm] = out
        want[prm, "sub"] = restate_texture(o, inp, vertex, face, sub_rs, *prm)[0]
        why = reasons(per, out)
        textured = out["view"] >= 0
        front_somewhere = np.stack([p["drawn"] & p["front"] for p in per]).any(axis=0)
        assert why["back"].sum() > 10 and textured.sum() > 100                        # several faces of each kind
        assert why["occluded"].sum() > 5
        assert set(np.unique(out["view"])) == {-1, 0, 1, 2, 3}
        assert rejected_best(per, out).sum() > 0 and through_empty(per, out).sum() > 0
        assert (out["score"][textured] > 0).all() and not out["score"][~textured].any() and not out["uv"][~textured].any()
        if prm[1] > 0:
            assert why["small"].sum() > 10
        want[prm, "shares"] = (textured.sum() / front_somewhere.sum(), int(why["occluded"].sum()))
    loose, tight = want[PARAMS[0], "shares"], want[PARAMS[1], "shares"]
    assert loose[0] > tight[0] and tight[1] > loose[1]                                 # depth_rel decides
    assert want[PARAMS[0]]["view"].tobytes() != want[PARAMS[0], "sub"]["view"].tobytes()
    return want


def check_hand_texture(o, inp, vertex, face, names, rs):
    """The restated outputs of mesh (b) per parameter set (and over HAND_SUB), with the branch asserts."""
    want = {}
    sub_rs = [rs[t] for t in range(HAND_SUB[0], HAND_SUB[0] + HAND_SUB[1])]
    for prm in PARAMS:
        out, per = restate_texture(o, inp, vertex, face, rs, *prm)
        want[prm] = out
        want[prm, "sub"] = restate_texture(o, inp, vertex, face, sub_rs, *prm)[0]
        why = reasons(per, out)
        assert why["never"][names["nan"][0]] and why["never"][names["zero_area"][0]]   # never drawn
        tie = (out["view"] == 2) & per[7]["eligible"] & (per[7]["s"] == out["score"])   # the copy of target 2 ties
        assert tie.sum() > 0 and not (out["view"] == 7).any()
        assert (per[2]["s"] == per[7]["s"]).all()
    assert (want[PARAMS[0]]["view"] >= 0).any() and want[PARAMS[0]]["uv"].any()
    return want


@pytest.fixture(scope="module")
def texture_wants(real_case, hand_case):
    P, g, o, inp, vertex, face, _, _, rs = real_case
    real = check_real_texture(o, inp, vertex, face, rs)
    P, h, ho, hinp, hvertex, hface, names, _, hrs = hand_case
    hand = check_hand_texture(ho, hinp, hvertex, hface, names, hrs)
    return real, hand


def texture_call(P, g, vertex, face, prm, first, num, device, names=NAMES):
    """pmvs_mesh_texture through ctypes into arrays with CANARY extra elements; the canaries are checked here."""
    nf = len(face)
    dt = {"view": (np.int32, torch.int32, -77, 1), "uv": (np.float32, torch.float32, -77.0, 6),
          "score": (np.float32, torch.float32, -77.0, 1)}
    buf, arrays = P.TextureBuffers(), {}
    if device:
        dev = torch.device("cuda", g.device)
        v, f = torch.as_tensor(vertex, device=dev).contiguous(), torch.as_tensor(face, device=dev).contiguous()
        ptrs = (v.data_ptr(), f.data_ptr())
        for k in names:
            arrays[k] = torch.full((nf * dt[k][3] + CANARY,), dt[k][2], dtype=dt[k][1], device=dev)
            setattr(buf, k, arrays[k].data_ptr())
    else:
        v, f = np.ascontiguousarray(vertex, np.float32), np.ascontiguousarray(face, np.int32)
        ptrs = (v.ctypes.data, f.ctypes.data)
        for k in names:
            arrays[k] = np.full(nf * dt[k][3] + CANARY, dt[k][2], dt[k][0])
            setattr(buf, k, arrays[k].ctypes.data)
    params = P.TextureParams(*prm)
    st = g.lib.pmvs_mesh_texture(g.handle, P.EXPORT_DEVICE if device else 0, first, num, C.byref(params), len(vertex), ptrs[0], nf,
                                 ptrs[1], C.byref(buf))
    assert st == 0, g.lib.pmvs_last_error()
    out = {}
    for k in names:
        a = arrays[k].cpu().numpy() if device else arrays[k]
        assert (a[nf * dt[k][3]:] == dt[k][2]).all(), k
        out[k] = a[:nf * dt[k][3]].reshape((nf, 6) if k == "uv" else (nf,))
    return out


def assert_same(got, want, names=NAMES):
    assert set(got) == set(names)
    for k in names:
        a = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        assert a.dtype == want[k].dtype and a.shape == want[k].shape, k
        assert a.tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("prm", PARAMS)
def test_texture_matches_restatement(real_case, hand_case, texture_wants, prm, device):
    real, hand = texture_wants
    P, g, o, inp, vertex, face, _, _, _ = real_case
    assert_same(texture_call(P, g, vertex, face, prm, 0, 4, device), real[prm])
    assert_same(texture_call(P, g, vertex, face, prm, SUB[0], len(SUB), device), real[prm, "sub"])
    P, h, ho, hinp, hvertex, hface, names, _, _ = hand_case
    assert_same(texture_call(P, h, hvertex, hface, prm, 0, 10, device), hand[prm])
    assert_same(texture_call(P, h, hvertex, hface, prm, *HAND_SUB, device), hand[prm, "sub"])


def test_texture_properties(real_case):
    """Without the restatement: a textured face is drawn and front-facing in its view, its corners at the scene's
    level lie inside that image, its score is positive and its uv are the level-0 projections."""
    P, g, o, inp, vertex, face, _, _, _ = real_case
    got = g.mesh_texture(vertex, face)   # the defaults: depth_rel 0.01, min_area 0
    view, uv, score = got["view"], got["uv"], got["score"]
    assert view.dtype == np.int32 and uv.shape == (len(face), 6) and (view >= 0).sum() > 100
    c4, dims = homogeneous(vertex), image_dims(inp)
    V = [vertex[face[:, k]].astype(np.float64) for k in range(3)]
    N = np.cross(V[1] - V[0], V[2] - V[0])
    for t in range(4):
        sel = view == t
        assert sel.any()
        xy, z = o.project(t, inp.level, c4), o.depth(t, c4)
        centre = o.camera(t, inp.level)[0:3].astype(np.float64)
        assert ((N[sel] * (centre - V[0][sel])).sum(axis=1) > 0).all()
        for k in range(3):
            x, y = xy[face[sel, k], 0].astype(np.float64), xy[face[sel, k], 1].astype(np.float64)
            assert (z[face[sel, k]] > 0).all()
            assert (np.floor(x + 0.5) >= 0).all() and (np.floor(x + 0.5) <= dims[t][0] - 1).all()
            assert (np.floor(y + 0.5) >= 0).all() and (np.floor(y + 0.5) <= dims[t][1] - 1).all()
        xy0 = o.project(t, 0, c4)
        assert np.array_equal(uv[sel].reshape(-1, 3, 2), xy0[face[sel]][:, :, :2])
        assert not np.array_equal(xy0[face[sel]][:, :, :2], xy[face[sel]][:, :, :2])   # level 0, not the scene's level 1
    assert (score[view >= 0] > 0).all() and not score[view < 0].any() and not uv[view < 0].any()


def test_texture_python_mirror_and_selected_arrays(hand_case, texture_wants):
    """Scene.mesh_texture in device mode with tensor inputs; each array alone (the running view and score are then
    the call's own scratch); no face writes nothing."""
    P, h, ho, hinp, hvertex, hface, names, _, _ = hand_case
    want = texture_wants[1][PARAMS[0]]
    dev = torch.device("cuda", h.device)
    got = h.mesh_texture(torch.as_tensor(hvertex, device=dev), torch.as_tensor(hface, device=dev), device=True)
    assert all(t.is_cuda and t.device.index == h.device for t in got.values())
    assert_same(got, want)
    for k in NAMES:
        assert_same(h.mesh_texture(hvertex, hface, arrays=(k,)), want, (k,))
        assert_same(texture_call(P, h, hvertex, hface, PARAMS[0], 0, 10, True, names=(k,)), want, (k,))
    for device in (False, True):
        texture_call(P, h, hvertex, hface[:0], PARAMS[0], 0, 10, device)   # only the canaries exist


def test_texture_errors(hand_case):
    """The rejection list with a real scene: the argument itself is what is rejected."""
    P, h, ho, hinp, vertex, face, names, _, _ = hand_case
    lib, nv, nf = h.lib, len(vertex), len(face)
    view = np.full(nf, -77, np.int32)
    buf, good = P.TextureBuffers(view=view.ctypes.data), P.TextureParams(0.01, 0.0)

    def call(flags=0, first=0, num=10, prm=good, nv=nv, v=vertex.ctypes.data, nf=nf, f=face.ctypes.data, b=buf, scene=h.handle):
        return lib.pmvs_mesh_texture(scene, flags, first, num, None if prm is None else C.byref(prm), nv, v, nf, f,
                                     None if b is None else C.byref(b))

    nan, inf = float("nan"), float("inf")
    assert call() == 0 and (view != -77).all()
    view[:] = -77
    assert call(scene=None) == 1 and call(b=None) == 1 and call(prm=None) == 1
    for flags in (1, 4, 2 | 8, -1):
        assert call(flags=flags) == 1
    for first, num in ((-1, 1), (0, 0), (9, 2), (10, 1), (0, 11)):
        assert call(first=first, num=num) == 1
    for prm in ((-0.01, 0.0), (nan, 0.0), (inf, 0.0), (0.01, -1.0), (0.01, nan), (0.01, inf)):
        assert call(prm=P.TextureParams(*prm)) == 1
    assert call(nv=-1) == 1 and call(nf=-1) == 1 and call(nv=1 << 31) == 1 and call(nf=1 << 31) == 1
    assert call(v=None) == 1 and call(f=None) == 1
    dev = torch.device("cuda", h.device)
    for bad in (nv, -1):
        f = face.copy()
        f[len(f) // 2, 2] = bad
        assert call(f=f.ctypes.data) == 1 and b"vertex id" in lib.pmvs_last_error()
        dv, df = torch.as_tensor(vertex, device=dev), torch.as_tensor(f, device=dev)
        out = torch.full((nf,), -77, dtype=torch.int32, device=dev)
        b = P.TextureBuffers(view=out.data_ptr())
        assert call(flags=P.EXPORT_DEVICE, v=dv.data_ptr(), f=df.data_ptr(), b=b) == 1 and b"vertex id" in lib.pmvs_last_error()
        assert (out == -77).all()   # rejected before anything was written
    assert (view == -77).all()      # and no rejected call wrote
    assert call(nf=0, f=None) == 0 and (view == -77).all()
