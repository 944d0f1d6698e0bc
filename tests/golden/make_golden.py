#!/usr/bin/env python3
"""Regenerates tests/golden/*.npz -- golden input/output vectors for the PMVS hot path.

Scenes are the deterministic synthetic rings of SURVEY.md §8(d) (pmvs_synth_ring, CPU code
in libpmvs_amd.so; the images themselves are not stored, only their CRC32, since the
renderer regenerates them bit-for-bit).  Expected outputs come from two sources:
  * oracle/_ref (the reference's own camera.cpp compiled unmodified, and its header-inline
    CImage::getColor / isSafe): per-view camera centre / optical axis / axes / per-level
    projection, CCamera::project and computeDepth of sample points, and bilinear getColor
    samples on every pyramid level; the candidate centres of CExpand::findEmptyBlocks
    (expand.cpp:176-177 evaluated with the reference headers, expand_dirs.npz); the Harris and
    DoG feature points of every golden view (harris.cpp / dog.cpp, features.npz); the seed
    phase's setF / computeEPD / triangulation of feature pairs (seeds.npz); the depth-map winners,
    visible-image lists and _vpgrids of CFilter::setDepthMapsVGridsVPGridsAddPatchV and the answers of
    CExpand::checkCounts / updateCounts (oracle/_ref/filter, filter_pin.npz) -- these vectors are
    REFERENCE outputs;
  * oracle/liboracle.so (the CPU restatement, pinned on the pieces above): pyramid CRCs,
    grabTex textures, my_f values, full preProcess->refinePatch->postProcess records and the
    seed phase's seed patches (seeds.npz).
Run from the repo root in the build container:  python tests/golden/make_golden.py [name ...]
"""
import os
import sys
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "cmvs-pmvs_amd"), os.path.join(ROOT, "oracle"), os.path.dirname(HERE)]

import pmvs_amd as P  # noqa: E402
import pyoracle as O  # noqa: E402
import pmvs_cases  # noqa: E402

# name: (views, width, height, level, csize, n_tex_cands, n_eval_cands, n_refine)
SCENES = {
    "c1": (3, 640, 480, 2, 4, 60, 60, 300),
    "ring8": (8, 320, 240, 1, 2, 60, 60, 300),
}


def write_contour(path, proj):
    with open(path, "w") as f:
        f.write("CONTOUR\n")
        for row in proj:
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def ref_cameras(proj, max_level, level_count):
    """Per view: 29 floats per level from the reference CCamera (camera.cpp:13-121)."""
    R = O.ref_lib()
    if R is None:
        raise SystemExit("oracle/_ref not built (reference absent): cannot regenerate reference vectors")
    out = np.zeros((len(proj), level_count, 29), np.float32)
    with tempfile.TemporaryDirectory() as d:
        for v, pm in enumerate(proj):
            path = os.path.join(d, "%08d.txt" % v)
            write_contour(path, pm)
            for lv in range(level_count):
                R.ref_camera(path.encode(), max_level, lv, out[v, lv].ctypes.data)
    return out


def ref_project(proj, max_level, level, pts):
    R = O.ref_lib()
    out = np.zeros((len(proj), len(pts), 3), np.float32)
    with tempfile.TemporaryDirectory() as d:
        for v, pm in enumerate(proj):
            path = os.path.join(d, "%08d.txt" % v)
            write_contour(path, pm)
            R.ref_project(path.encode(), max_level, level, pts.ctypes.data, len(pts), out[v].ctypes.data)
    return out


def ref_depth(proj, max_level, pts):
    """CCamera::computeDepth (camera.cpp:445-452) per view and point."""
    R = O.ref_lib()
    out = np.zeros((len(proj), len(pts)), np.float32)
    with tempfile.TemporaryDirectory() as d:
        for v, pm in enumerate(proj):
            path = os.path.join(d, "%08d.txt" % v)
            write_contour(path, pm)
            R.ref_camera_depth(path.encode(), max_level, pts.ctypes.data, len(pts), out[v].ctypes.data)
    return out


def color_points(rng, w, h, n):
    """Sample positions inside CImage::isSafe (x in [0, w-2], y in [0, h-2]) incl. the corners,
    integer positions and positions one float ulp below an integer."""
    xy = np.stack([rng.uniform(0, w - 2, n), rng.uniform(0, h - 2, n)], 1).astype(np.float32)
    xy[:8] = np.array([[0, 0], [w - 2, h - 2], [0, h - 2], [w - 2, 0], [1, 1], [w / 2, h / 2],
                       [np.nextafter(np.float32(1), np.float32(0)), 2], [3.5, 2.25]], np.float32)
    xy[8:40] = np.floor(xy[8:40])
    xy[40:72] = np.nextafter(np.ceil(xy[40:72]), np.float32(0))
    return xy


def ref_colors(o, views, maxlv, n=512):
    """CImage::getColor (image.hpp:435-476) of the reference header on the oracle's pyramid levels."""
    R = O.ref_lib()
    rng = np.random.default_rng(11)
    xys, cols = [], []
    for v in range(views):
        for lv in range(maxlv):
            img = np.ascontiguousarray(o.get_level(v, lv))
            h, w = img.shape[:2]
            xy = color_points(rng, w, h, n)
            out = np.zeros((n, 3), np.float32)
            safe = np.zeros(n, np.int32)
            R.ref_get_color(img.ctypes.data, w, h, xy.ctypes.data, n, out.ctypes.data, safe.ctypes.data)
            assert safe.all()
            xys.append(xy)
            cols.append(out)
    return (np.stack(xys).reshape(views, maxlv, n, 2), np.stack(cols).reshape(views, maxlv, n, 3))


def expand_dir_inputs(rng, n=2000):
    """Parent (coord, normal, radius) triples for findEmptyBlocks' candidate centres: random and
    axis-aligned normals (ortho's branches), radii from 1e-3 to 1."""
    coord = np.concatenate([rng.normal(0, 1, (n, 3)), np.ones((n, 1))], 1).astype(np.float32)
    nrm = rng.normal(0, 1, (n, 3))
    nrm[:6] = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    normal = np.concatenate([nrm, np.zeros((n, 1))], 1).astype(np.float32)
    radius = np.exp(rng.uniform(np.log(1e-3), 0, n)).astype(np.float32)
    return coord, normal, radius


def make_expand_dirs():
    R = O.ref_lib()
    coord, normal, radius = expand_dir_inputs(np.random.default_rng(13))
    out = np.zeros((len(coord), 6, 4), np.float32)
    R.ref_expand_dirs(coord.ctypes.data, normal.ctypes.data, radius.ctypes.data, len(coord), out.ctypes.data)
    path = os.path.join(HERE, "expand_dirs.npz")
    np.savez_compressed(path, coord=coord, normal=normal, radius=radius, ref_coords=out)
    print(f"{path}: {os.path.getsize(path)} B")


def isneighbor_records(rng, n):
    """Patch pairs for CFindMatch::isNeighbor / isNeighborRadius (findMatch.cpp:125-185): (n, 21) float32
    records (lhs coord, normal, dscale, rhs coord, normal, dscale, hunit, threshold, radius) with
    random geometry at the scales of a patch model (dscale and hunit ~1e-2 around a unit sphere)."""
    c0 = rng.normal(0, 1, (n, 3))
    n0 = rng.normal(0, 1, (n, 3))
    n0 /= np.linalg.norm(n0, axis=1, keepdims=True)
    tang = rng.normal(0, 1, (n, 3))
    tang -= (tang * n0).sum(1, keepdims=True) * n0
    tang /= np.linalg.norm(tang, axis=1, keepdims=True)
    ds0 = np.exp(rng.uniform(np.log(2e-3), np.log(2e-2), n))
    ds1 = ds0 * np.exp(rng.uniform(-0.3, 0.3, n))
    hunit = ds0 * np.exp(rng.uniform(-1, 1, n))
    along = rng.uniform(0, 6, n) * hunit
    off = rng.normal(0, 1, n) * ds0 * rng.choice([0.3, 1, 3], n)
    c1 = c0 + along[:, None] * tang + off[:, None] * n0
    ang = rng.uniform(0, np.pi, n) * rng.choice([0.05, 0.3, 1.0], n)
    axis = np.cross(n0, tang)
    n1 = n0 * np.cos(ang)[:, None] + axis * np.sin(ang)[:, None]
    thr = rng.choice([0.5, 1.0, 2.0, 4.0], n)
    radius = hunit * rng.uniform(0.5, 6, n)
    r = np.zeros((n, 21), np.float32)
    r[:, 0:3], r[:, 3] = c0, 1
    r[:, 4:7] = n0
    r[:, 8] = ds0
    r[:, 9:12], r[:, 12] = c1, 1
    r[:, 13:16] = n1
    r[:, 17], r[:, 18], r[:, 19], r[:, 20] = ds1, hunit, thr, radius
    return r


def isneighbor_boundary(rng, n, col, lo, hi, steps=40):
    """Records on the decision boundary of the REFERENCE's isNeighbor (or isNeighborRadius, col 1):
    per record one scalar (the normal offset of rhs, scaled) is bisected between lo and hi until the
    reference's answer flips between adjacent float32 values; both sides are kept."""
    base = isneighbor_records(rng, n)
    d = base[:, 9:12] - base[:, 0:3]
    a = np.full(n, lo, np.float64)
    b = np.full(n, hi, np.float64)

    def at(t):
        r = base.copy()
        r[:, 9:12] = (base[:, 0:3] + d * t[:, None]).astype(np.float32)
        return r
    fa = O.ref_is_neighbor(at(a))[:, col]
    fb = O.ref_is_neighbor(at(b))[:, col]
    keep = fa != fb
    for _ in range(steps):
        m = 0.5 * (a + b)
        fm = O.ref_is_neighbor(at(m))[:, col]
        same = fm == fa
        a = np.where(same, m, a)
        b = np.where(same, b, m)
    return np.concatenate([at(a)[keep], at(b)[keep]])


def make_isneighbor():
    """CFindMatch::isNeighbor / isNeighborRadius of the reference's own findMatch.cpp (compiled
    unmodified in oracle/_ref/isneighbor) on random patch pairs and on pairs bisected onto the
    reference's decision boundaries (threshold, radius, and the 120-degree normal test)."""
    rng = np.random.default_rng(125)
    recs = [isneighbor_records(rng, 3000), isneighbor_boundary(rng, 1000, 0, 0.0, 4.0),
            isneighbor_boundary(rng, 1000, 1, 0.0, 4.0)]
    # normals near 120 degrees apart: lhs . rhs against cos(120 deg) (findMatch.cpp:135)
    r = isneighbor_records(rng, 500)
    r[:, 9:12] = r[:, 0:3]
    n0 = r[:, 4:7].astype(np.float64)
    perp = np.cross(n0, rng.normal(0, 1, (len(r), 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    ang = 2 * np.pi / 3 + rng.normal(0, 1e-6, len(r))
    r[:, 13:16] = (n0 * np.cos(ang)[:, None] + perp * np.sin(ang)[:, None]).astype(np.float32)
    recs.append(r)
    records = np.concatenate(recs).astype(np.float32)
    ref = O.ref_is_neighbor(records)
    path = os.path.join(HERE, "isneighbor.npz")
    np.savez_compressed(path, records=records, ref=ref)
    print(f"{path}: {os.path.getsize(path)} B, {len(records)} pairs, isNeighbor true {int(ref[:, 0].sum())}, "
          f"isNeighborRadius true {int(ref[:, 1].sum())}")


def make_features():
    """CDetectFeatures' two detectors (harris.cpp / dog.cpp compiled unmodified in oracle/_ref) on
    every view of the scene goldens at their option level: REFERENCE outputs (features.npz)."""
    g = {}
    for name, (views, width, height, level, csize, *_rest) in SCENES.items():
        inp, p = P.synth_scene(views, width, height, level=level, csize=csize, supersample=2)
        o = O.OracleScene(inp)
        pts, off = [], [0]
        for v in range(views):
            f = O.ref_detect_features(o.get_level(v, level), fcsize=16)
            pts.append(f)
            off.append(off[-1] + len(f))
        o.close()
        g[f"{name}_points"] = np.concatenate(pts).astype(np.float32)
        g[f"{name}_offsets"] = np.array(off, np.int64)
    path = os.path.join(HERE, "features.npz")
    np.savez_compressed(path, **g)
    print(f"{path}: {os.path.getsize(path)} B, " + ", ".join(f"{k} {len(v)}" for k, v in g.items() if k.endswith("points")))


def ref_seed_geometry(proj, max_level, level, i0, i1, xy0, xy1):
    """Image::setF / computeEPD and the CSeed::unproject triangulation evaluated with the
    reference's CCamera (camera.cpp) and numeric headers (oracle/_ref ref_seed_geometry)."""
    R = O.ref_lib()
    n = len(xy0)
    F = np.zeros(9, np.float64)
    epd = np.zeros(n, np.float32)
    co = np.zeros((n, 4), np.float32)
    with tempfile.TemporaryDirectory() as d:
        p0, p1 = os.path.join(d, "a.txt"), os.path.join(d, "b.txt")
        write_contour(p0, proj[i0])
        write_contour(p1, proj[i1])
        R.ref_seed_geometry(p0.encode(), p1.encode(), max_level, level, xy0.ctypes.data, xy1.ctypes.data, n,
                            F.ctypes.data, epd.ctypes.data, co.ctypes.data)
    return F.reshape(3, 3), epd, co


def make_seeds():
    """Seed phase vectors (seeds.npz): per golden scene, setF / computeEPD / triangulation of feature
    point pairs from the REFERENCE (oracle/_ref), and the oracle's CSeed::run result (seed patches
    in addPatch order + trial/pass/fail counts) on the reference-detected features (regression)."""
    feats = dict(np.load(os.path.join(HERE, "features.npz")))
    g = {}
    rng = np.random.default_rng(17)
    for name, (views, width, height, level, csize, *_rest) in SCENES.items():
        inp, p = P.synth_scene(views, width, height, level=level, csize=csize, supersample=2)
        off = feats[f"{name}_offsets"]
        pts = [feats[f"{name}_points"][off[v]:off[v + 1]] for v in range(views)]
        pairs = [(0, 1), (1, 0), (0, views - 1), (views - 1, 1)]
        F_all, epd_all, co_all, xy_all = [], [], [], []
        for i0, i1 in pairs:
            a = pts[i0][:, :2]
            b = pts[i1][rng.integers(0, len(pts[i1]), len(a)), :2]
            xy0 = np.ascontiguousarray(a, np.float32)
            xy1 = np.ascontiguousarray(b, np.float32)
            F, epd, co = ref_seed_geometry(inp.projections, level + 3, level, i0, i1, xy0, xy1)
            F_all.append(F); epd_all.append(epd); co_all.append(co); xy_all.append(np.stack([xy0, xy1], 1))
        g[f"{name}_pairs"] = np.array(pairs, np.int32)
        g[f"{name}_ref_F"] = np.stack(F_all)
        g[f"{name}_xy"] = np.concatenate(xy_all)
        g[f"{name}_pair_len"] = np.array([len(e) for e in epd_all], np.int64)
        g[f"{name}_ref_epd"] = np.concatenate(epd_all)
        g[f"{name}_ref_coords"] = np.concatenate(co_all)
        o = O.OracleScene(inp)
        seeds, st = o.seed_run(pts)
        o.close()
        g[f"{name}_seeds"] = seeds
        g[f"{name}_seed_stats"] = np.array([st[k] for k in ("trial", "pass", "fail0", "fail1")], np.int64)
        print(f"{name}: {len(seeds)} seeds, {st}")
    path = os.path.join(HERE, "seeds.npz")
    np.savez_compressed(path, **g)
    print(f"{path}: {os.path.getsize(path)} B")


def organizer_cases(o, inp, p, rng, n=600):
    """Inputs of the organizer / photo-set pins: points on and around the synthetic surface
    (candidates jittered along their normals, so several compete for a depth-map cell) and far
    points; image lists of every length; view sets and angle bounds for checkAngles."""
    V = len(inp.images)
    c = P.synth_candidates(p, inp.projections, n, seed=int(rng.integers(1 << 30)))
    coords = c["coord"].astype(np.float32).copy()
    coords[:, :3] += (c["normal"][:, :3] * rng.normal(0, 0.02, (n, 1))).astype(np.float32)
    coords[-40:, :3] = rng.normal(0, 5.0, (40, 3)).astype(np.float32)  # far, often outside every grid
    coords[:, 3] = 1.0
    lists = [sorted(rng.choice(V, int(rng.integers(1, V + 1)), replace=False).tolist()) for _ in range(n)]
    lists = [rng.permutation(l).tolist() for l in lists]
    vis_images = rng.integers(0, inp.num_targets, n).astype(np.int32)
    ang_lists = [rng.choice(V, int(rng.integers(2, min(V, 7) + 1)), replace=False).tolist() for _ in range(n)]
    return coords, lists, vis_images, ang_lists


def organizer_ops(coords, lists, vis_images, ang_lists, min_angle, max_angle):
    return [("grids_images", coords, lists), ("grids", coords, lists), ("depth", coords[:300]),
            ("depth", coords), ("vis0", coords, vis_images), ("angles", coords, ang_lists, min_angle, max_angle),
            ("angles", coords, ang_lists, 0.05, 0.6), ("dist",)]


def make_organizer():
    """CPatchOrganizerS::setGridsImages / setGrids / updateDepthMaps / isVisible0 and
    CPhotoSetS::checkAngles / setDistances of the reference's own patchOrganizerS.cpp /
    photoSetS.cpp (oracle/_ref/organizer) on the ring8 scene."""
    views, width, height, level, csize = SCENES["ring8"][:5]
    inp, p = P.synth_scene(views, width, height, level=level, csize=csize, supersample=2)
    o = O.OracleScene(inp)
    maxlv = level + 3
    w, h = o.level_sizes(maxlv)
    coords, lists, vis_images, ang_lists = organizer_cases(o, inp, p, np.random.default_rng(17))
    min_angle = float(np.float32(inp.max_angle_rad()))
    max_angle = float(np.float32(np.float64(np.float32(60.0)) * np.pi / 180.0))
    ops = organizer_ops(coords, lists, vis_images, ang_lists, min_angle, max_angle)
    ref = O.ref_organizer(inp.projections, w, h, inp.num_targets, level, csize, ops)
    if ref is None:
        raise SystemExit("oracle/_ref/organizer not built (reference absent)")
    o.close()
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    aoff = np.zeros(len(ang_lists) + 1, np.int64)
    aoff[1:] = np.cumsum([len(l) for l in ang_lists])
    g = {"params": np.array([views, width, height, level, csize, inp.num_targets], np.int64),
         "widths": w, "heights": h, "coords": coords, "list_off": off,
         "lists": np.array([x for l in lists for x in l], np.int32), "vis_images": vis_images,
         "ang_off": aoff, "ang_lists": np.array([x for l in ang_lists for x in l], np.int32),
         "angles": np.array([min_angle, max_angle], np.float32)}
    for k, (op, r) in enumerate(zip(ops, ref)):
        if op[0] in ("grids_images", "grids"):
            g[f"ref{k}_n"] = np.array([len(x) for x in r], np.int32)
            g[f"ref{k}"] = np.concatenate(r).astype(np.int32)
        else:
            g[f"ref{k}"] = r
    path = os.path.join(HERE, "organizer.npz")
    np.savez_compressed(path, **g)
    kept = g["ref0_n"].sum()
    print(f"{path}: {os.path.getsize(path)} B, setGridsImages kept {kept} of {off[-1]} entries, "
          f"depth cells set {(g['ref3'] >= 0).sum()}, visible {g['ref4'][:, 0].sum()}/{len(coords)}")


FILTER_PIN = dict(views=6, width=320, height=240, level=1, num_targets=4, crop=(1, 300, 200), n_cand=2600, seed=41,
                  copies=48, count_ops=((1, 4, 360), (2, 2, 360)))


def filter_pin_scene():
    """6 views at 320 x 240, level 1, 4 targets, target 1 cropped to 300 x 200 as in
    tests/test_gpu_depth_maps.py: the targets' cell grids differ in size (80 x 60, 75 x 50, 80 x 60, 80 x 60)."""
    c = FILTER_PIN
    inp, p = P.synth_scene(c["views"], c["width"], c["height"], level=c["level"], num_targets=c["num_targets"],
                           supersample=2)
    t, w, h = c["crop"]
    inp.images[t] = np.ascontiguousarray(inp.images[t][:h, :w])
    return inp, p


def filter_pin_patches(o, inp, p):
    """The patch set of the filter pins, as PATCH_DTYPE records, the (original, copy) row pairs and the
    number of leading rows that are a plain model (refined patches, outliers, fixed rows):
    oracle-refined patches of the scene; the outliers of tests/test_gpu_filter.make_patch_set (copies
    pushed 25 dscale towards their reference camera); a few fixed rows; rows far outside every image and
    rows on the images' border cells (their lists point at arbitrary in-grid cells: addPatch takes the
    lists as given); and, last, exact copies of rows that win depth-map cells -- depth ties far apart in
    the array."""
    c = FILTER_PIN
    rng = np.random.default_rng(c["seed"])
    cands = P.synth_candidates(p, inp.projections, c["n_cand"], seed=c["seed"])
    pa = P.patches_from_refined(o.refine_batch(cands, nthreads=8)[0])
    src = pa[rng.choice(len(pa), max(1, len(pa) // 50), replace=False)].copy()
    for q in src:
        cam = np.asarray(inp.projections[int(q["images"][0])], np.float64)
        d = -np.linalg.solve(cam[:, :3], cam[:, 3]) - q["coord"][:3].astype(np.float64)
        d /= np.linalg.norm(d)
        q["coord"][:3] = (q["coord"][:3] + d * 25.0 * q["dscale"]).astype(np.float32)
        q["ncc"] = np.float32(inp.threshold + 0.02)
    pa = np.concatenate([pa, src])
    pa["fix"][rng.random(len(pa)) < 0.01] = 1
    gw, gh = o.grid_sizes()
    far = pa[rng.choice(len(pa), 60, replace=False)].copy()
    far["coord"][:40, :3] = rng.uniform(-1.6, 1.6, (40, 3)).astype(np.float32)  # many leave the images
    far["coord"][40:43, :3] = [(0, 0, 50), (50, 0, 0), (0, -50, 0)]
    # points whose projection into a target falls on a first or last column / row of its cells: a surface
    # point is moved along the image's x or y direction in space, bisecting on the oracle's isVisible0
    # (depth 0: "inside the grid") until the last position inside
    edge = pa[rng.choice(len(pa), 64, replace=False)].copy()
    for i, q in enumerate(edge):
        t, axis, sign = i % inp.num_targets, (i // inp.num_targets) % 2, 1 - 2 * ((i // (2 * inp.num_targets)) % 2)
        step = np.linalg.pinv(np.asarray(inp.projections[t], np.float64)[:, :3])[:, axis]
        step *= sign / np.linalg.norm(step)
        x0 = q["coord"].astype(np.float64)

        def at(a):
            x = x0.copy()
            x[:3] += a * step
            return x.astype(np.float32)

        def inside(a):
            return bool(o.organizer_ops([("vis0", at(a)[None], [t])])[0][0, 0])
        lo, hi = 0.0, 4.0
        if not inside(lo) or inside(hi):
            continue
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if inside(mid) else (lo, mid)
        q["coord"] = at(lo)
    n_plain = len(pa)
    crafted = np.concatenate([far[:43], edge])
    for q in crafted:  # arbitrary in-grid cells of one or two targets, plus a non-target image
        k = int(rng.integers(1, 3))
        ts = rng.permutation(inp.num_targets)[:k]
        q["num_images"] = k + 1
        q["images"][:k] = ts
        q["grids"][:k, 0] = [rng.integers(0, gw[t]) for t in ts]
        q["grids"][:k, 1] = [rng.integers(0, gh[t]) for t in ts]
        q["images"][k] = inp.num_targets + int(rng.integers(0, len(inp.images) - inp.num_targets))
        q["grids"][k] = (3, 3)
        q["fix"] = 0
    pa = np.concatenate([pa, crafted])
    coords, lists = filter_pin_lists(pa)
    win = np.unique(o.filter_ops(coords, lists, [("depth_maps",)])[0]["winner"])
    orig = rng.permutation(win[(win >= 0) & (win < len(pa) // 2)])[:c["copies"]]
    orig.sort()
    pairs = np.stack([orig, len(pa) + np.arange(len(orig))], 1).astype(np.int32)
    return np.concatenate([pa, pa[orig]]), pairs, n_plain


def filter_pin_lists(pa):
    """PATCH_DTYPE records -> (coords [n, 4], per row its (image, ix, iy) list)."""
    lists = []
    for q in pa:
        k = int(q["num_images"])
        lists.append(np.concatenate([q["images"][:k, None].astype(np.int32), q["grids"][:k].astype(np.int32)], 1))
    return np.ascontiguousarray(pa["coord"], np.float32), lists


def filter_pin_count_calls(rng, lists, gw, gh, V, tnum, depth, k):
    """A sequence of (kind, images3, vimages3) calls for checkCounts (kind 0) / updateCounts (kind 1):
    candidates with 0-4 cells taken from a pool of three unoccupied cells per target (so their counts climb
    through the threshold as the updates accumulate) and 0-2 occupied cells, sometimes an image >= tnum,
    sometimes a cell outside the grid; vimages in the remaining targets.  Every eighth call is the same
    probe check, whose answer the earlier updates change."""
    occ = [[] for _ in range(tnum)]
    for l in lists:
        for t, ix, iy in l:
            if t < tnum:
                occ[t].append((int(ix), int(iy)))
    pool = []
    for t in range(tnum):
        taken, cells = set(occ[t]), []
        while len(cells) < 3:
            c = (int(rng.integers(0, gw[t])), int(rng.integers(0, gh[t])))
            if c not in taken:
                taken.add(c)
                cells.append(c)
        pool.append(cells)
    ne = 3 if depth <= 1 else 2
    probe = [(t,) + pool[t][0] for t in range(ne)] + [(tnum - 1,) + occ[tnum - 1][0]]
    calls = []
    for c in range(k):
        if c % 8 == 7:
            calls.append((0, probe, []))
            continue
        e, f = int(rng.integers(0, 5)), int(rng.integers(0, 3))
        ts = rng.permutation(tnum).tolist()
        il = [(t,) + pool[t][int(rng.integers(0, 3))] for t in ts[:e]]
        il += [(t,) + occ[t][int(rng.integers(0, len(occ[t])))] for t in ts[e:e + f]]
        rest = ts[e + f:]
        if rest and rng.random() < 0.25:  # a cell outside the grid
            t = rest.pop()
            il.append((t,) + [(-1, 2), (int(gw[t]), 2), (2, -1), (2, int(gh[t]))][int(rng.integers(0, 4))])
        if rng.random() < 0.3:
            il.append((int(rng.integers(tnum, V)), int(rng.integers(0, 40)), int(rng.integers(0, 40))))
        il = [il[i] for i in rng.permutation(len(il))]
        vl = []
        for t in rest:
            r = rng.random()
            if r < 0.5:
                vl.append((t,) + pool[t][int(rng.integers(0, 3))])
            elif r < 0.6:
                vl.append((t, int(gw[t]), int(gh[t])))
        calls.append((int(rng.random() < 0.4), il, vl))
    return calls


def filter_pin_coverage(g):
    """The edges the filter pins need, asserted from the fixture's inputs and the REFERENCE's outputs."""
    tnum, min_num = int(g["params"][5]), int(g["params"][9])
    n = len(g["coords"])
    off = g["list_off"]
    # ---- depth maps
    win, pairs = g["ref_dm_winner"], g["copies"]
    assert len(g["ref_dm_collected"]) == n and len(np.unique(g["ref_dm_collected"])) == n  # every row is in a target cell
    assert not np.array_equal(g["ref_dm_collected"], np.arange(n))  # collectPatches' order is its own
    assert len(pairs) >= 40 and (pairs[:, 1] - pairs[:, 0]).min() > n // 3
    assert all(np.array_equal(g["coords"][a], g["coords"][b]) for a, b in pairs)
    assert np.isin(pairs[:, 0], win).sum() >= 40 and not np.isin(pairs[:, 1], win).any()  # ties: the earlier row
    filled = win >= 0
    assert filled.sum() >= 1000 and len(np.unique(win[filled])) >= 100 and (~filled).any()
    assert not g["ref_dm_depth"][~filled].view(np.uint32).any()
    vrow = np.repeat(np.arange(n), g["ref_dm_vcount"])
    listed = np.zeros((n, tnum), bool)
    for i in range(n):
        t = g["lists"][off[i]:off[i + 1], 0]
        listed[i, t[t < tnum]] = True
    assert not listed[vrow, g["ref_dm_vlists"][:, 0]].any()  # vimages are the targets not in images
    # rows outside every grid they are not listed in; none of them wins a cell (their lists are arbitrary)
    outside = np.flatnonzero((g["ref_dm_vcount"] == 0) & (listed.sum(1) <= 2))
    assert len(outside) >= 3 and (~np.isin(outside, win)).sum() >= 3
    gw, gh = g["grid_dims"][:, 0], g["grid_dims"][:, 1]
    vl = g["ref_dm_vlists"]
    assert ((vl[:, 1] == gw[vl[:, 0]] - 1) | (vl[:, 2] == gh[vl[:, 0]] - 1)).sum() >= 5  # border cells
    assert ((vl[:, 1] == 0) | (vl[:, 2] == 0)).any()
    assert g["ref_dm_vpcount"].sum() == len(vl) and g["ref_dm_vpcount"].max() >= 2
    # ---- counts: replay the bookkeeping the calls imply (counts only ever grow by one per touched cell)
    cell0 = np.concatenate([[0], np.cumsum(gw[:tnum].astype(np.int64) * gh[:tnum])])
    occupied = np.zeros(cell0[-1], bool)
    lt = g["lists"]
    m = lt[:, 0] < tnum
    occupied[cell0[lt[m, 0]] + lt[m, 2].astype(np.int64) * gw[lt[m, 0]] + lt[m, 1]] = True
    depths = set()
    for j in range(int(g["count_ops"])):
        depth, cthr = (int(x) for x in g[f"c{j}_params"])
        depths.add(depth <= 1)
        kinds, ret = g[f"c{j}_kinds"], g[f"c{j}_ret"]
        ioff, il, voff, vl = g[f"c{j}_ioff"], g[f"c{j}_ilists"], g[f"c{j}_voff"], g[f"c{j}_vlists"]
        counts = np.zeros(cell0[-1], np.int64)
        seen_empty, seen_full0, at, oob, nontarget, probes = set(), False, set(), False, False, {}
        for c in range(len(kinds)):
            full = empty = 0
            entries = [tuple(x) for x in il[ioff[c]:ioff[c + 1]]]
            ventries = [tuple(x) for x in vl[voff[c]:voff[c + 1]]] if kinds[c] else []
            for t, ix, iy in entries + ventries:
                if t >= tnum:
                    nontarget = True
                    continue
                if not (0 <= ix < gw[t] and 0 <= iy < gh[t]):
                    oob = True
                    continue
                i = cell0[t] + iy * gw[t] + ix
                if kinds[c] == 0 and occupied[i]:
                    full += 1
                    continue
                at.add(int(counts[i]))
                if cthr <= counts[i]:
                    full += 1
                else:
                    empty += 1
                if kinds[c]:
                    counts[i] += 1
            if kinds[c] == 0:
                if full:
                    seen_empty.add(empty)
                else:
                    seen_full0 = True
                probes.setdefault((tuple(entries),), set()).add(int(ret[c]))
        assert np.array_equal(counts, g[f"c{j}_counts"]) and counts.max() < 255
        edge = min_num if depth <= 1 else min_num - 1
        assert {edge - 1, edge} <= seen_empty and {min_num - 2, min_num - 1, min_num} <= seen_empty and seen_full0
        assert {cthr - 1, cthr} <= at and oob and nontarget
        for kind in (0, 1):
            assert set(ret[kinds == kind].tolist()) == {0, 1}, (j, kind)
        assert any(len(v) == 2 for v in probes.values())  # earlier updates change a later answer
    assert depths == {True, False}


def save_npz(path, g):
    """np.savez_compressed with fixed member dates, so a second run writes the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in g.items():
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue())


def filter_pin_ops(g):
    """The op list of OracleScene.filter_ops / pyoracle.ref_filter that the fixture's inputs describe."""
    ops = [("depth_maps",)]
    for j in range(int(g["count_ops"])):
        depth, cthr = (int(x) for x in g[f"c{j}_params"])
        ioff, il, voff, vl = g[f"c{j}_ioff"], g[f"c{j}_ilists"], g[f"c{j}_voff"], g[f"c{j}_vlists"]
        calls = [(int(g[f"c{j}_kinds"][c]), il[ioff[c]:ioff[c + 1]], vl[voff[c]:voff[c + 1]])
                 for c in range(len(ioff) - 1)]
        ops.append(("counts", depth, cthr, calls))
    return ops


def filter_pin_inputs(g):
    off = g["list_off"]
    return g["coords"], [g["lists"][off[i]:off[i + 1]] for i in range(len(off) - 1)]


def filter_pin_records(g):
    """The fixture's patch set as PATCH_DTYPE records (empty vimages)."""
    coords, lists = filter_pin_inputs(g)
    pa = np.zeros(len(coords), P.PATCH_DTYPE)
    pa["coord"] = coords
    for f in ("normal", "ncc", "dscale", "ascale", "timages", "fix"):
        pa[f] = g[f]
    for q, l in zip(pa, lists):
        q["num_images"] = len(l)
        q["images"][:len(l)] = l[:, 0]
        q["grids"][:len(l)] = l[:, 1:]
    return pa


def make_filter():
    """CFilter::setDepthMapsVGridsVPGridsAddPatchV(0) (depth-map winners, visible-image lists, _vpgrids)
    and CExpand::checkCounts / updateCounts of the reference's own filter.cpp / expand.cpp
    (oracle/_ref/filter) on the filter-pin patch set: inputs and REFERENCE outputs only (filter_pin.npz)."""
    c = FILTER_PIN
    inp, p = filter_pin_scene()
    o = O.OracleScene(inp)
    maxlv = inp.level + 3
    w, h = o.level_sizes(maxlv)
    gw, gh = o.grid_sizes()
    pa, pairs, n_plain = filter_pin_patches(o, inp, p)
    coords, lists = filter_pin_lists(pa)
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(l) for l in lists])
    t, cw, ch = c["crop"]
    g = {"params": np.array([c["views"], c["width"], c["height"], inp.level, inp.csize, inp.num_targets, t, cw, ch,
                             inp.min_image_num, n_plain], np.int64),
         "widths": w, "heights": h, "grid_dims": np.stack([gw, gh], 1).astype(np.int32),
         "coords": coords, "normal": pa["normal"], "ncc": pa["ncc"], "dscale": pa["dscale"],
         "ascale": pa["ascale"], "timages": pa["timages"].astype(np.int16), "fix": pa["fix"].astype(np.int8), "list_off": off, "lists": np.concatenate(lists).astype(np.int16),
         "copies": pairs, "count_ops": np.int64(len(c["count_ops"]))}
    rng = np.random.default_rng(c["seed"] + 1)
    for j, (depth, cthr, k) in enumerate(c["count_ops"]):
        calls = filter_pin_count_calls(rng, lists, gw, gh, len(inp.images), inp.num_targets, depth, k)
        g[f"c{j}_params"] = np.array([depth, cthr], np.int32)
        g[f"c{j}_kinds"] = np.array([x[0] for x in calls], np.int8)
        for name, col in (("i", 1), ("v", 2)):
            lo = np.zeros(len(calls) + 1, np.int32)
            lo[1:] = np.cumsum([len(x[col]) for x in calls])
            g[f"c{j}_{name}off"] = lo
            g[f"c{j}_{name}lists"] = np.array([e for x in calls for e in x[col]], np.int16).reshape(-1, 3)
    ops = filter_pin_ops(g)
    ref = O.ref_filter(inp.projections, w, h, inp.num_targets, inp.level, inp.csize, inp.min_image_num, coords, lists,
                       ops)
    o.close()
    if ref is None:
        raise SystemExit("oracle/_ref/filter not built (reference absent)")
    for k, v in ref[0].items():
        g["ref_dm_" + k] = v
    for j in range(len(c["count_ops"])):
        g[f"c{j}_ret"] = ref[1 + j]["ret"].astype(np.int8)
        g[f"c{j}_counts"] = ref[1 + j]["counts"].astype(np.uint8)
    filter_pin_coverage(g)
    path = os.path.join(HERE, "filter_pin.npz")
    save_npz(path, g)
    win = g["ref_dm_winner"]
    print(f"{path}: {os.path.getsize(path)} B, {len(coords)} patches, {(win >= 0).sum()} of {len(win)} cells filled by "
          f"{len(np.unique(win[win >= 0]))} winners, {len(g['ref_dm_vlists'])} vimages")


def make(name, views, width, height, level, csize, ntex, neval, nref):
    inp, p = P.synth_scene(views, width, height, level=level, csize=csize, supersample=2)
    o = O.OracleScene(inp)
    maxlv = level + 3
    g = {"params": np.array([views, width, height, level, csize], np.int64),
         "projections": inp.projections.astype(np.float32),
         "image_crc": np.array([zlib.crc32(im.tobytes()) for im in inp.images], np.uint32)}
    g["pyramid_crc"] = np.array([[zlib.crc32(o.get_level(v, lv).tobytes()) for lv in range(maxlv)]
                                 for v in range(views)], np.uint32)
    g["ref_camera"] = ref_cameras(inp.projections, maxlv, maxlv)
    rng = np.random.default_rng(7)
    pts = np.concatenate([rng.normal(0, 1.0, (200, 3)), np.ones((200, 1))], 1).astype(np.float32)
    pts[150:, 3] = 0.0  # directions (w = 0): the paxes / ray projections
    pts[140:150, :3] *= 50.0  # far and behind-camera points
    g["proj_points"] = pts
    g["ref_project"] = ref_project(inp.projections, maxlv, level, pts)
    g["ref_depth"] = ref_depth(inp.projections, maxlv, pts)
    g["color_xy"], g["ref_color"] = ref_colors(o, views, maxlv)

    tc = P.synth_candidates(p, inp.projections, ntex, seed=101)
    tq = pmvs_cases.tex_queries(o, views, tc)
    tex, valid = o.grab_tex(tq)
    g["tex_query"], g["tex"], g["tex_valid"] = tq, tex, valid

    ec = P.synth_candidates(p, inp.projections, neval, seed=102)
    eq = pmvs_cases.eval_queries(views, ec, per=4, nimg=min(6, views))
    f, enc = o.incc_eval(eq, want_encode=True)
    g["eval_query"], g["eval_f"], g["eval_encode"] = eq, f, enc

    rc = P.synth_candidates(p, inp.projections, nref, seed=103)
    out, st = o.refine_batch(rc, nthreads=8)
    g["refine_in"], g["refine_out"] = rc, out
    g["refine_stats"] = np.array([st[k] for k in ("accepted", "fail_pre", "fail_post", "refine_failed",
                                                  "evals", "tex_valid")], np.int64)
    o.close()
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **g)
    print(f"{path}: {os.path.getsize(path)} B, accepted {st['accepted']}/{nref}, "
          f"valid tex {int(valid.sum())}/{len(tq)}, f<2 {(f < 2).sum()}/{len(eq)}")


if __name__ == "__main__":
    O.build()
    if len(sys.argv) > 1:  # named fixtures only, e.g. `make_golden.py organizer`
        for name in sys.argv[1:]:
            globals()["make_" + name]()
        raise SystemExit(0)
    make_organizer()
    make_filter()
    make_isneighbor()
    make_expand_dirs()
    make_features()
    make_seeds()
    for k, v in SCENES.items():
        make(k, *v)
