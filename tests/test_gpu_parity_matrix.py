"""GPU parity across the option space the reference exposes for this path (option.cpp keys
level / csize / wsize / minImageNum / threshold / maxAngle / sequence / timages+oimages /
useVisData / bimages, plus masks/ and edges/): for every configuration the HIP refine batch,
grabTex and my_f equal the CPU oracle bit-for-bit."""
import numpy as np
import pytest

from pmvs_cases import bits, eval_queries, tex_queries

pytestmark = pytest.mark.gpu


def blob_masks(num, h, w, seed, keep=0.85):
    """Binary images (0/255) with random rectangular holes (for masks/ and edges/)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num):
        m = np.full((h, w), 255, np.uint8)
        area = 0
        while area < (1 - keep) * h * w:
            y0, x0 = rng.integers(0, h), rng.integers(0, w)
            hh, ww = rng.integers(h // 20 + 1, h // 5 + 2), rng.integers(w // 20 + 1, w // 5 + 2)
            m[y0:y0 + hh, x0:x0 + ww] = 0
            area = int((m == 0).sum())
        out.append(m)
    return out


CONFIGS = {
    "level0_w5_c1": dict(views=6, w=320, h=240, level=0, opts=dict(csize=1, wsize=5)),
    "level2_w9_c4_min2": dict(views=6, w=640, h=480, level=2, opts=dict(csize=4, wsize=9, min_image_num=2)),
    "masks_edges_bimages": dict(views=8, w=480, h=360, level=1, masks=True, edges=True,
                                opts=dict(bindexes=(0, 2, 5))),
    "targets_vis_seq_angle": dict(views=8, w=480, h=360, level=1, targets=4,
                                  opts=dict(sequence=3, max_angle_deg=25.0, threshold=0.6),
                                  vis="ring2"),
    "min4_thr08": dict(views=10, w=400, h=300, level=1, opts=dict(min_image_num=4, threshold=0.8)),
    # tau = min(2 * minImageNum, views) above 8: image selection, set_scales, the expand and filter stages
    # and the seed phase with more than 8 images per patch (views `arc` degrees apart)
    "min7_v16": dict(views=16, w=320, h=240, level=1, arc=6.0, opts=dict(min_image_num=7)),
    "min5_v9_w5": dict(views=9, w=320, h=240, level=1, arc=8.0, opts=dict(min_image_num=5, wsize=5)),
    # photometrically hard scenes (per-view gain/bias, sensor noise, low-texture regions, an occluder):
    # final NCCs spread over ~0.6-1 and image selection / filterOutside decisions sit near their thresholds
    "hard_level0": dict(views=10, w=400, h=300, level=0, hard=True),
    "hard_level1_masks": dict(views=8, w=480, h=360, level=1, hard=True, masks=True, edges=True,
                              opts=dict(threshold=0.6)),
}
# near-threshold decisions a hard loop must make (constraintImages within 0.02 of 1 - threshold,
# filterOutside gains within 0.05 of 0); the level-1 masked scene has fewer patches
HARD_NEAR_MIN = {"hard_level0": {"constraint_near": 20, "gains_near": 2},
                 "hard_level1_masks": {"constraint_near": 10, "gains_near": 0}}


def build(cfg):
    import pmvs_amd as P
    inp, p = P.synth_scene(cfg["views"], cfg["w"], cfg["h"], level=cfg["level"], num_targets=cfg.get("targets"),
                           supersample=2, hard=cfg.get("hard", False), arc_step_deg=cfg.get("arc"),
                           **cfg.get("opts", {}))
    V = cfg["views"]
    if cfg.get("masks"):
        inp.masks = blob_masks(V, cfg["h"], cfg["w"], 1, keep=0.9)
    if cfg.get("edges"):
        inp.edges = blob_masks(V, cfg["h"], cfg["w"], 2, keep=0.8)
    if cfg.get("vis") == "ring2":
        inp.visdata2 = [[x for x in range(V) if x != y and min(abs(x - y), V - abs(x - y)) <= 2] for y in range(V)]
    return inp, p


@pytest.fixture(scope="module", params=sorted(CONFIGS), ids=sorted(CONFIGS))
def pair(request, gpu_available, oracle_mod):
    import pmvs_amd as P
    inp, p = build(CONFIGS[request.param])
    g = P.Scene(inp)
    o = oracle_mod.OracleScene(inp)
    yield request.param, inp, p, g, o
    g.close()
    o.close()


def test_refine_matrix(pair):
    import pmvs_amd as P
    name, inp, p, g, o = pair
    cands = P.synth_candidates(p, inp.projections, 300, seed=77)
    rg, sg = g.refine_batch(cands)
    ro, so = o.refine_batch(cands, nthreads=8)
    assert np.array_equal(rg["status"], ro["status"]), name
    acc = ro["status"] == 0
    for f in ("refine_code", "evals", "num_images", "timages"):
        assert np.array_equal(rg[f][acc], ro[f][acc]), (name, f)
    for f in ("coord", "normal", "ncc", "dscale", "ascale", "tmp"):
        assert np.array_equal(bits(rg[f][acc]), bits(ro[f][acc])), (name, f)
    for i in np.flatnonzero(acc):
        n = ro["num_images"][i]
        assert np.array_equal(rg["images"][i][:n], ro["images"][i][:n]), name
        assert np.array_equal(rg["grids"][i][:n], ro["grids"][i][:n]), name
    for k in ("accepted", "fail_pre", "fail_post", "refine_failed", "evals", "tex_valid", "tex_grabs"):
        assert sg[k] == so[k], (name, k)


def test_thresholds_matrix(pair):
    """updateThreshold-style changes (findMatch.cpp:23-28) take effect identically."""
    import pmvs_amd as P
    name, inp, p, g, o = pair
    cands = P.synth_candidates(p, inp.projections, 150, seed=78)
    for ncc, before in ((0.55, 0.45), (0.8, 0.7)):
        g.set_thresholds(ncc, before)
        o.set_thresholds(ncc, before)
        rg, sg = g.refine_batch(cands)
        ro, so = o.refine_batch(cands, nthreads=8)
        assert np.array_equal(rg["status"], ro["status"]), (name, ncc)
        assert sg["accepted"] == so["accepted"]
        acc = ro["status"] == 0
        assert np.array_equal(bits(rg["ncc"][acc]), bits(ro["ncc"][acc]))
    thr = inp.threshold
    g.set_thresholds(thr, thr - 0.1)
    o.set_thresholds(thr, thr - 0.1)


def test_grab_and_my_f_matrix(pair):
    import pmvs_amd as P
    name, inp, p, g, o = pair
    V = len(inp.images)
    cands = P.synth_candidates(p, inp.projections, 60, seed=79)
    tq = tex_queries(o, V, cands)
    tg, vg = g.grab_tex(tq)
    to, vo = o.grab_tex(tq)
    assert np.array_equal(vg, vo) and np.array_equal(bits(tg), bits(to)), name
    eq = eval_queries(V, cands, per=3, nimg=min(6, V))
    fg, _ = g.incc_eval(eq)
    fo = o.incc_eval(eq)
    assert np.array_equal(bits(fg), bits(fo)), name
    tau = min(2 * inp.min_image_num, V)
    if tau > 6:  # my_f over as many images as a patch of this scene holds
        eq = eval_queries(V, cands, per=3, nimg=min(tau, V))
        fg, _ = g.incc_eval(eq)
        fo = o.incc_eval(eq)
        assert (fo < 2.0).any(), name  # some query has enough valid textures for a value
        assert np.array_equal(bits(fg), bits(fo)), (name, tau)


def test_empty_and_invalid_batches(gpu_available):
    import pmvs_amd as P
    inp, p = P.synth_scene(4, 160, 120, level=1)
    g = P.Scene(inp)
    out, st = g.refine_batch(np.zeros(0, P.CANDIDATE_DTYPE))
    assert len(out) == 0 and st["accepted"] == 0
    bad = P.synth_candidates(p, inp.projections, 4, seed=1)
    bad["images"][2][1] = 99  # image index out of range -> PMVS_EINVAL, nothing launched
    with pytest.raises(P.PmvsError):
        g.refine_batch(bad)
    bad = P.synth_candidates(p, inp.projections, 4, seed=1)
    bad["num_images"][0] = 0
    with pytest.raises(P.PmvsError):
        g.refine_batch(bad)
    g.close()


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_full_loop_matrix(gpu_available, oracle_mod, name):
    """The whole expand/filter loop (pmvs_run_loop, CFindMatch::run after the seeds) under every
    option configuration above -- masks, edges, bimages, visdata, timages subsets, sequence,
    maxAngle, csize 1/4, wsize 5/9, levels 0-2, minImageNum 2/4/5/7 -- equals the oracle's loop
    patch for patch (wave 128, min_candidates 256)."""
    import pmvs_amd as P
    inp, p = build(CONFIGS[name])
    g = P.Scene(inp)
    o = oracle_mod.OracleScene(inp)
    cands = P.synth_candidates(p, inp.projections, 150, seed=21)
    r, _ = g.refine_batch(cands)
    seeds = P.patches_from_refined(r)
    out_g, log_g = g.run_loop(seeds, inp.threshold, wave=128, min_candidates=256)
    oracle_mod.near_threshold(reset=True)
    out_o, log_o = o.run_loop(seeds, inp.threshold, wave=128, min_candidates=256)
    near = oracle_mod.near_threshold(reset=True)
    g.close()
    o.close()
    print(f"{name}: {[it['patches'] for it in log_o]} patches, ncc p1/p50 "
          f"{np.percentile(out_o['ncc'], [1, 50]).round(3).tolist()}, near-threshold decisions {near}")
    assert len(seeds) > 0 and len(out_o) > len(seeds)
    for a, b in zip(log_g, log_o):
        assert a["patches"] == b["patches"], (a, b)
        assert {k: v for k, v in a["expand"].items() if k not in P.ExpandStats.WORK} == b["expand"]
        assert [a["filter"][k] for k in ("removed_outside", "removed_exact", "removed_neighbor",
                                         "removed_groups")] == b["filter"]
    assert out_g.tobytes() == out_o.tobytes() or _same_patches(out_g, out_o)
    for k, v in HARD_NEAR_MIN.get(name, {}).items():  # the parity above is not vacuous near the thresholds
        assert near[k] >= v, (name, near)


def _same_patches(a, b):
    """Every defined field equal (image / vimage arrays compared up to their counts)."""
    if len(a) != len(b):
        return False
    for f in ("coord", "normal", "ncc", "dscale", "ascale", "tmp", "timages", "flag", "fix", "num_images",
              "num_vimages", "dflag"):
        if bits(a[f]).tobytes() != bits(b[f]).tobytes() if a[f].dtype.kind == "f" else not np.array_equal(a[f], b[f]):
            return False
    for i in range(len(a)):
        n, m = b["num_images"][i], b["num_vimages"][i]
        if not (np.array_equal(a["images"][i][:n], b["images"][i][:n]) and np.array_equal(a["grids"][i][:n], b["grids"][i][:n])
                and np.array_equal(a["vimages"][i][:m], b["vimages"][i][:m])
                and np.array_equal(a["vgrids"][i][:m], b["vgrids"][i][:m])):
            return False
    return True
