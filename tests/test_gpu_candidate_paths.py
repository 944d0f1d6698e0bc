"""GPU parity of the candidate kernels' image-selection paths around setRefImage (pre_kernel,
post_kernel, filter_refimage_kernel): refine_batch records and stats equal the CPU oracle's field
for field on scenes built to take the paths the small parity scenes do not --

  * more images than LDS texture slots (16): constraintImages in several batches, setRefImage's
    blocked pair matrix above 16 targets;
  * targets a strict subset of the views, so that setRefImage's target list skips list positions;
  * one filter pass: filterExact runs setRefImage on every patch it keeps, on the candidate
    kernels' grid.

Each scene's condition is checked on the oracle's output alone."""
import numpy as np
import pytest

from pmvs_cases import bits

pytestmark = pytest.mark.gpu

TEXCAP = 16  # LDS texture slots per wavefront (pmvs_layout.h)

CASES = {
    # a full ring with all-pairs visibility: up to 17 (64 views) / 26 (96 views) images per patch
    "ring64_level0_w7": dict(views=64, w=320, h=240, level=0, n=300, seed=77, opts=dict(wsize=7)),
    "ring96_level0_w7": dict(views=96, w=320, h=240, level=0, n=300, seed=77, opts=dict(wsize=7)),
    # ... and with 24 of the 64 views as targets
    "ring64_t24_w5": dict(views=64, targets=24, w=320, h=240, level=0, n=300, seed=79, opts=dict(wsize=5)),
    "ring64_t24_w7": dict(views=64, targets=24, w=320, h=240, level=0, n=300, seed=79, opts=dict(wsize=7)),
    "arc12_t5_w5": dict(views=12, targets=5, w=400, h=300, level=1, n=200, seed=78, opts=dict(wsize=5)),
    "arc12_t5_w7": dict(views=12, targets=5, w=400, h=300, level=1, n=200, seed=78, opts=dict(wsize=7)),
}


def refine_both(oracle_mod, cfg):
    import pmvs_amd as P
    inp, p = P.synth_scene(cfg["views"], cfg["w"], cfg["h"], level=cfg["level"], num_targets=cfg.get("targets"),
                           supersample=2, **cfg["opts"])
    cands = P.synth_candidates(p, inp.projections, cfg["n"], seed=cfg["seed"])
    g = P.Scene(inp)
    o = oracle_mod.OracleScene(inp)
    rg, sg = g.refine_batch(cands)
    ro, so = o.refine_batch(cands, nthreads=8)
    g.close()
    o.close()
    return rg, sg, ro, so


def assert_same_records(name, rg, sg, ro, so):
    assert np.array_equal(rg["status"], ro["status"]), name
    acc = ro["status"] == 0
    for f in ("refine_code", "evals", "num_images", "timages"):
        assert np.array_equal(rg[f][acc], ro[f][acc]), (name, f)
    for f in ("coord", "normal", "ncc", "dscale", "ascale", "tmp"):
        assert np.array_equal(bits(rg[f][acc]), bits(ro[f][acc])), (name, f)
    for i in np.flatnonzero(acc):
        n = ro["num_images"][i]
        assert np.array_equal(rg["images"][i][:n], ro["images"][i][:n]), (name, i)
        assert np.array_equal(rg["grids"][i][:n], ro["grids"][i][:n]), (name, i)
    for k in ("accepted", "fail_pre", "fail_post", "refine_failed", "evals", "tex_valid", "tex_grabs"):
        assert sg[k] == so[k], (name, k)


@pytest.mark.parametrize("name", ["ring64_level0_w7", "ring96_level0_w7"])
def test_more_images_than_texture_slots(gpu_available, oracle_mod, name):
    rg, sg, ro, so = refine_both(oracle_mod, CASES[name])
    ni = ro["num_images"][ro["status"] == 0]
    assert (ni > TEXCAP).sum() >= 10 and (ni <= TEXCAP).sum() >= 10, (name, np.bincount(ni).tolist())
    assert_same_records(name, rg, sg, ro, so)


@pytest.mark.parametrize("name", ["arc12_t5_w5", "arc12_t5_w7", "ring64_t24_w5", "ring64_t24_w7"])
def test_targets_strict_subset(gpu_available, oracle_mod, name):
    cfg = CASES[name]
    rg, sg, ro, so = refine_both(oracle_mod, cfg)
    acc = np.flatnonzero(ro["status"] == 0)
    nontarget = sum(bool((ro["images"][i][:ro["num_images"][i]] >= cfg["targets"]).any()) for i in acc)
    assert nontarget >= 10, (name, nontarget)
    assert_same_records(name, rg, sg, ro, so)


def test_filter_pass_set_ref_image(gpu_available, oracle_mod):
    """filterExact rebuilds every non-fixed patch's image list and, while it has minImageNum images,
    runs setRefImage + setGrids on it (filter.cpp:262-281): filter_refimage_kernel on pre / post's
    grid, thousands of patches, with a changed reference image in many."""
    import pmvs_amd as P
    from test_gpu_filter import compare, make_patch_set
    inp, p = P.synth_scene(6, 480, 360, level=1, supersample=2)
    g = P.Scene(inp)
    o = oracle_mod.OracleScene(inp)
    pa = make_patch_set(P, g, inp, p, 8000, 9)
    for sc in (g, o):
        sc.set_thresholds(inp.threshold, inp.threshold - 0.3, 1)
    out_g, keep_g, st_g = g.filter_run(pa)
    out_o, keep_o, counts_o = o.filter_run(pa)
    g.close()
    o.close()
    ran = (keep_o == 1) & (pa["fix"] == 0)  # kept and not fixed: went through setRefImage
    newref = ran & (out_o["images"][:, 0] != pa["images"][:, 0])
    assert ran.sum() >= 3000 and newref.sum() >= 100, (int(ran.sum()), int(newref.sum()))
    compare(out_g, keep_g, st_g, out_o, keep_o, counts_o)
