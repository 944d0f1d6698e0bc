"""GPU parity of the refine launcher's fallback rules (pmvs_refine_layouts.h resolve) through the real
entry, pmvs_refine_batch: a split-form layout at wsize 9 runs the wavefront form 1206, and a wavefront
layout with fewer texture slots than tau runs 2408 on half the grid.  Records and the six counters
against the CPU oracle, as in test_gpu_parity.py::test_refine_configs_bit_exact.  (The lane form's
choice of lanes per texture at tau <= 8 is what every small batch of the other tests runs; above tau = 8,
where it takes 4 lanes per texture, and every other form above tau = 8 and at wsize 5 and 9:
test_gpu_refine_envelope.py.)"""
import pytest

from conftest import small_scene
from test_gpu_parity import compare_refined

pytestmark = pytest.mark.gpu

COUNTERS = ("accepted", "fail_pre", "fail_post", "refine_failed", "evals", "tex_valid")
LAYOUT_VARS = ("PMVS_REFINE_CONFIG", "PMVS_REFINE_LARGE_CONFIG", "PMVS_REFINE_SMALL_CONFIG", "PMVS_REFINE_SMALL_N")


def check(inp, p, oracle_mod, batches, min_share=None):
    import pmvs_amd as P
    g = P.Scene(inp)  # reads the layout variables
    o = oracle_mod.OracleScene(inp)
    try:
        for n, seed in batches:
            cands = P.synth_candidates(p, inp.projections, n, seed=seed)
            rg, sg = g.refine_batch(cands)
            ro, so = o.refine_batch(cands, nthreads=8)
            if min_share is not None:
                assert so["accepted"] >= min_share * n, (n, so["accepted"])
            compare_refined(rg, ro)
            for k in COUNTERS:
                assert sg[k] == so[k], (n, k)
    finally:
        g.close()
        o.close()


def test_split_layout_at_wsize9_runs_wavefront_form(gpu_available, oracle_mod, monkeypatch):
    """Every batch on the default large layout (split form), which wsize 9 turns into 1206."""
    for v in LAYOUT_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("PMVS_REFINE_SMALL_N", "0")
    inp, p = small_scene(8, 480, 360, level=1, wsize=9)
    check(inp, p, oracle_mod, ((3000, 21), (5, 22)))


def test_wavefront_layout_below_tau_runs_2408(gpu_available, oracle_mod, monkeypatch):
    """16 views 6 degrees apart with minImageNum 7: tau = 14 > 1206's 12 texture slots.  The scene was
    picked on the CPU so that the oracle accepts well over a quarter of the candidates (246 of 400)."""
    for v in LAYOUT_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("PMVS_REFINE_CONFIG", "1206")
    inp, p = small_scene(16, 320, 240, level=1, arc_step_deg=6.0, min_image_num=7)
    assert min(2 * inp.min_image_num, len(inp.images)) >= 13
    check(inp, p, oracle_mod, ((400, 41),), min_share=0.25)
