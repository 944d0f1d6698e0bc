"""GPU parity of every refine kernel the launchers build, over the envelope pmvs_scene_create accepts:
wsize 5, 7 and 9 and tau = min(2 * minImageNum, views) up to 16 (tests/refine_configs.py ENVELOPE).  The
other refine tests run wsize 7 at tau 6; here the split and wavefront forms run at wsize 5, and every form
runs above tau = 8, where the lane form puts textures 9-16 on lanes 32-63 and the split form packs requests
of up to 16 textures into its chunks.  Every record and the six counters against the CPU oracle, bit for
bit; tests/test_refine_layouts.py::test_every_built_kernel_has_a_gpu_case keeps the case table complete."""
import pytest
import torch  # before libpmvs_amd.so is loaded (see test_gpu_loop_export.py); _size reads the CU count from it

from conftest import small_scene
from refine_configs import (ENVELOPE, ENVELOPE_DEFAULT_LARGE_N, ENVELOPE_DEFAULT_SMALL_N, ENVELOPE_HIGH_TAU,
                            ENVELOPE_SCENES, ENVELOPE_SEED)
from test_gpu_parity import compare_refined
from test_gpu_refine_fallbacks import COUNTERS, LAYOUT_VARS

pytestmark = pytest.mark.gpu

MIN_SHARE = 0.45  # of the candidates the oracle must accept: the comparison is of refined patches


def _size(config, n):
    if n != "full":
        return n
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * ((config // 1000) % 10) * (config % 1000) + 777


class _Holder:
    """One envelope scene, its largest candidate set (the smaller batches are prefixes) and the oracle's
    result per batch size, computed once."""

    def __init__(self, oracle_mod, name):
        import pmvs_amd as P
        sc = ENVELOPE_SCENES[name]
        self.inp, self.p = small_scene(sc["views"], *sc["size"], level=1, **sc["kw"])
        assert self.inp.wsize == sc["wsize"]
        assert min(2 * self.inp.min_image_num, len(self.inp.images)) == sc["tau"]
        self.o = oracle_mod.OracleScene(self.inp)
        nmax = max([_size(c, n) for s, c, n in ENVELOPE if s == name] + [ENVELOPE_DEFAULT_LARGE_N])
        self.cands = P.synth_candidates(self.p, self.inp.projections, nmax, seed=ENVELOPE_SEED)
        self.ref = {}

    def oracle(self, n):
        if n not in self.ref:
            self.ref[n] = self.o.refine_batch(self.cands[:n], nthreads=16)
        return self.ref[n]


@pytest.fixture(scope="module")
def holders(gpu_available, oracle_mod):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _Holder(oracle_mod, name)
        return made[name]

    yield get
    for h in made.values():
        h.o.close()


def check(h, n):
    """A scene made now (it reads the layout variables) against the oracle on the first n candidates."""
    import pmvs_amd as P
    g = P.Scene(h.inp)
    try:
        rg, sg = g.refine_batch(h.cands[:n])
    finally:
        g.close()
    ro, so = h.oracle(n)
    assert so["accepted"] >= MIN_SHARE * n, (n, so["accepted"])
    compare_refined(rg, ro)
    for k in COUNTERS:
        assert sg[k] == so[k], (n, k)


@pytest.mark.parametrize("scene,config,n", ENVELOPE, ids=[f"{s}-{c}-{n}" for s, c, n in ENVELOPE])
def test_refine_envelope_bit_exact(holders, monkeypatch, scene, config, n):
    """PMVS_REFINE_CONFIG = config for every batch size on the scene: the kernel resolve() picks for the
    scene's wsize and tau gives the oracle's records."""
    for v in LAYOUT_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("PMVS_REFINE_CONFIG", str(config))
    check(holders(scene), _size(config, n))


@pytest.mark.parametrize("scene", ENVELOPE_HIGH_TAU)
def test_default_small_batch_above_tau8(holders, monkeypatch, scene):
    """Nothing set, 300 candidates: the lane form with the lanes per texture it takes from tau, as every
    loop wave and seed round of a scene with minImageNum >= 5 runs it."""
    for v in LAYOUT_VARS:
        monkeypatch.delenv(v, raising=False)
    check(holders(scene), ENVELOPE_DEFAULT_SMALL_N)


@pytest.mark.parametrize("scene", ENVELOPE_HIGH_TAU)
def test_default_large_layout_above_tau8(holders, monkeypatch, scene):
    """Only PMVS_REFINE_SMALL_N = 0: the default large layout, as a scene of this tau runs it at size."""
    for v in LAYOUT_VARS:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("PMVS_REFINE_SMALL_N", "0")
    check(holders(scene), ENVELOPE_DEFAULT_LARGE_N)
