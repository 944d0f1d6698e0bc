"""GPU parity of the split-form refine layouts that hold 90-96 chains per CU (the optimizer's cold
state in global memory, bobyqa_dev.h BqCold): every record and the six counters against the CPU
oracle, at the batch sizes where the kernel takes another path, and the whole loop's digest against
the 84-chain layout's."""
import pytest
import torch  # before libpmvs_amd.so is loaded (see test_gpu_loop_export.py); _full reads the CU count from it

from conftest import small_scene
from refine_configs import NEW_CONFIGS
from test_gpu_parity import compare_refined

pytestmark = pytest.mark.gpu

COUNTERS = ("accepted", "fail_pre", "fail_post", "refine_failed", "evals", "tex_valid")
NMAX = 40000


class _Shared:
    """The small 8-view scene, one candidate set (its prefixes are the smaller batches) and the oracle's
    result per batch size, computed once."""

    def __init__(self, oracle_mod):
        import pmvs_amd as P
        self.inp, self.p = small_scene(8, 480, 360, level=1)
        self.o = oracle_mod.OracleScene(self.inp)
        self.cands = P.synth_candidates(self.p, self.inp.projections, NMAX, seed=31)
        self.ref = {}

    def oracle(self, n):
        if n not in self.ref:
            self.ref[n] = self.o.refine_batch(self.cands[:n], nthreads=8)
        return self.ref[n]


@pytest.fixture(scope="module")
def shared(gpu_available, oracle_mod):
    s = _Shared(oracle_mod)
    yield s
    s.o.close()


def _full(config):
    """Every lane 0..CG-1 of every workgroup holds a chain and is refilled at least once."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * ((config // 1000) % 10) * (config % 1000) + 777


@pytest.mark.parametrize("size", ["5", "full", "40000"])
@pytest.mark.parametrize("config", NEW_CONFIGS)
def test_split_chain_configs_bit_exact(shared, monkeypatch, config, size):
    """n = 5: fewer candidates than optimizer wavefronts; n = CUs * G * CG + 777: every chain slot of the
    grid in use; n = 40000: several refills and the final computeINCC (need == 2) under load."""
    import pmvs_amd as P
    n = _full(config) if size == "full" else int(size)
    assert 0 < n <= NMAX
    monkeypatch.setenv("PMVS_REFINE_CONFIG", str(config))
    g = P.Scene(shared.inp)
    try:
        rg, sg = g.refine_batch(shared.cands[:n])
    finally:
        g.close()
    ro, so = shared.oracle(n)
    assert so["accepted"] > n // 2
    compare_refined(rg, ro)
    for k in COUNTERS:
        assert sg[k] == so[k], (n, k)


@pytest.fixture(scope="module")
def loop_case(gpu_available):
    """A 1080p scene of test_gpu_loop_hash's size (6 views, 300 seed candidates, two iterations), and
    its loop digest with every batch on the 84-chain layout 226014."""
    import os
    import pmvs_amd as P
    inp, p = P.synth_scene(6, 1920, 1080, level=1, supersample=2)
    cands = P.synth_candidates(p, inp.projections, 300, seed=3)

    def digest(config):
        # PMVS_REFINE_SMALL_N = 0: the batches of this small loop run the large-batch layout too
        old = {k: os.environ.get(k) for k in ("PMVS_REFINE_LARGE_CONFIG", "PMVS_REFINE_SMALL_N")}
        os.environ["PMVS_REFINE_LARGE_CONFIG"] = str(config)
        os.environ["PMVS_REFINE_SMALL_N"] = "0"
        try:
            g = P.Scene(inp)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        try:
            r, _ = g.refine_batch(cands)
            seeds = P.patches_from_refined(r)
            n, log = g.run_loop(seeds, inp.threshold, iterations=2, wave=256, fetch=False)
            assert n == log[-1]["patches"] > 1000
            return n, g.loop_hash()
        finally:
            g.close()

    return digest, digest(226014)


@pytest.mark.parametrize("config", NEW_CONFIGS)
def test_loop_digest_equals_default_layout(loop_case, config):
    digest, ref = loop_case
    assert digest(config) == ref
