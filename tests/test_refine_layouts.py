"""CPU test: the table of refine layouts (cmvs-pmvs_amd/csrc/pmvs_refine_layouts.h).  A stand-alone
program (tests/csrc/refine_layouts_test.cpp, built with g++ against the host stub of HIP) checks what
parse accepts, decodes and rejects and what resolve picks for every wsize and tau, also under
AddressSanitizer and UBSan; the set it prints must be the configs that have a bit-exact GPU case, and the
kernels it resolves the GPU cases' (config, wsize, tau) triples to must be every kernel the launchers
build, each of them above tau = 8 too where it can hold more than 8 textures."""
import os
import subprocess

import pytest

from refine_configs import (EXISTING_TRIPLES, LANE_WSIZES, NEW_CONFIGS, REFINE_CONFIGS, RETIRED_CONFIG, SPLIT_WSIZES,
                            WAVE_WSIZES, envelope_triples)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name, flags):
    exe = tmp_path / name
    # tests/csrc first: its hip/hip_runtime.h stands in for HIP's
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "tests", "csrc"), "-I",
                    os.path.join(ROOT, "cmvs-pmvs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "refine_layouts_test.cpp"), "-o", str(exe)], check=True)
    return exe


def run(exe, args=()):
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""
    return r.stdout


def triple_args():
    return [f"{c}:{w}:{t}" for c, w, t in sorted(set(EXISTING_TRIPLES) | set(envelope_triples()))]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("layouts"), "refine_layouts_test", ["-O1"])


@pytest.fixture(scope="module")
def output(exe):
    return run(exe)


@pytest.fixture(scope="module")
def resolved(exe):
    return run(exe, triple_args())


def test_parse_and_resolve(output):
    assert output.startswith("accepted:")


def test_every_built_layout_has_a_gpu_case(output):
    built = [int(x) for x in output.split(":", 1)[1].split()]
    assert len(built) == len(set(built))
    assert set(built) == set(REFINE_CONFIGS) | set(NEW_CONFIGS)
    assert RETIRED_CONFIG not in built  # test_refine_configs_bit_exact runs it as an unsupported number


def kernel_name(config, wsize):
    if config >= 300000:
        return f"lane<{wsize},{config - 300000}>"
    if config >= 200000:
        return f"split<{wsize},{config}>"
    return f"v2<{wsize},{config // 100},{config % 100}>"


def test_every_built_kernel_has_a_gpu_case(output, resolved):
    """A layout number is not a kernel: the launchers expand every layout over their wsize switch, and the
    same kernel takes other paths above tau = 8.  The GPU cases' triples, resolved by the table itself, must
    launch exactly the built kernels, and reach each of them above tau = 8 where it can hold that."""
    layouts = [int(x) for x in output.split(":", 1)[1].split()]  # 300000 is no layout: "lanes from tau"
    lane = [c for c in layouts if c > 300000]
    split = [c for c in layouts if 200000 <= c < 300000]
    wave = [c for c in layouts if c < 200000]
    assert lane and split and wave
    built = ({(c, w) for c in lane for w in LANE_WSIZES} | {(c, w) for c in wave for w in WAVE_WSIZES}
             | {(c, w) for c in split for w in SPLIT_WSIZES})

    ran = {}  # (resolved config, wsize) -> the taus it runs at
    lines = resolved.splitlines()
    assert len(lines) == len(triple_args())
    for line in lines:
        asked, arrow, got = line.partition(" -> ")
        config, wsize, tau = (int(x) for x in asked.split())
        rconfig, grid_div = (int(x) for x in got.split())
        assert arrow and grid_div in (1, 2)
        ran.setdefault((rconfig, wsize), set()).add(tau)

    missing = sorted(kernel_name(c, w) for c, w in built - set(ran))
    assert not missing, f"built kernels no GPU case launches: {missing}"
    extra = sorted(kernel_name(c, w) for c, w in set(ran) - built)
    assert not extra, f"GPU cases resolve to kernels the launchers do not build: {extra}"

    def above8(config, wsize, upto=16):
        assert any(8 < t <= upto for t in ran[(config, wsize)]), \
            f"{kernel_name(config, wsize)} has no GPU case at 8 < tau <= {upto}"

    # what can hold more than 8 textures per request: 4 lanes per texture, 12 and 24 texture slots, every
    # split layout (CG * 16 slots per group)
    for c in split:
        above8(c, 7)
    above8(1206, 7, upto=12)
    for w in (5, 7, 9):
        above8(300004, w)
        above8(2408, w)


def test_clean_under_sanitizers(tmp_path, output, resolved):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    san = build(tmp_path, "refine_layouts_test_san", flags)
    assert run(san) == output
    assert run(san, triple_args()) == resolved
