"""CPU test: the table of refine layouts (cmvs-pmvs_amd/csrc/pmvs_refine_layouts.h).  A stand-alone
program (tests/csrc/refine_layouts_test.cpp, built with g++ against the host stub of HIP) checks what
parse accepts, decodes and rejects and what resolve picks for every wsize and tau, also under
AddressSanitizer and UBSan; the set it prints must be the configs that have a bit-exact GPU case."""
import os
import subprocess

import pytest

from refine_configs import NEW_CONFIGS, REFINE_CONFIGS, RETIRED_CONFIG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path, name, flags):
    exe = tmp_path / name
    # tests/csrc first: its hip/hip_runtime.h stands in for HIP's
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "tests", "csrc"), "-I",
                    os.path.join(ROOT, "cmvs-pmvs_amd", "csrc"),
                    os.path.join(ROOT, "tests", "csrc", "refine_layouts_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""
    return r.stdout


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    return build_and_run(tmp_path_factory.mktemp("layouts"), "refine_layouts_test", ["-O1"])


def test_parse_and_resolve(output):
    assert output.startswith("accepted:")


def test_every_built_layout_has_a_gpu_case(output):
    built = [int(x) for x in output.split(":", 1)[1].split()]
    assert len(built) == len(set(built))
    assert set(built) == set(REFINE_CONFIGS) | set(NEW_CONFIGS)
    assert RETIRED_CONFIG not in built  # test_refine_configs_bit_exact runs it as an unsupported number


def test_clean_under_sanitizers(tmp_path, output):
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    assert build_and_run(tmp_path, "refine_layouts_test_san", flags) == output
