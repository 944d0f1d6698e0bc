"""CPU test: CallArena and Staging (cmvs-pmvs_amd/csrc/pmvs_devbuf.h), the call-scoped device memory and
the output staging of the model-output calls, against a host stub of the HIP calls they make
(tests/csrc/hip/hip_runtime.h): host mode allocates max(count, 1) elements and copies back, device mode
passes the caller's pointer through without an allocation, a NULL array stays NULL, a partial copy-back
copies exactly the written prefix, a failed allocation returns its error with nothing leaked, nothing is
live at exit, and the PMVS_POISON_ALLOC fill.  A stand-alone program (tests/csrc/staging_test.cpp), run as
a child process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def staging_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("staging") / "staging_test"
    # tests/csrc first: its hip/hip_runtime.h stands in for HIP's
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "csrc"), "-I",
                    os.path.join(ROOT, "cmvs-pmvs_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "staging_test.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def run(exe, args, poison):
    env = {k: v for k, v in os.environ.items() if k != "PMVS_POISON_ALLOC"}
    if poison is not None:
        env["PMVS_POISON_ALLOC"] = str(poison)
    r = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("staging ok")


def test_staging(staging_exe):
    run(staging_exe, [], None)


def test_staging_poison(staging_exe):
    run(staging_exe, ["poison"], 165)
