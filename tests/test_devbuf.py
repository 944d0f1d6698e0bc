"""CPU test: DevBuf<T>, the owner type of every device array of the loop
(cmvs-pmvs_amd/csrc/pmvs_devbuf.h), against a host stub of the HIP calls it makes
(tests/csrc/hip/hip_runtime.h): the capacities of its four (re)allocation forms, no reallocation at or
below the capacity, kept contents, moves, release, failed allocations, nothing live at exit, and the
PMVS_POISON_ALLOC fill.  A stand-alone program (tests/csrc/devbuf_test.cpp), run as a child process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def devbuf_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("devbuf") / "devbuf_test"
    # tests/csrc first: its hip/hip_runtime.h stands in for HIP's
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "csrc"), "-I",
                    os.path.join(ROOT, "cmvs-pmvs_amd", "csrc"), os.path.join(ROOT, "tests", "csrc", "devbuf_test.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def run(exe, args, poison):
    env = {k: v for k, v in os.environ.items() if k != "PMVS_POISON_ALLOC"}
    if poison is not None:
        env["PMVS_POISON_ALLOC"] = str(poison)
    r = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("devbuf ok")


def test_devbuf(devbuf_exe):
    run(devbuf_exe, [], None)


def test_devbuf_poison(devbuf_exe):
    run(devbuf_exe, ["poison"], 165)
