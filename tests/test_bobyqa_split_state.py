"""CPU test: bobyqa_dev.h's state machine with its state in two parts -- the hot part (BqHot, what the
split-form refine kernel keeps in LDS) and the cold part (BqCold, what only PRELIM, RESCUE and the
exits touch) in separate allocations -- takes the trajectory of the one-object layout (BqState),
bit for bit: result code, every evaluation point and value, the final point and the minimum.

The starts are test_lane_bobyqa_matches_state_machine's 1 230 (ten objective kinds, maxeval
1000 / 40 / 13).  The lane form's host build runs them too, because its hit counters say which
branches these trajectories take: RESCUE, its den2 retry, the xbase shift and the XTOL exit must
have run, otherwise the cold fields were never exercised."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cmvs-pmvs_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "csrc", "bq_split_host.cpp")
MAXREC = 1024

RUN_ARGS = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]


@pytest.fixture(scope="module")
def bqsplit(tmp_path_factory):
    so = tmp_path_factory.mktemp("bqs") / "libbqsplit.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    L.bq_embed_run.argtypes = RUN_ARGS
    L.bq_split_run.argtypes = RUN_ARGS
    return L


@pytest.fixture(scope="module")
def bqlhost(tmp_path_factory):
    so = tmp_path_factory.mktemp("bql") / "libbqlhost.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                    "-DBQL_COUNT", "-I", CSRC, os.path.join(ROOT, "tests", "csrc", "bql_host.cpp"), "-o", str(so)],
                   check=True)
    L = C.CDLL(str(so))
    L.bql_host_run.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                               C.POINTER(C.c_int)]
    L.bql_host_hits.restype = C.POINTER(C.c_longlong)
    return L


def run(fn, kind, x0, maxeval):
    x0 = np.ascontiguousarray(x0, np.float64)
    xo, fo, pts, rec, n = np.zeros(3), np.zeros(1), np.zeros((MAXREC, 3)), np.zeros(MAXREC), C.c_int()
    rc = fn(kind, x0.ctypes.data, maxeval, xo.ctypes.data, fo.ctypes.data, pts.ctypes.data, rec.ctypes.data, MAXREC,
            C.byref(n))
    assert n.value <= MAXREC
    return rc, xo, fo, pts[:n.value], rec[:n.value]


def run_lane(L, kind, x0, maxeval):
    x0 = np.ascontiguousarray(x0, np.float64)
    xo, fo, rec, n = np.zeros(3), np.zeros(1), np.zeros(MAXREC), C.c_int()
    rc = L.bql_host_run(kind, x0.ctypes.data, maxeval, xo.ctypes.data, fo.ctypes.data, rec.ctypes.data, MAXREC,
                        C.byref(n))
    return rc, xo, fo, rec[:n.value]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def test_split_state_matches_one_object_state(bqsplit, bqlhost):
    hits0 = [bqlhost.bql_host_hits()[i] for i in range(11)]
    n = 0
    for kind in range(10):
        for maxeval in (1000, 40, 13):
            rng = np.random.default_rng(kind * 1000 + maxeval)
            starts = np.concatenate([[[0.0, 0.0, 0.0]], rng.normal(0, [3.0, 8.0, 8.0], (40, 3))])
            starts[:, 1:] = np.clip(starts[:, 1:], -23.99999, 23.99999)
            for x0 in starts:
                a = run(bqsplit.bq_embed_run, kind, x0, maxeval)
                b = run(bqsplit.bq_split_run, kind, x0, maxeval)
                assert a[0] == b[0], (kind, maxeval, x0, a[0], b[0])
                assert len(a[3]) == len(b[3]) <= maxeval, (kind, maxeval, x0)
                for i, what in ((1, "final point"), (2, "minimum"), (3, "evaluation points"), (4, "values")):
                    assert same(a[i], b[i]), (what, kind, maxeval, x0)
                # the lane form on the same start: its counters below are of these trajectories
                c = run_lane(bqlhost, kind, x0, maxeval)
                assert c[0] == b[0] and same(c[1], b[1]) and same(c[2], b[2]) and same(c[3], b[4]), (kind, maxeval, x0)
                n += 1
    assert n == 10 * 3 * 41
    hits = [bqlhost.bql_host_hits()[i] - hits0[i] for i in range(11)]
    # [0] RESCUE, [1] xbase shift, [4] RESCUE's den2 retry, [5] RESCUE evaluations, [8] XTOL exit
    for i in (0, 1, 4, 5, 8):
        assert hits[i] > 0, (i, hits)


def test_split_state_under_sanitizers(tmp_path):
    """The stand-alone comparison program (bq_split_host.cpp with its own main: 360 starts in both
    layouts, the two parts in heap blocks of exactly their sizes, filled with a pattern first) built with
    the address and undefined-behaviour sanitizers.  The array-bounds check is left out: the header's
    1-based views of Powell's matrices address a row's element BQN, which is the next row's first, on
    purpose and in either layout; every address is still checked by the address sanitizer."""
    exe = tmp_path / "bq_split_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize=bounds", "-fno-sanitize-recover=undefined", "-DBQ_SPLIT_MAIN", "-I", CSRC, SRC,
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "360 runs" in r.stdout and "layouts equal" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
