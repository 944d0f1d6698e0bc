"""CPU tests of the device text export's boundary and of its number formatter (csrc/pmvs_fmt.h, one
source for host and device): the new entry points are exported, the PMVS_TEXT_* constants agree with the
header, argument checks that need no device answer PMVS_EINVAL, and pmvs_selftest_format on the host
(device = -1) gives, byte for byte, printf("%.{p}g") of every value of the number set at precision 6
and 17 -- random bit patterns, every exponent field, the round-half-even ties of both precisions, and
zeros, infinities, NaNs, denormals and the notation thresholds."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from text_cases import SPECIALS, expected, number_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stdio.h>
#include "pmvs_amd.h"
int main(void) {
  printf("ply %d\npatch %d\npset %d\n", PMVS_TEXT_PLY, PMVS_TEXT_PATCH, PMVS_TEXT_PSET);
  return 0;
}
"""


def test_text_symbols_exported(product_lib):
    import pmvs_amd as P
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cmvs-pmvs_amd", "libpmvs_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for sym in ("pmvs_loop_text", "pmvs_text_patches", "pmvs_selftest_format"):
        assert sym in exported and sym in P.EXPORTS, sym


def test_text_constants_match_c(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    import pmvs_amd as P
    assert (P.TEXT_PLY, P.TEXT_PATCH, P.TEXT_PSET) == (int(c["ply"]), int(c["patch"]), int(c["pset"]))


def test_text_rejects_bad_arguments(product_lib):
    lib = product_lib
    import pmvs_amd as P
    size = C.c_int64(-1)
    fake = C.c_void_p(1)  # a scene handle that is not null is not looked at before the check fails
    buf = (C.c_char * 8)()
    # a NULL scene
    assert lib.pmvs_loop_text(None, P.TEXT_PLY, 0, None, None, 0, C.byref(size)) == 1
    assert lib.pmvs_text_patches(None, None, 0, P.TEXT_PLY, 0, None, None, 0, C.byref(size)) == 1
    assert lib.pmvs_last_error()
    # a NULL bytes
    assert lib.pmvs_loop_text(fake, P.TEXT_PLY, 0, None, None, 0, None) == 1
    assert lib.pmvs_text_patches(fake, None, 0, P.TEXT_PLY, 0, None, None, 0, None) == 1
    # a bad kind, a bad flag
    for kind, flags in ((3, 0), (-1, 0), (P.TEXT_PSET, 4), (P.TEXT_PATCH, 1 << 8)):
        assert lib.pmvs_loop_text(fake, kind, flags, None, None, 0, C.byref(size)) == 1, (kind, flags)
        assert lib.pmvs_text_patches(fake, None, 0, kind, flags, None, None, 0, C.byref(size)) == 1, (kind, flags)
    # a capacity without a buffer
    assert lib.pmvs_loop_text(fake, P.TEXT_PLY, 0, None, None, 8, C.byref(size)) == 1
    assert lib.pmvs_text_patches(fake, None, 0, P.TEXT_PLY, 0, None, None, 8, C.byref(size)) == 1
    # the formatter's self-test: precision 6 or 17 only, no NULL
    x, ln = np.ones(1, np.float32), np.zeros(1, np.int32)
    for prec in (0, 7, 9, 18):
        assert lib.pmvs_selftest_format(-1, prec, x.ctypes.data, 1, buf, ln.ctypes.data) == 1
    assert lib.pmvs_selftest_format(-1, 17, None, 1, buf, ln.ctypes.data) == 1
    assert lib.pmvs_selftest_format(-1, 17, x.ctypes.data, 1, None, ln.ctypes.data) == 1
    assert lib.pmvs_selftest_format(-1, 17, x.ctypes.data, 1, buf, None) == 1


def test_expected_bytes_of_known_values():
    """The oracle itself on values whose printf output is known."""
    x = np.array([0.100040435791015625, 100000.5, 100001.5, 999999.5, 1e-45, -1e-45], np.float32)
    assert expected(x, 17)[0] == b"0.10004043579101562"          # an 18-digit tie: to the even digit
    assert expected(x, 6)[1:4] == [b"100000", b"100002", b"1e+06"]
    assert expected(x, 17)[4:] == [b"1.4012984643248171e-45", b"-1.4012984643248171e-45"]
    assert expected(SPECIALS[:7], 6) == [b"0", b"-0", b"inf", b"-inf", b"nan", b"-nan", b"nan"]


@pytest.mark.parametrize("precision", [6, 17])
def test_format_number_set_on_host(product_lib, precision):
    import pmvs_amd as P
    x = number_set()
    assert len(x) > 1_160_000
    got = P.selftest_format(precision, x, device=-1)
    want = expected(x, precision)
    bad = [(hex(int(b)), g, w) for b, g, w in zip(x.view(np.uint32), got, want) if g != w]
    assert not bad, (len(bad), bad[:10])
    assert max(map(len, got)) == (23 if precision == 17 else 12)
