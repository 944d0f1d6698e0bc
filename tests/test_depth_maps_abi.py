"""CPU tests of the depth-map entry points' boundary: the ctypes mirror of pmvs_depthmap_buffers has
the C compiler's layout, the argument checks that need no device answer PMVS_EINVAL, and
pmvs_write_pfm writes the bytes a numpy restatement of the format gives."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "pmvs_amd.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("pmvs_depthmap_buffers.sizeof %zu\n", sizeof(pmvs_depthmap_buffers));
  F(pmvs_depthmap_buffers, patch); F(pmvs_depthmap_buffers, depth); F(pmvs_depthmap_buffers, normal);
  F(pmvs_depthmap_buffers, ncc);
  return 0;
}
"""


def test_depthmap_struct_matches_c(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    import pmvs_amd as P
    T, name = P.DepthMapBuffers, "pmvs_depthmap_buffers"
    assert C.sizeof(T) == int(c[name + ".sizeof"])
    for f, _ in T._fields_:
        assert getattr(T, f).offset == int(c[f"{name}.{f}"]), f
    assert [f for f, _ in T._fields_] == list(P.Scene.DEPTH_MAP_ARRAYS)


def test_depth_maps_reject_null_arguments(product_lib):
    lib = product_lib
    import pmvs_amd as P
    buf = P.DepthMapBuffers()
    dims, off = np.zeros(2, np.int32), np.zeros(2, np.int64)
    assert lib.pmvs_depth_map_layout(None, dims.ctypes.data, off.ctypes.data) == 1
    assert lib.pmvs_loop_depth_maps(None, 0, C.byref(buf)) == 1
    assert lib.pmvs_depth_maps_patches(None, None, 0, 0, C.byref(buf)) == 1
    assert lib.pmvs_last_error()
    # null buffers: a scene handle that is not null is not looked at before the check fails
    fake = C.c_void_p(1)
    assert lib.pmvs_loop_depth_maps(fake, 0, None) == 1
    assert lib.pmvs_depth_maps_patches(fake, None, 0, 0, None) == 1


def pfm_bytes(a):
    """The format restated: header, then the rows bottom to top as little-endian float32."""
    h, w = a.shape
    return b"Pf\n%d %d\n-1.0\n" % (w, h) + a[::-1].astype("<f4").tobytes()


def test_write_pfm_bytes(product_lib, tmp_path):
    import pmvs_amd as P
    a = np.array([[0.0, -2.5, 1e-40], [3.25, 7.0, 1234.5]], np.float32)  # 3 wide, 2 high; 1e-40 is a denormal
    assert a.shape == (2, 3) and 0 < a[0, 2] < np.finfo(np.float32).tiny
    path = str(tmp_path / "a.pfm")
    P.write_pfm(path, a)
    got = open(path, "rb").read()
    assert got == pfm_bytes(a)
    assert got.startswith(b"Pf\n3 2\n-1.0\n") and len(got) == 12 + 4 * 6


def test_write_pfm_rejects_bad_arguments(product_lib, tmp_path):
    lib = product_lib
    a = np.zeros(6, np.float32)
    path = str(tmp_path / "b.pfm").encode()
    assert lib.pmvs_write_pfm(None, 3, 2, a.ctypes.data) == 1
    assert lib.pmvs_write_pfm(path, 0, 2, a.ctypes.data) == 1
    assert lib.pmvs_write_pfm(path, 3, 0, a.ctypes.data) == 1
    assert lib.pmvs_write_pfm(path, -3, 2, a.ctypes.data) == 1
    assert lib.pmvs_write_pfm(path, 3, 2, None) == 1
    assert not os.path.exists(path)
