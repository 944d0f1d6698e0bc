"""CPU tests of the export entry points' boundary: the ctypes mirrors of pmvs_export_sizes and
pmvs_export_buffers have the C compiler's layout, the flag values agree with the header, and the
argument checks that need no device answer PMVS_EINVAL."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "pmvs_amd.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
  printf("pmvs_export_sizes.sizeof %zu\n", sizeof(pmvs_export_sizes));
  F(pmvs_export_sizes, patches); F(pmvs_export_sizes, reserved); F(pmvs_export_sizes, image_entries);
  F(pmvs_export_sizes, vimage_entries);
  printf("pmvs_export_buffers.sizeof %zu\n", sizeof(pmvs_export_buffers));
  F(pmvs_export_buffers, fields); F(pmvs_export_buffers, colors); F(pmvs_export_buffers, image_off);
  F(pmvs_export_buffers, image_ids); F(pmvs_export_buffers, image_idx); F(pmvs_export_buffers, vimage_off);
  F(pmvs_export_buffers, vimage_ids); F(pmvs_export_buffers, source);
  printf("flags.writer_order %d\nflags.device %d\n", PMVS_EXPORT_WRITER_ORDER, PMVS_EXPORT_DEVICE);
  return 0;
}
"""


def test_export_structs_match_c(tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    c = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                     check=True).stdout.splitlines())
    import pmvs_amd as P
    for name, T in (("pmvs_export_sizes", P.ExportSizes), ("pmvs_export_buffers", P.ExportBuffers)):
        assert C.sizeof(T) == int(c[name + ".sizeof"]), name
        for f, _ in T._fields_:
            assert getattr(T, f).offset == int(c[f"{name}.{f}"]), (name, f)
    assert [f for f, _ in P.ExportBuffers._fields_] == list(P.Scene.EXPORT_ARRAYS)
    assert (P.EXPORT_WRITER_ORDER, P.EXPORT_DEVICE) == (int(c["flags.writer_order"]), int(c["flags.device"]))


def test_export_rejects_null_arguments(product_lib):
    lib = product_lib
    import pmvs_amd as P
    sz, buf = P.ExportSizes(), P.ExportBuffers()
    assert lib.pmvs_loop_export_sizes(None, C.byref(sz)) == 1
    assert lib.pmvs_loop_export(None, 0, None, C.byref(buf)) == 1
    assert lib.pmvs_export_patches_sizes(None, None, 0, C.byref(sz)) == 1
    assert lib.pmvs_export_patches(None, None, 0, 0, None, C.byref(buf)) == 1
    assert lib.pmvs_last_error()
