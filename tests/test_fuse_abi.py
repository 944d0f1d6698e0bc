"""CPU tests of the fusion's boundary (pmvs_loop_fuse, pmvs_fuse_patches, pmvs_write_ply_binary): the
symbols are exported, the Python mirror's struct layouts equal the C compiler's, NULL arguments are
rejected without a device, and the binary PLY round-trips through a numpy parse."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmvs_loop_fuse", "pmvs_fuse_patches", "pmvs_write_ply_binary")
PLY_DTYPE = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3), ("support", "u1")])
PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\n"
              "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar diffuse_red\n"
              "property uchar diffuse_green\nproperty uchar diffuse_blue\nproperty uchar support\nend_header\n")


def parse_ply_binary(raw: bytes):
    """The vertex records of a binary PLY as pmvs_write_ply_binary writes it; the header must be exactly
    the documented one."""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode()
    n = int(head.split("element vertex ")[1].split("\n")[0])
    assert head == PLY_HEADER.format(n=n)
    assert PLY_DTYPE.itemsize == 28 and len(raw) - end == 28 * n
    return np.frombuffer(raw[end:], PLY_DTYPE)


def test_fuse_symbols_exported(product_lib):
    import pmvs_amd as P
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cmvs-pmvs_amd", "libpmvs_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS:
        assert s in exported and s in P.EXPORTS, s


def test_fuse_layouts_match_c(tmp_path):
    import pmvs_amd as P
    exe = tmp_path / "fuse_layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "csrc", "fuse_layout.c"), "-o", str(exe)], check=True)
    c = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *rest = line.split()
        c[k if rest[0] != "sizeof" else k + ".sizeof"] = int(rest[-1])
    for name, T in (("pmvs_fuse_params", P.FuseParams), ("pmvs_fuse_buffers", P.FuseBuffers)):
        assert C.sizeof(T) == c[name + ".sizeof"], name
        for f, _ in T._fields_:
            assert getattr(T, f).offset == c[f"{name}.{f}"], (name, f)
    assert len(c) == 2 + 4 + 7  # every field of both structs was printed and compared


def test_fuse_null_arguments_rejected(product_lib):
    import pmvs_amd as P
    lib = product_lib
    prm, buf, cnt = P.FuseParams(2, 2, 0.01, 0.5), P.FuseBuffers(), C.c_int64(-7)
    assert lib.pmvs_loop_fuse(None, 0, 0, 1, C.byref(prm), 0, C.byref(buf), C.byref(cnt)) == 1  # PMVS_EINVAL
    assert lib.pmvs_fuse_patches(None, None, 0, 0, 0, 1, C.byref(prm), 0, C.byref(buf), C.byref(cnt)) == 1
    assert lib.pmvs_last_error()
    assert cnt.value == -7
    assert lib.pmvs_write_ply_binary(None, 0, None, None, None, None) == 1
    assert lib.pmvs_write_ply_binary(b"/nonexistent-dir/x.ply", 0, None, None, None, None) == 1


def test_write_ply_binary_round_trip(product_lib, tmp_path):
    import pmvs_amd as P
    rng = np.random.default_rng(5)
    for n in (0, 1, 4097):  # none, one, more than one write of the writer
        coord = rng.normal(size=(n, 3)).astype(np.float32)
        normal = rng.normal(size=(n, 3)).astype(np.float32)
        if n:
            coord[0] = [np.float32("-0.0"), np.float32("inf"), np.float32(1e-42)]  # bits, not values
        color = rng.integers(0, 256, (n, 3)).astype(np.uint8)
        support = rng.integers(0, 256, n).astype(np.uint8)
        path = str(tmp_path / f"cloud{n}.ply")
        P.write_ply_binary(path, coord, normal, color, support)
        v = parse_ply_binary(open(path, "rb").read())
        assert len(v) == n
        assert v["xyz"].tobytes() == coord.tobytes() and v["n"].tobytes() == normal.tobytes()
        assert np.array_equal(v["rgb"], color) and np.array_equal(v["support"], support)
    lib = product_lib
    one = np.zeros(3, np.float32)
    assert lib.pmvs_write_ply_binary(str(tmp_path / "bad.ply").encode(), 1, one.ctypes.data, None, None, None) == 1
    assert lib.pmvs_write_ply_binary(str(tmp_path / "bad.ply").encode(), -1, None, None, None, None) == 1
