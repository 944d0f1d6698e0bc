"""CPU tests of the meshing's boundary (pmvs_loop_tsdf, pmvs_tsdf_patches, pmvs_tsdf_mesh, pmvs_loop_mesh,
pmvs_mesh_patches, pmvs_volume_from_points, pmvs_write_ply_mesh_binary): the symbols are exported, the
Python mirror's struct layouts equal the C compiler's, NULL and out-of-range arguments are rejected without
a device, and the mesh PLY round-trips through a numpy parse that checks the exact header."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmvs_loop_tsdf", "pmvs_tsdf_patches", "pmvs_tsdf_mesh", "pmvs_loop_mesh", "pmvs_mesh_patches",
           "pmvs_volume_from_points", "pmvs_write_ply_mesh_binary")
VERTEX_DTYPE = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
FACE_DTYPE = np.dtype([("count", "u1"), ("ids", "<i4", 3)])
PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {nv}\nproperty float x\nproperty float y\n"
              "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar diffuse_red\n"
              "property uchar diffuse_green\nproperty uchar diffuse_blue\nelement face {nf}\n"
              "property list uchar int vertex_indices\nend_header\n")
EINVAL = 1


def parse_ply_mesh_binary(raw: bytes):
    """(vertex records, face ids [nf, 3]) of a binary PLY as pmvs_write_ply_mesh_binary writes it; the header
    must be exactly the documented one and every face a triangle."""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode()
    nv = int(head.split("element vertex ")[1].split("\n")[0])
    nf = int(head.split("element face ")[1].split("\n")[0])
    assert head == PLY_HEADER.format(nv=nv, nf=nf)
    assert VERTEX_DTYPE.itemsize == 27 and FACE_DTYPE.itemsize == 13 and len(raw) - end == 27 * nv + 13 * nf
    v = np.frombuffer(raw[end:end + 27 * nv], VERTEX_DTYPE)
    f = np.frombuffer(raw[end + 27 * nv:], FACE_DTYPE)
    assert (f["count"] == 3).all()
    return v, f["ids"]


def test_mesh_symbols_exported(product_lib):
    import pmvs_amd as P
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cmvs-pmvs_amd", "libpmvs_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS:
        assert s in exported and s in P.EXPORTS, s


def test_mesh_layouts_match_c(tmp_path):
    import pmvs_amd as P
    exe = tmp_path / "mesh_layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "csrc", "mesh_layout.c"), "-o", str(exe)], check=True)
    c = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *rest = line.split()
        c[k if rest[0] != "sizeof" else k + ".sizeof"] = int(rest[-1])
    for name, T in (("pmvs_volume", P.Volume), ("pmvs_tsdf_params", P.TsdfParams), ("pmvs_tsdf_buffers", P.TsdfBuffers),
                    ("pmvs_mesh_buffers", P.MeshBuffers)):
        assert C.sizeof(T) == c[name + ".sizeof"], name
        for f, _ in T._fields_:
            assert getattr(T, f).offset == c[f"{name}.{f}"], (name, f)
    assert len(c) == 4 + 3 + 2 + 3 + 4  # every field of the four structs was printed and compared
    assert C.sizeof(P.TsdfParams) == C.sizeof(P.FuseParams) + 4


def test_mesh_arguments_rejected_without_a_device(product_lib):
    """No scene exists here, so every call must fail before it touches a device: with the NULL scene alone, and
    with each other NULL or out-of-range argument beside it.  (tests/test_gpu_mesh.py repeats the list with a
    real scene, where the argument itself is what is rejected.)"""
    import pmvs_amd as P
    lib = product_lib
    prm = P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), 0.1)
    vol = P.volume((0, 0, 0), 0.1, (4, 4, 4))
    tb, mb, nv, nf = P.TsdfBuffers(), P.MeshBuffers(), C.c_int64(-7), C.c_int64(-7)
    tsdf, obs = np.ones(64, np.float32), np.ones(64, np.uint8)
    nan, inf = float("nan"), float("inf")
    bad_volumes = [None, P.volume((nan, 0, 0), 0.1, (4, 4, 4)), P.volume((0, inf, 0), 0.1, (4, 4, 4)),
                   P.volume((0, 0, 0), 0.0, (4, 4, 4)), P.volume((0, 0, 0), -1.0, (4, 4, 4)), P.volume((0, 0, 0), nan, (4, 4, 4)),
                   P.volume((0, 0, 0), inf, (4, 4, 4)), P.volume((0, 0, 0), 0.1, (0, 4, 4)), P.volume((0, 0, 0), 0.1, (4, 4, -1)),
                   P.volume((0, 0, 0), 0.1, (2048, 1024, 1024))]
    bad_params = [None, P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), 0.0), P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), -0.1),
                  P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), nan), P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), inf),
                  P.TsdfParams(P.FuseParams(-1, 2, 0.01, 0.5), 0.1), P.TsdfParams(P.FuseParams(2, 256, 0.01, 0.5), 0.1)]

    def ref(x):
        return None if x is None else C.byref(x)

    def calls(p=prm, v=vol, t=tb, m=mb, flags=0, min_obs=1, vcap=0, fcap=0, cv=nv, cf=nf):
        tail = (min_obs, vcap, fcap, ref(m), ref(cv), ref(cf))
        return [lib.pmvs_loop_tsdf(None, flags, 0, 1, ref(p), ref(v), ref(t)),
                lib.pmvs_tsdf_patches(None, None, 0, flags, 0, 1, ref(p), ref(v), ref(t)),
                lib.pmvs_tsdf_mesh(None, flags, ref(v), min_obs, tsdf.ctypes.data, obs.ctypes.data, None, vcap, fcap, ref(m),
                                   ref(cv), ref(cf)),
                lib.pmvs_loop_mesh(None, flags, 0, 1, ref(p), ref(v), *tail),
                lib.pmvs_mesh_patches(None, None, 0, flags, 0, 1, ref(p), ref(v), *tail)]

    assert calls() == [EINVAL] * 5 and lib.pmvs_last_error()
    for v in bad_volumes:
        assert calls(v=v) == [EINVAL] * 5
    for p in bad_params:
        assert calls(p=p) == [EINVAL] * 5
    for kw in (dict(t=None), dict(m=None), dict(cv=None), dict(cf=None), dict(flags=4), dict(flags=-1), dict(min_obs=0),
               dict(min_obs=256), dict(vcap=-1), dict(fcap=-1)):
        assert calls(**kw) == [EINVAL] * 5, kw
    assert lib.pmvs_tsdf_mesh(None, 0, C.byref(vol), 1, None, None, None, 0, 0, C.byref(mb), C.byref(nv), C.byref(nf)) == EINVAL
    assert (nv.value, nf.value) == (-7, -7)
    assert lib.pmvs_write_ply_mesh_binary(None, 0, None, None, None, 0, None) == EINVAL
    assert lib.pmvs_write_ply_mesh_binary(b"/nonexistent-dir/x.ply", 0, None, None, None, 0, None) == EINVAL


def test_volume_from_points(product_lib):
    """The documented arithmetic, restated: the box, the voxel as its longest extent / cells in f32, the origin
    `pad` voxels below the box, and dims that cover the box plus the padding."""
    import pmvs_amd as P
    rng = np.random.default_rng(11)
    pts = (rng.normal(size=(500, 3)) * [1.0, 0.37, 0.11] + [3, -2, 0.5]).astype(np.float32)
    v = P.volume_from_points(pts, 256, 3)
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    voxel = np.float32((hi - lo).max() / 256.0)
    assert np.float32(v.voxel) == voxel
    assert list(v.origin) == [float(np.float32(lo[a] - 3.0 * np.float64(voxel))) for a in range(3)]
    assert list(v.dims) == [int(max(1.0, np.ceil((hi[a] - lo[a]) / np.float64(voxel)))) + 6 for a in range(3)]
    assert 262 <= v.dims[0] <= 263 and v.dims[1] < v.dims[0] and v.dims[2] < v.dims[1]
    one = P.volume_from_points(pts, 8, 0)
    assert 8 <= max(one.dims) <= 9
    lib, out = product_lib, P.Volume()
    flat = np.zeros((4, 3), np.float32)
    for n, coord, cells, pad, o in ((0, pts, 256, 3, out), (500, None, 256, 3, out), (500, pts, 0, 3, out), (500, pts, 256, -1, out),
                                    (500, pts, 256, 3, None), (4, flat, 256, 3, out)):
        assert lib.pmvs_volume_from_points(n, None if coord is None else coord.ctypes.data, cells, pad,
                                           None if o is None else C.byref(o)) == EINVAL
    bad = pts.copy()
    bad[7, 1] = np.inf
    assert lib.pmvs_volume_from_points(500, bad.ctypes.data, 256, 3, C.byref(out)) == EINVAL
    assert lib.pmvs_volume_from_points(500, pts.ctypes.data, 2000000, 3, C.byref(out)) == EINVAL  # past 2^31-1 voxels


def test_write_ply_mesh_binary_round_trip(product_lib, tmp_path):
    import pmvs_amd as P
    rng = np.random.default_rng(6)
    for nv, nf in ((0, 0), (3, 1), (4097, 8200), (5, 0)):  # none, one, more than one write of the writer, no faces
        vertex = rng.normal(size=(nv, 3)).astype(np.float32)
        normal = rng.normal(size=(nv, 3)).astype(np.float32)
        if nv:
            vertex[0] = [np.float32("-0.0"), np.float32("inf"), np.float32(1e-42)]  # bits, not values
        color = rng.integers(0, 256, (nv, 3)).astype(np.uint8)
        face = rng.integers(0, max(nv, 1), (nf, 3)).astype(np.int32)
        path = str(tmp_path / f"mesh{nv}.ply")
        P.write_ply_mesh_binary(path, vertex, normal, color, face)
        v, f = parse_ply_mesh_binary(open(path, "rb").read())
        assert len(v) == nv and f.shape == (nf, 3)
        assert v["xyz"].tobytes() == vertex.tobytes() and v["n"].tobytes() == normal.tobytes()
        assert np.array_equal(v["rgb"], color) and np.array_equal(f, face)
    lib = product_lib
    one, tri = np.zeros(3, np.float32), np.zeros(3, np.int32)
    bad = str(tmp_path / "bad.ply").encode()
    assert lib.pmvs_write_ply_mesh_binary(bad, 1, one.ctypes.data, None, None, 0, None) == EINVAL
    assert lib.pmvs_write_ply_mesh_binary(bad, 0, None, None, None, 1, None) == EINVAL
    assert lib.pmvs_write_ply_mesh_binary(bad, -1, None, None, None, 0, None) == EINVAL
    assert lib.pmvs_write_ply_mesh_binary(bad, 0, None, None, None, -1, tri.ctypes.data) == EINVAL
