"""CPU tests of the texturing's boundary (pmvs_mesh_raster, pmvs_mesh_texture, pmvs_write_ply_texmesh_binary): the
symbols are exported, the Python mirror's struct layouts equal the C compiler's, NULL and out-of-range arguments
are rejected without a device and leave the outputs untouched, and the textured-mesh PLY round-trips through a
numpy parse that checks the exact header, the 42-byte face record and the texture coordinates' formula."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pmvs_mesh_raster", "pmvs_mesh_texture", "pmvs_write_ply_texmesh_binary")
VERTEX_DTYPE = np.dtype([("xyz", "<f4", 3), ("n", "<f4", 3), ("rgb", "u1", 3)])
FACE_DTYPE = np.dtype([("count", "u1"), ("ids", "<i4", 3), ("tcount", "u1"), ("tex", "<f4", 6), ("texnumber", "<i4")])
PLY_HEADER = ("ply\nformat binary_little_endian 1.0\n{tex}element vertex {nv}\nproperty float x\nproperty float y\n"
              "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nproperty uchar diffuse_red\n"
              "property uchar diffuse_green\nproperty uchar diffuse_blue\nelement face {nf}\n"
              "property list uchar int vertex_indices\nproperty list uchar float texcoord\nproperty int texnumber\n"
              "end_header\n")
EINVAL = 1


def parse_ply_texmesh_binary(raw: bytes):
    """(texture file names, vertex records, face records) of a binary PLY as pmvs_write_ply_texmesh_binary writes
    it; the header must be exactly the documented one, every face a triangle with six texture coordinates."""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode()
    nv = int(head.split("element vertex ")[1].split("\n")[0])
    nf = int(head.split("element face ")[1].split("\n")[0])
    tex = [l[len("comment TextureFile "):] for l in head.split("\n") if l.startswith("comment TextureFile ")]
    assert head == PLY_HEADER.format(tex="".join(f"comment TextureFile {n}\n" for n in tex), nv=nv, nf=nf)
    assert VERTEX_DTYPE.itemsize == 27 and FACE_DTYPE.itemsize == 42 and len(raw) - end == 27 * nv + 42 * nf
    v = np.frombuffer(raw[end:end + 27 * nv], VERTEX_DTYPE)
    f = np.frombuffer(raw[end + 27 * nv:], FACE_DTYPE)
    assert (f["count"] == 3).all() and (f["tcount"] == 6).all()
    return tex, v, f


def texcoords(view, uv, dims):
    """The writer's formula, restated: u = clamp((x + 0.5) / W0, 0, 1), v = clamp(1 - (y + 0.5) / H0, 0, 1) in
    double, rounded to float32; six zeros for a face without a view."""
    out = np.zeros((len(view), 6), np.float32)
    has = view >= 0
    wh = np.asarray(dims, np.float64).reshape(-1, 2)[np.where(has, view, 0)]
    for k in range(3):
        x, y = uv[:, 2 * k].astype(np.float64), uv[:, 2 * k + 1].astype(np.float64)
        out[:, 2 * k] = np.clip((x + 0.5) / wh[:, 0], 0.0, 1.0).astype(np.float32)
        out[:, 2 * k + 1] = np.clip(1.0 - (y + 0.5) / wh[:, 1], 0.0, 1.0).astype(np.float32)
    out[~has] = 0
    return out


def test_texmesh_symbols_exported(product_lib):
    import pmvs_amd as P
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "cmvs-pmvs_amd", "libpmvs_amd.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for s in SYMBOLS:
        assert s in exported and s in P.EXPORTS, s


def test_texmesh_layouts_match_c(tmp_path):
    import pmvs_amd as P
    exe = tmp_path / "texmesh_layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "csrc", "texmesh_layout.c"), "-o", str(exe)], check=True)
    c = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *rest = line.split()
        c[k if rest[0] != "sizeof" else k + ".sizeof"] = int(rest[-1])
    for name, T in (("pmvs_raster_buffers", P.RasterBuffers), ("pmvs_texture_params", P.TextureParams),
                    ("pmvs_texture_buffers", P.TextureBuffers)):
        assert C.sizeof(T) == c[name + ".sizeof"], name
        for f, _ in T._fields_:
            assert getattr(T, f).offset == c[f"{name}.{f}"], (name, f)
    assert len(c) == 3 + 2 + 2 + 3  # every field of the three structs was printed and compared


def test_texmesh_arguments_rejected_without_a_device(product_lib):
    """No scene exists here, so every call must fail before it touches a device: with the NULL scene alone, and with
    each other NULL or out-of-range argument beside it; the outputs keep their bytes.  (tests/test_gpu_mesh_raster.py
    and test_gpu_mesh_texture.py repeat the list with a real scene, where the argument itself is what is rejected.)"""
    import pmvs_amd as P
    lib = product_lib
    vertex = np.zeros((3, 3), np.float32)
    face = np.array([[0, 1, 2]], np.int32)
    out_face, out_depth = np.full(16, -7, np.int32), np.full(16, -7, np.float32)
    out_view, out_uv, out_score = np.full(1, -7, np.int32), np.full(6, -7, np.float32), np.full(1, -7, np.float32)
    rb = P.RasterBuffers(out_face.ctypes.data, out_depth.ctypes.data)
    tb = P.TextureBuffers(out_view.ctypes.data, out_uv.ctypes.data, out_score.ctypes.data)
    good = P.TextureParams(0.01, 0.0)
    nan, inf = float("nan"), float("inf")

    def ref(x):
        return None if x is None else C.byref(x)

    def calls(flags=0, first=0, num=1, prm=good, nv=3, v=vertex.ctypes.data, nf=1, f=face.ctypes.data, r=rb, t=tb):
        return [lib.pmvs_mesh_raster(None, flags, first, num, nv, v, nf, f, ref(r)),
                lib.pmvs_mesh_texture(None, flags, first, num, ref(prm), nv, v, nf, f, ref(t))]

    assert calls() == [EINVAL] * 2 and lib.pmvs_last_error()
    for kw in (dict(r=None, t=None), dict(flags=1), dict(flags=4), dict(flags=-1), dict(first=-1), dict(num=0), dict(num=-1),
               dict(nv=-1), dict(nf=-1), dict(nv=1 << 31), dict(nf=1 << 31), dict(v=None), dict(f=None), dict(nv=2),
               dict(flags=2), dict(nf=0, f=None), dict(nv=0, v=None, nf=0, f=None)):
        assert calls(**kw) == [EINVAL] * 2, kw
    for prm in (None, P.TextureParams(-0.01, 0.0), P.TextureParams(nan, 0.0), P.TextureParams(inf, 0.0),
                P.TextureParams(0.01, -1.0), P.TextureParams(0.01, nan), P.TextureParams(0.01, inf)):
        assert calls(prm=prm)[1] == EINVAL
    for a in (out_face, out_view):
        assert (a == -7).all()
    for a in (out_depth, out_uv, out_score):
        assert (a == -7).all()
    name = (C.c_char_p * 1)(b"a.jpg")
    dims = np.array([4, 4], np.int32)
    assert lib.pmvs_write_ply_texmesh_binary(None, 0, None, None, None, 0, None, None, None, 0, None, None) == EINVAL
    assert lib.pmvs_write_ply_texmesh_binary(b"/nonexistent-dir/x.ply", 0, None, None, None, 0, None, None, None, 1, name,
                                             dims.ctypes.data) == EINVAL


def test_write_ply_texmesh_binary_round_trip(product_lib, tmp_path):
    import pmvs_amd as P
    rng = np.random.default_rng(9)
    files = ["../visualize/00000000.jpg", "../visualize/00000001.ppm", "with space.png"]
    dims = np.array([[640, 480], [300, 200], [7, 5]], np.int32)
    # none; one face; more than one write of the writer (4096 records); no faces; no textures (every view -1)
    for nv, nf, ntex in ((0, 0, 3), (3, 1, 3), (4097, 8200, 3), (5, 0, 1), (4, 6, 0)):
        vertex = rng.normal(size=(nv, 3)).astype(np.float32)
        normal = rng.normal(size=(nv, 3)).astype(np.float32)
        if nv:
            vertex[0] = [np.float32("-0.0"), np.float32("inf"), np.float32(1e-42)]  # bits, not values
        color = rng.integers(0, 256, (nv, 3)).astype(np.uint8)
        face = rng.integers(0, max(nv, 1), (nf, 3)).astype(np.int32)
        view = rng.integers(-1, ntex, nf).astype(np.int32)
        uv = (rng.uniform(-0.2, 1.2, (nf, 6)) * 300.0).astype(np.float32)   # some clamp on every side
        if nf > 4 and ntex == 3:
            view[:3] = (-1, 0, ntex - 1)
            uv[1] = [-0.5, -0.5, 639.5, 479.5, -0.75, 480.0]                 # the borders' exact values and beyond
        path = str(tmp_path / f"texmesh{nv}.ply")
        P.write_ply_texmesh_binary(path, vertex, normal, color, face, view, uv, files[:ntex], dims[:ntex])
        tex, v, f = parse_ply_texmesh_binary(open(path, "rb").read())
        assert tex == files[:ntex] and len(v) == nv and len(f) == nf
        assert v["xyz"].tobytes() == vertex.tobytes() and v["n"].tobytes() == normal.tobytes()
        assert np.array_equal(v["rgb"], color) and np.array_equal(f["ids"], face) and np.array_equal(f["texnumber"], view)
        want = texcoords(view, uv, dims[:max(ntex, 1)])
        assert f["tex"].tobytes() == want.tobytes()
        if nf > 4 and ntex == 3:
            assert (view == -1).any() and not f["tex"][view == -1].any()       # a face without a view: six zeros
            assert (want == 0).any() and (want == 1).any() and ((want > 0) & (want < 1)).any()   # clamped and not
            assert list(f["tex"][1]) == [0.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    lib = product_lib
    one, tri, vw, tc = np.zeros(3, np.float32), np.zeros(3, np.int32), np.zeros(1, np.int32), np.zeros(6, np.float32)
    col = np.zeros(3, np.uint8)
    bad = str(tmp_path / "bad.ply").encode()
    names = (C.c_char_p * 1)(b"a.jpg")
    d1 = np.array([4, 4], np.int32)

    def write(nv=1, v=one, n=one, c=col, nf=1, f=tri, view=vw, uv=tc, ntex=1, files=names, dims=d1):
        p = [None if a is None else a.ctypes.data for a in (v, n, c)]
        q = [None if a is None else a.ctypes.data for a in (f, view, uv)]
        return lib.pmvs_write_ply_texmesh_binary(bad, nv, *p, nf, *q, ntex, files, None if dims is None else dims.ctypes.data)

    assert write() == 0
    assert write(v=None) == EINVAL and write(c=None) == EINVAL and write(f=None) == EINVAL and write(view=None) == EINVAL
    assert write(uv=None) == EINVAL and write(nv=-1) == EINVAL and write(nf=-1) == EINVAL and write(ntex=-1) == EINVAL
    assert write(files=None) == EINVAL and write(dims=None) == EINVAL
    assert write(view=np.array([1], np.int32)) == EINVAL and write(view=np.array([-2], np.int32)) == EINVAL   # outside -1 .. ntex-1
    assert write(ntex=0, files=None, dims=None) == EINVAL and write(ntex=0, files=None, dims=None, view=np.array([-1], np.int32)) == 0
    assert write(dims=np.array([0, 4], np.int32)) == EINVAL
    with pytest.raises(ValueError):
        P.write_ply_texmesh_binary(bad.decode(), one, one, col, tri, vw, tc, ["a", "b"], d1)
