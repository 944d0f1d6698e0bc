"""pmvs_tsdf_mesh / pmvs_mesh_patches: a TSDF volume meshed by naive surface nets on the device.
The restatement case compares vertices, normals, colours, faces and both counts byte for byte with a numpy
restatement of the extraction's definition in include/pmvs_amd.h (whole-array float64 operations in the
definition's order) on tests/test_gpu_tsdf.py's volume.  The analytic sphere and the open-boundary case need no
restatement: they check what any correct mesh of that volume must satisfy (closed, manifold, consistently
wound, Euler characteristic 2, outward facing, within a cell's diagonal of the sphere)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does

from test_gpu_tsdf import PARAMS, TRUNC, kw, volume_case  # noqa: F401 -- volume_case is a fixture

pytestmark = pytest.mark.gpu

NAMES = ("vertex", "normal", "color", "face")


def corner(A, c):
    """The values of corner c of every cell of the [nz, ny, nx, ...] array A, as [nz-1, ny-1, nx-1, ...]."""
    nz, ny, nx = A.shape[:3]
    dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
    return A[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def extract(vol, tsdf, obs, color, min_obs):
    """The extraction's definition; color may be None."""
    nx, ny, nz = vol.dims
    n = [nx, ny, nz]
    T, O = np.asarray(tsdf, np.float32).reshape(nz, ny, nx), np.asarray(obs, np.uint8).reshape(nz, ny, nx)
    Cl = np.zeros((nz, ny, nx, 4), np.uint8) if color is None else np.asarray(color, np.uint8).reshape(nz, ny, nx, 4)
    observed, inside = O >= min_obs, T < 0
    if min(n) < 2:
        return {"vertex": np.zeros((0, 3), np.float32), "normal": np.zeros((0, 3), np.float32),
                "color": np.zeros((0, 3), np.uint8), "face": np.zeros((0, 3), np.int32)}
    allobs = np.logical_and.reduce([corner(observed, c) for c in range(8)])
    n_in = sum(corner(inside, c).astype(np.int64) for c in range(8))
    active = allobs & (n_in > 0) & (n_in < 8)
    cells = np.nonzero(active.ravel())[0]
    vid = np.cumsum(active.ravel()) - 1
    # vertices
    shape = active.shape
    sums, count, g = [np.zeros(shape, np.float64) for _ in range(3)], np.zeros(shape, np.int64), [None] * 3
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for k in range(4):
            lo = ((k & 1) << b) | (((k >> 1) & 1) << c)
            hi = lo | (1 << a)
            v0, v1 = corner(T, lo).astype(np.float64), corner(T, hi).astype(np.float64)
            d = v1 - v0
            g[a] = d if k == 0 else g[a] + d
            crosses = corner(inside, lo) != corner(inside, hi)
            with np.errstate(all="ignore"):
                t = v0 / (v0 - v1)
            p = [None] * 3
            p[a], p[b], p[c] = t, np.float64(k & 1), np.float64((k >> 1) & 1)
            for x in range(3):
                sums[x] = sums[x] + np.where(crosses, p[x], 0.0)
            count += crosses
    kk, jj, ii = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    idx = [ii, jj, kk]
    origin, voxel = [np.float64(np.float32(x)) for x in vol.origin], np.float64(np.float32(vol.voxel))
    with np.errstate(all="ignore"):
        m = [sums[x] / count.astype(np.float64) for x in range(3)]
        vertex = np.stack([(origin[x] + (idx[x].astype(np.float64) + 0.5 + m[x]) * voxel).astype(np.float32) for x in range(3)], -1)
        length = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
        ok = (length > 0) & np.isfinite(length)
        normal = np.stack([np.where(ok, (g[x] / length).astype(np.float32), np.float32(0)) for x in range(3)], -1).astype(np.float32)
    has = np.stack([corner(Cl, c)[..., 3] == 255 for c in range(8)])
    mcount = has.sum(0).astype(np.int64)
    csum = sum(np.where(has[c][..., None], corner(Cl, c)[..., :3].astype(np.int64), 0) for c in range(8))
    colour = np.where(mcount[..., None] > 0, (csum + (mcount // 2)[..., None]) // np.maximum(mcount, 1)[..., None], 0).astype(np.uint8)
    # faces
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    vidx = [ii.ravel(), jj.ravel(), kk.ravel()]
    flat = np.arange(nx * ny * nz, dtype=np.int64)
    stride = [1, nx, nx * ny]
    obs_f, in_f, act_f = observed.ravel(), inside.ravel(), active.ravel()
    keys, quads, lower_in = [], [], []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        cond = (vidx[a] + 1 < n[a]) & (vidx[b] >= 1) & (vidx[b] <= n[b] - 2) & (vidx[c] >= 1) & (vidx[c] <= n[c] - 2)
        v = flat[cond]
        w = v + stride[a]
        Q = []
        for db, dc in ((1, 1), (0, 1), (0, 0), (1, 0)):
            cc = [None] * 3
            cc[a], cc[b], cc[c] = vidx[a][v], vidx[b][v] - db, vidx[c][v] - dc
            Q.append((cc[2] * (ny - 1) + cc[1]) * (nx - 1) + cc[0])
        emit = obs_f[v] & obs_f[w] & (in_f[v] != in_f[w]) & act_f[Q[0]] & act_f[Q[1]] & act_f[Q[2]] & act_f[Q[3]]
        keys.append(v[emit] * 3 + a)
        quads.append(np.stack([vid[q[emit]] for q in Q], 1))
        lower_in.append(in_f[v[emit]])
    keys, quads, lower_in = np.concatenate(keys), np.concatenate(quads), np.concatenate(lower_in)
    srt = np.argsort(keys, kind="stable")
    quads, lower_in = quads[srt], lower_in[srt]
    face = np.zeros((len(quads), 2, 3), np.int64)
    for flag, first, second in ((True, (0, 1, 2), (0, 2, 3)), (False, (0, 2, 1), (0, 3, 2))):
        sel = lower_in == flag
        face[sel, 0], face[sel, 1] = quads[sel][:, first], quads[sel][:, second]
    return {"vertex": vertex.reshape(-1, 3)[cells], "normal": normal.reshape(-1, 3)[cells], "color": colour.reshape(-1, 3)[cells],
            "face": face.reshape(-1, 3).astype(np.int32)}


def assert_same(got, want, names=NAMES):
    assert set(got) == set(names)
    for k in names:
        a = got[k].cpu().numpy() if hasattr(got[k], "cpu") else np.asarray(got[k])
        assert a.dtype == want[k].dtype and a.shape == want[k].shape, (k, a.shape, want[k].shape)
        assert a.tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("min_obs", [1, 2])
def test_mesh_matches_restatement(volume_case, min_obs):
    P, g, o, inp, recs, vol, want, aux = volume_case
    v = want[PARAMS[0]]
    w = extract(vol, v["tsdf"], v["obs"], v["color"], min_obs)
    assert len(w["vertex"]) > 100 and len(w["face"]) > 100 and w["color"].any() and np.isfinite(w["normal"]).all()
    assert w["face"].min() >= 0 and w["face"].max() < len(w["vertex"])
    assert_same(g.tsdf_mesh(vol, v["tsdf"], v["obs"], v["color"], min_obs=min_obs), w)
    dev = torch.device("cuda", g.device)
    got = g.tsdf_mesh(vol, torch.as_tensor(v["tsdf"], device=dev), torch.as_tensor(v["obs"], device=dev),
                      torch.as_tensor(v["color"], device=dev), min_obs=min_obs, device=True)
    assert all(t.is_cuda for t in got.values())
    assert_same(got, w)
    # integrate-then-extract in one call, the volume never on the host
    assert_same(g.mesh_patches(recs, vol, TRUNC, min_obs=min_obs, writer_order=True, **kw(PARAMS[0])), w)
    if min_obs == 2:   # fewer voxels count as observed: another mesh
        assert len(w["vertex"]) != len(extract(vol, v["tsdf"], v["obs"], v["color"], 1)["vertex"])
        # no colour volume: the same mesh with colour 0
        nocol = g.tsdf_mesh(vol, v["tsdf"], v["obs"], None, min_obs=min_obs)
        assert_same(nocol, dict(w, color=np.zeros_like(w["color"])))


def raw_mesh(P, g, vol, tsdf, obs, color, vcap, fcap, arrays, min_obs=1):
    """pmvs_tsdf_mesh through ctypes with caller-made host arrays; returns (status, nverts, nfaces)."""
    buf = P.MeshBuffers()
    for k, a in arrays.items():
        setattr(buf, k, a.ctypes.data)
    nv, nf = C.c_int64(-1), C.c_int64(-1)
    st = g.lib.pmvs_tsdf_mesh(g.handle, 0, C.byref(vol), min_obs, tsdf.ctypes.data, obs.ctypes.data,
                              None if color is None else color.ctypes.data, vcap, fcap, C.byref(buf), C.byref(nv), C.byref(nf))
    return st, int(nv.value), int(nf.value)


def test_mesh_caps_and_counting_call(volume_case):
    P, g, o, inp, recs, vol, want, aux = volume_case
    v = want[PARAMS[0]]
    w = extract(vol, v["tsdf"], v["obs"], v["color"], 1)
    nv, nf = len(w["vertex"]), len(w["face"])
    args = (P, g, vol, v["tsdf"], v["obs"], v["color"])
    assert raw_mesh(*args, 0, 0, {}) == (0, nv, nf)              # the counting call: every pointer NULL
    vcap, fcap, guard = nv // 3, nf // 5, 64
    assert 0 < vcap < nv and 0 < fcap < nf
    shapes = {"vertex": (vcap, np.float32), "normal": (vcap, np.float32), "color": (vcap, np.uint8), "face": (fcap, np.int32)}
    arrays = {k: np.full((cap + guard, 3), 0x5A, dt) for k, (cap, dt) in shapes.items()}
    assert raw_mesh(*args, vcap, fcap, arrays) == (0, nv, nf)    # the counts are the totals, not what was written
    for k, (cap, dt) in shapes.items():
        assert arrays[k][:cap].tobytes() == w[k][:cap].tobytes(), k
        assert (arrays[k][cap:] == np.array(0x5A, dt)).all(), k
    # caps beyond the counts, however large, write the counts
    big = {"vertex": np.full((nv + guard, 3), 0x5A, np.float32), "face": np.full((nf + guard, 3), -3, np.int32)}
    assert raw_mesh(*args, 2 ** 62, 2 ** 62, big) == (0, nv, nf)
    assert big["vertex"][:nv].tobytes() == w["vertex"].tobytes() and (big["vertex"][nv:] == np.float32(0x5A)).all()
    assert np.array_equal(big["face"][:nf], w["face"]) and (big["face"][nf:] == -3).all()
    # device mode by hand: the same prefix and guard
    dev = torch.device("cuda", g.device)
    dface = torch.full((fcap + guard, 3), -3, dtype=torch.int32, device=dev)
    ins = [torch.as_tensor(v[k], device=dev) for k in ("tsdf", "obs", "color")]
    buf, cv, cf = P.MeshBuffers(), C.c_int64(-1), C.c_int64(-1)
    buf.face = dface.data_ptr()
    assert g.lib.pmvs_tsdf_mesh(g.handle, P.EXPORT_DEVICE, C.byref(vol), 1, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
                                0, fcap, C.byref(buf), C.byref(cv), C.byref(cf)) == 0
    assert (cv.value, cf.value) == (nv, nf)
    dface = dface.cpu().numpy()
    assert np.array_equal(dface[:fcap], w["face"][:fcap]) and (dface[fcap:] == -3).all()


def test_mesh_degenerate_volumes(volume_case):
    P, g = volume_case[0], volume_case[1]
    vol = P.volume((0, 0, 0), 1.0, (2, 2, 2))
    tsdf, obs = np.full(8, 0.5, np.float32), np.ones(8, np.uint8)
    tsdf[5] = -0.5                                             # one inside corner: (1, 0, 1)
    m = g.tsdf_mesh(vol, tsdf, obs)
    assert m["vertex"].shape == (1, 3) and m["face"].shape == (0, 3)
    assert_same(m, extract(vol, tsdf, obs, None, 1))
    # the mean of the three mid-edge crossings (0.5, 0, 1), (1, 0.5, 1), (1, 0, 0.5)
    assert np.array_equal(m["vertex"][0], np.float32([0.5 + 2.5 / 3, 0.5 + 0.5 / 3, 0.5 + 2.5 / 3]))
    assert m["normal"][0, 0] < 0 < m["normal"][0, 1] and m["normal"][0, 2] < 0              # away from the inside corner
    obs[0] = 0                                                 # an unobserved corner: no cell is active
    assert raw_mesh(P, g, vol, tsdf, obs, None, 0, 0, {}) == (0, 0, 0)
    for dims in ((1, 5, 4), (5, 1, 4), (5, 4, 1), (1, 1, 1)):  # no cells: an empty mesh, not an error
        flat = P.volume((0, 0, 0), 1.0, dims)
        nvox = dims[0] * dims[1] * dims[2]
        t = np.where(np.arange(nvox) % 2 == 0, -0.5, 0.5).astype(np.float32)
        assert raw_mesh(P, g, flat, t, np.ones(nvox, np.uint8), None, 0, 0, {}) == (0, 0, 0)
        m = g.tsdf_mesh(flat, t, np.ones(nvox, np.uint8), device=False)
        assert m["vertex"].shape == (0, 3) and m["face"].shape == (0, 3)


# ---- the analytic sphere
S_DIMS, S_VOXEL, S_ORIGIN, S_R = (24, 22, 20), 0.05, (1.0, -2.0, 0.5), 7.3
S_CENTRE = np.array([12.3, 10.9, 9.8])  # in voxels from the origin; >= 2 voxels clear of every face with S_R


def sphere_volume(P):
    nx, ny, nz = S_DIMS
    assert all(S_CENTRE[a] - S_R >= 2.5 and S_DIMS[a] - S_CENTRE[a] - S_R >= 2.5 for a in range(3))
    vol = P.volume(S_ORIGIN, S_VOXEL, S_DIMS)
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    pos = np.stack([ii, jj, kk], -1) + 0.5                    # voxel centres, in voxels
    dist = np.sqrt(((pos - S_CENTRE) ** 2).sum(-1))
    tsdf = np.clip((dist - S_R) / 3.0, -1, 1).astype(np.float32)   # trunc = 3 voxels
    centre = np.array([np.float64(np.float32(S_ORIGIN[a])) + S_CENTRE[a] * np.float64(np.float32(S_VOXEL)) for a in range(3)])
    return vol, tsdf, np.ones((nz, ny, nx), np.uint8), pos, centre


def directed_edges(face):
    e = np.concatenate([face[:, [0, 1]], face[:, [1, 2]], face[:, [2, 0]]]).astype(np.int64)
    return e[:, 0] * (1 << 32) + e[:, 1], e[:, 1] * (1 << 32) + e[:, 0]


def test_mesh_analytic_sphere(volume_case):
    P, g = volume_case[0], volume_case[1]
    vol, tsdf, obs, pos, centre = sphere_volume(P)
    m = g.tsdf_mesh(vol, tsdf, obs)
    V, F = m["vertex"].astype(np.float64), m["face"]
    assert len(V) > 500 and len(F) > 1000 and F.min() >= 0 and F.max() < len(V)
    fwd, rev = directed_edges(F)
    assert len(np.unique(fwd)) == len(fwd)                     # every directed edge exactly once ...
    assert np.array_equal(np.sort(fwd), np.sort(rev))          # ... and its reverse exactly once: closed, manifold, wound one way
    assert len(np.unique(F)) == len(V)                         # no vertex without a face
    assert len(V) - len(fwd) // 2 + len(F) == 2                # V - E + F = 2
    tri = V[F]
    gn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert ((gn * (tri.mean(1) - centre)).sum(1) > 0).all()    # every triangle faces outward
    assert ((m["normal"].astype(np.float64) * (V - centre)).sum(1) > 0).all()   # and so does every stored normal
    assert np.allclose(np.linalg.norm(m["normal"], axis=1), 1, atol=1e-6)
    radius = S_R * np.float64(np.float32(S_VOXEL))
    assert (np.abs(np.linalg.norm(V - centre, axis=1) - radius) <= np.sqrt(3) * np.float64(np.float32(S_VOXEL))).all()
    assert not m["color"].any()


def test_mesh_open_boundary(volume_case):
    """The sphere with one octant unobserved: the mesh ends there, and stays a manifold with a boundary."""
    P, g = volume_case[0], volume_case[1]
    vol, tsdf, obs, pos, centre = sphere_volume(P)
    obs = obs.copy()
    obs[(pos > S_CENTRE).all(-1)] = 0
    assert 0 < (obs == 0).sum() < obs.size // 4
    m = g.tsdf_mesh(vol, tsdf, obs)
    V, F = m["vertex"].astype(np.float64), m["face"]
    assert len(F) > 500 and F.min() >= 0 and F.max() < len(V)
    # vertices come in ascending index of the active cells: cells with 8 observed corners and both signs
    allobs = np.logical_and.reduce([corner(obs > 0, c) for c in range(8)])
    n_in = sum(corner(tsdf < 0, c).astype(int) for c in range(8))
    cells = np.nonzero((allobs & (n_in > 0) & (n_in < 8)).ravel())[0]
    assert len(cells) == len(V)
    assert allobs.ravel()[cells[F]].all()                      # no face uses a cell with an unobserved corner
    nx, ny, nz = S_DIMS
    cidx = np.stack([cells % (nx - 1), (cells // (nx - 1)) % (ny - 1), cells // ((nx - 1) * (ny - 1))], -1)
    local = (V - np.float64(np.float32(S_ORIGIN))) / np.float64(np.float32(S_VOXEL)) - 0.5 - cidx
    assert (local > -1e-4).all() and (local < 1 + 1e-4).all()  # and every vertex lies in its own cell
    assert not (cidx + 1.5 > S_CENTRE).all(-1).any()           # no vertex in a cell whose upper corner is unobserved
    fwd, rev = directed_edges(F)
    assert len(np.unique(fwd)) == len(fwd)                     # at most once per direction
    boundary = ~np.isin(fwd, rev)
    assert 0 < boundary.sum() < len(fwd) // 4                  # it is open, along the octant's rim only
    full = g.tsdf_mesh(vol, tsdf, np.ones_like(obs), arrays=("face",))
    assert len(F) < len(full["face"])


def test_mesh_errors(volume_case):
    P, g, o, inp, recs, vol, want, aux = volume_case
    lib = g.lib
    small = P.volume((0, 0, 0), 1.0, (2, 2, 2))
    tsdf, obs = np.full(8, 0.5, np.float32), np.ones(8, np.uint8)
    pa = np.ascontiguousarray(recs[:4], P.PATCH_DTYPE)
    good, buf, nv, nf = P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), TRUNC), P.MeshBuffers(), C.c_int64(0), C.c_int64(0)
    nan, inf = float("nan"), float("inf")

    def ref(x):
        return None if x is None else C.byref(x)

    def mesh(scene=g.handle, flags=0, v=small, min_obs=1, t=tsdf.ctypes.data, ob=obs.ctypes.data, vcap=0, fcap=0, b=buf, cv=nv, cf=nf,
             **_):
        return lib.pmvs_tsdf_mesh(scene, flags, ref(v), min_obs, t, ob, None, vcap, fcap, ref(b), ref(cv), ref(cf))

    def patches(scene=g.handle, flags=0, v=small, min_obs=1, vcap=0, fcap=0, b=buf, cv=nv, cf=nf, prm=good, first=0, num=4, n=4,
                p=pa.ctypes.data, **_):
        return lib.pmvs_mesh_patches(scene, p, n, flags, first, num, ref(prm), ref(v), min_obs, vcap, fcap, ref(b), ref(cv), ref(cf))

    def loop(scene=g.handle, flags=0, v=small, min_obs=1, vcap=0, fcap=0, b=buf, cv=nv, cf=nf, prm=good, first=0, num=4, **_):
        return lib.pmvs_loop_mesh(scene, flags, first, num, ref(prm), ref(v), min_obs, vcap, fcap, ref(b), ref(cv), ref(cf))

    assert mesh() == 0 and patches() == 0
    assert loop() == 1                                         # valid arguments, but no loop result
    with pytest.raises(P.PmvsError, match="pmvs status 1:"):
        g.loop_mesh(small, TRUNC)
    bad_volumes = [None, P.volume((nan, 0, 0), 1.0, (2, 2, 2)), P.volume((0, inf, 0), 1.0, (2, 2, 2)), P.volume((0, 0, 0), 0.0, (2, 2, 2)),
                   P.volume((0, 0, 0), -1.0, (2, 2, 2)), P.volume((0, 0, 0), nan, (2, 2, 2)), P.volume((0, 0, 0), inf, (2, 2, 2)),
                   P.volume((0, 0, 0), 1.0, (0, 2, 2)), P.volume((0, 0, 0), 1.0, (2, -1, 2)), P.volume((0, 0, 0), 1.0, (2048, 1024, 1024))]
    for f in (mesh, patches, loop):
        assert f(scene=None) == 1 and f(b=None) == 1 and f(cv=None) == 1 and f(cf=None) == 1
        for v in bad_volumes:
            assert f(v=v) == 1
        for kwargs in (dict(min_obs=0), dict(min_obs=256), dict(min_obs=-1), dict(vcap=-1), dict(fcap=-1), dict(flags=4), dict(flags=-1)):
            assert f(**kwargs) == 1, kwargs
    assert mesh(flags=1) == 1                                  # the writer order means nothing to a volume
    assert mesh(t=None) == 1 and mesh(ob=None) == 1
    assert mesh(min_obs=255) == 0 and patches(min_obs=255) == 0
    for f in (patches, loop):
        assert f(prm=None) == 1
        for trunc in (0.0, -1.0, nan, inf):
            assert f(prm=P.TsdfParams(P.FuseParams(2, 2, 0.01, 0.5), trunc)) == 1
        assert f(prm=P.TsdfParams(P.FuseParams(17, 2, 0.01, 0.5), TRUNC)) == 1
        for first, num in ((-1, 1), (0, 0), (3, 2), (4, 1)):
            assert f(first=first, num=num) == 1
    assert patches(n=-1) == 1 and patches(p=None) == 1
