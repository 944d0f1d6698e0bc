"""pmvs_loop_depth_maps / pmvs_depth_maps_patches: the model's per-target depth maps produced on the
device.  The oracle is the CPU restatement pinned to the reference's object code:
OracleScene.organizer_ops([("depth", coords)]) gives the winning patch of every cell for patches added
in order (CFilter::setDepthMapsThread's rule) and OracleScene.depth the exact f32 depth.  Every array is
compared for exact equality of dtype, shape and bytes."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does: a torch build that ships
#               its own HIP runtime finds no device when the system's runtime was opened first

pytestmark = pytest.mark.gpu

NAMES = ("patch", "depth", "normal", "ncc")
EINVAL = "pmvs status 1:"
COPIES = (range(100, 140), range(1300, 1340))  # rows 1300-1339 are copies of rows 100-139


def order_keys(model, inp):
    """pmvs2's key of collectPatches(1), as tests/test_gpu_loop_export.py restates it: bt = the lowest
    view index below tnum in images (first position k0), (bt << 40) + grids[k0][1] * gwidth(bt) +
    grids[k0][0]; no target image: last."""
    tnum = inp.num_targets
    gw = [((inp.images[t].shape[1] >> inp.level) + inp.csize - 1) // inp.csize for t in range(tnum)]
    key = np.empty(len(model), np.int64)
    for p, q in enumerate(model):
        bt, k0 = np.iinfo(np.int32).max, -1
        for k in range(q["num_images"]):
            v = int(q["images"][k])
            if v < tnum and v < bt:
                bt, k0 = v, k
        key[p] = np.iinfo(np.int64).max if k0 < 0 else \
            (bt << 40) + int(q["grids"][k0][1]) * gw[bt] + int(q["grids"][k0][0])
    return key


def crafted_scene(P):
    """6 views at 320 x 240, level 1, 4 targets; target 1's image cropped to 300 x 200 (rows and
    columns removed at the bottom and right keep the projection valid), so the cell grids are 80 x 60,
    75 x 50, 80 x 60, 80 x 60: a wrong per-target offset or width cannot pass."""
    inp, _ = P.synth_scene(6, 320, 240, level=1, num_targets=4)
    inp.images[1] = np.ascontiguousarray(inp.images[1][:200, :300])
    return inp


def crafted_records(P):
    """1500 records: coordinates uniform in +-0.5; rows 1000-1299 uniform in +-1.6 (many leave the images
    or fall on the border cells); rows 1300-1339 exact copies of rows 100-139 (depth ties far apart in
    the array); rows 1340-1342 far outside or behind cameras; random non-trivial images / grids (the
    writer order is not the identity); random normals and ncc."""
    rng = np.random.default_rng(20261)
    n = 1500
    r = np.zeros(n, P.PATCH_DTYPE)
    r["coord"][:, :3] = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    r["coord"][1000:1300, :3] = rng.uniform(-1.6, 1.6, (300, 3)).astype(np.float32)
    r["coord"][1300:1340] = r["coord"][100:140]
    r["coord"][1340:1343, :3] = [(0, 0, 50), (50, 0, 0), (0, -50, 0)]
    r["coord"][:, 3] = 1.0
    r["normal"][:, :3] = rng.normal(size=(n, 3)).astype(np.float32)
    for f in ("ncc", "dscale", "ascale"):
        r[f] = rng.uniform(0, 1, n).astype(np.float32)
    for i in range(n):
        k = int(rng.integers(1, 6))
        r["num_images"][i] = k
        r["images"][i, :k] = rng.integers(0, 6, k)
        r["grids"][i, :k, 0] = rng.integers(0, 75, k)
        r["grids"][i, :k, 1] = rng.integers(0, 50, k)
    return r


def oracle_maps(o, inp, recs, rows):
    """The four arrays for the records taken in the order `rows`, from the oracle alone."""
    m = recs[rows]
    coords = np.ascontiguousarray(m["coord"], np.float32)
    patch = o.organizer_ops([("depth", coords)])[0].astype(np.int32)
    gw, gh = o.grid_sizes()
    depth = np.zeros(len(patch), np.float32)
    off = 0
    for t in range(inp.num_targets):
        c = int(gw[t]) * int(gh[t])
        w = patch[off:off + c]
        depth[off:off + c][w >= 0] = o.depth(t, coords[w[w >= 0]])
        off += c
    assert off == len(patch)
    filled = patch >= 0
    normal = np.zeros((len(patch), 3), np.float32)
    normal[filled] = m["normal"][patch[filled], :3]
    ncc = np.zeros(len(patch), np.float32)
    ncc[filled] = m["ncc"][patch[filled]]
    return {"patch": patch, "depth": depth, "normal": normal, "ncc": ncc}


def assert_same(got, want, names=NAMES):
    assert set(got) == set(names)
    for k in names:
        a = np.asarray(got[k])
        assert a.dtype == want[k].dtype and a.shape == want[k].shape, k
        assert a.tobytes() == want[k].tobytes(), k


def check_empty_cells(maps):
    e = maps["patch"] < 0
    assert (maps["patch"][e] == -1).all()
    for k in ("depth", "normal", "ncc"):
        assert not maps[k][e].view(np.uint32).any(), k  # +0.0 exactly


@pytest.fixture(scope="module")
def crafted(gpu_available, oracle_mod):
    import pmvs_amd as P
    inp = crafted_scene(P)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    recs = crafted_records(P)
    order = np.argsort(order_keys(recs, inp), kind="stable")
    want = {False: oracle_maps(o, inp, recs, np.arange(len(recs))), True: oracle_maps(o, inp, recs, order)}
    # coverage, on the oracle's result alone
    mo = want[False]["patch"]
    assert (mo < 0).any() and (mo >= 0).any()
    assert np.isin(mo, COPIES[0]).any() and not np.isin(mo, COPIES[1]).any()  # ties go to the earlier row
    rev = oracle_maps(o, inp, recs, np.arange(len(recs))[::-1])["patch"]
    rev = np.where(rev >= 0, len(recs) - 1 - rev, -1)
    assert (rev != mo).any()                                                 # the order matters
    assert not np.array_equal(order, np.arange(len(recs)))                   # the writer order is a real permutation
    yield P, g, o, inp, recs, order, want
    g.close()
    o.close()


@pytest.fixture(scope="module")
def looped(gpu_available, oracle_mod):
    """One loop result left on the device (the shape of test_gpu_loop_export.py's fixture)."""
    import pmvs_amd as P
    inp, p = P.synth_scene(6, 480, 360, level=1, supersample=2, num_targets=4)
    g, o = P.Scene(inp), oracle_mod.OracleScene(inp)
    cands = P.synth_candidates(p, inp.projections, 300, seed=3)
    r, _ = g.refine_batch(cands)
    seeds = P.patches_from_refined(r)
    n, _ = g.run_loop(seeds, inp.threshold, iterations=2, wave=256, fetch=False)
    yield P, g, o, inp, n
    g.close()
    o.close()


def test_depth_map_layout(crafted):
    P, g, o, inp, recs, order, want = crafted
    dims, off = g.depth_map_layout()
    gw, gh = o.grid_sizes()
    assert dims.dtype == np.int32 and off.dtype == np.int64
    assert dims.tolist() == [[int(gw[t]), int(gh[t])] for t in range(4)] == [[80, 60], [75, 50], [80, 60], [80, 60]]
    assert off.tolist() == [0] + np.cumsum([int(gw[t]) * int(gh[t]) for t in range(4)]).tolist()
    assert off[-1] == 18150
    v = P.depth_map_view(want[False]["normal"], dims, off, 1)
    assert v.shape == (50, 75, 3) and v.base is not None
    assert P.depth_map_view(want[False]["patch"], dims, off, 3).shape == (60, 80)


@pytest.mark.parametrize("writer_order", [False, True])
def test_depth_maps_crafted(crafted, writer_order):
    P, g, o, inp, recs, order, want = crafted
    got = g.depth_maps_patches(recs, writer_order=writer_order)
    assert_same(got, want[writer_order])
    check_empty_cells(got)
    if writer_order:  # `patch` indexes the rows of the export of the same records
        src = g.export_patches(recs, writer_order=True, arrays=("source",))["source"]
        assert np.array_equal(src, order)


def test_depth_maps_device_mode_and_partial(crafted):
    P, g, o, inp, recs, order, want = crafted
    dv = g.depth_maps_patches(recs, writer_order=True, device=True)
    assert all(t.is_cuda and t.device.index == g.device for t in dv.values())
    assert_same({k: t.cpu().numpy() for k, t in dv.items()}, want[True])
    assert_same(g.depth_maps_patches(recs, writer_order=False, arrays=("patch",)), want[False], ("patch",))
    # a request for patch alone writes nothing else: the other pointers stay NULL, and buffers the call
    # is not given keep their contents
    buf = P.DepthMapBuffers()
    patch = np.full(18150, 7, np.int32)
    buf.patch = patch.ctypes.data
    pa = np.ascontiguousarray(recs, P.PATCH_DTYPE)
    assert g.lib.pmvs_depth_maps_patches(g.handle, pa.ctypes.data, len(pa), 0, buf) == 0
    assert np.array_equal(patch, want[False]["patch"])
    assert_same(g.depth_maps_patches(recs, writer_order=True, arrays=("depth", "ncc")), want[True], ("depth", "ncc"))


def test_depth_maps_no_records(crafted):
    P, g, o, inp, recs, order, want = crafted
    for writer_order in (False, True):
        got = g.depth_maps_patches(recs[:0], writer_order=writer_order)
        assert (got["patch"] == -1).all() and got["patch"].shape == (18150,)
        check_empty_cells(got)


def test_loop_depth_maps_match_oracle(looped):
    P, g, o, inp, n = looped
    h = g.loop_hash()
    wr = g.loop_depth_maps(writer_order=True)
    mo = g.loop_depth_maps(writer_order=False)
    dv = g.loop_depth_maps(writer_order=True, device=True)
    assert g.loop_hash() == h                      # the maps change nothing in the model
    assert_same({k: t.cpu().numpy() for k, t in dv.items()}, wr)
    ex = g.loop_export(writer_order=True)          # and do not consume it
    model = g.loop_fetch(n)                        # still there
    assert n > 1000 and len(model) == n
    src = ex["source"]
    assert np.array_equal(ex["fields"][:, :4], model["coord"][src])
    assert_same(wr, oracle_maps(o, inp, model, src))
    assert_same(mo, oracle_maps(o, inp, model, np.arange(n)))
    assert (wr["patch"] >= 0).any() and (wr["patch"] < 0).any()
    check_empty_cells(wr)


def test_depth_maps_errors(crafted):
    P, g, o, inp, recs, order, want = crafted
    with pytest.raises(P.PmvsError, match=EINVAL):   # no run_loop on this scene yet
        g.loop_depth_maps()
    buf = P.DepthMapBuffers()
    pa = np.ascontiguousarray(recs[:4], P.PATCH_DTYPE)
    for flags in (4, 8, 1 | 16, -1):                 # any bit beyond WRITER_ORDER | DEVICE
        assert g.lib.pmvs_depth_maps_patches(g.handle, pa.ctypes.data, 4, flags, buf) == 1
        assert g.lib.pmvs_loop_depth_maps(g.handle, flags, buf) == 1
    bad = recs[:4].copy()
    bad["num_images"][2] = 0
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.depth_maps_patches(bad)
    bad = recs[:4].copy()
    bad["images"][1, 0] = 6                          # view index >= num_views
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.depth_maps_patches(bad)
