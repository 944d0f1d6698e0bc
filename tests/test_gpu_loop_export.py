"""pmvs_loop_export / pmvs_export_patches: the model as compact, writer-ordered arrays produced on the
device.  The oracle of every comparison is the path that existed before them: the fetched 1608-byte
records, a numpy restatement of pmvs2's collectPatches(1) key with a stable argsort, and
Scene.patch_colors for the colours.  Every array is compared for exact equality."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as bench.py does: a torch build that ships
#               its own HIP runtime finds no device when the system's runtime was opened first

pytestmark = pytest.mark.gpu

NAMES = ("fields", "colors", "image_off", "image_ids", "image_idx", "vimage_off", "vimage_ids", "source")
TAB = [10, 3, 7, 0, 22, 5]  # a non-identity index2image for 6 views
EINVAL = "pmvs status 1:"


def order_keys(model, inp):
    """pmvs2's key of collectPatches(1): bt = the lowest view index below tnum in images (first
    position k0), (bt << 40) + grids[k0][1] * gwidth(bt) + grids[k0][0]; no target image: last."""
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


def host_export(g, inp, model, writer_order, index2image):
    """The arrays of pmvs_export_buffers from host records, as pmvs2 made them before the export."""
    n = len(model)
    order = np.argsort(order_keys(model, inp), kind="stable") if writer_order else np.arange(n)
    m = model[order]
    tab = np.arange(len(inp.images)) if index2image is None else np.asarray(index2image)
    lists = [[int(v) for v in q["images"][:q["num_images"]]] for q in m]
    vlists = [[int(v) for v in q["vimages"][:q["num_vimages"]]] for q in m]
    idx = np.array([v for x in lists for v in x], np.int32)
    vidx = np.array([v for x in vlists for v in x], np.int32)
    return {
        "fields": np.concatenate([m["coord"], m["normal"], m["ncc"].reshape(-1, 1), m["dscale"].reshape(-1, 1),
                                  m["ascale"].reshape(-1, 1)], 1).astype(np.float32),
        "colors": g.patch_colors(m["coord"], lists),
        "image_off": np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64),
        "image_ids": tab[idx].astype(np.int32),
        "image_idx": idx,
        "vimage_off": np.concatenate([[0], np.cumsum([len(x) for x in vlists])]).astype(np.int64),
        "vimage_ids": tab[vidx].astype(np.int32),
        "source": order.astype(np.int32),
    }


def assert_same(got, want, names=NAMES):
    assert set(got) == set(names)
    for k in names:
        a = np.asarray(got[k])
        assert a.dtype == want[k].dtype and a.shape == want[k].shape, k
        assert a.tobytes() == want[k].tobytes(), k


def crafted_records(P):
    """200 hand-made records for a 6-view scene with 4 targets (views 4 and 5 are not targets), cell
    grids 80 x 60: random lists, plus the edges listed in the comments below."""
    rng = np.random.default_rng(20260)
    n = 200
    r = np.zeros(n, P.PATCH_DTYPE)
    r["coord"][:, :3] = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)  # projects well inside every image
    r["coord"][:, 3] = 1.0
    r["normal"][:, :3] = rng.normal(size=(n, 3)).astype(np.float32)
    for f in ("ncc", "dscale", "ascale", "tmp"):
        r[f] = rng.uniform(0, 1, n).astype(np.float32)

    def set_images(i, views, cells=None):
        k = len(views)
        r["num_images"][i] = k
        r["images"][i, :k] = views
        r["grids"][i, :k, 0] = rng.integers(0, 80, k) if cells is None else [c[0] for c in cells]
        r["grids"][i, :k, 1] = rng.integers(0, 60, k) if cells is None else [c[1] for c in cells]

    def set_vimages(i, views):
        k = len(views)
        r["num_vimages"][i] = k
        r["vimages"][i, :k] = views
        r["vgrids"][i, :k, 0] = rng.integers(0, 80, k)
        r["vgrids"][i, :k, 1] = rng.integers(0, 60, k)

    for i in range(n):
        set_images(i, rng.integers(0, 6, rng.integers(1, 9)))
        set_vimages(i, rng.integers(0, 4, rng.integers(0, 5)))
    # groups of records that share (bt, cell), far apart in the array: ties must keep model order; the
    # lowest target is at position 1, not images[0]
    groups = {(0, (7, 3)): [5, 61, 120, 190], (2, (79, 59)): [6, 64, 127, 189], (3, (0, 0)): [9, 70, 134, 188, 199],
              (1, (40, 30)): [0, 99, 198]}
    for (bt, cell), members in groups.items():
        for i in members:
            set_images(i, [5, bt, 4], [(11, 13), cell, (1, 2)])
    # the lowest target occurs twice: its first position counts
    set_images(12, [3, 1, 5, 1], [(1, 1), (20, 21), (2, 2), (50, 51)])
    # no target image at all: last, in model order
    set_images(17, [4, 5])
    set_images(150, [5])
    set_images(151, [5, 4, 4])
    # no vimages; full lists (view indexes repeat for the purpose); lengths around the wavefront size
    set_vimages(3, [])
    set_vimages(17, [])
    set_images(40, rng.integers(0, 6, 128))
    set_vimages(41, rng.integers(0, 4, 128))
    for i, k in ((80, 63), (81, 64), (82, 65)):
        set_images(i, rng.integers(0, 6, k))
    for i, k in ((83, 63), (84, 64), (85, 65)):
        set_vimages(i, rng.integers(0, 4, k))
    return r, groups


@pytest.fixture(scope="module")
def crafted(gpu_available):
    import pmvs_amd as P
    inp, _ = P.synth_scene(6, 320, 240, level=1, num_targets=4)
    g = P.Scene(inp)
    recs, groups = crafted_records(P)
    yield P, g, inp, recs, groups
    g.close()


@pytest.fixture(scope="module")
def looped(gpu_available):
    """One loop result left on the device (the shape of test_gpu_loop_hash.py, 4 of 6 views targets)."""
    import pmvs_amd as P
    inp, p = P.synth_scene(6, 480, 360, level=1, supersample=2, num_targets=4)
    g = P.Scene(inp)
    cands = P.synth_candidates(p, inp.projections, 300, seed=3)
    r, _ = g.refine_batch(cands)
    seeds = P.patches_from_refined(r)
    n, _ = g.run_loop(seeds, inp.threshold, iterations=2, wave=256, fetch=False)
    yield P, g, inp, n
    g.close()


def check_crafted_edges(inp, recs, groups):
    """The hand-made records contain what they are meant to test (checked on the host restatement)."""
    key = order_keys(recs, inp)
    order = np.argsort(key, kind="stable")
    for members in groups.values():
        assert len(members) >= 3 and len(set(key[members])) == 1
        pos = [int(np.nonzero(order == i)[0][0]) for i in members]
        assert pos == sorted(pos) and pos[-1] - pos[0] == len(members) - 1  # adjacent, in model order
    none = np.nonzero(key == np.iinfo(np.int64).max)[0]  # no target image: last, in model order
    assert {17, 150, 151} <= set(none) and list(order[-len(none):]) == list(none)
    assert recs["num_images"].max() == 128 and recs["num_vimages"].max() == 128 and recs["num_vimages"].min() == 0
    assert {63, 64, 65} <= set(recs["num_images"]) and {63, 64, 65} <= set(recs["num_vimages"])
    lowest_first = [min([v for v in q["images"][:q["num_images"]] if v < 4], default=-1) == q["images"][0] for q in recs]
    assert not all(lowest_first)


@pytest.mark.parametrize("writer_order", [True, False])
@pytest.mark.parametrize("index2image", [TAB, None])
def test_export_patches_crafted(crafted, writer_order, index2image):
    P, g, inp, recs, groups = crafted
    check_crafted_edges(inp, recs, groups)
    got = g.export_patches(recs, writer_order=writer_order, index2image=index2image)
    want = host_export(g, inp, recs, writer_order, index2image)
    assert_same(got, want)
    if not writer_order:
        assert np.array_equal(got["source"], np.arange(len(recs)))


@pytest.mark.parametrize("n", [0, 1])
def test_export_patches_tiny(crafted, n):
    P, g, inp, recs, _ = crafted
    for writer_order in (True, False):
        got = g.export_patches(recs[40:40 + n], writer_order=writer_order, index2image=TAB)
        assert_same(got, host_export(g, inp, recs[40:40 + n], writer_order, TAB))
        assert got["image_off"][0] == 0 and got["vimage_off"][0] == 0 and len(got["image_off"]) == n + 1


@pytest.mark.parametrize("names", [("fields",), ("colors",), tuple(k for k in NAMES if k != "colors")])
def test_export_patches_null_pointers(crafted, names):
    """NULL pointers skip their arrays and leave the others as they are."""
    P, g, inp, recs, _ = crafted
    want = host_export(g, inp, recs, True, TAB)
    assert_same(g.export_patches(recs, index2image=TAB, arrays=names), want, names)


def test_loop_export_matches_fetched_model(looped):
    P, g, inp, n = looped
    h = g.loop_hash()
    sizes = g.loop_export_sizes()
    wr = g.loop_export(writer_order=True, index2image=TAB)
    mo = g.loop_export(writer_order=False, index2image=None)
    assert g.loop_hash() == h            # the export changes nothing in the model
    assert g.loop_export_sizes() == sizes  # and does not consume it
    # device mode (torch tensors on the scene's device) gives the host-mode arrays
    dv = g.loop_export(writer_order=True, index2image=TAB, device=True)
    assert all(t.is_cuda and t.device.index == g.device for t in dv.values())
    assert_same({k: t.cpu().numpy() for k, t in dv.items()}, wr)

    model = g.loop_fetch(n)              # still there after the exports
    assert n > 1000 and len(model) == n
    assert sizes == {"patches": n, "image_entries": int(model["num_images"].sum()),
                     "vimage_entries": int(model["num_vimages"].sum())}
    key = order_keys(model, inp)
    assert len(np.unique(key)) < n       # cells hold several patches: the stable-tie path is exercised
    assert_same(wr, host_export(g, inp, model, True, TAB))
    assert_same(mo, host_export(g, inp, model, False, None))
    assert np.array_equal(mo["source"], np.arange(n))
    # the fetch consumed the result
    for call in (g.loop_export, g.loop_export_sizes):
        with pytest.raises(P.PmvsError, match=EINVAL):
            call()


def test_export_errors(crafted):
    P, g, inp, recs, _ = crafted
    with pytest.raises(P.PmvsError, match=EINVAL):   # no run_loop on this scene yet
        g.loop_export()
    bad = recs[:4].copy()
    bad["num_images"][2] = 0
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.export_patches(bad)
    bad = recs[:4].copy()
    bad["images"][1, 0] = 6                          # view index >= num_views
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.export_patches(bad)
