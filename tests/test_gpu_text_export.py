"""pmvs_loop_text / pmvs_text_patches: the .ply / .patch / .pset text formatted on the device.  The
oracle of every comparison is the path that existed before them: the export arrays of the same records
and flags written to a file by the reference-pinned host writers (pmvs_write_ply / _patches / _pset,
tests/test_io_pinning.py).  Every comparison is byte for byte."""
import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded (see test_gpu_loop_export.py)

from test_gpu_loop_export import crafted_records
from text_cases import SPECIALS, number_set

pytestmark = pytest.mark.gpu

TAB = [10, 3, 1 << 26, 0, 22, (1 << 26) - 1]  # a non-identity index2image for 6 views, numbers up to 2^26
EINVAL = "pmvs status 1:"
KINDS = ("ply", "patch", "pset")


def kind_id(P, kind):
    return {"ply": P.TEXT_PLY, "patch": P.TEXT_PATCH, "pset": P.TEXT_PSET}[kind]


def host_text(P, exp, kind, path):
    """The file the host writers write from export arrays."""
    path = str(path)
    if kind == "ply":
        P.write_ply(path, exp["fields"], exp["colors"])
    elif kind == "pset":
        P.write_pset(path, exp["fields"])
    else:
        io, vo = exp["image_off"], exp["vimage_off"]
        images = [exp["image_ids"][io[r]:io[r + 1]].tolist() for r in range(len(io) - 1)]
        vimages = [exp["vimage_ids"][vo[r]:vo[r + 1]].tolist() for r in range(len(vo) - 1)]
        P.write_patches(path, exp["fields"], images, vimages)
    with open(path, "rb") as f:
        return f.read()


def adversarial_records(P):
    """test_gpu_loop_export.py's 200 crafted records (coordinates inside every image; lists of 1 and 128
    images, 0 and 128 vimages) with the formatter's hard floats in normal, ncc, dscale and ascale."""
    recs, _ = crafted_records(P)
    rng = np.random.default_rng(7)
    hard = np.concatenate([SPECIALS, -SPECIALS[7:], np.float32([0.100040435791015625, 100000.5, 100001.5, 999999.5]),
                           rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    n = len(recs)
    take = lambda k: hard[(np.arange(n) * 7 + k) % len(hard)]  # noqa: E731
    for j in range(4):
        recs["normal"][:, j] = take(j)
    recs["ncc"], recs["dscale"], recs["ascale"] = take(4), take(5), take(6)
    assert recs["num_images"].min() == 1 and recs["num_images"].max() == 128
    assert recs["num_vimages"].min() == 0 and recs["num_vimages"].max() == 128
    return recs


@pytest.fixture(scope="module")
def crafted(gpu_available):
    import pmvs_amd as P
    inp, _ = P.synth_scene(6, 320, 240, level=1, num_targets=4)
    g = P.Scene(inp)
    yield P, g, adversarial_records(P)
    g.close()


@pytest.fixture(scope="module")
def looped(gpu_available):
    """The loop result of test_gpu_loop_export.py's loop case, left on the device."""
    import pmvs_amd as P
    inp, p = P.synth_scene(6, 480, 360, level=1, supersample=2, num_targets=4)
    g = P.Scene(inp)
    cands = P.synth_candidates(p, inp.projections, 300, seed=3)
    r, _ = g.refine_batch(cands)
    n, _ = g.run_loop(P.patches_from_refined(r), inp.threshold, iterations=2, wave=256, fetch=False)
    yield P, g, n
    g.close()


@pytest.mark.parametrize("precision", [6, 17])
def test_format_number_set_on_device(gpu_available, precision):
    import pmvs_amd as P
    x = number_set()
    got = P.selftest_format(precision, x, device=0)
    want = P.selftest_format(precision, x, device=-1)
    bad = [(hex(int(b)), g, w) for b, g, w in zip(x.view(np.uint32), got, want) if g != w]
    assert not bad, (len(bad), bad[:10])


@pytest.mark.parametrize("writer_order", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_text_patches_crafted(crafted, tmp_path, kind, writer_order):
    P, g, recs = crafted
    exp = g.export_patches(recs, writer_order=writer_order, index2image=TAB)
    want = host_text(P, exp, kind, tmp_path / "want")
    if kind != "pset":
        assert b"nan" in want and b"inf" in want and b"e-45" in want  # the hard floats reach the file
    got = g.text_patches(recs, kind_id(P, kind), writer_order=writer_order, index2image=TAB)
    assert got.dtype == np.uint8 and got.tobytes() == want
    dv = g.text_patches(recs, kind_id(P, kind), writer_order=writer_order, index2image=TAB, device=True)
    assert dv.is_cuda and dv.device.index == g.device and dv.dtype == torch.uint8
    assert dv.cpu().numpy().tobytes() == want


@pytest.mark.parametrize("kind", KINDS)
def test_loop_text_matches_host_writers(looped, tmp_path, kind):
    P, g, n = looped
    h = g.loop_hash()
    for writer_order in (True, False):
        exp = g.loop_export(writer_order=writer_order, index2image=TAB)
        want = host_text(P, exp, kind, tmp_path / "want")
        got = g.loop_text(kind_id(P, kind), writer_order=writer_order, index2image=TAB)
        assert got.tobytes() == want, writer_order
    dv = g.loop_text(kind_id(P, kind), writer_order=False, index2image=TAB, device=True)
    assert dv.is_cuda and dv.cpu().numpy().tobytes() == want
    assert n > 1000 and g.loop_hash() == h  # the text changes nothing in the model


def test_loop_text_does_not_consume(looped):
    """Runs after the cases above: the result is still there, loop_fetch takes it, then there is none."""
    P, g, n = looped
    assert len(g.loop_text(P.TEXT_PSET)) > 0
    model = g.loop_fetch(n)
    assert len(model) == n and int(model["num_images"].min()) >= 1
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.loop_text(P.TEXT_PLY)


@pytest.mark.parametrize("kind", KINDS)
def test_text_boundaries(crafted, tmp_path, kind):
    import ctypes as C
    P, g, recs = crafted
    k = kind_id(P, kind)
    # no patches: the header alone (the .pset has none)
    empty = {"fields": np.zeros((0, 11), np.float32), "colors": np.zeros((0, 3), np.int32),
             "image_off": np.zeros(1, np.int64), "vimage_off": np.zeros(1, np.int64),
             "image_ids": np.zeros(0, np.int32), "vimage_ids": np.zeros(0, np.int32)}
    want0 = host_text(P, empty, kind, tmp_path / "empty")
    assert len(want0) == {"ply": 261, "patch": 10, "pset": 0}[kind]  # 13 lines, "PATCHES\n0\n", nothing
    for device in (False, True):
        got0 = g.text_patches(recs[:0], k, index2image=TAB, device=device)
        assert bytes(got0.cpu().numpy() if device else got0) == want0
    # a size query, then the exact capacity; one byte less fails with *bytes set
    want = host_text(P, g.export_patches(recs[:70], index2image=TAB), kind, tmp_path / "want")
    pa = np.ascontiguousarray(recs[:70], P.PATCH_DTYPE)
    tab = np.asarray(TAB, np.int32)
    size = C.c_int64(-1)
    call = lambda out, cap: g.lib.pmvs_text_patches(g.handle, pa.ctypes.data, len(pa), k, P.EXPORT_WRITER_ORDER,  # noqa: E731
                                                    tab.ctypes.data, out, cap, C.byref(size))
    assert call(None, 0) == 0 and size.value == len(want)
    buf = np.full(len(want) + 8, 0xAA, np.uint8)
    size.value = -1
    assert call(buf.ctypes.data, len(want)) == 0 and size.value == len(want)
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
    buf[:] = 0xAA
    size.value = -1
    assert call(buf.ctypes.data, len(want) - 1) == 1 and size.value == len(want)
    assert (buf == 0xAA).all()
    # a caller's buffer, larger than the text
    out = np.zeros(len(want) + 100, np.uint8)
    got = g.text_patches(recs[:70], k, index2image=TAB, out=out)
    assert got.tobytes() == want and np.shares_memory(got, out)


def test_text_errors(crafted):
    P, g, recs = crafted
    with pytest.raises(P.PmvsError, match=EINVAL):   # no run_loop on this scene
        g.loop_text(P.TEXT_PLY)
    bad = recs[:4].copy()
    bad["num_images"][2] = 0
    with pytest.raises(P.PmvsError, match=EINVAL):   # validated as export_patches validates
        g.text_patches(bad, P.TEXT_PATCH)
    bad = recs[:4].copy()
    bad["images"][1, 0] = 6
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.text_patches(bad, P.TEXT_PLY)
    with pytest.raises(P.PmvsError, match=EINVAL):
        g.text_patches(recs[:4], 3)
