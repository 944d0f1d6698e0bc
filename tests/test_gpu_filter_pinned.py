"""The device against the reference's own records: tests/golden/filter_pin.npz holds a patch set and what
the reference's object code (filter.cpp, patchOrganizerS.cpp compiled unmodified, oracle/_ref/filter)
computed for it in CFilter::setDepthMapsVGridsVPGridsAddPatchV(0) at depth 0 -- no restatement stands
between the device and these numbers.  Only the fixture is read.
  * depth maps: pmvs_depth_maps_patches in model order gives the reference's _dpgrids winner in every
    cell of every target (48 exact coordinate copies far apart in the array: the earlier row wins; rows
    outside every grid; rows on border cells; one target of another size), and OpticalAxis * coord of the
    winner bit for bit;
  * visible images: after one device filter pass at depth 0 over the plain rows, every surviving row
    carries exactly the _vimages / _vgrids the reference's setVImagesVGrids gave it.  At depth 0 isVisible
    accepts every in-grid cell, so a row's lists depend on no other row, filterExact keeps every target
    image, and the later additive rebuilds have nothing to add.
The gains of filterOutside are not in the fixture: computeGain calls the three-argument isNeighbor and
through it COptim::getUnit, which the reference recipe cannot reach."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- before libpmvs_amd.so is loaded, as tests/test_gpu_depth_maps.py does

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


@pytest.fixture(scope="module")
def pinned(gpu_available):
    import make_golden as M
    import pmvs_amd as P
    g = np.load(os.path.join(ROOT, "tests", "golden", "filter_pin.npz"))
    inp, _ = M.filter_pin_scene()
    sc = P.Scene(inp)
    dims, off = sc.depth_map_layout()
    assert np.array_equal(dims, g["grid_dims"][:inp.num_targets]) and off[-1] == len(g["ref_dm_winner"])
    yield g, sc, M.filter_pin_records(g)
    sc.close()


def test_depth_maps_equal_reference_records(pinned):
    g, sc, recs = pinned
    got = sc.depth_maps_patches(recs, writer_order=False)
    win = g["ref_dm_winner"]
    bad = np.flatnonzero(got["patch"] != win)
    assert len(bad) == 0, (len(bad), bad[:10], got["patch"][bad[:10]], win[bad[:10]])
    assert got["depth"].dtype == np.float32
    assert np.array_equal(got["depth"].view(np.uint32), g["ref_dm_depth"].view(np.uint32))
    filled = win >= 0
    assert np.array_equal(got["normal"][filled], recs["normal"][win[filled], :3])
    assert np.array_equal(got["ncc"][filled], recs["ncc"][win[filled]])
    pairs = g["copies"]  # the fixture's ties, once more from the device's side
    assert np.isin(pairs[:, 0], got["patch"]).sum() >= 40 and not np.isin(pairs[:, 1], got["patch"]).any()


def test_depth0_pass_keeps_reference_vimages(pinned):
    g, sc, recs = pinned
    n = int(g["params"][10])
    out, keep, st = sc.filter_run(recs[:n])  # a fresh scene is at depth 0
    assert st["removed_outside"] > 0 and keep.sum() > n // 2
    assert (keep[recs["fix"][:n] == 1] == 1).all() and (recs["fix"][:n] == 1).any()
    voff = np.concatenate([[0], np.cumsum(g["ref_dm_vcount"])])
    vl = g["ref_dm_vlists"]
    rows = np.flatnonzero(keep == 1)
    assert (g["ref_dm_vcount"][rows] > 0).sum() >= 1000
    for i in rows:
        r = vl[voff[i]:voff[i + 1]]
        m = int(out["num_vimages"][i])
        assert m == len(r), i
        assert np.array_equal(out["vimages"][i][:m], r[:, 0]) and np.array_equal(out["vgrids"][i][:m], r[:, 1:]), i
