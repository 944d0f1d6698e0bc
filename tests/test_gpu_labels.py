"""GPU test of filterSmallGroups' label stage (pmvs_filter.hip, label_stage) through
pmvs_selftest_labels: label for label against the reference's BFS (test_groups_labels.bfs_labels) on
the smallest graphs at which the kernels can go wrong, and twice in a row with identical results."""
import functools

import numpy as np
import pytest

from test_groups_labels import bfs_labels

pytestmark = pytest.mark.gpu


def csr(adj):
    off = np.zeros(len(adj) + 1, np.int32)
    off[1:] = np.cumsum([len(a) for a in adj])
    edges = np.array([v for a in adj for v in a], np.int32)
    return off, edges


def ring(n):
    return [[(i + 1) % n, (i - 1) % n] for i in range(n)]


def grid_adj(w, h, base=0):
    adj = []
    for y in range(h):
        for x in range(w):
            a = []
            if x > 0: a.append(base + y * w + x - 1)
            if x + 1 < w: a.append(base + y * w + x + 1)
            if y > 0: a.append(base + (y - 1) * w + x)
            if y + 1 < h: a.append(base + (y + 1) * w + x)
            adj.append(a)
    return adj


def two_grids(forward):
    adj = grid_adj(40, 40) + grid_adj(40, 40, base=1600)
    if forward:
        adj[1599].append(1600)
    else:
        adj[1600].append(1599)
    return adj


def big_grid():
    """A mutual 300 x 300 grid, 5 % of the edges made one-way and 1 % of the vertices isolated."""
    rng = np.random.default_rng(300)
    w = 300
    n = w * w
    adj = grid_adj(w, w)
    isolated = rng.random(n) < 0.01
    for u in range(n):
        adj[u] = [] if isolated[u] else [v for v in adj[u] if not isolated[v] and rng.random() >= 0.05]
    return adj


def random_graph(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(2, 5001))
    deg = float(rng.uniform(0.3, 4.0))
    mutual = float(rng.uniform(0.0, 1.0))
    m = int(n * deg)
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)
    adj = [[] for _ in range(n)]
    back = rng.random(m) < mutual
    for u, v, b in zip(src.tolist(), dst.tolist(), back.tolist()):
        adj[u].append(v)
        if b:
            adj[v].append(u)
    return adj


CASES = {
    "n1": lambda: [[]],
    "n2": lambda: [[], []],
    "ring65": lambda: ring(65),
    "ring257": lambda: ring(257),
    "chain_down": lambda: [[i - 1] if i else [] for i in range(2001)],  # 2000 -> ... -> 0
    "chain_up": lambda: [[i + 1] if i < 2000 else [] for i in range(2001)],  # 0 -> ... -> 2000: nothing to contract
    "cycle300": lambda: [[(i + 1) % 300] for i in range(300)],
    "grids_forward": lambda: two_grids(True),
    "grids_backward": lambda: two_grids(False),
    "grid300": big_grid,
    "dups_self": lambda: [[0, 1, 1, 2], [0, 0, 1], [2, 2], [3], [3, 2, 2]],
}
CASES.update({f"random{k}": functools.partial(random_graph, k) for k in range(20)})


@functools.lru_cache(maxsize=None)
def case(name):
    adj = CASES[name]()
    return adj, tuple(bfs_labels(len(adj), adj))


@pytest.mark.parametrize("name", list(CASES))
def test_labels_match_bfs(gpu_available, name):
    import pmvs_amd as P
    adj, want = case(name)
    off, edges = csr(adj)
    lab, stats = P.selftest_labels(off, edges)
    print(name, len(adj), len(edges), stats)
    assert lab.tolist() == list(want)
    lab2, stats2 = P.selftest_labels(off, edges)
    assert np.array_equal(lab, lab2)
    assert stats2["supernodes"] == stats["supernodes"] and stats2["residual"] == stats["residual"]
    n = len(adj)
    assert 1 <= stats["supernodes"] <= n and 0 <= stats["residual"] <= n
    if stats["residual"] == 0:
        assert stats["sweeps"] == 0


def test_contraction_statistics(gpu_available):
    """What the stage reports: a mutual ring is one set with nothing left over; a one-way chain keeps
    every vertex its own set and every vertex but the last has an edge into another set."""
    import pmvs_amd as P
    _, stats = P.selftest_labels(*csr(ring(257)))
    assert stats == {"supernodes": 1, "residual": 0, "sweeps": 0}
    _, stats = P.selftest_labels(*csr(case("chain_up")[0]))
    assert stats["supernodes"] == 2001 and stats["residual"] == 2000 and stats["sweeps"] >= 2
    _, stats = P.selftest_labels(*csr(case("grids_forward")[0]))
    assert stats["supernodes"] == 2 and stats["residual"] == 1


def test_invalid_graph_rejected(product_lib):
    import pmvs_amd as P
    with pytest.raises(P.PmvsError):
        P.selftest_labels(np.array([0, 1], np.int32), np.array([1], np.int32))  # target outside the graph
    with pytest.raises(P.PmvsError):
        P.selftest_labels(np.array([0, 2, 1], np.int32), np.array([0, 1], np.int32))  # offsets decrease
