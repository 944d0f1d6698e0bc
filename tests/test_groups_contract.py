"""CPU model of the device label stage (pmvs_filter.hip, label_stage): the sets connected by mutual
edge pairs (i -> j and j -> i) are contracted by union-find with min-root hooking, and the fixpoint
slab[r] = min(r, slab of the sets with an edge into r), with the pointer jump slab[r] = slab[slab[r]],
runs on the contracted graph over the vertices that have an edge into another set.  Checked against
the reference's BFS labelling (test_groups_labels.bfs_labels) on random directed graphs whose share
of mutual edges runs from 0 to 1, with one-way chains and cycles added."""
import numpy as np

from test_groups_labels import bfs_labels


def contract_labels(n, adj):
    """Serial model of the kernels, in their order.  Returns (labels, root, residual list, sweeps)."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    targets = [set(a) for a in adj]
    for i in range(n):  # lab_hook_kernel
        for j in adj[i]:
            if j <= i or i not in targets[j]:
                continue
            ri, rj = find(i), find(j)
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
    root = [find(i) for i in range(n)]  # lab_flatten_kernel
    rlist = [i for i in range(n) if any(root[j] != root[i] for j in adj[i])]  # lab_cross / lab_residual
    slab = list(range(n))  # read at the roots only
    sweeps = 0
    changed = bool(rlist)
    while changed:  # lab_sweep_kernel
        changed = False
        sweeps += 1
        for i in rlist:
            ri = root[i]
            if slab[slab[ri]] < slab[ri]:
                slab[ri] = slab[slab[ri]]
                changed = True
            for j in adj[i]:
                rj = root[j]
                if rj != ri and slab[ri] < slab[rj]:
                    slab[rj] = slab[ri]
                    changed = True
    return [slab[root[i]] for i in range(n)], root, rlist, sweeps  # lab_assign_kernel


def random_graph(rng, n, p, mutual):
    """Directed edges with probability p each; a share `mutual` of them gets its reverse edge."""
    adj = [[] for _ in range(n)]
    for u in range(n):
        for v in np.nonzero(rng.random(n) < p)[0]:
            v = int(v)
            if v == u:
                continue
            adj[u].append(v)
            if rng.random() < mutual:
                adj[v].append(u)
    return adj


def add_chain(rng, adj, k, cycle):
    n = len(adj)
    if n < 2:
        return
    path = [int(v) for v in rng.permutation(n)[:max(2, min(k, n))]]
    for a, b in zip(path, path[1:]):
        adj[a].append(b)
    if cycle:
        adj[path[-1]].append(path[0])


def check(n, adj, what):
    want = bfs_labels(n, adj)
    got, root, rlist, _ = contract_labels(n, adj)
    assert got == want, what
    members = {}
    for i, r in enumerate(root):
        members.setdefault(r, []).append(i)
    for r, m in members.items():
        assert r == min(m), what  # every set's root is its minimum member
    for i in range(n):
        assert got[i] == root[got[i]], what  # a label is the root of a set


def test_contraction_gives_bfs_labels():
    rng = np.random.default_rng(15)
    for trial in range(600):
        n = int(rng.integers(1, 70))
        p = float(rng.uniform(0.0, 0.12))
        mutual = [0.0, 1.0, float(rng.uniform(0.0, 1.0))][trial % 3]
        adj = random_graph(rng, n, p, mutual)
        if trial % 4 == 1:
            add_chain(rng, adj, int(rng.integers(2, 30)), cycle=False)
        if trial % 4 == 2:
            add_chain(rng, adj, int(rng.integers(2, 30)), cycle=True)
        check(n, adj, (trial, n, mutual))


def test_contraction_edge_cases():
    check(1, [[]], "single")
    check(2, [[], []], "two isolated")
    check(3, [[0, 1, 1], [0, 0], [2]], "self-edges and duplicates")
    n = 50
    check(n, [[i - 1] if i else [] for i in range(n)], "one-way chain downwards")
    check(n, [[i + 1] if i + 1 < n else [] for i in range(n)], "one-way chain upwards")
    check(n, [[(i + 1) % n] for i in range(n)], "one-way cycle")
    check(n, [[(i + 1) % n, (i - 1) % n] for i in range(n)], "mutual ring")


def test_fully_mutual_graph_needs_no_sweep():
    rng = np.random.default_rng(3)
    adj = random_graph(rng, 60, 0.05, 1.0)
    got, _, rlist, sweeps = contract_labels(60, adj)
    assert got == bfs_labels(60, adj)
    assert rlist == [] and sweeps == 0
