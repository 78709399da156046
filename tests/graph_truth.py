"""Hand-built graphs for the clustering kernels, and what the reference makes of them.

A graph is (counts u64[U], pairs i64[E, 2]): the read count of every leaf and a duplicate-free list of
linked leaves (a != b).  Leaves are walked in index order (src/humid.cc:176-189 with walk order = index),
neighbour lists are scanned in the order to_csr() gives them, so both orders are inputs of a case.

Three things live here, none of which touches a GPU:
  * builders: topologies, count patterns, disjoint_union / relabel / to_csr;
  * the truth, stated twice: oracle_clusters (the C oracle over a CSR, explicit stack) and
    reference_clusters_py (the literal recursive loop of src/cluster.cc:39-80 in plain Python, for graphs small
    enough for Python recursion);
  * joined_component_sizes: which leaves the device treats as ONE component (a statement about inputs,
    kernels_graph.hip.h joins_for_clustering), and CASES, the case table of tests/test_gpu_cluster_graphs.py,
    which tests/test_graph_truth_host.py checks for components at every size where the device changes form.
"""
from collections import deque

import numpy as np

from oracle import pyoracle as orc

U32_MAX = 0xFFFFFFFF
ORDERS = ("ascending", "descending", "link", ("shuffled", 7))


# ------------------------------------------------------------------------------------------
# topologies: pairs over k leaves
# ------------------------------------------------------------------------------------------
def _pairs(a, b):
    a, b = np.asarray(a, np.int64).ravel(), np.asarray(b, np.int64).ravel()
    return np.stack([a, b], axis=1) if len(a) else np.zeros((0, 2), np.int64)


def path(k):
    i = np.arange(max(k - 1, 0))
    return _pairs(i, i + 1)


def ring(k):
    return np.concatenate([path(k), _pairs([k - 1], [0])]) if k >= 3 else path(k)


def star(k, hub=0):
    """hub plus k - 1 leaves"""
    others = np.arange(k)[np.arange(k) != hub]
    return _pairs(np.full(len(others), hub), others)


def clique(k):
    a, b = np.triu_indices(k, 1)
    return _pairs(a, b)


def complete_bipartite(k, left=None):
    """K(left, k - left): leaves 0 .. left-1 against the rest (left = k // 2 by default)"""
    left = k // 2 if left is None else min(left, k)
    a, b = np.meshgrid(np.arange(left), np.arange(left, k), indexing="ij")
    return _pairs(a, b)


def binary_tree(k):
    i = np.arange(1, k)
    return _pairs((i - 1) // 2, i)


def caterpillar(k):
    """a path of ceil(k / 2) leaves with one pendant leaf per node (the last node goes without when k is odd)"""
    s = (k + 1) // 2
    i = np.arange(k - s)
    return np.concatenate([path(s), _pairs(i, s + i)])


def ladder(k):
    """two paths (0 .. h-1 and h .. k-1, h = ceil(k / 2)) joined rung by rung"""
    h = (k + 1) // 2
    i = np.arange(k - h)
    rail_b = path(k - h) + h
    return np.concatenate([path(h), rail_b, _pairs(i, h + i)])


def random_sparse(k, avg_degree=3.0, seed=0):
    """a random spanning tree (so the k leaves are one connected component) plus random links up to about
    avg_degree * k / 2 pairs, in random order and orientation"""
    rng = np.random.default_rng(seed)
    if k < 2:
        return _pairs([], [])
    child = np.arange(1, k)
    parent = (rng.random(k - 1) * child).astype(np.int64)          # parent[i] < child[i]
    extra = max(int(round(avg_degree * k / 2)) - (k - 1), 0)
    xa, xb = rng.integers(0, k, size=2 * extra), rng.integers(0, k, size=2 * extra)
    lo = np.concatenate([parent, np.minimum(xa, xb)])
    hi = np.concatenate([child, np.maximum(xa, xb)])
    keep = lo != hi
    key = lo[keep] * k + hi[keep]
    _, first = np.unique(key, return_index=True)                    # the tree comes first: it survives
    first = np.sort(first)[:k - 1 + extra]
    p = _pairs(lo[keep][first], hi[keep][first])
    flip = rng.random(len(p)) < 0.5
    p[flip] = p[flip][:, ::-1]
    return p[rng.permutation(len(p))]


# ------------------------------------------------------------------------------------------
# count patterns: factories of f(k, pairs) -> u64[k]
# ------------------------------------------------------------------------------------------
def _rows(k, pairs):
    nb = [[] for _ in range(k)]
    for a, b in np.asarray(pairs).tolist():
        nb[a].append(b)
        nb[b].append(a)
    return nb


def _bfs(k, pairs, hub=0):
    """(order of discovery, parent or -1, depth) of a breadth-first walk from hub, restarted at the lowest
    unreached leaf until every leaf is reached"""
    nb = _rows(k, pairs)
    parent, depth, order = [-2] * k, [0] * k, []
    for root in [hub] + list(range(k)):
        if root >= k or parent[root] != -2:
            continue
        parent[root] = -1
        q = deque([root])
        while q:
            u = q.popleft()
            order.append(u)
            for v in nb[u]:
                if parent[v] == -2:
                    parent[v], depth[v] = u, depth[u] + 1
                    q.append(v)
    return order, parent, depth


def equal(c):
    return lambda k, pairs: np.full(k, c, np.uint64)


def alternating(a=1, b=2):
    """a on even indices, b on odd ones"""
    return lambda k, pairs: np.where(np.arange(k) % 2 == 0, a, b).astype(np.uint64)


def doubling():
    """1, 2, 4, ... by index, capped at 2^31"""
    return lambda k, pairs: (np.uint64(1) << np.minimum(np.arange(k), 31).astype(np.uint64))


def halving_from_hub(hub=0):
    """2^T at the hub and half of it with every step away from it, never below 1 (T = the depth of the walk, at
    most 31); what the hub does not reach is walked from its own lowest leaf in the same way"""
    def f(k, pairs):
        _, _, depth = _bfs(k, pairs, hub)
        top = min(max(depth), 31)
        return np.asarray([1 << max(top - d, 0) for d in depth], np.uint64)
    return f


def boundary():
    """every link of a breadth-first tree sits on the edge of atLeastDouble_: the larger count is exactly 2b, 2b - 1
    or 2b + 1 for the smaller count b, in turn.  Leaves at even depth are the large ones."""
    def f(k, pairs):
        order, parent, depth = _bfs(k, pairs, 0)
        c = [0] * k
        for j, u in enumerate(order):
            p = parent[u]
            if p < 0:
                c[u] = 100
            elif depth[u] % 2 == 1:                       # small under a large parent P: P = 2b, 2b - 1 or 2b + 1
                P = c[p]
                c[u] = P // 2 if P % 2 == 0 else ((P + 1) // 2 if (j // 2) % 2 == 0 else (P - 1) // 2)
            else:                                         # large under a small parent b
                d = (0, -1, 1)[(j // 2) % 3]
                if c[p] < 20:
                    d = 1
                elif c[p] > 1 << 20:
                    d = -1
                c[u] = 2 * c[p] + d
        return np.asarray(c, np.uint64)
    return f


HUGE_VALUES = (0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF, 1, 2)


def huge(seed=0):
    """values around 2^31 and 2^32 - 1: 2 * b leaves 32 bits, and a few such leaves make a cluster of more
    than 2^32 reads"""
    def f(k, pairs):
        rng = np.random.default_rng(seed)
        return np.asarray(HUGE_VALUES, np.uint64)[rng.integers(0, len(HUGE_VALUES), size=k)]
    return f


def with_zeros(seed=0):
    """random counts with some leaves of count 0, never two of them linked"""
    def f(k, pairs):
        rng = np.random.default_rng(seed)
        c = rng.integers(1, 9, size=k).astype(np.uint64)
        nb = _rows(k, pairs)
        for u in rng.permutation(k)[:(k + 2) // 3].tolist():
            if all(c[v] != 0 for v in nb[u]):
                c[u] = 0
        return c
    return f


def random_geometric(seed=0):
    """geometrically distributed counts (mean 5): many ties and near-ties, a few leaves far above the rest"""
    def f(k, pairs):
        return np.random.default_rng(seed).geometric(0.2, size=k).astype(np.uint64)
    return f


def graph(topology, pattern, k, **kw):
    pairs = topology(k, **kw)
    return pattern(k, pairs), pairs


# ------------------------------------------------------------------------------------------
# combinators
# ------------------------------------------------------------------------------------------
def disjoint_union(graphs):
    counts, pairs, base = [], [], 0
    for c, p in graphs:
        counts.append(np.asarray(c, np.uint64))
        pairs.append(np.asarray(p, np.int64).reshape(-1, 2) + base)
        base += len(c)
    return np.concatenate(counts), np.concatenate(pairs)


def relabel(g, perm):
    """leaf i becomes leaf perm[i].  A random permutation interleaves the members of different components in
    walk order; the identity keeps them contiguous."""
    counts, pairs = g
    perm = np.asarray(perm, np.int64)
    assert np.array_equal(np.sort(perm), np.arange(len(counts)))
    out = np.empty_like(np.asarray(counts, np.uint64))
    out[perm] = counts
    return out, perm[np.asarray(pairs, np.int64).reshape(-1, 2)]


def reversed_labels(g):
    k = len(g[0])
    return relabel(g, np.arange(k)[::-1])


def shuffled_labels(g, seed):
    return relabel(g, np.random.default_rng(seed).permutation(len(g[0])))


def shuffled(seed):
    return ("shuffled", seed)


def to_csr(counts, pairs, order):
    """symmetric CSR (off u64[U + 1], idx u32[2 E]) with every row in the requested order: "ascending",
    "descending", "link" (the order link(a, b) calls in pair order would leave: tests/test_cluster.cc:11-14) or
    shuffled(seed)"""
    u = len(counts)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    src, dst = pairs.ravel(), pairs[:, ::-1].ravel()          # a0 b0 a1 b1 ... / b0 a0 b1 a1 ...
    if order == "link":
        o = np.argsort(src, kind="stable")
    elif order == "ascending":
        o = np.lexsort((dst, src))
    elif order == "descending":
        o = np.lexsort((-dst, src))
    elif isinstance(order, tuple) and order[0] == "shuffled":
        o = np.lexsort((np.random.default_rng(order[1]).random(len(src)), src))
    else:
        raise ValueError("unknown list order %r" % (order,))
    off = np.zeros(u + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(src, minlength=u), dtype=np.uint64)
    return off, dst[o].astype(np.uint32)


def csr_rows(off, idx):
    off = [int(x) for x in off]
    idx = np.asarray(idx).tolist()
    return [idx[off[i]:off[i + 1]] for i in range(len(off) - 1)]


# ------------------------------------------------------------------------------------------
# truth
# ------------------------------------------------------------------------------------------
def check_no_linked_zeros(counts, off, idx):
    """two linked leaves of count 0: maxNeighbour_ (src/cluster.cc:39-51) hops between them for ever, and so does the
    oracle.  Raise instead."""
    counts = np.asarray(counts, np.uint64)
    row = np.repeat(np.arange(len(counts)), np.diff(np.asarray(off, np.uint64)).astype(np.int64))
    bad = (counts[row] == 0) & (counts[np.asarray(idx, np.int64)] == 0)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError("leaves %d and %d are linked and both have count 0" % (int(row[k]), int(idx[k])))


def oracle_clusters(counts, off, idx, maximum):
    """findClusters of the C oracle over the CSR, lists in row order.
    Returns (leaf_cluster u32[U] in 1 .. C, size u64[C], max_count u64[C], max_leaf i64[C], C); max_leaf is -1 for a
    cluster whose leaves all have count 0 (updateMaxCount_ compares with >, src/cluster.cc:20-25)."""
    check_no_linked_zeros(counts, off, idx)
    g = orc.Graph(np.asarray(counts, np.uint64))
    g.append_csr(off, idx)
    nc = g.find_clusters(bool(maximum))
    lc, size, mc, ml = g.export(nc)
    return lc, size, mc, ml, nc


def reference_clusters_py(counts, nbrs, maximum):
    """The same definition once more, as the reference writes it: recursive maxNeighbour_ /
    assignDirectionalCluster_ / assignMaxCluster (src/cluster.cc:39-80) under the findClusters loop
    (src/humid.cc:176-189).  nbrs: one Python list of neighbours per leaf."""
    cnt = [int(c) for c in counts]
    n = len(cnt)
    for a in range(n):
        for b in nbrs[a]:
            if cnt[a] == 0 and cnt[b] == 0:
                raise ValueError("leaves %d and %d are linked and both have count 0" % (a, b))
    cluster = [0] * n
    size, max_count, max_leaf = [], [], []

    def at_least_double(a, b):
        return a >= 2 * b

    def assign_leaf(leaf, c):
        cluster[leaf] = c
        size[c - 1] += cnt[leaf]

    def update_max_count(leaf, c):
        if cnt[leaf] > max_count[c - 1]:
            max_leaf[c - 1] = leaf
            max_count[c - 1] = cnt[leaf]

    def max_neighbour(leaf):
        i = 0
        while i < len(nbrs[leaf]):
            nb = nbrs[leaf][i]
            i += 1
            if not cluster[nb] and at_least_double(cnt[nb], cnt[leaf]):
                leaf = nb
                i = 0
        return leaf

    def assign_directional_(leaf, c):
        assign_leaf(leaf, c)
        for nb in nbrs[leaf]:
            if not cluster[nb] and at_least_double(cnt[leaf], cnt[nb]):
                assign_directional_(nb, c)

    def assign_max(leaf, c):
        assign_leaf(leaf, c)
        update_max_count(leaf, c)
        for nb in nbrs[leaf]:
            if not cluster[nb]:
                assign_max(nb, c)

    next_id = 1
    for leaf in range(n):
        if cluster[leaf]:
            continue
        c = next_id
        next_id += 1
        size.append(0)
        max_count.append(0)
        max_leaf.append(-1)
        if maximum:
            assign_max(leaf, c)
        else:
            node = max_neighbour(leaf)
            update_max_count(node, c)
            assign_directional_(node, c)
    return (np.asarray(cluster, np.uint32), np.asarray(size, np.uint64), np.asarray(max_count, np.uint64),
            np.asarray(max_leaf, np.int64), next_id - 1)


def _union_roots(n, a, b):
    """host union-find over the pairs (a[i], b[i]): the smallest member of every component, per leaf.  Hooks every
    root under the smallest root it is linked to, then flattens, until no pair spans two roots."""
    parent = np.arange(n, dtype=np.int64)
    while len(a):
        ra, rb = parent[a], parent[b]
        m = ra != rb
        if not m.any():
            break
        a, b, ra, rb = a[m], b[m], ra[m], rb[m]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return parent


def joined_component_sizes(counts, pairs, maximum):
    """For every leaf, the number of leaves in the component the device would cluster it in: maximum method, union
    over all pairs; directional method, union over the pairs a climb or a flood can cross, max(ca, cb) >= 2 min(ca, cb).
    Computed from the inputs alone."""
    counts = np.asarray(counts, np.uint64)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    a, b = pairs[:, 0], pairs[:, 1]
    if not maximum:
        ca, cb = counts[a], counts[b]
        m = np.maximum(ca, cb) >= np.uint64(2) * np.minimum(ca, cb)     # (counts stay below 2^32: no wrap in 64 bits)
        a, b = a[m], b[m]
    root = _union_roots(len(counts), a, b)
    return np.bincount(root, minlength=len(counts))[root]


# ------------------------------------------------------------------------------------------
# the case table of tests/test_gpu_cluster_graphs.py
# ------------------------------------------------------------------------------------------
# component sizes at which the device changes form: closed forms for 1 and 2 leaves, one lane with LDS columns up
# to SMALL_COMP = 32, the big forms beyond; 64 = the lanes of the flood scan, 256 = the threads of the climb and
# member scans of k_cluster_big_coop, 1024 = four such rounds; and one component far beyond all of them
BOUNDARY_SIZES = (1, 2, 3, 4, 31, 32, 33, 34, 63, 64, 65, 255, 256, 257, 1023, 1025)
LARGE_SIZE = 5003
HUB_DEGREES = (31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 20000)


class Case:
    """one graph of the table: `make()` builds (counts, pairs); route_b says whether humid_stage_graph_edges takes it
    too (counts of at least 1 only)"""

    def __init__(self, group, name, make, route_b=True):
        self.group, self.name, self.make, self.route_b = group, name, make, route_b

    @property
    def id(self):
        return "%s/%s" % (self.group, self.name)


def _size_cases():
    out = []
    patterns = (("alternating", alternating(1, 2)), ("halving", halving_from_hub()),
                ("geometric", random_geometric(11)), ("boundary", boundary()))
    for k in BOUNDARY_SIZES + (LARGE_SIZE,):
        tops = [("path", path), ("star", star), ("tree", binary_tree), ("caterpillar", caterpillar),
                ("sparse", lambda n: random_sparse(n, 3.0, seed=n))]
        if k <= 257:                       # the one-lane kernels walk every edge
            tops += [("clique", clique), ("bipartite", complete_bipartite)]
        for tn, top in tops:
            for pn, pat in patterns:
                out.append(Case("size%d" % k, "%s-%s" % (tn, pn), lambda top=top, pat=pat, k=k: graph(top, pat, k)))
    return out


def _hub_counts(kind, n_hubs, m):
    """hub(s) first, then m leaves.  target: every leaf climbs to a hub (which hub: the first in ITS list); stolen:
    hubs of count 1 between leaves of 2 .. 5, taken by whoever floods first; equal: nothing moves (directional)"""
    if kind == "target":
        hubs = [9, 4][:n_hubs]
        leaves = np.where(np.arange(m) % 2 == 0, 1, 2)
    elif kind == "stolen":
        hubs = [1] * n_hubs
        leaves = 2 + np.arange(m) % 4
    else:
        hubs = [3] * n_hubs
        leaves = np.full(m, 3)
    return np.concatenate([np.asarray(hubs), leaves]).astype(np.uint64)


def _hub_cases():
    out = []
    for m in HUB_DEGREES:
        for tn, n_hubs in (("star", 1), ("k2m", 2)):
            for kind in ("target", "stolen", "equal"):
                def make(m=m, n_hubs=n_hubs, kind=kind, last=False):
                    k = n_hubs + m
                    pairs = star(k) if n_hubs == 1 else complete_bipartite(k, 2)
                    g = (_hub_counts(kind, n_hubs, m), pairs)
                    return reversed_labels(g) if last else g
                out.append(Case("hub%d" % m, "%s-%s-hubfirst" % (tn, kind), make))
                out.append(Case("hub%d" % m, "%s-%s-hublast" % (tn, kind), lambda make=make: make(last=True)))
    return out


def deep_path():
    """32 leaves, counts 1, 2, 4 .. 2^31: leaf 0 climbs 31 hops"""
    return graph(path, doubling(), 32)


def deep_path_pendants():
    """the same with 8 pendant leaves of count 1 on the top leaf: 40 leaves"""
    c, p = deep_path()
    return np.concatenate([c, np.ones(8, np.uint64)]), np.concatenate([p, _pairs(np.full(8, 31), 32 + np.arange(8))])


def deep_path_zero():
    """a leaf of count 0 in front of it: 32 hops, 33 leaves"""
    c, p = deep_path()
    return np.concatenate([[0], c]).astype(np.uint64), np.concatenate([_pairs([0], [1]), p + 1])


def _deep_cases():
    out = []
    for name, make, rb in (("path32", deep_path, True), ("path32+8", deep_path_pendants, True),
                           ("zero+path32", deep_path_zero, False)):
        out.append(Case("deep", name, make, rb))
        out.append(Case("deep", name + "-reversed", lambda make=make: reversed_labels(make()), rb))
    return out


TRIANGLES = ((0xFFFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF),     # 0xFFFFFFFF >= 2 * 0x7FFFFFFF: one cluster of more than 2^32 reads
             (0xFFFFFFFF, 0x80000000, 0xFFFFFFFE),     # 2 * 0x80000000 does not fit 32 bits: nothing merges (directional)
             (0x80000000, 0xFFFFFFFF, 2),
             (0xFFFFFFFE, 0x7FFFFFFF, 1),
             (1, 2, 0xFFFFFFFF))


def huge_pair():
    """must NOT merge under the directional method: 2 * 0x80000000 = 2^32 > 0xFFFFFFFF"""
    return np.asarray([0xFFFFFFFF, 0x80000000], np.uint64), path(2)


def huge_caterpillar_joined():
    """40 leaves, every link crossable although 2 * b passes 2^32 nowhere near: spine 0xFFFFFFFF / 0x7FFFFFFF in turn,
    pendants of 1 and 2 -- one directional component of 40 leaves with clusters of more than 2^32 reads"""
    c = np.concatenate([np.where(np.arange(20) % 2 == 0, 0xFFFFFFFF, 0x7FFFFFFF), 1 + np.arange(20) % 2])
    return c.astype(np.uint64), caterpillar(40)


def _huge_cases():
    out = [Case("huge", "pair", huge_pair), Case("huge", "caterpillar40-joined", huge_caterpillar_joined)]
    for i, t in enumerate(TRIANGLES):
        out.append(Case("huge", "triangle%d" % i, lambda t=t: (np.asarray(t, np.uint64), clique(3))))
    for seed in (1, 2, 3):
        out.append(Case("huge", "caterpillar40-random%d" % seed, lambda seed=seed: graph(caterpillar, huge(seed), 40)))
    return out


def _long_cases():
    return [Case("long", "path20000-alternating", lambda: graph(path, alternating(1, 2), 20000)),
            Case("long", "path20000-geometric", lambda: graph(path, random_geometric(5), 20000)),
            Case("long", "ladder2x5000-alternating", lambda: graph(ladder, alternating(1, 2), 10000)),
            Case("long", "ladder2x5000-geometric", lambda: graph(ladder, random_geometric(6), 10000))]


def many_big_components():
    """2100 components of 33 leaves and 50 of 300, every link crossable under both methods: more big components
    than the 2048 workgroups k_cluster_big_coop is launched with"""
    kinds33 = (graph(path, alternating(1, 2), 33), graph(star, halving_from_hub(), 33),
               graph(binary_tree, halving_from_hub(), 33), graph(caterpillar, alternating(2, 1), 33))
    kinds300 = (graph(path, alternating(1, 2), 300), graph(binary_tree, halving_from_hub(), 300))
    return disjoint_union([kinds33[i % 4] for i in range(2100)] + [kinds300[i % 2] for i in range(50)])


def many_small_components(blocks=86667):
    """paths of 1, 2, 3, 4 and 5 leaves with counts 1, 2, 1, .. in a repeating pattern of 15 leaves: 1 300 005 leaves,
    so a workgroup of k_comp_count (512 x 256 leaves a round) makes more than 8 rounds and flushes its root buffer
    inside the loop, and listed roots (components of 3 to 5) lie in every stretch of the index range"""
    starts = np.asarray([0, 1, 3, 6, 10])
    a = np.concatenate([s + np.arange(n - 1) for s, n in zip(starts, range(1, 6))])       # 10 links per block
    pos = np.concatenate([np.arange(n) for n in range(1, 6)])
    base = (np.arange(blocks, dtype=np.int64) * 15)[:, None]
    counts = np.tile(1 + pos % 2, blocks).astype(np.uint64)
    aa = (base + a[None, :]).ravel()
    return counts, _pairs(aa, aa + 1)


def every_family():
    """one graph of every family of the groups above (counts of at least 1 only), side by side"""
    gs = [graph(t, p, k) for k in (33, 65) for t, p in
          ((path, alternating(1, 2)), (star, halving_from_hub()), (binary_tree, boundary()),
           (caterpillar, random_geometric(3)), (lambda n: random_sparse(n, 3.0, seed=n), random_geometric(4)),
           (clique, boundary()), (complete_bipartite, alternating(1, 2)))]
    gs += [graph(path, alternating(1, 2), k) for k in (1, 2, 3, 4, 31, 32)]
    gs += [(_hub_counts("target", 1, 64), star(65)), reversed_labels((_hub_counts("stolen", 2, 33), complete_bipartite(35, 2))),
           (_hub_counts("equal", 1, 40), star(41))]
    gs += [deep_path(), reversed_labels(deep_path_pendants())]
    gs += [huge_pair(), huge_caterpillar_joined()] + [(np.asarray(t, np.uint64), clique(3)) for t in TRIANGLES]
    return disjoint_union(gs)


def _many_cases():
    return [Case("many_big", "identity", many_big_components),
            Case("many_big", "shuffled", lambda: shuffled_labels(many_big_components(), 21)),
            Case("many_small", "identity", many_small_components),
            Case("every_family", "identity", every_family),
            Case("every_family", "shuffled", lambda: shuffled_labels(every_family(), 22))]


CASES = _size_cases() + _hub_cases() + _deep_cases() + _huge_cases() + _long_cases() + _many_cases()
GROUPS = list(dict.fromkeys(c.group for c in CASES))


def cases_of(group):
    return [c for c in CASES if c.group == group]
