"""tests/graph_truth.py without a GPU: the two statements of the clustering definition agree on every builder, the
CSR builder is sound, and the case table of tests/test_gpu_cluster_graphs.py holds a component at every size where
the device changes form -- for each method, so that no change of a count pattern moves a case off its boundary
unnoticed."""
import numpy as np
import pytest

import graph_truth as gt

TOPOLOGIES = (("path", gt.path), ("ring", gt.ring), ("star", gt.star), ("clique", gt.clique),
              ("bipartite", gt.complete_bipartite), ("tree", gt.binary_tree), ("caterpillar", gt.caterpillar),
              ("ladder", gt.ladder), ("sparse", lambda k: gt.random_sparse(k, 3.0, seed=k)))
PATTERNS = (("equal", gt.equal(3)), ("alternating", gt.alternating(1, 2)), ("doubling", gt.doubling()),
            ("halving", gt.halving_from_hub()), ("boundary", gt.boundary()), ("huge", gt.huge(1)),
            ("zeros", gt.with_zeros(2)), ("geometric", gt.random_geometric(3)))
SIZES = (1, 2, 3, 4, 7, 33, 70)
NAMES = ("leaf_cluster", "size", "max_count", "max_leaf", "n_clusters")


def same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), (what, name)


@pytest.mark.parametrize("k", SIZES)
@pytest.mark.parametrize("maximum", [False, True], ids=["directional", "maximum"])
def test_oracle_equals_the_recursive_definition(k, maximum):
    for tn, top in TOPOLOGIES:
        for pn, pat in PATTERNS:
            counts, pairs = gt.graph(top, pat, k)
            assert len(counts) == k
            for order in gt.ORDERS:
                off, idx = gt.to_csr(counts, pairs, order)
                got = gt.oracle_clusters(counts, off, idx, maximum)
                want = gt.reference_clusters_py(counts, gt.csr_rows(off, idx), maximum)
                same(got, want, (tn, pn, k, order))
                assert int(got[1].sum()) == int(counts.sum())            # every read is in exactly one cluster
                assert got[0].min() >= 1 and got[0].max() == got[4]


def test_builders_are_duplicate_free_and_sized():
    for tn, top in TOPOLOGIES:
        for k in SIZES + (257,):
            pairs = top(k)
            assert pairs.shape == (len(pairs), 2) and (pairs[:, 0] != pairs[:, 1]).all(), (tn, k)
            assert pairs.size == 0 or (0 <= pairs.min() and pairs.max() < k), (tn, k)
            key = np.minimum(pairs[:, 0], pairs[:, 1]) * k + np.maximum(pairs[:, 0], pairs[:, 1])
            assert len(np.unique(key)) == len(key), (tn, k)
            if tn != "bipartite" or k > 1:                               # one connected component of k leaves
                assert (gt.joined_component_sizes(np.ones(k, np.uint64), pairs, True) == k).all(), (tn, k)
    assert len(gt.star(9)) == 8 and len(gt.clique(9)) == 36 and len(gt.complete_bipartite(9, 2)) == 14
    assert len(gt.caterpillar(9)) == 8 and len(gt.ladder(10)) == 13 and len(gt.ring(9)) == 9


def test_count_patterns():
    p = gt.path(40)
    assert gt.doubling()(40, p).tolist() == [1 << min(i, 31) for i in range(40)]
    assert gt.halving_from_hub()(5, gt.star(5)).tolist() == [2, 1, 1, 1, 1]
    assert gt.halving_from_hub()(7, gt.binary_tree(7)).tolist() == [4, 2, 2, 1, 1, 1, 1]
    assert set(gt.huge(1)(500, p).tolist()) == set(gt.HUGE_VALUES)
    for tn, top in TOPOLOGIES:                                           # never two linked zeros, and some zeros
        pairs = top(70)
        c = gt.with_zeros(2)(70, pairs)
        assert (c == 0).any() and not ((c[pairs[:, 0]] == 0) & (c[pairs[:, 1]] == 0)).any(), tn
    # boundary: along a path every link is at exactly 2b, 2b - 1 or 2b + 1, and all three occur
    c = gt.boundary()(200, gt.path(200)).astype(np.int64)
    big, small = np.maximum(c[1:], c[:-1]), np.minimum(c[1:], c[:-1])
    assert set((big - 2 * small).tolist()) == {-1, 0, 1}
    # equal counts: no link can be crossed, every leaf is its own directional component
    assert (gt.joined_component_sizes(gt.equal(3)(40, p), p, False) == 1).all()
    assert (gt.joined_component_sizes(gt.equal(3)(40, p), p, True) == 40).all()
    # 2b - 1 does not join, 2b and 2b + 1 do
    assert gt.joined_component_sizes([7, 4, 2, 5, 3], gt.path(5), False).tolist() == [1, 3, 3, 3, 1]


@pytest.mark.parametrize("order", gt.ORDERS, ids=str)
def test_to_csr_is_symmetric_and_duplicate_free(order):
    for tn, top in TOPOLOGIES:
        for k in (1, 2, 7, 70):
            pairs = top(k)
            off, idx = gt.to_csr(np.ones(k), pairs, order)
            assert off.dtype == np.uint64 and idx.dtype == np.uint32
            assert len(off) == k + 1 and off[0] == 0 and int(off[-1]) == len(idx) == 2 * len(pairs)
            rows = gt.csr_rows(off, idx)
            arcs = [(u, v) for u, r in enumerate(rows) for v in r]
            assert len(set(arcs)) == len(arcs), (tn, k)
            assert set(arcs) == {(v, u) for u, v in arcs}, (tn, k)
            assert set(arcs) == {(a, b) for a, b in pairs.tolist()} | {(b, a) for a, b in pairs.tolist()}, (tn, k)
            if order == "ascending":
                assert all(r == sorted(r) for r in rows)
            elif order == "descending":
                assert all(r == sorted(r, reverse=True) for r in rows)
            elif order == "link":
                linked = [[] for _ in range(k)]
                for a, b in pairs.tolist():
                    linked[a].append(b)
                    linked[b].append(a)
                assert rows == linked
    if isinstance(order, tuple):                                         # a shuffled order is none of the others
        pairs = gt.clique(20)
        assert not np.array_equal(gt.to_csr(np.ones(20), pairs, order)[1], gt.to_csr(np.ones(20), pairs, "ascending")[1])


def test_combinators():
    g = gt.graph(gt.caterpillar, gt.random_geometric(1), 9)
    h = gt.graph(gt.star, gt.alternating(1, 2), 4)
    counts, pairs = gt.disjoint_union([g, h, g])
    assert len(counts) == 22 and len(pairs) == 2 * len(g[1]) + len(h[1])
    assert sorted(set(gt.joined_component_sizes(counts, pairs, True).tolist())) == [4, 9]
    # relabelling moves names, not structure: the clusters are the same sets of leaves when the walk order is kept
    perm = np.random.default_rng(0).permutation(22)
    rc, rp = gt.relabel((counts, pairs), perm)
    assert np.array_equal(rc[perm], counts)
    assert np.array_equal(np.sort(gt.joined_component_sizes(rc, rp, False)), np.sort(gt.joined_component_sizes(counts, pairs, False)))
    ident = gt.relabel((counts, pairs), np.arange(22))
    assert np.array_equal(ident[0], counts) and np.array_equal(ident[1], pairs)
    back = gt.reversed_labels(gt.reversed_labels((counts, pairs)))
    assert np.array_equal(back[0], counts) and np.array_equal(back[1], pairs)


def test_linked_zero_counts_are_refused_before_the_oracle_runs():
    counts, pairs = np.asarray([3, 0, 0, 5], np.uint64), gt.path(4)
    off, idx = gt.to_csr(counts, pairs, "ascending")
    with pytest.raises(ValueError):
        gt.oracle_clusters(counts, off, idx, False)
    with pytest.raises(ValueError):
        gt.oracle_clusters(counts, off, idx, True)
    with pytest.raises(ValueError):
        gt.reference_clusters_py(counts, gt.csr_rows(off, idx), False)
    counts[2] = 1                                                        # a single zero between two others is fine
    lc, size, mc, ml, nc = gt.oracle_clusters(counts, off, idx, False)
    assert lc.tolist() == [1, 1, 2, 2] and size.tolist() == [3, 6] and ml.tolist() == [0, 3] and nc == 2
    # an isolated leaf of count 0 is a cluster without a maxLeaf (updateMaxCount_ compares with >)
    off, idx = gt.to_csr([0], gt.path(1), "link")
    assert gt.oracle_clusters([0], off, idx, False)[3].tolist() == [-1]
    assert gt.reference_clusters_py([0], [[]], True)[3].tolist() == [-1]


@pytest.fixture(scope="module")
def table_sizes():
    """per method: the component sizes that occur in the case table, and per group"""
    out = {False: {}, True: {}}
    for case in gt.CASES:
        counts, pairs = case.make()
        assert counts.dtype == np.uint64 and int(counts.max()) <= gt.U32_MAX, case.id
        assert case.route_b == bool(counts.min() >= 1), case.id
        for maximum in (False, True):
            sizes = set(np.unique(gt.joined_component_sizes(counts, pairs, maximum)).tolist())
            out[maximum].setdefault(case.group, set()).update(sizes)
    return out


@pytest.mark.parametrize("maximum", [False, True], ids=["directional", "maximum"])
def test_case_table_covers_every_form_boundary(table_sizes, maximum):
    seen = set().union(*table_sizes[maximum].values())
    missing = [k for k in gt.BOUNDARY_SIZES if k not in seen]
    assert not missing, "no component of exactly %s leaves under this method" % missing
    assert max(seen) >= 5000
    # and group by group what each is there for
    for k in gt.BOUNDARY_SIZES:
        assert k in table_sizes[maximum]["size%d" % k], k
    assert max(table_sizes[maximum]["size%d" % gt.LARGE_SIZE]) >= 5000
    for m in gt.HUB_DEGREES:                                             # the hub and all its leaves in one component
        assert m + 1 in table_sizes[maximum]["hub%d" % m] and m + 2 in table_sizes[maximum]["hub%d" % m], m
    assert {32, 40} <= table_sizes[maximum]["deep"] and 33 in table_sizes[maximum]["deep"]
    assert 40 in table_sizes[maximum]["huge"]
    assert max(table_sizes[maximum]["long"]) >= 5000
    assert {33, 300} <= table_sizes[maximum]["many_big"]
    assert table_sizes[maximum]["many_small"] == {1, 2, 3, 4, 5}


def test_case_table_shapes():
    ids = [c.id for c in gt.CASES]
    assert len(set(ids)) == len(ids)
    counts, pairs = gt.many_big_components()
    sizes = gt.joined_component_sizes(counts, pairs, False)
    big = sizes > 32
    assert len(counts) == 2100 * 33 + 50 * 300 and big.all()
    assert int((1.0 / sizes).sum().round()) == 2150 > 2048              # components, all of them big ones
    counts, pairs = gt.many_small_components()
    assert len(counts) > 9 * 512 * 256                                   # a ninth round after the flush of the eighth
    # clusters of more than 2^32 reads, and the pair that must not merge
    for maximum in (False, True):
        c, p = gt.huge_caterpillar_joined()
        off, idx = gt.to_csr(c, p, "ascending")
        assert int(gt.oracle_clusters(c, off, idx, maximum)[1].max()) > 1 << 32
    c, p = gt.huge_pair()
    off, idx = gt.to_csr(c, p, "ascending")
    assert gt.oracle_clusters(c, off, idx, False)[4] == 2 and gt.oracle_clusters(c, off, idx, True)[4] == 1
    c, p = gt.deep_path_zero()
    off, idx = gt.to_csr(c, p, "ascending")
    lc, size, mc, ml, nc = gt.oracle_clusters(c, off, idx, False)
    assert nc == 1 and ml.tolist() == [32] and int(mc[0]) == 1 << 31      # leaf 0 climbs 32 hops to the top
