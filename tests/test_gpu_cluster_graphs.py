"""-m gpu: the clustering kernels on hand-built graphs (tests/graph_truth.py), bit for bit against the CPU oracle.

Every graph of the case table goes through both entry points that take an explicit graph:
  route A  humid_cluster_graph (raw C ABI, host CSR): neighbour lists in four orders -- ascending, descending, link()
           order and shuffled -- so every tie-break that follows list order is pinned; leaf_cluster, size, max_count,
           max_leaf and n_clusters against the oracle on the same CSR;
  route B  humid_stage_graph_edges (device pair list, rows sorted on the device): pairs ascending and shuffled; cluster
           ids, maxLeaf flags and the summary against the oracle on the ascending CSR.  The words are not read when the
           pairs are given (stage_graph searches nothing then); distinct ascending words are passed all the same.
with both methods, and on one context with coop_big = 1 (k_cluster_big_coop) and one with coop_big = 0 (one lane per
component).  Which component sizes the table holds is checked without a GPU by tests/test_graph_truth_host.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_truth as gt
from humid_amd.api import HumidError, _vp
from humid_amd.sharded import HipStageOps

pytestmark = pytest.mark.gpu

E_INVALID = -1
NAMES = ("leaf_cluster", "size", "max_count", "max_leaf", "n_clusters")


@pytest.fixture(scope="module")
def ctxs():
    """{coop_big: context}"""
    out = {}
    for coop in (1, 0):
        out[coop] = HipStageOps(0)
        out[coop].set_option("coop_big", coop)
    yield out
    for o in out.values():
        o.close()


def cluster_graph(ctx, counts, off, idx, method):
    """humid_cluster_graph with CSR arrays as they are (ClusterGraph.link builds Python lists: too slow for 10^5
    leaves).  Returns (rc, (leaf_cluster, size, max_count i.e. u64, max_leaf as i64, n_clusters))."""
    u = len(counts)
    cnt = np.ascontiguousarray(counts).astype(np.uint32)
    assert np.array_equal(cnt.astype(np.uint64), np.asarray(counts, np.uint64))
    o32 = np.ascontiguousarray(off).astype(np.uint32)
    x32 = np.ascontiguousarray(idx, dtype=np.uint32) if len(idx) else np.zeros(1, np.uint32)
    lc, size = np.zeros(u, np.uint32), np.zeros(u, np.uint64)
    mc, ml = np.zeros(u, np.uint32), np.zeros(u, np.uint32)
    nc = C.c_uint32()
    rc = ctx._lib.humid_cluster_graph(ctx._h, _vp(cnt), _vp(o32), _vp(x32), u, method, _vp(lc), _vp(size), _vp(mc),
                                      _vp(ml), C.byref(nc))
    c = nc.value
    return rc, (lc, size[:c], mc[:c].astype(np.uint64), ml[:c].astype(np.int64), c)


def edge_list(pairs, shuffle_seed=None):
    """(smaller << 32 | larger) per pair, ascending or shuffled, on the device"""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    e = np.sort((p.min(axis=1) << 32) | p.max(axis=1))
    if shuffle_seed is not None:
        e = e[np.random.default_rng(shuffle_seed).permutation(len(e))]
    return torch.from_numpy(e).cuda()


def stage_graph_edges(ctx, counts, edges, method):
    """humid_stage_graph_edges over words 0 .. U-1 (32 nt) with the given counts; (cluster ids u32, is_max u8, summary)"""
    u = len(counts)
    g_word = torch.arange(u, dtype=torch.int64, device="cuda")
    g_cnt = torch.from_numpy(np.asarray(counts, np.uint64).astype(np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    cid, ismax, s = ctx.graph_edges(g_word, g_cnt, edges, 32, 1, method)
    return cid.cpu().numpy().view(np.uint32), ismax.cpu().numpy(), s


def check_route_a(ctx, counts, off, idx, method, want, what):
    rc, got = cluster_graph(ctx, counts, off, idx, method)
    assert rc == 0, (what, rc, ctx._lib.humid_last_error(ctx._h))
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g, w), (what, name)


def check_route_b(ctx, counts, pairs, edges, method, want, what):
    lc, _, _, ml, nc = want
    cid, ismax, s = stage_graph_edges(ctx, counts, edges, method)
    assert np.array_equal(cid, lc), (what, "cid")
    assert np.array_equal(ismax, (ml[lc.astype(np.int64) - 1] == np.arange(len(lc))).astype(np.uint8)), (what, "is_max")
    linked = len(np.unique(np.asarray(pairs).ravel()))
    assert (s["unique"], s["edges"], s["nonsingle"], s["clusters"]) == (len(counts), len(pairs), linked, nc), what


def check_graph(ctxs, g, method, what, route_b=True):
    counts, pairs = g
    want_ascending = None
    for order in gt.ORDERS:
        off, idx = gt.to_csr(counts, pairs, order)
        want = gt.oracle_clusters(counts, off, idx, method == 1)
        if order == "ascending":
            want_ascending = want
        for coop, ctx in ctxs.items():
            check_route_a(ctx, counts, off, idx, method, want, (what, "A", order, "coop_big=%d" % coop))
    if route_b:
        for seed in (None, 5):
            edges = edge_list(pairs, seed)
            for coop, ctx in ctxs.items():
                check_route_b(ctx, counts, pairs, edges, method, want_ascending,
                              (what, "B", "pairs shuffled" if seed else "pairs ascending", "coop_big=%d" % coop))


@pytest.mark.parametrize("method", [0, 1], ids=["directional", "maximum"])
@pytest.mark.parametrize("group", gt.GROUPS)
def test_case_table(ctxs, group, method):
    for case in gt.cases_of(group):
        check_graph(ctxs, case.make(), method, case.id, case.route_b)


def test_what_the_32_bit_cases_are_for(ctxs):
    """a cluster of more than 2^32 reads comes back whole, and (0xFFFFFFFF, 0x80000000) stays two clusters under the
    directional method: 2 * 0x80000000 must not wrap to 0"""
    c, p = gt.huge_caterpillar_joined()
    off, idx = gt.to_csr(c, p, "ascending")
    for ctx in ctxs.values():
        for method in (0, 1):
            rc, (lc, size, mc, ml, nc) = cluster_graph(ctx, c, off, idx, method)
            assert rc == 0 and int(size.max()) > 1 << 32 and int(size.sum()) == int(c.sum())
    c, p = gt.huge_pair()
    off, idx = gt.to_csr(c, p, "ascending")
    for ctx in ctxs.values():
        rc, (lc, size, mc, ml, nc) = cluster_graph(ctx, c, off, idx, 0)
        assert rc == 0 and nc == 2 and lc.tolist() == [1, 2] and size.tolist() == [0xFFFFFFFF, 0x80000000]
        cid, ismax, s = stage_graph_edges(ctx, c, edge_list(p), 0)
        assert cid.tolist() == [1, 2] and ismax.tolist() == [1, 1] and s["clusters"] == 2


# ------------------------------------------------------------------------------------------
# refusals leave the context usable
# ------------------------------------------------------------------------------------------
def usable(ctxs, method=0):
    check_graph(ctxs, gt.graph(gt.caterpillar, gt.boundary(), 33), method, "after a refusal")


def refused(ctx, counts, off, idx, method=0):
    rc, (lc, size, mc, ml, nc) = cluster_graph(ctx, np.asarray(counts, np.uint64), np.asarray(off), np.asarray(idx), method)
    assert rc == E_INVALID and nc == 0, rc


def test_route_a_refuses_an_asymmetric_list(ctxs):
    for ctx in ctxs.values():
        refused(ctx, [1, 2, 3], [0, 1, 1, 1], [1])                         # 1 in 0's list, 0 not in 1's
        refused(ctx, [1, 2, 3], [0, 2, 3, 4], [1, 1, 0, 0], method=1)     # (0, 1) twice on one side
    usable(ctxs)


def test_route_a_refuses_two_linked_leaves_of_count_zero(ctxs):
    counts, pairs = np.asarray([0, 0, 4], np.uint64), gt.path(3)
    off, idx = gt.to_csr(counts, pairs, "link")
    with pytest.raises(ValueError):
        gt.oracle_clusters(counts, off, idx, False)
    for ctx in ctxs.values():
        for method in (0, 1):
            refused(ctx, counts, off, idx, method)
    usable(ctxs)


def test_route_a_refuses_an_index_out_of_range(ctxs):
    for ctx in ctxs.values():
        refused(ctx, [1, 2, 3], [0, 1, 2, 2], [3, 0])
        refused(ctx, [1, 2, 3], [0, 1, 2, 2], [0xFFFFFFFF, 0])
    usable(ctxs, 1)


def test_route_b_refuses_a_pair_naming_leaf_u(ctxs):
    counts = np.asarray([1, 2, 4, 1], np.uint64)
    for bad in ([[0, 1], [1, 4]], [[0, 1], [2, 0xFFFFFFFF]]):
        for ctx in ctxs.values():
            with pytest.raises(HumidError) as e:
                stage_graph_edges(ctx, counts, edge_list(bad), 0)
            assert e.value.code == E_INVALID
    usable(ctxs)


# ------------------------------------------------------------------------------------------
# repeatability: claims and frontier order of the cooperative kernel come from atomics, the result may not
# ------------------------------------------------------------------------------------------
def all_outputs(ctx, g, method):
    counts, pairs = g
    off, idx = gt.to_csr(counts, pairs, gt.shuffled(3))
    rc, a = cluster_graph(ctx, counts, off, idx, method)
    assert rc == 0
    cid, ismax, s = stage_graph_edges(ctx, counts, edge_list(pairs, 9), method)
    return list(a[:4]) + [np.asarray([a[4], s["unique"], s["edges"], s["nonsingle"], s["clusters"]]), cid, ismax]


@pytest.mark.parametrize("method", [0, 1], ids=["directional", "maximum"])
@pytest.mark.parametrize("which", ["every_family/shuffled", "hub257/k2m-target-hublast"])
def test_same_answer_twice_and_on_a_fresh_context(ctxs, which, method):
    g = next(c for c in gt.CASES if c.id == which).make()
    for coop, ctx in ctxs.items():
        first = all_outputs(ctx, g, method)
        again = all_outputs(ctx, g, method)
        fresh_ctx = HipStageOps(0)
        try:
            fresh_ctx.set_option("coop_big", coop)
            fresh = all_outputs(fresh_ctx, g, method)
        finally:
            fresh_ctx.close()
        for a, b, c in zip(first, again, fresh):
            assert np.array_equal(a, b) and np.array_equal(a, c), (which, coop)
