"""-m gpu: per-group statistics (include/humid_hip.h, humid_get_group_stats / humid_group_stats_device) after plain,
grouped and keyed runs.

Truth at small sizes: tests/grouped_truth.per_group (one oracle pass per group).  numpy derives every quantity of
the definition from it two independent ways -- from the leaves (bincount of the leaf groups weighted by count /
degree, searchsorted for the offsets, the adjacency for the pairs) and from the reads (bincount of the usable reads'
groups, the distinct cluster ids per group) -- and the two must agree with each other and with the device.
At 10 M reads the oracle is too slow: the truth is numpy over the accessors that existed before (leaves() and the
per-read outputs), which the existing suite pins to the oracle and which the new kernels do not touch."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from humid_amd.synth import synth_words

import grouped_truth as gt

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP = (1 << 64) - 1
KEYS = ("reads", "unique", "clusters", "edges", "leaf_off", "cluster_off")


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def pack(rows):
    n = rows.shape[1]
    if n <= 32:
        w = np.zeros(len(rows), U64)
        for t in range(n):
            w = (w << U64(2)) | rows[:, t].astype(U64)
        return w
    return np.stack([pack(rows[:, :n - 32]), pack(rows[:, n - 32:])], 1)


def make_words(seed, n_reads, word_nt, n_base=60, p_sub=0.04, p_filt=0.03):
    """a few base words with substitutions (exact repeats and near neighbours in every group), some filtered reads"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, size=(n_base, word_nt))
    rows = base[rng.integers(0, n_base, size=n_reads)] if n_reads else np.zeros((0, word_nt), np.int64)
    rows = np.where(rng.random(rows.shape) < p_sub, rng.integers(0, 4, size=rows.shape), rows)
    filt = (rng.random(n_reads) < p_filt).astype(np.uint8)
    return pack(rows), filt


def from_leaves(group, count, degree, cluster_id, G, off=None, idx=None):
    """the definition over the leaf arrays (walk order)"""
    g = np.asarray(group, np.int64)
    leaf_off = np.searchsorted(g, np.arange(G + 1), side="left").astype(np.uint32)
    reads = np.bincount(g, weights=np.asarray(count, np.float64), minlength=G).astype(U64)      # (exact below 2^53)
    deg = np.bincount(g, weights=np.asarray(degree, np.float64), minlength=G).astype(U64)
    assert not (deg & U64(1)).any()
    pairs = np.unique((g.astype(U64) << U64(32)) | np.asarray(cluster_id, U64))                  # distinct (group, id)
    clusters = np.bincount((pairs >> U64(32)).astype(np.int64), minlength=G)
    out = dict(reads=reads, unique=np.diff(leaf_off.astype(np.int64)).astype(np.uint32), clusters=clusters.astype(np.uint32),
               edges=(deg >> U64(1)).astype(np.uint32), leaf_off=leaf_off,
               cluster_off=np.concatenate([[0], np.cumsum(clusters)]).astype(np.uint32))
    if off is not None:                                                                          # pairs (i < j) by the group of i
        src = np.repeat(np.arange(len(g)), np.diff(np.asarray(off, np.int64)))
        fwd = src < np.asarray(idx, np.int64)
        assert np.array_equal(np.bincount(g[src[fwd]], minlength=G).astype(np.uint32), out["edges"])
    return out


def from_reads(groups, filt, cid, keep, G):
    """what the per-read arrays alone say: reads, clusters and the cluster-id ranges"""
    us = filt == 0
    g = np.asarray(groups)[us].astype(np.int64)
    reads = np.bincount(g, minlength=G).astype(U64)
    pairs = np.unique((g.astype(U64) << U64(32)) | np.asarray(cid)[us].astype(U64))
    pg = (pairs >> U64(32)).astype(np.int64)
    clusters = np.bincount(pg, minlength=G).astype(np.uint32)
    kept = np.bincount(g, weights=np.asarray(keep)[us].astype(np.float64), minlength=G).astype(np.uint32)
    assert np.array_equal(kept, clusters)                               # one kept read per molecule
    lo = np.full(G, np.iinfo(np.int64).max)
    hi = np.zeros(G, np.int64)
    ids = (pairs & U64(0xFFFFFFFF)).astype(np.int64)
    np.minimum.at(lo, pg, ids)
    np.maximum.at(hi, pg, ids)
    return dict(reads=reads, clusters=clusters, kept=kept, id_lo=lo, id_hi=hi)


def check_stats(st, s, lv_truth, rd_truth, G):
    """device == leaves' truth == reads' truth, and the invariants of the definition"""
    assert len(st["reads"]) == G and len(st["leaf_off"]) == G + 1 and len(st["cluster_off"]) == G + 1
    assert st["reads"].dtype == U64 and all(st[k].dtype == np.uint32 for k in KEYS[1:])
    for k in KEYS:
        assert np.array_equal(st[k], lv_truth[k]), k
    assert np.array_equal(st["reads"], rd_truth["reads"]) and np.array_equal(st["clusters"], rd_truth["clusters"])
    assert np.array_equal(st["clusters"], rd_truth["kept"])             # clusters[g] == keep[groups == g].sum()
    lo, co = st["leaf_off"].astype(np.int64), st["cluster_off"].astype(np.int64)
    assert (np.diff(lo) >= 0).all() and (np.diff(co) >= 0).all()
    assert lo[0] == 0 and co[0] == 0 and lo[-1] == s["unique"] and co[-1] == s["clusters"]
    assert int(st["reads"].sum()) == s["usable"] and int(st["unique"].astype(U64).sum()) == s["unique"]
    assert int(st["clusters"].astype(U64).sum()) == s["clusters"] and int(st["edges"].astype(U64).sum()) == s["edges"]
    some = st["clusters"] > 0                                           # the ids of g: cluster_off[g] + 1 .. cluster_off[g + 1]
    assert np.array_equal(rd_truth["id_lo"][some], co[:-1][some] + 1)
    assert np.array_equal(rd_truth["id_hi"][some], co[1:][some])


def check_against_oracle(d, st, s, cid, keep, words, groups, filt, word_nt, G, distance, method, edit):
    t = gt.per_group(words, groups, filt, word_nt, distance, method, edit=edit, first_read=False)
    assert np.array_equal(cid, t["cid"]) and np.array_equal(keep, t["keep"])
    for k in ("usable", "unique", "clusters", "edges"):
        assert int(s[k]) == int(t["summary"][k]), k
    lv = t["leaves"]
    check_stats(st, t["summary"], from_leaves(lv["group"], lv["count"], lv["degree"], lv["cluster_id"], G, t["off"], t["idx"]),
                from_reads(groups, filt, t["cid"], t["keep"], G), G)
    return t


def grouped_case(d, words, groups, filt, word_nt, n_groups, distance=1, method=0, edit=False):
    cid, keep, s = d.run_grouped(words, groups, filt, word_nt=word_nt, n_groups=n_groups, distance=distance,
                                 method=method, edit=edit)
    st = d.group_stats()
    assert "key" not in st
    g = np.zeros(len(filt), np.uint32) if groups is None else groups
    check_against_oracle(d, st, s, cid, keep, words, g, filt, word_nt, n_groups, distance, method, edit)
    return st


def keyed_case(d, words, keys, filt, word_nt, distance=1, method=0, edit=False):
    keys = np.asarray(keys, U64)
    K, inv = np.unique(keys[filt == 0], return_inverse=True)
    groups = np.full(len(filt), 0xFFFFFFFF, np.uint32)
    groups[filt == 0] = inv.astype(np.uint32)
    cid, keep, s = d.run_keyed(words, keys, filt, word_nt=word_nt, distance=distance, method=method, edit=edit)
    st = d.group_stats()
    assert st["key"].dtype == U64 and np.array_equal(st["key"], K)
    check_against_oracle(d, st, s, cid, keep, words, groups, filt, word_nt, len(K), distance, method, edit)
    return st


@pytest.mark.parametrize("distance,method,edit", [(1, 0, False), (1, 1, False), (2, 0, False), (2, 1, False),
                                                  (2, 0, True), (2, 1, True)])
def test_distances_methods_and_edit(dd, distance, method, edit):
    rng = np.random.default_rng(distance * 4 + method * 2 + edit)
    words, filt = make_words(50 + distance, 2500, 16, n_base=40, p_sub=0.06)
    groups = rng.integers(0, 11, size=len(filt)).astype(np.uint32)
    st = grouped_case(dd, words, groups, filt, 16, 11, distance, method, edit)
    assert st["edges"].sum() > 0
    keyed_case(dd, words, rng.integers(0, 1 << 64, size=9, dtype=U64)[groups % 9], filt, 16, distance, method, edit)


# (word_nt, n_groups): internal words of one uint64, of exactly 32 nt, and of two uint64 with the group field below
# and above bit 64 of the pair (caller words of one and of two uint64)
@pytest.mark.parametrize("word_nt,n_groups", [(12, 40), (24, 200), (28, 256), (30, 200), (32, 5), (40, 100), (60, 256)])
def test_word_lengths(dd, word_nt, n_groups):
    rng = np.random.default_rng(word_nt)
    words, filt = make_words(200 + word_nt, 3000, word_nt)
    groups = rng.integers(0, n_groups, size=len(filt)).astype(np.uint32)
    grouped_case(dd, words, groups, filt, word_nt, n_groups, 1, 0)
    keys = rng.integers(0, 1 << 64, size=n_groups, dtype=U64)[groups]
    keyed_case(dd, words, keys, filt, word_nt, 2, 1)


@pytest.mark.parametrize("word_nt", [24, 40])
def test_one_group_and_a_plain_run(dd, word_nt):
    words, filt = make_words(300 + word_nt, 4000, word_nt)
    st = grouped_case(dd, words, None, filt, word_nt, 1)
    cid, keep, s = dd.run(words, filt, word_nt=word_nt, distance=1)
    plain = dd.group_stats()
    assert "key" not in plain
    for k in KEYS:
        assert np.array_equal(plain[k], st[k]), k
    assert plain["reads"].tolist() == [s["usable"]] and plain["unique"].tolist() == [s["unique"]]
    assert plain["clusters"].tolist() == [s["clusters"]] == [int(keep.sum())] and plain["edges"].tolist() == [s["edges"]]
    assert plain["leaf_off"].tolist() == [0, s["unique"]] and plain["cluster_off"].tolist() == [0, s["clusters"]]
    # run_bases: the same words packed on the device
    n = word_nt
    w = words.reshape(len(filt), -1)
    sym = np.zeros((len(filt), n), np.int64)
    for t in range(n):
        col, sh = (0, 2 * (n - 32 - 1 - t)) if (n > 32 and t < n - 32) else (w.shape[1] - 1, 2 * (n - 1 - t))
        sym[:, t] = (w[:, col] >> U64(sh)) & U64(3)
    bases = np.frombuffer(b"ACGT", np.uint8)[sym]
    bases[filt == 1, 0] = ord("N")
    dd.run_bases(bases, word_nt=word_nt, distance=1)
    st_b = dd.group_stats()
    for k in KEYS:
        assert np.array_equal(st_b[k], st[k]), k


@pytest.mark.parametrize("word_nt,n_groups,present", [
    (16, 50, [20, 21, 49]),                      # absent at the front and in the middle
    (16, 50, [0, 7, 30]),                        # ... in the middle and at the end
    (12, 1 << 24, [5, 1 << 20, (1 << 24) - 2]),  # three groups of 2^24: one uint64
    (24, 1 << 24, [0, 1 << 23, (1 << 24) - 1]),  # ... two uint64 (24 + 12 nt)
])
def test_absent_groups(dd, word_nt, n_groups, present):
    rng = np.random.default_rng(n_groups % 1000 + word_nt)
    words, filt = make_words(400 + word_nt, 3000, word_nt)
    groups = np.asarray(present, np.uint32)[rng.integers(0, len(present), size=len(filt))]
    st = grouped_case(dd, words, groups, filt, word_nt, n_groups)
    assert sorted(np.flatnonzero(st["unique"]).tolist()) == sorted(present)


def test_keyed_random_keys_with_the_extremes(dd):
    rng = np.random.default_rng(7)
    words, filt = make_words(8, 5000, 24, p_filt=0.2)
    pool = np.concatenate([rng.integers(0, 1 << 64, size=300, dtype=U64), np.asarray([0, TOP], U64)])
    keys = pool[rng.integers(0, len(pool), size=len(filt))]
    keys[:4] = np.asarray([0, TOP, 0, TOP], U64)
    filt[:4] = 0
    keys[filt == 1] = rng.integers(1 << 40, 1 << 41, size=int(filt.sum())).astype(U64)   # keys no usable read has
    st = keyed_case(dd, words, keys, filt, 24)
    assert st["key"][0] == 0 and st["key"][-1] == TOP and len(st["key"]) == len(np.unique(keys[filt == 0]))
    assert not np.isin(keys[filt == 1], st["key"]).any()


def test_all_filtered_and_no_reads(dd):
    words, filt = make_words(10, 500, 24)
    none = np.ones(500, np.uint8)
    keys = np.arange(500, dtype=U64)
    dd.run_keyed(words, keys, none, word_nt=24)
    st = dd.group_stats()
    assert len(st["key"]) == 0 and all(len(st[k]) == 0 for k in KEYS[:4])
    assert st["leaf_off"].tolist() == [0] and st["cluster_off"].tolist() == [0]
    assert dd.group_stats_device()["n"] == 0
    dd.run_grouped(words, (keys % 7).astype(np.uint32), none, word_nt=24, n_groups=7)
    st = dd.group_stats()
    assert all(st[k].tolist() == [0] * 7 for k in KEYS[:4])
    assert st["leaf_off"].tolist() == [0] * 8 and st["cluster_off"].tolist() == [0] * 8
    e_w, e_f = np.zeros(0, U64), np.zeros(0, np.uint8)
    dd.run_keyed(e_w, np.zeros(0, U64), e_f, word_nt=24)
    st = dd.group_stats()
    assert len(st["reads"]) == 0 and st["leaf_off"].tolist() == [0] and len(st["key"]) == 0
    dd.run_grouped(e_w, np.zeros(0, np.uint32), e_f, word_nt=24, n_groups=3)
    st = dd.group_stats()
    assert st["reads"].tolist() == [0, 0, 0] and st["cluster_off"].tolist() == [0] * 4
    dd.run(e_w, e_f, word_nt=24)
    st = dd.group_stats()
    assert st["reads"].tolist() == [0] and st["leaf_off"].tolist() == [0, 0]


def test_state_and_caching(dd):
    fresh = humid_amd.Dedup()
    try:
        for call in (fresh.group_stats, fresh.group_stats_device):
            with pytest.raises(humid_amd.HumidError) as ei:
                call()
            assert ei.value.code == -6                                   # HUMID_E_STATE before any run
    finally:
        fresh.close()
    rng = np.random.default_rng(41)
    words, filt = make_words(42, 4000, 24)
    groups = rng.integers(0, 30, size=len(filt)).astype(np.uint32)
    a = grouped_case(dd, words, groups, filt, 24, 30)
    b = dd.group_stats()
    p1, p2 = dd.group_stats_device(), dd.group_stats_device()
    assert p1 == p2 and p1["n"] == 30
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    # another shape on the same context: the new run's statistics, not the cached ones
    w2, f2 = make_words(43, 1500, 40)
    c = keyed_case(dd, w2, rng.integers(0, 5, size=len(f2)).astype(U64) << U64(60), f2, 40)
    assert len(c["reads"]) == 5
    again = grouped_case(dd, words, groups, filt, 24, 30)
    for k in KEYS:
        assert np.array_equal(a[k], again[k]), k
    # a refused run leaves no statistics behind
    with pytest.raises(humid_amd.HumidError):
        dd.run_grouped(words, groups, filt, word_nt=24, n_groups=10)       # groups >= n_groups
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.group_stats()
    assert ei.value.code == -6


def test_cluster_graph_call_ends_the_statistics():
    g = humid_amd.ClusterGraph([3, 1, 1])
    try:
        g.link(0, 1)
        g.find_clusters()
        n = C.c_uint64()
        assert g._lib.humid_get_group_stats(g._h, 0, C.byref(n), None, None, None, None) == -6
    finally:
        g.close()


def test_host_buffers_are_never_overrun(dd):
    """guard words behind every output buffer; cap < G writes exactly cap groups and cap + 1 offsets"""
    rng = np.random.default_rng(51)
    words, filt = make_words(52, 3000, 24)
    groups = rng.integers(0, 64, size=len(filt)).astype(np.uint32)
    dd.run_grouped(words, groups, filt, word_nt=24, n_groups=64)
    full = dd.group_stats()
    lib, h = dd._lib, dd._h
    for cap in (0, 1, 17, 63, 64, 100):
        take = min(cap, 64)
        reads = np.full(take + 4, 0xA5A5A5A5A5A5A5A5, U64)
        loff = np.full(take + 1 + 4, 0xDEADBEEF, np.uint32)
        coff = np.full(take + 1 + 4, 0xDEADBEEF, np.uint32)
        edges = np.full(take + 4, 0xDEADBEEF, np.uint32)
        n = C.c_uint64()
        vp = lambda a: C.c_void_p(a.ctypes.data)                      # noqa: E731
        assert lib.humid_get_group_stats(h, cap, C.byref(n), vp(reads), vp(loff), vp(coff), vp(edges)) == 0
        assert n.value == 64
        assert np.array_equal(reads[:take], full["reads"][:take]) and (reads[take:] == U64(0xA5A5A5A5A5A5A5A5)).all()
        assert np.array_equal(edges[:take], full["edges"][:take]) and (edges[take:] == 0xDEADBEEF).all()
        assert np.array_equal(loff[:take + 1], full["leaf_off"][:take + 1]) and (loff[take + 1:] == 0xDEADBEEF).all()
        assert np.array_equal(coff[:take + 1], full["cluster_off"][:take + 1]) and (coff[take + 1:] == 0xDEADBEEF).all()
        # single arrays: every other pointer NULL
        only = np.full(take + 1 + 2, 0xDEADBEEF, np.uint32)
        assert lib.humid_get_group_stats(h, cap, None, None, None, vp(only), None) == 0
        assert np.array_equal(only[:take + 1], full["cluster_off"][:take + 1]) and (only[take + 1:] == 0xDEADBEEF).all()


class _DevArray:
    """zero-copy view of context-owned device memory for torch (CUDA array interface)"""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def device_view(ptr, n, typestr, dtype):
    import torch
    if n == 0:
        return np.zeros(0, dtype)
    return torch.as_tensor(_DevArray(ptr, n, typestr), device="cuda:0").cpu().numpy().view(dtype)


def shapes_10m(rng, n):
    yield "distinct_keys_2_5M", rng.integers(0, 1 << 64, size=2_500_000, dtype=U64)[rng.integers(0, 2_500_000, size=n)]
    yield "one_group", np.full(n, 0x0123456789ABCDEF, U64)
    small = rng.integers(0, 1 << 64, size=100_000, dtype=U64)
    yield "skewed", np.where(rng.random(n) < 0.5, U64(1 << 63), small[rng.integers(0, 100_000, size=n)])


def test_ten_million_reads_three_shapes(dd):
    """the bench's metric words under 2.5 M distinct keys, one key, and one key with half the reads + 10^5 small ones,
    against numpy over leaves() and the per-read outputs; the device pointers equal the host copies"""
    rng = np.random.default_rng(61)
    words, filt = synth_words(10_000_000, 1001, 24)
    for name, keys in shapes_10m(rng, len(filt)):
        cid, keep, s = dd.run_keyed(words, keys, filt, word_nt=24, distance=1)
        dev = dd.group_stats_device()
        st = dd.group_stats()
        K = np.unique(keys[filt == 0])
        G = len(K)
        assert np.array_equal(st["key"], K) and dev["n"] == G, name
        groups = np.searchsorted(K, keys).astype(np.uint32)
        lv = dd.leaves()
        check_stats(st, s, from_leaves(lv["group"], lv["count"], lv["degree"], lv["cluster_id"], G),
                    from_reads(groups, filt, cid, keep, G), G)
        assert np.array_equal(device_view(dev["reads"], G, "<i8", U64), st["reads"]), name
        assert np.array_equal(device_view(dev["edges"], G, "<i4", np.uint32), st["edges"]), name
        assert np.array_equal(device_view(dev["leaf_off"], G + 1, "<i4", np.uint32), st["leaf_off"]), name
        assert np.array_equal(device_view(dev["cluster_off"], G + 1, "<i4", np.uint32), st["cluster_off"]), name
        if name == "one_group":
            assert G == 1 and st["unique"].tolist() == [s["unique"]]
        if name == "skewed":
            assert int(st["reads"].max()) > s["usable"] // 3
    # the grouped entry point at this size: 2^24 groups, three present, one of them with nearly everything
    groups = np.where(rng.random(len(filt)) < 0.001, np.uint32(7), np.uint32((1 << 24) - 1))
    groups[:100] = 1 << 12
    cid, keep, s = dd.run_grouped(words, groups, filt, word_nt=24, n_groups=1 << 24)
    st = dd.group_stats()
    lv = dd.leaves()
    G = 1 << 24
    check_stats(st, s, from_leaves(lv["group"], lv["count"], lv["degree"], lv["cluster_id"], G),
                from_reads(groups, filt, cid, keep, G), G)
    assert np.flatnonzero(st["unique"]).tolist() == [7, 1 << 12, G - 1]
