"""-m gpu: strand-symmetric (duplex) deduplication through the C ABI (humid_dedup_run_paired, humid_paired_canonical,
humid_get_strands) against tests/paired_truth.py, bit for bit: cluster ids, keep flags, the summary counts, leaves,
adjacency, clusters, the three histograms, the strand of every read, the reads of each strand per cluster and the
strand summary."""
import collections
import functools
import itertools

import numpy as np
import pytest

import edit_truth as et
import humid_amd
import paired_truth as pt
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_STATE = -1, -2, -6


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def assert_matches(dd, got, t, strands=True):
    cid, keep, s = got
    for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle"):
        assert s[k] == t["summary"][k], (k, s[k], t["summary"][k])
    assert np.array_equal(cid, t["cluster_id"]) and np.array_equal(keep, t["keep"])
    lv = dd.leaves()
    for k in ("word", "count", "first_read", "degree", "cluster_id", "is_max_leaf"):
        assert np.array_equal(lv[k], t["leaves"][k]), k
    off, idx = dd.adjacency()
    assert np.array_equal(off.astype(np.uint64), t["off"]) and np.array_equal(idx, t["idx"])
    cl = dd.clusters()
    for k in ("size", "max_count", "max_leaf"):
        assert np.array_equal(cl[k].astype(np.int64), np.asarray(t["clusters"][k]).astype(np.int64)), k
    assert dd.histograms() == t["hist"]
    gs = dd.group_stats()
    assert len(gs["reads"]) == 1 and int(gs["reads"][0]) == t["summary"]["usable"]
    assert int(gs["unique"][0]) == t["summary"]["unique"] and int(gs["clusters"][0]) == t["summary"]["clusters"]
    assert int(gs["edges"][0]) == t["summary"]["edges"]
    if strands:
        strand, top, bottom, sm = dd.strands()
        assert np.array_equal(strand, t["strand"])
        assert np.array_equal(top, t["top"]) and np.array_equal(bottom, t["bottom"])
        assert sm == t["strands"]


@functools.lru_cache(maxsize=None)
def case(n, d, n_reads=700):
    words, filt = pt.families(1000 * n + d, n, n_reads, d)
    return words, filt, {m: pt.run(words, filt, n, d, m) for m in (0, 1)}


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("d", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [2, 8, 24, 32, 34, 48, 64])
def test_families_of_both_strands(dd, n, d, method):
    words, filt, t = case(n, d)
    assert t[method]["strands"]["bottom_reads"] > 0 and (n == 2 or t[method]["strands"]["duplex"] > 0)
    assert_matches(dd, dd.run_paired(words, filt, word_nt=n, distance=d, method=method), t[method])


@pytest.mark.parametrize("n_reads", [0, 1, 2, 63, 64, 65, 5000])
@pytest.mark.parametrize("n", [24, 48])
def test_read_counts(dd, n, n_reads):
    words, filt, t = case(n, 1, n_reads)
    for method in (0, 1):
        assert_matches(dd, dd.run_paired(words, filt, word_nt=n, distance=1, method=method), t[method])


@pytest.mark.parametrize("n", [2, 8, 24, 34, 64])
def test_orientation_flip(dd, n):
    """one error in front of the first position where the halves differ: one cluster (two for any implementation that
    only canonicalises)"""
    a, b = pt.flip_pair(n)
    words, filt = pt.from_ints([a, b, a], n), np.zeros(3, np.uint8)
    t = pt.run(words, filt, n, 1)
    assert t["summary"]["clusters"] == 1
    got = dd.run_paired(words, filt, word_nt=n, distance=1)
    assert got[2]["clusters"] == 1 and got[2]["unique"] == 2 and got[2]["edges"] == 1
    assert_matches(dd, got, t)
    cw, _ = dd.canonical_words(words, filt, word_nt=n)
    assert dd.run(cw, filt, word_nt=n, distance=1)[2]["clusters"] == 2


@pytest.mark.parametrize("n,d", [(8, 1), (24, 1), (24, 2), (48, 3)])
def test_forced_cases_alone(dd, n, d):
    """palindromes, a leaf within d of its own mirror (no self edge), a pair under both terms (one edge)"""
    vals = pt.forced_reads(np.random.default_rng(n + d), n, d)
    words, filt = pt.from_ints(vals, n), np.zeros(len(vals), np.uint8)
    for method in (0, 1):
        assert_matches(dd, dd.run_paired(words, filt, word_nt=n, distance=d, method=method), pt.run(words, filt, n, d, method))


@pytest.mark.parametrize("n", [24, 48])
def test_all_filtered_and_one_leaf(dd, n):
    words = case(n, 1, 64)[0]
    filt = np.ones(len(words), np.uint8)
    assert_matches(dd, dd.run_paired(words, filt, word_nt=n, distance=1), pt.run(words, filt, n, 1))
    v = [x for x in pt.to_ints(words, n) if x != pt.mirror(x, n)][0]
    one = pt.from_ints([v, pt.mirror(v, n), v, v, pt.mirror(v, n)], n)             # U == 1, both strands
    f1 = np.array([0, 0, 1, 0, 0], np.uint8)
    t = pt.run(one, f1, n, 1)
    assert t["summary"]["unique"] == 1 and t["strands"]["duplex"] == 1
    assert_matches(dd, dd.run_paired(one, f1, word_nt=n, distance=1), t)


def longest_key_run(t, n, d, s):
    """(the longest run of equal join keys among the leaves' keys and among their mirrors' keys, the widest key in
    bits): a key is a combination of s - d of the s segments of the plan"""
    leaves = pt.to_ints(t["leaves"]["word"], n)
    longest, bits = 0, 0
    for combo in itertools.combinations(et.segments(n, s), s - d):
        bits = max(bits, 2 * sum(ln for _, ln in combo))
        for vals in (leaves, [pt.mirror(v, n) for v in leaves]):
            keys = collections.Counter(tuple((v >> 2 * (n - at - ln)) & ((1 << 2 * ln) - 1) for at, ln in combo) for v in vals)
            longest = max(longest, max(keys.values()))
    assert bits <= 64                                   # (no key of these cases is cut)
    return longest, bits


# (n, d, plan_segments, segments of the plan, bits of a key): words of one or two u64 x keys of 32 or 64 bits.  Without
# plan_segments the plan of a few hundred leaves is two halves at d = 1: the fewest segments whose key tells them apart.
LONG_RUNS = [(24, 1, 0, 2, 24), (48, 2, 3, 3, 32), (64, 1, 0, 2, 64), (32, 1, 3, 3, 44)]


@pytest.mark.parametrize("n,d,forced,s,key_bits", LONG_RUNS, ids=["n%d_d%d" % c[:2] for c in LONG_RUNS])
def test_key_runs_longer_than_the_walk(dd, n, d, forced, s, key_bits):
    """a few hundred leaves share one half (n = 32: the 22 nucleotides of the first two of three segments): with
    bucket_walk 8 the joins take their long runs in pieces; where a half is shared the plain and the mirror join both
    meet a run (X.R against X.R, and against the mirrors X.R' of the leaves R'.X)"""
    words, filt = pt.shared_prefix_words(7, n, 22) if n == 32 else pt.long_run_words(7, n)
    t = pt.run(words, filt, n, d)
    assert t["summary"]["unique"] > (299 if n == 32 else 400) and t["summary"]["edges"] > 50
    if n == 32:
        assert t["strands"]["bottom_reads"] > 0
    run, bits = longest_key_run(t, n, d, s)
    assert run > 8 and bits == key_bits, (run, bits)
    dd.set_option("bucket_walk", 8)
    dd.set_option("plan_segments", forced)
    try:
        got = dd.run_paired(words, filt, word_nt=n, distance=d)
        pieces = [dd.run_roads()]
        assert_matches(dd, got, t)
        assert dd.run_roads() == pieces[0]
        if n == 24:
            t2 = pt.run(words, filt, 24, 2, 1)
            got = dd.run_paired(words, filt, word_nt=24, distance=2, method=1)
            pieces.append(dd.run_roads())
            assert_matches(dd, got, t2)
    finally:
        dd.set_option("bucket_walk", 1024)
        dd.set_option("plan_segments", 0)
    got = dd.run_paired(words, filt, word_nt=n, distance=d)
    whole_runs = dd.run_roads()
    assert_matches(dd, got, t)
    print("roads", pieces, whole_runs)
    for r in pieces:                                     # (the pairs are given to the graph stage: one attempt)
        assert r["n_events"] >= 1 and set(r["events"]) == {"JOIN_PIECES"} and r["graph_attempts"] == 1, r
    assert run <= 1024 and whole_runs == dict(events=[], n_events=0, graph_attempts=1), (run, whole_runs)


@pytest.mark.parametrize("n", [8, 24, 48, 64])
def test_distance_zero_is_the_plain_run_on_the_canonical_words(dd, n):
    words, filt, t = case(n, 0)
    cw, _ = pt.canonical(words, filt, n)
    for method in (0, 1):
        a = dd.run_paired(words, filt, word_nt=n, distance=0, method=method)
        la, adj_a, cl_a, h_a = dd.leaves(), dd.adjacency(), dd.clusters(), dd.histograms()
        b = dd.run(cw, filt, word_nt=n, distance=0, method=method)
        lb, adj_b, cl_b, h_b = dd.leaves(), dd.adjacency(), dd.clusters(), dd.histograms()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle"):
            assert a[2][k] == b[2][k]
        assert all(np.array_equal(la[k], lb[k]) for k in la) and all(np.array_equal(cl_a[k], cl_b[k]) for k in cl_a)
        assert np.array_equal(adj_a[0], adj_b[0]) and np.array_equal(adj_a[1], adj_b[1]) and h_a == h_b


@pytest.mark.parametrize("n,d", [(8, 1), (24, 1), (24, 2), (34, 3), (64, 1)])
def test_words_canonical_words_and_mirrored_words_agree(dd, n, d):
    words, filt, t = case(n, d)
    for method in (0, 1):
        a = dd.run_paired(words, filt, word_nt=n, distance=d, method=method)
        cw, strand = pt.canonical(words, filt, n)
        b = dd.run_paired(cw, filt, word_nt=n, distance=d, method=method)
        sb = dd.strands()
        c = dd.run_paired(pt.mirror_words(words, n), filt, word_nt=n, distance=d, method=method)
        for x in (b, c):
            assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])
        assert sb[3]["bottom_reads"] == 0 and np.all(sb[0][filt == 0] == humid_amd.STRAND_TOP)


@pytest.mark.parametrize("n", [2, 8, 24, 32, 34, 48, 64])
def test_canonical_words(dd, n):
    import torch
    words, filt, _ = case(n, 1)
    cw, strand = pt.canonical(words, filt, n)
    w0 = words.copy()
    got_w, got_s = dd.canonical_words(words, filt, word_nt=n)
    assert np.array_equal(words, w0)
    assert np.array_equal(got_w, cw) and np.array_equal(got_s, strand)       # (a filtered read keeps its word)
    assert set(np.unique(got_s)) <= {humid_amd.STRAND_TOP, humid_amd.STRAND_BOTTOM, humid_amd.STRAND_NONE}
    # device pointers, words_out aliased to words; the arrays behind the last read stay as they are
    dev = torch.device("cuda:0")
    N = len(filt)
    flat = np.concatenate([words.reshape(-1), np.full(4, 0x5A5A5A5A5A5A5A5A, np.uint64)])
    d_w = torch.from_numpy(flat.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_s = torch.full((N + 16,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    dd.canonical_words_device(d_w.data_ptr(), d_f.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), N, word_nt=n)
    out_w, out_s = d_w.cpu().numpy().view(np.uint64), d_s.cpu().numpy()
    assert np.array_equal(out_w[:cw.size].reshape(cw.shape), cw) and np.all(out_w[cw.size:] == 0x5A5A5A5A5A5A5A5A)
    assert np.array_equal(out_s[:N], strand) and np.all(out_s[N:] == 0xA5)


def test_canonical_words_leave_the_last_run_alone(dd):
    words, filt, t = case(24, 1)
    got = dd.run_paired(words, filt, word_nt=24, distance=1)
    other, ofilt, _ = case(48, 1)
    dd.canonical_words(other, ofilt, word_nt=48)
    dd._wide = False
    assert_matches(dd, got, t[0])


@pytest.mark.parametrize("n", [24, 48])
def test_run_on_device_pointers(dd, n):
    import torch
    words, filt, t = case(n, 1)
    dev = torch.device("cuda:0")
    N = len(filt)
    d_w = torch.from_numpy(words.reshape(-1).view(np.int64).copy()).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_cid = torch.full((N + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_keep = torch.full((N + 16,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s = dd.run_paired_device(d_w.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), N, word_nt=n, distance=1)
    cid, keep = d_cid.cpu().numpy().view(np.uint32), d_keep.cpu().numpy()
    assert np.all(cid[N:] == 0x5A5A5A5A) and np.all(keep[N:] == 0xA5)
    assert np.array_equal(d_w.cpu().numpy().view(np.uint64), words.reshape(-1))             # the input is not written
    assert_matches(dd, (cid[:N], keep[:N], s), t[0])


@pytest.mark.parametrize("n", [24, 48])
def test_select_best_with_the_canonical_words(dd, n):
    words, filt, t = case(n, 1)
    cid, keep, s = dd.run_paired(words, filt, word_nt=n, distance=1)
    cw, _ = pt.canonical(words, filt, n)
    out, rep, changed = dd.select_best(cw, cid, keep, np.full(len(filt), 7, np.uint32), word_nt=n, scope="leaf")
    assert changed == 0 and np.array_equal(out, keep)
    # the best-scoring read of a cluster may be a bottom-strand read: it is found through its canonical word
    strand = t[0]["strand"]
    scores = np.where(strand == pt.BOTTOM, 9, 7).astype(np.uint32)
    out, rep, changed = dd.select_best(cw, cid, keep, scores, word_nt=n, scope="leaf")
    cvals = pt.to_ints(cw, n)
    want = np.zeros(len(filt), np.uint8)
    for k in np.flatnonzero(keep):
        cand = [i for i in np.flatnonzero(cid == cid[k]) if cvals[i] == cvals[k]]
        want[max(cand, key=lambda i: (scores[i], -i))] = 1
    assert np.array_equal(out, want) and changed == int((want != keep).sum()) // 2 and changed > 0


def test_error_codes_leave_the_context_usable(dd):
    words, filt, t = case(24, 1)

    def refused(code, **kw):
        with pytest.raises(humid_amd.HumidError) as ei:
            dd.run_paired(kw.pop("words", words), filt, **kw)
        assert ei.value.code == code, (kw, ei.value)
        with pytest.raises(humid_amd.HumidError) as ei:           # a failed call leaves no run behind
            dd.strands()
        assert ei.value.code == E_STATE

    refused(E_INVALID, word_nt=23, distance=1)
    refused(E_UNSUPPORTED, word_nt=66, distance=1, words=np.zeros((len(filt), 2), np.uint64))
    refused(E_UNSUPPORTED, word_nt=65, distance=1, words=np.zeros((len(filt), 2), np.uint64))
    refused(E_INVALID, word_nt=24, distance=1, method=2)
    dd.set_option("edit_distance", 1)
    try:
        refused(E_UNSUPPORTED, word_nt=24, distance=2)
        assert_matches(dd, dd.run_paired(words, filt, word_nt=24, distance=1), t[0])      # distance <= 1 is Hamming
    finally:
        dd.set_option("edit_distance", 0)
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.canonical_words(words, filt, word_nt=23)
    assert ei.value.code == E_INVALID
    # the context is usable: a plain run on it matches the oracle
    cid, keep, s = dd.run(words, filt, word_nt=24, distance=1)
    ocid, okeep, osum, _ = orc.dedup_run(words, filt, 24, 1, 0)
    assert np.array_equal(cid, ocid) and np.array_equal(keep, okeep) and s["clusters"] == osum["clusters"]


def test_a_plain_run_afterwards_answers_for_itself(dd):
    words, filt, t = case(24, 1)
    assert_matches(dd, dd.run_paired(words, filt, word_nt=24, distance=1), t[0])
    cid, keep, s = dd.run(words, filt, word_nt=24, distance=1)
    p = orc.Pipeline(24)
    p.read_data(words, filt)
    p.find_hamming_neighbours(1)
    p.find_clusters(False)
    ocid, okeep = p.map_reads()
    assert np.array_equal(cid, ocid) and np.array_equal(keep, okeep)
    assert s["unique"] > t[0]["summary"]["unique"]                    # (the mirrored copies are leaves of their own again)
    lv, olv = dd.leaves(), p.leaves()
    assert np.array_equal(lv["word"], olv["word"]) and np.array_equal(lv["count"], olv["count"].astype(np.uint32))
    off, idx = dd.adjacency()
    ooff, oidx = p.adjacency()
    assert np.array_equal(off.astype(np.uint64), ooff) and np.array_equal(idx, oidx)
    assert np.array_equal(dd.clusters()["size"], p.clusters()["size"])
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.strands()
    assert ei.value.code == E_STATE
