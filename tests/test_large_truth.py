"""tests/large_truth.py -- the exact reference of tests/test_gpu_large.py -- against the oracle
(oracle.pyoracle.Pipeline) and tests/bruteforce.py, on read sets the oracle finishes in seconds: 24-nt and 36-nt
words with filtered reads, d = 1 and d = 2, both methods."""
import functools

import numpy as np
import pytest

import bruteforce as bf
import large_truth as lt
from humid_amd.synth import synth_wide_words, synth_words
from oracle import pyoracle as orc

N = 200_000
PREFIXES = (1, 777, 65_537, 150_001, N)


@functools.lru_cache(maxsize=None)
def reads(nt, mode):
    """uniform UMI words of one and of two uint64; genome prefixes of a short genome (BASELINE config 5's shape,
    dense at d = 2)"""
    if nt > 32:
        return synth_wide_words(N, 2100 + nt, nt, p_sub=3e-3, p_n=1e-3)
    return synth_words(N, 2100 + nt, nt, p_sub=3e-3, p_n=1e-3, mode=mode, genome_bp=200_000)


@functools.lru_cache(maxsize=None)
def truth(nt, mode):
    return lt.PrefixTruth(*reads(nt, mode))


@functools.lru_cache(maxsize=None)
def oracle(nt, mode, d, maximum):
    p = orc.Pipeline(nt)
    p.read_data(*reads(nt, mode))
    p.find_hamming_neighbours(d)
    p.find_clusters(maximum)
    cid, keep = p.map_reads()
    return p, cid, keep


CASES = [(24, "umi"), (36, "umi"), (24, "genome")]


@pytest.mark.parametrize("nt,mode", CASES)
def test_prefixes_equal_a_fresh_unique(nt, mode):
    """prefixes cut from one sort: unique words, counts, first reads and every read's leaf equal np.unique of the
    prefix on its own (and tests/bruteforce.py's unique_counts); the whole set's words and counts equal the oracle's"""
    words, filt = reads(nt, mode)
    assert filt.any()
    pt = truth(nt, mode)
    for n in PREFIXES:
        t = pt.prefix(n)
        use = np.flatnonzero(filt[:n] == 0)
        uw, first, inv, cnt = np.unique(words[use], axis=0, return_index=True, return_inverse=True,
                                        return_counts=True)
        assert (t["n"], t["usable"], t["unique"]) == (n, len(use), len(uw))
        assert np.array_equal(t["word"], uw) and np.array_equal(t["count"], cnt)
        assert np.array_equal(t["first_read"], use[first])
        leaf = np.full(n, -1)
        leaf[use] = inv.reshape(-1)
        assert np.array_equal(t["leaf"], leaf)
        bw, bc = bf.unique_counts(words[:n], filt[:n])
        assert np.array_equal(bw, t["word"]) and np.array_equal(bc, t["count"])
    lv = oracle(nt, mode, 1, False)[0].leaves()
    assert np.array_equal(lv["word"], t["word"]) and np.array_equal(lv["count"], t["count"])


@pytest.mark.parametrize("nt,mode", CASES)
def test_pairs_d1_equal_the_oracle(nt, mode):
    """the complete d = 1 pair set, as CSR, equals the oracle's lists; the pairs of a prefix cut from those of the
    whole set equal the prefix's own"""
    pt = truth(nt, mode)
    t = pt.prefix(N)
    a, b = lt.pairs_d1(t["word"], nt)
    off, idx = lt.csr(a, b, t["unique"])
    p = oracle(nt, mode, 1, False)[0]
    ooff, oidx = p.adjacency()
    assert len(a) == p.n_edges > 1000
    assert np.array_equal(off, ooff) and np.array_equal(idx, oidx)
    for n in PREFIXES[:-1]:
        sa, sb = lt.sub_pairs(a, b, t["first_read"], n)
        ea, eb = lt.pairs_d1(pt.prefix(n)["word"], nt)
        assert np.array_equal(sa, ea) and np.array_equal(sb, eb)


def dense_words(rng, nt, n_words, n_base=4):
    """unique words a few substitutions away from n_base words: long runs of equal halves, many neighbours"""
    base = [sum(int(s) << (2 * i) for i, s in enumerate(rng.integers(0, 4, nt))) for _ in range(n_base)]
    out = set()
    while len(out) < n_words:
        w = base[int(rng.integers(n_base))]
        for p in rng.integers(0, nt, size=int(rng.integers(0, 5))):
            w ^= int(rng.integers(1, 4)) << (2 * int(p))
        out.add(w)
    vals = sorted(out)
    if nt <= 32:
        return np.asarray(vals, np.uint64)
    return np.asarray([(v >> 64, v & ((1 << 64) - 1)) for v in vals], np.uint64)


@pytest.mark.parametrize("nt", [7, 24, 36])
def test_pairs_in_long_runs_equal_the_all_pairs_matrix(nt):
    """words crowded around four centres (runs of hundreds of words with one half equal): the d = 1 pairs and the
    enumerated d = 2 rows of every leaf equal tests/bruteforce.py's all-pairs matrix"""
    uw = dense_words(np.random.default_rng(nt), nt, 1500)
    for d in (1, 2):
        rows = bf.adjacency(uw, d)
        lens = np.asarray([len(r) for r in rows])
        want = (np.repeat(np.arange(len(uw), dtype=np.uint64), lens) << np.uint64(32)) | \
            np.asarray([x for r in rows for x in r], np.uint64)
        if d == 1:
            off, idx = lt.csr(*lt.pairs_d1(uw, nt), len(uw))
            got = lt.rows_of(off, idx, np.arange(len(uw)))
        else:
            got = lt.sampled_rows_d2(uw, nt, np.arange(len(uw)))
        assert len(want) > 1000
        assert np.array_equal(got, want)


@pytest.mark.parametrize("nt,mode", CASES)
def test_sampled_d2_rows_equal_the_oracle(nt, mode):
    """every word within distance 2 of a sampled leaf, looked up: the rows equal the oracle's; the soundness and
    sample checks pass the oracle's lists and catch one pair taken out of both its rows"""
    t = truth(nt, mode).prefix(N)
    p = oracle(nt, mode, 2, False)[0]
    off, idx = p.adjacency()
    sample = lt.check_pairs_d2(t["word"], nt, off, idx, n_sample=3000, seed=1, chunk=500)
    assert np.array_equal(lt.rows_of(off, idx, sample), lt.sampled_rows_d2(t["word"], nt, sample))
    # leaves named besides the uniform sample are checked too (the GPU test adds leaves with a d = 1 neighbour)
    near = np.unique(np.concatenate(lt.pairs_d1(t["word"], nt)))[:700]
    both = lt.check_pairs_d2(t["word"], nt, off, idx, n_sample=3000, seed=1, chunk=500, also=near)
    assert np.array_equal(both, np.union1d(sample, near))
    # one pair of a sampled leaf out of both rows: the lists stay symmetric, ascending and close
    off = off.astype(np.int64)
    a = int(sample[np.flatnonzero(np.diff(off)[sample])[0]])
    b = int(idx[off[a]])
    drop = np.ones(len(idx), bool)
    drop[off[a]] = False
    drop[off[b] + np.flatnonzero(idx[off[b]:off[b + 1]] == a)[0]] = False
    off2 = off.copy()
    off2[a + 1:] -= 1
    off2[b + 1:] -= 1
    with pytest.raises(AssertionError, match="not complete"):
        lt.check_pairs_d2(t["word"], nt, off2, idx[drop], n_sample=3000, seed=1, chunk=500)
    # and one end replaced by a word far away: no longer symmetric
    bad = idx.copy()
    bad[off[a]] = len(t["word"]) - 1 if b != len(t["word"]) - 1 else 0
    with pytest.raises(AssertionError):
        lt.check_pairs_d2(t["word"], nt, off, bad, n_sample=10, seed=1)


@pytest.mark.parametrize("maximum", [False, True], ids=["directional", "maximum"])
@pytest.mark.parametrize("nt,mode,d", [(24, "umi", 1), (36, "umi", 1), (24, "genome", 2), (36, "umi", 2)])
def test_batch_graph_equals_the_pipeline(nt, mode, d, maximum):
    """counts and lists imported into the oracle's hand-built graph in one call each, clustered by
    orc_graph_find_clusters: leaf cluster ids, is_max_leaf, the clusters, the six summary counts, the histograms and
    the per-read results equal the Pipeline's.  d = 1 over the truth's own pairs, d = 2 over the oracle's lists (the
    GPU test's d = 2 case imports the device's)"""
    t = truth(nt, mode).prefix(N)
    p, cid, keep = oracle(nt, mode, d, maximum)
    off, idx = lt.csr(*lt.pairs_d1(t["word"], nt), t["unique"]) if d == 1 else p.adjacency()
    x = lt.unique_level(t, off, idx, maximum)
    lv, cl, s = p.leaves(), p.clusters(), p.summary()
    for k in ("total", "usable", "unique", "clusters", "edges"):
        assert x["summary"][k] == s[k], k
    assert x["summary"]["nonsingle"] == int(np.count_nonzero(lv["degree"]))
    for k in ("degree", "cluster_id", "is_max_leaf"):
        assert np.array_equal(x[k], lv[k]), k
    for k in ("size", "max_count", "max_leaf"):
        assert np.array_equal(x["clusters"][k].astype(np.uint64), cl[k].astype(np.uint64)), k
    assert x["hist"] == orc.histograms(p)
    ecid, ekeep = lt.per_read(t, x["cluster_id"], x["is_max_leaf"])
    assert np.array_equal(ecid, cid) and np.array_equal(ekeep, keep)


@pytest.mark.parametrize("maximum", [False, True], ids=["directional", "maximum"])
def test_per_read_equals_bruteforce(maximum):
    """8-nt words (dense: ties, chains, steals): the per-read results from the truth equal tests/bruteforce.py's
    literal recursion"""
    words, filt = synth_words(3000, 2200, 8, p_sub=0.02, p_n=0.02)
    t = lt.PrefixTruth(words, filt).prefix(len(words))
    x = lt.unique_level(t, *lt.csr(*lt.pairs_d1(t["word"], 8), t["unique"]), maximum)
    cid, keep, _ = bf.dedup(words, filt, 1, maximum)
    ecid, ekeep = lt.per_read(t, x["cluster_id"], x["is_max_leaf"])
    assert np.array_equal(ecid, cid) and np.array_equal(ekeep, keep)
