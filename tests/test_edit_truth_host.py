"""Host-only checks of the truth and the generator behind tests/test_gpu_edit_sweep.py: the all-pairs Levenshtein
adjacency of the CPU oracle (oracle/humid_oracle.c, orc_allpairs_*) against the Python brute force and the oracle's
trie search, and the pairs of tests/edit_truth.py against that truth."""
import collections
import itertools

import numpy as np
import pytest

import bruteforce as bf
import edit_truth as et
from oracle import pyoracle as orc
from test_gpu_edit import many_indel_words, wide_indel_words
from test_oracle_vs_bruteforce import indel_words


def csr_of_lists(nbrs):
    off = np.zeros(len(nbrs) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in nbrs])
    return off, np.asarray([j for x in nbrs for j in x], np.uint32)


def trie_adjacency(uw, n, d):
    p = orc.Pipeline(n)
    p.read_data(uw, np.zeros(len(uw), np.uint8))
    p.find_edit_neighbours(d)
    assert p.unique == len(uw)
    return p.adjacency()


@pytest.mark.parametrize("n,d", [(1, 1), (2, 2), (5, 2), (6, 3), (9, 4), (16, 3), (24, 6), (31, 2), (32, 5)])
def test_allpairs_is_the_brute_force_and_the_trie_search(n, d):
    rng = np.random.default_rng(10 * n + d)
    words = many_indel_words(rng, 160 if n <= 16 else 70, n, 3) if n >= 6 else rng.integers(0, 4 ** n, size=160).astype(np.uint64)
    uw = et.unique_words(words)
    off, idx = orc.edit_adjacency_allpairs(uw, n, d)
    boff, bidx = csr_of_lists(bf.edit_adjacency(uw, n, d))
    assert np.array_equal(off, boff) and np.array_equal(idx, bidx)
    toff, tidx = trie_adjacency(uw, n, d)
    assert np.array_equal(off, toff) and np.array_equal(idx, tidx)
    assert len(idx) > 0


@pytest.mark.parametrize("n,d", [(33, 2), (34, 3), (48, 4), (63, 6), (64, 2)])
def test_allpairs_two_word_words(n, d):
    rng = np.random.default_rng(n + d)
    uw = et.unique_words(wide_indel_words(rng, 60 if n <= 48 else 45, n))
    off, idx = orc.edit_adjacency_allpairs(uw, n, d)
    boff, bidx = csr_of_lists(bf.edit_adjacency(uw, n, d))
    assert np.array_equal(off, boff) and np.array_equal(idx, bidx)
    toff, tidx = trie_adjacency(uw, n, d)
    assert np.array_equal(off, toff) and np.array_equal(idx, tidx)
    assert len(idx) > 0


def test_allpairs_on_larger_one_word_input_equals_the_trie_search():
    rng = np.random.default_rng(5)
    uw = et.unique_words(indel_words(rng, 1500, 20, p_indel=0.5))
    for d in (2, 4):
        off, idx = orc.edit_adjacency_allpairs(uw, 20, d)
        toff, tidx = trie_adjacency(uw, 20, d)
        assert np.array_equal(off, toff) and np.array_equal(idx, tidx)


def test_lev_pairs_is_the_python_programme():
    rng = np.random.default_rng(8)
    for n in (1, 2, 7, 31, 32, 33, 64):
        rows = rng.integers(0, 4, size=(60, n))
        other = np.where(rng.random(rows.shape) < 0.15, rng.integers(0, 4, size=rows.shape), rows)
        other[::3] = np.roll(other[::3], 1, axis=1)                    # shifted text
        got = orc.lev_pairs(et.pack(rows), et.pack(other), n)
        want = [bf.levenshtein(a, b) for a, b in zip(rows.tolist(), other.tolist())]
        assert got.tolist() == want
    assert orc.lev_pairs(et.pack(rows), et.pack(rows), 64).tolist() == [0] * 60


@pytest.mark.parametrize("n", [4, 8, 9, 24, 31, 32, 33, 47, 64])
def test_segment_cut(n):
    """the documented layout, from first principles: s contiguous parts that cover the word, lengths n // s or one
    more, the longer ones first"""
    for s in range(1, min(n, 14) + 1):
        segs = et.segments(n, s)
        assert len(segs) == s and segs[0][0] == 0
        for (a, la), (b, lb) in zip(segs, segs[1:]):
            assert a + la == b and la >= lb
        assert segs[-1][0] + segs[-1][1] == n
        lens = [ln for _, ln in segs]
        assert set(lens) <= {n // s, n // s + 1} and min(lens) >= 1
        assert sum(1 for ln in lens if ln == n // s + 1) == n % s
    assert et.segments(24, 5) == [(0, 5), (5, 5), (10, 5), (15, 5), (20, 4)]
    assert et.segments(33, 4) == [(0, 9), (9, 8), (17, 8), (25, 8)]


def test_kind_assignments():
    for d, want in ((2, 3), (3, 7), (4, 19), (5, 51), (6, 141), (7, 393)):
        ks = et.kind_assignments(d)
        assert len(ks) == want == len(set(ks))
        assert {k.count("D") for k in ks} == set(range(d // 2 + 1))
    assert ("D", "I") in et.kind_assignments(2) and ("I", "D") in et.kind_assignments(2)
    assert ("D", "D", "I", "I") in et.kind_assignments(4) and ("I", "D", "D", "I") in et.kind_assignments(4)


GRID = [(8, 2, 3), (8, 2, 6), (8, 7, 8), (12, 3, 4), (12, 4, 6), (16, 2, 5), (16, 3, 6), (16, 5, 6), (24, 2, 4),
        (24, 4, 5), (24, 6, 7), (31, 3, 5), (32, 2, 6), (32, 4, 6), (33, 2, 3), (33, 4, 5), (34, 3, 4), (48, 5, 6),
        (63, 2, 6), (64, 3, 6), (64, 6, 7)]


@pytest.mark.parametrize("n,d,s", GRID)
def test_generated_pairs_cover_every_assignment(n, d, s):
    """every (alphabet, damaged segments, kinds) has a pair at true distance 1 .. d; no pair is further than d; the
    share of pairs outside 1 .. d (equal words: an insertion undoing a deletion inside a repeat) stays below one half"""
    x, y, meta = et.all_pairs(n * 100 + d * 10 + s, n, d, s)
    assert len(x) == len(meta) <= et.n_placed(n, d, s)
    dist = orc.lev_pairs(et.pack(x), et.pack(y), n)
    assert int(dist.max()) <= d
    good = collections.defaultdict(int)
    for t, m in zip(dist.tolist(), meta):
        good[m[:3]] += 1 <= t <= d
    assert all(v >= 1 for v in good.values()), [k for k, v in good.items() if v == 0][:5]
    assert len(good) == 2 * (len(list(itertools.combinations(range(s), d))) * len(et.kind_assignments(d)) + 1)
    outside = float(np.mean((dist < 1) | (dist > d)))
    print("n=%d d=%d s=%d: %d pairs, share outside 1..d = %.4f, at exactly d = %.3f"
          % (n, d, s, len(x), outside, float(np.mean(dist == d))))
    assert outside < 0.5
    # the edit really sits in each damaged segment: x and y agree outside the span of the damaged segments
    segs = et.segments(n, s)
    for xr, yr, m in list(zip(x.tolist(), y.tolist(), meta))[::7]:
        if m[3] == "edge":
            continue
        lo, hi = segs[m[1][0]][0], segs[m[1][-1]][0] + segs[m[1][-1]][1]
        assert xr[:lo] == yr[:lo] and xr[hi + 1:] == yr[hi + 1:]


def test_offset_vectors_of_two_indel_pairs_occur():
    """d = 4, s = 6: the two untouched segments are seen at offsets (+1, -1) and (2, 1) by some pair"""
    rng = np.random.default_rng(1)
    x, y, meta = et.placed_pairs(rng, 24, 4, 6)
    segs = et.segments(24, 6)
    seen = set()
    for xr, yr, (damaged, kinds, mode) in zip(x.tolist(), y.tolist(), meta):
        if mode != "interior":
            continue
        offs = []
        for t in range(6):
            if t in damaged:
                continue
            shift = sum((k == "I") - (k == "D") for q, k in zip(damaged, kinds) if q < t)
            a, ln = segs[t]
            assert xr[a:a + ln] == yr[a + shift:a + shift + ln]
            offs.append(shift)
        seen.add(tuple(offs))
    assert {(1, -1), (-1, 1), (2, 1), (-2, -1), (1, 2), (0, 0), (1, 1), (0, 1)} <= seen, seen
