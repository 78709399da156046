"""CPU: the truth for accumulated runs (tests/accum_truth.py) against the independent brute-force checker
(tests/bruteforce.py) on a few hundred reads: contiguous and non-contiguous bases, both chunk orders."""
import numpy as np
import pytest

import bruteforce as bf
from accum_truth import accum_expected, accum_leaves
from humid_amd.synth import synth_wide_words, synth_words


def split(w, f, cuts, bases):
    edges = [0] + list(cuts) + [len(f)]
    return [(w[a:b], f[a:b], base) for a, b, base in zip(edges[:-1], edges[1:], bases)]


CUTS = (0, 90, 91, 240)               # an empty chunk, a chunk of one read
CONTIGUOUS = (0, 0, 90, 91, 240)
SCATTERED = (2 ** 40, 2 ** 33 + 7, 2 ** 33, 5, 1000)     # global order: the fourth chunk, the fifth, the third, the second


@pytest.mark.parametrize("n", [12, 40])
@pytest.mark.parametrize("bases", [CONTIGUOUS, SCATTERED])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d,method", [(1, 0), (2, 1), (0, 0)])
def test_truth_equals_bruteforce_on_the_sorted_reads(n, bases, reverse, d, method):
    if n > 32:
        w, f = synth_wide_words(300, 11 + n, n, p_sub=0.03, p_n=0.03)
    else:
        w, f = synth_words(300, 11 + n, n, p_sub=0.03, p_n=0.03)
    chunks = split(w, f, CUTS, bases)
    if reverse:
        chunks = chunks[::-1]
    got, summary, keep_orc = accum_expected(chunks, n, d, method)
    # brute force over all reads sorted by global index
    order = sorted(range(len(chunks)), key=lambda k: chunks[k][2])
    ws = np.concatenate([np.asarray(chunks[k][0]).reshape(-1, 2 if n > 32 else 1) for k in order])
    fs = np.concatenate([chunks[k][1] for k in order])
    cid, keep, detail = bf.dedup(ws if n > 32 else ws[:, 0], fs, d, bool(method))
    at = 0
    for k in order:
        m = len(chunks[k][1])
        assert np.array_equal(got[k][0], cid[at:at + m])
        assert np.array_equal(got[k][1], keep[at:at + m])
        assert np.array_equal(keep_orc[k], keep[at:at + m])      # the re-derived keep is the oracle's own
        at += m
    assert summary["total"] == 300 and summary["usable"] == int((fs == 0).sum())
    assert summary["unique"] == len(detail["unique"]) and summary["clusters"] == len(detail["info"])
    assert summary["edges"] == sum(len(x) for x in detail["nbrs"]) // 2
    # the list: words, counts, and the smallest GLOBAL index of each word
    lv = accum_leaves(chunks, n)
    assert np.array_equal(lv["word"], detail["unique"]) and np.array_equal(lv["count"], detail["count"].astype(np.uint64))
    g = np.concatenate([np.uint64(chunks[k][2]) + np.arange(len(chunks[k][1]), dtype=np.uint64) for k in order])
    key = (lambda x: tuple(int(v) for v in x)) if n > 32 else int
    first = {}
    for word, fl, gi in zip(ws.tolist() if n > 32 else ws[:, 0].tolist(), fs.tolist(), g.tolist()):
        if not fl:
            first.setdefault(key(word), gi)                      # (sorted by global index: the first seen is the minimum)
    assert lv["first"].dtype == np.uint64
    assert [first[key(x)] for x in lv["word"].tolist()] == lv["first"].tolist()


def test_leaves_of_nothing_and_of_filtered_reads_only():
    for n in (24, 48):
        lv = accum_leaves([], n)
        assert len(lv["count"]) == 0 and lv["word"].shape == ((0, 2) if n > 32 else (0,))
        w = np.zeros((5, 2) if n > 32 else 5, np.uint64)
        lv = accum_leaves([(w, np.ones(5, np.uint8), 3)], n)
        assert len(lv["count"]) == 0
        got, summary, _ = accum_expected([(w, np.ones(5, np.uint8), 3)], n)
        assert not got[0][0].any() and not got[0][1].any() and summary["unique"] == 0
