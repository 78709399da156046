"""-m gpu: a whole single-cell run fed in chunks -- the barcode counter and its finish (the whitelist from the data),
the posterior's prior, every chunk corrected against it and added to a keyed accumulator, finish, every chunk mapped --
against the one-shot path over all reads on another context: discover_whitelist, then run_keyed(correct=True,
barcode_quals=...).  Integer arithmetic: every comparison is exact."""
import numpy as np
import pytest

import humid_amd

import cells_truth as ct
from test_gpu_keyed import make_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
K, WORD_NT, N = 8, 10, 3000
EXPECTED, RATIO, MIN_ODDS = 30, 3, 5
FIELDS = ("total", "usable", "unique", "clusters", "edges", "nonsingle")


def reads(seed=801):
    """N reads of 30 cells with skewed sizes: exact barcodes, barcodes one substitution off (some between two cells a
    distance 2 apart), ambient barcodes, filtered reads; a few UMIs per cell with their own errors"""
    rng = np.random.default_rng(seed)
    cells = [int(v) for v in ct.random_barcodes(rng, 24, K)]
    cells += [c ^ (1 << 2) ^ (2 << 10) for c in cells[:6]]            # six twins at distance 2: their midpoints have two candidates
    cells = np.asarray(cells, U64)
    keys = cells[np.minimum(rng.geometric(0.08, size=N) - 1, len(cells) - 1)]
    u = rng.random(N)
    sub = rng.integers(1, 4, size=N).astype(U64) << (U64(2) * rng.integers(0, K, size=N).astype(U64))
    keys = np.where(u < 0.10, keys ^ sub, keys)
    mid = np.flatnonzero((u >= 0.10) & (u < 0.16))
    keys[mid] = cells[rng.integers(0, 6, size=len(mid))] ^ U64(1 << 2)      # between cell j and its twin
    amb = np.flatnonzero((u >= 0.16) & (u < 0.20))
    keys[amb] = rng.integers(0, 4 ** K, size=len(amb)).astype(U64)
    keys[rng.choice(N, size=25, replace=False)] = cells[0] ^ U64(3 << 6)     # an error abundant enough to be selected: the merge removes it
    quals = (rng.choice(np.asarray([2, 12, 25, 37]), size=(N, K)) + 33).astype(np.uint8)
    words, filt = make_words(seed + 1, N, WORD_NT, n_base=25)
    return words, keys, quals, filt


def equal(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.fixture(scope="module")
def one_shot():
    """the reference, computed once"""
    words, keys, quals, filt = reads()
    d = humid_amd.Dedup()
    try:
        cells = d.discover_whitelist(keys, filt, barcode_nt=K, expected=EXPECTED, merge_ratio=RATIO)
        cid, keep, s = d.run_keyed(words, keys, filt, word_nt=WORD_NT, correct=True, barcode_quals=quals, min_odds=MIN_ODDS)
        ref = dict(cells=cells, cid=cid, keep=keep, summary=s, keys=d.group_keys(), stats=d.group_stats(),
                   counts=d.barcode_status()[1], posterior=d.barcode_posterior(), whitelist=d.discovered_cells())
    finally:
        d.close()
    assert 10 < ref["cells"]["cells"] < ref["cells"]["distinct"] and ref["cells"]["merged"] > 0
    assert ref["posterior"]["multi"] > 20 and ref["posterior"]["rescued"] > 0 and s["usable"] < int((filt == 0).sum())
    return words, keys, quals, filt, ref


def chunked(d, words, keys, quals, filt, pieces):
    """the whole chunked run over pieces [(lo, hi)] in the order given, every chunk with its explicit base"""
    bc = d.barcode_counter(barcode_nt=K)
    for lo, hi in pieces:
        bc.add(keys[lo:hi], filt[lo:hi])
    cells = bc.finish(expected=EXPECTED, merge_ratio=RATIO)
    whitelist = d.discovered_cells()
    d.prior_begin()
    for lo, hi in pieces:
        d.prior_add(keys[lo:hi], filt[lo:hi])
    acc = d.keyed_accumulator(word_nt=WORD_NT, key_nt=K)
    corrected, counts, multi, rescued = {}, np.zeros(5, np.uint64), 0, 0
    for lo, hi in pieces:
        ko, st, c, extra = d.correct_keys(keys[lo:hi], filt[lo:hi], quals=quals[lo:hi], min_odds=MIN_ODDS, prior=True)
        corrected[lo] = (words[lo:hi], ko, (filt[lo:hi] | (st >= humid_amd.BC_AMBIGUOUS)).astype(np.uint8), lo)
        acc.add(*corrected[lo])
        counts += c
        multi += extra["multi"]
        rescued += extra["rescued"]
    s = acc.finish(1, 0)
    gkeys, stats = d.group_keys(), d.group_stats()                   # (before the first map ends the record they answer from)
    cid, keep = np.zeros(len(filt), np.uint32), np.zeros(len(filt), np.uint8)
    for lo, hi in pieces:
        cid[lo:hi], keep[lo:hi], unknown = acc.map(*corrected[lo])
        assert unknown == 0
    acc.clear()
    bc.clear()
    return dict(cells=cells, cid=cid, keep=keep, summary=s, keys=gkeys, stats=stats, counts=counts,
                posterior=dict(multi=multi, rescued=rescued), whitelist=whitelist)


@pytest.mark.parametrize("order", ["in_order", "shuffled"])
def test_the_chunked_run_equals_the_one_shot_run(one_shot, order):
    words, keys, quals, filt, ref = one_shot
    pieces = [(a, min(a + 700, N)) for a in range(0, N, 700)]
    if order == "shuffled":
        pieces = [pieces[i] for i in (3, 0, 4, 2, 1)]
    d = humid_amd.Dedup()
    try:
        got = chunked(d, words, keys, quals, filt, pieces)
    finally:
        d.close()
    assert got["cells"] == ref["cells"] and equal(got["whitelist"], ref["whitelist"])
    assert np.array_equal(got["cid"], ref["cid"]) and np.array_equal(got["keep"], ref["keep"])
    assert {x: got["summary"][x] for x in FIELDS} == {x: ref["summary"][x] for x in FIELDS}
    assert np.array_equal(got["keys"], ref["keys"]) and equal(got["stats"], ref["stats"])
    assert np.array_equal(got["counts"], ref["counts"]) and got["posterior"] == ref["posterior"]
