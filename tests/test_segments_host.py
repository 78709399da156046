"""CPU: the two truths of the segmented whitelist correction (tests/segments_truth.py) agree with each other, and
with the plain truth (tests/whitelist_truth.py) where the definition says they must: S = 1 is the plain correction with
that list, max_inexact = 1 is the plain correction against the product list."""
import numpy as np
import pytest

import segments_truth as sg
import whitelist_truth as wt

U64 = np.uint64

SHAPES = [
    ([3, 2, 4], [6, 4, 10]),
    ([1, 5, 2], [2, 12, 5]),
    ([4, 4], [12, 9]),
    ([2, 1, 1, 3, 2, 1, 2, 2], [2, 2, 4, 2, 2, 1, 16, 1]),          # S = 8; a full list (4^2) and a full 1-nt one
]


@pytest.mark.parametrize("seg_nt,sizes", SHAPES)
@pytest.mark.parametrize("max_inexact", [0, 1, None])
def test_the_two_truths_agree(seg_nt, sizes, max_inexact):
    rng = np.random.default_rng(sum(seg_nt) * 7 + len(sizes))
    lists = sg.make_lists(rng, sizes, seg_nt)
    keys, filt = sg.make_keys(rng, lists, seg_nt, 400 if len(seg_nt) == 8 else 1500, p1=0.15, p2=0.1, p3=0.05, pr=0.05)
    a = sg.correct(keys, filt, lists, seg_nt, max_inexact)
    b = sg.correct_all_pairs(keys, filt, lists, seg_nt, max_inexact)
    sg.assert_covers(sg.correct(keys, filt, lists, seg_nt), inexact=(0, 1, 2))
    sg.assert_same(a, b)
    assert int(a[2].sum()) == len(keys) and int(a[4].sum()) == int(a[3][0].sum())
    if max_inexact == 0:
        assert set(np.unique(a[1])) <= {0, 1, 4}                    # nothing is corrected, nothing ambiguous


def test_hand_cases():
    enc = lambda s: sum("ACGT".index(ch) << (2 * (len(s) - 1 - i)) for i, ch in enumerate(s))    # noqa: E731
    lists, nt = [[enc("AA"), enc("CC")], [enc("GGG")]], [2, 3]
    reads = ["AAGGG", "ACGGG", "AGGGG", "AAGGT", "AGGGT", "TTGGG", "AATTT", "ACGGT", "CCGGG"]
    keys = np.asarray([enc(r) for r in reads] + [enc("AAGGG") | (1 << 10)], U64)
    f = np.zeros(len(keys), np.uint8)
    f[-2] = 1
    out, status, counts, seg_counts, hist = sg.correct(keys, f, lists, nt)
    #                      exact  ambig.  corr.   corr.   2 x corr.  unm.   unm.   ambig.  filtered  >= 4^K
    assert list(status) == [1,    3,      2,      2,      2,         4,     4,     3,      0,        4]
    want = ["AAGGG", "ACGGG", "AAGGG", "AAGGG", "AAGGG", "TTGGG", "AATTT", "ACGGT"]
    assert [int(x) for x in out] == [enc(w) for w in want] + [0, int(keys[-1])]
    assert list(counts) == [1, 1, 3, 2, 3]
    assert seg_counts.tolist() == [[3, 2, 2, 1], [4, 3, 0, 1]] and list(hist) == [1, 5, 2]
    # one inexact segment at the most: the read with two corrected segments is unmatched, the rest stays
    status1 = sg.correct(keys, f, lists, nt, 1)[1]
    assert list(status1) == [1, 3, 2, 2, 4, 4, 4, 4, 0, 4]
    # a list entry with another one substitution away is exact, not corrected
    out, status, _, _, _ = sg.correct(np.asarray([enc("AC")], U64), np.zeros(1, np.uint8), [[enc("AA"), enc("AC")]], [2])
    assert list(status) == [1] and int(out[0]) == enc("AC")


@pytest.mark.parametrize("nt,n_wl", [(1, 2), (5, 40), (10, 300)])
def test_one_segment_is_the_plain_correction(nt, n_wl):
    rng = np.random.default_rng(nt)
    wl = wt.whitelist_with_neighbours(rng, n_wl, nt)
    keys, filt = wt.make_keys(rng, wl, nt, 5000, p1=0.1, p2=0.05, pr=0.05)
    high = np.flatnonzero(rng.random(len(keys)) < 0.02)
    keys[high] |= U64(1) << U64(2 * nt + 3)
    t = wt.correct(keys, filt, wl, nt)
    for mi in (1, None):
        s = sg.correct(keys, filt, [wl], [nt], mi)
        sg.assert_same(t, s[:3])
    if nt > 1:
        sg.assert_covers(s, inexact=(0, 1))                         # (one segment: m is 0 or 1)


@pytest.mark.parametrize("seg_nt,sizes", SHAPES[:3])
def test_one_inexact_segment_is_the_plain_correction_against_the_product(seg_nt, sizes):
    rng = np.random.default_rng(len(sizes) + 40)
    lists = sg.make_lists(rng, sizes, seg_nt)
    keys, filt = sg.make_keys(rng, lists, seg_nt, 4000, p1=0.15, p2=0.1, p3=0.05, pr=0.05)
    product = sg.product_list(lists, seg_nt)
    assert len(product) == np.prod([len(np.unique(w)) for w in lists])
    s = sg.correct(keys, filt, lists, seg_nt, 1)
    sg.assert_covers(s)
    for plain in (wt.correct, wt.correct_all_pairs):
        sg.assert_same(plain(keys, filt, product, sum(seg_nt)), s[:3])
