"""-m gpu: the neighbour search that rides in the kernel which builds its bucket order (option fused_search;
k_group_fine with a search, kernels_part.hip.h / kernels_cgraph.hip.h) against the CPU
oracle AND against the same pass with a launch of k_pairs_append per combination (fused_search = 0), bit for bit.

Every input runs twice on the fused context: the append regions start small (max(U / 4, 4096) pairs), so a first run
may fill one and finish on the retry -- k_pairs_append over the stored orders -- and only the second run is fused
from end to end."""
import numpy as np
import pytest

import humid_amd
from humid_amd.synth import synth_words
from test_gpu_parity import check_against_oracle, dense_words

import grouped_truth as gt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fused():
    d = humid_amd.Dedup()
    d.set_option("fused_search", 1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def alone():
    d = humid_amd.Dedup()
    d.set_option("fused_search", 0)
    yield d
    d.close()


def snapshot(dd, words, filt, n, d, maximum):
    """one more pass and everything the accessors give of it"""
    cid, keep, s = dd.run(words, filt, word_nt=n, distance=d, method=int(maximum))
    off, idx = dd.adjacency()
    return dict(cid=cid, keep=keep, leaves=dd.leaves(), off=off, idx=idx, clusters=dd.clusters())


def assert_same_arrays(a, b):
    for k in ("cid", "keep", "off", "idx"):
        assert np.array_equal(a[k], b[k]), k
    for part in ("leaves", "clusters"):
        assert a[part].keys() == b[part].keys()
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k]), (part, k)


def fused_and_alone(fused, alone, words, filt, n, d, methods=(False,), options=()):
    """twice fused, once with a launch per combination: all three equal the oracle, and each other array for array.
    options: (key, value, value to restore) set on both contexts for these runs"""
    try:
        for key, value, _ in options:
            fused.set_option(key, value)
            alone.set_option(key, value)
        for maximum in methods:
            s1 = check_against_oracle(fused, words, filt, n, d, maximum)
            s2 = check_against_oracle(fused, words, filt, n, d, maximum)
            a = snapshot(fused, words, filt, n, d, maximum)
            s3 = check_against_oracle(alone, words, filt, n, d, maximum)
            b = snapshot(alone, words, filt, n, d, maximum)
            for k in ("unique", "clusters", "edges"):
                assert s1[k] == s2[k] == s3[k], k
            assert_same_arrays(a, b)
    finally:
        for key, _, restore in options:
            fused.set_option(key, restore)
            alone.set_option(key, restore)
    return s2


@pytest.fixture(scope="module")
def umi_words():
    return synth_words(40_000, 6, 24, p_sub=8e-3, p_n=1e-3)


def test_umi_words_over_two_scatter_tiles(fused, alone, umi_words):
    """U = 16 290 (two tiles of the level-1 scatter), 5 743 pairs: more than the 4 096 the regions start with, so the
    first run ends on the retry over the stored orders and the second is fused only"""
    words, filt = umi_words
    s = fused_and_alone(fused, alone, words, filt, 24, 1, methods=(False, True))
    assert s["unique"] > 8192 and s["edges"] > 4096


def test_six_combinations(fused, alone):
    """d = 2 over 12 nt: combinations 1-5 are searched inside their grouping, combination 0 by k_pairs_append"""
    words, filt = synth_words(60_000, 6, 12, p_sub=8e-3, p_n=1e-3)
    s = fused_and_alone(fused, alone, words, filt, 12, 2)
    assert s["unique"] > 8192


@pytest.fixture(scope="module")
def long_bucket_words():
    """3 prefixes x 5000 suffixes of 12 nt each: the prefix combination has three buckets of ~5000 words -- across
    position 8192 and beyond any walk, so the tiles take over and the search is taken again over the stored orders;
    the suffix combination has buckets of three"""
    rng = np.random.default_rng(21)
    prefix = rng.choice(1 << 24, size=3, replace=False).astype(np.uint64)
    suffix = rng.choice(1 << 24, size=5000, replace=False).astype(np.uint64)
    mol = ((prefix[:, None] << np.uint64(24)) | suffix[None, :]).reshape(-1)
    words = np.repeat(mol, 1 + rng.geometric(1.0 / 3.0, size=len(mol)))
    hit = np.flatnonzero(rng.random(len(words)) < 0.02)
    shift = (2 * rng.integers(0, 24, size=len(hit))).astype(np.uint64)
    words[hit] ^= rng.integers(1, 4, size=len(hit)).astype(np.uint64) << shift
    words = np.ascontiguousarray(words[rng.permutation(len(words))])
    return words, np.zeros(len(words), np.uint8)


@pytest.mark.parametrize("walk", [1024, 7, 1])
def test_buckets_across_tile_edges_and_beyond_the_walk(fused, alone, long_bucket_words, walk):
    words, filt = long_bucket_words
    s = fused_and_alone(fused, alone, words, filt, 24, 1, options=[("bucket_walk", walk, 1024)])
    assert s["unique"] > 15_000


@pytest.mark.parametrize("walk", [1, 7])
def test_small_walk_on_umi_words(fused, alone, umi_words, walk):
    """nearly every bucket of two words and more, in both combinations, goes on in the tiles"""
    words, filt = umi_words
    fused_and_alone(fused, alone, words, filt, 24, 1, options=[("bucket_walk", walk, 1024)])


def test_region_full_behind_the_tiles():
    """The fused search spreads its pairs over one append region per coarse bin, k_pairs_append over one per 1024
    positions.  A context whose regions were sized by 120 000 reads at d = 1 has room for the fused search of six
    combinations over 12 nt, the tiles run, and the search behind them -- k_pairs_append over the stored orders --
    fills a region: the retry must not take the tiles' list again, which the graph build relabelled in place."""
    for fused_search in (1, 0):
        d = humid_amd.Dedup()
        try:
            d.set_option("fused_search", fused_search)
            d.set_option("bucket_walk", 1)
            w, f = synth_words(120_000, 6, 24, p_sub=8e-3, p_n=1e-3)
            check_against_oracle(d, w, f, 24, 1, False, deep=False)
            check_against_oracle(d, w, f, 24, 1, True, deep=False)
            w, f = synth_words(60_000, 6, 12, p_sub=8e-3, p_n=1e-3)
            check_against_oracle(d, w, f, 12, 2, False)
            check_against_oracle(d, w, f, 12, 2, False, deep=False)
        finally:
            d.close()


def test_not_eligible_falls_back(fused, alone, umi_words):
    """one coarse bin takes everything (the padded grouping overflows: exact bins, nothing fused), fewer than 4096
    unique words, and orders from the library sort: parity only"""
    w = dense_words(np.random.default_rng(5), 60_000, 24, 7)
    f = np.zeros(len(w), np.uint8)
    for dd in (fused, fused, alone):
        s = check_against_oracle(dd, w, f, 24, 1, False)
    assert s["edges"] > 100_000
    words, filt = umi_words
    for dd in (fused, fused, alone):
        s = check_against_oracle(dd, words[:3000], filt[:3000], 24, 1, False)
    assert s["unique"] < 4096
    fused_and_alone(fused, alone, words, filt, 24, 1, options=[("group_buckets", 0, 1)])


@pytest.fixture(scope="module")
def sparse_bins_words():
    """U just above 4096: about 8 words per coarse bin of the suffix combination, bins of one word, empty bins"""
    words, filt = synth_words(5000, 6, 24, p_sub=0.05, p_n=1e-3)
    u = np.unique(words[filt == 0])
    assert 4096 < len(u) < 4300
    return words, filt, u


def test_last_two_words_of_the_order_are_neighbours(fused, alone, sparse_bins_words):
    words, filt, u = sparse_bins_words
    last = u[-1]
    extra = np.array([last ^ np.uint64(1)], np.uint64)            # the last nucleotide: same prefix, next to it in the order
    w = np.concatenate([words, extra, extra])
    f = np.concatenate([filt, np.zeros(2, np.uint8)])
    uu = np.unique(w[f == 0])
    assert {int(uu[-1]), int(uu[-2])} == {int(last), int(extra[0])}
    fused_and_alone(fused, alone, w, f, 24, 1)


def test_last_word_of_a_bin_is_a_neighbour_of_the_one_before(fused, alone, sparse_bins_words):
    """the suffix combination's coarse bins are the top 9 of its 24 key bits, and a bin's buckets come out by
    ascending key: a word that shares the largest suffix of its bin and differs in the prefix makes the bin's last
    two positions a pair"""
    words, filt, u = sparse_bins_words
    suf = u & np.uint64((1 << 24) - 1)
    coarse = suf >> np.uint64(15)
    extras = []
    for c in (int(coarse[0]), int(coarse[len(u) // 2]), 511 if (coarse == 511).any() else int(coarse.max())):
        in_bin = u[coarse == c]
        top = in_bin[np.argmax(in_bin & np.uint64((1 << 24) - 1))]
        extras.append(top ^ (np.uint64(2) << np.uint64(40)))       # one nucleotide of the prefix
    extras = np.array(extras, np.uint64)
    w = np.concatenate([words, extras])
    f = np.concatenate([filt, np.zeros(len(extras), np.uint8)])
    s = fused_and_alone(fused, alone, w, f, 24, 1)
    assert s["unique"] > 4096


def test_grouped_pass(fused, alone):
    """the same words in two groups: equal words of different groups stay strangers"""
    words, filt = synth_words(20_000, 6, 24, p_sub=8e-3, p_n=1e-3)
    w = np.concatenate([words, words])
    f = np.concatenate([filt, filt])
    g = np.repeat(np.arange(2, dtype=np.uint32), len(words))
    truth = gt.per_group(w, g, f, 24, distance=1, method=0, first_read=False)
    assert truth["summary"]["unique"] > 8192
    for dd in (fused, fused, alone):
        gt.assert_same(truth, gt.device_result(dd, w, g, f, 24, n_groups=2, distance=1, method=0))
