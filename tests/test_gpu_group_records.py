"""-m gpu: the grouping on 8-byte records (option group_records; k_p8_scatter1 over FieldsRecs, k_group_fine_recs;
kernels_graph.hip.h / kernels_part.hip.h) against the CPU oracle AND against the same pass on 12-byte pairs with every
order stored (group_records = 0): cluster ids, keep flags, summary, every accessor; the roads of a run and its attempts
equal on both contexts.  Dedup.group_records_info says which groupings moved records (and stored no order) and how
many orders were stored, so a shape that must take the record road, or must not, is asserted and not assumed.

A combination is grouped at 4 096 unique words and more, by a key of at most 24 bits whose top 9 (of 18 and more) are the
coarse bin; a level-1 tile is 8 192 words; the padded room of a coarse bin is U / bins + U / bins / 4 + 1 024; a fresh
context has max(U / 4, 4 096) slots for pairs in 64 regions; a record holds 2 n - 9 + bits_for(U) bits."""
import numpy as np
import pytest

import humid_amd
from humid_amd.synth import synth_words
from test_gpu_parity import check_against_oracle

import grouped_truth as gt

pytestmark = pytest.mark.gpu

U64 = np.uint64
NO_RETRY = dict(events=[], n_events=0, graph_attempts=1)


def context(group_records):
    d = humid_amd.Dedup()
    d.set_option("group_records", group_records)
    return d


@pytest.fixture(scope="module")
def recs():
    d = context(1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def pairs():
    d = context(0)
    yield d
    d.close()


@pytest.fixture
def fresh_both():
    """two contexts nothing has run on: full padding, no room remembered"""
    a, b = context(1), context(0)
    yield a, b
    a.close()
    b.close()


def n_unique(words, filt):
    return len(np.unique(words[filt == 0]))


def bits_for(n):
    """bits needed for values < n (the library's bits_for): the walk index of a record"""
    return int(n - 1).bit_length()


def both(recs, pairs, words, filt, n, d, methods=(False,), options=(), deep=True):
    """the run on both contexts against the oracle; the roads and attempts equal.  Returns (summary, roads, info) of the
    last run on the records context and the info of the pairs context.  options: (key, value, restore) on both"""
    try:
        for key, value, _ in options:
            recs.set_option(key, value)
            pairs.set_option(key, value)
        for maximum in methods:
            ra, rb = [], []
            s = check_against_oracle(recs, words, filt, n, d, maximum, deep=deep, roads=ra)
            info = recs.group_records_info()
            s0 = check_against_oracle(pairs, words, filt, n, d, maximum, deep=deep, roads=rb)
            info0 = pairs.group_records_info()
            print("group_records", info, info0)
            assert ra[0] == rb[0], (ra[0], rb[0])
            for k in ("total", "usable", "unique", "clusters", "edges"):
                assert s[k] == s0[k], k
            assert info0["searched_on_records"] == 0, info0
    finally:
        for key, _, restore in options:
            recs.set_option(key, restore)
            pairs.set_option(key, restore)
    return s, ra[0], info, info0


def steady(recs, pairs, words, filt, n, d, **kw):
    """twice: a first run may regrow the regions, the second is the steady state and retries nothing"""
    both(recs, pairs, words, filt, n, d, **kw)
    s, roads, info, info0 = both(recs, pairs, words, filt, n, d, **kw)
    assert roads == NO_RETRY, roads
    return s, info, info0


# ---- 24 nt, d = 1 ----

def test_one_scatter_tile(recs, pairs):
    """U = 4 858: one tile of the level-1 scatter, about nine words per coarse bin, just above the grouping's floor"""
    words, filt = synth_words(12_000, 7, 24, p_sub=8e-3, p_n=1e-3)
    assert 4096 < n_unique(words, filt) <= 8192
    s, info, info0 = steady(recs, pairs, words, filt, 24, 1, methods=(False, True))
    assert info == dict(searched_on_records=1, orders_stored=0), info
    assert info0 == dict(searched_on_records=0, orders_stored=1), info0


@pytest.fixture(scope="module")
def three_tiles():
    words, filt = synth_words(50_000, 6, 24, p_sub=8e-3, p_n=1e-3)
    assert 2 * 8192 < n_unique(words, filt) <= 3 * 8192
    return words, filt


def test_three_scatter_tiles(recs, pairs, three_tiles):
    """U = 20 467: the records of a coarse bin come in runs from three tiles"""
    words, filt = three_tiles
    s, info, info0 = steady(recs, pairs, words, filt, 24, 1, methods=(False, True))
    assert info == dict(searched_on_records=1, orders_stored=0), info


def test_below_the_floor_of_the_grouping(recs, pairs, three_tiles):
    words, filt = three_tiles
    words, filt = words[:4000], filt[:4000]
    assert n_unique(words, filt) < 4096
    s, info, info0 = steady(recs, pairs, words, filt, 24, 1)
    assert info["searched_on_records"] == 0, info


def test_same_shape_twice_then_smaller_shapes(recs, pairs, three_tiles):
    """k_group_fine_recs leaves the cursors it read at zero: a count left behind by the 512 bins of the first shape would
    show as doubled or missing pairs in the second run, in the 512 sparser bins of the next shape or in the 256 bins
    of the last (d = 2: keys of 16 bits)"""
    words, filt = three_tiles
    small, sfilt = synth_words(12_000, 7, 24, p_sub=8e-3, p_n=1e-3)
    on_records = 0
    for w, f, d in ((words, filt, 1), (words, filt, 1), (small, sfilt, 1), (words, filt, 2), (words, filt, 2), (small, sfilt, 2),
                    (words, filt, 1)):
        s, roads, info, info0 = both(recs, pairs, w, f, 24, d, deep=False)
        assert info["searched_on_records"] == d, (d, info)
        if roads == NO_RETRY:                                 # (the first run of a shape with more pairs may regrow the regions)
            assert info["orders_stored"] == 0, (d, info)
            on_records += 1
    assert on_records >= 4


# ---- 24 nt, d = 2 ----

@pytest.fixture(scope="module")
def ten_thousand():
    words, filt = synth_words(25_000, 6, 24, p_sub=8e-3, p_n=1e-3)
    assert 9000 < n_unique(words, filt) < 11_000
    return words, filt


def test_six_combinations_of_two_fields(recs, pairs, ten_thousand):
    """U = 10 356 in four segments of 6 nt (plan_segments 4; the plan of this U takes three): six combinations of two
    12-bit fields, five of them grouped -- fields 0+2, 0+3, 1+2, 1+3, 2+3, so the squeezed bits sit at 39, 27 and 15 of
    the word and the second field is not next to the first in three of them"""
    words, filt = ten_thousand
    s, info, info0 = steady(recs, pairs, words, filt, 24, 2, options=[("plan_segments", 4, 0)])
    assert info == dict(searched_on_records=5, orders_stored=0), info
    assert info0 == dict(searched_on_records=0, orders_stored=5), info0


def test_three_combinations_of_one_field(recs, pairs, ten_thousand):
    """the plan this U takes by itself: three segments of 8 nt, keys of 16 bits in 256 coarse bins"""
    words, filt = ten_thousand
    s, info, info0 = steady(recs, pairs, words, filt, 24, 2)
    assert info == dict(searched_on_records=2, orders_stored=0), info


# ---- the 64-bit boundary of a record ----

@pytest.mark.parametrize("which", ["fits", "one_more", "n32"])
def test_record_of_64_bits_and_beyond(recs, pairs, which):
    """13 bits of walk index (U <= 8 192): 2 n - 9 + 13 <= 64 holds up to n = 30, a record of exactly 64 bits; the key of the
    second combination is the top 24 bits of the word's second half, so the squeezed bits start at bit 21 there.  n = 31 and
    n = 32 must take the 12-byte pairs"""
    ibits = 13
    fits = max(n for n in range(1, 33) if 2 * n - 9 + ibits <= 64)
    assert fits == 30
    n = dict(fits=fits, one_more=fits + 1, n32=32)[which]
    words, filt = synth_words(18_000, 6, n, p_sub=8e-3, p_n=1e-3)
    u = n_unique(words, filt)
    assert 4096 < u <= 8192 and bits_for(u) == ibits
    s, info, info0 = steady(recs, pairs, words, filt, n, 1, methods=(False, True))
    assert s["edges"] > 100
    assert info == (dict(searched_on_records=1, orders_stored=0) if n == fits else dict(searched_on_records=0, orders_stored=1)), (n, info)


# ---- a pair at the very end of a bin, and of the order ----

def test_bin_and_order_end_at_a_neighbour_pair(recs, pairs):
    """A bin's buckets come out by ascending key, so the words with the largest suffix a bin can hold (c << 15 | 0x7fff) are
    its last: two of them that differ in one nucleotide of the prefix make the bin's last two positions a pair -- in the
    first bin, in one in the middle, and in bin 511, where they are the last two words of the whole order"""
    rng = np.random.default_rng(77)
    uniq = np.unique(rng.integers(0, 4 ** 24, size=5000, dtype=U64))
    extras = []
    for c in (0, 200, 511):
        a = (U64(int(rng.integers(0, 4 ** 12))) << U64(24)) | U64(c << 15 | 0x7FFF)
        extras += [a, a ^ (U64(2) << U64(40))]
        assert not ((uniq & U64(0xFFFFFF)) == (a & U64(0xFFFFFF))).any()
    uniq = np.unique(np.concatenate([uniq, np.array(extras, U64)]))
    assert 4096 < len(uniq) <= 8192
    words = np.repeat(uniq, rng.integers(1, 4, size=len(uniq)))
    words = np.ascontiguousarray(words[rng.permutation(len(words))])
    s, info, info0 = steady(recs, pairs, words, np.zeros(len(words), np.uint8), 24, 1, methods=(False, True))
    assert s["edges"] >= 3
    assert info == dict(searched_on_records=1, orders_stored=0), info


# ---- the retries ----

def far_bucket_words():
    """5 000 random words and 40 that share one suffix: ten pairs of prefixes one nucleotide apart and twenty random
    prefixes -- a bucket of 40 in the suffix combination, beyond a walk of 7 or 1"""
    rng = np.random.default_rng(40)
    uniq = rng.integers(0, 4 ** 24, size=5000, dtype=U64)
    prefix = rng.choice(4 ** 12, size=30, replace=False).astype(U64)
    twin = prefix[:10] ^ (U64(1) << (U64(2) * rng.integers(0, 12, size=10).astype(U64)))
    bucket = (np.concatenate([prefix, twin]) << U64(24)) | U64(0x2B67C1)
    uniq = np.unique(np.concatenate([uniq, bucket]))
    assert ((uniq & U64(0xFFFFFF)) == U64(0x2B67C1)).sum() == 40
    words = np.repeat(uniq, rng.integers(1, 4, size=len(uniq)))
    return np.ascontiguousarray(words[rng.permutation(len(words))])


@pytest.mark.parametrize("walk", [7, 1])
def test_order_made_after_the_fact_for_the_tiles(fresh_both, walk):
    """the search rides on records and reports a bucket beyond the walk; only then is the order of that combination made,
    by the launches that store it, for the tiles and for k_pairs_append in the second attempt"""
    a, b = fresh_both
    words = far_bucket_words()
    filt = np.zeros(len(words), np.uint8)
    for _ in range(2):
        s, roads, info, info0 = both(a, b, words, filt, 24, 1, options=[("bucket_walk", walk, 1024)])
        assert roads == dict(events=["FAR_TILES"], n_events=1, graph_attempts=2), roads
        assert info == dict(searched_on_records=1, orders_stored=1), info
        assert info0 == dict(searched_on_records=0, orders_stored=1), info0
        assert s["edges"] >= 10


def test_full_region_behind_a_ride(fresh_both):
    """5 743 pairs against the 4 096 slots of a fresh context: the attempt is thrown away and nothing was stored.  The next
    attempt makes the order and searches it with k_pairs_append, as a context that stored it in the first attempt does --
    the attempts are the same on both (a ride in every attempt would take fewer: one region per coarse bin against one
    per 1 024 positions) -- and finds every pair"""
    a, b = fresh_both
    words, filt = synth_words(40_000, 6, 24, p_sub=8e-3, p_n=1e-3)
    s, roads, info, info0 = both(a, b, words, filt, 24, 1)
    assert s["edges"] > 4096 and roads["events"] == ["REGIONS_REGROWN"] * roads["n_events"] and roads["n_events"] >= 1, roads
    assert info == dict(searched_on_records=1, orders_stored=1), info
    assert info0 == dict(searched_on_records=0, orders_stored=1), info0
    s, roads, info, info0 = both(a, b, words, filt, 24, 1)
    assert roads == NO_RETRY and info == dict(searched_on_records=1, orders_stored=0), (roads, info)


def test_full_padded_bin(fresh_both):
    """6 000 words that share their last twelve nucleotides among 5 000 random ones: one coarse bin of the suffix
    combination gets 6 000 records against a room of 1 050.  The scatter of records raises the grouping's own counter,
    the run goes on with exact bins and the launches that store the orders, and so does every later run of the context"""
    a, b = fresh_both
    rng = np.random.default_rng(512)
    hi = rng.choice(4 ** 9, size=6000, replace=False).astype(U64)
    uniq = np.unique(np.concatenate([(hi << U64(24)) | U64(0x5A3C96), rng.integers(0, 4 ** 24, size=5000, dtype=U64)]))
    assert len(uniq) // 512 + len(uniq) // 512 // 4 + 1024 < 6000
    words = np.repeat(uniq, rng.integers(1, 4, size=len(uniq)))
    words = np.ascontiguousarray(words[rng.permutation(len(words))])
    filt = np.zeros(len(words), np.uint8)
    s, roads, info, info0 = both(a, b, words, filt, 24, 1)
    assert roads["events"][0] == "ORDERS_REDONE" and roads["events"].count("ORDERS_REDONE") == 1, roads
    assert info == dict(searched_on_records=1, orders_stored=1), info
    s, roads, info, info0 = both(a, b, words, filt, 24, 1)
    assert "ORDERS_REDONE" not in roads["events"] and info == dict(searched_on_records=0, orders_stored=1), (roads, info)
    words, filt = synth_words(12_000, 7, 24, p_sub=8e-3, p_n=1e-3)
    s, roads, info, info0 = both(a, b, words, filt, 24, 1)
    assert info == dict(searched_on_records=0, orders_stored=1), info


# ---- grouped runs ----

def grouped_both(recs, pairs, words, groups, filt, n, n_groups):
    truth = gt.per_group(words, groups, filt, n, distance=1, method=0, first_read=False)
    assert truth["summary"]["unique"] > 4096 and truth["summary"]["edges"] > 0
    out = []
    for dd in (recs, recs, pairs, pairs):                     # (a first run may regrow the regions)
        gt.assert_same(truth, gt.device_result(dd, words, groups, filt, n, n_groups=n_groups, distance=1, method=0))
        out.append((dd.run_roads(), dd.group_records_info()))
    assert out[0][0] == out[2][0] and out[1][0] == out[3][0] == NO_RETRY, out
    assert out[3][1]["searched_on_records"] == 0, out
    return out[1][1], out[3][1]


def test_grouped_run_of_two_groups(recs, pairs):
    """the group field (one nucleotide) is the first field of every key and narrower than the coarse bin's 9 bits: no
    squeeze, the 12-byte pairs"""
    words, filt = synth_words(12_000, 7, 24, p_sub=8e-3, p_n=1e-3)
    w, f = np.concatenate([words, words]), np.concatenate([filt, filt])
    g = np.repeat(np.arange(2, dtype=np.uint32), len(words))
    info, info0 = grouped_both(recs, pairs, w, g, f, 24, 2)
    assert info == dict(searched_on_records=0, orders_stored=1), info


def test_grouped_run_whose_group_field_holds_the_coarse_bin(recs, pairs):
    """300 groups: a group field of 5 nucleotides above 12-nt words, 10 bits of which the top 9 are the coarse bin -- the
    squeezed bits lie in the group field, at bit 25 of a 34-bit word"""
    words, filt = synth_words(16_000, 9, 12, p_sub=8e-3, p_n=1e-3, shuffle=False)      # (families stay together: 1 377 pairs)
    g = ((np.arange(len(words), dtype=np.uint64) * 300) // len(words)).astype(np.uint32)
    info, info0 = grouped_both(recs, pairs, words, g, filt, 12, 300)
    assert info == dict(searched_on_records=1, orders_stored=0), info
