"""-m gpu: the host waits that stand behind their publishing kernel with work queued after it (option overlap_waits:
the record count's squeeze behind the publish of U; the front of the rest graph's build -- rank blocks and nodes --
behind the publish of the split's counters) and the level 2 of the record count without a tile table (option
static_tiles).  Every case runs on a context with both options on, on a context with both off, and against the CPU
oracle: cluster ids, keep flags, summary; the roads of a run and its attempts equal on both contexts.
Dedup.wait_overlap_info says how many host waits a run took and how many had work queued behind the publishing kernel,
so the road is asserted and not assumed: both contexts wait equally often, and the one with the options on has one
more overlapped wait for a record count and one more for every attempt of the compact graph stage.

The count takes the record road above 11 200 reads (350 << 5: six bucket bits and more); its first level has 2^d1 padded
coarse bins, d1 = (bucket bits + 1) / 2, each with room cap1 = N / bins + N / bins / 4 + 1 024 records; a level-2 tile
is 8 192 records; a component of more than 32 nodes needs the late fetch of the node count."""
import numpy as np
import pytest

import humid_amd
import paired_truth as pt
from humid_amd.synth import synth_wide_words, synth_words
from test_gpu_edit import check_edit
from test_gpu_group_records import NO_RETRY, n_unique
from test_gpu_parity import oracle_full
from test_oracle_vs_bruteforce import indel_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
TILE = 8192


def context(on):
    """word-ordered buckets forced: the default decides for them from 65 536 reads on only, and the record road is
    theirs"""
    d = humid_amd.Dedup()
    d.set_option("count_order", 1)
    d.set_option("overlap_waits", on)
    d.set_option("static_tiles", on)
    return d


@pytest.fixture(scope="module")
def on():
    d = context(1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def off():
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


def assert_waits(r_on, r_off):
    """(roads, wait info, summary) of the same run on the two contexts"""
    (roads, wo, s), (roads0, wo0, s0) = r_on, r_off
    print("waits", wo, wo0, roads)
    assert roads == roads0, (roads, roads0)
    assert wo["host_waits"] == wo0["host_waits"], (wo, wo0)
    rec = 1 if s["records8"] or "PART_PADDED_REDO" in roads["events"] else 0
    assert wo["overlapped"] - wo0["overlapped"] == rec + roads["graph_attempts"], (wo, wo0, roads, rec)
    for k in ("total", "usable", "unique", "clusters", "edges", "count_mode_used", "records8"):
        assert s[k] == s0[k], k


def three_ways(on, off, words, filt, n, d, maximum=False, deep=True):
    """the run on both contexts against ONE oracle run; returns (summary, roads, wait info) of the context with the
    options on.  deep: the accessors that build the graph over all pairs, on both"""
    p, ocid, okeep = oracle_full(words, filt, n, d, maximum)
    os_ = p.summary()
    res = []
    for dd in (on, off):
        cid, keep, s = dd.run(words, filt, word_nt=n, distance=d, method=int(maximum))
        roads, wo = dd.run_roads(), dd.wait_overlap_info()
        for k in ("total", "usable", "unique", "clusters", "edges"):
            assert s[k] == os_[k], (k, s[k], os_[k])
        assert np.array_equal(cid, ocid) and np.array_equal(keep, okeep)
        if deep and s["unique"]:
            lv, olv = dd.leaves(), p.leaves()
            for k in ("word", "degree", "cluster_id", "is_max_leaf"):
                assert np.array_equal(lv[k], olv[k]), k
            assert np.array_equal(lv["count"].astype(np.uint64), olv["count"])
            off_, idx = dd.adjacency()
            ooff, oidx = p.adjacency()
            assert np.array_equal(off_.astype(np.uint64), ooff) and np.array_equal(idx, oidx)
            cl, ocl = dd.clusters(), p.clusters()
            assert np.array_equal(cl["size"], ocl["size"]) and np.array_equal(cl["max_leaf"], ocl["max_leaf"])
            assert dd.run_roads() == roads and dd.wait_overlap_info() == wo       # (the accessors leave both records alone)
        res.append((roads, wo, s))
    assert_waits(res[0], res[1])
    return res[0][2], res[0][0], res[0][1]


def reads_of(rng, uniq, hi=4):
    words = np.repeat(uniq, rng.integers(1, hi, size=len(uniq)))
    return np.ascontiguousarray(words[rng.permutation(len(words))])


# ---- the record road ----

@pytest.mark.parametrize("maximum", [False, True])
def test_record_road_reached(on, off, maximum):
    """40 000 reads: seven bucket bits, 16 coarse bins of one tile each.  The second run of a context is the steady
    state: one attempt, and exactly two overlapped waits more than without the options -- behind the count, behind the
    split"""
    words, filt = synth_words(40_000, 6, 24, p_sub=8e-3, p_n=1e-3)
    three_ways(on, off, words, filt, 24, 1, maximum, deep=False)
    s, roads, wo = three_ways(on, off, words, filt, 24, 1, maximum)
    assert s["records8"], s
    assert roads == NO_RETRY, roads
    wo0 = off.wait_overlap_info()
    assert wo["overlapped"] == wo0["overlapped"] + 2 and wo["overlapped"] >= 2, (wo, wo0)


def test_second_tile_slot_of_every_coarse_bin(on, off):
    """600 000 uniform reads: 350 << 10 < 600 000 <= 350 << 11, eleven bucket bits, d1 = 6: 64 coarse bins of about 9 350
    records in a room of 9 375 + 2 343 + 1 024 = 12 742 -- every bin has one full tile and one partial tile, the grid two
    tile slots per bin"""
    words, filt = synth_words(600_000, 9, 24, p_sub=3e-3, p_n=1e-3)
    N = len(words)
    cap1 = N // 64 + N // 64 // 4 + 1024
    assert TILE < (N - int(filt.sum())) // 64 * 0.95 and (cap1 + TILE - 1) // TILE == 2
    s, roads, wo = three_ways(on, off, words, filt, 24, 1, deep=False)
    assert s["records8"], s


def test_one_bin_between_a_tile_and_its_room(on, off):
    """400 000 uniform reads and 2 270 reads more in the middle of coarse bin 37: eleven bucket bits as above, 64 bins,
    N = 402 270, cap1 = 6 285 + 1 571 + 1 024 = 8 880.  A bin of the uniform reads holds about 6 230 records, one partial
    tile; bin 37 about 8 500: more than a tile (8 192), less than its room -- the only bin with a second tile, of about
    300 records.  The key of a read is its word over 48 bits, its coarse bin the top six of them"""
    rng = np.random.default_rng(37)
    base, bfilt = synth_words(400_000, 11, 24, p_sub=3e-3, p_n=1e-3)
    extra = (U64(37) << U64(42)) | (U64(1) << U64(41)) | rng.integers(0, 1 << 40, size=2270, dtype=U64)
    words = np.concatenate([base, extra])
    filt = np.concatenate([bfilt, np.zeros(len(extra), np.uint8)])
    order = rng.permutation(len(words))
    words, filt = np.ascontiguousarray(words[order]), np.ascontiguousarray(filt[order])
    N = len(words)
    assert 350 << 10 < N <= 350 << 11
    cap1 = N // 64 + N // 64 // 4 + 1024
    usable = words[filt == 0]
    fills = np.bincount((usable >> U64(42)).astype(np.int64), minlength=64)
    assert TILE < fills[37] <= cap1 and (np.delete(fills, 37) < TILE).all(), (fills[37], cap1, fills.max())
    s, roads, wo = three_ways(on, off, words, filt, 24, 1, deep=False)
    assert s["records8"], s


def test_a_bin_outgrows_its_room(fresh_both):
    """60 000 reads, a third of them one word: eight bucket bits, 16 coarse bins with room for 3 750 + 937 + 1 024 = 5 711
    records, one of which receives 21 000.  Level 2 cuts that bin's fill to its room, the run is discarded
    (PART_PADDED_REDO) and counted again by the exact partition, as without the options; the context remembers"""
    a, b = fresh_both
    rng = np.random.default_rng(77)
    words, filt = synth_words(60_000, 9, 24, p_sub=3e-3, p_n=1e-3)
    words = words.copy()
    words[rng.random(len(words)) < 0.35] = U64(0x0123456789AB)
    assert (words == U64(0x0123456789AB)).sum() > 60_000 // 16 + 60_000 // 16 // 4 + 1024
    s, roads, wo = three_ways(a, b, words, filt, 24, 1)
    assert roads["events"].count("PART_PADDED_REDO") == 1, roads
    assert not s["records8"], s
    s, roads, wo = three_ways(a, b, words, filt, 24, 1, deep=False)
    assert "PART_PADDED_REDO" not in roads["events"] and not s["records8"], (roads, s)


def test_two_word_record_count(on, off):
    """48 nt: the second site of the early publish, around k_compact_padded8_wide (70 000 reads: the two-word count takes
    buckets from 65 536 reads on)"""
    words, filt = synth_wide_words(70_000, 948, 48, p_sub=4e-3, p_n=1e-3)
    for maximum in (False, True):
        s, roads, wo = three_ways(on, off, words, filt, 48, 1, maximum, deep=not maximum)
        assert s["records8"], s


# ---- the front of the rest build on discarded attempts ----

def test_front_on_attempts_that_regrow_the_regions(fresh_both):
    """U = 4 858 on fresh contexts: the regions are full twice, three attempts; the front ran behind each publish and
    only the last one's output is used"""
    a, b = fresh_both
    words, filt = synth_words(12_000, 7, 24, p_sub=8e-3, p_n=1e-3)
    s, roads, wo = three_ways(a, b, words, filt, 24, 1)
    assert roads == dict(events=["REGIONS_REGROWN"] * 2, n_events=2, graph_attempts=3), roads
    assert wo["overlapped"] >= 3, wo
    s, roads, wo = three_ways(a, b, words, filt, 24, 1, maximum=True)
    assert roads == NO_RETRY, roads


def test_front_on_attempts_with_a_full_padded_bin_and_far_tiles(fresh_both):
    """the 6 000 words of tests/test_gpu_retries.py that share their last twelve nucleotides: a padded bin of a bucket
    order is full (ORDERS_REDONE), then a bucket is longer than the walk (FAR_TILES: the tiles run between the front
    and the next attempt, and the last attempt's back follows its own front)"""
    a, b = fresh_both
    rng = np.random.default_rng(512)
    hi = rng.choice(4 ** 9, size=6000, replace=False).astype(U64)
    uniq = np.unique((hi << U64(24)) | U64(0x5A3C96))
    words = reads_of(rng, uniq, 6)
    filt = np.zeros(len(words), np.uint8)
    s, roads, wo = three_ways(a, b, words, filt, 24, 1)
    ev = roads["events"]
    assert "ORDERS_REDONE" in ev and "FAR_TILES" in ev[ev.index("ORDERS_REDONE"):], roads
    # (the words all lie below 2^42, in the count's first coarse bin: with word-ordered buckets forced that bin outgrows
    # its room too, PART_PADDED_REDO in front of the graph stage's events -- a discarded record count, then discarded attempts)
    assert ev[0] == "PART_PADDED_REDO" and roads["graph_attempts"] == roads["n_events"], roads
    s, roads, wo = three_ways(a, b, words, filt, 24, 1, deep=False)
    assert roads == dict(events=["FAR_TILES"], n_events=1, graph_attempts=2), roads


# ---- no rest pair ----

def test_no_pair_at_all(on, off):
    rng = np.random.default_rng(3)
    words = reads_of(rng, np.unique(rng.integers(0, 4 ** 24, size=2000, dtype=U64)))
    s, roads, wo = three_ways(on, off, words, np.zeros(len(words), np.uint8), 24, 1)
    assert s["edges"] == 0 and roads == NO_RETRY, (s, roads)


def test_isolated_pairs_only(on, off):
    """500 words and one neighbour of each: every pair is settled from the pair list, the front runs over an empty
    bitmap and no back follows; the accessors build the graph over all pairs afterwards"""
    rng = np.random.default_rng(4)
    a = np.unique(rng.integers(0, 4 ** 24, size=500, dtype=U64))
    b = a ^ (U64(1) << (U64(2) * rng.integers(0, 24, size=len(a)).astype(U64)))
    words = reads_of(rng, np.concatenate([a, b]))
    filt = np.zeros(len(words), np.uint8)
    for maximum in (False, True):
        p, ocid, okeep = oracle_full(words, filt, 24, 1, maximum)
        for dd in (on, off):
            cid, keep, s = dd.run(words, filt, word_nt=24, distance=1, method=int(maximum))
            assert np.array_equal(cid, ocid) and np.array_equal(keep, okeep)
            info = dd.graph_split_info()
            assert info == dict(pairs_direct=len(a), pairs_graph=0, full_graph_built=0), info
        s, roads, wo = three_ways(on, off, words, filt, 24, 1, maximum)
        assert s["edges"] == len(a) and roads == NO_RETRY, (s, roads)


# ---- the late fetch of the node count behind the new order ----

def chain(rng, length):
    """`length` words, each one nucleotide from the one before: one component"""
    w = [int(rng.integers(0, 4 ** 24))]
    for i in range(1, length):
        w.append(w[-1] ^ (1 << (2 * (i % 24))))
    assert len(set(w)) == length
    return np.array(w, U64)


@pytest.mark.parametrize("length,fetched", [(40, True), (5, False), (33, True), (32, False)])
def test_one_chain(on, off, length, fetched):
    """a chain of 40 words has 39 rest pairs (32 and more: the node count and the members of large components are fetched
    while the small components are clustered) and one component above 32 nodes; a chain of 5 has 4 rest pairs and
    the fetch is skipped; 33 and 32 words stand on the two sides of both thresholds"""
    rng = np.random.default_rng(length)
    words = reads_of(rng, chain(rng, length), 6)
    filt = np.zeros(len(words), np.uint8)
    for maximum in (False, True):
        s, roads, wo = three_ways(on, off, words, filt, 24, 1, maximum)
        assert s["edges"] >= length - 1 and roads == NO_RETRY, (s, roads)
        # (the split's wait, and the fetch beside k_cluster_small_lds where it is taken)
        assert wo["overlapped"] == (2 if fetched else 1), wo


# ---- other inputs of the same branch ----

def test_given_pairs(on, off):
    """-e, d = 2 over 16-nt words: the graph stage gets its pairs as a list and splits them in the same branch"""
    rng = np.random.default_rng(16)
    words = indel_words(rng, 3000, 16)
    filt = (rng.random(len(words)) < 0.02).astype(np.uint8)
    got = []
    for dd in (on, off):
        roads = []
        try:
            check_edit(dd, words, filt, 16, 2, False, deep=False, roads=roads)
            wo, s = dd.wait_overlap_info(), dd.summary
            check_edit(dd, words, filt, 16, 2, True, deep=True)
        finally:
            dd.set_option("edit_distance", 0)
        got.append((roads[0], wo, s))
    assert got[0][0] == got[1][0] and got[0][0]["graph_attempts"] == 1, got
    assert got[0][1]["host_waits"] == got[1][1]["host_waits"] and got[0][1]["overlapped"] > got[1][1]["overlapped"], got


@pytest.mark.parametrize("n", [24, 48])
def test_strand_symmetric_run(on, off, n):
    words, filt = pt.families(1000 * n + 1, n, 5000, 1)
    for method in (0, 1):
        t = pt.run(words, filt, n, 1, method)
        got = []
        for dd in (on, off):
            cid, keep, s = dd.run_paired(words, filt, word_nt=n, distance=1, method=method)
            got.append((dd.run_roads(), dd.wait_overlap_info()))
            for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle"):
                assert s[k] == t["summary"][k], (k, s[k], t["summary"][k])
            assert np.array_equal(cid, t["cluster_id"]) and np.array_equal(keep, t["keep"])
            lv = dd.leaves()
            for k in ("word", "degree", "cluster_id", "is_max_leaf"):
                assert np.array_equal(lv[k], t["leaves"][k]), k
        assert got[0][0] == got[1][0], got
        assert got[0][1]["host_waits"] == got[1][1]["host_waits"] and got[0][1]["overlapped"] > got[1][1]["overlapped"], got


def test_edge_cases(on, off):
    """everything filtered; one usable read; and a large shape followed by a small one on the same contexts -- the
    front's arrays are sized by a bound, the back's by the rest pairs of the run"""
    w = np.array([5, 6, 7, 8], U64)
    three_ways(on, off, w, np.ones(4, np.uint8), 24, 1)
    three_ways(on, off, w, np.array([1, 1, 0, 1], np.uint8), 24, 1)
    big, bfilt = synth_words(120_000, 21, 24, p_sub=8e-3, p_n=1e-3)
    small, sfilt = synth_words(3000, 22, 24, p_sub=2e-2, p_n=1e-3)
    assert n_unique(small, sfilt) < 4096
    for words, filt in ((big, bfilt), (small, sfilt), (big, bfilt), (small, sfilt)):
        s, roads, wo = three_ways(on, off, words, filt, 24, 1, deep=len(words) < 10_000)
        assert s["edges"] > 0
