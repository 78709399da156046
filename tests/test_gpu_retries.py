"""-m gpu: the retries of the pair search, asserted from the record the host keeps of them (Dedup.run_roads,
humid_get_run_roads) -- several retries in ONE run, which is the state that crosses the attempts of the compact graph
stage's loop (the bucket orders kept, the far list dropped on a regrow), and what the context remembers from run to run
(the room of the regions, the padding of the groupings).  Every run is compared with the CPU oracle in all arrays, on a
context that splits its pairs (pair_split 1) and on one that does not.

Inputs are small (about 10 000 to 16 000 unique words).  The padded room of a coarse bin is U / bins + U / bins / 4 +
1 024 words, the bounded walk 1 024 followers, and a fresh context starts with max(U / 4, 4 096) slots for pairs in 64
regions."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib
from test_gpu_edit import check_edit
from test_gpu_keyed import keyed_result
from test_gpu_parity import check_against_oracle
from test_oracle_vs_bruteforce import indel_words

import grouped_truth as gt

pytestmark = pytest.mark.gpu

U64 = np.uint64
GRAPH_ROADS = ("ORDERS_REDONE", "REGIONS_REGROWN", "FAR_TILES")


@pytest.fixture(params=[1, 0], ids=["pair_split", "whole_graph"])
def fresh(request):
    """a context nothing has run on: full padding, no room remembered"""
    d = humid_amd.Dedup()
    d.set_option("pair_split", request.param)
    d.pair_split = request.param
    yield d
    d.close()


def reads_of(rng, uniq):
    """every word one to five times, read order shuffled"""
    words = np.repeat(uniq, rng.integers(1, 6, size=len(uniq)))
    return np.ascontiguousarray(words[rng.permutation(len(words))])


def assert_loop_counted(r):
    """every event of a plain Hamming run on the compact graph is one discarded attempt of its loop"""
    assert set(r["events"]) <= set(GRAPH_ROADS), r
    assert r["graph_attempts"] == 1 + r["n_events"] and r["graph_attempts"] <= 6, r


def three_retry_words():
    """block A: the 6 000 words of test_padded_coarse_bin_full_on_the_first_run (last twelve nucleotides constant: one
    coarse bin and one bucket of 6 000 in the second combination).  Block B: 16 random 20-nt prefixes with all 256
    values of the last four nucleotides: every word has 12 neighbours inside its family, 16 * 256 * 12 / 2 = 24 576
    pairs at least"""
    rng = np.random.default_rng(512)
    hi = rng.choice(4 ** 9, size=6000, replace=False).astype(U64)
    a = (hi << U64(24)) | U64(0x5A3C96)
    prefixes = rng.choice(4 ** 20, size=16, replace=False).astype(U64)
    b = ((prefixes << U64(8))[:, None] | np.arange(256, dtype=U64)[None, :]).reshape(-1)
    uniq = np.unique(np.concatenate([a, b]))
    assert 10_000 <= len(uniq) <= 6000 + 4096
    assert len(uniq) // 512 + len(uniq) // 512 // 4 + 1024 < 6000                 # a padded bin is full
    assert 24_576 > 64 * 64 and max(len(uniq) // 4, 4096) == 4096                 # a region is full, wherever the pairs land
    return reads_of(rng, uniq)


def test_three_retries_in_one_run_and_the_context_forgets(fresh):
    """24 nt, d = 1, default options.  The first run of a fresh context meets a full padded bin (6 000 words against a room
    of 1 047), a bucket longer than the walk (6 000 against 1 024) and full regions (24 576 pairs and more against 4 096
    slots): each of ORDERS_REDONE, REGIONS_REGROWN and FAR_TILES at least once, every one a discarded attempt.  The
    second run of the same input is the steady state: the tiles alone.

    Then the context forgets: 10 000 random words with almost no pairs retry nothing and shrink the regions' room, so the
    first input regrows the regions again -- but the padding of the groupings stays off for the context.

    Observed on the MI355X, both contexts alike:
      first run   ['ORDERS_REDONE', 'REGIONS_REGROWN', 'FAR_TILES']   (graph_attempts 4)
      second run  ['FAR_TILES']                                       (graph_attempts 2)
      random      []                                                  (graph_attempts 1)
      again       ['REGIONS_REGROWN', 'FAR_TILES']                    (graph_attempts 3)"""
    words = three_retry_words()
    filt = np.zeros(len(words), np.uint8)
    roads = []
    check_against_oracle(fresh, words, filt, 24, 1, False, deep=True, roads=roads)
    first = roads[0]
    for road in GRAPH_ROADS:
        assert first["events"].count(road) >= 1, first
    assert_loop_counted(first)
    check_against_oracle(fresh, words, filt, 24, 1, False, deep=True, roads=roads)
    assert roads[1] == dict(events=["FAR_TILES"], n_events=1, graph_attempts=2), roads[1]

    rng = np.random.default_rng(513)
    sparse = rng.integers(0, 4 ** 24, size=10_000, dtype=U64)
    s = check_against_oracle(fresh, sparse, np.zeros(len(sparse), np.uint8), 24, 1, False, deep=True, roads=roads)
    assert s["edges"] < 64                                    # (almost no pairs)
    assert roads[2] == dict(events=[], n_events=0, graph_attempts=1), roads[2]

    check_against_oracle(fresh, words, filt, 24, 1, False, deep=True, roads=roads)
    again = roads[3]
    assert again["events"].count("REGIONS_REGROWN") >= 1 and "ORDERS_REDONE" not in again["events"], again
    assert "FAR_TILES" in again["events"], again
    assert_loop_counted(again)


def wide(lo):
    """36-nt words whose first four nucleotides are A: u64[N, 2], [:, 1] = the last 32 nucleotides"""
    return np.stack([np.zeros(len(lo), U64), lo], 1)


def test_two_word_words(fresh):
    """36 nt, d = 2: three segments of 12 nt, three combinations of one segment, every key 24 bits -- grouped at U >=
    4 096 (at 40 nt, d = 1 the keys are 40 bits and nothing is grouped).  6 000 words that differ in nucleotides 7 .. 11
    and 19 .. 23 only and share their last twelve: one coarse bin and one bucket of 6 000 in the third combination.  And
    16 random values of nucleotides 4 .. 31 with all 256 values of the last four nucleotides: 66 neighbours a word inside the family,
    135 168 pairs against 4 096 slots.

    Observed on the MI355X, both contexts alike:
      first run   ['ORDERS_REDONE', 'REGIONS_REGROWN', 'FAR_TILES']   (graph_attempts 4)
      second run  ['FAR_TILES']                                       (graph_attempts 2)
    so the full padded bin IS reached on two-word words, and asserted."""
    nc, pb = C.c_uint32(), C.c_uint32()
    rng = np.random.default_rng(36)
    hi = rng.choice(4 ** 10, size=6000, replace=False).astype(U64)
    a = ((hi >> U64(10)) << U64(48)) | ((hi & U64(1023)) << U64(24)) | U64(0x5A3C96)
    tails = rng.integers(0, 4 ** 28, size=16, dtype=U64)                           # nucleotides 4 .. 31
    b = ((tails << U64(8))[:, None] | np.arange(256, dtype=U64)[None, :]).reshape(-1)
    uniq = np.unique(np.concatenate([a, b]))
    assert len(uniq) == 6000 + 4096
    assert _lib.load().humid_stage_plan_info(None, 36, 2, len(uniq), C.byref(nc), C.byref(pb)) == 0
    assert (nc.value, pb.value) == (3, 24)
    lo = reads_of(rng, uniq)
    words, filt = wide(lo), np.zeros(len(lo), np.uint8)
    roads = []
    check_against_oracle(fresh, words, filt, 36, 2, False, deep=True, roads=roads)
    first = roads[0]
    for road in GRAPH_ROADS:
        assert first["events"].count(road) >= 1, first
    assert_loop_counted(first)
    check_against_oracle(fresh, words, filt, 36, 2, True, deep=True, roads=roads)
    assert roads[1] == dict(events=["FAR_TILES"], n_events=1, graph_attempts=2), roads[1]


def grouped_words():
    """four groups of all 4 096 six-nt prefixes in front of one six-nt suffix per group: the key of the second
    combination is the group field and the suffix, 14 bits in 128 coarse bins -- 4 096 words a bin against a room of
    16384 / 128 + 16384 / 128 / 4 + 1024 = 1 184; buckets of 4 096 against the walk of 1 024; 4 096 * 18 / 2 = 36 864 pairs
    a group against 4 096 slots"""
    rng = np.random.default_rng(12)
    suffix = rng.choice(4 ** 6, size=4, replace=False).astype(U64)
    uniq = ((np.arange(4096, dtype=U64) << U64(12))[None, :] | suffix[:, None]).reshape(-1)
    groups = np.repeat(np.arange(4, dtype=np.uint32), 4096)
    reps = rng.integers(1, 4, size=len(uniq))
    perm = rng.permutation(int(reps.sum()))
    return np.repeat(uniq, reps)[perm], np.repeat(groups, reps)[perm]


@pytest.fixture(scope="module")
def grouped_case():
    words, groups = grouped_words()
    filt = np.zeros(len(words), np.uint8)
    truth = gt.per_group(words, groups, filt, 12, distance=1, method=0, first_read=False)
    assert truth["summary"]["unique"] == 16_384 and truth["summary"]["edges"] == 4 * 36_864
    return words, groups, filt, truth


def test_run_with_a_group_field(fresh, grouped_case):
    """run_grouped, 12-nt words, 4 groups, d = 1: all three kinds on the first run of a fresh context, and the truth is
    one oracle pass per group, so no pair crosses a group.  The same reads through run_keyed with four arbitrary 64-bit
    keys (ascending with the group, so the ranks are the groups) on another fresh context: the same results and the same
    kinds.

    Observed on the MI355X, both contexts alike:
      grouped, first run   ['ORDERS_REDONE', 'REGIONS_REGROWN', 'FAR_TILES']   (graph_attempts 4)
      grouped, second run  ['FAR_TILES']                                       (graph_attempts 2)
      keyed, first run     ['ORDERS_REDONE', 'REGIONS_REGROWN', 'FAR_TILES']   (graph_attempts 4)"""
    words, groups, filt, truth = grouped_case
    got = gt.device_result(fresh, words, groups, filt, 12, n_groups=4, distance=1, method=0)
    gt.assert_same(truth, got)
    first = fresh.run_roads()
    print("roads", first)
    for road in GRAPH_ROADS:
        assert first["events"].count(road) >= 1, first
    assert_loop_counted(first)
    assert got["idx"].max() < 16_384 and np.array_equal(got["leaves"]["group"], np.repeat(np.arange(4, dtype=np.uint32), 4096))
    lo = np.repeat(np.arange(16_384, dtype=np.int64), np.diff(got["off"].astype(np.int64)))
    assert np.array_equal(lo // 4096, got["idx"].astype(np.int64) // 4096)               # no pair crosses a group
    gt.assert_same(truth, gt.device_result(fresh, words, groups, filt, 12, n_groups=4, distance=1, method=0))
    second = fresh.run_roads()
    print("roads", second)
    assert second == dict(events=["FAR_TILES"], n_events=1, graph_attempts=2), second

    keyed = humid_amd.Dedup()
    try:
        keyed.set_option("pair_split", fresh.pair_split)
        K = np.array([0x11, 0x8000000000000000, 0xDEADBEEF00000007, 0xFFFFFFFFFFFFFFFF], U64)
        kgot = keyed_result(keyed, words, K[groups], filt, 12, distance=1, method=0)
        kroads = keyed.run_roads()
        print("roads", kroads)
        gt.assert_same(truth, kgot)
        assert np.array_equal(kgot["K"], K)
        assert set(kroads["events"]) == set(first["events"]), (kroads, first)
        assert_loop_counted(kroads)
    finally:
        keyed.close()


def test_given_pairs_take_one_attempt(fresh):
    """-e at d = 2 over 16-nt words: the graph stage gets its pairs as a list, which neither regrows nor tiles -- one
    attempt, none of the loop's events.  The candidate joins go through the pieces only where a run of equal keys is
    longer than the walk: not with the default walk of 1 024, with a walk of 8 they do"""
    rng = np.random.default_rng(16)
    words = indel_words(rng, 3000, 16)
    filt = (rng.random(len(words)) < 0.02).astype(np.uint8)
    roads = []
    check_edit(fresh, words, filt, 16, 2, False, deep=True, roads=roads)
    assert roads[0] == dict(events=[], n_events=0, graph_attempts=1), roads[0]
    fresh.set_option("bucket_walk", 8)
    check_edit(fresh, words, filt, 16, 2, False, deep=True, roads=roads)
    assert roads[1]["n_events"] >= 1 and set(roads[1]["events"]) == {"JOIN_PIECES"} and roads[1]["graph_attempts"] == 1, roads[1]


def test_no_record_before_the_first_run():
    dd = humid_amd.Dedup()
    try:
        with pytest.raises(humid_amd.HumidError) as ei:
            dd.run_roads()
        assert ei.value.code == -6                                   # HUMID_E_STATE
        dd.run(np.arange(5, dtype=U64), np.zeros(5, np.uint8), word_nt=24, distance=1)
        assert dd.run_roads() == dict(events=[], n_events=0, graph_attempts=1)
    finally:
        dd.close()


def test_accumulator_calls_report_their_own_events():
    """the record belongs to the last mutating call: add and map count a chunk (no event here, and no graph stage);
    finish builds the per-unique-word graph over the accumulated list, where a bucket of 3 000 words (one shared
    12-nt prefix) is longer than the walk of 1 024 and the tiles complete it: CSR_TILES.  Results against the oracle's
    run over all reads."""
    from oracle import pyoracle as orc
    from test_gpu_parity import one_prefix_words
    words = one_prefix_words(np.random.default_rng(24), 3000, 24, 12)
    filt = np.zeros(len(words), np.uint8)
    ocid, okeep, osum, _ = orc.dedup_run(words, filt, 24, 1, 0)
    nothing = dict(events=[], n_events=0, graph_attempts=0)
    half = len(words) // 2
    dd = humid_amd.Dedup()
    try:
        acc = dd.accumulator(word_nt=24)
        for lo, hi in ((0, half), (half, len(words))):
            acc.add(words[lo:hi], filt[lo:hi])
            assert dd.run_roads() == nothing
        s = acc.finish(distance=1)
        assert dd.run_roads() == dict(events=["CSR_TILES"], n_events=1, graph_attempts=0)
        for k in ("total", "usable", "unique", "clusters", "edges"):
            assert s[k] == osum[k], k
        dd.adjacency()
        assert dd.run_roads() == dict(events=["CSR_TILES"], n_events=1, graph_attempts=0)       # (accessors leave it alone)
        for lo, hi in ((0, half), (half, len(words))):
            cid, keep, unknown = acc.map(words[lo:hi], filt[lo:hi], lo)
            assert unknown == 0 and np.array_equal(cid, ocid[lo:hi]) and np.array_equal(keep, okeep[lo:hi])
            assert dd.run_roads() == nothing
    finally:
        dd.close()
