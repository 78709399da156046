"""-m gpu: the merge of accumulated runs alone (kernels_accum.hip.h), through add + Accumulator.leaves(), no finish.
The words are built by hand so that the merge pattern is known; word, count and first index are compared bit for bit
with the numpy truth (tests/accum_truth.py).  accum_tile = 64 makes a 200-entry merge cross three tile boundaries."""
import numpy as np
import pytest

import humid_amd
from accum_truth import accum_leaves

pytestmark = pytest.mark.gpu

TILES = [64, 2048]                    # the smallest tile and the default
WORD_NT = [24, 33, 48, 64]


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def words_of(vals, n):
    """order-preserving words from small integers: one uint64, or [hi, lo] with BOTH halves varying"""
    if n <= 32:
        return np.array(vals, dtype=np.uint64).reshape(-1)
    q = 1500 if n == 33 else 100          # (n = 33: hi has two bits)
    return np.array([[v // q, v % q] for v in vals], dtype=np.uint64).reshape(-1, 2)


def reads_of(vals, n, seed=0):
    """a chunk holding value v (v % 3) + 1 times, shuffled, with one filtered read in front"""
    rep = [v for v in vals for _ in range(v % 3 + 1)]
    rng = np.random.default_rng(seed + len(rep))
    rng.shuffle(rep)
    w = words_of([0] + rep, n)
    f = np.zeros(len(rep) + 1, np.uint8)
    f[0] = 1
    return w, f


def check(dd, n, tile, chunks):
    """adds the chunks [(words, filtered, base)] and compares the list with the truth after EVERY add"""
    dd.set_option("accum_tile", tile)
    acc = dd.accumulator(n)
    try:
        for k, (w, f, base) in enumerate(chunks):
            assert acc.add(w, f, base) == base
            got, exp = acc.leaves(), accum_leaves(chunks[:k + 1], n)
            assert got["first"].dtype == np.uint64 and got["count"].dtype == np.uint32
            assert np.array_equal(got["word"], exp["word"]), (n, tile, k)
            assert np.array_equal(got["count"], exp["count"].astype(np.uint32)), (n, tile, k)
            assert np.array_equal(got["first"], exp["first"]), (n, tile, k)
        i = acc.info()
        assert i["word_nt"] == n and i["chunks"] == len(chunks) and not i["finished"]
        assert i["total"] == sum(len(f) for _, f, _ in chunks)
        assert i["usable"] == sum(int((f == 0).sum()) for _, f, _ in chunks)
        assert i["unique"] == len(accum_leaves(chunks, n)["count"])
    finally:
        dd.set_option("accum_tile", 2048)
    return acc


def two(dd, n, tile, a, b):
    ca, cb = reads_of(a, n, 1), reads_of(b, n, 2)
    check(dd, n, tile, [ca + (0,), cb + (len(ca[1]),)])


EVEN, ODD = list(range(0, 400, 2)), list(range(1, 400, 2))
PATTERNS = {
    "a_empty": ([], EVEN), "b_empty": (EVEN, []), "equal": (EVEN, EVEN),
    "b_subset_of_a": (list(range(300)), list(range(0, 300, 7))), "a_subset_of_b": (list(range(0, 300, 7)), list(range(300))),
    "even_odd": (EVEN, ODD), "b_below_a": (list(range(200, 400)), list(range(0, 150))),
    "b_above_a": (list(range(0, 150)), list(range(200, 400))), "one_one_equal": ([5], [5]), "one_one_differ": ([5], [4]),
}


@pytest.mark.parametrize("name", sorted(PATTERNS))
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("n", WORD_NT)
def test_merge_patterns(dd, n, tile, name):
    a, b = PATTERNS[name]
    two(dd, n, tile, a, b)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("n", [24, 48])
def test_merge_lengths_on_either_side(dd, n, tile):
    """1, 63, 64, 65, 127, 128, 129 and 1000 entries on either side, about a third of the smaller list shared"""
    rng = np.random.default_rng(n + tile)
    sizes = [1, 63, 64, 65, 127, 128, 129, 1000]
    for la in sizes:
        for lb in sizes:
            pool = rng.permutation(3000)
            a = sorted(pool[:la].tolist())
            share = min(la, lb) // 3
            b = sorted(pool[la - share:la - share + lb].tolist())
            two(dd, n, tile, a, b)


@pytest.mark.parametrize("n", [24, 33, 64])
def test_duplicate_pair_slides_over_a_tile_boundary(dd, n):
    """200 merge positions that alternate a, b, a, b ...; ONE value is in both lists, its a at position p and its b at
    p + 1, for every p in 60 .. 70: with tiles of 64 the pair lies before the boundary, across it (a the last entry of
    tile 0, b the first of tile 1) and behind it"""
    for p in range(60, 71):
        val = [2 * k for k in range(200)]
        val[p + 1] = val[p]
        src = ["a" if k % 2 == 0 else "b" for k in range(200)]
        src[p], src[p + 1] = "a", "b"
        a = [v for v, s in zip(val, src) if s == "a"]
        b = [v for v, s in zip(val, src) if s == "b"]
        assert len(set(a)) == len(a) and len(set(b)) == len(b) and len(set(a) & set(b)) == 1
        for tile in TILES:
            two(dd, n, tile, a, b)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("n", [24, 48])
def test_counts_add_up_over_five_chunks_and_first_is_the_minimum(dd, n, tile):
    """every chunk holds every third value of a common pool plus values of its own; the chunk with the smallest base
    comes LATER, so first indices must go down, and bases beyond 2^32 must come back whole"""
    bases = [2 ** 40, 2 ** 33, 5, 2 ** 40 + 10 ** 6, 2 ** 20]
    chunks = []
    for k, base in enumerate(bases):
        vals = sorted(set(range(k % 3, 900, 3)) | set(range(1000 + 50 * k, 1100 + 50 * k)))
        chunks.append(reads_of(vals, n, 10 + k) + (base,))
    acc = check(dd, n, tile, chunks)
    lv = acc.leaves()
    assert lv["first"].min() >= 5 and lv["first"].max() > 2 ** 32 and lv["count"].max() >= 6


@pytest.mark.parametrize("tile", TILES)
def test_wide_words_that_differ_in_one_half_only(dd, tile):
    ones = 0xffffffffffffffff
    for n, hi_max in ((33, 3), (48, ones >> 32), (64, ones)):
        a = np.array([[0, 5], [1, 5], [hi_max, 5], [hi_max, ones - 1]], dtype=np.uint64)       # differ in hi only / lo only
        b = np.array([[0, 4], [0, 5], [0, 6], [hi_max, 5], [hi_max, ones], [1, 5]], dtype=np.uint64)   # (64: the all-ones word)
        chunks = [(a, np.zeros(len(a), np.uint8), 2 ** 40), (b, np.zeros(len(b), np.uint8), 5),
                  (b[::-1].copy(), np.zeros(len(b), np.uint8), 2 ** 33)]
        acc = check(dd, n, tile, chunks)
        lv = acc.leaves()
        assert len(lv["count"]) == 7 and lv["count"].sum() == 16
        assert lv["word"][-1].tolist() == [hi_max, ones] and lv["first"][-1] == 5 + 4


@pytest.mark.parametrize("n", [24, 48])
def test_empty_and_all_filtered_chunks_leave_the_list_unchanged(dd, n):
    w, f = reads_of(list(range(0, 500, 3)), n)
    empty = (words_of([], n), np.zeros(0, np.uint8), 10 ** 9)
    junk = (words_of([7, 8, 9, 10], n), np.ones(4, np.uint8), 2 * 10 ** 9)
    acc = check(dd, n, 64, [empty, junk, (w, f, 0), empty, junk[:2] + (3 * 10 ** 9,)])
    i = acc.info()
    assert i["chunks"] == 5 and i["total"] == len(f) + 8 and i["usable"] == len(f) - 1
    acc.clear()
    with pytest.raises(humid_amd.HumidError) as ei:
        acc.leaves()
    assert ei.value.code == -6
