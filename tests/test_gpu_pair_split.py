"""-m gpu: neighbour pairs whose two ends have no other pair are settled from the pair list (k_pairs_split,
kernels_cgraph.hip.h; option pair_split), the others go through the compact graph.  Every input runs on a context with
the option on and on one with it off (every pair through the graph): both equal the CPU oracle, their accessors equal
each other array for array, and humid_graph_split_info says which road the pairs took.

Hand-built words are 24 nt at d = 1.  FILLERS come from a code of minimum distance 2: nucleotides 0 .. 18 count i in
base 4, nucleotide 19 is the sum of those digits mod 4, nucleotides 20 .. 23 are zero -- no two fillers are
neighbours.  Changing one of the last four nucleotides of a filler gives a CHILD that is a neighbour of that filler
alone and sorts right behind it, so the number of fillers in front sets the walk indices."""
import numpy as np
import pytest

import humid_amd
from humid_amd.synth import synth_words
from test_gpu_parity import check_against_oracle, dense_words

import grouped_truth as gt

pytestmark = pytest.mark.gpu

U64 = np.uint64


@pytest.fixture(scope="module")
def split():
    d = humid_amd.Dedup()
    d.set_option("pair_split", 1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def whole():
    d = humid_amd.Dedup()
    d.set_option("pair_split", 0)
    yield d
    d.close()


def filler(i):
    digits, x = 0, i
    while x:
        digits += x & 3
        x >>= 2
    return (i << 10) | ((digits & 3) << 8)


def child(word, pos, value):
    """nucleotide 23 - pos (pos 0 .. 3: one of the last four) changed by value 1 .. 3"""
    return word ^ (value << (2 * pos))


class Builder:
    """words in walk order with their counts; every shape takes the next filler as its parent"""

    def __init__(self):
        self.words, self.counts, self.next = [], [], 0
        self.direct = self.graph = 0

    def _parent(self, count):
        w = filler(self.next)
        self.next += 1
        self.words.append(w)
        self.counts.append(count)
        return w

    def _add(self, w, count):
        self.words.append(w)
        self.counts.append(count)

    def fillers(self, k, count=1):
        for _ in range(k):
            self._parent(count)
        return self

    def fill_to(self, index):
        """fillers until the next word gets walk index `index`"""
        assert len(self.words) <= index
        return self.fillers(index - len(self.words))

    def pair(self, cp, cc):
        p = self._parent(cp)
        self._add(child(p, 0, 1), cc)
        self.direct += 1
        return self

    def star(self, cp=5, c1=1, c2=1):
        p = self._parent(cp)
        self._add(child(p, 0, 1), c1)            # 0x1 < 0x4: already ascending
        self._add(child(p, 1, 1), c2)
        self.graph += 2
        return self

    def triangle(self, cp=5, c1=1, c2=2):
        p = self._parent(cp)
        self._add(child(p, 0, 1), c1)
        self._add(child(p, 0, 2), c2)
        self.graph += 3
        return self

    def chain(self, counts=(9, 4, 2, 1)):
        p = self._parent(counts[0])
        c1 = child(p, 0, 1)                      # ...0001
        c2 = child(c1, 1, 1)                     # ...0101
        c3 = child(c2, 2, 1)                     # ...010101
        for w, c in zip((c1, c2, c3), counts[1:]):
            self._add(w, c)
        self.graph += 3
        return self

    def reads(self, seed=0):
        w = np.array(self.words, U64)
        assert np.all(w[1:] > w[:-1]), "not in walk order"
        r = np.repeat(w, np.array(self.counts))
        r = np.ascontiguousarray(r[np.random.default_rng(seed).permutation(len(r))])
        return r, np.zeros(len(r), np.uint8)


def snapshot(dd, words, filt, n, d, maximum, **kw):
    cid, keep, s = dd.run(words, filt, word_nt=n, distance=d, method=int(maximum), **kw)
    before = dd.graph_split_info()
    taken = dd.run_roads()
    off, idx = dd.adjacency()
    return dict(cid=cid, keep=keep, summary={k: s[k] for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle")},
                leaves=dd.leaves(), off=off, idx=idx, clusters=dd.clusters(), info=before, info_after=dd.graph_split_info(),
                roads=taken, roads_after=dd.run_roads())


def assert_same_arrays(a, b):
    for k in ("cid", "keep", "off", "idx"):
        assert np.array_equal(a[k], b[k]), k
    assert a["summary"] == b["summary"]
    for part in ("leaves", "clusters"):
        assert a[part].keys() == b[part].keys()
        for k in a[part]:
            assert np.array_equal(a[part][k], b[part][k]), (part, k)


def split_and_whole(split, whole, words, filt, n=24, d=1, methods=(False, True), options=(), roads=None):
    """both contexts against the oracle and against each other; returns the split context's info per method.
    roads: a list that receives, per method, what the runs retried (Dedup.run_roads): dict(split, whole) of the two
    runs against the oracle -- the FIRST runs of the input on fresh contexts -- and dict(split, whole) of the two runs
    of the same input behind them"""
    infos = []
    try:
        for key, value, _ in options:
            split.set_option(key, value)
            whole.set_option(key, value)
        for maximum in methods:
            first = []
            s1 = check_against_oracle(split, words, filt, n, d, maximum, roads=first)
            s2 = check_against_oracle(whole, words, filt, n, d, maximum, roads=first)
            a = snapshot(split, words, filt, n, d, maximum)
            b = snapshot(whole, words, filt, n, d, maximum)
            print("roads of the second runs", a["roads"], b["roads"])
            assert a["roads_after"] == a["roads"] and b["roads_after"] == b["roads"]      # (the accessors record nothing)
            if roads is not None:
                roads.append(dict(split=first[0], whole=first[1]))
                roads.append(dict(split=a["roads"], whole=b["roads"]))
            for k in ("unique", "clusters", "edges", "nonsingle"):
                assert s1[k] == s2[k] == a["summary"][k], k
            assert_same_arrays(a, b)
            ia, ib = a["info"], b["info"]
            assert ia["pairs_direct"] + ia["pairs_graph"] == s1["edges"]
            assert ib == dict(pairs_direct=0, pairs_graph=s2["edges"], full_graph_built=1)
            assert ia["full_graph_built"] == 0 and a["info_after"]["full_graph_built"] == 1
            assert {k: a["info_after"][k] for k in ("pairs_direct", "pairs_graph")} == {k: ia[k] for k in ("pairs_direct", "pairs_graph")}
            infos.append(ia)
    finally:
        for key, _, restore in options:
            split.set_option(key, restore)
            whole.set_option(key, restore)
    return infos


def hand_built(split, whole, b):
    words, filt = b.reads()
    for info in split_and_whole(split, whole, words, filt):
        assert info["pairs_direct"] == b.direct and info["pairs_graph"] == b.graph, (info, b.direct, b.graph)


# ---- hand-built graphs ---------------------------------------------------------------------------------------------
def test_no_pair_at_all(split, whole):
    hand_built(split, whole, Builder().fillers(300, 2))


def test_only_isolated_pairs(split, whole):
    """the parent absorbs the child (5 : 1, 3 : 2), the child has at least double the parent's count (1 : 4, 1 : 1, 2 : 3),
    neither joins (2 : 2, 3 : 3, 5 : 4): no pair goes to the graph, which is only built when an accessor asks"""
    b = Builder()
    for cp, cc in ((5, 1), (1, 4), (2, 2), (1, 1), (3, 3), (3, 2), (2, 3), (5, 4), (1, 7), (7, 1)):
        b.fillers(3).pair(cp, cc)
    b.fillers(40)
    assert b.graph == 0
    hand_built(split, whole, b)


@pytest.mark.parametrize("shape", ["star", "triangle", "chain"])
def test_one_shape_among_isolated_pairs(split, whole, shape):
    """the degree-1 children of a star are ends of rest pairs: the star's two pairs are both in the graph"""
    b = Builder().fillers(5).pair(5, 1).fillers(2).pair(1, 3)
    getattr(b, shape)()
    b.fillers(4).pair(2, 2).fillers(7)
    assert b.direct > 0 and b.graph > 0
    hand_built(split, whole, b)


def test_every_pair_in_the_rest(split, whole):
    """40 pairs in the rest (more than SMALL_COMP: the cluster kernels fetch the node count) and 5 (fewer: it comes
    with the pass's last wait)"""
    b = Builder()
    for k in range(8):
        b.fillers(k % 3).star(5, 1 + k % 2, 2).chain()
    assert b.direct == 0 and b.graph == 40
    hand_built(split, whole, b)
    hand_built(split, whole, Builder().fillers(2).star().fillers(1).triangle(4, 4, 1))


def test_many_rest_pairs_among_isolated_ones(split, whole):
    """a parent with all twelve children (a component of 13 nodes, 12 + 4 * 3 pairs) twice, and a chain: more than
    SMALL_COMP rest pairs next to isolated pairs"""
    b = Builder().fillers(3).pair(4, 1)
    for _ in range(2):
        p = b._parent(20)
        kids = sorted(child(p, pos, v) for pos in range(4) for v in (1, 2, 3))
        for k, w in enumerate(kids):
            b._add(w, 1 + k % 3)
        b.graph += 12 + 4 * 3
        b.fillers(2).pair(1, 2)
    b.chain().fillers(9)
    hand_built(split, whole, b)


@pytest.mark.parametrize("shape", ["pair", "star"])
def test_bitmap_and_rank_edges(split, whole, shape):
    """ends on both sides of a bitmap word (31 | 32), of a rank block (255 | 256) and at the end of the walk
    (U - 2 | U - 1)"""
    b = Builder()
    for first in (31, 255, 600):
        b.fill_to(first)
        if shape == "pair":
            b.pair(3, 1)
        else:
            b.star()
    assert len(b.words) == (602 if shape == "pair" else 603)
    hand_built(split, whole, b)


def test_one_component_beyond_the_small_kernels(split, whole):
    """4^4 words that differ in four nucleotides only: one component of 256 nodes, every pair in the rest, clustered by
    the kernels for components of more than SMALL_COMP nodes (their size is fetched while the small ones run)"""
    w = dense_words(np.random.default_rng(3), 3000, 24, 4)
    for info in split_and_whole(split, whole, w, np.zeros(len(w), np.uint8)):
        assert info["pairs_direct"] == 0 and info["pairs_graph"] > 256


def test_the_lazy_full_build_does_not_leak(split, whole):
    """runs and their accessors one after the other on the same two contexts, in both methods: each run starts without
    a full graph, and is right although the context's graph arrays held the full graph of the run before -- against the
    oracle and against the context that never splits"""
    w1, f1 = Builder().fillers(40).pair(5, 1).star().fillers(3).pair(2, 2).reads()
    w2, f2 = Builder().fillers(7).triangle().pair(1, 1).fillers(90).chain().pair(1, 5).reads(1)
    w3, f3 = synth_words(3000, 11, 24, p_sub=0.02)
    for maximum in (False, True):
        for words, filt in ((w1, f1), (w2, f2), (w3, f3), (w1, f1)):
            split.run(words, filt, word_nt=24, distance=1, method=int(maximum))
            assert split.graph_split_info()["full_graph_built"] == 0
            split_and_whole(split, whole, words, filt, methods=(maximum,))
            assert split.graph_split_info()["full_graph_built"] == 1
            split.leaves()
            split.adjacency()                                              # (a second time: built once)
            assert split.graph_split_info()["full_graph_built"] == 1


def test_kernel_timing_without_a_rest_pair():
    """option kernel_timing: the cluster kernels' pair of events is recorded by a stage that builds no graph too (no
    pair at all, only isolated pairs) -- on a new context, whose events were never recorded, and behind a run with rest
    pairs, whose events must not be measured again"""
    none = Builder().fillers(300, 2).reads()
    isolated = Builder().fillers(9).pair(5, 1).fillers(3).pair(2, 2).fillers(20).pair(1, 4).reads()
    rest = synth_words(40_000, 6, 24, p_sub=8e-3, p_n=1e-3)
    for first in (none, isolated):
        dd = humid_amd.Dedup()
        try:
            dd.set_option("kernel_timing", 1)
            for words, filt in (first, rest, none, isolated):
                for maximum in (False, True):
                    s = check_against_oracle(dd, words, filt, 24, 1, maximum)          # (with the accessors' full build)
                    cid, keep, s = dd.run(words, filt, word_nt=24, distance=1, method=int(maximum))
                    assert 0.0 <= s["ms_k_cluster"] <= s["ms_total"], (s["ms_k_cluster"], s["ms_total"])
                    if words is not rest[0]:
                        assert dd.graph_split_info()["pairs_graph"] == 0
        finally:
            dd.close()


# ---- the other roads of the search ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def umi_words():
    return synth_words(40_000, 6, 24, p_sub=8e-3, p_n=1e-3)


def test_region_full_on_the_first_run(umi_words):
    """U = 16 290 and 5 743 pairs, more than the 4 096 the regions start with: the first run of a new context retries
    behind a full region (no graph was built for the attempt it throws away)"""
    words, filt = umi_words
    a, b = humid_amd.Dedup(), humid_amd.Dedup()
    try:
        b.set_option("pair_split", 0)
        roads = []
        infos = split_and_whole(a, b, words, filt, roads=roads)
        assert infos[0]["pairs_direct"] + infos[0]["pairs_graph"] == 5743
        assert infos[0]["pairs_direct"] > 0 and infos[0]["pairs_graph"] > 0
        for dd in ("split", "whole"):
            assert roads[0][dd]["events"].count("REGIONS_REGROWN") >= 1, roads[0]
            assert roads[0][dd]["graph_attempts"] == 1 + roads[0][dd]["n_events"]
            for later in roads[1:]:                         # (the context remembers the room)
                assert later[dd] == dict(events=[], n_events=0, graph_attempts=1), later
    finally:
        a.close()
        b.close()


def test_unfused_search_below_4096_words(split, whole, umi_words):
    words, filt = umi_words
    infos = split_and_whole(split, whole, words[:3000], filt[:3000])
    assert infos[0]["pairs_direct"] > 0


def test_tiles_make_a_far_list(split, whole, umi_words):
    """bucket_walk = 1: nearly every bucket of two words and more goes on in the tiles, whose pairs are marked by
    k_mark_pairs"""
    words, filt = umi_words
    roads = []
    infos = split_and_whole(split, whole, words, filt, options=[("bucket_walk", 1, 1024)], roads=roads)
    assert infos[0]["pairs_direct"] > 0 and infos[0]["pairs_graph"] > 0
    for r in roads:
        assert "FAR_TILES" in r["split"]["events"] and "FAR_TILES" in r["whole"]["events"], r


def test_padded_coarse_bin_full_on_the_first_run():
    """6 000 distinct 24-nt words at d = 1 whose last twelve nucleotides are all the same.  The plan has two
    combinations of one 12-nt segment each (4^12 >= 6 000 keys apiece); the second one's key is nucleotides 12 .. 23,
    24 bits, grouped into 2^9 coarse bins (group_words_by_stretch).  Every word has the same key, so all 6 000 land in ONE bin,
    whose padded room is 6000 / 512 + 6000 / 512 / 4 + 1024 = 11 + 2 + 1024 = 1 037 words: the bin is full, the first
    run of a new context throws its attempt away and makes every order again with exact bins (and that one bucket of
    6 000 words, longer than the walk of 1 024, goes on in the tiles).  The padding stays off for the context, hence two
    fresh ones.  The first twelve nucleotides are 6 000 of the 4^9 values of nine of them: about 0.6 neighbours a word,
    isolated pairs and rest pairs both."""
    rng = np.random.default_rng(512)
    hi = rng.choice(4 ** 9, size=6000, replace=False).astype(U64)
    u = (hi << U64(24)) | U64(0x5A3C96)
    words = np.repeat(u, rng.integers(1, 6, size=len(u)))
    words = np.ascontiguousarray(words[rng.permutation(len(words))])
    a, b = humid_amd.Dedup(), humid_amd.Dedup()
    try:
        b.set_option("pair_split", 0)
        roads = []
        infos = split_and_whole(a, b, words, np.zeros(len(words), np.uint8), roads=roads)
        assert infos[0]["pairs_direct"] > 0 and infos[0]["pairs_graph"] > 0
        for dd in ("split", "whole"):
            ev = roads[0][dd]["events"]
            assert "ORDERS_REDONE" in ev and "FAR_TILES" in ev[ev.index("ORDERS_REDONE"):], roads[0]
            for later in roads[1:]:                         # (the padding stays off: the tiles alone)
                assert later[dd] == dict(events=["FAR_TILES"], n_events=1, graph_attempts=2), later
    finally:
        a.close()
        b.close()


def test_six_combinations(split, whole):
    words, filt = synth_words(20_000, 6, 12, p_sub=8e-3, p_n=1e-3)
    """d = 2 over 12 nt: six combinations, five of them searched inside their grouping"""
    for info in split_and_whole(split, whole, words, filt, n=12, d=2):
        assert info["pairs_direct"] > 0 and info["pairs_graph"] > 0


def test_grouped_pass(split, whole):
    words, filt = synth_words(20_000, 6, 24, p_sub=8e-3, p_n=1e-3)
    w = np.concatenate([words, words])
    f = np.concatenate([filt, filt])
    g = np.repeat(np.arange(2, dtype=np.uint32), len(words))
    for method in (0, 1):
        truth = gt.per_group(w, g, f, 24, distance=1, method=method, first_read=False)
        for dd in (split, whole):
            gt.assert_same(truth, gt.device_result(dd, w, g, f, 24, n_groups=2, distance=1, method=method))
    info = split.graph_split_info()
    assert info["pairs_direct"] > 0 and info["pairs_direct"] + info["pairs_graph"] == truth["summary"]["edges"]


def test_given_pairs_of_the_edit_search(split, whole):
    """-e at d = 2: the pairs are given to the graph stage as a list (k_mark_pairs marks them)"""
    from test_gpu_edit import check_edit
    words, filt = synth_words(3000, 77, 24, p_sub=0.02)
    for maximum in (False, True):
        check_edit(split, words, filt, 24, 2, maximum)
        a = snapshot(split, words, filt, 24, 2, maximum, edit=True)
        check_edit(whole, words, filt, 24, 2, maximum)
        b = snapshot(whole, words, filt, 24, 2, maximum, edit=True)
        assert_same_arrays(a, b)
        assert a["info"]["pairs_direct"] > 0 and a["info"]["pairs_direct"] + a["info"]["pairs_graph"] == a["summary"]["edges"]
        assert a["info"]["full_graph_built"] == 0 and b["info"]["full_graph_built"] == 1


# ---- random differential at the metric's parameters -----------------------------------------------------------------
def probe_pairs(words, filt, n=24):
    """all pairs at Hamming distance 1 among the unique usable words (72 single-substitution probes by searchsorted):
    (pairs, those whose two ends have degree 1)"""
    u = np.unique(words[filt == 0])
    lo, hi = [], []
    for pos in range(n):
        sh = U64(2 * pos)
        for v in (1, 2, 3):
            q = u ^ (U64(v) << sh)
            at = np.searchsorted(u, q)
            at[at == len(u)] = 0
            hit = np.flatnonzero((u[at] == q) & (q > u))
            lo.append(hit)
            hi.append(at[hit])
    lo, hi = np.concatenate(lo), np.concatenate(hi)
    deg = np.bincount(lo, minlength=len(u)) + np.bincount(hi, minlength=len(u))
    return len(lo), int(np.count_nonzero((deg[lo] == 1) & (deg[hi] == 1)))


@pytest.mark.parametrize("seed", [1002, 1003, 1004])
def test_random_differential(split, whole, seed):
    words, filt = synth_words(200_000, seed, 24)
    pairs, isolated = probe_pairs(words, filt)
    assert 0.70 * pairs <= isolated <= 0.95 * pairs, (pairs, isolated)     # the shape the split is made for
    for info in split_and_whole(split, whole, words, filt):
        assert info["pairs_direct"] == isolated and info["pairs_graph"] == pairs - isolated
