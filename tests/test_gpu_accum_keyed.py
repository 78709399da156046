"""-m gpu: keyed accumulated runs (include/humid_hip.h, humid_accum_*_keyed): add every chunk with its keys, finish, map
every chunk.  The results must be those of the per-group oracle over all reads sorted by global index
(tests/accum_keyed_truth.py) and of Dedup.run_keyed on the concatenation, bit for bit, whatever the chunking, the order
of the chunks, the merge tile and the layout of an entry on the device."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from accum_keyed_truth import keyed_expected, keyed_leaves
from humid_amd.synth import synth_words
from whitelist_truth import make_keys, whitelist_with_neighbours

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP = 2 ** 64 - 1
FIELDS = ("total", "usable", "unique", "clusters", "edges", "nonsingle")
CUTS = (4000, 4000, 9000, 9500, 17000, 29999)      # 7 uneven chunks: the second empty, the fourth all filtered, the last one read
# (key_nt, word_nt): one-word entry; a short one; two-word entry, one-word internal word; any 64-bit key; two-word internal word
SHAPES = [(16, 12), (4, 8), (16, 24), (0, 12), (0, 32)]


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def barcodes(rng, key_nt, n=300):
    """n distinct keys (fewer where 4^key_nt is small); key_nt 0: any 64-bit value, the extremes and near-twins among them"""
    if key_nt == 0:
        x, y = (int(v) for v in rng.integers(1, 1 << 62, 2))
        special = [0, TOP, x, x | (1 << 63), y & ~1, y | 1]         # pairs that differ only in bit 63 / only in the low bit
        rest = rng.integers(0, 1 << 64, n - len(special), dtype=U64, endpoint=False).tolist()
        b = np.array(special + rest, U64)
    elif 4 ** key_nt <= 2 * n:
        b = rng.permutation(4 ** key_nt)[:4 ** key_nt * 3 // 4].astype(U64)
    else:
        b = rng.integers(0, 4 ** key_nt, n).astype(U64)
    b = np.unique(b)
    return b[rng.permutation(len(b))]


def skewed(rng, pool, n):
    """n draws from pool, entry r with weight 1 / (r + 1)"""
    p = 1.0 / np.arange(1, len(pool) + 1)
    return pool[rng.choice(len(pool), n, p=p / p.sum())]


def split(w, k, f, cuts, bases=None):
    """chunks [(words, keys, filtered, base)]; base = the running total unless given"""
    edges = [0] + list(cuts) + [len(f)]
    return [(w[a:b], k[a:b], f[a:b], a if bases is None else bases[j]) for j, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]


_inputs = {}


def case(shape, n_reads=30000):
    """the input of a shape, its 7 chunks (computed once, never changed)"""
    if (shape, n_reads) not in _inputs:
        key_nt, word_nt = shape
        w, f = synth_words(n_reads, 900 + 40 * key_nt + word_nt, word_nt, p_sub=0.01, p_n=0.01)
        rng = np.random.default_rng(7 + 100 * key_nt + word_nt)
        k = skewed(rng, barcodes(rng, key_nt), n_reads)
        f = f.copy()
        f[9000:9500] = 1
        k[f != 0] = rng.integers(1 << 63, 1 << 64, int((f != 0).sum()), dtype=U64, endpoint=False)   # garbage, beyond any key_nt: never read
        for a in (w, k, f):
            a.setflags(write=False)
        _inputs[(shape, n_reads)] = (w, k, f, split(w, k, f, CUTS))
    return _inputs[(shape, n_reads)]


_truth = {}


def truth(key, chunks, word_nt, d, method, edit=False):
    if key not in _truth:
        _truth[key] = keyed_expected(chunks, word_nt, d, method, edit)
    return _truth[key]


def accumulate(dd, shape, chunks, d=1, method=0, edit=False, order=None, tile=2048):
    """(accumulator, summary, [(cid, keep, n_unknown)] per chunk in the order of `chunks`)"""
    dd.set_option("accum_tile", tile)
    try:
        acc = dd.keyed_accumulator(word_nt=shape[1], key_nt=shape[0])
        for j in (order if order is not None else range(len(chunks))):
            acc.add(*chunks[j])
        assert acc.info()["n_keys"] == 0
        s = dict(acc.finish(d, method, edit))
        assert acc.info()["finished"]
        return acc, s, [acc.map(*c) for c in chunks]
    finally:
        dd.set_option("accum_tile", 2048)


def assert_results(res, exp, what=""):
    for j, ((cid, keep, unknown), (ecid, ekeep)) in enumerate(zip(res, exp)):
        assert unknown == 0, (what, j)
        assert np.array_equal(cid, ecid), (what, j)
        assert np.array_equal(keep, ekeep), (what, j)


def cat(res, j):
    return np.concatenate([r[j] for r in res])


def assert_list(acc, chunks):
    got, exp = acc.leaves(), keyed_leaves(chunks)
    assert got["first"].dtype == U64 and got["count"].dtype == np.uint32
    for f in ("key", "word", "first"):
        assert np.array_equal(got[f], exp[f]), f
    assert np.array_equal(got["count"], exp["count"].astype(np.uint32))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("method", [humid_amd.DIRECTIONAL, humid_amd.MAXIMUM])
def test_chunked_equals_truth_and_one_shot(dd, shape, d, method):
    w, k, f, chunks = case(shape)
    exp, esum, t = truth((shape, d, method), chunks, shape[1], d, method)
    acc, s, res = accumulate(dd, shape, chunks, d, method)
    assert_results(res, exp)
    assert {x: s[x] for x in FIELDS[:5]} == esum
    i = acc.info()
    assert i["n_keys"] == len(t["keys"]) and i["key_nt"] == shape[0] and i["word_nt"] == shape[1]
    assert i["entry_words"] == (1 if shape[0] and sum(shape) <= 32 else 2)
    assert i["total"] == len(f) and i["usable"] == esum["usable"] and i["unique"] == esum["unique"] and i["chunks"] == 7
    cid, keep, rs = dd.run_keyed(w, k, f, shape[1], d, method)
    assert np.array_equal(cat(res, 0), cid) and np.array_equal(cat(res, 1), keep)
    assert {x: s[x] for x in FIELDS} == {x: rs[x] for x in FIELDS}


@pytest.mark.parametrize("shape", SHAPES)
def test_the_list(dd, shape):
    w, k, f, chunks = case(shape)
    acc = dd.keyed_accumulator(word_nt=shape[1], key_nt=shape[0])
    for j in (5, 2, 0, 6, 1, 4, 3):
        acc.add(*chunks[j])
    assert_list(acc, chunks)
    acc.finish(1, 0)
    assert_list(acc, chunks)                                        # (finish leaves the list as it was)


@pytest.mark.parametrize("shape", [(16, 12), (0, 12), (0, 32)])
def test_order_of_the_chunks_gaps_and_the_tile_do_not_matter(dd, shape):
    w, k, f, chunks = case(shape)
    exp, esum, _ = truth((shape, 1, 0), chunks, shape[1], 1, 0)
    _, s_perm, res = accumulate(dd, shape, chunks, order=[5, 2, 0, 6, 1, 4, 3])
    assert_results(res, exp, "permuted")
    _, s_64, res = accumulate(dd, shape, chunks, tile=64)
    assert_results(res, exp, "tile 64")
    _, s_2048, res = accumulate(dd, shape, chunks[::-1], tile=2048)
    assert_results(res, exp[::-1], "reversed")
    for s in (s_perm, s_64, s_2048):
        assert {x: s[x] for x in FIELDS[:5]} == esum
    # bases that leave gaps and do not follow the order of the chunks: the first chunk given is the LAST in global order
    bases = [2 ** 40, 2 ** 33 + 10 ** 5, 2 ** 33, 5, 2 ** 20, 2 ** 34, 0]
    gapped = split(w, k, f, CUTS, bases)
    gexp, gsum, _ = keyed_expected(gapped, shape[1], 1, 0)
    acc, s, res = accumulate(dd, shape, gapped)
    assert_results(res, gexp, "gaps")
    assert {x: s[x] for x in FIELDS[:5]} == gsum
    assert_list(acc, gapped)
    assert not np.array_equal(cat(res, 1), cat([e + (0,) for e in exp], 1))     # (other reads are the global firsts now)


def test_edit_distance(dd):
    shape = (16, 12)
    w, k, f, _ = case(shape)
    w, k, f = w[:3000], k[:3000], f[:3000]
    chunks = split(w, k, f, (100, 100, 1500, 2999))
    exp, esum, _ = keyed_expected(chunks, 12, 2, 0, edit=True)
    try:
        acc, s, res = accumulate(dd, shape, chunks, 2, 0, edit=True)
        assert_results(res, exp)
        assert {x: s[x] for x in FIELDS[:5]} == esum
        cid, keep, rs = dd.run_keyed(w, k, f, 12, 2, 0, edit=True)
        assert np.array_equal(cat(res, 0), cid) and np.array_equal(cat(res, 1), keep)
        assert {x: s[x] for x in FIELDS} == {x: rs[x] for x in FIELDS}
    finally:
        dd.set_option("edit_distance", 0)


def leaf_view(dd, u):
    """the leaves through the C calls a finish answers: words, cluster ids, is-max, groups (no first_read)"""
    word, cid, ismax, group = np.zeros(u, U64), np.zeros(u, np.uint32), np.zeros(u, np.uint8), np.zeros(u, np.uint32)
    dd._check(dd._lib.humid_get_leaves(dd._h, word.ctypes.data, None, None, None, cid.ctypes.data, ismax.ctypes.data))
    dd._check(dd._lib.humid_get_leaf_groups(dd._h, group.ctypes.data))
    return dict(word=word, cluster_id=cid, is_max_leaf=ismax, group=group)


@pytest.mark.parametrize("shape", [(16, 12), (16, 24), (0, 32)])
def test_accessors_after_finish(dd, shape):
    w, k, f, chunks = case(shape)
    _, _, rs = dd.run_keyed(w, k, f, shape[1], 1, 0)
    u = rs["unique"]
    ref = dict(keys=dd.group_keys(), gs=dd.group_stats(), adj=dd.adjacency(), cl=dd.clusters(),
               h=[dd.histogram(j) for j in range(3)], lv=leaf_view(dd, u))
    acc = dd.keyed_accumulator(word_nt=shape[1], key_nt=shape[0])
    for c in chunks:
        acc.add(*c)
    acc.finish(1, 0)
    assert np.array_equal(dd.group_keys(), ref["keys"]) and acc.info()["n_keys"] == len(ref["keys"])
    gs = dd.group_stats()
    assert sorted(gs) == sorted(ref["gs"]) and "key" in gs
    for x in gs:
        assert np.array_equal(gs[x], ref["gs"][x]), x
    dev = dd.group_stats_device()
    assert dev["n"] == len(ref["keys"]) and dev["reads"] and dev["edges"]
    off, idx = dd.adjacency()
    assert np.array_equal(off, ref["adj"][0]) and np.array_equal(idx, ref["adj"][1])
    cl = dd.clusters()
    for x in ("size", "max_count", "max_leaf"):
        assert np.array_equal(cl[x], ref["cl"][x]), x
    assert [dd.histogram(j) for j in range(3)] == ref["h"]
    lv = leaf_view(dd, u)
    for x in lv:
        assert np.array_equal(lv[x], ref["lv"][x]), x
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.leaves()                                               # first_read needs a complete run
    assert ei.value.code == -6
    acc.map(*chunks[0])                                           # the first map ends the record finish published
    group = np.zeros(u, np.uint32)
    for call in (dd.group_keys, dd.group_stats, dd.group_stats_device, dd.adjacency,
                 lambda: dd._check(dd._lib.humid_get_leaf_groups(dd._h, group.ctypes.data))):
        with pytest.raises(humid_amd.HumidError) as ei:
            call()
        assert ei.value.code == -6


def test_a_plain_finish_still_has_no_groups(dd):
    w, k, f, chunks = case((16, 12))
    acc = dd.accumulator(12)
    acc.add(w[:5000], f[:5000])
    acc.finish(1, 0)
    group = np.zeros(5000, np.uint32)
    for call in (dd.group_keys, dd.group_stats, lambda: dd._check(dd._lib.humid_get_leaf_groups(dd._h, group.ctypes.data))):
        with pytest.raises(humid_amd.HumidError) as ei:
            call()
        assert ei.value.code == -6


# ---- the ranking of the keys at finish ---------------------------------------------------------------------------
def hand_list(key_of_entry, keys, rng, word_nt=12):
    """two chunks whose list is entry i = (keys[key_of_entry[i]], word i): entry i is read i % 3 + 1 times, the reads
    shuffled and dealt to the chunks; one more key sits on filtered reads only"""
    u = len(key_of_entry)
    e = np.repeat(np.arange(u), np.arange(u) % 3 + 1)
    e = e[rng.permutation(len(e))]
    w, k, f = e.astype(U64), keys[np.asarray(key_of_entry)[e]], np.zeros(len(e), np.uint8)
    ghost = U64(int(keys.max()) - 1 if int(keys.max()) - 1 not in set(keys.tolist()) else int(keys.max()) + 1)
    at = rng.choice(len(e), 20, replace=False)
    w, k, f = np.insert(w, at, 3), np.insert(k, at, ghost), np.insert(f, at, 1)
    cut = len(f) // 3
    return w, k, f, ghost, split(w, k, f, (cut,), [10 ** 6, 0])


def check_hand_list(dd, shape, key_of_entry, keys, seed):
    rng = np.random.default_rng(seed)
    w, k, f, ghost, chunks = hand_list(key_of_entry, keys, rng, shape[1])
    g = len(np.unique(key_of_entry))
    exp, esum, t = keyed_expected(chunks, shape[1], 1, 0)
    assert len(t["keys"]) == g and esum["unique"] == len(key_of_entry)
    acc = dd.keyed_accumulator(word_nt=shape[1], key_nt=shape[0])
    for c in chunks:
        acc.add(*c)
    s = dict(acc.finish(1, 0))
    assert acc.info()["n_keys"] == g and acc.info()["unique"] == len(key_of_entry)
    got = dd.group_keys()
    assert np.array_equal(got, t["keys"]) and int(ghost) not in set(got.tolist())
    group = np.zeros(len(key_of_entry), np.uint32)
    dd._check(dd._lib.humid_get_leaf_groups(dd._h, group.ctypes.data))
    assert np.array_equal(group, t["leaves"]["group"])
    assert np.array_equal(dd.group_stats()["unique"], np.bincount(key_of_entry, minlength=g))
    assert_results([acc.map(*c) for c in chunks], exp)
    assert {x: s[x] for x in FIELDS[:5]} == esum
    cid, keep, rs = dd.run_keyed(w, k, f, shape[1], 1, 0)
    assert np.array_equal(np.concatenate([e[0] for e in exp]), cid)     # (ids do not depend on the order of the reads; keep does)
    assert {x: s[x] for x in FIELDS} == {x: rs[x] for x in FIELDS}


def keys_for(shape, g, rng):
    if shape[0] == 0:
        k = np.unique(np.concatenate([rng.integers(0, 1 << 64, g, dtype=U64, endpoint=False), np.array([0, TOP], U64)]))
    else:
        k = np.unique(rng.integers(2, 4 ** shape[0] - 2, 2 * g + 8).astype(U64))
    assert len(k) >= g
    return np.sort(k[rng.permutation(len(k))[:g]])


U_HAND = 2000


@pytest.mark.parametrize("shape", [(16, 12), (0, 12)])
@pytest.mark.parametrize("g", [1, 2, 4, 5, 16, 17, 64, 65, 256, 257, 1024, 1025, U_HAND])
def test_ranking_on_both_sides_of_every_group_field(dd, shape, g):
    """G distinct keys over 2000 entries, G on both sides of every value where the group field grows a nucleotide
    (1 | 2, 4 | 5, 16 | 17, 64 | 65, 256 | 257, 1024 | 1025) and G = U"""
    rng = np.random.default_rng(1000 * g + shape[0])
    key_of_entry = np.arange(U_HAND) * g // U_HAND
    check_hand_list(dd, shape, key_of_entry, keys_for(shape, g, rng), g)


@pytest.mark.parametrize("shape", [(16, 12), (0, 12)])
@pytest.mark.parametrize("shift", [-1, 0, 1, 100])
def test_runs_of_equal_keys_against_the_256_entry_boundaries(dd, shape, shift):
    """runs of 256 entries that end one entry before, at and one entry behind every multiple of 256, and (100) runs laid
    across every one"""
    rng = np.random.default_rng(77 + shift)
    key_of_entry = (np.arange(U_HAND) + 256 + shift) // 256
    key_of_entry -= key_of_entry.min()
    g = int(key_of_entry.max()) + 1
    check_hand_list(dd, shape, key_of_entry, keys_for(shape, g, rng), 5 + shift)


# ---- the merge over entries ----------------------------------------------------------------------------------------
def entry_reads(entries, seed):
    """a chunk holding entry (key, word) (word % 3) + 1 times, shuffled, with one filtered read in front"""
    rep = [e for e in entries for _ in range(e[1] % 3 + 1)]
    np.random.default_rng(seed + len(rep)).shuffle(rep)
    k = np.array([TOP] + [e[0] for e in rep], U64)
    w = np.array([0] + [e[1] for e in rep], U64)
    f = np.zeros(len(rep) + 1, np.uint8)
    f[0] = 1
    return w, k, f


@pytest.mark.parametrize("shape", [(16, 12), (0, 12)])
@pytest.mark.parametrize("background", ["same_word_other_key", "same_key_other_word"])
def test_merge_pairs_slide_over_a_tile_boundary(dd, shape, background):
    """200 merge positions that alternate a, b, a, b ... with tiles of 64.  Every neighbouring (a, b) has an equal word
    under different keys (these must NOT combine) or an equal key with different words, at every position and so across
    every tile boundary; ONE entry is in both lists, key and word equal, its a at position p and its b at p + 1 for
    every p in 60 .. 70: before the boundary, across it and behind it."""
    big = TOP - 1000 if shape[0] == 0 else 4 ** shape[0] - 1000

    def entry(v):
        return (big + v, 5) if background == "same_word_other_key" else (big, 3 * v)

    dd.set_option("accum_tile", 64)
    try:
        for p in [None] + list(range(60, 71)):
            val = [2 * q for q in range(200)]
            src = ["a" if q % 2 == 0 else "b" for q in range(200)]
            if p is not None:
                val[p + 1] = val[p]
                src[p], src[p + 1] = "a", "b"
            a = [entry(v) for v, s in zip(val, src) if s == "a"]
            b = [entry(v) for v, s in zip(val, src) if s == "b"]
            assert len(set(a) & set(b)) == (0 if p is None else 1)
            ca, cb = entry_reads(a, 1), entry_reads(b, 2)
            chunks = [ca + (2 ** 35,), cb + (7,)]
            acc = dd.keyed_accumulator(word_nt=shape[1], key_nt=shape[0])
            for j, c in enumerate(chunks):
                acc.add(*c)
                assert_list(acc, chunks[:j + 1])
            assert acc.info()["unique"] == (200 if p is None else 199)
    finally:
        dd.set_option("accum_tile", 2048)


# ---- unknown and invalid reads -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 12), (0, 12)])
def test_map_of_a_chunk_that_was_never_added(dd, shape):
    w, k, f, _ = case(shape)
    w, k, f = w[:6000], k[:6000], f[:6000]
    added = (w[:4000], k[:4000], f[:4000], 0)
    ow, ok, of = w[4000:].copy(), k[4000:].copy(), f[4000:].copy()
    seen = set(int(x) for x in added[1][added[2] == 0])
    fresh = U64(next(x for x in range(5, 10 ** 6) if x not in seen))
    ow[:200], ok[:200] = added[0][:200], fresh                    # known words under a key never seen
    acc = dd.keyed_accumulator(word_nt=shape[1], key_nt=shape[0])
    acc.add(*added)
    acc.finish(1, 0)
    exp = keyed_expected([added], shape[1], 1, 0)[0][0]
    known = {}
    for word, key, fl, c in zip(added[0].tolist(), added[1].tolist(), added[2].tolist(), exp[0].tolist()):
        if not fl:
            known[(key, word)] = c
    rows = list(zip(ok.tolist(), ow.tolist(), of.tolist()))
    want = np.array([0 if fl else known.get((key, word), 0) for key, word, fl in rows], np.uint32)
    n_unknown = sum(1 for key, word, fl in rows if not fl and (key, word) not in known)
    assert int((of[:200] == 0).sum()) <= n_unknown < int((of == 0).sum())          # (the case holds both kinds)
    cid, keep, unknown = acc.map(ow, ok, of, 10 ** 12)
    assert np.array_equal(cid, want) and unknown == n_unknown
    assert not cid[:200].any() and not keep.any()                 # no read of it is a global first
    cid3, keep3, u3 = acc.map(*added)
    assert np.array_equal(cid3, exp[0]) and np.array_equal(keep3, exp[1]) and u3 == 0


@pytest.mark.parametrize("shape", [(16, 12), (4, 8), (16, 24)])
def test_a_key_beyond_key_nt_is_refused_and_changes_nothing(dd, shape):
    w, k, f, chunks = case(shape)
    acc = dd.keyed_accumulator(word_nt=shape[1], key_nt=shape[0])
    for c in chunks[:3]:
        acc.add(*c)
    held, info = acc.leaves(), acc.info()

    def unchanged():
        now = acc.leaves()
        return all(np.array_equal(now[x], held[x]) for x in held) and acc.info() == info

    bw, bk, bf, base = chunks[4]
    bad = bk.copy()
    at = int(np.flatnonzero(bf == 0)[17])
    bad[at] = U64(4 ** shape[0])                                   # the smallest key that does not fit
    with pytest.raises(humid_amd.HumidError) as ei:
        acc.add(bw, bad, bf, base)
    assert ei.value.code == -1 and unchanged()
    bad[at] = U64(TOP)
    with pytest.raises(humid_amd.HumidError) as ei:
        acc.add(bw, bad, bf, base)
    assert ei.value.code == -1 and unchanged()
    for c in chunks[3:]:
        acc.add(*c)
    acc.finish(1, 0)
    info = acc.info()
    held = acc.leaves()
    with pytest.raises(humid_amd.HumidError) as ei:
        acc.map(bw, bad, bf, base)
    assert ei.value.code == -1 and unchanged()
    exp, esum, _ = truth((shape, 1, 0), chunks, shape[1], 1, 0)
    assert_results([acc.map(*c) for c in chunks], exp)            # still finished, and right


def test_state_and_argument_errors():
    d = humid_amd.Dedup()
    lib, h = d._lib, d._h
    w, k, f, _ = case((16, 12))
    w, k, f = np.ascontiguousarray(w[:2000]), np.ascontiguousarray(k[:2000]), np.ascontiguousarray(f[:2000])
    cid, keep = np.zeros(2000, np.uint32), np.zeros(2000, np.uint8)
    v, a, b = C.c_uint64(), C.c_uint32(), C.c_uint32()
    P = lambda x: x.ctypes.data                                     # noqa: E731
    keyed_calls = [
        lambda: lib.humid_accum_add_keyed(h, P(w), P(k), P(f), 2000, 0),
        lambda: lib.humid_accum_map_keyed(h, P(w), P(k), P(f), 2000, 0, P(cid), P(keep), None),
        lambda: lib.humid_accum_get_leaves_keyed(h, None, None, None, None, 0, C.byref(v)),
        lambda: lib.humid_accum_keyed_info(h, C.byref(a), C.byref(b), C.byref(v)),
    ]
    plain_calls = [
        lambda: lib.humid_accum_add(h, P(w), P(f), 2000, 0),
        lambda: lib.humid_accum_map(h, P(w), P(f), 2000, 0, P(cid), P(keep), None),
        lambda: lib.humid_accum_get_leaves(h, None, None, None, 0, C.byref(v)),
    ]
    for call in keyed_calls:
        assert call() == -6                                       # before any begin
    assert lib.humid_accum_begin_keyed(h, 33, 16) == -2 and lib.humid_accum_begin_keyed(h, 0, 16) == -1
    assert lib.humid_accum_begin_keyed(h, 12, 33) == -1
    for call in keyed_calls:
        assert call() == -6                                       # a refused begin begins nothing
    plain = d.accumulator(12)
    plain.add(w, f)
    for call in keyed_calls:
        assert call() == -6                                       # keyed calls on a plain accumulator
    assert plain.info()["chunks"] == 1
    acc = d.keyed_accumulator(12, 16)                             # empties the plain one
    assert acc.info()["chunks"] == 0 and acc.info()["unique"] == 0 and len(acc.leaves()["key"]) == 0
    acc.add(w, k, f)
    for call in plain_calls:
        assert call() == -6                                       # plain calls on a keyed accumulator
    assert acc.info()["chunks"] == 1
    with pytest.raises(humid_amd.HumidError) as ei:
        acc.map(w, k, f, 0)                                       # map before finish
    assert ei.value.code == -6
    assert lib.humid_accum_add_keyed(h, P(w), None, P(f), 5, 0) == -1
    assert lib.humid_accum_add_keyed(h, P(w), P(k), P(f), 2 ** 31, 0) == -5
    with pytest.raises(ValueError):
        acc.add(w[:10], k[:9], f[:10])
    s = acc.finish(1, 0)
    ref = d.run_keyed(w, k, f, 12, 1, 0)
    got = acc.map(w, k, f, 0)                                     # (an unrelated run between finish and map)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and got[2] == 0
    assert {x: s[x] for x in FIELDS} == {x: ref[2][x] for x in FIELDS}
    again = d.accumulator(12)                                     # and a plain begin empties the keyed one
    assert again.info()["chunks"] == 0
    for call in keyed_calls:
        assert call() == -6
    again.clear()
    d.close()


def test_an_empty_and_an_all_filtered_accumulator(dd):
    acc = dd.keyed_accumulator(12, 16)
    s = acc.finish(1, 0)
    assert s["unique"] == 0 and s["clusters"] == 0 and acc.info()["n_keys"] == 0 and len(dd.group_keys()) == 0
    w, k, f = np.arange(50, dtype=U64), np.full(50, TOP, U64), np.ones(50, np.uint8)
    acc.add(w, k, f)
    s = acc.finish(1, 0)
    assert s["total"] == 50 and s["usable"] == 0 and len(dd.group_keys()) == 0
    cid, keep, unknown = acc.map(w, k, f, 0)
    assert not cid.any() and not keep.any() and unknown == 0


# ---- composition with the whitelist --------------------------------------------------------------------------------
def test_corrected_chunk_by_chunk_equals_the_corrected_run():
    d = humid_amd.Dedup()
    rng = np.random.default_rng(2024)
    n = 8000
    wl = whitelist_with_neighbours(rng, 300, 16)
    k, kf = make_keys(rng, wl, 16, n)
    w, wf = synth_words(n, 61, 12, p_sub=0.01, p_n=0.01)
    f = (wf | kf).astype(np.uint8)
    d.set_whitelist(wl, 16)
    acc = d.keyed_accumulator(12, 16)
    corrected = []
    for cw, ck, cf, base in split(w, k, f, (1000, 1000, 4500, 7999)):
        ko, st, _ = d.correct_keys(ck, cf)
        corrected.append((cw, ko, (cf | (st >= humid_amd.BC_AMBIGUOUS)).astype(np.uint8), base))
        acc.add(*corrected[-1])
    s = acc.finish(1, 0)
    keys = d.group_keys()
    res = [acc.map(*c) for c in corrected]
    cid, keep, rs = d.run_keyed(w, k, f, 12, 1, 0, correct=True)
    assert rs["usable"] < int((f == 0).sum())                     # (the correction dropped reads)
    assert np.array_equal(cat(res, 0), cid) and np.array_equal(cat(res, 1), keep) and not any(r[2] for r in res)
    assert {x: s[x] for x in FIELDS} == {x: rs[x] for x in FIELDS}
    assert np.array_equal(keys, d.group_keys()) and set(keys.tolist()) <= set(wl.tolist())
    d.close()
