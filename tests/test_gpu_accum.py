"""-m gpu: whole accumulated runs (include/humid_hip.h, humid_accum_*): add every chunk, finish, map every chunk.
The results must be those of the oracle over all reads sorted by global index (tests/accum_truth.py) and of Dedup.run
on the concatenation, whatever the chunking, the order of the chunks and the merge tile."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from accum_truth import accum_expected, accum_leaves
from humid_amd.synth import synth_wide_words, synth_words

pytestmark = pytest.mark.gpu

FIELDS = ("total", "usable", "unique", "clusters", "edges", "nonsingle")
CUTS = (4000, 4000, 9000, 9500, 17000, 29999)      # 7 uneven chunks: the second empty, the fourth all filtered, the last one read


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def synth(n_reads, seed, n, p_sub=0.01, p_n=0.01):
    return (synth_wide_words if n > 32 else synth_words)(n_reads, seed, n, p_sub=p_sub, p_n=p_n)


def split(w, f, cuts, bases=None):
    """chunks [(words, filtered, base)]; base = the running total unless given"""
    edges = [0] + list(cuts) + [len(f)]
    return [(w[a:b], f[a:b], a if bases is None else bases[k]) for k, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]


_inputs = {}


def case(n, n_reads=30000):
    """the input of word length n, its 7 chunks and the one-shot results (computed once, never changed)"""
    if (n, n_reads) not in _inputs:
        w, f = synth(n_reads, 500 + n, n)
        f = f.copy()
        f[9000:9500] = 1
        w.setflags(write=False)
        f.setflags(write=False)
        _inputs[(n, n_reads)] = (w, f, split(w, f, CUTS))
    return _inputs[(n, n_reads)]


_truth = {}


def truth(key, chunks, n, d, method, edit=False):
    if key not in _truth:
        _truth[key] = accum_expected(chunks, n, d, method, edit)[:2]
    return _truth[key]


def accumulate(dd, n, chunks, d=1, method=0, edit=False, order=None, tile=2048):
    """(accumulator, summary, [(cid, keep, n_unknown)] per chunk in the order of `chunks`)"""
    dd.set_option("accum_tile", tile)
    try:
        acc = dd.accumulator(n)
        for k in (order if order is not None else range(len(chunks))):
            acc.add(*chunks[k])
        s = dict(acc.finish(d, method, edit))
        assert acc.info()["finished"]
        return acc, s, [acc.map(*c) for c in chunks]
    finally:
        dd.set_option("accum_tile", 2048)


def assert_results(res, exp, what=""):
    for k, ((cid, keep, unknown), (ecid, ekeep)) in enumerate(zip(res, exp)):
        assert unknown == 0, (what, k)
        assert np.array_equal(cid, ecid), (what, k)
        assert np.array_equal(keep, ekeep), (what, k)


def cat(res, j):
    return np.concatenate([r[j] for r in res])


@pytest.mark.parametrize("n", [24, 48, 64])
@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("method", [humid_amd.DIRECTIONAL, humid_amd.MAXIMUM])
def test_chunked_equals_oracle_and_one_shot(dd, n, d, method):
    w, f, chunks = case(n)
    exp, esum = truth((n, d, method), chunks, n, d, method)
    acc, s, res = accumulate(dd, n, chunks, d, method)
    assert_results(res, exp)
    assert {k: s[k] for k in FIELDS[:5]} == esum
    cid, keep, rs = dd.run(w, f, n, d, method)
    assert np.array_equal(cat(res, 0), cid) and np.array_equal(cat(res, 1), keep)
    assert {k: s[k] for k in FIELDS} == {k: rs[k] for k in FIELDS}


def test_edit_distance(dd):
    w, f = synth(3000, 77, 24, p_sub=0.02)
    chunks = split(w, f, (100, 100, 1500, 2999))
    exp, esum = accum_expected(chunks, 24, 2, 0, edit=True)[:2]
    acc, s, res = accumulate(dd, 24, chunks, 2, 0, edit=True)
    assert_results(res, exp)
    assert {k: s[k] for k in FIELDS[:5]} == esum
    cid, keep, rs = dd.run(w, f, 24, 2, 0, edit=True)
    assert np.array_equal(cat(res, 0), cid) and np.array_equal(cat(res, 1), keep)
    assert {k: s[k] for k in FIELDS} == {k: rs[k] for k in FIELDS}
    dd.set_option("edit_distance", 0)


@pytest.mark.parametrize("n", [24, 48])
def test_order_of_the_chunks_one_chunk_and_the_tile_do_not_matter(dd, n):
    w, f, chunks = case(n)
    exp, esum = truth((n, 1, 0), chunks, n, 1, 0)
    _, s_rev, res = accumulate(dd, n, chunks, order=list(range(len(chunks)))[::-1])
    assert_results(res, exp, "reverse")
    _, s_64, res = accumulate(dd, n, chunks, tile=64)
    assert_results(res, exp, "tile 64")
    _, s_one, res = accumulate(dd, n, [(w, f, 0)])
    assert np.array_equal(res[0][0], np.concatenate([e[0] for e in exp]))
    assert np.array_equal(res[0][1], np.concatenate([e[1] for e in exp]))
    for s in (s_rev, s_64, s_one):
        assert {k: s[k] for k in FIELDS[:5]} == esum


@pytest.mark.parametrize("n", [24, 40])
def test_chunks_of_one_read(dd, n):
    w, f = synth(300, 9, n, p_sub=0.03, p_n=0.03)
    chunks = split(w, f, range(1, 300))
    exp, esum = accum_expected(chunks, n, 1, 0)[:2]
    acc, s, res = accumulate(dd, n, chunks)
    assert_results(res, exp)
    assert {k: s[k] for k in FIELDS[:5]} == esum and acc.info()["chunks"] == 300


@pytest.mark.parametrize("n", [24, 48])
def test_non_contiguous_bases(dd, n):
    w, f = synth(5000, 31, n, p_sub=0.02)
    bases = [2 ** 40, 2 ** 33 + 10 ** 5, 2 ** 33, 5, 2 ** 20]       # the first chunk given is the LAST in global order
    chunks = split(w, f, (1000, 1001, 2500, 4000), bases)
    exp, esum = accum_expected(chunks, n, 1, 0)[:2]
    acc, s, res = accumulate(dd, n, chunks)
    assert_results(res, exp)
    assert {k: s[k] for k in FIELDS[:5]} == esum
    lv, elv = acc.leaves(), accum_leaves(chunks, n)
    assert np.array_equal(lv["word"], elv["word"]) and np.array_equal(lv["first"], elv["first"])
    # the kept reads are not those of the concatenation: the chunk at base 5 holds the global firsts of its words
    assert not np.array_equal(cat(res, 1), dd.run(w, f, n, 1, 0)[1])


def test_reopen_add_after_finish(dd):
    w, f, chunks = case(24)
    first, rest = chunks[:3], chunks[3:]
    acc = dd.accumulator(24)
    for c in first:
        acc.add(*c)
    acc.finish(1, 0)
    exp_small = accum_expected(first, 24, 1, 0)[0]
    assert_results([acc.map(*c) for c in first], exp_small)
    acc.add(*rest[0])
    assert not acc.info()["finished"]
    with pytest.raises(humid_amd.HumidError) as ei:
        acc.map(*first[0])
    assert ei.value.code == -6
    for c in rest[1:]:
        acc.add(*c)
    s = acc.finish(1, 0)
    exp, esum = truth((24, 1, 0), chunks, 24, 1, 0)
    assert_results([acc.map(*c) for c in chunks], exp)
    assert {k: s[k] for k in FIELDS[:5]} == esum


@pytest.mark.parametrize("n", [24, 48])
def test_map_of_a_chunk_that_was_never_added(dd, n):
    w, f = synth(6000, 41, n, p_sub=0.02)
    added, other = split(w, f, (4000,))
    other = (other[0], other[1], 10 ** 12)
    acc = dd.accumulator(n)
    acc.add(*added)
    acc.finish(1, 0)
    exp = accum_expected([added], n, 1, 0)[0][0]
    cid, keep, unknown = acc.map(*other)
    # what the words of the added chunk were given: word -> cluster id
    key = (lambda x: tuple(int(v) for v in x)) if n > 32 else int
    known = {}
    for word, fl, c in zip(added[0].tolist(), added[1].tolist(), exp[0].tolist()):
        if not fl:
            known[key(word)] = c
    want = np.array([0 if fl else known.get(key(word), 0) for word, fl in zip(other[0].tolist(), other[1].tolist())], np.uint32)
    n_unknown = sum(1 for word, fl in zip(other[0].tolist(), other[1].tolist()) if not fl and key(word) not in known)
    assert 0 < n_unknown < int((other[1] == 0).sum())            # (the case holds both kinds)
    assert np.array_equal(cid, want) and unknown == n_unknown
    assert not keep.any()                                         # no read of it is a global first: every known word came earlier
    # the added chunk again, from a base BELOW the one it was added with: same ids, and still no global first
    cid2, keep2, unknown2 = acc.map(added[0], added[1], 10 ** 6)
    assert np.array_equal(cid2, exp[0]) and unknown2 == 0 and not keep2.any()
    cid3, keep3, _ = acc.map(*added)
    assert np.array_equal(cid3, exp[0]) and np.array_equal(keep3, exp[1])


@pytest.mark.parametrize("n", [24, 48])
def test_accessors_after_finish(dd, n):
    w, f, chunks = case(n)
    dd.run(w, f, n, 1, 0)
    ref = dict(adj=dd.adjacency(), cl=dd.clusters(), h=[dd.histogram(k) for k in range(3)], lv=dd.leaves())
    acc = dd.accumulator(n)
    for c in chunks:
        acc.add(*c)
    acc.finish(1, 0)
    off, idx = dd.adjacency()
    assert np.array_equal(off, ref["adj"][0]) and np.array_equal(idx, ref["adj"][1])
    cl = dd.clusters()
    for k in ("size", "max_count", "max_leaf"):
        assert np.array_equal(cl[k], ref["cl"][k]), k
    assert [dd.histogram(k) for k in range(3)] == ref["h"]
    u = len(ref["lv"]["count"])
    word = np.zeros((u, 2) if n > 32 else u, np.uint64)
    cid, ismax = np.zeros(u, np.uint32), np.zeros(u, np.uint8)
    dd._check(dd._lib.humid_get_leaves(dd._h, word.ctypes.data, None, None, None, cid.ctypes.data, ismax.ctypes.data))
    assert np.array_equal(word, ref["lv"]["word"]) and np.array_equal(cid, ref["lv"]["cluster_id"])
    assert np.array_equal(ismax, ref["lv"]["is_max_leaf"])
    for call in (dd.group_stats, dd.leaves):                      # what needs a complete single-GPU run (leaves(): first_read)
        with pytest.raises(humid_amd.HumidError) as ei:
            call()
        assert ei.value.code == -6
    acc.map(*chunks[0])                                           # the first map ends the record finish published
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.adjacency()
    assert ei.value.code == -6


def test_state_and_argument_errors():
    d = humid_amd.Dedup()
    lib, h = d._lib, d._h
    w, f = synth(2000, 3, 24)
    cid, keep = np.zeros(2000, np.uint32), np.zeros(2000, np.uint8)
    s = humid_amd._lib.HumidSummary()
    nt, fin, v = C.c_uint32(), C.c_uint32(), C.c_uint64()
    before_begin = [
        lambda: lib.humid_accum_add(h, w.ctypes.data, f.ctypes.data, 2000, 0),
        lambda: lib.humid_accum_map(h, w.ctypes.data, f.ctypes.data, 2000, 0, cid.ctypes.data, keep.ctypes.data, None),
        lambda: lib.humid_accum_finish(h, 1, 0, C.byref(s)),
        lambda: lib.humid_accum_get_leaves(h, None, None, None, 0, C.byref(v)),
        lambda: lib.humid_accum_info(h, C.byref(nt), None, None, None, None, C.byref(fin)),
    ]
    for call in before_begin:
        assert call() == -6
    assert lib.humid_accum_begin(h, 0) == -1 and lib.humid_accum_begin(h, 65) == -2
    for call in before_begin:
        assert call() == -6                                       # a refused begin begins nothing
    ref = d.run(w, f, 24, 1, 0)
    acc = d.accumulator(24)
    acc.add(w[:1200], f[:1200])
    held = acc.leaves()

    def unchanged():
        now = acc.leaves()
        return all(np.array_equal(now[k], held[k]) for k in held) and acc.info()["chunks"] == 1

    with pytest.raises(humid_amd.HumidError) as ei:
        acc.map(w[:1200], f[:1200], 0)                            # map before finish
    assert ei.value.code == -6 and unchanged()
    with pytest.raises(humid_amd.HumidError) as ei:
        acc.finish(1, 2)                                          # method 2
    assert ei.value.code == -1 and unchanged() and not acc.info()["finished"]
    assert lib.humid_accum_begin(h, 0) == -1 and lib.humid_accum_begin(h, 65) == -2 and unchanged()
    with pytest.raises(ValueError):
        acc.add(np.zeros((10, 2), np.uint64), np.zeros(10, np.uint8))      # two-word layout for word_nt 24
    with pytest.raises(ValueError):
        acc.map(w[:10], f[:9], 0)
    assert lib.humid_accum_add(h, None, None, 5, 0) == -1 and unchanged()
    assert lib.humid_accum_add(h, w.ctypes.data, f.ctypes.data, 2 ** 31, 0) == -5 and unchanged()
    wide = d.accumulator(48)
    with pytest.raises(ValueError):
        wide.add(w[:10], f[:10])                                  # one-word layout for word_nt 48
    wide.clear()
    # the context is as usable as before, and an accumulator survives an unrelated run between add and finish
    acc = d.accumulator(24)
    acc.add(w[:1200], f[:1200])
    got = d.run(w, f, 24, 1, 0)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    acc.add(w[1200:], f[1200:])
    d.run(w[:500], f[:500], 24, 2, 1)
    sm = acc.finish(1, 0)
    d.run(w[:700], f[:700], 24, 1, 0)
    c0, k0, _ = acc.map(w[:1200], f[:1200], 0)
    c1, k1, _ = acc.map(w[1200:], f[1200:], 1200)
    assert np.array_equal(np.concatenate([c0, c1]), ref[0]) and np.array_equal(np.concatenate([k0, k1]), ref[1])
    assert {k: sm[k] for k in FIELDS} == {k: ref[2][k] for k in FIELDS}
    d.close()


def test_larger(dd):
    w, f = synth(200_000, 5, 24, p_sub=1e-3, p_n=1e-4)
    chunks = split(w, f, (50_000, 120_000, 199_000))
    acc, s, res = accumulate(dd, 24, chunks)
    exp, esum = accum_expected(chunks, 24, 1, 0)[:2]
    assert_results(res, exp)
    assert {k: s[k] for k in FIELDS[:5]} == esum
    cid, keep, rs = dd.run(w, f, 24, 1, 0)
    assert np.array_equal(cat(res, 0), cid) and np.array_equal(cat(res, 1), keep)
    assert {k: s[k] for k in FIELDS} == {k: rs[k] for k in FIELDS}
