"""-m gpu: the best-scoring read of every cluster (humid_select_best*, kernels_best.hip.h) against the two truths of
tests/best_truth.py, bit for bit (keep_out, rep_out, n_changed), with guard words behind every output: read counts
around the wave and workgroup sizes, both scopes, one cluster / all singletons, ties, winners at both ends, sorted and
shuffled input, every word layout, after every kind of run, aliasing, the device-pointer form, every refusal, and
the state rules of the context."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from humid_amd.synth import synth_wide_words, synth_words

import best_truth as bt
from test_gpu_keyed import make_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
E_INVALID = -1
SCOPES = (bt.LEAF, bt.CLUSTER)


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_select(d, words, cid, keep, scores, word_nt, scope, alias=False, rep=True, rc_only=False):
    """humid_select_best through the C ABI with guard words behind every output buffer"""
    n = len(cid)
    w = np.ascontiguousarray(words, U64)
    cid = np.ascontiguousarray(cid, np.uint32)
    sc = np.ascontiguousarray(scores, np.uint32)
    kin = np.full(n + 16, 0xA5, np.uint8)
    kin[:n] = keep
    kout = kin if alias else np.full(n + 16, 0xA5, np.uint8)
    rout = np.full(n + 8, 0xA5A5A5A5, np.uint32) if rep else None
    ch = (C.c_uint64 * 2)(0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5A5A5A5A5)
    rc = d._lib.humid_select_best(d._h, vp(w), vp(cid), vp(kin), vp(sc), n, word_nt, scope, vp(kout), vp(rout),
                                  C.cast(ch, C.POINTER(C.c_uint64)))
    assert np.all(kout[n:] == 0xA5) and (rout is None or np.all(rout[n:] == 0xA5A5A5A5)) and ch[1] == 0xA5A5A5A5A5A5A5A5
    if rc_only:
        return rc, kout[:n].copy(), None if rout is None else rout[:n].copy()
    d._check(rc)
    return kout[:n].copy(), None if rout is None else rout[:n].copy(), int(ch[0])


def truth(words, cid, keep, scores, scope, loop=None):
    """the sort truth, cross-checked against the dict loop up to 20 000 reads"""
    t = bt.select_sort(words, cid, keep, scores, scope)
    if loop if loop is not None else len(cid) <= 20_000:
        bt.assert_same(t, bt.select_loop(words, cid, keep, scores, scope), "the two truths")
    assert int(t[0].sum()) == int(np.asarray(cid).max(initial=0))     # sum(keep_out) == clusters
    return t


def check(d, words, cid, keep, scores, word_nt, scopes=SCOPES, **kw):
    out = {}
    for scope in scopes:
        t = truth(words, cid, keep, scores, scope)
        bt.assert_same(t, raw_select(d, words, cid, keep, scores, word_nt, scope, **kw), "scope %d" % scope)
        out[scope] = t
    return out


@pytest.fixture(scope="module")
def big():
    """200 000 reads, 24 nt, d = 1, scores uniform in [0, 12000): shared by the tests that only read it"""
    words, filt = synth_words(200_000, 5, 24)
    scores = np.random.default_rng(5).integers(0, 12000, len(words)).astype(np.uint32)
    return words, filt, scores


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_small_read_counts(dd, n):
    rng = np.random.default_rng(n)
    words, filt = make_words(10 + n, n, 24, n_base=max(1, n // 8))
    cid, keep, _ = dd.run(words, filt, word_nt=24)
    check(dd, words, cid, keep, rng.integers(0, 50, n).astype(np.uint32), 24)


def test_200k_both_scopes_not_degenerate(dd, big):
    words, filt, scores = big
    cid, keep, s = dd.run(words, filt, word_nt=24)
    t = check(dd, words, cid, keep, scores, 24)
    assert t[bt.LEAF][2] > s["clusters"] // 4                          # representatives change ...
    assert np.count_nonzero(t[bt.LEAF][0] != t[bt.CLUSTER][0]) > 100   # ... and the scopes differ
    # constant scores give back keep under LEAF (keep IS the first read of the maxLeaf); under CLUSTER the first read
    # of the whole cluster wins, which the truth says is another read in some clusters
    const = np.full(len(cid), 7, np.uint32)
    k2, rep, ch = raw_select(dd, words, cid, keep, const, 24, bt.LEAF)
    assert np.array_equal(k2, keep) and ch == 0
    first = np.zeros(s["clusters"] + 1, np.uint32)
    first[cid[keep != 0]] = np.flatnonzero(keep)
    assert np.array_equal(rep[cid != 0], first[cid[cid != 0]]) and np.all(rep[cid == 0] == bt.NO_READ)
    tc = check(dd, words, cid, keep, const, 24, scopes=(bt.CLUSTER,))[bt.CLUSTER]
    lowest = np.full(s["clusters"] + 1, len(cid), np.int64)
    np.minimum.at(lowest, cid, np.arange(len(cid)))
    assert np.array_equal(np.flatnonzero(tc[0]), np.sort(lowest[1:])) and tc[2] > 0


def test_one_cluster_and_all_singletons(dd):
    n = 100_000
    rng = np.random.default_rng(1)
    words = np.full(n, 0x123456789ABC, U64)                             # every atomic hits one address
    filt = np.zeros(n, np.uint8)
    cid, keep, s = dd.run(words, filt, word_nt=24)
    assert s["clusters"] == 1
    scores = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    check(dd, words, cid, keep, scores, 24)
    words = (np.arange(n, dtype=U64) * U64(0x9E3779B97F4A7C15)) >> U64(16)   # 48 random-looking bits, distinct
    words = rng.permutation(words)
    cid, keep, s = dd.run(words, filt, word_nt=24, distance=0)
    assert s["clusters"] == n
    t = check(dd, words, cid, keep, scores, 24)
    assert t[bt.LEAF][2] == 0 and np.array_equal(t[bt.LEAF][0], keep)


def test_ties_and_winners_at_both_ends(dd):
    """the top score several times (smallest index wins); the winner is read 0; the winner is read N - 1; scores 0
    and 2^32 - 1"""
    n = 1000
    words, filt = make_words(3, n, 24, n_base=5, p_sub=0.01, p_filt=0.0)
    words[0] = words[n - 1] = words[500]                                # (one word at both ends and in the middle)
    cid, keep, _ = dd.run(words, filt, word_nt=24)
    assert cid[0] == cid[n - 1] != 0
    rng = np.random.default_rng(3)
    base = rng.integers(0, 100, n).astype(np.uint32)
    for name in ("ties", "first", "last", "extremes"):
        sc = base.copy()
        if name == "ties":
            sc[rng.integers(0, n, 300)] = 100                           # many reads share the top score
        elif name == "first":
            sc[0] = 0xffffffff
        elif name == "last":
            sc[n - 1] = 0xffffffff
        else:
            sc[:] = 0
            sc[n // 2] = 0xffffffff
        t = check(dd, words, cid, keep, sc, 24)
        if name == "first":
            assert t[bt.CLUSTER][0][0] == 1
        if name == "last":
            assert t[bt.CLUSTER][0][n - 1] == 1 and t[bt.CLUSTER][1][0] == n - 1


def test_sorted_runs_and_the_same_input_shuffled(dd, big):
    words, filt, scores = big
    words, filt, scores = words[:50_000], filt[:50_000], scores[:50_000]
    order = np.argsort(words, kind="stable")                            # runs of equal ids inside a wave
    for o in (order, np.random.default_rng(9).permutation(len(words))):
        w, f, sc = words[o], filt[o], scores[o]
        cid, keep, _ = dd.run(w, f, word_nt=24)
        check(dd, w, cid, keep, sc, 24)


@pytest.mark.parametrize("word_nt", [8, 24, 32, 33, 48, 64])
def test_word_lengths(dd, word_nt):
    n = 5000
    rng = np.random.default_rng(word_nt)
    words, filt = make_words(word_nt, n, word_nt, n_base=40)
    if word_nt > 32:
        # pairs of words that agree in hi only and in lo only, inside one cluster at d >= 1 or not: the comparison
        # must take both halves
        words[10] = words[11]
        words[11, 1] ^= U64(1)
        words[20] = words[21]
        words[21, 0] ^= U64(1)
    cid, keep, _ = dd.run(words, filt, word_nt=word_nt, distance=1)
    t = check(dd, words, cid, keep, rng.integers(0, 1000, n).astype(np.uint32), word_nt)
    assert np.count_nonzero(t[bt.LEAF][0] != t[bt.CLUSTER][0]) > 0


def test_wide_synthetic(dd):
    words, filt = synth_wide_words(30_000, 4, 48)
    cid, keep, _ = dd.run(words, filt, word_nt=48)
    check(dd, words, cid, keep, np.random.default_rng(4).integers(0, 12000, len(filt)).astype(np.uint32), 48)


def test_after_every_kind_of_run(dd):
    n, nt = 4000, 24
    rng = np.random.default_rng(21)
    words, filt = make_words(21, n, nt, n_base=30)
    scores = rng.integers(0, 1000, n).astype(np.uint32)
    # bases
    rows = rng.integers(0, 4, size=(n, nt))
    rows[1::2] = rows[0::2]                                             # pairs of equal words
    bases = np.frombuffer(b"ACGT", np.uint8)[rows]
    bases[5, 3] = ord("N")
    cid, keep, _ = dd.run_bases(bases, word_nt=nt)
    w, f = dd.packed_words()
    assert cid[5] == 0
    check(dd, w, cid, keep, scores, nt)
    # grouped: the same word in two groups, the top score in the wrong group
    groups = rng.integers(0, 7, n).astype(np.uint32)
    words[100], words[101], words[102] = words[103], words[103], words[103]
    groups[[100, 101, 102, 103]] = [1, 1, 2, 2]
    filt[100:104] = 0
    sc = scores.copy()
    sc[100:104] = [5, 4, 0xfffffff0, 3]
    cid, keep, _ = dd.run_grouped(words, groups, filt, word_nt=nt, n_groups=7)
    assert cid[100] == cid[101] != cid[102] == cid[103]
    t = check(dd, words, cid, keep, sc, nt)
    assert t[bt.CLUSTER][1][100] != 102
    # keyed
    keys = rng.integers(0, 1 << 40, 50, dtype=np.uint64)[rng.integers(0, 50, n)]
    cid, keep, _ = dd.run_keyed(words, keys, filt, word_nt=nt)
    check(dd, words, cid, keep, scores, nt)
    # corrected: an unmatched read carries the top score
    wl = np.unique(keys)[:40]
    dd.set_whitelist(wl, 20)
    sc = scores.copy()
    bad = int(np.flatnonzero((filt == 0) & ~np.isin(keys, wl))[0])
    sc[bad] = 0xffffffff
    cid, keep, _ = dd.run_keyed(words, keys, filt, word_nt=nt, correct=True)
    status, counts = dd.barcode_status()
    assert status[bad] >= humid_amd.BC_AMBIGUOUS and cid[bad] == 0
    t = check(dd, words, cid, keep, sc, nt)
    assert t[bt.CLUSTER][0][bad] == 0 and t[bt.CLUSTER][1][bad] == bt.NO_READ
    st2, c2 = dd.barcode_status()                                       # the run's accessors are intact
    assert np.array_equal(st2, status) and np.array_equal(c2, counts)
    dd.set_whitelist(None)


def test_edit_distance_and_method_maximum(dd):
    words, filt = make_words(33, 6000, 24, n_base=50, p_sub=0.05)
    scores = np.random.default_rng(33).integers(0, 1000, len(filt)).astype(np.uint32)
    for kw in (dict(distance=2, edit=True), dict(distance=1, method=humid_amd.MAXIMUM), dict(distance=2)):
        cid, keep, _ = dd.run(words, filt, word_nt=24, **kw)
        check(dd, words, cid, keep, scores, 24)
    dd.set_option("edit_distance", 0)


def test_garbage_on_reads_without_a_cluster(dd):
    words, filt = make_words(41, 3000, 24, n_base=30, p_filt=0.2)
    cid, keep, _ = dd.run(words, filt, word_nt=24)
    scores = np.random.default_rng(41).integers(0, 1000, len(filt)).astype(np.uint32)
    t = check(dd, words, cid, keep, scores, 24)
    w2, s2 = words.copy(), scores.copy()
    w2[cid == 0] = U64(0xFFFFFFFFFFFFFFFF)
    s2[cid == 0] = 0xffffffff
    for scope in SCOPES:
        bt.assert_same(t[scope], raw_select(dd, w2, cid, keep, s2, 24, scope))


def test_aliasing_no_rep_and_the_python_call(dd, big):
    words, filt, scores = (a[:30_000] for a in big)
    cid, keep, _ = dd.run(words, filt, word_nt=24)
    for scope, name in zip(SCOPES, ("leaf", "cluster")):
        t = truth(words, cid, keep, scores, scope)
        k2, rep, ch = raw_select(dd, words, cid, keep, scores, 24, scope, alias=True)
        bt.assert_same(t, (k2, rep, ch), "keep_out aliasing keep")
        k2, rep, ch = raw_select(dd, words, cid, keep, scores, 24, scope, rep=False)
        assert rep is None and np.array_equal(k2, t[0]) and ch == t[2]
        bt.assert_same(t, dd.select_best(words, cid, keep, scores, word_nt=24, scope=name))
    assert humid_amd.BEST_LEAF == 0 and humid_amd.BEST_CLUSTER == 1 and humid_amd.NO_READ == 0xffffffff


def test_device_pointer_form(dd, big):
    import torch
    words, filt, scores = (a[:60_000] for a in big)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_sc = torch.from_numpy(scores.view(np.int32)).to(dev)
    n = len(filt)
    d_cid = torch.zeros(n + 4, dtype=torch.int32, device=dev)
    d_keep = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    d_out = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=dev)
    d_rep = torch.full((n + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    dd.run_device(d_w.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), n)
    cid, keep = d_cid.cpu().numpy().view(np.uint32)[:n], d_keep.cpu().numpy()[:n]
    for scope, name in zip(SCOPES, ("leaf", "cluster")):
        t = truth(words, cid, keep, scores, scope)
        ch = dd.select_best_device(d_w.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), d_sc.data_ptr(), d_out.data_ptr(),
                                   d_rep.data_ptr(), n, word_nt=24, scope=name)
        out, rep = d_out.cpu().numpy(), d_rep.cpu().numpy().view(np.uint32)
        assert np.all(out[n:] == 0xA5) and np.all(rep[n:] == 0x5A5A5A5A)
        bt.assert_same(t, (out[:n], rep[:n], ch))
        ch = dd.select_best_device(d_w.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), d_sc.data_ptr(), d_out.data_ptr(),
                                   0, n, word_nt=24, scope=name)
        assert ch == t[2] and np.array_equal(d_out.cpu().numpy()[:n], t[0])
    # in place: keep_out is keep
    t = truth(words, cid, keep, scores, bt.LEAF)
    ch = dd.select_best_device(d_w.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), d_sc.data_ptr(), d_keep.data_ptr(), 0, n)
    assert ch == t[2] and np.array_equal(d_keep.cpu().numpy()[:n], t[0])
    # wide words off the 16-byte alignment are refused
    wide, wfilt = synth_wide_words(1000, 2, 48)
    d_ww = torch.zeros(2 * 1000 + 1, dtype=torch.int64, device=dev)
    d_ww[1:] = torch.from_numpy(wide.view(np.int64).reshape(-1)).to(dev)
    cidw, keepw, _ = dd.run(wide, wfilt, word_nt=48)
    d_c2, d_k2 = torch.from_numpy(cidw.view(np.int32)).to(dev), torch.from_numpy(keepw).to(dev)
    torch.cuda.synchronize()
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.select_best_device(d_ww.data_ptr() + 8, d_c2.data_ptr(), d_k2.data_ptr(), d_sc.data_ptr(), d_out.data_ptr(), 0, 1000,
                              word_nt=48)
    assert ei.value.code == E_INVALID and "aligned" in str(ei.value)


def test_every_refusal_leaves_the_context_usable(dd):
    n = 3000
    words, filt = make_words(51, n, 24, n_base=30)
    scores = np.random.default_rng(51).integers(0, 1000, n).astype(np.uint32)
    fresh = humid_amd.Dedup()
    rc, _, _ = raw_select(fresh, words, np.zeros(n, np.uint32), np.zeros(n, np.uint8), scores, 24, 0, rc_only=True)
    assert rc == E_INVALID                                              # no run in this context
    fresh.close()
    cid, keep, s = dd.run(words, filt, word_nt=24)
    clusters = dd.clusters()
    leaves = dd.leaves()
    t = truth(words, cid, keep, scores, bt.LEAF)

    def refused(**kw):
        a = dict(words=words, cid=cid, keep=keep, scores=scores, word_nt=24, scope=0)
        a.update(kw)
        rc, kout, rout = raw_select(dd, a["words"], a["cid"], a["keep"], a["scores"], a["word_nt"], a["scope"], rc_only=True)
        assert rc == E_INVALID, kw
        assert np.all(kout == 0xA5) and np.all(rout == 0xA5A5A5A5)      # nothing was written
        assert dd._lib.humid_last_error(dd._h)
        # the context is usable and the run's accessors answer as before
        got = dd.clusters()
        assert all(np.array_equal(got[k], clusters[k]) for k in clusters)
        bt.assert_same(t, raw_select(dd, words, cid, keep, scores, 24, 0))

    refused(scope=2)
    refused(word_nt=23)
    refused(words=words[:-1], cid=cid[:-1], keep=keep[:-1], scores=scores[:-1])          # another n_reads
    bad = cid.copy()
    bad[7] = s["clusters"] + 1
    refused(cid=bad)                                                    # an id above the cluster count
    bad[7] = 0xffffffff
    refused(cid=bad)                                                    # garbage ids: nothing faults
    bad = np.random.default_rng(1).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    refused(cid=bad)
    k0 = keep.copy()
    k0[np.flatnonzero(keep)[3]] = 0
    refused(keep=k0)                                                    # a cluster with no kept read
    k2 = keep.copy()
    k2[np.flatnonzero((keep == 0) & (cid != 0))[0]] = 1
    refused(keep=k2)                                                    # a cluster with two
    k2[np.flatnonzero(keep)[-1]] = 0                                    # ... and another with none: the count is right
    refused(keep=k2)
    for hole in range(5):                                               # null buffers
        args = [vp(words), vp(cid), vp(keep), vp(scores), vp(np.zeros(n, np.uint8))]
        args[hole] = None
        rc = dd._lib.humid_select_best(dd._h, args[0], args[1], args[2], args[3], n, 24, 0, args[4], None, None)
        assert rc == E_INVALID, hole
    assert dd._lib.humid_select_best(None, vp(words), vp(cid), vp(keep), vp(scores), n, 24, 0, vp(np.zeros(n, np.uint8)),
                                     None, None) == E_INVALID
    bt.assert_same(t, raw_select(dd, words, cid, keep, scores, 24, 0))
    got = dd.leaves()
    assert all(np.array_equal(got[k], leaves[k]) for k in leaves)
    # after humid_cluster_graph the context holds no run
    g = humid_amd.ClusterGraph([3, 1])
    g.link(0, 1)
    g.find_clusters()
    rc, _, _ = raw_select(g, np.zeros(2, U64), np.ones(2, np.uint32), np.asarray([1, 0], np.uint8), np.zeros(2, np.uint32), 24, 0,
                          rc_only=True)
    assert rc == E_INVALID
    g.close()


def test_no_state_leaks_into_a_following_run(dd):
    words, filt = make_words(61, 5000, 24, n_base=40)
    scores = np.random.default_rng(61).integers(0, 1000, len(filt)).astype(np.uint32)
    cid, keep, s = dd.run(words, filt, word_nt=24)
    before = (dd.leaves(), dd.clusters(), dd.group_stats())
    check(dd, words, cid, keep, scores, 24)
    after = (dd.leaves(), dd.clusters(), dd.group_stats())              # the accessors of the run are intact
    for a, b in zip(before, after):
        assert all(np.array_equal(a[k], b[k]) for k in a)
    cid2, keep2, s2 = dd.run(words, filt, word_nt=24)
    assert np.array_equal(cid, cid2) and np.array_equal(keep, keep2)
    assert all(s[k] == s2[k] for k in ("total", "usable", "unique", "clusters", "edges"))
    w3, f3 = make_words(62, 700, 30, n_base=10)                         # another shape: the old tables do not serve it
    cid3, keep3, _ = dd.run(w3, f3, word_nt=30)
    check(dd, w3, cid3, keep3, scores[:700], 30)


def test_three_million_reads(dd):
    words, filt = synth_words(3_000_000, 77, 24)
    scores = np.random.default_rng(77).integers(0, 12000, len(filt)).astype(np.uint32)
    cid, keep, s = dd.run(words, filt, word_nt=24)
    for scope in SCOPES:
        t = bt.select_sort(words, cid, keep, scores, scope)
        assert int(t[0].sum()) == s["clusters"] and t[2] > 0
        bt.assert_same(t, raw_select(dd, words, cid, keep, scores, 24, scope))
