"""-m gpu: consensus reads per cluster (humid_consensus*, kernels_consensus.hip.h) against the two truths of
tests/consensus_truth.py, bit for bit (out_off, both blobs, depth, errors, the summary), through the raw C ABI with
guard words behind every output: read counts around the wave and workgroup sizes, mixed read lengths 0 .. 5000, cluster
sizes on both sides of every path (singleton, one wave's member batch of 64, the large-cluster bound of 1024 and its
pieces), one cluster of 10^5 reads, all singletons, 200 k reads after every kind of run, ids sorted and shuffled, a
representative moved by select_best, thresholds and caps, odd quality bytes, garbage in reads without a cluster,
independence of the member order, the device-pointer forms, the getter's NULLs and room, every refusal, and the state
rules of the context."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib
from humid_amd.synth import synth_words

import consensus_truth as ct
from test_gpu_group_stats import device_view
from test_gpu_keyed import make_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
E_INVALID, E_STATE = -1, -6
BIG = 1024                     # CONS_BIG / CONS_PIECE of kernels_consensus.hip.h
G8, G32, G64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_get(d, sm):
    """humid_get_consensus with guard words behind every output"""
    c, t = sm["n_clusters"], sm["total_bytes"]
    ooff = np.full(c + 1 + 4, G64, U64)
    ob, oq = np.full(t + 16, G8, np.uint8), np.full(t + 16, G8, np.uint8)
    depth, errors = np.full(c + 8, G32, np.uint32), np.full(c + 4, G64, U64)
    d._check(d._lib.humid_get_consensus(d._h, t, vp(ooff), vp(ob), vp(oq), vp(depth), vp(errors)))
    assert np.all(ooff[c + 1:] == G64) and np.all(ob[t:] == G8) and np.all(oq[t:] == G8)
    assert np.all(depth[c:] == G32) and np.all(errors[c:] == G64)
    return dict(out_off=ooff[:c + 1].copy(), bases=ob[:t].copy(), quals=oq[:t].copy(), depth=depth[:c].copy(),
                errors=errors[:c].copy(), summary=sm)


def raw_call(d, b, q, off, cid, keep, C_, min_q=10, cap_q=93, n_bytes=None):
    """humid_consensus through the C ABI; returns (rc, summary dict)"""
    b, q = np.ascontiguousarray(b, np.uint8), np.ascontiguousarray(q, np.uint8)
    off, cid, keep = np.ascontiguousarray(off, U64), np.ascontiguousarray(cid, np.uint32), np.ascontiguousarray(keep, np.uint8)
    sm = (_lib.HumidConsensusSummary * 2)()
    C.memset(C.byref(sm[1]), G8, C.sizeof(sm[1]))
    rc = d._lib.humid_consensus(d._h, vp(b), vp(q), vp(off), len(b) if n_bytes is None else n_bytes, vp(cid), vp(keep), len(cid),
                                C_, min_q, cap_q, C.cast(sm, C.POINTER(_lib.HumidConsensusSummary)))
    assert sm[1].n_clusters == G64 and sm[1].errors == G64
    return rc, sm[0].asdict()


def raw_consensus(d, b, q, off, cid, keep, C_, min_q=10, cap_q=93):
    rc, sm = raw_call(d, b, q, off, cid, keep, C_, min_q, cap_q)
    d._check(rc)
    return raw_get(d, sm)


def truth(b, q, off, cid, keep, C_, min_q=10, cap_q=93, loop=None):
    """the numpy truth, cross-checked against the dict loop on small inputs"""
    t = ct.consensus_numpy(b, q, off, cid, keep, C_, min_q, cap_q)
    if loop if loop is not None else len(b) <= 400_000:
        ct.assert_same(t, ct.consensus_loop(b, q, off, np.asarray(cid), np.asarray(keep), C_, min_q, cap_q), "the two truths")
    return t


def check(d, b, q, off, cid, keep, C_, what="", **kw):
    t = truth(b, q, off, cid, keep, C_, **kw)
    kw.pop("loop", None)
    ct.assert_same(t, raw_consensus(d, b, q, off, cid, keep, C_, **kw), what)
    return t


def sized_clusters(rng, sizes, n_zero=0, shuffle=True):
    """cluster ids for clusters of the given sizes (ids in the given order) + n_zero reads without a cluster; keep =
    a random member of every cluster"""
    cid = np.repeat(np.arange(1, len(sizes) + 1, dtype=np.uint32), sizes)
    cid = np.concatenate([cid, np.zeros(n_zero, np.uint32)])
    if shuffle:
        cid = rng.permutation(cid)
    keep = np.zeros(len(cid), np.uint8)
    order = np.argsort(cid, kind="stable")
    start = np.cumsum(np.r_[n_zero, sizes])[:-1]
    keep[order[start + rng.integers(0, np.asarray(sizes))]] = 1
    return cid, keep


LENGTHS = np.asarray([0, 1, 63, 64, 65, 151, 300])


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_small_read_counts(dd, n):
    rng = np.random.default_rng(n)
    words, filt = make_words(10 + n, n, 24, n_base=max(1, n // 8))
    cid, keep, s = dd.run(words, filt, word_nt=24)
    b, q, off = ct.random_reads(rng, cid, rng.choice(LENGTHS, n), odd_quals=True)
    t = check(dd, b, q, off, cid, keep, s["clusters"])
    assert t["summary"]["n_clusters"] == s["clusters"]
    assert len(dd.leaves()["count"]) == s["unique"]                     # the run's accessors are intact


@pytest.mark.parametrize("shuffle", [False, True])
def test_mixed_lengths_and_cluster_sizes(dd, shuffle):
    """every length, one read of 5000, inside clusters of 1, 2, 63, 64, 65, 129 reads and both sides of the large-cluster
    bound (1023, 1024, 1025: two pieces, 2049: three), ids sorted and shuffled, garbage in the reads without a cluster"""
    rng = np.random.default_rng(7 + shuffle)
    sizes = [1, 2, 63, 64, 65, 129, 1, BIG - 1, BIG, BIG + 1, 2 * BIG + 1, 1, 3]
    cid, keep = sized_clusters(rng, sizes, n_zero=50, shuffle=shuffle)
    lengths = rng.choice(LENGTHS, len(cid), p=[.05, .05, .2, .2, .2, .2, .1])
    for c in (2, 5, 9, 10):                                             # a long representative, a long member
        lengths[np.flatnonzero((cid == c) & (keep != 0))[0]] = 300
    lengths[np.flatnonzero((cid == 11) & (keep != 0))[0]] = 5000
    lengths[np.flatnonzero((cid == 11) & (keep == 0))[:3]] = [5000, 4000, 65]
    lengths[np.flatnonzero(cid == 7)[0]] = 0                            # a singleton of length 0
    b, q, off = ct.random_reads(rng, cid, lengths, odd_quals=True)
    zero = np.flatnonzero(cid == 0)
    for i in zero:
        b[int(off[i]):int(off[i + 1])] = rng.integers(0, 256, int(lengths[i]))
        q[int(off[i]):int(off[i + 1])] = rng.integers(0, 256, int(lengths[i]))
    t = check(dd, b, q, off, cid, keep, len(sizes), loop=False)
    assert list(t["depth"]) == sizes and t["summary"]["multi_read"] == len(sizes) - 3
    assert t["summary"]["bases_changed"] > 0 and t["summary"]["errors"] > 0 and np.any(t["bases"] == ord("N"))
    for min_q, cap_q in ((0, 1), (10, 40), (93, 93)):
        check(dd, b, q, off, cid, keep, len(sizes), loop=False, min_q=min_q, cap_q=cap_q)


def test_small_clusters_against_the_loop_truth(dd):
    """the same shapes at sizes the dict loop takes in a second: it and the numpy form both agree with the device"""
    rng = np.random.default_rng(3)
    cid, keep = sized_clusters(rng, [1, 2, 63, 64, 65, 1, 7], n_zero=9)
    b, q, off = ct.random_reads(rng, cid, rng.choice(LENGTHS, len(cid)), odd_quals=True)
    for min_q, cap_q in ((0, 93), (10, 40), (93, 1)):
        check(dd, b, q, off, cid, keep, 7, loop=True, min_q=min_q, cap_q=cap_q)


def test_member_order_does_not_matter(dd):
    """two calls on differently shuffled copies of the same reads give identical bytes per cluster"""
    rng = np.random.default_rng(11)
    cid, keep = sized_clusters(rng, [5, 70, BIG + 300, 1, 200], shuffle=False)
    b, q, off = ct.random_reads(rng, cid, rng.choice(LENGTHS[2:], len(cid)), p_err=0.2)
    first = raw_consensus(dd, b, q, off, cid, keep, 5)
    again = raw_consensus(dd, b, q, off, cid, keep, 5)
    ct.assert_same(first, again, "the same call twice")
    lens = np.diff(off).astype(np.int64)
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(cid))
        rb = [bytes(b[int(off[i]):int(off[i + 1])]) for i in perm]
        rq = [bytes(q[int(off[i]):int(off[i + 1])]) for i in perm]
        pb, pq, poff = ct.flat(rb, rq)
        assert np.array_equal(np.diff(poff).astype(np.int64), lens[perm])
        ct.assert_same(first, raw_consensus(dd, pb, pq, poff, cid[perm], keep[perm], 5), "shuffled copy %d" % seed)
    ct.assert_same(first, truth(b, q, off, cid, keep, 5, loop=False), "truth")


def test_one_cluster_of_100k_reads(dd):
    n, length = 100_000, 150
    rng = np.random.default_rng(5)
    cid = np.ones(n, np.uint32)
    keep = np.zeros(n, np.uint8)
    keep[77_777] = 1
    b, q, off = ct.random_reads(rng, cid, np.full(n, length), p_err=0.3)
    t = ct.consensus_numpy(b, q, off, cid, keep, 1)
    assert t["summary"]["errors"] > n * length // 10 and int(t["depth"][0]) == n
    # through the Python wrapper, as u8[N, L] matrices (off implied)
    got = dd.consensus(b.reshape(n, length), q.reshape(n, length), cid, keep)
    ct.assert_same(t, got, "one cluster")
    assert np.all(t["quals"] == 33 + 93)                                # 10^5 reads agree far beyond the cap


def test_all_singletons(dd):
    n = 20_000
    rng = np.random.default_rng(9)
    cid = rng.permutation(np.arange(1, n + 1, dtype=np.uint32))
    keep = np.ones(n, np.uint8)
    b, q, off = ct.random_reads(rng, cid, rng.integers(90, 111, n))
    t = check(dd, b, q, off, cid, keep, n, loop=False)
    assert t["summary"]["multi_read"] == 0 and t["summary"]["bases_changed"] == 0 and t["summary"]["errors"] == 0
    # a singleton's consensus is its own record (cap_q >= p), laid out by cluster id
    order = np.argsort(cid)
    assert bytes(t["bases"]) == b"".join(bytes(b[int(off[i]):int(off[i + 1])]) for i in order)
    assert bytes(t["quals"]) == b"".join(bytes(q[int(off[i]):int(off[i + 1])]) for i in order)


@pytest.fixture(scope="module")
def big():
    """200 000 words of 24 nt and 50 keys, shared by the tests that only read them.  The key is a function of the
    word's first 12 nucleotides, so the reads of a family share it (random keys per read would cut nearly every cluster
    into singletons, and the consensus would have nothing to vote on)"""
    words, filt = synth_words(200_000, 5, 24)
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 1 << 40, 50, dtype=np.uint64)[((words >> U64(24)) % U64(50)).astype(np.int64)]
    return words, filt, keys


@pytest.mark.parametrize("kind", ["run", "keyed", "corrected"])
def test_200k_reads_after_every_kind_of_run(dd, big, kind):
    words, filt, keys = big
    if kind == "run":
        cid, keep, s = dd.run(words, filt, word_nt=24)
    elif kind == "keyed":
        cid, keep, s = dd.run_keyed(words, keys, filt, word_nt=24)
    else:
        dd.set_whitelist(np.unique(keys)[:40], 20)
        cid, keep, s = dd.run_keyed(words, keys, filt, word_nt=24, correct=True)
        status, counts = dd.barcode_status()
        assert np.any((cid == 0) & (filt == 0))                         # unmatched reads are no members
    rng = np.random.default_rng(len(kind))
    b, q, off = ct.random_reads(rng, cid, np.full(len(cid), 100))
    t = ct.consensus_numpy(b, q, off, cid, keep, s["clusters"])
    ct.assert_same(t, raw_consensus(dd, b, q, off, cid, keep, s["clusters"]), kind)
    assert t["summary"]["multi_read"] > s["clusters"] // 4 and t["summary"]["bases_changed"] > 1000
    assert len(dd.leaves()["count"]) == s["unique"]                     # the run's accessors are intact
    if kind == "corrected":
        st2, c2 = dd.barcode_status()
        assert np.array_equal(st2, status) and np.array_equal(c2, counts)
        dd.set_whitelist(None)


def test_a_representative_moved_by_select_best(dd):
    """keep rewritten by select_best (scope cluster): the representative may carry a minority word and another length"""
    words, filt = make_words(21, 6000, 24, n_base=40, p_sub=0.05)
    cid, keep, s = dd.run(words, filt, word_nt=24)
    rng = np.random.default_rng(21)
    keep2, _, changed = dd.select_best(words, cid, keep, rng.integers(0, 1000, len(cid)).astype(np.uint32), scope="cluster")
    assert changed > 0
    b, q, off = ct.random_reads(rng, cid, rng.choice(LENGTHS[2:], len(cid)))
    t1 = check(dd, b, q, off, cid, keep, s["clusters"], loop=False)
    t2 = check(dd, b, q, off, cid, keep2, s["clusters"], loop=False)
    assert not np.array_equal(t1["out_off"], t2["out_off"]) and np.array_equal(t1["depth"], t2["depth"])


def dev(t):
    return t.data_ptr()


def test_device_pointer_forms(dd):
    import torch
    rng = np.random.default_rng(13)
    cid, keep = sized_clusters(rng, [3, 100, BIG + 5, 1], n_zero=4)
    b, q, off = ct.random_reads(rng, cid, rng.choice(LENGTHS[1:], len(cid)))
    t = truth(b, q, off, cid, keep, 4, loop=False)
    tb, tq = torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda()
    toff = torch.from_numpy(off.astype(np.int64)).cuda()
    tcid, tkeep = torch.from_numpy(cid.astype(np.int32)).cuda(), torch.from_numpy(keep).cuda()
    torch.cuda.synchronize()
    sm = dd.consensus_device(dev(tb), dev(tq), dev(toff), len(b), dev(tcid), dev(tkeep), len(cid), 4)
    assert sm == t["summary"]
    ct.assert_same(t, raw_get(dd, sm), "device form, host getter")
    p = dd.consensus_result_device()
    assert all(p[k] for k in ("out_off", "bases", "quals", "depth", "errors"))

    tot = sm["total_bytes"]
    got = dict(out_off=device_view(p["out_off"], 5, "<i8", U64), bases=device_view(p["bases"], tot, "|u1", np.uint8),
               quals=device_view(p["quals"], tot, "|u1", np.uint8), depth=device_view(p["depth"], 4, "<i4", np.uint32),
               errors=device_view(p["errors"], 4, "<i8", U64), summary=sm)
    ct.assert_same(t, got, "device form, device getter")
    assert np.array_equal(tb.cpu().numpy(), b) and np.array_equal(tcid.cpu().numpy().astype(np.uint32), cid)   # inputs untouched


def test_getter_nulls_and_room(dd):
    rng = np.random.default_rng(17)
    cid, keep = sized_clusters(rng, [4, 1, 9])
    b, q, off = ct.random_reads(rng, cid, rng.integers(1, 80, len(cid)))
    t = check(dd, b, q, off, cid, keep, 3)
    tot = t["summary"]["total_bytes"]
    lib, h = dd._lib, dd._h
    assert lib.humid_get_consensus(h, 0, None, None, None, None, None) == 0
    ooff = np.zeros(4, U64)
    assert lib.humid_get_consensus(h, 0, vp(ooff), None, None, None, None) == 0 and np.array_equal(ooff, t["out_off"])
    depth = np.full(3 + 2, G32, np.uint32)
    assert lib.humid_get_consensus(h, 0, None, None, None, vp(depth), None) == 0
    assert np.array_equal(depth[:3], t["depth"]) and np.all(depth[3:] == G32)
    ob = np.full(tot + 8, G8, np.uint8)
    assert lib.humid_get_consensus(h, tot - 1, None, vp(ob), None, None, None) == E_INVALID and np.all(ob == G8)
    assert b"room" in lib.humid_last_error(h)
    assert lib.humid_get_consensus(h, tot, None, vp(ob), None, None, None) == 0
    assert np.array_equal(ob[:tot], t["bases"]) and np.all(ob[tot:] == G8)
    oq = np.full(tot + 8, G8, np.uint8)
    assert lib.humid_get_consensus(h, tot + 5, None, None, vp(oq), None, None) == 0
    assert np.array_equal(oq[:tot], t["quals"]) and np.all(oq[tot:] == G8)


def test_empty_inputs(dd):
    e8, e32 = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    rc, sm = raw_call(dd, e8, e8, np.zeros(1, U64), e32, e8, 0)
    assert rc == 0 and sm == dict.fromkeys(ct.KEYS, 0)
    got = raw_get(dd, sm)
    assert list(got["out_off"]) == [0] and len(got["bases"]) == 0 and len(got["depth"]) == 0
    # C == 0 with reads: an empty result as well
    rc, sm = raw_call(dd, np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"IIII", np.uint8), np.asarray([0, 4], U64),
                      np.zeros(1, np.uint32), np.zeros(1, np.uint8), 0)
    assert rc == 0 and sm == dict.fromkeys(ct.KEYS, 0) and list(raw_get(dd, sm)["out_off"]) == [0]
    assert dd._lib.humid_consensus(dd._h, None, None, None, 0, None, None, 0, 5, 10, 93, None) == 0    # no reads, NULLs


def test_every_refusal_leaves_the_context_usable():
    d = humid_amd.Dedup()
    try:
        lib, h = d._lib, d._h
        # before any call: HUMID_E_STATE from both getters
        assert lib.humid_get_consensus(h, 0, None, None, None, None, None) == E_STATE
        ptrs = [C.c_void_p() for _ in range(5)]
        assert lib.humid_consensus_result_device(h, *[C.byref(x) for x in ptrs]) == E_STATE
        words, filt = make_words(31, 3000, 24, n_base=40)
        cid, keep, s = d.run(words, filt, word_nt=24)
        leaves = d.leaves()
        Cn = s["clusters"]
        rng = np.random.default_rng(31)
        b, q, off = ct.random_reads(rng, cid, rng.integers(0, 90, len(cid)))
        good = truth(b, q, off, cid, keep, Cn, loop=False)
        member = np.flatnonzero(cid != 0)
        multi = np.flatnonzero(np.bincount(cid)[cid] >= 2)
        multi = multi[cid[multi] != 0]

        def refused(code=E_INVALID, text=None, **kw):
            a = dict(b=b, q=q, off=off, cid=cid, keep=keep, C_=Cn)
            a.update(kw)
            rc, _ = raw_call(d, **a)
            assert rc == code, (rc, lib.humid_last_error(h))
            assert text is None or text in lib.humid_last_error(h), lib.humid_last_error(h)
            # a refused call leaves no result behind, the run's accessors intact and the context usable
            assert lib.humid_get_consensus(h, 0, None, None, None, None, None) == E_STATE
            lv = d.leaves()
            assert all(np.array_equal(lv[k], leaves[k]) for k in leaves)
            ct.assert_same(good, raw_consensus(d, b, q, off, cid, keep, Cn), "after a refusal")

        bad = cid.copy()
        bad[member[5]] = Cn + 1
        refused(cid=bad, text=b"above")                                 # an id above C
        refused(C_=Cn - 1)                                              # ... the same through a smaller C
        bad = keep.copy()
        bad[np.flatnonzero(keep)[3]] = 0
        refused(keep=bad, text=b"keep == 1")                            # a cluster without a kept read
        bad = keep.copy()
        bad[multi[np.flatnonzero(keep[multi] == 0)[0]]] = 1
        refused(keep=bad, text=b"more than one")                        # ... with two
        bad = off.copy()
        i = int(np.flatnonzero(np.diff(off.astype(np.int64)) > 0)[10])
        bad[i + 1] = bad[i] - U64(1) if bad[i] else bad[i + 2] + U64(1)
        refused(off=bad, text=b"decreases")                             # off decreasing
        refused(n_bytes=len(b) - 1, text=b"beyond")                     # off[n] > n_bytes
        bad = off.copy()
        bad[-1] += U64(1 << 40)
        refused(off=bad, text=b"beyond")
        refused(C_=len(cid) + 1)                                        # more clusters than reads
        for kw in (dict(min_q=94), dict(cap_q=0), dict(cap_q=94)):     # parameters out of range
            refused(**kw)
        args = [vp(b), vp(q), vp(off), len(b), vp(cid), vp(keep), len(cid), Cn, 10, 93, None]
        for k in (0, 1, 2, 4, 5):                                       # a NULL buffer
            a = list(args)
            a[k] = None
            assert lib.humid_consensus(h, *a) == E_INVALID
        assert lib.humid_consensus(h, *args) == 0                       # (summary may be NULL)
        # the results survive a later run, and that run is unharmed
        got = raw_consensus(d, b, q, off, cid, keep, Cn)
        sm = got["summary"]
        w2, f2 = make_words(32, 5000, 24)
        d.run(w2, f2, word_nt=24)
        d.select_best(w2, *d.run(w2, f2, word_nt=24)[:2], np.zeros(5000, np.uint32))
        ct.assert_same(good, raw_get(d, sm), "after a later run")
    finally:
        d.close()
