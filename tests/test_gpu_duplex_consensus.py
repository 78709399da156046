"""-m gpu: duplex consensus reads per cluster (humid_duplex_consensus*, kernels_dconsensus.hip.h) against the two truths
of tests/duplex_truth.py, bit for bit (out_off, both blobs, depth, errors, depth_same, depth_other, disagree, the
eleven-field summary), through the raw C ABI with guard words behind every output: read counts around the wave size
after a real strand-symmetric run, read lengths 0 .. 5000 drawn independently per layer, cluster sizes on both sides of
every path (singleton, one of each class, one wave's member batch of 64, the large-cluster bound of 1024 and its
pieces) with the class boundary at 0, 1, 64, 256, 1024, d - 1 and d, ids sorted and shuffled, garbage in reads without
a cluster, representatives of either strand and one moved by select_best, independence of the member order, the two
calls of a pair, thresholds and caps, odd quality bytes, the reduction to humid_consensus, the state rule the two kinds
of call share, the device-pointer form, the getter's NULLs, every HUMID_E_INVALID refusal, and empty inputs.
Two decisions.  A refused call ENDS the consensus results of the call before it, as the header says ("until the next
call, successful or not") and as humid_consensus does; what a refusal leaves intact, and what the refusal test checks,
are the accessors of the last run and a context on which the same call then succeeds.  HUMID_E_OVERFLOW (a cluster of
more than 46 182 444 reads) is left out: no test of a few seconds holds such a cluster; the check is k_cons_big_list's,
shared with the plain pass."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib

import consensus_truth as ct
import duplex_truth as dt
import paired_truth as pt
from test_gpu_group_stats import device_view

pytestmark = pytest.mark.gpu

U64 = np.uint64
E_INVALID, E_OVERFLOW, E_STATE = -1, -5, -6
BIG = 1024                     # CONS_BIG / CONS_PIECE of kernels_consensus.hip.h
G8, G32, G64 = 0xA5, 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
LENGTHS = np.asarray([0, 1, 63, 64, 65, 151, 300])


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_get(d, sm):
    """humid_get_consensus and humid_get_duplex_consensus with guard words behind every output"""
    c, t = sm["n_clusters"], sm["total_bytes"]
    ooff = np.full(c + 1 + 4, G64, U64)
    ob, oq = np.full(t + 16, G8, np.uint8), np.full(t + 16, G8, np.uint8)
    depth, errors = np.full(c + 8, G32, np.uint32), np.full(c + 4, G64, U64)
    d._check(d._lib.humid_get_consensus(d._h, t, vp(ooff), vp(ob), vp(oq), vp(depth), vp(errors)))
    assert np.all(ooff[c + 1:] == G64) and np.all(ob[t:] == G8) and np.all(oq[t:] == G8)
    assert np.all(depth[c:] == G32) and np.all(errors[c:] == G64)
    same, other, dis = [np.full(c + 8, G32, np.uint32) for _ in range(3)]
    s2 = (_lib.HumidDuplexSummary * 2)()
    C.memset(C.byref(s2[1]), G8, C.sizeof(s2[1]))
    d._check(d._lib.humid_get_duplex_consensus(d._h, vp(same), vp(other), vp(dis), C.cast(s2, C.POINTER(_lib.HumidDuplexSummary))))
    assert s2[1].n_clusters == G64 and s2[1].masked == G64 and s2[0].asdict() == sm
    assert np.all(same[c:] == G32) and np.all(other[c:] == G32) and np.all(dis[c:] == G32)
    return dict(out_off=ooff[:c + 1].copy(), bases=ob[:t].copy(), quals=oq[:t].copy(), depth=depth[:c].copy(),
                errors=errors[:c].copy(), depth_same=same[:c].copy(), depth_other=other[:c].copy(), disagree=dis[:c].copy(),
                summary=sm)


def raw_call(d, ls, lo, cid, keep, strand, C_, min_q=10, strand_cap_q=40, cap_q=93, n_bytes_s=None, n_bytes_o=None):
    """humid_duplex_consensus through the C ABI; returns (rc, summary dict)"""
    bs, qs, os_ = np.ascontiguousarray(ls[0], np.uint8), np.ascontiguousarray(ls[1], np.uint8), np.ascontiguousarray(ls[2], U64)
    bo, qo, oo = np.ascontiguousarray(lo[0], np.uint8), np.ascontiguousarray(lo[1], np.uint8), np.ascontiguousarray(lo[2], U64)
    cid, keep = np.ascontiguousarray(cid, np.uint32), np.ascontiguousarray(keep, np.uint8)
    strand = np.ascontiguousarray(strand, np.uint8)
    sm = (_lib.HumidDuplexSummary * 2)()
    C.memset(C.byref(sm[1]), G8, C.sizeof(sm[1]))
    rc = d._lib.humid_duplex_consensus(d._h, vp(bs), vp(qs), vp(os_), len(bs) if n_bytes_s is None else n_bytes_s, vp(bo), vp(qo), vp(oo),
                                       len(bo) if n_bytes_o is None else n_bytes_o, vp(cid), vp(keep), vp(strand), len(cid), C_, min_q,
                                       strand_cap_q, cap_q, C.cast(sm, C.POINTER(_lib.HumidDuplexSummary)))
    assert sm[1].n_clusters == G64 and sm[1].masked == G64
    return rc, sm[0].asdict()


def raw_duplex(d, ls, lo, cid, keep, strand, C_, **kw):
    rc, sm = raw_call(d, ls, lo, cid, keep, strand, C_, **kw)
    d._check(rc)
    return raw_get(d, sm)


def truth(ls, lo, cid, keep, strand, C_, loop=None, **kw):
    """the numpy truth, cross-checked against the dict loop on small inputs"""
    t = dt.duplex_numpy(ls, lo, cid, keep, strand, C_, **kw)
    if loop if loop is not None else len(ls[0]) + len(lo[0]) <= 400_000:
        dt.assert_same(t, dt.duplex_loop(ls, lo, cid, keep, strand, C_, **kw), "the two truths")
    return t


def check(d, ls, lo, cid, keep, strand, C_, what="", loop=None, **kw):
    t = truth(ls, lo, cid, keep, strand, C_, loop=loop, **kw)
    dt.assert_same(t, raw_duplex(d, ls, lo, cid, keep, strand, C_, **kw), what)
    return t


def garbage_outside(rng, cid, strand, *layers):
    """random bytes in the records, and random strand values, of the reads without a cluster"""
    zero = np.flatnonzero(cid == 0)
    strand[zero] = rng.integers(0, 256, len(zero))
    for b, q, off in layers:
        for i in zero:
            lo, hi = int(off[i]), int(off[i + 1])
            b[lo:hi] = rng.integers(0, 256, hi - lo)
            q[lo:hi] = rng.integers(0, 256, hi - lo)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_small_read_counts_after_a_paired_run(dd, n):
    rng = np.random.default_rng(n)
    words, filt = pt.families(10 + n, 24, n)
    cid, keep, s = dd.run_paired(words, filt, word_nt=24)
    strand = dd.strands()[0]
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS, n), rng.choice(LENGTHS, n), p_err=0.1, odd_quals=True)
    t = check(dd, l1, l2, cid, keep, strand, s["clusters"], "file 1")
    check(dd, l2, l1, cid, keep, strand, s["clusters"], "file 2")
    assert t["summary"]["n_clusters"] == s["clusters"]
    if n >= 63:
        assert t["summary"]["duplex_clusters"] > 0 and t["summary"]["both_called"] > 0
    assert len(dd.leaves()["count"]) == s["unique"]                     # the run's accessors are intact
    assert np.array_equal(dd.strands()[0], strand)


# cluster sizes on both sides of every path, and the number of TOP members of each: the class boundary at 0, 1, 64, 256,
# 1024, d - 1 and d, so that a piece (and a wave's quarter of it) lies wholly in one class, wholly in the other, or across
SIZES = [1, 2, 63, 64, 65, 129, 1, BIG - 1, BIG, BIG + 1, 2 * BIG + 1, 2 * BIG + 1, BIG + 1, BIG + 1, 2 * BIG + 1, 3, 2 * BIG + 1]
TOPS = [1, 1, 0, 64, 1, 64, 0, 256, BIG - 1, BIG, 256, BIG, 0, BIG + 1, 2 * BIG, 3, 1]
REP_TOP = [True, False, False, True, True, False, False, True, False, True, False, True, False, True, False, True, True]


@pytest.fixture(scope="module")
def mixed():
    """the inputs of the mixed test, ids sorted and shuffled, with the numpy truth of the default parameters; shared
    and left unchanged"""
    out = {}
    for shuffle in (False, True):
        rng = np.random.default_rng(7 + shuffle)
        cid, keep, strand = dt.sized_clusters(rng, SIZES, TOPS, n_zero=50, shuffle=shuffle, rep_top=REP_TOP)
        n = len(cid)
        len1 = rng.choice(LENGTHS, n, p=[.05, .05, .2, .2, .2, .2, .1])
        len2 = rng.choice(LENGTHS, n, p=[.05, .05, .2, .2, .2, .2, .1])
        for c in (2, 5, 9, 10, 12):                                     # a long representative in both layers
            r = np.flatnonzero((cid == c) & (keep != 0))[0]
            len1[r] = len2[r] = 300
        r = np.flatnonzero((cid == 11) & (keep != 0))[0]
        len1[r] = 5000                                                  # one read of 5000 ...
        same = np.flatnonzero((cid == 11) & (keep == 0) & (strand == strand[r]))
        other = np.flatnonzero((cid == 11) & (strand != strand[r]))
        len1[same[:2]] = [5000, 65]
        len2[other[:3]] = [5000, 4000, 65]                              # ... and members of the other class that reach its end
        len1[np.flatnonzero(cid == 7)[0]] = 0                           # a singleton of length 0
        l1, l2 = dt.duplex_reads(rng, cid, strand, keep, len1, len2, p_err=0.1, odd_quals=True)
        garbage_outside(rng, cid, strand, l1, l2)
        for a in (cid, keep, strand) + l1 + l2:
            a.setflags(write=False)
        out[shuffle] = (cid, keep, strand, l1, l2, dt.duplex_numpy(l1, l2, cid, keep, strand, len(SIZES)))
    return out


@pytest.mark.parametrize("shuffle", [False, True])
def test_mixed_lengths_cluster_sizes_and_class_boundaries(dd, mixed, shuffle):
    cid, keep, strand, l1, l2, t = mixed[shuffle]
    dt.assert_same(t, raw_duplex(dd, l1, l2, cid, keep, strand, len(SIZES)), "file 1")
    assert list(t["depth"]) == SIZES and t["summary"]["multi_read"] == len(SIZES) - 2
    rs = dt.rep_strand(cid, keep, strand)
    reps = np.flatnonzero(keep & (cid != 0))
    order = reps[np.argsort(cid[reps])]
    assert [bool(x) for x in rs[order] == dt.TOP] == REP_TOP
    assert list(t["depth_same"]) == [tp if r else d - tp for d, tp, r in zip(SIZES, TOPS, REP_TOP)]
    sm = t["summary"]
    assert sm["bases_changed"] > 0 and sm["errors"] > 0 and sm["disagree"] > 0 and sm["agree"] > 0 and sm["masked"] > 0
    assert sm["duplex_clusters"] == sum(0 < tp < d for d, tp in zip(SIZES, TOPS)) and sm["both_called"] == sm["agree"] + sm["disagree"]
    check(dd, l2, l1, cid, keep, strand, len(SIZES), "file 2", loop=False)          # the second call of the pair


@pytest.mark.parametrize("min_q,strand_cap_q,cap_q", [(0, 1, 93), (10, 40, 1), (93, 93, 93), (0, 93, 1), (10, 1, 1)])
def test_thresholds_and_caps(dd, mixed, min_q, strand_cap_q, cap_q):
    cid, keep, strand, l1, l2, _ = mixed[True]
    check(dd, l1, l2, cid, keep, strand, len(SIZES), loop=False, min_q=min_q, strand_cap_q=strand_cap_q, cap_q=cap_q)


def test_small_clusters_against_the_loop_truth(dd):
    """the same shapes at sizes the dict loop takes in a second: it and the numpy form both agree with the device"""
    rng = np.random.default_rng(3)
    sizes, tops = [1, 2, 63, 64, 65, 1, 7, 130], [0, 1, 62, 0, 64, 1, 3, 65]
    cid, keep, strand = dt.sized_clusters(rng, sizes, tops, n_zero=9)
    n = len(cid)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS[:6], n), rng.choice(LENGTHS[:6], n), p_err=0.15, odd_quals=True)
    garbage_outside(rng, cid, strand, l1, l2)
    for min_q, scap, cap_q in ((0, 93, 93), (10, 40, 40), (93, 1, 1), (10, 40, 93)):
        check(dd, l1, l2, cid, keep, strand, len(sizes), loop=True, min_q=min_q, strand_cap_q=scap, cap_q=cap_q)
        check(dd, l2, l1, cid, keep, strand, len(sizes), loop=True, min_q=min_q, strand_cap_q=scap, cap_q=cap_q)


def test_member_order_does_not_matter(dd):
    """two calls on differently shuffled copies of the same reads give identical bytes per cluster"""
    rng = np.random.default_rng(11)
    sizes, tops = [5, 70, BIG + 300, 1, 200], [2, 30, 500, 0, 199]
    cid, keep, strand = dt.sized_clusters(rng, sizes, tops, shuffle=False)
    n = len(cid)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS[2:], n), rng.choice(LENGTHS[2:], n), p_err=0.2)
    first = raw_duplex(dd, l1, l2, cid, keep, strand, 5)
    dt.assert_same(first, raw_duplex(dd, l1, l2, cid, keep, strand, 5), "the same call twice")

    def permuted(layer, perm):
        b, q, off = layer
        return ct.flat([bytes(b[int(off[i]):int(off[i + 1])]) for i in perm], [bytes(q[int(off[i]):int(off[i + 1])]) for i in perm])

    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(n)
        got = raw_duplex(dd, permuted(l1, perm), permuted(l2, perm), cid[perm], keep[perm], strand[perm], 5)
        dt.assert_same(first, got, "shuffled copy %d" % seed)
    dt.assert_same(first, truth(l1, l2, cid, keep, strand, 5, loop=False), "truth")
    # flipping every strand changes nothing
    dt.assert_same(first, raw_duplex(dd, l1, l2, cid, keep, strand ^ 1, 5), "flipped strands")


def test_a_representative_moved_by_select_best(dd):
    """keep rewritten by select_best (scope cluster) after a paired run: the representative may be of the other strand"""
    words, filt = pt.families(21, 24, 3000)
    cid, keep, s = dd.run_paired(words, filt, word_nt=24)
    strand = dd.strands()[0]
    cw, cs = dd.canonical_words(words, filt, word_nt=24)
    assert np.array_equal(cs, strand)
    rng = np.random.default_rng(21)
    keep2, _, changed = dd.select_best(cw, cid, keep, rng.integers(0, 1000, len(cid)).astype(np.uint32), scope="cluster")
    assert changed > 0
    n = len(cid)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS[2:], n), rng.choice(LENGTHS[2:], n), p_err=0.1)
    t1 = check(dd, l1, l2, cid, keep, strand, s["clusters"], loop=False)
    t2 = check(dd, l1, l2, cid, keep2, strand, s["clusters"], loop=False)
    assert np.array_equal(t1["depth"], t2["depth"]) and not np.array_equal(t1["depth_same"], t2["depth_same"])
    assert not np.array_equal(t1["out_off"], t2["out_off"])


def test_single_class_input_is_the_plain_consensus_on_the_device(dd):
    """every member of every cluster on its representative's strand, strand_cap_q = 93: the buffers humid_get_consensus
    returns are those of humid_consensus on layer S, whatever layer O holds"""
    rng = np.random.default_rng(13)
    sizes = [1, 2, 64, 65, 300, BIG, BIG + 1, 2 * BIG + 1, 1]
    tops = [1, 0, 64, 0, 300, 0, BIG + 1, 0, 0]
    cid, keep, strand = dt.sized_clusters(rng, sizes, tops, n_zero=20)
    n = len(cid)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS, n), rng.choice(LENGTHS, n), p_err=0.2, odd_quals=True)
    junk = (rng.integers(0, 256, len(l2[0])).astype(np.uint8), rng.integers(0, 256, len(l2[1])).astype(np.uint8), l2[2])
    for min_q, cap_q in ((10, 93), (0, 20)):
        got = raw_duplex(dd, l1, junk, cid, keep, strand, len(sizes), min_q=min_q, strand_cap_q=93, cap_q=cap_q)
        plain = dd.consensus(l1[0], l1[1], cid, keep, off=l1[2], n_clusters=len(sizes), min_q=min_q, cap_q=cap_q)
        ct.assert_same(plain, got, "against humid_consensus")           # five arrays, six summary fields
        ct.assert_same(ct.consensus_numpy(l1[0], l1[1], l1[2], cid, keep, len(sizes), min_q, cap_q), got, "against its truth")
        assert got["summary"]["duplex_clusters"] == 0 and got["summary"]["both_called"] == 0 and not got["depth_other"].any()
    # ... and on the device: both device-pointer forms on the same device arrays, the result buffers left in HBM compared
    import torch
    ten = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (l1[0], l1[1], l1[2].astype(np.int64), junk[0], junk[1],
                                                                      l2[2].astype(np.int64), cid.astype(np.int32), keep, strand)]
    torch.cuda.synchronize()
    p = [t.data_ptr() for t in ten]

    def device_buffers(sm):
        r, c, tot = dd.consensus_result_device(), sm["n_clusters"], sm["total_bytes"]
        return dict(out_off=device_view(r["out_off"], c + 1, "<i8", U64).copy(), bases=device_view(r["bases"], tot, "|u1", np.uint8).copy(),
                    quals=device_view(r["quals"], tot, "|u1", np.uint8).copy(), depth=device_view(r["depth"], c, "<i4", np.uint32).copy(),
                    errors=device_view(r["errors"], c, "<i8", U64).copy(), summary=sm)

    plain = device_buffers(dd.consensus_device(p[0], p[1], p[2], len(l1[0]), p[6], p[7], n, len(sizes), min_q=10, cap_q=93))
    dup = device_buffers(dd.duplex_consensus_device(p[0], p[1], p[2], len(l1[0]), p[3], p[4], p[5], len(junk[0]), p[6], p[7], p[8], n,
                                                    len(sizes), min_q=10, strand_cap_q=93, cap_q=93))
    ct.assert_same(plain, dup, "device forms, device buffers")


def test_the_state_rule_shared_with_the_plain_consensus(dd):
    rng = np.random.default_rng(15)
    cid, keep, strand = dt.sized_clusters(rng, [4, 1, 9], [2, 1, 3])
    n = len(cid)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.integers(1, 80, n), rng.integers(1, 80, n), p_err=0.2)
    lib, h = dd._lib, dd._h
    t = check(dd, l1, l2, cid, keep, strand, 3)
    # a plain call ends the duplex results: the duplex getter refuses, the shared getters answer for the plain call
    plain = dd.consensus(l1[0], l1[1], cid, keep, off=l1[2], n_clusters=3)
    ct.assert_same(ct.consensus_numpy(l1[0], l1[1], l1[2], cid, keep, 3), plain, "plain")
    assert lib.humid_get_duplex_consensus(h, None, None, None, None) == E_STATE
    assert b"duplex" in lib.humid_last_error(h)
    assert lib.humid_get_consensus(h, 0, None, None, None, None, None) == 0
    # a duplex call after a plain one: all getters answer for the duplex call
    dt.assert_same(t, raw_duplex(dd, l1, l2, cid, keep, strand, 3), "after a plain call")
    p = dd.consensus_result_device()
    tot = t["summary"]["total_bytes"]
    assert np.array_equal(device_view(p["bases"], tot, "|u1", np.uint8), t["bases"])
    assert np.array_equal(device_view(p["errors"], 3, "<i8", U64), t["errors"])
    # a refused plain call ends them as well
    assert lib.humid_consensus(h, vp(l1[0]), vp(l1[1]), vp(l1[2]), len(l1[0]), vp(cid), vp(keep), n, 3, 94, 93, None) == E_INVALID
    assert lib.humid_get_duplex_consensus(h, None, None, None, None) == E_STATE
    assert lib.humid_get_consensus(h, 0, None, None, None, None, None) == E_STATE


def dev(t):
    return t.data_ptr()


def test_device_pointer_form_and_python_wrapper(dd):
    import torch
    rng = np.random.default_rng(17)
    sizes, tops = [3, 100, BIG + 5, 1], [1, 40, 1000, 0]
    cid, keep, strand = dt.sized_clusters(rng, sizes, tops, n_zero=4)
    n = len(cid)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS[1:], n), rng.choice(LENGTHS[1:], n), p_err=0.1)
    t = truth(l1, l2, cid, keep, strand, 4, loop=False)
    ten = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (l1[0], l1[1], l1[2].astype(np.int64), l2[0], l2[1],
                                                                      l2[2].astype(np.int64), cid.astype(np.int32), keep, strand)]
    torch.cuda.synchronize()
    sm = dd.duplex_consensus_device(dev(ten[0]), dev(ten[1]), dev(ten[2]), len(l1[0]), dev(ten[3]), dev(ten[4]), dev(ten[5]),
                                    len(l2[0]), dev(ten[6]), dev(ten[7]), dev(ten[8]), n, 4)
    assert sm == t["summary"]
    dt.assert_same(t, raw_get(dd, sm), "device form, host getters")
    p = dd.consensus_result_device()
    tot = sm["total_bytes"]
    got = dict(out_off=device_view(p["out_off"], 5, "<i8", U64), bases=device_view(p["bases"], tot, "|u1", np.uint8),
               quals=device_view(p["quals"], tot, "|u1", np.uint8), depth=device_view(p["depth"], 4, "<i4", np.uint32),
               errors=device_view(p["errors"], 4, "<i8", U64), summary=sm)
    dt.assert_same(t, got, "device form, device getter", keys=("out_off", "bases", "quals", "depth", "errors"))
    assert np.array_equal(ten[0].cpu().numpy(), l1[0]) and np.array_equal(ten[8].cpu().numpy(), strand)     # inputs untouched
    # the Python wrapper: flat blobs with off, and u8[N, L] matrices
    dt.assert_same(t, dd.duplex_consensus(l1[0], l1[1], l2[0], l2[1], cid, keep, strand, off_same=l1[2], off_other=l2[2]), "wrapper")
    m1, m2 = dt.duplex_reads(rng, cid, strand, keep, np.full(n, 70), np.full(n, 33), p_err=0.1)
    got = dd.duplex_consensus(m1[0].reshape(n, 70), m1[1].reshape(n, 70), m2[0].reshape(n, 33), m2[1].reshape(n, 33), cid, keep,
                              strand, strand_cap_q=30, cap_q=50)
    dt.assert_same(truth(m1, m2, cid, keep, strand, 4, loop=False, strand_cap_q=30, cap_q=50), got, "wrapper, matrices")
    assert set(got) == set(dt.ARRAYS) | {"summary"} and tuple(got["summary"]) == dt.KEYS


def test_getter_nulls(dd):
    rng = np.random.default_rng(19)
    cid, keep, strand = dt.sized_clusters(rng, [4, 1, 9], [2, 0, 8])
    n = len(cid)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.integers(1, 80, n), rng.integers(1, 80, n), p_err=0.2)
    t = check(dd, l1, l2, cid, keep, strand, 3)
    lib, h = dd._lib, dd._h
    assert lib.humid_get_duplex_consensus(h, None, None, None, None) == 0
    for k, name in enumerate(("depth_same", "depth_other", "disagree")):
        a = np.full(3 + 2, G32, np.uint32)
        args = [None, None, None, None]
        args[k] = vp(a)
        assert lib.humid_get_duplex_consensus(h, *args) == 0
        assert np.array_equal(a[:3], t[name]) and np.all(a[3:] == G32)
    sm = _lib.HumidDuplexSummary()
    assert lib.humid_get_duplex_consensus(h, None, None, None, C.byref(sm)) == 0 and sm.asdict() == t["summary"]
    assert lib.humid_get_duplex_consensus(None, None, None, None, None) == E_INVALID
    rc = lib.humid_duplex_consensus(h, vp(l1[0]), vp(l1[1]), vp(l1[2]), len(l1[0]), vp(l2[0]), vp(l2[1]), vp(l2[2]), len(l2[0]), vp(cid),
                                    vp(keep), vp(strand), n, 3, 10, 40, 93, None)
    assert rc == 0                                                     # (summary may be NULL)
    dt.assert_same(t, raw_get(dd, t["summary"]), "summary NULL")


def test_empty_inputs(dd):
    e8, e32 = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    empty = (e8, e8, np.zeros(1, U64))
    rc, sm = raw_call(dd, empty, empty, e32, e8, e8, 0)
    assert rc == 0 and sm == dict.fromkeys(dt.KEYS, 0)
    got = raw_get(dd, sm)
    assert list(got["out_off"]) == [0] and len(got["bases"]) == 0 and len(got["depth_same"]) == 0
    # C == 0 with reads: an empty result as well
    one = (np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"IIII", np.uint8), np.asarray([0, 4], U64))
    rc, sm = raw_call(dd, one, one, np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.full(1, 2, np.uint8), 0)
    assert rc == 0 and sm == dict.fromkeys(dt.KEYS, 0) and list(raw_get(dd, sm)["out_off"]) == [0]
    args = [None, None, None, 0] * 2 + [None, None, None, 0, 5, 10, 40, 93, None]
    assert dd._lib.humid_duplex_consensus(dd._h, *args) == 0           # no reads, NULLs
    # both layers empty while there are reads: every consensus has length 0
    cid, keep, strand = np.asarray([1, 1, 2], np.uint32), np.asarray([1, 0, 1], np.uint8), np.asarray([0, 1, 1], np.uint8)
    nothing = (e8, e8, np.zeros(4, U64))
    t = check(dd, nothing, nothing, cid, keep, strand, 2)
    assert t["summary"]["total_bytes"] == 0 and list(t["depth_other"]) == [1, 0]


def test_every_refusal_leaves_the_context_usable():
    d = humid_amd.Dedup()
    try:
        lib, h = d._lib, d._h
        assert lib.humid_get_duplex_consensus(h, None, None, None, None) == E_STATE       # before any call
        words, filt = pt.families(31, 24, 3000)
        cid, keep, s = d.run_paired(words, filt, word_nt=24)
        strand, top, bottom, ssum = d.strands()
        leaves = d.leaves()
        Cn = s["clusters"]
        rng = np.random.default_rng(31)
        n = len(cid)
        l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.integers(0, 90, n), rng.integers(0, 90, n), p_err=0.1)
        good = truth(l1, l2, cid, keep, strand, Cn, loop=False)
        assert good["summary"]["duplex_clusters"] == ssum["duplex"] > 0
        member = np.flatnonzero(cid != 0)
        multi = np.flatnonzero((np.bincount(cid)[cid] >= 2) & (cid != 0))

        def refused(code=E_INVALID, text=None, **kw):
            a = dict(ls=l1, lo=l2, cid=cid, keep=keep, strand=strand, C_=Cn)
            a.update(kw)
            rc, _ = raw_call(d, **a)
            assert rc == code, (rc, lib.humid_last_error(h))
            assert text is None or text in lib.humid_last_error(h), lib.humid_last_error(h)
            # a refused call leaves no result behind, the run's accessors intact and the context usable
            assert lib.humid_get_duplex_consensus(h, None, None, None, None) == E_STATE
            assert lib.humid_get_consensus(h, 0, None, None, None, None, None) == E_STATE
            lv = d.leaves()
            assert all(np.array_equal(lv[k], leaves[k]) for k in leaves)
            st2 = d.strands()
            assert np.array_equal(st2[0], strand) and np.array_equal(st2[1], top) and st2[3] == ssum
            dt.assert_same(good, raw_duplex(d, l1, l2, cid, keep, strand, Cn), "after a refusal")

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
        for which in ("ls", "lo"):                                      # off decreasing, off[n] beyond the bytes: either layer
            b, q, off = l1 if which == "ls" else l2
            bad = off.copy()
            i = int(np.flatnonzero(np.diff(off.astype(np.int64)) > 0)[10])
            bad[i + 1] = bad[i] - U64(1) if bad[i] else bad[i + 2] + U64(1)
            refused(text=b"decreases", **{which: (b, q, bad)})
            bad = off.copy()
            bad[-1] += U64(1 << 40)
            refused(text=b"beyond", **{which: (b, q, bad)})
        refused(n_bytes_s=len(l1[0]) - 1, text=b"beyond")
        refused(n_bytes_o=len(l2[0]) - 1, text=b"beyond")
        for v in (2, 3, 255):                                           # a member with a strand above 1
            bad = strand.copy()
            bad[member[7]] = v
            refused(strand=bad, text=b"strand")
        refused(C_=n + 1)                                               # more clusters than reads
        for kw in (dict(min_q=94), dict(strand_cap_q=0), dict(strand_cap_q=94), dict(cap_q=0), dict(cap_q=94)):
            refused(**kw)                                               # parameters out of range
        args = [vp(l1[0]), vp(l1[1]), vp(l1[2]), len(l1[0]), vp(l2[0]), vp(l2[1]), vp(l2[2]), len(l2[0]), vp(cid), vp(keep), vp(strand),
                n, Cn, 10, 40, 93, None]
        for k in (0, 1, 2, 4, 5, 6, 8, 9, 10):                          # a NULL buffer
            a = list(args)
            a[k] = None
            assert lib.humid_duplex_consensus(h, *a) == E_INVALID
        assert lib.humid_duplex_consensus(h, *args) == 0
        # the results survive a later run, and that run is unharmed
        got = raw_duplex(d, l1, l2, cid, keep, strand, Cn)
        w2, f2 = pt.families(32, 24, 2000)
        t2 = pt.run(w2, f2, 24, 1)
        c2, k2, s2 = d.run_paired(w2, f2, word_nt=24)
        assert np.array_equal(c2, t2["cluster_id"]) and np.array_equal(k2, t2["keep"])
        dt.assert_same(good, raw_get(d, got["summary"]), "after a later run")
    finally:
        d.close()
