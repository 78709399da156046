"""-m gpu: optical duplicates per cluster (humid_optical_duplicates*, kernels_optical.hip.h) against the two truths of
tests/optical_truth.py, bit for bit -- optical, origin, per_cluster and the summary -- through the host entry point
(guard words behind every output) and through the device entry point (torch tensors): read counts around the wave
and workgroup sizes, cluster counts around the radix sort's digit, the distance thresholds and the wrap case, chains
and a grid, the three kinds of origin, the boundary between the lane's walk and the wave's under option
"optical_walk", a random input of 2 x 10^5 reads with a heavy tail, the pass after real runs and after select_best,
and every refusal."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import humid_amd
from humid_amd.synth import synth_words

import optical_truth as ot

pytestmark = pytest.mark.gpu

NT, NR = ot.NO_TILE, ot.NO_READ
E_INVALID, E_OVERFLOW = -1, -5


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def raw_host(d, cid, keep, tile, x, y, D, n_cl, rc_only=False):
    """humid_optical_duplicates through the C ABI with guard words behind every output buffer"""
    n = len(cid)
    ins = [np.ascontiguousarray(cid, np.uint32), np.ascontiguousarray(keep, np.uint8)] + \
          [np.ascontiguousarray(np.asarray(a).astype(np.uint64), np.uint32) for a in (tile, x, y)]
    opt = np.full(n + 16, 0xA5, np.uint8)
    org = np.full(n + 8, 0xA5A5A5A5, np.uint32)
    pc = np.full(n_cl + 8, 0xA5A5A5A5, np.uint32)
    sm = humid_amd._lib.HumidOpticalSummary()
    rc = d._lib.humid_optical_duplicates(d._h, *[vp(a) for a in ins], n, n_cl, int(D), vp(opt), vp(org), vp(pc), C.byref(sm))
    assert np.all(opt[n:] == 0xA5) and np.all(org[n:] == 0xA5A5A5A5) and np.all(pc[n_cl:] == 0xA5A5A5A5)
    if rc_only:
        return rc, opt[:n], org[:n], pc[:n_cl], sm.asdict()
    d._check(rc)
    return opt[:n].copy(), org[:n].copy(), pc[:n_cl].copy(), sm.asdict()


def on_device(d, cid, keep, tile, x, y, D, n_cl):
    """Dedup.optical_duplicates on torch tensors (the _device entry point); results back as numpy"""
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(cid, np.uint32).view(np.int32)).to(dev),
         torch.from_numpy(np.ascontiguousarray(keep, np.uint8)).to(dev)] + \
        [torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint64), np.uint32).view(np.int32)).to(dev) for a in (tile, x, y)]
    opt, org, pc, s = d.optical_duplicates(*t, distance=D, n_clusters=n_cl)
    assert opt.is_cuda and org.is_cuda and pc.is_cuda
    return opt.cpu().numpy(), org.cpu().numpy().view(np.uint32), pc.cpu().numpy().view(np.uint32), s


def check(d, cid, keep, tile, x, y, D, n_cl, t=None, what=""):
    """host and device entry point against the truth; returns the truth"""
    if t is None:
        t = ot.truth(cid, keep, tile, x, y, D, n_cl)
    ot.assert_same(raw_host(d, cid, keep, tile, x, y, D, n_cl), t, (what, "host"))
    ot.assert_same(on_device(d, cid, keep, tile, x, y, D, n_cl), t, (what, "device"))
    return t


def clustered(seed, n, n_cl, p_zero=0.1):
    """n reads over n_cl clusters (every cluster has a read), a share without a cluster, one kept read per cluster"""
    rng = np.random.default_rng(seed)
    cid = np.where(rng.random(n) < p_zero, 0, rng.integers(1, n_cl + 1, n)).astype(np.uint32)
    cid[rng.permutation(n)[:n_cl]] = np.arange(1, n_cl + 1)
    order = rng.permutation(n)
    first = np.unique(cid[order], return_index=True)
    keep = np.zeros(n, np.uint8)
    keep[order[first[1]]] = 1
    keep[cid == 0] = rng.integers(0, 2, int((cid == 0).sum()))        # (never read)
    return cid, keep


def one_cluster(d, x, y, D, tile=None, keep_at=0, what=""):
    n = len(x)
    keep = np.zeros(n, np.uint8)
    keep[keep_at] = 1
    return check(d, np.ones(n, np.uint32), keep, np.full(n, 7) if tile is None else tile, x, y, D, 1, what=what)


# ---- 1. sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257])
def test_read_counts(dd, n):
    n_cl = min(n, 5)
    cid, keep = clustered(n, n, n_cl) if n else (np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    tile, x, y = ot.make_positions(cid, keep, n + 1, D=50, n_tiles=2, side=400, p_near=0.4, p_none=0.05)
    t = check(dd, cid, keep, tile, x, y, 50, n_cl)
    if n >= 63:
        assert t[3]["optical"] > 0


@pytest.mark.parametrize("n_cl", [255, 256, 257])
def test_cluster_counts_around_a_sort_digit(dd, n_cl):
    cid, keep = clustered(n_cl, 3000, n_cl)
    tile, x, y = ot.make_positions(cid, keep, n_cl + 1, D=50, n_tiles=2, side=300, p_near=0.4)
    t = check(dd, cid, keep, tile, x, y, 50, n_cl)
    assert t[3]["optical"] > 0 and np.count_nonzero(t[2]) > 100


# ---- 2. thresholds ---------------------------------------------------------------------------------------------------
def test_thresholds(dd):
    D = 10
    u = np.array
    for dx, dy, close in ((D, 0, 1), (D + 1, 0, 0), (0, D, 1), (0, D + 1, 0), (D, D, 1), (D + 1, D + 1, 0)):
        for flip in (False, True):                                       # either read may be the one further along
            xs, ys = u([100, 100 + dx]), u([50, 50 + dy])
            t = one_cluster(dd, xs[::-1] if flip else xs, ys[::-1] if flip else ys, D, what=(dx, dy))
            assert t[0].tolist() == [0, close]
    assert one_cluster(dd, u([5, 5, 6]), u([9, 9, 9]), 0)[0].tolist() == [0, 1, 0]
    assert one_cluster(dd, u([0, 0xffffffff, 7]), u([0xffffffff, 0, 7]), 0xffffffff)[0].tolist() == [0, 1, 1]
    t = one_cluster(dd, u([0, 0xffffffff, 0xfffffff0, 3]), u([0, 0xffffffff, 0xfffffff8, 0xffffffff]), 16, what="wrap")
    assert t[0].tolist() == [0, 0, 1, 0] and t[1].tolist() == [0, 1, 1, 3]
    t31 = np.full(3, 0x80000001, np.uint32)
    assert one_cluster(dd, u([0x80000000, 0x80000005, 0x7ffffffb]), u([1, 1, 1]), 5, tile=t31)[0].tolist() == [0, 1, 1]
    assert one_cluster(dd, u([4, 4]), u([4, 4]), 50, tile=u([7, 8]))[0].tolist() == [0, 0]
    assert one_cluster(dd, u([4, 4]), u([4, 4]), 50, tile=u([0x80000007, 7]))[0].tolist() == [0, 0]
    t = check(dd, u([1, 2], np.uint32), u([1, 1], np.uint8), u([7, 7]), u([4, 4]), u([4, 4]), 50, 2)
    assert t[0].tolist() == [0, 0] and t[3]["largest_group"] == 1
    t = one_cluster(dd, u([4, 4]), u([4, 4]), 50, tile=u([NT, NT]))
    assert t[0].tolist() == [0, 0] and t[1].tolist() == [0, 1]
    t = check(dd, u([0, 1, 0, 1], np.uint32), u([1, 1, 1, 0], np.uint8), u([7] * 4), u([4] * 4), u([4] * 4), 50, 1)
    assert t[0].tolist() == [0, 0, 0, 1] and t[1].tolist() == [NR, 1, NR, 1] and t[3]["members"] == 2


# ---- 3. transitivity -------------------------------------------------------------------------------------------------
def test_chains_and_a_grid(dd):
    D = 25
    x = np.arange(1000) * D
    perm = np.random.default_rng(1).permutation(1000)
    t = one_cluster(dd, x[perm], np.zeros(1000, np.int64), D, keep_at=5)
    assert t[3]["groups"] == 1 and t[3]["largest_group"] == 1000 and np.all(t[1] == 5)
    x[500:] += 1
    t = one_cluster(dd, x[perm], np.zeros(1000, np.int64), D, keep_at=5)
    assert t[3]["groups"] == 2 and t[3]["largest_group"] == 500 and t[3]["optical"] == 998
    gx, gy = np.meshgrid(np.arange(40) * D, np.arange(40) * D)
    perm = np.random.default_rng(3).permutation(1600)
    t = one_cluster(dd, gx.ravel()[perm], gy.ravel()[perm], D, keep_at=77)
    assert t[3]["groups"] == 1 and t[3]["largest_group"] == 1600 and np.all(t[1] == 77)


# ---- 4. origin -------------------------------------------------------------------------------------------------------
def test_origins(dd):
    cid = np.array([1, 1, 1, 1, 1, 2, 2, 2], np.uint32)
    keep = np.array([0, 0, 1, 0, 0, 1, 0, 0], np.uint8)
    x = np.array([10, 12, 14, 900, 905, 10, 500, 501])
    t = check(dd, cid, keep, np.full(8, 3), x, x, 8, 2)
    assert t[1].tolist() == [2, 2, 2, 3, 3, 5, 6, 6] and t[0].tolist() == [1, 1, 0, 0, 1, 0, 0, 1] and t[2].tolist() == [3, 1]
    assert t[3] == dict(n_clusters=2, members=8, duplicates=6, optical=4, groups=3, largest_group=3)


# ---- 5. the walk boundary --------------------------------------------------------------------------------------------
@pytest.fixture()
def walk(dd):
    yield lambda w: dd.set_option("optical_walk", w)
    dd.set_option("optical_walk", 64)


def test_windows_around_the_walk_bound(dd, walk):
    W = 8
    walk(W)
    for m in (W - 1, W, W + 1, W + 2, 64 + W, 64 + W + 1, 2 * 64 + W + 1):
        # the first read's window holds exactly m reads: m + 1 reads on one x (equal keys keep their input order), of
        # which only the LAST is close to the first in y, and three reads beyond the window
        x = np.r_[np.zeros(m + 1, np.int64), 500 + np.arange(3)]
        y = np.r_[0, np.full(m - 1, 1000), 3, 0, 1000, 0]
        t = one_cluster(dd, x, y, 100, what=("window", m))
        assert t[1][m] == 0 and t[0][m] == 1                          # found across the whole window
    with pytest.raises(humid_amd.HumidError):
        walk(-1)


def test_a_long_window_under_three_walk_bounds(dd, walk):
    n, D = 5000, 100
    rng = np.random.default_rng(8)
    x = rng.integers(0, D + 1, n)                                      # all x within D
    y = np.where(np.arange(n) % 2 == 0, rng.integers(0, 60, n), rng.integers(5000, 5060, n))   # two bands
    cid, keep = np.ones(n, np.uint32), np.zeros(n, np.uint8)
    keep[1234] = 1
    tile = np.full(n, 9)
    t = ot.truth(cid, keep, tile, x, y, D, 1, loop=False)
    assert t[3]["groups"] == 2 and t[3]["largest_group"] == 2500 and t[3]["optical"] == n - 2
    t0 = time.time()
    outs = []
    for w in (8, 64, 0):
        walk(w)
        outs.append(raw_host(dd, cid, keep, tile, x, y, D, 1))
        ot.assert_same(outs[-1], t, ("walk", w))
    ot.assert_same(on_device(dd, cid, keep, tile, x, y, D, 1), t, "device")
    assert time.time() - t0 < 10


# ---- 6. random differential ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def heavy():
    """about 2 x 10^5 reads: cluster sizes from a Zipf law (cut at 3000), one cluster of 20 000 reads, 8 tiles"""
    rng = np.random.default_rng(42)
    sizes = [20_000]
    while sum(sizes) < 195_000:
        sizes.append(int(min(rng.zipf(1.6), 3000)))
    n_cl = len(sizes)
    cid = np.repeat(np.arange(1, n_cl + 1, dtype=np.uint32), sizes)
    cid = np.r_[cid, np.zeros(5000, np.uint32)]
    cid = cid[rng.permutation(len(cid))]
    order = rng.permutation(len(cid))
    first = np.unique(cid[order], return_index=True)
    keep = np.zeros(len(cid), np.uint8)
    keep[order[first[1]][first[0] != 0]] = 1
    tile, x, y = ot.make_positions(cid, keep, 43, D=100, n_tiles=8, side=20000, p_near=0.4, p_none=0.01)
    sizes = np.bincount(cid)
    small = np.flatnonzero((sizes <= 400) & (np.arange(len(sizes)) > 0))[:400]   # the loop truth: a subset of whole clusters
    sub = np.flatnonzero(np.isin(cid, small))
    t = ot.truth(cid, keep, tile, x, y, 100, n_cl, loop=False)
    return dict(cid=cid, keep=keep, tile=tile, x=x, y=y, n_cl=n_cl, truth=t, sub=sub, small=small)


def test_random_heavy_tailed_input(dd, heavy):
    h = heavy
    s = h["truth"][3]
    assert len(h["cid"]) >= 195_000 and int(np.bincount(h["cid"])[1:].max()) >= 20_000
    assert 0.2 * s["duplicates"] <= s["optical"] <= 0.5 * s["duplicates"], s   # the case cannot degenerate
    # the loop truth on a subset of whole clusters (400 of at most 400 reads, renumbered 1 ..): the two truths and the device
    sub = h["sub"]
    cs = (np.searchsorted(h["small"], h["cid"][sub]) + 1).astype(np.uint32)
    args = (cs, h["keep"][sub], h["tile"][sub], h["x"][sub], h["y"][sub], 100, len(h["small"]))
    check(dd, *args, t=ot.truth(*args, loop=True), what="subset")
    a = raw_host(dd, h["cid"], h["keep"], h["tile"], h["x"], h["y"], 100, h["n_cl"])
    ot.assert_same(a, h["truth"], "host")
    b = raw_host(dd, h["cid"], h["keep"], h["tile"], h["x"], h["y"], 100, h["n_cl"])
    ot.assert_same(a, b, "the same input twice")
    ot.assert_same(on_device(dd, h["cid"], h["keep"], h["tile"], h["x"], h["y"], 100, h["n_cl"]), h["truth"], "device")


# ---- 7. after a real run ---------------------------------------------------------------------------------------------
def test_after_a_run_and_after_select_best(dd):
    words, filt = synth_words(30_000, 77, 24, p_sub=4e-3)
    cid, keep, s = dd.run(words, filt, 24, 1)
    leaves, clusters = dd.leaves(), dd.clusters()
    tile, x, y = ot.make_positions(cid, keep, 78, D=100, n_tiles=4, side=5000)
    got = dd.optical_duplicates(cid, keep, tile, x, y, distance=100)             # n_clusters: the run's
    t = ot.truth(cid, keep, tile, x, y, 100, s["clusters"])
    ot.assert_same(got, t, "after a run")
    assert t[3]["optical"] > 0 and got[3]["n_clusters"] == s["clusters"]
    for a, b in ((dd.leaves(), leaves), (dd.clusters(), clusters)):            # the run's accessors still answer
        for k in b:
            assert np.array_equal(a[k], b[k]), k
    scores = np.random.default_rng(79).integers(0, 50, len(cid)).astype(np.uint32)
    keep2, rep, changed = dd.select_best(words, cid, keep, scores, 24)
    assert changed > 0
    got2 = dd.optical_duplicates(cid, keep2, tile, x, y, distance=100)
    t2 = ot.truth(cid, keep2, tile, x, y, 100, s["clusters"])
    ot.assert_same(got2, t2, "after select_best")
    assert not np.array_equal(t2[1], t[1]) and np.all(t2[0][keep2 != 0] == 0)    # the origins follow the new keep


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_malformed_input_is_refused_and_nothing_written(dd):
    cid, keep = clustered(5, 500, 7)
    tile, x, y = ot.make_positions(cid, keep, 6, D=50, n_tiles=2, side=300)
    good = ot.truth(cid, keep, tile, x, y, 50, 7)

    def refused(c, k, n_cl, text):
        rc, opt, org, pc, sm = raw_host(dd, c, k, tile, x, y, 50, n_cl, rc_only=True)
        assert rc == E_INVALID and text in dd._lib.humid_last_error(dd._h).decode(), dd._lib.humid_last_error(dd._h)
        assert np.all(opt == 0xA5) and np.all(org == 0xA5A5A5A5) and np.all(pc == 0xA5A5A5A5)
        assert all(v == 0 for v in sm.values())
        dev = torch.device("cuda:0")
        tt = [torch.from_numpy(a).to(dev) for a in (c.view(np.int32), k, tile.view(np.int32), x.view(np.int32), y.view(np.int32))]
        o8 = torch.full((len(c),), 0x5A, dtype=torch.uint8, device=dev)
        o32 = torch.full((len(c),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        p32 = torch.full((n_cl,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        rc = dd._lib.humid_optical_duplicates_device(dd._h, *[C.c_void_p(a.data_ptr()) for a in tt], len(c), n_cl, 50,
                                                     C.c_void_p(o8.data_ptr()), C.c_void_p(o32.data_ptr()),
                                                     C.c_void_p(p32.data_ptr()), None)
        assert rc == E_INVALID
        assert bool((o8 == 0x5A).all()) and bool((o32 == 0x5A5A5A5A).all()) and bool((p32 == 0x5A5A5A5A).all())
        ot.assert_same(raw_host(dd, cid, keep, tile, x, y, 50, 7), good, "the context runs again")

    bad = cid.copy()
    bad[np.flatnonzero((cid == 3) & (keep == 0))[0]] = 8                # an id C + 1
    refused(bad, keep, 7, "above")
    k0 = keep.copy()
    k0[(cid == 4) & (keep != 0)] = 0                                    # a cluster with no kept read
    refused(cid, k0, 7, "keep == 1")
    k2 = keep.copy()
    k2[np.flatnonzero((cid == 2) & (keep == 0))[0]] = 1                 # a cluster with two
    refused(cid, k2, 7, "more than one")
    refused(cid, keep, 501, "keep == 1")                                # more clusters than reads


def test_host_side_refusals_and_empty_calls(dd):
    lib, h = dd._lib, dd._h
    a4, a1 = np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    sm = humid_amd._lib.HumidOpticalSummary()
    ins = [vp(a4), vp(a1), vp(a4), vp(a4), vp(a4)]
    for k in range(5):                                                  # a NULL required buffer
        bad = list(ins)
        bad[k] = None
        assert lib.humid_optical_duplicates(h, *bad, 4, 1, 5, vp(a1), None, None, None) == E_INVALID
        assert lib.humid_optical_duplicates_device(h, *bad, 4, 1, 5, vp(a1), None, None, None) == E_INVALID
    assert lib.humid_optical_duplicates(h, *ins, 4, 1, 5, None, None, None, None) == E_INVALID
    assert lib.humid_optical_duplicates(None, *ins, 4, 1, 5, vp(a1), None, None, None) == E_INVALID
    assert lib.humid_optical_duplicates(h, *ins, 1 << 31, 1, 5, vp(a1), None, None, C.byref(sm)) == E_OVERFLOW
    assert lib.humid_optical_duplicates_device(h, *ins, 1 << 31, 1, 5, vp(a1), None, None, None) == E_OVERFLOW
    assert lib.humid_optical_duplicates(h, None, None, None, None, None, 0, 3, 5, None, None, None, C.byref(sm)) == 0
    assert all(v == 0 for v in sm.asdict().values())
    # C == 0: every read counts as no member
    opt, org, pc, s = raw_host(dd, a4, np.ones(4, np.uint8), a4, a4, a4, 5, 0)
    assert opt.tolist() == [0] * 4 and org.tolist() == [NR] * 4 and all(v == 0 for v in s.values())
    # origin and per_cluster may be NULL
    cid, keep = clustered(9, 300, 4)
    tile, x, y = ot.make_positions(cid, keep, 10, D=50, n_tiles=2, side=300)
    t = ot.truth(cid, keep, tile, x, y, 50, 4)
    opt = np.zeros(300, np.uint8)
    assert lib.humid_optical_duplicates(h, vp(cid), vp(keep), vp(tile), vp(x), vp(y), 300, 4, 50, vp(opt), None, None, C.byref(sm)) == 0
    assert np.array_equal(opt, t[0]) and sm.asdict() == t[3]
    # a context that never ran anything: the pass needs no run, and n_clusters=None has nothing to take
    d2 = humid_amd.Dedup()
    try:
        ot.assert_same(d2.optical_duplicates(cid, keep, tile, x, y, distance=50, n_clusters=4), t, "fresh context")
        assert d2._lib.humid_get_leaves(d2._h, None, None, None, None, None, None) == -6    # HUMID_E_STATE: still no run
    finally:
        d2.close()
