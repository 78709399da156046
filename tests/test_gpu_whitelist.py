"""-m gpu: barcode whitelist correction (humid_whitelist_*, humid_dedup_run_keyed_corrected) against the truths of
tests/whitelist_truth.py, bit for bit: key_out, status and counts of the standalone correction in both forms of its
kernel; the corrected keyed run against the per-group truth on truth-corrected keys and against run_keyed on the same
precorrected inputs; the state rules of the context."""
import ctypes as C

import numpy as np
import pytest

import humid_amd

import grouped_truth as gt
import whitelist_truth as wt
from test_gpu_keyed import make_words, ranks_of

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP = wt.TOP
E_STATE, E_INVALID = -6, -1
ALL_STATUSES = {0, 1, 2, 3, 4}


@pytest.fixture(scope="module", params=[1, 0], ids=["wave_cooperative", "lane_serial"])
def dd(request):
    """the two forms of the correction kernel (option "whitelist_coop")"""
    d = humid_amd.Dedup()
    d.set_option("whitelist_coop", request.param)
    yield d
    d.close()


@pytest.fixture(scope="module")
def plain():
    d = humid_amd.Dedup()
    yield d
    d.close()


def raw_correct(d, keys, filt):
    """humid_whitelist_correct through the C ABI with guard words behind every output buffer"""
    keys = np.ascontiguousarray(keys, U64)
    filt = np.ascontiguousarray(filt, np.uint8)
    n = len(filt)
    out = np.full(n + 8, 0xA5A5A5A5A5A5A5A5, U64)
    status = np.full(n + 16, 0xA5, np.uint8)
    counts = np.full(5 + 3, 0xA5A5A5A5A5A5A5A5, U64)
    vp = lambda a: C.c_void_p(a.ctypes.data)                        # noqa: E731
    d._check(d._lib.humid_whitelist_correct(d._h, vp(keys), vp(filt), n, vp(out), vp(status), vp(counts)))
    assert np.all(out[n:] == U64(0xA5A5A5A5A5A5A5A5)) and np.all(status[n:] == 0xA5)
    assert np.all(counts[5:] == U64(0xA5A5A5A5A5A5A5A5))
    return out[:n], status[:n], counts[:5]


def check(d, keys, filt, wl, k, expect=None):
    """the device against the truth; expect: the statuses the TRUTH must contain (the input exercises them)"""
    t = wt.correct_np(keys, filt, wl, k)
    if expect is not None:
        assert wt.status_set(t[1]) >= set(expect), (wt.status_set(t[1]), expect)
    got = raw_correct(d, keys, filt)
    for name, a, b in zip(("key_out", "status", "counts"), t, got):
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    return t


def set_wl(d, wl, k):
    d.set_whitelist(wl, k)
    info = d.whitelist_info()
    n = len(wl)
    assert info["n_distinct"] == len(np.unique(wl)) and info["barcode_nt"] == k
    assert (1 << info["table_log2"]) >= 2 * n and ((1 << info["table_log2"]) < 4 * n or info["table_log2"] == 1)


@pytest.mark.parametrize("k", [1, 2, 3, 16, 21, 22, 31, 32])
def test_barcode_lengths_whitelist_sizes_read_counts(dd, k):
    """21 and 22 nt are 63 and 66 variants: the wave boundary of the variant rounds.  The truth holds every status
    wherever the shape allows it"""
    rng = np.random.default_rng(100 + k)
    full = 4 ** k if k <= 3 else None
    sizes = [1, 2, 1000] + ([full, {1: 1, 2: 2, 3: 5}[k]] if full else [100_000])
    for n_wl in sizes:
        wl = np.arange(full, dtype=U64) if n_wl == full else wt.whitelist_with_neighbours(rng, n_wl, k)
        if k == 2 and n_wl == 2:
            wl = np.asarray([0b0000, 0b0101], U64)                  # {AA, CC}: AC and CA are ambiguous
        if k == 32 and n_wl >= 1000:
            wl[5] = TOP                                             # the all-T barcode: the table's empty mark
            wl[6] = TOP ^ U64(2 << 10)
        set_wl(dd, wl, k)
        for n in (0, 1, 63, 64, 65, 257, 100_000):
            keys, filt = wt.make_keys(rng, wl, k, n)
            if k == 32 and n >= 257:
                keys[3] = TOP                                       # as a read's key: exact with wl[5], else looked up
                keys[4] = TOP ^ U64(1)
                filt[3:5] = 0
            expect = None
            if n == 100_000:
                if k >= 16:
                    expect = ALL_STATUSES if n_wl >= 1000 else {0, 1, 2, 4}
                elif (k, n_wl) in ((3, 5), (2, 2)):
                    expect = ALL_STATUSES
                elif n_wl == full:
                    expect = {0, 1}
                elif (k, n_wl) == (1, 1):
                    expect = {0, 1, 2}
            check(dd, keys, filt, wl, k, expect)
    if k == 32:                                                     # all-T absent: its neighbours still find it absent
        wl = wt.whitelist_with_neighbours(rng, 1000, k)
        wl = wl[wl != TOP]
        set_wl(dd, wl, k)
        keys = np.asarray([TOP, TOP ^ U64(1), TOP ^ U64(3 << 62), wl[0]], U64)
        t = check(dd, keys, np.zeros(4, np.uint8), wl, k)
        assert list(t[1]) == [4, 4, 4, 1]
        wl2 = np.concatenate([wl, [TOP]]).astype(U64)
        set_wl(dd, wl2, k)
        t = check(dd, keys, np.zeros(4, np.uint8), wl2, k)
        assert list(t[1]) == [1, 2, 2, 1] and int(t[0][1]) == TOP and int(t[0][2]) == TOP


def test_hand_cases(dd):
    enc = lambda s: sum("ACGT".index(ch) << (2 * (len(s) - 1 - i)) for i, ch in enumerate(s))    # noqa: E731
    dd.set_whitelist([enc("AA"), enc("CC")], 2)
    keys = np.asarray([enc(s) for s in ("AC", "CA", "AG", "GG", "AA", "CC", "TT")], U64)
    f = np.zeros(7, np.uint8)
    f[-1] = 1
    out, status, counts = raw_correct(dd, keys, f)
    assert list(status) == [3, 3, 2, 4, 1, 1, 0]
    assert list(out) == [enc("AC"), enc("CA"), enc("AA"), enc("GG"), enc("AA"), enc("CC"), 0]
    assert list(counts) == [1, 2, 1, 2, 1]
    dd.set_whitelist([enc("AA"), enc("AC")], 2)
    out, status, _ = raw_correct(dd, np.asarray([enc("AC")], U64), np.zeros(1, np.uint8))
    assert list(status) == [1] and list(out) == [enc("AC")]         # exact, not ambiguous


def test_duplicates_and_one_home_slot(dd):
    rng = np.random.default_rng(7)
    base = wt.whitelist_with_neighbours(rng, 300, 16)
    wl = np.concatenate([base, base[:100], base[:100], base[50:60]])
    rng.shuffle(wl)
    set_wl(dd, wl, 16)
    assert dd.whitelist_info()["n_distinct"] == len(np.unique(base))
    keys, filt = wt.make_keys(rng, base, 16, 20_000)
    check(dd, keys, filt, wl, 16, ALL_STATUSES)
    # barcodes whose hash starts with the same 40 bits: one home slot at every table size, one long probe chain
    same_home = np.asarray([wt.unmix64((0x5A5A5A5A5A << 24) | i) for i in range(150)], U64)
    same_home[1] = same_home[0] ^ U64(1 << 20)                      # (not of that home: a pair at distance 1)
    set_wl(dd, same_home, 32)
    keys, filt = wt.make_keys(rng, same_home, 32, 20_000, p1=0.2)
    check(dd, keys, filt, same_home, 32, {0, 1, 2, 4})


def test_runs_of_equal_keys_and_the_same_shuffled(dd):
    rng = np.random.default_rng(9)
    wl = wt.whitelist_with_neighbours(rng, 1000, 16)
    set_wl(dd, wl, 16)
    mids = wt.midpoints(wl, 16)
    assert len(mids)
    lengths = [1, 63, 64, 65, 10000, 1, 1, 64, 64, 63, 65, 10000, 1, 64]
    vals = wl[rng.integers(0, len(wl), size=len(lengths))]
    vals[1] = wt.substitute(rng, vals[1:2], 16)[0]                  # a run of a key to correct
    vals[4] = mids[0]                                               # a long ambiguous run
    vals[7] = vals[1]
    vals[11] = U64(rng.integers(0, 1 << 32))                        # a long run of a random key
    vals[13] = wt.substitute(rng, wt.substitute(rng, vals[13:14], 16), 16)[0]
    keys = np.concatenate([np.full(n, v, U64) for n, v in zip(lengths, vals)])
    filt = np.zeros(len(keys), np.uint8)
    check(dd, keys, filt, wl, 16, {1, 2, 3, 4})
    filt2 = filt.copy()
    filt2[::64] = 1                                                 # filtered reads at the head of every wave
    filt2[100:200] = 1
    check(dd, keys, filt2, wl, 16, ALL_STATUSES)
    order = rng.permutation(len(keys))
    check(dd, keys[order], filt2[order], wl, 16, ALL_STATUSES)


def test_wave_patterns(dd):
    rng = np.random.default_rng(11)
    for k in (16, 22):
        wl = wt.whitelist_with_neighbours(rng, 5000, k)
        set_wl(dd, wl, k)
        n = 64 * 50 + 17
        none = np.zeros(n, np.uint8)
        # every lane of every wave misses: random keys, and one substitution each (every lane is corrected)
        check(dd, wt.random_barcodes(rng, n, k), none, wl, k, {4})
        check(dd, wt.substitute(rng, wl[rng.integers(0, len(wl), size=n)], k), none, wl, k, {2})
        # exactly one lane of a wave misses: lane 0, lane 63
        for lane in (0, 63):
            keys = wl[rng.integers(0, len(wl), size=n)]
            at = np.arange(lane, n, 64)
            keys[at] = wt.substitute(rng, keys[at], k)
            keys[at[::3]] = wt.random_barcodes(rng, len(at[::3]), k)
            check(dd, keys, none, wl, k, {1, 2, 4})
        # around the number of missing lanes at which the cooperative kernel hands a wave to the lane-serial walk
        edge = 3 * k // ((3 * k + 63) // 64)
        for m in (edge - 1, edge, edge + 1):
            keys = wl[rng.integers(0, len(wl), size=n)]
            at = np.flatnonzero(np.arange(n) % 64 < m)
            keys[at] = wt.substitute(rng, keys[at], k)
            keys[at[::5]] = wt.random_barcodes(rng, len(at[::5]), k)
            check(dd, keys, none, wl, k, {1, 2, 4})
        # keys with bits above 2 K: unmatched, whatever lies below
        keys = wl[rng.integers(0, len(wl), size=n)]
        high = rng.random(n) < 0.3
        keys = np.where(high, keys | (U64(1) << U64(2 * k + rng.integers(0, 64 - 2 * k))), keys)
        t = check(dd, keys, none, wl, k, {1, 4})
        assert np.all(t[1][high] == 4)
        # filtered reads carry garbage; everything filtered
        keys, filt = wt.make_keys(rng, wl, k, n, p_filt=0.5)
        check(dd, keys, filt, wl, k, ALL_STATUSES)
        t = check(dd, keys, np.ones(n, np.uint8), wl, k, {0})
        assert int(t[2][0]) == n and not t[0].any()


def corrected_inputs(seed, n_reads, word_nt, k=16, n_wl=40):
    rng = np.random.default_rng(seed)
    wl = wt.whitelist_with_neighbours(rng, n_wl, k)
    words, filt = make_words(seed + 1, n_reads, word_nt)
    keys, kf = wt.make_keys(rng, wl, k, n_reads, p1=0.1, p2=0.04, pr=0.04, p_filt=0.0)
    garbage = rng.integers(0, 1 << 64, size=n_reads, dtype=U64)
    keys = np.where(filt == 1, garbage, keys)                       # filtered reads carry garbage keys
    return wl, words, keys, filt


def full_result(d, words, keys, filt, word_nt, distance, method, edit, correct):
    cid, keep, s = d.run_keyed(words, keys, filt, word_nt=word_nt, distance=distance, method=method, edit=edit, correct=correct)
    off, idx = d.adjacency()
    return dict(cid=cid, keep=keep, summary=s, leaves=d.leaves(), off=off, idx=idx, clusters=d.clusters(),
                hist=d.histograms(), K=d.group_keys(), stats=d.group_stats())


@pytest.mark.parametrize("word_nt", [12, 24, 40])
def test_corrected_run(plain, word_nt):
    """run_keyed(correct=True) == the per-group truth on truth-corrected keys and truth filtered', and == run_keyed
    on those precorrected inputs, array for array"""
    k = 16
    wl, words, keys, filt = corrected_inputs(word_nt, 3000, word_nt)
    plain.set_whitelist(wl, k)
    t_key, t_status, t_counts = wt.correct(keys, filt, wl, k)
    assert wt.status_set(t_status) == ALL_STATUSES
    filt2 = ((filt != 0) | (t_status >= 3)).astype(np.uint8)
    K, groups = ranks_of(t_key, filt2)
    other = humid_amd.Dedup()
    try:
        for distance, method, edit in ((0, 0, False), (1, 0, False), (1, 1, False), (2, 0, False), (2, 1, False), (2, 0, True)):
            t = gt.per_group(words, groups, filt2, word_nt, distance, method, edit=edit)
            got = full_result(plain, words, keys, filt, word_nt, distance, method, edit, True)
            gt.assert_same(t, got, first_read=True)
            status, counts = plain.barcode_status()
            assert np.array_equal(status, t_status) and np.array_equal(counts, t_counts) and counts.dtype == U64
            assert np.array_equal(got["K"], K) and np.all(np.isin(got["K"], wl))
            assert np.array_equal(got["leaves"]["key"], K[np.asarray(t["leaves"]["group"], np.int64)])
            st = got["stats"]
            assert int(st["reads"].sum()) == t["summary"]["usable"] == int(t_counts[1] + t_counts[2])
            assert int(st["clusters"].sum()) == t["summary"]["clusters"] and int(st["unique"].sum()) == t["summary"]["unique"]
            assert np.array_equal(st["key"], K)
            want = full_result(other, words, t_key, filt2, word_nt, distance, method, edit, False)
            gt.assert_same(want, got, first_read=True)
            assert np.array_equal(want["K"], got["K"])
            for name in ("reads", "unique", "clusters", "edges", "leaf_off", "cluster_off"):
                assert np.array_equal(want["stats"][name], st[name]), name
    finally:
        other.close()


def test_state_rules(plain):
    d = humid_amd.Dedup()
    try:
        wl, words, keys, filt = corrected_inputs(31, 2000, 24)
        # no whitelist: HUMID_E_STATE, and the context stays usable
        assert d.whitelist_info() == dict(n_distinct=0, barcode_nt=0, table_log2=0)
        for call in (lambda: d.correct_keys(keys, filt), lambda: d.run_keyed(words, keys, filt, correct=True)):
            with pytest.raises(humid_amd.HumidError) as ei:
                call()
            assert ei.value.code == E_STATE
        # barcode_status() after a plain or uncorrected keyed run
        d.run(words, filt, word_nt=24)
        with pytest.raises(humid_amd.HumidError) as ei:
            d.barcode_status()
        assert ei.value.code == E_STATE
        d.set_whitelist(wl, 16)
        d.run_keyed(words, keys, filt, word_nt=24)
        with pytest.raises(humid_amd.HumidError) as ei:
            d.barcode_status()
        assert ei.value.code == E_STATE
        # the whitelist survives plain, grouped and keyed runs
        t = wt.correct(keys, filt, wl, 16)
        K, groups = ranks_of(keys, filt)
        d.run(words, filt, word_nt=24)
        d.run_grouped(words, groups, filt, word_nt=24)
        d.run_keyed(words, keys, filt, word_nt=24)
        for a, b in zip(t, d.correct_keys(keys, filt)):
            assert np.array_equal(a, b)
        # correct_keys between a run and its accessors does not disturb them
        d.run_keyed(words, keys, filt, word_nt=24, correct=True)
        before = (d.leaves(), d.barcode_status(), d.group_keys())
        other_keys = wt.random_barcodes(np.random.default_rng(1), 777, 16)
        d.correct_keys(other_keys, np.zeros(777, np.uint8))
        after = (d.leaves(), d.barcode_status(), d.group_keys())
        for name in before[0]:
            assert np.array_equal(before[0][name], after[0][name]), name
        assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
        assert np.array_equal(before[1][0], t[1]) and np.array_equal(before[2], after[2])
        # a corrected run is a keyed run for the accessors, and a plain run after it is a plain one
        assert d.keyed_rank_info()["n_keys"] == len(after[2])
        d.run(words, filt, word_nt=24)
        with pytest.raises(humid_amd.HumidError):
            d.barcode_status()
        # a refused set leaves the old whitelist working
        for bad, nt in (([1 << 33], 16), (wl, 0), (wl, 33)):
            rc = d._lib.humid_whitelist_set(d._h, C.c_void_p(np.asarray(bad, U64).ctypes.data), len(bad), nt)
            assert rc == E_INVALID
        assert d.whitelist_info()["n_distinct"] == len(np.unique(wl))
        for a, b in zip(t, d.correct_keys(keys, filt)):
            assert np.array_equal(a, b)
        # replacing, clearing
        wl2 = wt.whitelist_with_neighbours(np.random.default_rng(2), 3000, 16)
        d.set_whitelist(wl2, 16)
        for a, b in zip(wt.correct_np(keys, filt, wl2, 16), d.correct_keys(keys, filt)):
            assert np.array_equal(a, b)
        d.set_whitelist(wl, 16)
        for a, b in zip(t, d.correct_keys(keys, filt)):
            assert np.array_equal(a, b)
        for clear in (None, np.zeros(0, U64)):
            d.set_whitelist(wl, 16)
            d.set_whitelist(clear)
            assert d.whitelist_info()["n_distinct"] == 0
            with pytest.raises(humid_amd.HumidError) as ei:
                d.correct_keys(keys, filt)
            assert ei.value.code == E_STATE
        # the default path of run_keyed is untouched by a whitelist on the context
        d.set_whitelist(wl, 16)
        a = d.run_keyed(words, keys, filt, word_nt=24)
        b = plain.run_keyed(words, keys, filt, word_nt=24)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        d.close()


def test_device_entry_points(plain):
    import torch
    wl, words, keys, filt = corrected_inputs(41, 30_000, 28, n_wl=500)
    plain.set_whitelist(wl, 16)
    t_key, t_status, t_counts = wt.correct_np(keys, filt, wl, 16)
    filt2 = ((filt != 0) | (t_status >= 3)).astype(np.uint8)
    K, groups = ranks_of(t_key, filt2)
    t = gt.repetition(words, groups, filt2, 28, 1, 0)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_k = torch.from_numpy(keys.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_ko = torch.zeros(len(filt), dtype=torch.int64, device=dev)
    d_st = torch.full((len(filt),), 9, dtype=torch.uint8, device=dev)
    d_cid = torch.zeros(len(filt), dtype=torch.int32, device=dev)
    d_keep = torch.zeros(len(filt), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    counts = plain.correct_keys_device(d_k.data_ptr(), d_f.data_ptr(), d_ko.data_ptr(), d_st.data_ptr(), len(filt))
    assert np.array_equal(counts, t_counts)
    assert np.array_equal(d_ko.cpu().numpy().view(U64), t_key) and np.array_equal(d_st.cpu().numpy(), t_status)
    assert np.array_equal(plain.correct_keys_device(d_k.data_ptr(), d_f.data_ptr(), 0, 0, len(filt)), t_counts)
    s = plain.run_keyed_corrected_device(d_w.data_ptr(), d_k.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(),
                                         len(filt), word_nt=28, distance=1)
    assert np.array_equal(d_cid.cpu().numpy().view(np.uint32), t["cid"])
    assert np.array_equal(d_keep.cpu().numpy(), t["keep"])
    assert s["clusters"] == t["summary"]["clusters"] and s["usable"] == int(t_counts[1] + t_counts[2])
    assert np.array_equal(d_k.cpu().numpy().view(U64), keys) and np.array_equal(d_f.cpu().numpy(), filt)   # inputs untouched
    assert np.array_equal(plain.group_keys(), K)
    status, counts = plain.barcode_status()
    assert np.array_equal(status, t_status) and np.array_equal(counts, t_counts)


def test_scale(plain):
    """10 M reads against a whitelist of 10^6 16-nt barcodes"""
    rng = np.random.default_rng(51)
    wl = wt.whitelist_with_neighbours(rng, 1_000_000, 16)
    keys, filt = wt.make_keys(rng, wl, 16, 10_000_000)
    plain.set_whitelist(wl, 16)
    check(plain, keys, filt, wl, 16, ALL_STATUSES)
