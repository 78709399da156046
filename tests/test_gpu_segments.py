"""-m gpu: segmented barcode whitelists (humid_whitelist_set_segments) against the truths of tests/segments_truth.py,
bit for bit: key_out, status, counts, seg_counts and inexact_hist of the standalone correction with host and device
pointers; the two identities with the plain correction kernels; the corrected keyed run; the state rules."""
import ctypes as C

import numpy as np
import pytest

import humid_amd

import segments_truth as sg
import whitelist_truth as wt
from test_gpu_keyed import make_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
E_INVALID, E_UNSUPPORTED, E_STATE = -1, -2, -6
GUARD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def raw_correct(d, keys, filt):
    """humid_whitelist_correct and humid_get_barcode_segments through the C ABI, guard words behind every output"""
    keys = np.ascontiguousarray(keys, U64)
    filt = np.ascontiguousarray(filt, np.uint8)
    n = len(filt)
    out = np.full(n + 8, GUARD, U64)
    status = np.full(n + 16, 0xA5, np.uint8)
    counts = np.full(5 + 3, GUARD, U64)
    sc, ih = np.full(32 + 2, GUARD, U64), np.full(9 + 2, GUARD, U64)
    vp = lambda a: C.c_void_p(a.ctypes.data)                        # noqa: E731
    d._check(d._lib.humid_whitelist_correct(d._h, vp(keys), vp(filt), n, vp(out), vp(status), vp(counts)))
    d._check(d._lib.humid_get_barcode_segments(d._h, vp(sc), vp(ih)))
    for a, m in ((out, n), (counts, 5), (sc, 32), (ih, 9)):
        assert np.all(a[m:] == U64(GUARD))
    assert np.all(status[n:] == 0xA5)
    S = d.whitelist_segments_info()["n_seg"]
    assert not sc[4 * S:32].any() and not ih[S + 1:9].any()         # rows behind the last segment are zero
    return out[:n], status[:n], counts[:5], sc[:4 * S].reshape(S, 4), ih[:S + 1]


def device_correct(d, keys, filt):
    import torch
    dev = torch.device("cuda:0")
    n = len(filt)
    d_k = torch.from_numpy(np.ascontiguousarray(keys, U64).view(np.int64)).to(dev)
    d_f = torch.from_numpy(np.ascontiguousarray(filt, np.uint8)).to(dev)
    d_o = torch.full((n + 8,), -1, dtype=torch.int64, device=dev)
    d_s = torch.full((n + 16,), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    counts = d.correct_keys_device(d_k.data_ptr(), d_f.data_ptr(), d_o.data_ptr(), d_s.data_ptr(), n)
    sc, ih = d.barcode_segments()
    out, st = d_o.cpu().numpy().view(U64), d_s.cpu().numpy()
    assert np.all(out[n:] == U64((1 << 64) - 1)) and np.all(st[n:] == 9)
    assert np.array_equal(d.correct_keys_device(d_k.data_ptr(), d_f.data_ptr(), 0, 0, n), counts)   # outputs may be null
    return out[:n], st[:n], counts, sc, ih


def set_segments(d, lists, seg_nt, max_inexact=None):
    d.set_whitelist_segments(lists, seg_nt, max_inexact)
    S = len(seg_nt)
    assert d.whitelist_segments_info() == dict(n_seg=S, seg_nt=list(seg_nt), seg_n=[len(np.unique(w)) for w in lists],
                                               max_inexact=S if max_inexact is None else max_inexact)
    info = d.whitelist_info()
    assert info["barcode_nt"] == sum(seg_nt) and info["table_log2"] == 0
    assert info["n_distinct"] == min(int(np.prod([len(np.unique(w)) for w in lists], dtype=object)), (1 << 64) - 1)


def check(d, keys, filt, lists, seg_nt, max_inexact=None, cover=None, device=False):
    t = sg.correct(keys, filt, lists, seg_nt, max_inexact)
    if cover is not None:
        sg.assert_covers(sg.correct(keys, filt, lists, seg_nt), **cover)
    sg.assert_same(t, raw_correct(d, keys, filt))
    if device:
        sg.assert_same(t, device_correct(d, keys, filt))
    return t


# the smallest and the largest table (1 and 10 nt), 5 nt between them; S = 1, 3 and 8; K = 32 with S = 4
SHAPES = [
    ([5], [40]),
    ([1, 5, 10], [2, 40, 300]),
    ([10, 10, 10], [96, 384, 96]),
    ([1, 1, 5, 2, 10, 3, 1, 4], [1, 4, 30, 16, 200, 10, 2, 50]),    # S = 8, K = 27; a full 1-nt list and a full 2-nt one
    ([10, 10, 10, 2], [300, 20, 1000, 3]),                          # K = 32: no key is >= 4^K
]


@pytest.mark.parametrize("seg_nt,sizes", SHAPES, ids=lambda v: "-".join(map(str, v)))
def test_shapes_and_read_counts(dd, seg_nt, sizes):
    rng = np.random.default_rng(sum(seg_nt) + len(sizes))
    lists = sg.make_lists(rng, sizes, seg_nt)
    S = len(seg_nt)
    for mi in sorted({0, 1, S}):
        set_segments(dd, lists, seg_nt, mi)
        for n in (0, 1, 63, 64, 65, 257, 20_011):
            keys, filt = sg.make_keys(rng, lists, seg_nt, n)
            cover = None
            if n > 20_000:                                          # (one segment: m is 0 or 1)
                cover = dict(inexact=(0, 1, 2) if S > 1 else (0, 1))
            check(dd, keys, filt, lists, seg_nt, mi, cover, device=n in (0, 65, 20_011))


def test_full_lists_neighbours_duplicates_and_order(dd):
    rng = np.random.default_rng(5)
    seg_nt = [3, 5, 4]
    # segment 0 holds all 4^3 values: always exact; the keys still cover everything through the other two
    lists = sg.make_lists(rng, [64, 40, 30], seg_nt)
    set_segments(dd, lists, seg_nt)
    keys, filt = sg.make_keys(rng, lists, seg_nt, 20_000)
    t = check(dd, keys, filt, lists, seg_nt, None, dict(inexact=(0, 1, 2)))
    assert int(t[3][0][0]) == int(t[3][0].sum()) > 0                # segment 0: every class count but EXACT is zero
    # every list full: every usable key below 4^K is exact
    full = sg.make_lists(rng, [64, 1024, 256], seg_nt)
    set_segments(dd, full, seg_nt, 0)
    t = check(dd, keys, filt, full, seg_nt, 0)
    assert set(np.unique(t[1])) == {0, 1, 4} and int(t[4][0]) == int(t[4].sum())
    # a pair at distance 1 in a list: the neighbour is exact, not corrected
    enc = lambda s: sum("ACGT".index(ch) << (2 * (len(s) - 1 - i)) for i, ch in enumerate(s))    # noqa: E731
    set_segments(dd, [[enc("AA"), enc("AC")], [enc("GGG")]], [2, 3])
    out, status, counts, sc, ih = raw_correct(dd, np.asarray([enc("ACGGG"), enc("AGGGG"), enc("ATGGT")], U64), np.zeros(3, np.uint8))
    assert list(status) == [1, 3, 3] and [int(x) for x in out] == [enc("ACGGG"), enc("AGGGG"), enc("ATGGT")]
    assert sc.tolist() == [[1, 0, 2, 0], [2, 1, 0, 0]] and list(ih) == [1, 1, 1] and list(counts) == [0, 1, 0, 2, 0]
    # lists given twice and shuffled: the same tables
    set_segments(dd, lists, seg_nt)
    want = raw_correct(dd, keys, filt)
    twice = [rng.permutation(np.concatenate([w, w[: len(w) // 2], w])) for w in lists]
    set_segments(dd, twice, seg_nt)
    sg.assert_same(want, raw_correct(dd, keys, filt))


def test_one_segment_equals_the_plain_correction_kernels(dd):
    rng = np.random.default_rng(7)
    plain = humid_amd.Dedup()
    try:
        for nt, n_wl in ((1, 2), (5, 40), (10, 3000)):
            wl = wt.whitelist_with_neighbours(rng, n_wl, nt)
            keys, filt = sg.make_keys(rng, [wl], [nt], 20_000)
            plain.set_whitelist(wl, nt)
            want = plain.correct_keys(keys, filt)
            set_segments(dd, [wl], [nt])
            got = raw_correct(dd, keys, filt)
            sg.assert_same(want, got[:3])
            if nt > 1:
                sg.assert_covers(sg.correct(keys, filt, [wl], [nt]), inexact=(0, 1))
    finally:
        plain.close()


def test_one_inexact_segment_equals_the_plain_correction_of_the_product(dd):
    rng = np.random.default_rng(8)
    plain = humid_amd.Dedup()
    try:
        for seg_nt, sizes in (([8, 8, 8], [96, 96, 96]), ([1, 5, 10], [2, 40, 300]), ([3, 2, 4], [6, 4, 10])):
            lists = sg.make_lists(rng, sizes, seg_nt)
            keys, filt = sg.make_keys(rng, lists, seg_nt, 20_000)
            sg.assert_covers(sg.correct(keys, filt, lists, seg_nt))
            plain.set_whitelist(sg.product_list(lists, seg_nt), sum(seg_nt))
            want = plain.correct_keys(keys, filt)
            set_segments(dd, lists, seg_nt, 1)
            sg.assert_same(want, raw_correct(dd, keys, filt)[:3])
    finally:
        plain.close()


def run_inputs(seed, n, word_nt, seg_nt, sizes):
    rng = np.random.default_rng(seed)
    lists = sg.make_lists(rng, sizes, seg_nt)
    words, filt = make_words(seed + 1, n, word_nt)
    keys, _ = sg.make_keys(rng, lists, seg_nt, n, p_filt=0.0)
    keys = np.where(filt == 1, rng.integers(0, 1 << 64, size=n, dtype=U64), keys)   # filtered reads carry garbage keys
    return lists, words, keys, filt


@pytest.mark.parametrize("word_nt,mi", [(24, None), (12, 1), (40, 3)])
def test_corrected_run(dd, word_nt, mi):
    """run_keyed(correct=True) over segments == run_keyed on the truth's corrected keys with ambiguous and unmatched
    reads marked filtered"""
    seg_nt = [4, 3, 4]
    lists, words, keys, filt = run_inputs(word_nt, 3000, word_nt, seg_nt, [10, 8, 12])
    t = sg.correct(keys, filt, lists, seg_nt, mi)
    sg.assert_covers(sg.correct(keys, filt, lists, seg_nt))
    filt2 = ((filt != 0) | (t[1] >= 3)).astype(np.uint8)
    set_segments(dd, lists, seg_nt, mi)
    other = humid_amd.Dedup()
    try:
        for distance, method in ((1, 0), (1, 1), (2, 0)):
            want = other.run_keyed(words, t[0], filt2, word_nt=word_nt, distance=distance, method=method)
            want_keys = other.group_keys()
            got = dd.run_keyed(words, keys, filt, word_nt=word_nt, distance=distance, method=method, correct=True)
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
            for name in ("total", "usable", "unique", "clusters", "edges"):
                assert want[2][name] == got[2][name], name
            assert got[2]["usable"] == int(t[2][1] + t[2][2])
            K = dd.group_keys()
            assert np.array_equal(K, want_keys) and np.all(np.isin(K, sg.product_list(lists, seg_nt)))
            status, counts = dd.barcode_status()
            assert np.array_equal(status, t[1]) and np.array_equal(counts, t[2])
            sc, ih = dd.barcode_segments()
            assert np.array_equal(sc, t[3]) and np.array_equal(ih, t[4])
    finally:
        other.close()


def test_corrected_run_device_pointers(dd):
    import torch
    seg_nt = [8, 8, 8]
    lists, words, keys, filt = run_inputs(41, 20_000, 28, seg_nt, [96, 96, 96])
    t = sg.correct(keys, filt, lists, seg_nt)
    sg.assert_covers(t)
    filt2 = ((filt != 0) | (t[1] >= 3)).astype(np.uint8)
    set_segments(dd, lists, seg_nt)
    other = humid_amd.Dedup()
    try:
        want = other.run_keyed(words, t[0], filt2, word_nt=28)
    finally:
        other.close()
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_k = torch.from_numpy(keys.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_cid = torch.zeros(len(filt), dtype=torch.int32, device=dev)
    d_keep = torch.zeros(len(filt), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s = dd.run_keyed_corrected_device(d_w.data_ptr(), d_k.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(),
                                      len(filt), word_nt=28, distance=1)
    assert np.array_equal(d_cid.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(d_keep.cpu().numpy(), want[1])
    assert s["clusters"] == want[2]["clusters"] and s["usable"] == int(t[2][1] + t[2][2])
    assert np.array_equal(d_k.cpu().numpy().view(U64), keys) and np.array_equal(d_f.cpu().numpy(), filt)   # inputs untouched
    sc, ih = dd.barcode_segments()
    assert np.array_equal(sc, t[3]) and np.array_equal(ih, t[4])


def test_state_rules():
    d = humid_amd.Dedup()
    try:
        seg_nt = [4, 3, 4]
        lists, words, keys, filt = run_inputs(31, 2000, 24, seg_nt, [10, 8, 12])
        t = sg.correct(keys, filt, lists, seg_nt)
        sg.assert_covers(t)
        none = dict(n_seg=0, seg_nt=[], seg_n=[], max_inexact=0)
        assert d.whitelist_segments_info() == none and d.whitelist_info()["n_distinct"] == 0
        with pytest.raises(humid_amd.HumidError) as ei:
            d.barcode_segments()
        assert ei.value.code == E_STATE
        # segments -> plain -> segments -> clear
        set_segments(d, lists, seg_nt)
        with pytest.raises(humid_amd.HumidError) as ei:             # set, but nothing corrected yet
            d.barcode_segments()
        assert ei.value.code == E_STATE
        sg.assert_same(t[:3], d.correct_keys(keys, filt))
        plain_wl = wt.whitelist_with_neighbours(np.random.default_rng(2), 300, 11)
        d.set_whitelist(plain_wl, 11)
        assert d.whitelist_segments_info() == none
        assert d.whitelist_info() == dict(n_distinct=len(np.unique(plain_wl)), barcode_nt=11, table_log2=10)
        sg.assert_same(wt.correct_np(keys, filt, plain_wl, 11), d.correct_keys(keys, filt))
        with pytest.raises(humid_amd.HumidError) as ei:
            d.barcode_segments()
        assert ei.value.code == E_STATE
        set_segments(d, lists, seg_nt, 2)
        sg.assert_same(sg.correct(keys, filt, lists, seg_nt, 2)[:3], d.correct_keys(keys, filt))
        d.set_whitelist(None)
        assert d.whitelist_segments_info() == none and d.whitelist_info() == dict(n_distinct=0, barcode_nt=0, table_log2=0)
        with pytest.raises(humid_amd.HumidError) as ei:
            d.correct_keys(keys, filt)
        assert ei.value.code == E_STATE
        # every refused set leaves the previous whitelist working: first a segmented one, then a plain one
        u32 = lambda a: np.asarray(a, np.uint32)                    # noqa: E731
        bad = [
            (0, [], [], [0], 0),                                    # no segment
            (9, [1] * 9, [1] * 9, [0] * 9, 9),                      # nine
            (2, [0, 4], [1, 1], [0, 0], 2),                         # a segment of no nucleotide
            (2, [11, 4], [1, 1], [0, 0], 2),                        # one of eleven
            (4, [10, 10, 10, 3], [1, 1, 1, 1], [0, 0, 0, 0], 4),    # K = 33
            (2, [4, 4], [1, 0], [0], 2),                            # an empty list
            (2, [4, 4], [1, 1], [0, 256], 2),                       # an entry >= 4^L
            (2, [4, 4], [1, 1], [0, 0], 3),                         # max_inexact > S
        ]
        for install, again in ((lambda: set_segments(d, lists, seg_nt), lambda: sg.assert_same(t[:3], d.correct_keys(keys, filt))),
                               (lambda: d.set_whitelist(plain_wl, 11),
                                lambda: sg.assert_same(wt.correct_np(keys, filt, plain_wl, 11), d.correct_keys(keys, filt)))):
            install()
            before = (d.whitelist_info(), d.whitelist_segments_info())
            for S, nt, n, b, mi in bad:
                nt_a, n_a, b_a = u32(nt + [0]), np.asarray(n + [0], U64), np.asarray(b + [0], U64)
                rc = d._lib.humid_whitelist_set_segments(d._h, S, C.c_void_p(nt_a.ctypes.data), C.c_void_p(n_a.ctypes.data),
                                                         C.c_void_p(b_a.ctypes.data), mi)
                assert rc == E_INVALID, (S, nt, n, b, mi)
            assert (d.whitelist_info(), d.whitelist_segments_info()) == before
            again()
        # the posterior calls and runs, and the reads per barcode, with segments in place
        set_segments(d, lists, seg_nt)
        q = np.full((len(keys), sum(seg_nt)), 70, np.uint8)
        for call in (lambda: d.correct_keys(keys, filt, quals=q),
                     lambda: d.run_keyed(words, keys, filt, word_nt=24, correct=True, barcode_quals=q),
                     lambda: d.correct_keys_posterior_device(0, 0, 0, 0, 0, 0)):
            with pytest.raises(humid_amd.HumidError) as ei:
                call()
            assert ei.value.code == E_UNSUPPORTED
        with pytest.raises(humid_amd.HumidError) as ei:
            d.whitelist_counts(lists[0])
        assert ei.value.code == E_STATE
        sg.assert_same(t[:3], d.correct_keys(keys, filt))          # ... and the context stays usable
        # a run's accessors survive a bare correct_keys; barcode_segments is the later of the two
        d.run_keyed(words, keys, filt, word_nt=24, correct=True)
        before = (d.leaves(), d.barcode_status(), d.group_keys(), d.barcode_segments())
        assert np.array_equal(before[3][0], t[3]) and np.array_equal(before[3][1], t[4])
        other_keys, other_filt = sg.make_keys(np.random.default_rng(1), lists, seg_nt, 777)
        o = sg.correct(other_keys, other_filt, lists, seg_nt)
        sg.assert_same(o[:3], d.correct_keys(other_keys, other_filt))
        after = (d.leaves(), d.barcode_status(), d.group_keys(), d.barcode_segments())
        for name in before[0]:
            assert np.array_equal(before[0][name], after[0][name]), name
        assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
        assert np.array_equal(before[2], after[2])
        assert np.array_equal(after[3][0], o[3]) and np.array_equal(after[3][1], o[4])
        # the segments survive plain and keyed runs; discover_whitelist replaces them
        d.run(words, filt, word_nt=24)
        d.run_keyed(words, keys, filt, word_nt=24)
        sg.assert_same(t[:3], d.correct_keys(keys, filt))
        filt2 = ((filt != 0) | (t[1] >= 3)).astype(np.uint8)
        sm = d.discover_whitelist(t[0], filt2, barcode_nt=sum(seg_nt), min_reads=2)
        assert sm["cells"] > 0 and d.whitelist_segments_info() == none
        cells, _ = d.discovered_cells()
        assert d.whitelist_info()["n_distinct"] == len(cells)
        sg.assert_same(wt.correct_np(t[0], filt2, cells, sum(seg_nt)), d.correct_keys(t[0], filt2))
        with pytest.raises(humid_amd.HumidError) as ei:
            d.barcode_segments()
        assert ei.value.code == E_STATE
    finally:
        d.close()
