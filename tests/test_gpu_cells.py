"""-m gpu: the whitelist taken from the data (humid_whitelist_discover*, humid_get_discovered_cells,
humid_get_barcode_count_hist) against the truth of tests/cells_truth.py, bit for bit: the cells, their reads, every
field of the summary and the histogram, in both forms of the merge kernel; the whitelist the call installs against
set_whitelist with the truth's cells; what the call must leave alone; its refusals and the state rules of the getters."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib

import cells_truth as ct
from test_gpu_keyed import make_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
ALL_T = ct.ALL_T
E_INVALID, E_OVERFLOW, E_STATE = -1, -5, -6
MODES = {ct.TOP: "top", ct.EXPECTED: "expected", ct.MIN_READS: "min_reads"}


@pytest.fixture(scope="module", params=[1, 0], ids=["wave_cooperative", "lane_serial"])
def dd(request):
    """the two forms of the merge kernel (option "whitelist_coop")"""
    d = humid_amd.Dedup()
    d.set_option("whitelist_coop", request.param)
    yield d
    d.close()


@pytest.fixture(scope="module")
def plain():
    d = humid_amd.Dedup()
    yield d
    d.close()


def enc(s):
    return sum("ACGT".index(ch) << (2 * (len(s) - 1 - i)) for i, ch in enumerate(s))


def check(d, keys, filt, k, mode, param, ratio=0, truth=None):
    """the device against the truth: everything the call and its getters return, and the whitelist it installs"""
    keys, filt = np.ascontiguousarray(keys, U64), np.ascontiguousarray(filt, np.uint8)
    t = truth if truth is not None else ct.discover(keys, filt, k, mode, param, ratio)
    sm = d.discover_whitelist(keys, filt, barcode_nt=k, merge_ratio=ratio, **{MODES[mode]: param})
    assert sm == t[2], (sm, t[2])
    cells, reads = d.discovered_cells()
    assert cells.dtype == t[0].dtype and np.array_equal(cells, t[0])
    assert reads.dtype == t[1].dtype and np.array_equal(reads, t[1])
    hn, hb = d.barcode_count_hist()
    assert hn.dtype == U64 and hb.dtype == U64 and np.array_equal(hn, t[3][0]) and np.array_equal(hb, t[3][1])
    info = d.whitelist_info()
    n = len(t[0])
    if n:
        assert info["n_distinct"] == n and info["barcode_nt"] == k
        assert (1 << info["table_log2"]) >= 2 * n and ((1 << info["table_log2"]) < 4 * n or info["table_log2"] == 1)
    else:
        assert info == dict(n_distinct=0, barcode_nt=0, table_log2=0)
    return t


def mixture(rng, k, n, p_err=0.05, p_ambient=0.1, p_invalid=0.02, p_filt=0.05):
    """n reads: cells with geometric sizes, reads one substitution off, ambient barcodes, keys >= 4^k (k < 32), filtered
    reads whose key must not be read"""
    if n == 0:
        return np.zeros(0, U64), np.zeros(0, np.uint8)
    mask = (1 << (2 * k)) - 1
    n_cells = max(1, min(n // 40, 4 ** k // 2))
    cells = np.asarray(ct.random_barcodes(rng, n_cells, k, apart=False), U64)
    keys = cells[np.minimum(rng.geometric(min(max(4.0 / n_cells, 0.02), 0.5), size=n) - 1, n_cells - 1)]
    sub = (rng.integers(1, 4, size=n).astype(U64) << (U64(2) * rng.integers(0, k, size=n).astype(U64)))
    keys = np.where(rng.random(n) < p_err, keys ^ sub, keys)
    amb = rng.integers(0, 1 << 62, size=n).astype(U64) * U64(4) + rng.integers(0, 4, size=n).astype(U64)
    keys = np.where(rng.random(n) < p_ambient, amb & U64(mask), keys)
    if k < 32:
        keys = np.where(rng.random(n) < p_invalid, keys | (U64(1 + int(rng.integers(0, 3))) << U64(2 * k)), keys)
    filt = (rng.random(n) < p_filt).astype(np.uint8)
    return np.where(filt != 0, U64(ALL_T), keys), filt


@pytest.mark.parametrize("k", [1, 4, 16, 31, 32])
def test_read_counts_and_barcode_lengths(dd, k):
    rng = np.random.default_rng(400 + k)
    seen_invalid = seen_merged = 0
    for n in (0, 1, 63, 64, 65, 257, 100_000):
        keys, filt = mixture(rng, k, n)
        if k == 32 and n >= 257:
            keys[:40] = U64(ALL_T)                                  # the all-T barcode: the table's empty mark, here a cell
            keys[40:44] = U64(ALL_T ^ 1)
            filt[:44] = 0
        for mode, param, ratio in ((ct.TOP, 5, 0), (ct.EXPECTED, 3, 3), (ct.MIN_READS, 2, 2), (ct.TOP, 10 ** 12, 1)):
            t = check(dd, keys, filt, k, mode, param, ratio)
            seen_invalid += t[2]["invalid_reads"]
            seen_merged += t[2]["merged"]
            if k == 32 and n >= 257 and mode == ct.MIN_READS:
                assert ALL_T in set(int(x) for x in t[0]) and (ALL_T ^ 1) not in set(int(x) for x in t[0])
    assert (seen_invalid > 0) == (k < 32) and seen_merged > 0
    check(dd, keys, np.ones(len(keys), np.uint8), k, ct.TOP, 5, 2)     # all filtered: no cell, the whitelist is cleared
    assert dd.whitelist_info()["n_distinct"] == 0


def test_all_t_barcode_at_32_nucleotides(dd):
    """all-T as a cell, as a neighbour that removes cells, and as a cell that a neighbour removes"""
    rng = np.random.default_rng(7)
    others = ct.random_barcodes(rng, 20, 32)
    table = [(ALL_T, 500), (ALL_T ^ 1, 40), (ALL_T ^ (3 << 62), 45), (ALL_T ^ (2 << 30), 101)] + [(v, 60) for v in others]
    keys, filt = ct.from_counts(table, rng, filtered_between=3)
    t = check(dd, keys, filt, 32, ct.MIN_READS, 40, 5)
    got = set(int(x) for x in t[0])
    assert ALL_T in got and (ALL_T ^ 1) not in got and (ALL_T ^ (3 << 62)) not in got and (ALL_T ^ (2 << 30)) in got
    assert t[2]["merged"] == 2
    check(dd, keys, filt, 32, ct.MIN_READS, 40, 0)
    table = [(ALL_T, 10), (ALL_T ^ (1 << 62), 1000)] + [(v, 60) for v in others]
    keys, filt = ct.from_counts(table, rng)
    t = check(dd, keys, filt, 32, ct.TOP, 100, 5)
    assert ALL_T not in set(int(x) for x in t[0]) and t[2]["merged"] == 1


def test_sorted_and_shuffled_reads_give_the_same(dd):
    """sorted by key: runs longer than a wave and crossing waves, one probe and one atomic add per run and wave"""
    rng = np.random.default_rng(8)
    keys, filt = mixture(rng, 16, 30_000, p_filt=0.0)
    filt[rng.integers(0, len(filt), size=300)] = 1                  # filtered reads inside the runs
    order = np.argsort(keys, kind="stable")
    a = check(dd, keys[order], filt[order], 16, ct.EXPECTED, 20, 3)
    b = check(dd, keys, filt, 16, ct.EXPECTED, 20, 3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and int(a[1].max()) > 200


def test_heavy_barcodes(dd):
    one = np.full(100_000, 0x1234ABCD, U64)
    t = check(dd, one, np.zeros(len(one), np.uint8), 16, ct.TOP, 3, 2)
    assert list(t[1]) == [100_000] and t[2]["distinct"] == 1
    rng = np.random.default_rng(9)
    table = [(enc("ACGTACGTACGTACGT"), 70_000), (enc("ACGTACGTACGTACGA"), 66_000), (enc("TTTTACGTACGTACGA"), 65_536), (5, 65_535)]
    keys, filt = ct.from_counts(table + [(v, 3) for v in ct.random_barcodes(rng, 50, 16)], rng)
    t = check(dd, keys, filt, 16, ct.MIN_READS, 65_536, 1)
    assert sorted(int(x) for x in t[1]) == [65_536, 70_000]
    check(dd, keys, filt, 16, ct.EXPECTED, 1, 0)


def test_top(dd):
    rng = np.random.default_rng(10)
    tie = sorted(ct.random_barcodes(rng, 9, 16))
    table = [(enc("CCCCCCCCCCCCCCCC"), 50)] + [(v, 7) for v in tie] + [(enc("GGGGGGGGGGGGGGGG"), 2)]
    keys, filt = ct.from_counts(table, rng)
    for T in (1, 2, 5, 10, 11):                                     # 2 .. 10 cut through the run of equal counts
        t = check(dd, keys, filt, 16, ct.TOP, T)
        assert set(int(x) for x in t[0]) == set([table[0][0]] + tie[:T - 1] + ([table[-1][0]] if T == 11 else []))
    for T in (12, 1000, 2 ** 64 - 1):                               # T > G
        assert check(dd, keys, filt, 16, ct.TOP, T)[2]["cells"] == 11


def test_expected(dd):
    rng = np.random.default_rng(11)
    rest = ct.random_barcodes(rng, 4, 16)
    for top, n_in in ((100, 3), (101, 2)):                          # 10 n = m is in, 10 n = m - 1 is out
        table = [(rest[0], top), (rest[1], 50), (rest[2], 10), (rest[3], 9)]
        keys, filt = ct.from_counts(table, rng)
        assert check(dd, keys, filt, 16, ct.EXPECTED, 1)[2]["selected"] == n_in          # X = 1: b = 0
        assert check(dd, keys, filt, 16, ct.EXPECTED, 49)[2]["selected"] == n_in         # still b = 0
        assert check(dd, keys, filt, 16, ct.EXPECTED, 50)[2]["selected"] == 4            # b = 1, m = 50
        assert check(dd, keys, filt, 16, ct.EXPECTED, 250)[2]["selected"] == 4           # b = 3 = G - 1
        assert check(dd, keys, filt, 16, ct.EXPECTED, 251)[2]["selected"] == 4           # beyond: capped at G - 1
        assert check(dd, keys, filt, 16, ct.EXPECTED, 2 ** 64 - 1)[2]["selected"] == 4


def test_min_reads(dd):
    rng = np.random.default_rng(12)
    bc = ct.random_barcodes(rng, 6, 16)
    keys, filt = ct.from_counts(list(zip(bc, (40, 20, 20, 7, 7, 1))), rng, filtered_between=2)
    for T, n_in in ((1, 6), (6, 5), (7, 5), (8, 3), (20, 3), (21, 1), (40, 1), (41, 0), (2 ** 64 - 1, 0)):
        t = check(dd, keys, filt, 16, ct.MIN_READS, T)
        assert t[2]["cells"] == n_in and t[2]["threshold_reads"] == (min(c for c in (40, 20, 7, 1) if c >= T) if n_in else 0)


@pytest.mark.parametrize("k", [4, 16, 22, 32])
def test_merge(dd, k):
    """22 nucleotides are 66 variants: the second round of the wave"""
    rng = np.random.default_rng(500 + k)
    lo, hi = 1, 1 << (2 * (k - 1))                                  # a substitution at nucleotide k - 1 and at nucleotide 0
    a = ct.random_barcodes(rng, 1, k)[0]
    far = [v for v in ct.random_barcodes(rng, 40, k) if bin(v ^ a).count("1") > 8][:6] if k > 4 else []
    # a chain a - b - c of 1000, 100, 10 reads, R = 5: b is removed and still removes c
    b, c = a ^ lo, a ^ lo ^ (2 * hi)
    keys, filt = ct.from_counts([(a, 1000), (b, 100), (c, 10)] + [(v, 30) for v in far], rng)
    t = check(dd, keys, filt, k, ct.MIN_READS, 1, 5)
    assert sorted(int(x) for x in t[0]) == sorted([a] + far) and t[2]["merged"] == 2
    # n_v = R n_w removes, n_v = R n_w - 1 keeps; at both ends of the barcode
    for sub in (lo, 3 * lo, hi, 3 * hi):
        for n_v, gone in ((500, True), (499, False)):
            keys, filt = ct.from_counts([(a, n_v), (a ^ sub, 100)] + [(v, 30) for v in far], rng)
            t = check(dd, keys, filt, k, ct.TOP, 50, 5)
            assert ((a ^ sub) in set(int(x) for x in t[0])) != gone and t[2]["merged"] == int(gone)
    # two neighbouring cells of equal count, R = 1: only the larger value goes
    keys, filt = ct.from_counts([(a, 80), (a ^ hi, 80)] + [(v, 30) for v in far], rng)
    t = check(dd, keys, filt, k, ct.TOP, 50, 1)
    assert t[2]["merged"] == 1 and min(a, a ^ hi) in set(int(x) for x in t[0]) and max(a, a ^ hi) not in set(int(x) for x in t[0])

def test_both_kernel_forms_agree(plain):
    rng = np.random.default_rng(13)
    keys, filt = mixture(rng, 16, 50_000, p_err=0.2)
    out = []
    for coop in (1, 0):
        plain.set_option("whitelist_coop", coop)
        t = check(plain, keys, filt, 16, ct.MIN_READS, 2, 3)
        out.append((plain.discovered_cells(), t[2]))
    plain.set_option("whitelist_coop", 1)
    assert np.array_equal(out[0][0][0], out[1][0][0]) and np.array_equal(out[0][0][1], out[1][0][1]) and out[0][1]["merged"] > 100


def test_table_growth(plain):
    """16 slots for 5 000 distinct barcodes: the count is repeated with 16 times the slots until they fit"""
    rng = np.random.default_rng(14)
    bc = np.asarray(ct.random_barcodes(rng, 5000, 16, apart=False), U64)
    keys = bc[rng.integers(0, 5000, size=40_000)]
    keys[:5000] = bc
    filt = np.zeros(len(keys), np.uint8)
    t = ct.discover(keys, filt, 16, ct.EXPECTED, 500, 2)
    assert t[2]["distinct"] == 5000
    plain.set_option("cells_table_log2", 4)
    check(plain, keys, filt, 16, ct.EXPECTED, 500, 2, truth=t)
    plain.set_option("cells_table_log2", 20)                         # a table beyond 2 n_reads is cut down to that
    check(plain, keys[:3], filt[:3], 16, ct.TOP, 5)
    plain.set_option("cells_table_log2", 0)
    check(plain, keys, filt, 16, ct.EXPECTED, 500, 2, truth=t)
    with pytest.raises(humid_amd.HumidError):
        plain.set_option("cells_table_log2", 3)
    with pytest.raises(humid_amd.HumidError):
        plain.set_option("cells_table_log2", 33)


def test_device_tensors(plain):
    import torch
    rng = np.random.default_rng(15)
    keys, filt = mixture(rng, 16, 20_000)
    t = ct.discover(keys, filt, 16, ct.EXPECTED, 30, 4)
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    df = torch.from_numpy(filt).cuda()
    sm = plain.discover_whitelist(dk, df, barcode_nt=16, expected=30, merge_ratio=4)
    assert sm == t[2]
    cells, reads = plain.discovered_cells()
    assert np.array_equal(cells, t[0]) and np.array_equal(reads, t[1])
    assert np.array_equal(dk.cpu().numpy().view(U64), keys) and np.array_equal(df.cpu().numpy(), filt)
    sm = plain.discover_whitelist(dk[:0], df[:0], barcode_nt=16, top=1)
    assert sm == ct.discover(keys[:0], filt[:0], 16, ct.TOP, 1)[2] and plain.whitelist_info()["n_distinct"] == 0


def test_the_installed_whitelist_is_that_of_set_whitelist(plain):
    rng = np.random.default_rng(16)
    keys, filt, _ = ct.planted(rng, 16, 40, 60, 1.05, 0.05, 2000)
    words, _ = make_words(21, len(keys), 12)
    quals = rng.integers(33, 74, size=(len(keys), 16)).astype(np.uint8)
    t = check(plain, keys, filt, 16, ct.EXPECTED, 40, 5)
    assert len(t[0]) == 40
    with pytest.raises(humid_amd.HumidError) as ei:                  # no posterior call over this whitelist yet
        plain.whitelist_counts(t[0])
    assert ei.value.code == E_STATE
    got = [plain.correct_keys(keys, filt), plain.run_keyed(words, keys, filt, word_nt=12, correct=True)[:2], plain.barcode_status(),
           plain.correct_keys(keys, filt, quals=quals), plain.whitelist_counts(t[0])]
    info = plain.whitelist_info()
    assert np.array_equal(plain.discovered_cells()[0], t[0])         # runs and corrections leave the getters alone
    plain.set_whitelist(t[0], 16)
    assert plain.whitelist_info() == info
    want = [plain.correct_keys(keys, filt), plain.run_keyed(words, keys, filt, word_nt=12, correct=True)[:2], plain.barcode_status(),
            plain.correct_keys(keys, filt, quals=quals), plain.whitelist_counts(t[0])]
    for g, w in zip(got, want):
        if isinstance(g, np.ndarray):
            g, w = [g], [w]
        for x, y in zip(g, w):
            assert (x == y) if isinstance(x, dict) else np.array_equal(x, y)
    assert set(int(s) for s in got[0][1]) == {0, 1, 2, 4} or set(int(s) for s in got[0][1]) == {0, 1, 2, 3, 4}
    assert np.array_equal(got[4], t[1])                              # the exact reads per cell are the cells' counts


def test_a_discover_call_leaves_the_last_run_alone(plain):
    rng = np.random.default_rng(18)
    n = 6000
    words, filt = make_words(23, n, 12)
    run_keys = np.asarray(ct.random_barcodes(rng, 300, 16, apart=False), U64)[rng.integers(0, 300, size=n)]
    plain.set_whitelist(None)
    cid, keep, s = plain.run_keyed(words, run_keys, filt, word_nt=12)

    def snapshot():
        lv = plain.leaves()
        return [plain.group_keys(), plain.keyed_rank_info(), plain.group_stats(), lv, plain.adjacency(), plain.clusters(), plain.histograms()]

    def equal(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
        return np.array_equal(a, b)

    before = snapshot()
    other, ofilt = mixture(rng, 16, 50_000)                          # more distinct keys than the run had: a larger table
    t = check(plain, other, ofilt, 16, ct.EXPECTED, 30, 3)
    assert t[2]["distinct"] > 3000 and equal(before, snapshot())
    check(plain, other[:0], ofilt[:0], 16, ct.TOP, 1)
    assert equal(before, snapshot())


def raw_discover(d, keys, filt, n, k, mode, param, ratio=0):
    sm = _lib.HumidCellsSummary()
    sm.cells = 12345
    vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)   # noqa: E731
    rc = d._lib.humid_whitelist_discover(d._h, vp(keys), vp(filt), n, k, mode, param, ratio, C.byref(sm))
    return rc, sm


def test_refusals_leave_the_whitelist_in_place(plain):
    rng = np.random.default_rng(19)
    keys, filt = mixture(rng, 16, 3000)
    t = check(plain, keys, filt, 16, ct.TOP, 20, 2)
    probe = np.concatenate([t[0], t[0] ^ U64(1)])
    expect = plain.correct_keys(probe, np.zeros(len(probe), np.uint8))
    info = plain.whitelist_info()
    for args, code in (((keys, filt, 3000, 0, 0, 5), E_INVALID), ((keys, filt, 3000, 33, 0, 5), E_INVALID),
                       ((keys, filt, 3000, 16, 3, 5), E_INVALID), ((keys, filt, 3000, 16, 1, 0), E_INVALID),
                       ((None, filt, 3000, 16, 0, 5), E_INVALID), ((keys, None, 3000, 16, 0, 5), E_INVALID),
                       ((keys, filt, 2 ** 31, 16, 0, 5), E_OVERFLOW)):
        rc, sm = raw_discover(plain, *args)
        assert rc == code and sm.cells == 12345, (args[2:], rc)
        assert plain.whitelist_info() == info
        again = plain.correct_keys(probe, np.zeros(len(probe), np.uint8))
        assert all(np.array_equal(x, y) for x, y in zip(expect, again))
        cells, reads = plain.discovered_cells()                      # the earlier call's results stay with its whitelist
        assert np.array_equal(cells, t[0]) and np.array_equal(reads, t[1])
    rc, sm = raw_discover(plain, None, None, 0, 16, 0, 5)            # no reads: legal, zero cells, the whitelist is cleared
    assert rc == 0 and sm.cells == 0 and plain.whitelist_info()["n_distinct"] == 0
    for kw in (dict(), dict(top=1, expected=2), dict(top=0), dict(top=1, merge_ratio=-1), dict(top=1, barcode_nt=0)):
        with pytest.raises(ValueError):
            plain.discover_whitelist(keys, filt, **kw)


def test_getters_answer_only_for_a_discovered_whitelist():
    d = humid_amd.Dedup()
    try:
        rng = np.random.default_rng(20)
        keys, filt = mixture(rng, 16, 2000)
        n = C.c_uint64(77)
        for fn in (d._lib.humid_get_discovered_cells, d._lib.humid_get_barcode_count_hist):
            assert fn(d._h, None, None, 0, C.byref(n)) == E_STATE and n.value == 77        # before any discover call
        check(d, keys, filt, 16, ct.TOP, 10)
        d.set_whitelist(d.discovered_cells()[0], 16)                 # the same barcodes, but set by the caller
        for fn in (d.discovered_cells, d.barcode_count_hist):
            with pytest.raises(humid_amd.HumidError) as ei:
                fn()
            assert ei.value.code == E_STATE
        check(d, keys, filt, 16, ct.TOP, 10)
        d.set_whitelist(None)                                        # a clear
        with pytest.raises(humid_amd.HumidError):
            d.discovered_cells()
        check(d, keys, filt, 16, ct.MIN_READS, 10 ** 9)              # a call that finds no cell still answers
        assert len(d.barcode_count_hist()[0]) > 0 and len(d.discovered_cells()[0]) == 0
        # partial buffers: the first `cap` entries, *n_out the whole number
        t = check(d, keys, filt, 16, ct.TOP, 10)
        b, r = np.full(4 + 2, 0xA5A5A5A5A5A5A5A5, U64), np.full(4 + 2, 0xA5A5A5A5, np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
        assert d._lib.humid_get_discovered_cells(d._h, vp(b), vp(r), 4, C.byref(n)) == 0 and n.value == 10
        assert np.array_equal(b[:4], t[0][:4]) and np.array_equal(r[:4], t[1][:4]) and np.all(b[4:] == b[5]) and r[4] == 0xA5A5A5A5
        hn, hb = np.full(2 + 2, 0xA5A5A5A5A5A5A5A5, U64), np.full(2 + 2, 0xA5A5A5A5A5A5A5A5, U64)
        assert d._lib.humid_get_barcode_count_hist(d._h, vp(hn), vp(hb), 2, C.byref(n)) == 0 and n.value == len(t[3][0]) > 2
        assert np.array_equal(hn[:2], t[3][0][:2]) and np.array_equal(hb[:2], t[3][1][:2]) and hn[2] == hn[3] == hb[2] == hb[3]
    finally:
        d.close()
