"""-m gpu: the barcode counter fed in chunks (humid_cells_*, Dedup.barcode_counter) against two references that are not
the code under test: the truth of tests/cells_truth.py over the concatenation of the chunks, and the one-shot
discover_whitelist over it on another context.  Everything is integer arithmetic: every comparison is exact.  Covered:
the chunkings around the wave boundaries of the run-of-equal-keys logic, in both orders; growth inside an add and
between adds (info()["n_grown"]); the reserved slot of the all-T barcode across a growth; invalid keys, empty and
all-filtered chunks; a chunk of one barcode; finish twice and add after finish; what the counter must leave alone and
what must leave it alone; states and refusals.

NOT tested here: the limit of 2^31 - 1 reads per barcode (HUMID_E_OVERFLOW) and the INVALID state a failed add leaves
behind.  Both need billions of reads or a failing device, and neither is simulated by provoking a failure."""
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
CASES = [(ct.TOP, 40, 0), (ct.TOP, 200, 3), (ct.EXPECTED, 60, 0), (ct.EXPECTED, 300, 3), (ct.MIN_READS, 2, 0), (ct.MIN_READS, 1, 3)]


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


@pytest.fixture(scope="module")
def ref():
    """the context of the one-shot calls"""
    d = humid_amd.Dedup()
    yield d
    d.close()


def skewed(seed, n=3000, k=8, n_cells=150, p_err=0.03, p_filt=0.02, p_invalid=0.0):
    """n reads over about 200 distinct barcodes (n_cells with geometric sizes and their one-substitution errors), some
    filtered reads (their key is all-T and must not be read), and with p_invalid keys >= 4^k"""
    rng = np.random.default_rng(seed)
    cells = np.asarray(ct.random_barcodes(rng, n_cells, k, apart=False), U64)
    keys = cells[np.minimum(rng.geometric(0.03, size=n) - 1, n_cells - 1)]
    sub = rng.integers(1, 4, size=n).astype(U64) << (U64(2) * rng.integers(0, k, size=n).astype(U64))
    keys = np.where(rng.random(n) < p_err, keys ^ sub, keys)
    if p_invalid:
        keys = np.where(rng.random(n) < p_invalid, keys | (U64(1 + int(rng.integers(0, 3))) << U64(2 * k)), keys)
    filt = (rng.random(n) < p_filt).astype(np.uint8)
    return np.where(filt != 0, U64(ALL_T), keys), filt


def cut(n, size):
    return [(a, min(a + size, n)) for a in range(0, n, size)] or [(0, 0)]


def answers(d):
    """what a finish or a discover call leaves behind its summary"""
    cells, reads = d.discovered_cells()
    hn, hb = d.barcode_count_hist()
    return cells, reads, hn, hb, d.whitelist_info()


def same(a, b):
    return all((x == y) if isinstance(x, dict) else (x.dtype == y.dtype and np.array_equal(x, y)) for x, y in zip(a, b))


class OneShot:
    """discover_whitelist over a whole read set on the reference context and the CPU truth, computed once per case"""

    def __init__(self, ref, keys, filt, k):
        self.ref, self.keys, self.filt, self.k = ref, np.ascontiguousarray(keys, U64), np.ascontiguousarray(filt, np.uint8), k
        self.memo = {}

    def __call__(self, mode, param, ratio):
        if (mode, param, ratio) not in self.memo:
            sm = self.ref.discover_whitelist(self.keys, self.filt, barcode_nt=self.k, merge_ratio=ratio, **{MODES[mode]: param})
            got = answers(self.ref)
            t = ct.discover(self.keys, self.filt, self.k, mode, param, ratio)
            assert sm == t[2] and same(got[:4], (t[0], t[1], t[3][0], t[3][1]))       # the two references agree
            self.memo[(mode, param, ratio)] = (sm, got)
        return self.memo[(mode, param, ratio)]

    def check(self, d, bc, mode, param, ratio):
        want_sm, want = self(mode, param, ratio)
        sm = bc.finish(merge_ratio=ratio, **{MODES[mode]: param})
        got = answers(d)
        assert sm == want_sm, (sm, want_sm)
        assert same(got, want), (mode, param, ratio)
        return sm, got


def feed(bc, keys, filt, pieces):
    for a, b in pieces:
        bc.add(keys[a:b], filt[a:b])


@pytest.fixture(scope="module")
def reads3000(ref):
    keys, filt = skewed(501)
    one = OneShot(ref, keys, filt, 8)
    sm, got = one(ct.MIN_READS, 1, 3)
    assert 150 <= sm["distinct"] <= 300 and sm["merged"] > 20 and 0 < sm["cells"] < sm["distinct"]
    return keys, filt, one


@pytest.mark.parametrize("size", [1, 63, 64, 65, 700, 3000])
@pytest.mark.parametrize("reverse", [False, True], ids=["in_order", "reversed"])
def test_chunkings_against_the_one_shot_and_the_truth(dd, reads3000, size, reverse):
    keys, filt, one = reads3000
    pieces = cut(len(keys), size)
    bc = dd.barcode_counter(barcode_nt=8)
    feed(bc, keys, filt, pieces[::-1] if reverse else pieces)
    for mode, param, ratio in CASES:
        sm, _ = one.check(dd, bc, mode, param, ratio)
    info = bc.info()
    assert info == dict(barcode_nt=8, chunks=len(pieces), reads=len(keys), usable=int((filt == 0).sum()), invalid_reads=0,
                        distinct=sm["distinct"], table_log2=16, n_grown=0)


def test_growth_inside_an_add_and_between_adds(reads3000):
    keys, filt, one = reads3000
    d = humid_amd.Dedup()
    try:
        d.set_option("cells_table_log2", 4)
        bc = d.barcode_counter(barcode_nt=8)
        first = keys[:400][filt[:400] == 0]
        assert len(np.unique(first)) > 16                            # more barcodes than the table starts with: growth inside the add
        bc.add(keys[:400], filt[:400])
        grown = bc.info()["n_grown"]
        assert grown >= 1 and bc.info()["distinct"] == len(np.unique(first))
        feed(bc, keys, filt, cut(len(keys), 400)[1:])
        info = bc.info()
        assert info["n_grown"] >= 2 and info["n_grown"] > grown and (1 << info["table_log2"]) >= 2 * info["distinct"]
        for mode, param, ratio in CASES:
            one.check(d, bc, mode, param, ratio)
        # every barcode in one add into 16 slots: the table grows more than once inside it
        bc = d.barcode_counter(barcode_nt=8)
        bc.add(keys, filt)
        assert bc.info()["n_grown"] >= 2
        one.check(d, bc, ct.MIN_READS, 1, 3)
        d.set_option("cells_table_log2", 0)                          # the default size: nothing grows
        bc = d.barcode_counter(barcode_nt=8)
        feed(bc, keys, filt, cut(len(keys), 400))
        assert bc.info()["n_grown"] == 0 and bc.info()["table_log2"] == 16
        one.check(d, bc, ct.MIN_READS, 1, 3)
    finally:
        d.close()


def test_the_reserved_slot_carries_over_a_growth(ref):
    """K = 32: the all-T barcode equals the table's empty mark and lives in the reserved slot"""
    rng = np.random.default_rng(502)
    a = [(ALL_T, 70), (ALL_T ^ 1, 9)] + [(v, 5) for v in ct.random_barcodes(rng, 12, 32)]
    b = [(ALL_T, 130), (ALL_T ^ (3 << 62), 11)] + [(v, 4) for v in ct.random_barcodes(rng, 60, 32)]
    ka, fa = ct.from_counts(a, rng, filtered_between=3)
    kb, fb = ct.from_counts(b, rng, filtered_between=3)
    one = OneShot(ref, np.concatenate([ka, kb]), np.concatenate([fa, fb]), 32)
    d = humid_amd.Dedup()
    try:
        d.set_option("cells_table_log2", 4)
        bc = d.barcode_counter(barcode_nt=32)
        bc.add(ka, fa)
        before = bc.info()["n_grown"]
        assert before >= 1                                           # (14 barcodes left 16 slots more than half full)
        bc.add(kb, fb)                                               # 60 new barcodes into at most 64 slots: a growth
        assert bc.info()["n_grown"] > before
        sm, got = one.check(d, bc, ct.MIN_READS, 5, 0)
        cells = dict(zip((int(x) for x in got[0]), (int(x) for x in got[1])))
        assert cells[ALL_T] == 200 and cells[ALL_T ^ 1] == 9 and cells[ALL_T ^ (3 << 62)] == 11
        sm, got = one.check(d, bc, ct.MIN_READS, 5, 5)               # all-T removes its two neighbours
        assert ALL_T in set(int(x) for x in got[0]) and sm["merged"] == 2
    finally:
        d.close()


def test_invalid_keys_and_special_chunks(dd, ref):
    keys, filt = skewed(503, p_invalid=0.03)
    one = OneShot(ref, keys, filt, 8)
    bc = dd.barcode_counter(barcode_nt=8)
    pieces = cut(len(keys), 500)
    n_invalid = 0
    for i, (a, b) in enumerate(pieces):
        bc.add(keys[a:b], filt[a:b])
        n_invalid += int(((keys[a:b] >= U64(4 ** 8)) & (filt[a:b] == 0)).sum())
        assert bc.info()["invalid_reads"] == n_invalid
        if i == 2:
            before = bc.info()
            bc.add(keys[:0], filt[:0])                                # a chunk of no reads
            bc.add(keys[:300], np.ones(300, np.uint8))                # a chunk of filtered reads only
            after = bc.info()
            assert after == dict(before, chunks=before["chunks"] + 2, reads=before["reads"] + 300)
    assert n_invalid > 30
    sm, got = one.check(dd, bc, ct.MIN_READS, 1, 0)                  # every barcode is a cell: none of them is an invalid key
    assert sm["invalid_reads"] == n_invalid and sm["cells"] == sm["distinct"] and int(got[0].max()) < 4 ** 8
    # (the one-shot reference saw none of the two special chunks: they changed nothing)
    one.check(dd, bc, ct.MIN_READS, 1, 3)


def test_a_heavily_duplicated_barcode(dd):
    bc = dd.barcode_counter(barcode_nt=8)
    bc.add(np.full(640, 0x1B2D, U64), np.zeros(640, np.uint8))      # ten waves, one run each
    sm = bc.finish(top=5)
    cells, reads = dd.discovered_cells()
    assert sm["distinct"] == 1 and sm["usable"] == 640 and list(cells) == [0x1B2D] and list(reads) == [640]
    assert bc.info()["distinct"] == 1


def test_finish_twice_and_add_after_a_finish(dd, ref):
    keys, filt = skewed(504)
    half = OneShot(ref, keys[:1400], filt[:1400], 8)
    whole = OneShot(ref, keys, filt, 8)
    bc = dd.barcode_counter(barcode_nt=8)
    feed(bc, keys, filt, cut(1400, 350))
    a, _ = half.check(dd, bc, ct.TOP, 25, 0)
    b, _ = half.check(dd, bc, ct.EXPECTED, 40, 3)                    # nothing added in between
    assert a["cells"] == 25 and a != b
    half.check(dd, bc, ct.TOP, 25, 0)
    feed(bc, keys, filt, [(1400, 2100), (2100, 3000)])
    whole.check(dd, bc, ct.EXPECTED, 40, 3)
    whole.check(dd, bc, ct.TOP, 25, 0)


def snapshot(d):
    return [d.leaves(), d.group_stats(), d.group_keys(), d.whitelist_info()]


def equal(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(equal(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(equal(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def test_the_counter_and_the_rest_of_the_context_leave_each_other_alone(dd, ref):
    keys, filt = skewed(505)
    other, ofilt = skewed(506, n=5000, n_cells=400)
    one = OneShot(ref, keys, filt, 8)
    # a one-shot discover over other data between two adds
    bc = dd.barcode_counter(barcode_nt=8)
    bc.add(keys[:1500], filt[:1500])
    dd.discover_whitelist(other, ofilt, barcode_nt=8, top=30, merge_ratio=2)
    oneshot_cells = dd.discovered_cells()
    bc.add(keys[1500:], filt[1500:])
    assert equal(dd.discovered_cells(), oneshot_cells)               # (an add installs nothing)
    one.check(dd, bc, ct.MIN_READS, 1, 3)
    # a keyed run's answers and a whitelist set by the caller: an add changes neither
    wl = np.unique(keys[filt == 0])[:50]
    dd.set_whitelist(wl, 8)
    words, wfilt = make_words(31, len(keys), 10)
    dd.run_keyed(words, keys & U64(0xFFFF), wfilt, word_nt=10)
    before = snapshot(dd)
    probe = np.concatenate([wl, wl ^ U64(1)])
    corrected = dd.correct_keys(probe, np.zeros(len(probe), np.uint8))
    bc = dd.barcode_counter(barcode_nt=8)
    bc.add(keys[:2000], filt[:2000])
    assert equal(before, snapshot(dd))
    assert equal(corrected, dd.correct_keys(probe, np.zeros(len(probe), np.uint8)))
    # a run and an accumulator's adds between two adds of the counter: the counter is as it was, and so is the accumulator
    dd.run_keyed(words, keys & U64(0xFFFF), wfilt, word_nt=10)
    acc = dd.keyed_accumulator(word_nt=10, key_nt=8)
    acc.add(words[:1000], keys[:1000] & U64(0xFFFF), wfilt[:1000])
    listed = acc.leaves()
    bc.add(keys[2000:], filt[2000:])
    assert equal(listed, acc.leaves())
    acc.add(words[1000:], keys[1000:] & U64(0xFFFF), wfilt[1000:])
    assert acc.info()["total"] == len(keys)
    one.check(dd, bc, ct.MIN_READS, 1, 3)
    acc.clear()


def raw(d, name, *args):
    return getattr(d._lib, name)(d._h, *args)


def test_states_and_refusals():
    d = humid_amd.Dedup()
    try:
        keys, filt = skewed(507, n=1000)
        vp = lambda a: C.c_void_p(a.ctypes.data)                     # noqa: E731
        sm = _lib.HumidCellsSummary()
        nt = C.c_uint32(77)
        none8 = [None] * 8
        # before begin
        assert raw(d, "humid_cells_add", vp(keys), vp(filt), len(keys)) == E_STATE
        assert raw(d, "humid_cells_add_device", None, None, 0) == E_STATE
        assert raw(d, "humid_cells_finish", 0, 5, 0, C.byref(sm)) == E_STATE
        assert raw(d, "humid_cells_info", C.byref(nt), *none8[:7]) == E_STATE and nt.value == 77
        assert raw(d, "humid_cells_clear") == E_STATE
        for k in (0, 33):
            assert raw(d, "humid_cells_begin", k) == E_INVALID
            assert raw(d, "humid_cells_add", vp(keys), vp(filt), len(keys)) == E_STATE
        # refusals leave the counter and the whitelist in place as they were
        bc = d.barcode_counter(barcode_nt=8)
        bc.add(keys, filt)
        want = bc.finish(top=10, merge_ratio=2)
        after = answers(d)
        info = bc.info()
        sm.cells = 12345
        for k in (0, 33):
            assert raw(d, "humid_cells_begin", k) == E_INVALID
        for args, code in (((3, 5, 0), E_INVALID), ((0, 0, 0), E_INVALID), ((1, 0, 2), E_INVALID)):
            assert raw(d, "humid_cells_finish", *args, C.byref(sm)) == code and sm.cells == 12345
        assert raw(d, "humid_cells_add", None, vp(filt), 5) == E_INVALID
        assert raw(d, "humid_cells_add", vp(keys), None, 5) == E_INVALID
        assert raw(d, "humid_cells_add", vp(keys), vp(filt), 2 ** 31) == E_OVERFLOW
        assert raw(d, "humid_cells_add_device", vp(keys), vp(filt), 2 ** 31) == E_OVERFLOW      # (refused on the host: never read)
        assert bc.info() == info and same(answers(d), after)
        assert bc.finish(top=10, merge_ratio=2) == want and same(answers(d), after)
        for kw in (dict(), dict(top=1, expected=2), dict(top=0), dict(top=1, merge_ratio=-1)):
            with pytest.raises(ValueError):
                bc.finish(**kw)
        # a finish that finds no cell clears the whitelist and answers
        sm0 = bc.finish(min_reads=10 ** 9)
        assert sm0["cells"] == 0 and sm0["distinct"] == want["distinct"] and d.whitelist_info() == dict(n_distinct=0, barcode_nt=0, table_log2=0)
        assert len(d.discovered_cells()[0]) == 0 and len(d.barcode_count_hist()[0]) > 0
        # begin empties the counter, clear ends it
        bc = d.barcode_counter(barcode_nt=8)
        assert bc.info() == dict(barcode_nt=8, chunks=0, reads=0, usable=0, invalid_reads=0, distinct=0, table_log2=16, n_grown=0)
        assert bc.finish(top=3)["distinct"] == 0                     # no reads: legal, zero cells
        bc.clear()
        with pytest.raises(humid_amd.HumidError) as ei:
            bc.add(keys, filt)
        assert ei.value.code == E_STATE
    finally:
        d.close()


def test_device_pointers(dd, reads3000):
    import torch
    keys, filt, one = reads3000
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    df = torch.from_numpy(filt).cuda()
    torch.cuda.synchronize()
    bc = dd.barcode_counter(barcode_nt=8)
    for a, b in cut(len(keys), 700):
        bc.add_device(dk.data_ptr() + 8 * a, df.data_ptr() + a, b - a)
    bc.add_device(0, 0, 0)
    one.check(dd, bc, ct.MIN_READS, 1, 3)
    assert np.array_equal(dk.cpu().numpy().view(U64), keys) and np.array_equal(df.cpu().numpy(), filt)
