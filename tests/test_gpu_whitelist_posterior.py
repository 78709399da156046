"""-m gpu: barcode correction by quality and abundance (humid_whitelist_correct_posterior*,
humid_dedup_run_keyed_posterior*, humid_whitelist_counts) against the truths of tests/whitelist_posterior_truth.py,
bit for bit, in both forms of the decision kernel (option "whitelist_coop"): key_out, status, the summary and the reads
per barcode of the stand-alone call; the posterior run against run_keyed on the truth's key_out and filtered'; the
state rules of the context; the device-pointer forms."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib

import whitelist_posterior_truth as pt
import whitelist_truth as wt
from test_gpu_keyed import make_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP = wt.TOP
E_STATE, E_INVALID = -6, -1
GUARD = 0xA5A5A5A5A5A5A5A5


class GuardedSummary(C.Structure):
    _fields_ = [("s", _lib.HumidBcPosteriorSummary), ("guard", C.c_uint64 * 2)]


@pytest.fixture(scope="module", params=[1, 0], ids=["wave_cooperative", "lane_serial"])
def dd(request):
    """the two forms of the decision kernel (option "whitelist_coop")"""
    d = humid_amd.Dedup()
    d.set_option("whitelist_coop", request.param)
    yield d
    d.close()


def raw_posterior(d, keys, quals, filt, min_odds=39):
    """humid_whitelist_correct_posterior through the C ABI with guard words behind every output"""
    keys = np.ascontiguousarray(keys, U64)
    filt = np.ascontiguousarray(filt, np.uint8)
    quals = np.ascontiguousarray(quals, np.uint8)
    n = len(filt)
    out = np.full(n + 8, GUARD, U64)
    status = np.full(n + 16, 0xA5, np.uint8)
    sm = GuardedSummary()
    sm.guard[0] = sm.guard[1] = GUARD
    vp = lambda a: C.c_void_p(a.ctypes.data)                        # noqa: E731
    d._check(d._lib.humid_whitelist_correct_posterior(d._h, vp(keys), vp(quals), vp(filt), n, min_odds, vp(out), vp(status),
                                                      C.cast(C.byref(sm), C.POINTER(_lib.HumidBcPosteriorSummary))))
    assert np.all(out[n:] == U64(GUARD)) and np.all(status[n:] == 0xA5) and list(sm.guard) == [GUARD, GUARD]
    return out[:n], status[:n], sm.s.asdict()


def check_counts(d, wl, n_w, extra=()):
    """whitelist_counts for the whole whitelist, duplicates as given, and values it does not hold, with a guard"""
    ask = np.concatenate([np.asarray(wl, U64), np.asarray(list(extra), U64)]).astype(U64)
    out = np.full(len(ask) + 4, 0xA5A5A5A5, np.uint32)
    d._check(d._lib.humid_whitelist_counts(d._h, C.c_void_p(ask.ctypes.data), len(ask), C.c_void_p(out.ctypes.data)))
    assert np.all(out[len(ask):] == 0xA5A5A5A5)
    W = set(int(w) for w in wl)
    want = [n_w.get(int(b), 0) if int(b) in W else 0 for b in ask]
    assert list(out[:len(ask)]) == want
    assert np.array_equal(d.whitelist_counts(ask), out[:len(ask)])


def check(d, keys, quals, filt, wl, k, min_odds=39, expect=None, outcomes=False):
    """the device against the truth; expect: statuses the TRUTH must contain; outcomes: it rescues some, not all"""
    t = pt.posterior_np(keys, quals, filt, wl, k, min_odds)
    if expect is not None:
        assert wt.status_set(t[1]) >= set(expect), (wt.status_set(t[1]), expect)
    if outcomes:
        assert 0 < t[2]["rescued"] < t[2]["multi"], t[2]
    got = raw_posterior(d, keys, quals, filt, min_odds)
    assert got[0].dtype == t[0].dtype and np.array_equal(got[0], t[0]), "key_out"
    assert np.array_equal(got[1], t[1]), "status"
    assert got[2] == t[2], (got[2], t[2])
    check_counts(d, wl, t[3], extra=[int(keys[0]) ^ 1] if len(keys) else [12345])
    return t


@pytest.mark.parametrize("k", [1, 2, 16, 21, 22, 32])
def test_barcode_lengths_and_read_counts(dd, k):
    """21 and 22 nt are 63 and 66 variants: the wave boundary of the variant rounds.  Quality bytes below 33 and above
    126, keys with bits above 2 K and garbage under filtered reads come from the generator."""
    rng = np.random.default_rng(300 + k)
    n_wl = {1: 2, 2: 5}.get(k, 400)
    for n in (0, 1, 63, 64, 65, 257, 100_000):
        wl, keys, quals, filt = pt.make_case(rng, n, k, n_wl=n_wl)
        if k == 32:
            wl[5] = TOP                                             # the all-T barcode: the table's empty mark
            wl[6] = TOP ^ U64(2 << 10)                              # and a neighbour of it
            if n >= 257:
                keys[3:6] = TOP                                     # exact, counted in the reserved slot
                keys[6:9] = TOP ^ U64(1)                            # all-T as a candidate
                keys[9] = TOP ^ U64(1 << 10)                        # all-T and its neighbour as candidates
                filt[3:10] = 0
        dd.set_whitelist(wl, k)
        big = n == 100_000
        t = check(dd, keys, quals, filt, wl, k, expect={0, 1, 2, 3, 4} if big and k >= 16 else None, outcomes=big and k >= 16)
        if k == 32 and n >= 257:
            assert t[3][TOP] >= 3 and list(t[1][3:6]) == [1, 1, 1] and int(t[1][6]) == 2 and int(t[0][6]) == TOP
    # other odds
    wl, keys, quals, filt = pt.make_case(rng, 5000, k, n_wl=n_wl)
    dd.set_whitelist(wl, k)
    for min_odds in (1, 2, 1000, (1 << 32) - 1):
        check(dd, keys, quals, filt, wl, k, min_odds=min_odds)


@pytest.mark.parametrize("case", pt.hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(dd, case):
    dd.set_whitelist(case["whitelist"], case["k"])
    out, status, sm = raw_posterior(dd, case["keys"], case["quals"], case["filtered"], case["min_odds"])
    assert int(status[-1]) == case["status"] and int(out[-1]) == case["key_out"]
    assert np.all(status[:-1] == pt.EXACT) and sm["multi"] == 1 and sm["rescued"] == (case["status"] == pt.CORRECTED)
    check(dd, case["keys"], case["quals"], case["filtered"], case["whitelist"], case["k"], case["min_odds"])
    # the query in front, in a wave of its own, in the middle of a wave
    for at in (0, 64, 31):
        if at < len(case["keys"]):
            order = np.r_[np.arange(len(case["keys"]) - 1), len(case["keys"]) - 1]
            order = np.r_[order[:at], order[-1], order[at:-1]]
            o2, s2, _ = raw_posterior(dd, case["keys"][order], case["quals"][order], case["filtered"][order], case["min_odds"])
            assert int(s2[at]) == case["status"] and int(o2[at]) == case["key_out"]


def test_bits_above_2k_and_exact_beside_a_neighbour(dd):
    AA, AC, AG = pt.key_of("AA"), pt.key_of("AC"), pt.key_of("AG")
    keys = np.asarray([AA | 16, AG | 16, AC, AG], U64)
    q = np.full((4, 2), 70, np.uint8)
    dd.set_whitelist([AA, AC], 2)
    # AG has AA and AC one substitution away, both at nucleotide 1; AC holds one exact read: 2 : 1
    out, status, sm = raw_posterior(dd, keys, q, np.zeros(4, np.uint8))
    assert list(status) == [4, 4, 1, 3] and list(out) == [AA | 16, AG | 16, AC, AG]
    assert sm == dict(counts=[0, 1, 0, 1, 2], multi=1, rescued=0) and list(dd.whitelist_counts([AA, AC, AG])) == [0, 1, 0]
    out, status, sm = raw_posterior(dd, keys, q, np.zeros(4, np.uint8), min_odds=2)
    assert list(status) == [4, 4, 1, 2] and int(out[3]) == AC and sm["rescued"] == 1


def test_wave_patterns(dd):
    rng = np.random.default_rng(13)
    for k in (16, 22):
        wl = wt.whitelist_with_neighbours(rng, 3000, k)
        mids = wt.midpoints(wl, k)
        assert len(mids)
        dd.set_whitelist(wl, k)
        n = 64 * 40 + 17
        none = np.zeros(n, np.uint8)
        quals = rng.integers(33, 74, size=(n, k), dtype=np.uint8)
        # every lane of every wave misses: midpoints and substitutions (no exact read at all), random keys
        keys = np.where(rng.random(n) < 0.5, mids[rng.integers(0, len(mids), size=n)],
                        wt.substitute(rng, wl[rng.integers(0, len(wl), size=n)], k))
        check(dd, keys, quals, none, wl, k, expect={2, 3})
        check(dd, wt.random_barcodes(rng, n, k), quals, none, wl, k, expect={4})
        # exactly one lane of a wave misses: lane 0, lane 63
        for lane in (0, 63):
            keys = wl[rng.integers(0, len(wl), size=n)]
            at = np.arange(lane, n, 64)
            keys[at] = mids[rng.integers(0, len(mids), size=len(at))]
            check(dd, keys, quals, none, wl, k, expect={1}, outcomes=True)
        # around the number of missing lanes at which the cooperative kernel hands a wave to the lane-serial walk
        edge = 3 * k // ((3 * k + 63) // 64)
        for m in (edge - 1, edge, edge + 1):
            keys = wl[rng.integers(0, len(wl), size=n)]
            at = np.flatnonzero(np.arange(n) % 64 < m)
            keys[at] = mids[rng.integers(0, len(mids), size=len(at))]
            keys[at[::5]] = wt.substitute(rng, wl[rng.integers(0, len(wl), size=len(at[::5]))], k)
            check(dd, keys, quals, none, wl, k, expect={1, 2, 3})
        # runs of equal missing keys with different qualities: every read is a query of its own
        keys = np.repeat(mids[rng.integers(0, len(mids), size=n // 32 + 1)], 32)[:n]
        keys[::7] = wl[3]
        t = check(dd, keys, quals, none, wl, k, outcomes=True)
        first = np.flatnonzero(keys == keys[1])
        assert len(set(int(s) for s in t[1][first])) == 2               # one key, both outcomes
        # keys with bits above 2 K: unmatched, whatever lies below
        keys = mids[rng.integers(0, len(mids), size=n)]
        high = rng.random(n) < 0.3
        keys = np.where(high, keys | (U64(1) << U64(2 * k + rng.integers(0, 64 - 2 * k))), keys)
        t = check(dd, keys, quals, none, wl, k)
        assert np.all(t[1][high] == 4)
        # everything filtered: garbage keys and quality rows are not read
        t = check(dd, rng.integers(0, 1 << 64, size=n, dtype=U64), rng.integers(0, 256, size=(n, k), dtype=np.uint8),
                  np.ones(n, np.uint8), wl, k, expect={0})
        assert t[2]["counts"][0] == n and not t[0].any() and t[3] == {}


def test_one_barcode_holds_every_read(dd):
    """the run head adds its run's length with one atomic: 100 000 reads of one key, whole and broken by filtered reads"""
    rng = np.random.default_rng(17)
    k = 16
    wl = wt.whitelist_with_neighbours(rng, 500, k)
    dd.set_whitelist(wl, k)
    n = 100_000
    keys = np.full(n, wl[7], U64)
    quals = np.full((n, k), 70, np.uint8)
    filt = np.zeros(n, np.uint8)
    t = check(dd, keys, quals, filt, wl, k)
    assert t[3] == {int(wl[7]): n} and int(dd.whitelist_counts(wl[7:8])[0]) == n
    filt[::5] = 1
    filt[1000:1100] = 1
    keys[-1] = wl[7] ^ U64(3)                                            # the one query: the prior of 10^5 reads decides
    filt[-1] = 0
    t = check(dd, keys, quals, filt, wl, k)
    assert t[3] == {int(wl[7]): int((filt == 0).sum()) - 1} and int(t[1][-1]) == pt.CORRECTED


def test_equal_qualities_and_no_exact_read_are_the_plain_correction(dd):
    rng = np.random.default_rng(19)
    for k in (16, 22):
        wl, keys, quals, filt = pt.make_case(rng, 20_000, k, n_wl=500)
        dd.set_whitelist(wl, k)
        plain = dd.correct_keys(keys, filt)
        # the superset rule: other statuses only where the plain correction is ambiguous
        out, status, counts, sm = dd.correct_keys(keys, filt, quals=quals)
        assert pt.plain_from_posterior(plain[1], status) and (plain[1] != status).any()
        assert sm["multi"] == int(plain[2][wt.AMBIGUOUS]) and sm["rescued"] == int((plain[1] != status).sum())
        assert np.array_equal(counts, np.asarray(sm["counts"], U64))
        one = plain[1] == wt.CORRECTED
        assert np.array_equal(out[one], plain[0][one])
        # no exact read, equal bytes, min_odds >= 2: bit for bit
        f2 = filt.copy()
        f2[np.isin(keys, wl)] = 1
        plain = dd.correct_keys(keys, f2)
        for byte, min_odds in ((60, 39), (33, 2), (255, 39), (0, 1000)):
            out, status, counts, sm = dd.correct_keys(keys, f2, quals=np.full_like(quals, byte), min_odds=min_odds)
            assert np.array_equal(out, plain[0]) and np.array_equal(status, plain[1]) and np.array_equal(counts, plain[2])
            assert sm["rescued"] == 0 and sm["multi"] == int(plain[2][wt.AMBIGUOUS]) > 0
            assert not dd.whitelist_counts(wl).any()


def run_inputs(seed, n_reads, word_nt, k=16, n_wl=60):
    rng = np.random.default_rng(seed)
    wl, keys, quals, _ = pt.make_case(rng, n_reads, k, n_wl=n_wl, p_filt=0.0)
    words, filt = make_words(seed + 1, n_reads, word_nt)
    sel = np.flatnonzero(filt)
    keys[sel] = rng.integers(0, 1 << 64, size=len(sel), dtype=U64)      # filtered reads carry garbage
    quals[sel] = rng.integers(0, 256, size=(len(sel), k), dtype=np.uint8)
    return wl, words, keys, quals, filt


def full_result(d, words, keys, filt, word_nt, distance, method, **kw):
    cid, keep, s = d.run_keyed(words, keys, filt, word_nt=word_nt, distance=distance, method=method, **kw)
    off, idx = d.adjacency()
    s = {x: s[x] for x in ("total", "usable", "unique", "clusters", "edges")}
    return dict(cid=cid, keep=keep, summary=s, leaves=d.leaves(), off=off, idx=idx, K=d.group_keys(), stats=d.group_stats())


def same_result(a, b):
    assert np.array_equal(a["cid"], b["cid"]) and np.array_equal(a["keep"], b["keep"]) and a["summary"] == b["summary"]
    assert np.array_equal(a["off"], b["off"]) and np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["K"], b["K"])
    for part in ("leaves", "stats"):
        assert a[part].keys() == b[part].keys()
        for name in a[part]:
            assert np.array_equal(a[part][name], b[part][name]), (part, name)


@pytest.mark.parametrize("word_nt", [24, 40])
def test_posterior_run(dd, word_nt):
    """run_keyed(correct=True, barcode_quals=...) == run_keyed on the truth's key_out and filtered', array for array"""
    k = 16
    wl, words, keys, quals, filt = run_inputs(word_nt, 4000, word_nt)
    dd.set_whitelist(wl, k)
    other = humid_amd.Dedup()
    try:
        for min_odds in (39, 1):
            t_key, t_status, t_sm, t_nw = pt.posterior(keys, quals, filt, wl, k, min_odds)
            assert wt.status_set(t_status) >= ({0, 1, 2, 4} if min_odds == 1 else {0, 1, 2, 3, 4})
            assert 0 < t_sm["rescued"] and (min_odds == 1 or t_sm["rescued"] < t_sm["multi"])
            filt2 = ((filt != 0) | (t_status >= 3)).astype(np.uint8)
            for distance, method in ((0, 0), (1, 0), (0, 1), (1, 1)):
                got = full_result(dd, words, keys, filt, word_nt, distance, method, correct=True, barcode_quals=quals, min_odds=min_odds)
                status, counts = dd.barcode_status()
                assert np.array_equal(status, t_status) and [int(c) for c in counts] == t_sm["counts"]
                assert dd.barcode_posterior() == dict(multi=t_sm["multi"], rescued=t_sm["rescued"])
                assert np.all(np.isin(got["K"], wl)) and got["summary"]["usable"] == t_sm["counts"][1] + t_sm["counts"][2]
                check_counts(dd, wl, t_nw)
                want = full_result(other, words, t_key, filt2, word_nt, distance, method)
                same_result(want, got)
    finally:
        other.close()


def test_state_rules():
    d = humid_amd.Dedup()
    try:
        wl, words, keys, quals, filt = run_inputs(31, 2000, 24)
        # no whitelist: HUMID_E_STATE, and the context stays usable
        for call in (lambda: d.correct_keys(keys, filt, quals=quals),
                     lambda: d.run_keyed(words, keys, filt, correct=True, barcode_quals=quals),
                     lambda: d.whitelist_counts(wl)):
            with pytest.raises(humid_amd.HumidError) as ei:
                call()
            assert ei.value.code == E_STATE
        d.set_whitelist(wl, 16)
        # whitelist_counts before any posterior call; barcode_posterior after a plain corrected run
        with pytest.raises(humid_amd.HumidError) as ei:
            d.whitelist_counts(wl)
        assert ei.value.code == E_STATE
        d.run_keyed(words, keys, filt, word_nt=24, correct=True)
        with pytest.raises(humid_amd.HumidError) as ei:
            d.barcode_posterior()
        assert ei.value.code == E_STATE
        plain_status = d.barcode_status()[0]
        # refusals of the library itself: min_odds 0, null buffers with reads; no reads at all is fine
        vp = lambda a: C.c_void_p(a.ctypes.data)                    # noqa: E731
        lib, n = d._lib, len(filt)
        assert lib.humid_whitelist_correct_posterior(d._h, vp(keys), vp(quals), vp(filt), n, 0, None, None, None) == E_INVALID
        assert lib.humid_whitelist_correct_posterior(d._h, None, vp(quals), vp(filt), n, 39, None, None, None) == E_INVALID
        assert lib.humid_whitelist_correct_posterior(d._h, vp(keys), None, vp(filt), n, 39, None, None, None) == E_INVALID
        assert lib.humid_whitelist_correct_posterior(d._h, vp(keys), vp(quals), None, n, 39, None, None, None) == E_INVALID
        assert lib.humid_whitelist_correct_posterior_device(d._h, None, None, None, n, 39, None, None, None) == E_INVALID
        assert lib.humid_whitelist_correct_posterior(d._h, None, None, None, 0, 39, None, None, None) == 0
        assert lib.humid_whitelist_correct_posterior(d._h, vp(keys), vp(quals), vp(filt), n, 39, None, None, None) == 0   # every output null
        cid, keep = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        assert lib.humid_dedup_run_keyed_posterior(d._h, vp(words), vp(keys), vp(quals), vp(filt), n, 24, 1, 0, 0, vp(cid), vp(keep),
                                                   None) == E_INVALID
        assert lib.humid_dedup_run_keyed_posterior(d._h, vp(words), vp(keys), None, vp(filt), n, 24, 1, 0, 39, vp(cid), vp(keep),
                                                   None) == E_INVALID
        # the stand-alone call between a run and its accessors does not disturb them
        t = pt.posterior(keys, quals, filt, wl, 16)
        d.run_keyed(words, keys, filt, word_nt=24, correct=True, barcode_quals=quals)
        before = (d.leaves(), d.barcode_status(), d.group_keys(), d.barcode_posterior())
        assert np.array_equal(before[1][0], t[1]) and (before[1][0] != plain_status).any()
        rng = np.random.default_rng(1)
        o_wl, o_keys, o_quals, o_filt = pt.make_case(rng, 777, 16, n_wl=60)
        o = d.correct_keys(wl[rng.integers(0, len(wl), size=777)], o_filt, quals=o_quals)
        after = (d.leaves(), d.barcode_status(), d.group_keys(), d.barcode_posterior())
        for name in before[0]:
            assert np.array_equal(before[0][name], after[0][name]), name
        assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])
        assert np.array_equal(before[2], after[2]) and before[3] == after[3] == dict(multi=t[2]["multi"], rescued=t[2]["rescued"])
        # ... while whitelist_counts follows the later of the two
        assert int(d.whitelist_counts(np.unique(wl)).sum()) == o[3]["counts"][1] == int((o_filt == 0).sum())
        # a posterior run is a corrected keyed run for the accessors; a plain corrected run after it is not a posterior one
        assert d.keyed_rank_info()["n_keys"] == len(after[2])
        d.run_keyed(words, keys, filt, word_nt=24, correct=True)
        assert np.array_equal(d.barcode_status()[0], plain_status)
        with pytest.raises(humid_amd.HumidError) as ei:
            d.barcode_posterior()
        assert ei.value.code == E_STATE
        d.run(words, filt, word_nt=24)
        for call in (d.barcode_posterior, d.barcode_status):
            with pytest.raises(humid_amd.HumidError) as ei:
                call()
            assert ei.value.code == E_STATE
        # the reads per barcode go with the whitelist they index
        d.correct_keys(keys, filt, quals=quals)
        assert int(d.whitelist_counts(wl[:1])[0]) == t[3].get(int(wl[0]), 0)
        d.set_whitelist(wl[:30], 16)
        with pytest.raises(humid_amd.HumidError) as ei:
            d.whitelist_counts(wl[:30])
        assert ei.value.code == E_STATE
    finally:
        d.close()


def test_device_entry_points(dd):
    import torch
    wl, words, keys, quals, filt = run_inputs(41, 30_000, 28, n_wl=500)
    dd.set_whitelist(wl, 16)
    t_key, t_status, t_sm, t_nw = pt.posterior_np(keys, quals, filt, wl, 16)
    filt2 = ((filt != 0) | (t_status >= 3)).astype(np.uint8)
    n = len(filt)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_k = torch.from_numpy(keys.view(np.int64)).to(dev)
    d_q = torch.from_numpy(quals).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_ko = torch.zeros(n + 8, dtype=torch.int64, device=dev)
    d_st = torch.full((n + 16,), 9, dtype=torch.uint8, device=dev)
    d_cid = torch.zeros(n, dtype=torch.int32, device=dev)
    d_keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    sm = dd.correct_keys_posterior_device(d_k.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_ko.data_ptr(), d_st.data_ptr(), n)
    assert sm == t_sm
    ko, st = d_ko.cpu().numpy().view(U64), d_st.cpu().numpy()
    assert np.array_equal(ko[:n], t_key) and np.array_equal(st[:n], t_status) and not ko[n:].any() and np.all(st[n:] == 9)
    assert dd.correct_keys_posterior_device(d_k.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0, n) == t_sm
    check_counts(dd, wl, t_nw)
    s = dd.run_keyed_posterior_device(d_w.data_ptr(), d_k.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(),
                                      d_keep.data_ptr(), n, word_nt=28, distance=1)
    other = humid_amd.Dedup()
    try:
        cid, keep, s2 = other.run_keyed(words, t_key, filt2, word_nt=28, distance=1)
        assert np.array_equal(d_cid.cpu().numpy().view(np.uint32), cid) and np.array_equal(d_keep.cpu().numpy(), keep)
        assert s["clusters"] == s2["clusters"] and s["usable"] == t_sm["counts"][1] + t_sm["counts"][2]
        assert np.array_equal(dd.group_keys(), other.group_keys())
    finally:
        other.close()
    for a, b in ((d_k, keys.view(np.int64)), (d_q, quals), (d_f, filt)):                                   # inputs untouched
        assert np.array_equal(a.cpu().numpy(), b)
    status, counts = dd.barcode_status()
    assert np.array_equal(status, t_status) and [int(c) for c in counts] == t_sm["counts"]
    assert dd.barcode_posterior() == dict(multi=t_sm["multi"], rescued=t_sm["rescued"])
