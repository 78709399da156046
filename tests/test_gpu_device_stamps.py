"""-m gpu: the four times of a lean pass from device stamps (option device_stamps) instead of four event records.

On the record road (stage_count_rec: one-word words in word-ordered buckets of 8-byte records) a pass without
kernel_timing stores the 100 MHz wall clock at the entry of its first k_zero_many, of k_dedup_rec, of the scan behind it
and of its last k_publish_counters, and records no event: ms_total and ms_k_insert are differences of those stamps.
Dedup.stamp_info() says whether a call was timed that way, returns the raw stamps and counts the call's event records,
so the road is asserted and not assumed.  Every case runs with the option on and off and against the CPU oracle.

The main shape is 70 000 reads of 24 nt (eight bucket bits, 16 coarse bins); 3 000 reads lie below the record road
(350 << 5 = 11 200 reads), 40-nt words take the two-word count, a grouped run and a pass with kernel_timing keep their
events.  With kernel_timing = 1 the kernels store their stamps all the same and stamp_info() returns them beside the
summary's event times: the one mode that has both clocks, compared in test_stamps_against_events.

Runs go through run_device on torch tensors: the host-array entry points record four events of their own around
their copies, which stamp_info() counts as well."""
import time

import numpy as np
import pytest
import torch

import grouped_truth
import humid_amd
from humid_amd.synth import synth_wide_words, synth_words
from test_gpu_parity import oracle_full

pytestmark = pytest.mark.gpu

U64 = np.uint64
COUNTS = ("total", "usable", "unique", "clusters", "edges")
# test_stamps_against_events: the largest difference between a stamp interval and the same pass's event interval seen
# on the MI355X over this file's shapes (profiles/r04e_device_stamps.md), plus two markers' worth, 12 us: each end of
# an event interval can sit one marker away from the kernel entry that the stamp reads
OBSERVED_MS = {"ms_total": 0.0013, "ms_k_insert": 0.0001}
MARKERS_MS = 0.012


def context(stamps, timing=0):
    """word-ordered buckets forced: the default decides for them from 65 536 reads on only, and the record road is
    theirs"""
    d = humid_amd.Dedup()
    d.set_option("count_order", 1)
    d.set_option("device_stamps", stamps)
    d.set_option("kernel_timing", timing)
    return d


@pytest.fixture(scope="module")
def on():
    d = context(1)
    yield d
    d.close()


@pytest.fixture(scope="module")
def off():
    d = context(0)
    yield d
    d.close()


class Case:
    """an input on the device and its oracle results, computed once"""

    def __init__(self, words, filt, n, maximum):
        self.n, self.maximum = n, maximum
        self.N = len(filt)
        dev = torch.device("cuda:0")
        self.d_w = torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(dev)
        self.d_f = torch.from_numpy(np.ascontiguousarray(filt)).to(dev)
        p, self.cid, self.keep = oracle_full(words, filt, n, 1, maximum)
        self.summary = p.summary()


def run(dd, case):
    """one run_device: (cluster ids, keep flags, summary, stamp info, roads, wait info, host span in ms)"""
    dev = case.d_w.device
    d_cid = torch.zeros(case.N, dtype=torch.int32, device=dev)
    d_keep = torch.zeros(case.N, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = dd.run_device(case.d_w.data_ptr(), case.d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), case.N,
                      word_nt=case.n, distance=1, method=int(case.maximum))
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    info, roads, wo = dd.stamp_info(), dd.run_roads(), dd.wait_overlap_info()
    cid, keep = d_cid.cpu().numpy().view(np.uint32), d_keep.cpu().numpy()
    assert np.array_equal(cid, case.cid) and np.array_equal(keep, case.keep)
    for k in COUNTS:
        assert s[k] == case.summary[k], (k, s[k], case.summary[k])
    return cid, keep, s, info, roads, wo, host_ms


def both(on, off, case):
    """the run with the option on and off: results, roads and waits equal (each is checked against the oracle in run)"""
    a, b = run(on, case), run(off, case)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in COUNTS + ("count_mode_used", "records8"):
        assert a[2][k] == b[2][k], k
    assert a[4] == b[4], (a[4], b[4])
    assert a[5] == b[5], (a[5], b[5])
    return a, b


def stamp_times(info):
    t0, k0, k1, t1 = info["stamps"]
    return (t1 - t0) / 1e5, (k1 - k0) / 1e5


@pytest.fixture(scope="module")
def main_cases():
    words, filt = synth_words(70_000, 704, 24, p_sub=6e-3, p_n=1e-3)
    return {maximum: Case(words, filt, 24, maximum) for maximum in (False, True)}


# ---- the record road, lean ----

@pytest.mark.parametrize("maximum", [False, True])
def test_lean_pass_on_the_record_road(on, off, main_cases, maximum):
    case = main_cases[maximum]
    for rep in range(2):                                     # a context's first pass on a shape, and the steady state
        a, b = both(on, off, case)
        s, info, host_ms = a[2], a[3], a[6]
        print("on", info, s["ms_total"], s["ms_k_insert"], host_ms, "off", b[3], b[2]["ms_total"], b[2]["ms_k_insert"])
        assert s["records8"], s
        assert info["used"] and info["event_records"] == 0, info
        t0, k0, k1, t1 = info["stamps"]
        assert t0 <= k0 < k1 <= t1, info
        assert 0 < s["ms_k_insert"] <= s["ms_total"], s
        assert s["ms_total"] <= host_ms, (s["ms_total"], host_ms)          # (a wrong clock rate shows from above)
        tot, ins = stamp_times(info)
        assert abs(tot - s["ms_total"]) < 1e-6 and abs(ins - s["ms_k_insert"]) < 1e-6, (tot, ins, s)
        for k in ("ms_count", "ms_neighbours", "ms_cluster", "ms_map"):
            assert s[k] == 0, (k, s[k])
        s0, info0 = b[2], b[3]
        assert not info0["used"] and info0["event_records"] == 4 and info0["stamps"] == [0, 0, 0, 0], info0
        assert 0 < s0["ms_k_insert"] <= s0["ms_total"] <= b[6], (s0, b[6])


# ---- roads the stamps do not cover: events with either value ----

def uncovered(on, off, case):
    a, b = both(on, off, case)
    for r in (a, b):
        s, info = r[2], r[3]
        assert not info["used"], info
        assert 0 < s["ms_k_insert"] <= s["ms_total"], s
    assert a[3]["event_records"] == b[3]["event_records"] > 0, (a[3], b[3])
    return a, b


def test_below_the_record_road(on, off):
    words, filt = synth_words(3000, 22, 24, p_sub=2e-2, p_n=1e-3)
    for maximum in (False, True):
        a, b = uncovered(on, off, Case(words, filt, 24, maximum))
        assert not a[2]["records8"] and a[3]["event_records"] == 4 and a[3]["stamps"] == [0, 0, 0, 0], (a[2], a[3])


def test_two_word_shape(on, off):
    words, filt = synth_wide_words(70_000, 948, 40, p_sub=4e-3, p_n=1e-3)
    for maximum in (False, True):
        a, b = uncovered(on, off, Case(words, filt, 40, maximum))
        assert a[3]["event_records"] == 4 and a[3]["stamps"] == [0, 0, 0, 0], a[3]


@pytest.mark.parametrize("method", [0, 1])
def test_grouped_run(on, off, method):
    words, filt = synth_words(70_000, 705, 24, p_sub=6e-3, p_n=1e-3)
    groups = (np.arange(len(words)) % 3).astype(np.uint32)
    t = grouped_truth.per_group(words, groups, filt, 24, 1, method, first_read=False)
    got = []
    for dd in (on, off):
        cid, keep, s = dd.run_grouped(words, groups, filt, word_nt=24, n_groups=3, distance=1, method=method)
        info = dd.stamp_info()
        assert np.array_equal(cid, t["cid"]) and np.array_equal(keep, t["keep"])
        for k in COUNTS:
            assert s[k] == t["summary"][k], (k, s[k], t["summary"][k])
        assert not info["used"] and info["stamps"] == [0, 0, 0, 0], info
        assert 0 < s["ms_k_insert"] <= s["ms_total"], s
        got.append((info["event_records"], dd.run_roads(), dd.wait_overlap_info()))
    assert got[0] == got[1] and got[0][0] > 0, got


# ---- kernel_timing = 1: both clocks in one pass ----

@pytest.fixture(scope="module")
def timed_both():
    a, b = context(1, timing=1), context(0, timing=1)
    yield a, b
    a.close()
    b.close()


@pytest.mark.parametrize("maximum", [False, True])
def test_stamps_against_events(timed_both, main_cases, maximum):
    """the events are the yardstick: with kernel_timing the summary's times are theirs, and the stamps the same pass's
    kernels stored must give the same two intervals"""
    a_ctx, b_ctx = timed_both
    case = main_cases[maximum]
    for rep in range(3):
        a, b = uncovered(a_ctx, b_ctx, case)
        s, info = a[2], a[3]
        assert s["records8"] and s["ms_count"] > 0 and s["ms_map"] > 0, s
        assert a[3]["event_records"] > 4, a[3]
        t0, k0, k1, t1 = info["stamps"]
        assert t0 <= k0 < k1 <= t1, info
        assert b[3]["stamps"] == [0, 0, 0, 0], b[3]
        tot, ins = stamp_times(info)
        d_tot, d_ins = tot - s["ms_total"], ins - s["ms_k_insert"]
        print("stamps vs events: ms_total %.4f %.4f (%+.4f)  ms_k_insert %.4f %.4f (%+.4f)"
              % (tot, s["ms_total"], d_tot, ins, s["ms_k_insert"], d_ins))
        assert abs(d_tot) <= OBSERVED_MS["ms_total"] + MARKERS_MS, (tot, s["ms_total"])
        assert abs(d_ins) <= OBSERVED_MS["ms_k_insert"] + MARKERS_MS, (ins, s["ms_k_insert"])


# ---- a count that is discarded and taken again ----

def test_padded_partition_outgrown_by_duplicated_words():
    """the input of tests/test_gpu_parity.py's test of that name: a third of 600 000 reads are one word, its coarse bin
    outgrows its room, the record count is discarded (PART_PADDED_REDO) and taken again by the exact partition -- which
    records its events: the pass's four times are all theirs"""
    rng = np.random.default_rng(77)
    words, filt = synth_words(600_000, 9, 24, p_sub=3e-3, p_n=1e-3)
    hot = rng.random(len(words)) < 0.35
    words = words.copy()
    words[hot] = np.uint64(0x0123456789ab)
    case = Case(words, filt, 24, False)
    a_ctx, b_ctx = context(1), context(0)
    try:
        a, b = both(a_ctx, b_ctx, case)
        for r in (a, b):
            s, info, roads = r[2], r[3], r[4]
            assert roads["events"].count("PART_PADDED_REDO") == 1, roads
            assert not s["records8"] and not info["used"], (s, info)
            assert 0 < s["ms_k_insert"] <= s["ms_total"] <= r[6], (s, r[6])
        # (the count that is taken again records its four; the discarded one three more, and none with stamps)
        assert a[3]["event_records"] == 4 and b[3]["event_records"] == 7, (a[3], b[3])
        a, b = both(a_ctx, b_ctx, case)                      # the context remembers: the exact partition at once
        for r in (a, b):
            assert "PART_PADDED_REDO" not in r[4]["events"] and not r[3]["used"], (r[4], r[3])
            assert 0 < r[2]["ms_k_insert"] <= r[2]["ms_total"], r[2]
        assert a[3]["event_records"] == b[3]["event_records"] == 4, (a[3], b[3])
    finally:
        a_ctx.close()
        b_ctx.close()
