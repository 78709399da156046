"""-m gpu: what a pass records of its own timing, on every count road in turn -- the twelve steps of
tests/test_gpu_count_record.py (every count road, the two inputs without a usable read, the long-word run) in ONE context
per configuration of (kernel_timing, device_stamps, entry points, HUMID_ALL_EVENTS), so that a flag the pass before left
set shows in the next pass's event records or in its summary.

Every step asserts
  - the results: cluster ids, keep flags and the summary counts equal the oracle's;
  - the event records: stamp_info()'s event_records and used equal RECORDS below;
  - the pattern: the set of ms_* summary fields that are not zero equals NONZERO below;
  - with kernel_timing 1, the order of the events: 0 < ms_k_insert <= ms_count <= ms_total, and the four stage times
    add up to ms_total within SUM_TOL.
RECORDS, NONZERO and SUM_TOL are not worked out from the code: they are what this file printed in table mode
(HUMID_PASS_TIMING_TABLE=1 pytest -s) on the commit before the pass's timing was gathered into one record, see
profiles/r05b_pass_timing.md.  The counter is an integer kept on the host: no margin.

The dense stage sequence (humid_stage_count_dense -> humid_stage_map_dense -> humid_stage_kernel_ms) runs on one rank
with kernel_timing 0 and 1."""
import os

import numpy as np
import pytest
import torch

import humid_amd
from test_gpu_count_record import COUNTS, STEPS, inputs  # noqa: F401  (inputs: the module's fixture, with the references)
from test_gpu_exchange import run_ranks

pytestmark = pytest.mark.gpu

TABLE_MODE = bool(os.environ.get("HUMID_PASS_TIMING_TABLE"))
MS = ("ms_count", "ms_neighbours", "ms_cluster", "ms_map", "ms_total", "ms_h2d", "ms_d2h", "ms_k_insert", "ms_k_pairs",
      "ms_k_cluster", "ms_k_map", "ms_k_part", "ms_k_unperm")

# name -> (kernel_timing, device_stamps, host entry points, HUMID_ALL_EVENTS)
CONFIGS = {
    "lean_stamps": (0, 1, False, False),
    "lean_events": (0, 0, False, False),
    "kernel_timing": (1, 1, False, False),
    "host_arrays": (0, 1, True, False),
    "all_events": (0, 1, False, True),
}

# the sets of non-zero ms_* fields, by letter
_STAGES = ("ms_count", "ms_neighbours", "ms_cluster", "ms_map", "ms_total")
PATTERNS = {
    "A": ("ms_total", "ms_k_insert"),
    "B": (),
    "C": _STAGES + ("ms_k_insert", "ms_k_pairs", "ms_k_cluster", "ms_k_map", "ms_k_part", "ms_k_unperm"),
    "D": _STAGES + ("ms_k_insert", "ms_k_pairs", "ms_k_cluster", "ms_k_map"),
    "E": _STAGES + ("ms_k_insert", "ms_k_pairs", "ms_k_cluster", "ms_k_map", "ms_k_unperm"),
    "F": _STAGES + ("ms_k_insert", "ms_k_map"),
    "G": ("ms_total", "ms_h2d", "ms_d2h", "ms_k_insert"),
    "H": ("ms_h2d", "ms_d2h"),
}
# per configuration and step: (event_records, used, pattern) -- read off the parent (c14a526), two runs, the same in both
T, F = True, False
RECORDS = {
    "lean_stamps": [(0, T, "A"), (4, F, "A"), (4, F, "A"), (4, F, "A"), (4, F, "A"), (4, F, "A"), (4, F, "A"), (3, F, "B"), (0, T, "A"),
                    (3, F, "B"), (4, F, "A"), (0, T, "A")],
    "lean_events": [(4, F, "A"), (4, F, "A"), (4, F, "A"), (4, F, "A"), (4, F, "A"), (4, F, "A"), (4, F, "A"), (3, F, "B"), (4, F, "A"),
                    (3, F, "B"), (4, F, "A"), (4, F, "A")],
    "kernel_timing": [(25, F, "C"), (13, F, "D"), (15, F, "E"), (17, F, "C"), (17, F, "C"), (11, F, "F"), (17, F, "C"), (6, F, "B"),
                      (17, F, "C"), (4, F, "B"), (17, F, "C"), (17, F, "C")],
    "host_arrays": [(4, T, "G"), (8, F, "G"), (8, F, "G"), (8, F, "G"), (8, F, "G"), (8, F, "G"), (8, F, "G"), (7, F, "H"), (4, T, "G"),
                    (7, F, "H"), (8, F, "G"), (4, T, "G")],
    "all_events": [(8, F, "F"), (7, F, "F"), (8, F, "F"), (8, F, "F"), (8, F, "F"), (8, F, "F"), (8, F, "F"), (4, F, "B"), (8, F, "F"),
                   (4, F, "B"), (8, F, "F"), (8, F, "F")],
}
# ms: twice the largest |ms_count + ms_neighbours + ms_cluster + ms_map - ms_total| the parent showed over the steps with
# kernel_timing 1 (2.2351741790771484e-08: the four times share their end events, the rest is the rounding to float)
SUM_TOL = 2 * 2.2351741790771484e-08


def run_step(dd, host, words, filt, n):
    if host:
        if n > 64:
            return dd.run_long(words, filt, n, distance=1, method=0)
        return dd.run(words, filt, word_nt=n, distance=1, method=0)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_cid = torch.zeros(len(filt), dtype=torch.int32, device=dev)
    d_keep = torch.zeros(len(filt), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    run = dd.run_long_device if n > 64 else dd.run_device
    s = run(d_w.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), len(filt), word_nt=n, distance=1, method=0)
    torch.cuda.synchronize()
    return d_cid.cpu().numpy().view(np.uint32), d_keep.cpu().numpy(), s


@pytest.mark.parametrize("config", list(CONFIGS))
def test_pass_timing_on_every_road(inputs, config, monkeypatch):  # noqa: F811
    timing, stamps, host, all_events = CONFIGS[config]
    if all_events:
        monkeypatch.setenv("HUMID_ALL_EVENTS", "1")
    dd = humid_amd.Dedup(device=0)
    seen, worst = [], 0.0
    try:
        dd.set_option("kernel_timing", timing)
        dd.set_option("device_stamps", stamps)
        for step, (name, options, mode, rec8) in enumerate(STEPS, 1):
            words, filt, n, t = inputs[name]
            for key, value in options.items():
                dd.set_option(key, value)
            cid, keep, s = run_step(dd, host, words, filt, n)
            for k in COUNTS:
                assert s[k] == t["summary"][k], (step, k, s[k], t["summary"][k])
            assert (s["count_mode_used"], s["records8"]) == (mode, rec8), (step, s["count_mode_used"], s["records8"])
            assert np.array_equal(cid, t["cid"]), step
            assert np.array_equal(keep, t["keep"]), step
            if s["unique"]:                                  # (the accessors' graph over all pairs records no event of its own)
                lv, tlv = dd.leaves(), t["leaves"]
                assert np.array_equal(lv["count"].astype(np.uint64), tlv["count"]), step
                assert np.array_equal(lv["cluster_id"], tlv["cluster_id"]), step
            info = dd.stamp_info()
            nonzero = tuple(k for k in MS if s[k] != 0)
            seen.append((info["event_records"], info["used"], nonzero))
            total = s["ms_count"] + s["ms_neighbours"] + s["ms_cluster"] + s["ms_map"]
            print(config, step, name, info["event_records"], info["used"], {k: s[k] for k in MS}, "sum - total %.6f" % (total - s["ms_total"]))
            if timing and s["unique"]:
                worst = max(worst, abs(total - s["ms_total"]))
                if not TABLE_MODE:
                    assert 0 < s["ms_k_insert"] <= s["ms_count"] <= s["ms_total"], (step, s)
                    assert abs(total - s["ms_total"]) <= SUM_TOL, (step, total, s["ms_total"])
            if not TABLE_MODE:
                records, used, pattern = RECORDS[config][step - 1]
                assert (info["event_records"], info["used"]) == (records, used), (step, info, records, used)
                assert nonzero == PATTERNS[pattern], (step, nonzero, PATTERNS[pattern])
    finally:
        dd.close()
    if TABLE_MODE:
        print("TABLE", config, seen, "worst sum - total", worst)


@pytest.mark.parametrize("timing", [0, 1])
def test_dense_stage_sequence(timing, monkeypatch):
    """count_dense -> map_dense -> kernel_ms of one rank (the stage-by-stage form of the exchange mode): the results, and
    which of the two kernel times are read"""
    from humid_amd.synth import synth_words
    from oracle import pyoracle as orc
    monkeypatch.setenv("HUMID_PY_ORCHESTRATION", "1")
    monkeypatch.setenv("HUMID_KERNEL_TIMING", str(timing))
    words, filt = synth_words(20_000, 77, 24, p_sub=4e-3, p_n=1e-3)
    ocid, okeep, osum, _ = orc.dedup_run(words, filt, 24, 1, 0)
    out, _ = run_ranks(1, words, filt, 24, 1, 0, "exchange")
    cid, keep, s, used = out[0]
    print("dense", timing, {k: s[k] for k in ("ms_k_insert", "ms_k_map", "count_mode_used", "records8")})
    assert used == "exchange"
    assert np.array_equal(cid, ocid) and np.array_equal(keep, okeep)
    for k in ("total", "usable", "unique", "clusters"):
        assert s[k] == osum[k], k
    assert s["ms_k_insert"] > 0                              # the count kernel's pair is always recorded
    assert (s["ms_k_map"] > 0) == bool(timing)               # the dense map's pair with kernel_timing only
