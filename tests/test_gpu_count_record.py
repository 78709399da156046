"""-m gpu: ONE context taken through every road of the count stage in turn -- records (one-word and two-word words),
the global table, the sorting count (two-word and long words), hashed buckets, ordered buckets on 12-byte pairs, an
input with no usable read (in ordered buckets and in the global table, each with a bucketed road behind it) -- so that anything the count before left in the context, and the
next count did not replace, shows in the graph stage, the read map or the timing tail behind it.

Every step compares cluster ids, keep flags and the summary counts with the C oracle (beyond 64 nt with
tests/long_truth.py), asserts the road from the summary's count_mode_used / records8, and reads the leaves back.  The
sequence runs with kernel_timing 0 and 1: with 1 the pass's tail reads the events that only some roads record.

The record road starts above 11 200 reads (350 << 5: six bucket bits); the two-word count takes buckets from 65 536
reads on."""
import numpy as np
import pytest

import humid_amd
import long_truth as lt
from humid_amd.synth import synth_long_words, synth_wide_words, synth_words
from test_gpu_long import planted
from test_gpu_parity import oracle_full

pytestmark = pytest.mark.gpu

U64 = np.uint64
COUNTS = ("total", "usable", "unique", "clusters", "edges")


def oracle_truth(words, filt, n):
    p, cid, keep = oracle_full(words, filt, n, 1, False)
    summary = p.summary()
    return dict(cid=cid, keep=keep, summary=summary, leaves=p.leaves() if summary["unique"] else None)


@pytest.fixture(scope="module")
def inputs():
    """name -> (words, filt, word_nt, truth); the references are computed once and never written to"""
    out = {}
    w, f = synth_words(12_000, 51, 24, p_sub=8e-3, p_n=1e-3)
    assert 350 << 5 < len(w) <= 350 << 6
    out["n24"] = (w, f, 24, oracle_truth(w, f, 24))
    w, f = synth_wide_words(6_000, 52, 48, p_sub=4e-3, p_n=1e-3)
    out["n48_small"] = (w, f, 48, oracle_truth(w, f, 48))
    w, f = synth_wide_words(70_000, 948, 48, p_sub=4e-3, p_n=1e-3)
    out["n48"] = (w, f, 48, oracle_truth(w, f, 48))
    w, f = planted(*synth_long_words(3000, 9080, 80, 0.01, 0.01), 80, 1, seed=80)
    t = lt.long_dedup(w, f, 1, 0, word_nt=80)
    out["n80"] = (w, f, 80, dict(cid=t["cid"], keep=t["keep"], summary=t["summary"], leaves=t["leaves"]))
    w = np.array([5, 6, 7, 8, 9], U64)
    f = np.ones(5, np.uint8)
    out["none"] = (w, f, 24, oracle_truth(w, f, 24))
    return out


# (input, options set in front of the step, count_mode_used, records8)
STEPS = [
    ("n24", dict(count_order=1), 2, True),                    # 1. records
    ("n24", dict(count_mode=1), 1, False),                    # 2. the global table
    ("n48_small", dict(count_mode=0, count_order=0), 3, False),   # 3. the sorting count
    ("n24", dict(), 0, False),                                # 4. hashed buckets
    ("n48", dict(count_order=1), 2, True),                    # 5. records of two-word words
    ("n80", dict(), 3, False),                                # 6. the sorting count of long words
    ("n24", dict(records8=0), 2, False),                      # 7. ordered buckets on (key, read) pairs
    ("none", dict(records8=1), 0, False),                     # 8. no usable read in ordered buckets: the summary names no road
    ("n24", dict(), 2, True),                                 # 9. records again
    ("none", dict(count_mode=1), 0, False),                   # 10. no usable read in the global table
    ("n24", dict(count_mode=0, count_order=0), 0, False),     # 11. hashed buckets behind it: bucket by bucket, in partition order
    ("n24", dict(count_order=1), 2, True),                    # 12. records behind those
]


@pytest.mark.parametrize("timing", [0, 1])
def test_every_road_in_turn(inputs, timing):
    dd = humid_amd.Dedup()
    try:
        dd.set_option("kernel_timing", timing)
        for step, (name, options, mode, rec8) in enumerate(STEPS, 1):
            words, filt, n, t = inputs[name]
            for key, value in options.items():
                dd.set_option(key, value)
            if n > 64:
                cid, keep, s = dd.run_long(words, filt, n, distance=1, method=0)
            else:
                cid, keep, s = dd.run(words, filt, word_nt=n, distance=1, method=0)
            print(step, name, options, {k: s[k] for k in COUNTS + ("count_mode_used", "records8")})
            for k in COUNTS:
                assert s[k] == t["summary"][k], (step, k, s[k], t["summary"][k])
            assert (s["count_mode_used"], s["records8"]) == (mode, rec8), (step, s["count_mode_used"], s["records8"])
            assert np.array_equal(cid, t["cid"]), step
            assert np.array_equal(keep, t["keep"]), step
            if name == "none":
                assert s["usable"] == 0 and s["unique"] == 0 and not cid.any() and not keep.any()
                assert all(len(v) == 0 for v in dd.leaves().values())
                continue
            assert s["unique"] > 500 and s["edges"] > 0, (step, s)
            lv, tlv = dd.leaves(), t["leaves"]
            assert np.array_equal(lv["word"], np.asarray(tlv["word"]).reshape(lv["word"].shape)), step
            assert np.array_equal(lv["count"].astype(U64), tlv["count"]), step
            for k in ("degree", "cluster_id", "is_max_leaf"):
                assert np.array_equal(lv[k], tlv[k]), (step, k)
    finally:
        dd.close()
