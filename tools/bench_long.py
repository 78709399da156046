"""Long words (humid_dedup_run_long_device) at size: 10 M reads of synth_long_words at n = 64, 100 and 150, d = 1,
device-resident inputs, device-event times (humid_summary.ms_total), --passes timed passes after --warmup warm-up
passes.  The yardstick, on the same n = 64 input: the existing two-word run (humid_dedup_run_device) with option
count_order 0, the sorting count of kernels_wide.hip.h, alternated with the long run pass by pass.  "verified": at
n = 64 the two give the same cluster ids, keep flags and summary counts.  "stages_ms": one further pass with option
kernel_timing, the four stage times of that pass (count, neighbours + graph build, clusters, map).  One JSON line on
stdout.

  python tools/bench_long.py [--reads 10000000] [--passes 10] [--warmup 2] [--lengths 64,100,150]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms, n_reads):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(ms_total=round(float(med), 4), p25_ms=round(float(q1), 4), p75_ms=round(float(q3), 4),
                min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4), passes=len(a),
                reads_per_s=round(n_reads / (float(med) * 1e-3), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lengths", default="64,100,150")
    a = ap.parse_args()
    import torch

    import humid_amd
    from humid_amd.synth import synth_long_words

    assert torch.cuda.is_available(), "bench_long.py needs a GPU"
    dev = torch.device("cuda:0")
    n = a.reads
    long_dd = humid_amd.Dedup(device=0)
    wide_dd = humid_amd.Dedup(device=0)
    wide_dd.set_option("count_order", 0)                   # the sorting count: the code the long count generalises
    out = dict(reads=n, distance=1, shapes=[])
    for nt in [int(x) for x in a.lengths.split(",")]:
        words, filt = synth_long_words(n, 6400 + nt, nt)
        k = words.shape[1]
        d_w = torch.from_numpy(words.view(np.int64)).to(dev)
        d_f = torch.from_numpy(filt).to(dev)
        d_cid = torch.zeros(n, dtype=torch.int32, device=dev)
        d_keep = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        args = (d_w.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), n)
        yard = nt == 64
        t_long, t_wide = [], []
        shape = dict(word_nt=nt, words_per_read=k)
        for p in range(a.warmup + a.passes):
            s = long_dd.run_long_device(*args, nt, distance=1)
            if p >= a.warmup:
                t_long.append(s["ms_total"])
            if yard:
                if p == 0:
                    cid_long, keep_long = d_cid.cpu().numpy().copy(), d_keep.cpu().numpy().copy()
                sw = wide_dd.run_device(*args, word_nt=64, distance=1)
                if p >= a.warmup:
                    t_wide.append(sw["ms_total"])
                if p == 0:
                    shape["verified"] = bool(np.array_equal(cid_long, d_cid.cpu().numpy()) and np.array_equal(keep_long, d_keep.cpu().numpy())
                                             and all(s[key] == sw[key] for key in ("usable", "unique", "clusters", "edges")))
                    shape["yardstick_count_mode_used"] = sw["count_mode_used"]
        # one more pass each with the stages' own events (option kernel_timing: not part of the timed passes)
        stage_keys = ("ms_count", "ms_neighbours", "ms_cluster", "ms_map")
        long_dd.set_option("kernel_timing", 1)
        st = long_dd.run_long_device(*args, nt, distance=1)
        long_dd.set_option("kernel_timing", 0)
        shape["stages_ms"] = {key: round(float(st[key]), 4) for key in stage_keys}
        if yard:
            wide_dd.set_option("kernel_timing", 1)
            st = wide_dd.run_device(*args, word_nt=64, distance=1)
            wide_dd.set_option("kernel_timing", 0)
            shape["yardstick_stages_ms"] = {key: round(float(st[key]), 4) for key in stage_keys}
        shape.update(stats(t_long, n))
        shape.update({key: int(s[key]) for key in ("usable", "unique", "clusters", "edges")})
        shape["ms_sorts"] = round(float(s["ms_k_insert"]), 4)          # the k (+1) radix sorts of the count, last pass
        shape["long_info"] = long_dd.long_info()
        if yard:
            shape["yardstick_two_word_sorting_count"] = stats(t_wide, n)
            shape["yardstick_ms_sorts"] = round(float(sw["ms_k_insert"]), 4)
        out["shapes"].append(shape)
        del d_w, d_f, d_cid, d_keep
    long_dd.close()
    wide_dd.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
