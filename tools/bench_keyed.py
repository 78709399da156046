"""Keyed deduplication (humid_dedup_run_keyed_device: 64-bit keys ranked on the device) against what a caller of
humid_dedup_run_grouped_device pays for the same result: the host-side ranking of the keys plus the grouped pass.
One JSON line per shape on stdout; device-event times, warmed contexts, median and quartiles over --passes passes,
the two device sides alternated inside this process.

  the metric words (10 M reads, 24 nt, d = 1) with
  a  10^5 random 32-bit keys
  b  2.5 M random 64-bit keys
  c  shape a sorted by key (long runs of equal keys)

  t_grouped    run_grouped_device on the pre-ranked u32 groups (n_groups = the number of distinct keys)
  t_keyed      run_keyed_device on the raw keys
  t_host_rank  wall time of np.unique(keys, return_inverse=True) plus the copy of the u32 groups to the device

"verified": the keyed pass's cluster ids and keep flags equal the grouped pass's, and group_keys() equals np.unique.

  python tools/bench_keyed.py [--passes 25] [--warmup 3] [--host-passes 3] [--shapes abc] [--which both|keyed]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(median_ms=round(float(med), 4), p25_ms=round(float(q1), 4), p75_ms=round(float(q3), 4),
                min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-passes", type=int, default=3)
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--which", default="both", choices=("both", "keyed"), help="keyed: that side alone (kernel traces)")
    a = ap.parse_args()
    import torch

    import humid_amd
    from humid_amd.synth import synth_words

    dev = torch.device("cuda:0")
    dk = humid_amd.Dedup(device=0)                               # keyed passes
    dg = humid_amd.Dedup(device=0)                               # grouped passes

    def to_dev(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)

    def timed_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    words, filt = synth_words(a.reads, 1002, 24)                 # bench.py's metric words
    n = len(filt)
    d_w, d_f = to_dev(words, np.int64), to_dev(filt, np.uint8)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_c2 = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k2 = torch.zeros(n, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(64)
    pool_a = rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64)
    keys_a = pool_a[rng.integers(0, len(pool_a), size=n)]
    shapes = dict(a=("1e5 random 32-bit keys", lambda: keys_a),
                  b=("2.5e6 random 64-bit keys",
                     lambda: rng.integers(0, 1 << 64, size=2_500_000, dtype=np.uint64)[rng.integers(0, 2_500_000, size=n)]),
                  c=("shape a sorted by key", lambda: np.sort(keys_a)))
    for name in a.shapes:
        what, make = shapes[name]
        keys = make()
        d_key = to_dev(keys, np.int64)
        # what a caller of the grouped entry point does first, on the host
        th, groups, K = [], None, None
        for _ in range(a.host_passes):
            t0 = time.perf_counter()
            K, inv = np.unique(keys, return_inverse=True)
            groups = inv.astype(np.uint32, copy=False)
            d_g = torch.from_numpy(groups.view(np.int32)).to(dev)
            torch.cuda.synchronize()
            th.append((time.perf_counter() - t0) * 1e3)
        G = len(np.unique(keys[filt == 0]))                      # the groups of the usable reads (the contract)
        n_groups = len(K)
        keyed = lambda: dk.run_keyed_device(d_w.data_ptr(), d_key.data_ptr(), d_f.data_ptr(), d_c.data_ptr(),  # noqa: E731
                                            d_k.data_ptr(), n, word_nt=24, distance=1)
        grouped = lambda: dg.run_grouped_device(d_w.data_ptr(), d_g.data_ptr(), d_f.data_ptr(), d_c2.data_ptr(),  # noqa: E731
                                                d_k2.data_ptr(), n, n_groups, word_nt=24, distance=1)
        tk, tg = [], []
        for _ in range(a.warmup):
            keyed()
            if a.which == "both":
                grouped()
        for _ in range(a.passes):
            tk.append(timed_ms(keyed))
            if a.which == "both":
                tg.append(timed_ms(grouped))
        info = dk.keyed_rank_info()
        line = dict(shape=name, what="10M metric words, 24 nt, d=1, " + what, reads=n, distinct_keys=int(info["n_keys"]),
                    table_log2=info["table_log2"], redo_in_last_pass=info["n_redo"], keyed=stats(tk))
        if a.which == "both":
            ok = bool(np.array_equal(dk.group_keys(), np.unique(keys[filt == 0])) and info["n_keys"] == G)
            ok = ok and bool(torch.equal(d_c, d_c2)) and bool(torch.equal(d_k, d_k2))
            sk, sg, sh = stats(tk), stats(tg), stats(th)
            both = sh["median_ms"] + sg["median_ms"]
            spread = (sk["p75_ms"] - sk["p25_ms"]) + (sg["p75_ms"] - sg["p25_ms"]) + (sh["p75_ms"] - sh["p25_ms"])
            line.update(grouped=sg, host_rank=sh, rank_cost_ms=round(sk["median_ms"] - sg["median_ms"], 4),
                        rank_share_of_keyed=round((sk["median_ms"] - sg["median_ms"]) / sk["median_ms"], 4),
                        host_rank_plus_grouped_over_keyed=round(both / sk["median_ms"], 2),
                        keyed_faster_beyond_spread=bool(both - sk["median_ms"] > spread),
                        groups_equal_distinct_keys=bool(G == n_groups), verified=ok)
        print(json.dumps(line), flush=True)
        del d_key
    dk.close()
    dg.close()


if __name__ == "__main__":
    main()
