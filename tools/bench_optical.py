"""Optical duplicates per cluster (humid_optical_duplicates_device) on the metric workload: what the pass costs beside
the run it follows and beside humid_select_best on the same arrays.  One JSON line per distance on stdout; device-event
times, warmed contexts, median and quartiles over --passes calls, the compared calls alternated inside this process.

  ids and keep: the run of bench.py's metric words (--reads 10 M reads, 24 nt, d = 1)
  positions:    tests/optical_truth.make_positions (8 tiles, a 20 000 x 20 000 square, 30 % of the reads moved to
                within D / 2 of a read of their cluster, 1 % without a position)
  distances:    --distances 100,2500

  t_optical[W]    humid_optical_duplicates_device with option "optical_walk" = W, for every W of --walks
  t_select        humid_select_best_device (scope leaf) on the same ids, keep and random scores
  t_run           humid_dedup_run_device on the same words; ms_total is the run's own device time

"verified": optical, origin, per_cluster and the summary equal tests/optical_truth.optical_sweep for every W.

  python tools/bench_optical.py [--passes 15] [--warmup 3] [--reads 10000000] [--walks 16,64,256,0] [--which all|optical]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(median_ms=round(float(med), 4), p25_ms=round(float(q1), 4), p75_ms=round(float(q3), 4),
                min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--distances", default="100,2500")
    ap.add_argument("--walks", default="16,64,256,0")
    ap.add_argument("--which", default="all", choices=("all", "optical"), help="optical: that pass alone, default walk (kernel traces)")
    a = ap.parse_args()
    import torch

    import humid_amd
    from humid_amd.synth import synth_words
    import optical_truth as ot

    dev = torch.device("cuda:0")
    dd = humid_amd.Dedup(device=0)

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
    torch.cuda.synchronize()
    run = lambda: dd.run_device(d_w.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n, word_nt=24, distance=1)  # noqa: E731
    s = run()
    n_cl = int(s["clusters"])
    cid, keep = d_c.cpu().numpy().view(np.uint32), d_k.cpu().numpy()
    d_sc = to_dev(np.random.default_rng(5).integers(0, 1 << 20, n).astype(np.uint32), np.int32)
    d_k2 = torch.zeros(n, dtype=torch.uint8, device=dev)
    select = lambda: dd.select_best_device(d_w.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), d_sc.data_ptr(), d_k2.data_ptr(), 0, n,  # noqa: E731
                                           word_nt=24, scope="leaf")
    walks = [int(w) for w in a.walks.split(",")] if a.which == "all" else [64]
    for D in (int(v) for v in a.distances.split(",")):
        tile, x, y = ot.make_positions(cid, keep, 7, D=D, n_tiles=8, side=20000, p_near=0.3, p_none=0.01)
        d_t, d_x, d_y = to_dev(tile, np.int32), to_dev(x, np.int32), to_dev(y, np.int32)
        out = {}

        def optical():
            out["r"] = dd.optical_duplicates(d_c, d_k, d_t, d_x, d_y, distance=D, n_clusters=n_cl)

        ok, summ = True, None
        if a.which == "all":
            t = ot.optical_sweep(cid, keep, tile, x, y, D, n_cl)
            summ = t[3]
            for w in walks:
                dd.set_option("optical_walk", w)
                optical()
                r = out["r"]
                got = (r[0].cpu().numpy(), r[1].cpu().numpy().view(np.uint32), r[2].cpu().numpy().view(np.uint32), r[3])
                try:
                    ot.assert_same(got, t, ("walk", w))
                except AssertionError:
                    ok = False
        times = {w: [] for w in walks}
        t_sel, t_run, ms_total = [], [], []
        for it in range(a.warmup + a.passes):
            for w in walks:
                dd.set_option("optical_walk", w)
                ms = timed_ms(optical)
                if it >= a.warmup:
                    times[w].append(ms)
            if a.which == "all":
                ms = timed_ms(select)
                if it >= a.warmup:
                    t_sel.append(ms)
                box = {}
                ms = timed_ms(lambda: box.update(s=run()))
                if it >= a.warmup:
                    t_run.append(ms)
                    ms_total.append(box["s"]["ms_total"])
        line = dict(what="10M metric words, 24 nt, d=1; positions: 8 tiles, 20000^2, 30 % near", reads=n, clusters=n_cl, distance=D,
                    optical={str(w): stats(times[w]) for w in walks})
        if a.which == "all":
            line.update(select_best=stats(t_sel), run_device=stats(t_run), run_ms_total=stats(ms_total), summary=summ, verified=ok)
        print(json.dumps(line), flush=True)
        del d_t, d_x, d_y
    dd.close()


if __name__ == "__main__":
    main()
