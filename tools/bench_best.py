"""The best-scoring read of every cluster (humid_select_best_device) beside the run that produced the ids: what the
selection pass costs.  One JSON line per shape on stdout; device-event times, warmed contexts, median and quartiles
over --passes calls, the compared calls alternated inside this process.

  the metric words (10 M reads, 24 nt, d = 1), scores uniform random in [0, 12000):
  a  the words as bench.py shuffles them
  b  the same words sorted (runs of equal ids inside a wave)
  c  shape a after run_keyed_device with 1e5 random 32-bit keys (shape a of tools/bench_keyed.py)

  t_run        run_device / run_keyed_device (the yardstick of the same tree)
  t_leaf       select_best_device, scope "leaf" (the call waits for the stream once)
  t_cluster    select_best_device, scope "cluster"
  t_truth      wall time of the numpy truth (tests/best_truth.py, select_sort), scope "leaf"

"verified": keep_out, rep_out and n_changed of both scopes equal the truth.

  python tools/bench_best.py [--passes 25] [--warmup 3] [--shapes abc] [--which all|select]
"""
import argparse
import json
import os
import sys
import time

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
    ap.add_argument("--passes", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--which", default="all", choices=("all", "select"), help="select: the selection alone, unverified (kernel traces)")
    a = ap.parse_args()
    import torch

    import humid_amd
    from humid_amd.synth import synth_words
    import best_truth as bt

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

    words0, filt0 = synth_words(a.reads, 1002, 24)               # bench.py's metric words
    n = len(filt0)
    rng = np.random.default_rng(67)
    scores = rng.integers(0, 12000, n).astype(np.uint32)
    pool = rng.integers(0, 1 << 32, size=100_000, dtype=np.uint64)
    keys = pool[rng.integers(0, len(pool), size=n)]
    d_sc = to_dev(scores, np.int32)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_rep = torch.zeros(n, dtype=torch.int32, device=dev)
    order = np.argsort(words0, kind="stable")
    shapes = dict(a=("shuffled", None, False), b=("sorted by word", order, False), c=("shuffled, after run_keyed (1e5 32-bit keys)", None, True))
    for name in a.shapes:
        what, perm, keyed = shapes[name]
        words, filt = (words0, filt0) if perm is None else (words0[perm], filt0[perm])
        d_w, d_f = to_dev(words, np.int64), to_dev(filt, np.uint8)
        d_key = to_dev(keys, np.int64) if keyed else None
        if keyed:
            run = lambda: dd.run_keyed_device(d_w.data_ptr(), d_key.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n,  # noqa: E731
                                              word_nt=24, distance=1)
        else:
            run = lambda: dd.run_device(d_w.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n, word_nt=24, distance=1)  # noqa: E731
        select = {s: (lambda s=s: dd.select_best_device(d_w.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), d_sc.data_ptr(),
                                                        d_out.data_ptr(), d_rep.data_ptr(), n, word_nt=24, scope=s))
                  for s in ("leaf", "cluster")}
        summary = run()
        line = dict(shape=name, what="10M metric words, 24 nt, d=1, scores uniform in [0, 12000): " + what, reads=n,
                    clusters=int(summary["clusters"]))
        ok, t_truth = True, None
        if a.which == "all":
            cid, keep = d_c.cpu().numpy().view(np.uint32), d_k.cpu().numpy()
            for s, scope in (("leaf", bt.LEAF), ("cluster", bt.CLUSTER)):
                t0 = time.perf_counter()
                t = bt.select_sort(words, cid, keep, scores, scope)
                if s == "leaf":
                    t_truth = (time.perf_counter() - t0) * 1e3
                ch = select[s]()
                ok = ok and ch == t[2] and bool(np.array_equal(d_out.cpu().numpy(), t[0]))
                ok = ok and bool(np.array_equal(d_rep.cpu().numpy().view(np.uint32), t[1]))
                line["changed_" + s] = int(t[2])
        tr, tl, tc = [], [], []
        for _ in range(a.warmup):
            if a.which == "all":
                run()
            select["leaf"]()
            select["cluster"]()
        for _ in range(a.passes):
            if a.which == "all":
                tr.append(timed_ms(run))
            tl.append(timed_ms(select["leaf"]))
            tc.append(timed_ms(select["cluster"]))
        line.update(select_leaf=stats(tl), select_cluster=stats(tc))
        if a.which == "all":
            sr, sl = stats(tr), stats(tl)
            line.update(run=sr, leaf_share_of_run=round(sl["median_ms"] / sr["median_ms"], 4), truth_ms=round(t_truth, 1), verified=ok)
        print(json.dumps(line), flush=True)
        del d_w, d_f, d_key
    dd.close()


if __name__ == "__main__":
    main()
