"""Strand-symmetric (duplex) deduplication (humid_dedup_run_paired_device) on the metric workload with half of the reads
read from the other strand: what the pass costs beside the plain run of the same tree.  One JSON line on stdout; times
of warmed calls with a device synchronise behind them, median and quartiles over --passes calls, the compared calls
alternated inside this process.

  words:  bench.py's metric words (synth_words, --reads 10 M reads, 24 nt), every read mirrored with probability 1/2
          (its two halves of 12 nt exchanged): the reads of a family lie on both strands

  t_paired          humid_dedup_run_paired_device on those words, d = 1
  t_run_mixed       humid_dedup_run_device on the same words (the mirrored copies are leaves of their own: what a user
                    without -P gets, about twice the clusters)
  t_run_canonical   humid_dedup_run_device on the canonical words (the same leaves as the paired pass, found without
                    the mirror join)
  ms_total_*        the run's own device time (humid_summary.ms_total: count .. per-read outputs)

"verified": the canonical words and strands equal numpy's; the paired runs on the words, on the canonical words and on
the mirrored words agree in cluster ids and keep flags; the strand tallies add up to the usable reads.  (The
bit-for-bit comparison with the all-pairs truth is tests/test_gpu_paired.py; 10 M reads are beyond it.)

  python tools/bench_paired.py [--passes 15] [--warmup 3] [--reads 10000000] [--which all|paired]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(median_ms=round(float(med), 4), p25_ms=round(float(q1), 4), p75_ms=round(float(q3), 4),
                min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4), n=len(a))


def mirror24(w):
    m = np.uint64((1 << 24) - 1)
    return ((w & m) << np.uint64(24)) | (w >> np.uint64(24))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--which", default="all", choices=("all", "paired"), help="paired: that pass alone (kernel traces)")
    a = ap.parse_args()
    import torch

    import humid_amd
    from humid_amd.synth import synth_words

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
    flip = np.random.default_rng(9).random(n) < 0.5
    mixed = np.where(flip, mirror24(words), words)
    canon = np.minimum(mixed, mirror24(mixed))
    strand = np.where(filt != 0, 2, (canon != mixed).astype(np.uint8)).astype(np.uint8)
    d_f = to_dev(filt, np.uint8)
    d_mixed, d_canon, d_mirr = to_dev(mixed, np.int64), to_dev(canon, np.int64), to_dev(mirror24(mixed), np.int64)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    box = {}

    def paired(d_w=d_mixed):
        box["s"] = dd.run_paired_device(d_w.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n, word_nt=24, distance=1)

    def plain(d_w):
        box["s"] = dd.run_device(d_w.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n, word_nt=24, distance=1)

    line = dict(what="10M metric words, 24 nt, d=1, every read mirrored with probability 1/2", reads=n)
    if a.which == "all":
        paired()
        s_paired = dict(box["s"])
        cid, keep = d_c.cpu().numpy().copy(), d_k.cpu().numpy().copy()
        got_strand, top, bottom, sm = dd.strands()
        ok = np.array_equal(got_strand, strand) and int(top.sum() + bottom.sum()) == int((filt == 0).sum())
        d_out = torch.zeros(n, dtype=torch.int64, device=dev)
        d_s = torch.zeros(n, dtype=torch.uint8, device=dev)
        dd.canonical_words_device(d_mixed.data_ptr(), d_f.data_ptr(), d_out.data_ptr(), d_s.data_ptr(), n, word_nt=24)
        use = filt == 0
        ok = ok and np.array_equal(d_out.cpu().numpy().view(np.uint64)[use], canon[use]) and np.array_equal(d_s.cpu().numpy(), strand)
        for d_w in (d_canon, d_mirr):
            paired(d_w)
            ok = ok and np.array_equal(d_c.cpu().numpy(), cid) and np.array_equal(d_k.cpu().numpy(), keep)
        plain(d_mixed)
        s_mixed = dict(box["s"])
        plain(d_canon)
        s_canon = dict(box["s"])
        keys = ("total", "usable", "unique", "clusters", "edges")
        line.update(paired={k: int(s_paired[k]) for k in keys}, run_mixed={k: int(s_mixed[k]) for k in keys},
                    run_canonical={k: int(s_canon[k]) for k in keys}, strands=sm, verified=bool(ok))
    t = dict(paired=[], run_mixed=[], run_canonical=[])
    tot = dict(paired=[], run_mixed=[], run_canonical=[])
    calls = dict(paired=paired, run_mixed=lambda: plain(d_mixed), run_canonical=lambda: plain(d_canon))
    names = ("paired", "run_mixed", "run_canonical") if a.which == "all" else ("paired",)
    for it in range(a.warmup + a.passes):
        for k in names:
            ms = timed_ms(calls[k])
            if it >= a.warmup:
                t[k].append(ms)
                tot[k].append(box["s"]["ms_total"])
    for k in names:
        line["t_" + k] = stats(t[k])
        line["ms_total_" + k] = stats(tot[k])
    print(json.dumps(line), flush=True)
    dd.close()


if __name__ == "__main__":
    main()
