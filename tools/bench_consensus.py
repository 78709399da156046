"""Consensus reads per cluster (humid_consensus_device) beside the run that produced the ids: what the pass costs.
One JSON line per shape on stdout; device-event times, warmed contexts, median and quartiles over --passes calls, the
compared calls alternated inside this process.

  the metric words (10 M reads, 24 nt, d = 1) as clusters; reads of 150 nt from humid_amd.synth.synth_reads (seed 71):
  one template per cluster, substitutions at --p-sub (default 0.005), qualities Phred 40 with probability 0.8, else
  uniform in 2 .. 39
  a  the reads in the order bench.py shuffles the words
  b  the same reads sorted by cluster id (a cluster's rows lie side by side)

  t_run_device         run_device (the yardstick of the same tree)
  t_consensus_device   humid_consensus_device: two host waits inside, the results left in HBM
  floor                the pass's byte floor, 2 x n_bytes read + 2 x total_bytes written, at 6.3 TB/s (the achievable
                       HBM rate DESIGN.md uses), and floor_share = floor / t_consensus_device
  t_truth              wall time of the numpy truth (tests/consensus_truth.py, consensus_matrix)

"verified": out_off, both blobs, depth, errors and the summary equal the truth.

  python tools/bench_consensus.py [--passes 15] [--warmup 2] [--shapes ab] [--reads 10000000] [--which all|consensus]
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

HBM_BYTES_PER_MS = 6.3e9       # 6.3 TB/s


def stats(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return dict(median_ms=round(float(med), 4), p25_ms=round(float(q1), 4), p75_ms=round(float(q3), 4),
                min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4), n=len(a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="ab")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--p-sub", type=float, default=5e-3)
    ap.add_argument("--which", default="all", choices=("all", "consensus"), help="consensus: the pass alone, unverified (kernel traces)")
    a = ap.parse_args()
    import torch

    import humid_amd
    from humid_amd.synth import synth_reads, synth_words
    import consensus_truth as ct

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
    n, L = len(filt0), a.read_len
    cid0, keep0, s0 = dd.run(words0, filt0, word_nt=24, distance=1)
    C = int(s0["clusters"])
    b0, q0 = synth_reads(cid0, 71, read_len=L, p_sub=a.p_sub)
    d_off = to_dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(L), np.int64)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
    shapes = dict(a=("shuffled", None), b=("sorted by cluster id", np.argsort(cid0, kind="stable")))
    for name in a.shapes:
        what, perm = shapes[name]
        words, filt, b, q = (words0, filt0, b0, q0) if perm is None else (words0[perm], filt0[perm], b0[perm], q0[perm])
        d_w, d_f = to_dev(words, np.int64), to_dev(filt, np.uint8)
        d_b, d_q = to_dev(b.reshape(-1), np.uint8), to_dev(q.reshape(-1), np.uint8)
        run = lambda: dd.run_device(d_w.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n, word_nt=24, distance=1)  # noqa: E731
        cons = lambda: dd.consensus_device(d_b.data_ptr(), d_q.data_ptr(), d_off.data_ptr(), n * L, d_c.data_ptr(), d_k.data_ptr(),  # noqa: E731
                                           n, C, min_q=10, cap_q=93)
        summary = run()
        assert int(summary["clusters"]) == C
        sm = cons()
        floor_ms = (2 * n * L + 2 * sm["total_bytes"]) / HBM_BYTES_PER_MS
        line = dict(shape=name, what="%d metric words as clusters, %d nt reads, p_sub %g: %s" % (n, L, a.p_sub, what), reads=n,
                    n_bytes=n * L, **sm)
        ok, t_truth = True, None
        if a.which == "all":
            cid, keep = d_c.cpu().numpy().view(np.uint32), d_k.cpu().numpy()
            t0 = time.perf_counter()
            t = ct.consensus_matrix(b, q, cid, keep, C)
            t_truth = (time.perf_counter() - t0) * 1e3
            res = dd._consensus_result(sm)
            try:
                ct.assert_same(t, res, name)
            except AssertionError as e:
                ok = False
                print(str(e), file=sys.stderr)
            del res, t
        tr, tc = [], []
        for _ in range(a.warmup):
            if a.which == "all":
                run()
            cons()
        for _ in range(a.passes):
            if a.which == "all":
                tr.append(timed_ms(run))
            tc.append(timed_ms(cons))
        sc = stats(tc)
        line.update(t_consensus_device=sc, floor_ms=round(floor_ms, 4), floor_share=round(floor_ms / sc["median_ms"], 4))
        if a.which == "all":
            sr = stats(tr)
            line.update(t_run_device=sr, consensus_over_run=round(sc["median_ms"] / sr["median_ms"], 2), truth_ms=round(t_truth, 1),
                        verified=ok)
        print(json.dumps(line), flush=True)
        del d_w, d_f, d_b, d_q
    dd.close()


if __name__ == "__main__":
    main()
