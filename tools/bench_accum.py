"""Cost of an accumulated run (humid_accum_*) beside the one-shot run, on the metric workload of BASELINE.md:
10 M reads, 24 nt, d = 1, words resident on the device.

    python tools/bench_accum.py [--reads 10000000] [--chunks 1 4 16] [--repeat 3] [--json FILE]

One process, one build: the one-shot pass (humid_dedup_run_device), then the same read set as an accumulated run in 1, 4
and 16 chunks.  Every configuration runs once untimed (warm-up: buffers, code object) and --repeat times timed; a time
is a host clock around a call that ends in a stream wait, the median over the repeats.  Results are compared with the
one-shot run's.  Per add the chunk's count stage alone (humid_stage_count on the same chunk) is timed too, so
merge = add - count is a difference of two medians, not a kernel time.  Bytes moved by a merge: the entries of A, of B
and of the output times their sizes (word 8 + count 4 + first 8 for A and the output, first 4 for B), each list
streamed once by the count pass (words only) and once by the fill pass.
Prints one JSON line per configuration and a summary table in markdown."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--word-nt", type=int, default=24)
    ap.add_argument("--distance", type=int, default=1)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch

    import humid_amd
    from humid_amd.synth import synth_words

    if not torch.cuda.is_available():
        sys.exit("bench_accum.py needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda", 0)
    n, nt, d = a.reads, a.word_nt, a.distance
    words, filt = synth_words(n, 1002, nt)                       # the metric configuration's read set (bench.py)
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_cid = torch.zeros(n, dtype=torch.int32, device=dev)
    d_keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    dd = humid_amd.Dedup()
    lib, h = dd._lib, dd._h

    def clock(f):
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r

    def med(x):
        return statistics.median(x)

    out = []
    # ---- one shot ----
    one = []
    for it in range(a.repeat + 1):
        ms, s = clock(lambda: dd.run_device(d_w.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), n, nt, d))
        if it:
            one.append((ms, s["ms_total"]))
    ref_cid, ref_keep = d_cid.clone(), d_keep.clone()
    ref_sum = {k: int(s[k]) for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle")}
    one_ms, one_dev = med([x[0] for x in one]), med([x[1] for x in one])
    out.append(dict(mode="one_shot", reads=n, ms_call=round(one_ms, 3), ms_device=round(one_dev, 3), **ref_sum))
    print(json.dumps(out[-1]), flush=True)

    # ---- accumulated, in k chunks ----
    for k in a.chunks:
        cuts = [n * i // k for i in range(k + 1)]
        t_add, t_cnt, t_map, t_fin, uniq = [[] for _ in range(k)], [[] for _ in range(k)], [[] for _ in range(k)], [], [0] * k
        u_chunk = [0] * k
        for it in range(a.repeat + 1):
            d_cid.zero_()
            d_keep.zero_()
            # the chunks' count stage alone, for merge = add - count
            for i in range(k):
                lo, m = cuts[i], cuts[i + 1] - cuts[i]
                nu, us = C.c_uint64(), C.c_uint64()
                ms, rc = clock(lambda: lib.humid_stage_count(h, d_w.data_ptr() + 8 * lo, d_f.data_ptr() + lo, m, nt, 0, 2 ** 64 - 1, 0,
                                                             C.byref(nu), C.byref(us)))
                dd._check(rc)
                u_chunk[i] = nu.value
                if it:
                    t_cnt[i].append(ms)
            acc = dd.accumulator(nt)
            for i in range(k):
                lo, m = cuts[i], cuts[i + 1] - cuts[i]
                ms, _ = clock(lambda: acc.add_device(d_w.data_ptr() + 8 * lo, d_f.data_ptr() + lo, m, lo))
                uniq[i] = acc.info()["unique"]
                if it:
                    t_add[i].append(ms)
            ms, s = clock(lambda: acc.finish(d, humid_amd.DIRECTIONAL))
            if it:
                t_fin.append(ms)
            unknown = 0
            for i in range(k):
                lo, m = cuts[i], cuts[i + 1] - cuts[i]
                ms, u = clock(lambda: acc.map_device(d_w.data_ptr() + 8 * lo, d_f.data_ptr() + lo, m, lo, d_cid.data_ptr() + 4 * lo,
                                                     d_keep.data_ptr() + lo))
                unknown += u
                if it:
                    t_map[i].append(ms)
            torch.cuda.synchronize()
            same = bool(torch.equal(d_cid, ref_cid)) and bool(torch.equal(d_keep, ref_keep)) and unknown == 0 and \
                {kk: int(s[kk]) for kk in ref_sum} == ref_sum
            if not same:
                sys.exit("bench_accum.py: the accumulated run in %d chunks differs from the one-shot run" % k)
        add, cnt, mp, fin = [med(x) for x in t_add], [med(x) for x in t_cnt], [med(x) for x in t_map], med(t_fin)
        total = sum(add) + fin + sum(mp)
        # the last merge: A = the list before it, B = the chunk's unique words, O = the list after it
        nA, nB, nO = (uniq[k - 2] if k > 1 else 0), u_chunk[k - 1], uniq[k - 1]
        merge_bytes = 2 * 8 * (nA + nB) + (4 + 8) * nA + (4 + 4) * nB + 20 * nO      # words twice; counts + firsts in; entries out
        merge_ms = add[-1] - cnt[-1]
        rec = dict(mode="accumulated", chunks=k, reads=n, identical=True, ms_total=round(total, 3), ratio_to_one_shot=round(total / one_ms, 3),
                   ms_add=[round(x, 3) for x in add], ms_count_alone=[round(x, 3) for x in cnt], ms_finish=round(fin, 3),
                   ms_map=[round(x, 3) for x in mp], unique_after_add=uniq, unique_of_chunk=u_chunk,
                   last_merge=dict(nA=nA, nB=nB, nO=nO, bytes=merge_bytes, ms=round(merge_ms, 3),
                                   gb_per_s=round(merge_bytes / max(merge_ms, 1e-6) / 1e6, 1)))
        out.append(rec)
        print(json.dumps(rec), flush=True)

    print("\n| run | calls (ms, medians of %d) | total ms | x one-shot |\n|---|---|---|---|" % a.repeat)
    print("| one shot | humid_dedup_run_device %.3f (events: %.3f) | %.3f | 1.00 |" % (one_ms, one_dev, one_ms))
    for r in out[1:]:
        print("| %d chunks | add %s; finish %.3f; map %s | %.3f | %.2f |" % (
            r["chunks"], " ".join("%.2f" % x for x in r["ms_add"]), r["ms_finish"], " ".join("%.2f" % x for x in r["ms_map"]),
            r["ms_total"], r["ratio_to_one_shot"]))
    for r in out[1:]:
        lm = r["last_merge"]
        print("last add of %d chunks: count alone %.3f ms, add %.3f ms, merge (difference) %.3f ms over %d + %d -> %d entries, %.1f MB: %.1f GB/s"
              % (r["chunks"], r["ms_count_alone"][-1], r["ms_add"][-1], lm["ms"], lm["nA"], lm["nB"], lm["nO"], lm["bytes"] / 1e6, lm["gb_per_s"]))
    if a.json:
        with open(a.json, "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")
    dd.close()


if __name__ == "__main__":
    main()
