"""Cost of a keyed accumulated run (humid_accum_*_keyed) beside the one-shot keyed run and the plain accumulator:
10 M reads, 3 000 barcodes of 16 nt, 12-nt UMIs, d = 1, words and keys resident on the device.

    python tools/bench_accum_keyed.py [--reads 10000000] [--barcodes 3000] [--chunks 1 4 16] [--repeat 3] [--json FILE]

One process, one build.  The one-shot pass (humid_dedup_run_keyed_device), then the same read set as a keyed accumulated
run in 1, 4 and 16 chunks, once with key_nt 16 (one uint64 per entry) and once with key_nt 0 (two), and as a PLAIN
accumulated run at word_nt 28 over the packed values key << 24 | word (the yardstick for the one-word entry: the same
count, merge and lookup, without the pack kernel and the ranking).  Every configuration runs once untimed and --repeat
times timed; a time is a host clock around a call that ends in a stream wait, the median over the repeats.  The results
of every keyed accumulated run are compared with the one-shot run's.
The count mode of a chunk (humid_summary.count_mode_used) is read off a plain distance-0 run over the chunk's entries,
packed on the host, at the entry's word length: the same count stage over the same input as the add's.
Prints one JSON line per configuration and a summary table in markdown."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("total", "usable", "unique", "clusters", "edges", "nonsingle")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--barcodes", type=int, default=3000)
    ap.add_argument("--distance", type=int, default=1)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch

    import humid_amd
    from humid_amd.synth import synth_words

    if not torch.cuda.is_available():
        sys.exit("bench_accum_keyed.py needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda", 0)
    n, d, wnt, knt = a.reads, a.distance, 12, 16
    words, filt = synth_words(n, 1002, wnt)
    rng = np.random.default_rng(1002)
    cells = np.unique(rng.integers(0, 4 ** knt, a.barcodes + 64).astype(np.uint64))[:a.barcodes]
    p = 1.0 / (np.arange(len(cells)) + 10.0)                       # reads per cell: the largest about 300 times the smallest
    keys = cells[rng.permutation(len(cells))][rng.choice(len(cells), n, p=p / p.sum())]
    packed = (keys << np.uint64(2 * wnt)) | words
    pairs = np.stack([keys, words], 1)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64 if x.dtype == np.uint64 else x.dtype)).to(dev)

    d_w, d_k, d_f, d_p, d_e = up(words), up(keys), up(filt), up(packed), up(pairs)
    d_cid = torch.zeros(n, dtype=torch.int32, device=dev)
    d_keep = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    dd = humid_amd.Dedup()

    def clock(f):
        t0 = time.perf_counter()
        r = f()
        return (time.perf_counter() - t0) * 1e3, r

    med = statistics.median
    out = []
    one = []
    for it in range(a.repeat + 1):
        ms, s = clock(lambda: dd.run_keyed_device(d_w.data_ptr(), d_k.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), n, wnt, d))
        if it:
            one.append((ms, s["ms_total"]))
    ref_cid, ref_keep = d_cid.clone(), d_keep.clone()
    ref_sum = {k: int(s[k]) for k in FIELDS}
    n_keys = len(dd.group_keys())
    one_ms = med([x[0] for x in one])
    out.append(dict(mode="one_shot_keyed", reads=n, keys=n_keys, ms_call=round(one_ms, 3), ms_device=round(med([x[1] for x in one]), 3),
                    count_mode_used=int(s["count_mode_used"]), **ref_sum))
    print(json.dumps(out[-1]), flush=True)

    def count_mode(ptr, m, nt, f_ptr):
        """the count mode of a plain distance-0 run over m entries of nt nucleotides"""
        s = dd.run_device(ptr, f_ptr, d_cid.data_ptr(), d_keep.data_ptr(), m, nt, 0)
        return int(s["count_mode_used"])

    # (label, accumulator factory, add(acc, lo, m), map(acc, lo, m), compared with the one-shot run, entry pointer + bytes + nt)
    def keyed(key_nt):
        def add(acc, lo, m):
            return acc.add_device(d_w.data_ptr() + 8 * lo, d_k.data_ptr() + 8 * lo, d_f.data_ptr() + lo, m, lo)

        def mp(acc, lo, m):
            return acc.map_device(d_w.data_ptr() + 8 * lo, d_k.data_ptr() + 8 * lo, d_f.data_ptr() + lo, m, lo, d_cid.data_ptr() + 4 * lo,
                                  d_keep.data_ptr() + lo)
        ent = (d_p, 8, wnt + knt) if key_nt else (d_e, 16, 64)
        return ("keyed, key_nt %d" % key_nt, lambda: dd.keyed_accumulator(wnt, key_nt), add, mp, True, ent)

    def plain():
        def add(acc, lo, m):
            return acc.add_device(d_p.data_ptr() + 8 * lo, d_f.data_ptr() + lo, m, lo)

        def mp(acc, lo, m):
            return acc.map_device(d_p.data_ptr() + 8 * lo, d_f.data_ptr() + lo, m, lo, d_cid.data_ptr() + 4 * lo, d_keep.data_ptr() + lo)
        return ("plain, word_nt %d (packed)" % (wnt + knt), lambda: dd.accumulator(wnt + knt), add, mp, False, (d_p, 8, wnt + knt))

    for label, make, add, mp, compare, (d_ent, ebytes, ent_nt) in (keyed(16), keyed(0), plain()):
        for k in a.chunks:
            cuts = [n * i // k for i in range(k + 1)]
            t_add, t_map, t_fin = [[] for _ in range(k)], [[] for _ in range(k)], []
            for it in range(a.repeat + 1):
                d_cid.zero_()
                d_keep.zero_()
                acc = make()
                for i in range(k):
                    ms, _ = clock(lambda: add(acc, cuts[i], cuts[i + 1] - cuts[i]))
                    if it:
                        t_add[i].append(ms)
                ms, s = clock(lambda: acc.finish(d, humid_amd.DIRECTIONAL))
                if it:
                    t_fin.append(ms)
                unknown = 0
                for i in range(k):
                    ms, u = clock(lambda: mp(acc, cuts[i], cuts[i + 1] - cuts[i]))
                    unknown += u
                    if it:
                        t_map[i].append(ms)
                torch.cuda.synchronize()
                if unknown or (compare and not (torch.equal(d_cid, ref_cid) and torch.equal(d_keep, ref_keep) and
                                                {x: int(s[x]) for x in FIELDS} == ref_sum)):
                    sys.exit("bench_accum_keyed.py: %s in %d chunks differs from the one-shot run" % (label, k))
            info = acc.info()
            madd, mmap, fin = [med(x) for x in t_add], [med(x) for x in t_map], med(t_fin)
            total = sum(madd) + fin + sum(mmap)
            mode = count_mode(d_ent.data_ptr(), cuts[1], ent_nt, d_f.data_ptr())
            rec = dict(mode=label, chunks=k, reads=n, identical=compare, entries=info["unique"], keys=info.get("n_keys"),
                       count_mode_used=mode, ms_total=round(total, 3), ratio_to_one_shot=round(total / one_ms, 3),
                       ms_add=[round(x, 3) for x in madd], ms_finish=round(fin, 3), ms_map=[round(x, 3) for x in mmap])
            out.append(rec)
            print(json.dumps(rec), flush=True)

    print("\n| run | chunks | count mode | add (ms) | finish (ms) | map (ms) | total (ms) | x one-shot |\n|---|---|---|---|---|---|---|---|")
    print("| one shot, humid_dedup_run_keyed_device | | 0x%x | | | | %.3f (events: %.3f) | 1.00 |" % (
        out[0]["count_mode_used"], one_ms, out[0]["ms_device"]))
    for r in out[1:]:
        print("| %s | %d | 0x%x | %.3f (sum; %.3f .. %.3f) | %.3f | %.3f (sum; %.3f .. %.3f) | %.3f | %.2f |" % (
            r["mode"], r["chunks"], r["count_mode_used"], sum(r["ms_add"]), min(r["ms_add"]), max(r["ms_add"]), r["ms_finish"],
            sum(r["ms_map"]), min(r["ms_map"]), max(r["ms_map"]), r["ms_total"], r["ratio_to_one_shot"]))
    if a.json:
        with open(a.json, "w") as fh:
            for r in out:
                fh.write(json.dumps(r) + "\n")
    dd.close()


if __name__ == "__main__":
    main()
