"""Per-group statistics reduced on the device (humid_group_stats_device) against what a caller paid for the same
table before: leaves() -- which includes humid_get_leaf_groups, a host-side split of every internal word -- followed
by the numpy reduction.  One JSON line per shape on stdout.

  the metric words (10 M reads, 24 nt, d = 1) under
  a  2.5 M distinct random 64-bit keys (mostly one-leaf groups)
  b  one key (one group holds every leaf)
  c  one key with half the reads + 10^5 small ones

  t_device  device events around the FIRST group_stats_device() after a keyed run (the later ones find the cached
            arrays); a run in front of every sample; median and quartiles of --passes samples after --warmup
  t_host    wall time of leaves() + the numpy reduction (--host-passes samples); t_host_numpy: the reduction alone

"verified": the device's arrays equal the numpy table of the same run.

  python tools/bench_group_stats.py [--passes 25] [--warmup 3] [--host-passes 5] [--shapes abc]
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


def host_table(lv, G):
    """the reduction a caller ran over the downloaded leaf arrays"""
    g = lv["group"].astype(np.int64)
    leaf_off = np.searchsorted(g, np.arange(G + 1), side="left").astype(np.uint32)
    reads = np.bincount(g, weights=lv["count"], minlength=G).astype(np.uint64)
    edges = (np.bincount(g, weights=lv["degree"], minlength=G).astype(np.uint64) >> np.uint64(1)).astype(np.uint32)
    cid = lv["cluster_id"]
    pairs = np.unique((g.astype(np.uint64) << np.uint64(32)) | cid.astype(np.uint64))
    clusters = np.bincount((pairs >> np.uint64(32)).astype(np.int64), minlength=G)
    cluster_off = np.concatenate([[0], np.cumsum(clusters)]).astype(np.uint32)
    return dict(reads=reads, edges=edges, leaf_off=leaf_off, cluster_off=cluster_off)


class _DevArray:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-passes", type=int, default=5)
    ap.add_argument("--shapes", default="abc")
    ap.add_argument("--reads", type=int, default=10_000_000)
    a = ap.parse_args()
    import torch

    import humid_amd
    from humid_amd.synth import synth_words

    dev = torch.device("cuda:0")
    dd = humid_amd.Dedup(device=0)

    def to_dev(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)

    def view(ptr, n, typestr, dtype):
        if n == 0:
            return np.zeros(0, dtype)
        return torch.as_tensor(_DevArray(ptr, n, typestr), device=dev).cpu().numpy().view(dtype)

    words, filt = synth_words(a.reads, 1002, 24)                 # bench.py's metric words
    n = len(filt)
    d_w, d_f = to_dev(words, np.int64), to_dev(filt, np.uint8)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(65)
    small = rng.integers(0, 1 << 64, size=100_000, dtype=np.uint64)
    shapes = dict(
        a=("2.5e6 distinct random 64-bit keys",
           lambda: rng.integers(0, 1 << 64, size=2_500_000, dtype=np.uint64)[rng.integers(0, 2_500_000, size=n)]),
        b=("one key", lambda: np.full(n, 0x0123456789ABCDEF, np.uint64)),
        c=("one key with half the reads + 1e5 small ones",
           lambda: np.where(rng.random(n) < 0.5, np.uint64(1 << 63), small[rng.integers(0, len(small), size=n)])))
    for name in a.shapes:
        what, make = shapes[name]
        d_key = to_dev(make(), np.int64)

        def run():
            dd.run_keyed_device(d_w.data_ptr(), d_key.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n,
                                word_nt=24, distance=1)

        td, t_run = [], []
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        for i in range(a.warmup + a.passes):
            e0.record()
            run()
            e1.record()
            out = dd.group_stats_device()                        # the first call after the run: computes
            e2.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                t_run.append(e0.elapsed_time(e1))
                td.append(e1.elapsed_time(e2))
        e1.record()
        again = dd.group_stats_device()                          # a later call: the cached arrays
        e2.record()
        torch.cuda.synchronize()
        t_cached = e1.elapsed_time(e2)
        G = out["n"]
        got = dict(reads=view(out["reads"], G, "<i8", np.uint64), edges=view(out["edges"], G, "<i4", np.uint32),
                   leaf_off=view(out["leaf_off"], G + 1, "<i4", np.uint32),
                   cluster_off=view(out["cluster_off"], G + 1, "<i4", np.uint32))
        th, tn, want = [], [], None
        for _ in range(a.host_passes):
            t0 = time.perf_counter()
            lv = dd.leaves()
            t1 = time.perf_counter()
            want = host_table(lv, G)
            t2 = time.perf_counter()
            th.append((t2 - t0) * 1e3)
            tn.append((t2 - t1) * 1e3)
        ok = again == out and all(np.array_equal(got[k], want[k]) for k in want)
        s = dd.summary
        ok = ok and int(got["reads"].sum()) == s["usable"] and int(got["leaf_off"][-1]) == s["unique"] \
            and int(got["cluster_off"][-1]) == s["clusters"] and int(got["edges"].astype(np.uint64).sum()) == s["edges"]
        sd, sh = stats(td), stats(th)
        spread = (sd["p75_ms"] - sd["p25_ms"]) + (sh["p75_ms"] - sh["p25_ms"])
        print(json.dumps(dict(shape=name, what="10M metric words, 24 nt, d=1, " + what, reads=n, groups=int(G),
                              unique=int(s["unique"]), largest_group_leaves=int(np.diff(got["leaf_off"].astype(np.int64)).max()) if G else 0,
                              t_device=sd, t_device_cached_call_ms=round(t_cached, 4), t_keyed_run=stats(t_run), t_host=sh,
                              t_host_numpy=stats(tn), host_over_device=round(sh["median_ms"] / sd["median_ms"], 1),
                              device_faster_beyond_spread=bool(sh["median_ms"] - sd["median_ms"] > spread), verified=bool(ok))),
              flush=True)
        del d_key
    dd.close()


if __name__ == "__main__":
    main()
