"""Grouped deduplication (humid_dedup_run_grouped_device) against the plain pass and against a loop of per-group
passes.  One JSON line per shape on stdout; device-event times of every pass, median and spread over --passes
warmed passes.

  A  the metric words (10 M reads, 24 nt, d = 1): n_groups = 1 against run_device, alternated within this
     process -- with group = NULL, and with an all-zero group array (checked on the device)
  B  the same words in 4096 groups (30 nt internal), against run_device on the same words (in blocks)
  C  the per-cell shape: 10^5 groups x ~100 reads, 12-nt UMIs, d = 1
  D  C done as a loop of per-group run_device calls over the first 1000 groups, extrapolated to all groups

"verified": the grouped pass against tests/grouped_truth.py's repetition-code truth (the rank of the group in a
repetition code in front of the word, one plain device pass); D against C's results for its groups.

  python tools/bench_grouped.py [--passes 25] [--warmup 3] [--shapes ABCD] [--which both|plain|grouped]
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
    ap.add_argument("--passes", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="ABCD")
    ap.add_argument("--loop-groups", type=int, default=1000)
    ap.add_argument("--which", default="both", choices=("both", "plain", "grouped"),
                    help="B only: time one side alone (kernel traces)")
    a = ap.parse_args()
    import torch

    import grouped_truth as gt
    import humid_amd
    from humid_amd.synth import synth_words

    dev = torch.device("cuda:0")
    dd = humid_amd.Dedup(device=0)
    ref = humid_amd.Dedup(device=0)
    engine = gt.device_engine(ref)

    def to_dev(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)

    def timed_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def out(line):
        print(json.dumps(line), flush=True)

    def grouped_fn(d_w, d_g, d_f, d_c, d_k, n, n_groups, word_nt):
        return lambda: dd.run_grouped_device(d_w.data_ptr(), d_g.data_ptr(), d_f.data_ptr(), d_c.data_ptr(),
                                             d_k.data_ptr(), n, n_groups, word_nt=word_nt, distance=1)

    def plain_fn(d_w, d_f, d_c, d_k, n, word_nt):
        return lambda: dd.run_device(d_w.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n,
                                     word_nt=word_nt, distance=1)

    def verify(words, groups, filt, word_nt, d_c, d_k):
        t = gt.repetition(words, groups, filt, word_nt, 1, 0, engine=engine)
        cid = d_c.cpu().numpy().view(np.uint32)
        keep = d_k.cpu().numpy()
        return bool(np.array_equal(cid, t["cid"]) and np.array_equal(keep, t["keep"])), t

    if "A" in a.shapes or "B" in a.shapes:
        words, filt = synth_words(10_000_000, 1002, 24)           # bench.py's metric words
        n = len(filt)
        d_w, d_f = to_dev(words, np.int64), to_dev(filt, np.uint8)
        d_c = torch.zeros(n, dtype=torch.int32, device=dev)
        d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        plain = plain_fn(d_w, d_f, d_c, d_k, n, 24)
        if "A" in a.shapes:
            zeros = np.zeros(n, np.uint32)
            d_g = to_dev(zeros, np.int32)
            grouped_null = lambda: dd.run_grouped_device(d_w.data_ptr(), 0, d_f.data_ptr(), d_c.data_ptr(),  # noqa: E731
                                                         d_k.data_ptr(), n, 1, word_nt=24, distance=1)
            grouped_zero = grouped_fn(d_w, d_g, d_f, d_c, d_k, n, 1, 24)
            for _ in range(a.warmup):
                plain()
                grouped_null()
                grouped_zero()
            tp, tn, tz = [], [], []
            for _ in range(a.passes):
                tp.append(timed_ms(plain))
                tn.append(timed_ms(grouped_null))
                tz.append(timed_ms(grouped_zero))
            ok, _ = verify(words, zeros, filt, 24, d_c, d_k)
            sp, sn, sz = stats(tp), stats(tn), stats(tz)
            out(dict(shape="A", what="10M reads, 24 nt, d=1: n_groups=1 vs run_device (alternated)", reads=n,
                     n_groups=1, grouped=sn, grouped_zero_array=sz, plain=sp,
                     ratio=round(sn["median_ms"] / sp["median_ms"], 4),
                     ratio_zero_array=round(sz["median_ms"] / sp["median_ms"], 4),
                     note="grouped: group = NULL; grouped_zero_array: an all-zero group array (checked on the device)",
                     target="within the plain pass's run-to-run spread", verified=ok))
        if "B" in a.shapes:
            rng = np.random.default_rng(4096)
            groups = rng.integers(0, 4096, size=n).astype(np.uint32)
            d_g = to_dev(groups, np.int32)
            grouped = grouped_fn(d_w, d_g, d_f, d_c, d_k, n, 4096, 24)
            tp, tg = [], []
            # in blocks, not alternated: a context remembers one shape's count-stage verdict (prefix_fits_ordered),
            # and alternating two shapes would make both pay its sampled histogram and host wait every pass
            if a.which in ("both", "plain"):
                for _ in range(a.warmup):
                    plain()
                tp = [timed_ms(plain) for _ in range(a.passes)]
            if a.which in ("both", "grouped"):
                for _ in range(a.warmup):
                    grouped()
                tg = [timed_ms(grouped) for _ in range(a.passes)]
                ok, _ = verify(words, groups, filt, 24, d_c, d_k)
            if a.which == "both":
                sp, sg = stats(tp), stats(tg)
                out(dict(shape="B", what="the same words in 4096 groups (30 nt internal) vs run_device, in blocks",
                         reads=n, n_groups=4096, grouped=sg, plain=sp, ratio=round(sg["median_ms"] / sp["median_ms"], 4),
                         target="<= 1.3x the plain pass", verified=ok))
        del d_w, d_f, d_c, d_k
    if "C" in a.shapes or "D" in a.shapes:
        n_groups, per = 100_000, 100
        n = n_groups * per
        rng = np.random.default_rng(12)
        words, filt = synth_words(n, 1003, 12)                     # 12-nt UMIs with their families' errors
        groups = np.sort(rng.integers(0, n_groups, size=n)).astype(np.uint32)
        perm = rng.permutation(n)                                  # cells interleaved in input order
        words, filt, groups = words[perm], filt[perm], groups[perm]
        d_w, d_f, d_g = to_dev(words, np.int64), to_dev(filt, np.uint8), to_dev(groups, np.int32)
        d_c = torch.zeros(n, dtype=torch.int32, device=dev)
        d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        grouped = grouped_fn(d_w, d_g, d_f, d_c, d_k, n, n_groups, 12)
        for _ in range(a.warmup):
            grouped()
        tg = [timed_ms(grouped) for _ in range(a.passes)]
        ok, t = verify(words, groups, filt, 12, d_c, d_k)
        sg = stats(tg)
        out(dict(shape="C", what="per-cell: 1e5 groups x ~100 reads, 12-nt UMIs, d=1", reads=n, n_groups=n_groups,
                 grouped=sg, verified=ok))
        if "D" in a.shapes:
            L = a.loop_groups
            cid_c = t["cid"]
            sel = [np.flatnonzero((groups == g)) for g in range(L)]
            dev_sets = []
            for s_ in sel:
                m = len(s_)
                dev_sets.append((to_dev(words[s_], np.int64), to_dev(filt[s_], np.uint8),
                                 torch.zeros(m, dtype=torch.int32, device=dev),
                                 torch.zeros(m, dtype=torch.uint8, device=dev), m))
            torch.cuda.synchronize()

            def loop():
                for (w_, f_, c_, k_, m) in dev_sets:
                    dd.run_device(w_.data_ptr(), f_.data_ptr(), c_.data_ptr(), k_.data_ptr(), m, word_nt=12, distance=1)
            for _ in range(a.warmup):
                loop()
            tl = [timed_ms(loop) for _ in range(max(3, a.passes // 5))]
            ok_d, base = True, 0
            for s_, (w_, f_, c_, k_, m) in zip(sel, dev_sets):        # per-group ids + offsets == C's ids
                c = c_.cpu().numpy().view(np.uint32).astype(np.int64)
                c = np.where(c > 0, c + base, 0)
                ok_d = ok_d and np.array_equal(c, cid_c[s_].astype(np.int64))
                base = int(c.max()) if c.max() > base else base
            sl = stats(tl)
            extr = sl["median_ms"] * n_groups / L
            out(dict(shape="D", what="C as a loop of per-group run_device calls over the first %d groups" % L,
                     label="extrapolated", loop_groups=L, loop=sl, extrapolated_ms=round(extr, 2),
                     per_pass_ms=round(sl["median_ms"] / L, 4), speedup_C_over_D=round(extr / sg["median_ms"], 1),
                     target="C >= 50x faster than D", verified=bool(ok_d)))
    dd.close()
    ref.close()


if __name__ == "__main__":
    main()
