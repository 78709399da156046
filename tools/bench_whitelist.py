"""Barcode whitelist correction (humid_dedup_run_keyed_corrected_device) against the keyed pass on keys that were
corrected beforehand: what the correction in front of the keyed pass costs.  One JSON line per shape on stdout;
device-event times, warmed contexts, median and quartiles over --passes passes, the compared passes alternated inside
this process.

  the metric words (10 M reads, 24 nt, d = 1) with 16-nt barcodes as keys:
  a  whitelist of 10^5 barcodes; keys drawn from it, 3 % with one substitution, 1 % random
  b  whitelist of 10^6 barcodes, the same error rates
  c  the worst case: whitelist of 10^5 barcodes, every key random (nearly every lane misses)

  t_corrected     run_keyed_corrected_device on the raw keys
  t_keyed         run_keyed_device on the truth-corrected keys and filtered' (the path as it was: the yardstick)
  t_kernel_coop   humid_whitelist_correct_device alone (the call waits for the stream), wave-cooperative kernel
  t_kernel_serial the same with option "whitelist_coop" 0: the lane-serial kernel
  t_set           wall time of humid_whitelist_set (table build, host array in)
  t_truth         wall time of the numpy truth (tests/whitelist_truth.py, correct_np)

"verified": key_out / status / counts of both kernels equal the truth; the corrected pass's cluster ids and keep flags
equal the keyed pass's on the precorrected inputs; barcode_status() equals the truth; group_keys() lies in the whitelist.

  python tools/bench_whitelist.py [--passes 25] [--warmup 3] [--shapes abc] [--which all|corrected]

--posterior: the correction by quality and abundance (humid_dedup_run_keyed_posterior_device) on shapes a and b, a
quality byte per barcode base drawn from Phred 2 .. 40, the shapes' own ambiguous keys present:
  t_posterior       run_keyed_posterior_device on the raw keys and qualities
  t_corrected       run_keyed_corrected_device on the same keys, the same build, alternated with it
  t_kernels_coop    humid_whitelist_correct_posterior_device alone (both kernels; the call waits for the stream)
  t_kernels_serial  the same with option "whitelist_coop" 0
"verified": key_out / status / summary of both kernel forms and the reads per barcode equal the numpy truth
(tests/whitelist_posterior_truth.py, posterior_np); the run's barcode_status() / barcode_posterior() equal it too.
--which posterior runs that pass alone (kernel traces).

  python tools/bench_whitelist.py --posterior [--passes 25] [--warmup 3] [--shapes ab] [--which all|posterior]
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
    ap.add_argument("--which", default="all", choices=("all", "corrected", "posterior"), help="corrected / posterior: that pass alone (kernel traces)")
    ap.add_argument("--posterior", action="store_true", help="the correction by quality and abundance next to the plain one")
    a = ap.parse_args()
    if a.posterior:
        return posterior_main(a)
    import torch

    import humid_amd
    from humid_amd.synth import synth_words
    import whitelist_truth as wt

    dev = torch.device("cuda:0")
    dc = humid_amd.Dedup(device=0)                               # corrected passes, wave-cooperative kernel
    dk = humid_amd.Dedup(device=0)                               # keyed passes on precorrected keys
    ds = humid_amd.Dedup(device=0)                               # the lane-serial kernel
    ds.set_option("whitelist_coop", 0)

    def to_dev(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)

    def timed_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    K = 16
    words, filt = synth_words(a.reads, 1002, 24)                 # bench.py's metric words
    n = len(filt)
    d_w, d_f = to_dev(words, np.int64), to_dev(filt, np.uint8)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_c2 = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k2 = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ko = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(66)

    def drawn(wl):
        keys, _ = wt.make_keys(rng, wl, K, n, p1=0.03, p2=0.0, pr=0.01, p_filt=0.0)
        return keys

    shapes = dict(a=("1e5-barcode whitelist, 3 % one substitution, 1 % random", 100_000, drawn),
                  b=("1e6-barcode whitelist, 3 % one substitution, 1 % random", 1_000_000, drawn),
                  c=("1e5-barcode whitelist, every key random", 100_000, lambda wl: wt.random_barcodes(rng, n, K)))
    for name in a.shapes:
        what, n_wl, make = shapes[name]
        wl = wt.whitelist_with_neighbours(rng, n_wl, K)
        keys = make(wl)
        t0 = time.perf_counter()
        t_key, t_status, t_counts = wt.correct_np(keys, filt, wl, K)
        t_truth = (time.perf_counter() - t0) * 1e3
        filt2 = ((filt != 0) | (t_status >= 3)).astype(np.uint8)
        ts = []
        for d in (dc, ds, dc, ds, dc):
            t0 = time.perf_counter()
            d.set_whitelist(wl, K)
            ts.append((time.perf_counter() - t0) * 1e3)
        d_key, d_key2, d_f2 = to_dev(keys, np.int64), to_dev(t_key, np.int64), to_dev(filt2, np.uint8)
        corrected = lambda: dc.run_keyed_corrected_device(d_w.data_ptr(), d_key.data_ptr(), d_f.data_ptr(), d_c.data_ptr(),  # noqa: E731
                                                          d_k.data_ptr(), n, word_nt=24, distance=1)
        keyed = lambda: dk.run_keyed_device(d_w.data_ptr(), d_key2.data_ptr(), d_f2.data_ptr(), d_c2.data_ptr(),  # noqa: E731
                                            d_k2.data_ptr(), n, word_nt=24, distance=1)
        kern = {}
        ok = True
        for label, d in (("coop", dc), ("serial", ds)):
            kern[label] = lambda d=d: d.correct_keys_device(d_key.data_ptr(), d_f.data_ptr(), d_ko.data_ptr(), d_st.data_ptr(), n)
            if a.which == "all":
                counts = kern[label]()
                ok = ok and bool(np.array_equal(counts, t_counts))
                ok = ok and bool(np.array_equal(d_ko.cpu().numpy().view(np.uint64), t_key))
                ok = ok and bool(np.array_equal(d_st.cpu().numpy(), t_status))
        tc, tk, tkc, tks = [], [], [], []
        for _ in range(a.warmup):
            corrected()
            if a.which == "all":
                keyed()
                kern["coop"]()
                kern["serial"]()
        for _ in range(a.passes):
            tc.append(timed_ms(corrected))
            if a.which == "all":
                tk.append(timed_ms(keyed))
                tkc.append(timed_ms(kern["coop"]))
                tks.append(timed_ms(kern["serial"]))
        info = dc.whitelist_info()
        line = dict(shape=name, what="10M metric words, 24 nt, d=1, 16-nt barcodes: " + what, reads=n,
                    whitelist_distinct=int(info["n_distinct"]), table_log2=info["table_log2"],
                    counts=dict(zip(("filtered", "exact", "corrected", "ambiguous", "unmatched"), (int(x) for x in t_counts))),
                    corrected=stats(tc))
        if a.which == "all":
            status, counts = dc.barcode_status()
            ok = ok and bool(np.array_equal(status, t_status) and np.array_equal(counts, t_counts))
            ok = ok and bool(torch.equal(d_c, d_c2)) and bool(torch.equal(d_k, d_k2))
            ok = ok and bool(np.all(np.isin(dc.group_keys(), wl)))
            sc, sk = stats(tc), stats(tk)
            line.update(keyed=sk, kernel_coop=stats(tkc), kernel_serial=stats(tks), set=stats(ts),
                        correction_cost_ms=round(sc["median_ms"] - sk["median_ms"], 4),
                        correction_share_of_corrected=round((sc["median_ms"] - sk["median_ms"]) / sc["median_ms"], 4),
                        truth_ms=round(t_truth, 1), verified=ok)
        print(json.dumps(line), flush=True)
        del d_key, d_key2, d_f2
    for d in (dc, dk, ds):
        d.close()


def posterior_main(a):
    import torch

    import humid_amd
    from humid_amd.synth import synth_words
    import whitelist_posterior_truth as pt
    import whitelist_truth as wt

    dev = torch.device("cuda:0")
    dp = humid_amd.Dedup(device=0)                               # posterior passes, wave-cooperative decision kernel
    dc = humid_amd.Dedup(device=0)                               # plain corrected passes
    ds = humid_amd.Dedup(device=0)                               # the lane-serial decision kernel
    ds.set_option("whitelist_coop", 0)

    def to_dev(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)

    def timed_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    K = 16
    words, filt = synth_words(a.reads, 1002, 24)                 # bench.py's metric words
    n = len(filt)
    d_w, d_f = to_dev(words, np.int64), to_dev(filt, np.uint8)
    d_c = torch.zeros(n, dtype=torch.int32, device=dev)
    d_k = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_ko = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(66)
    sizes = dict(a=100_000, b=1_000_000)
    for name in a.shapes:
        if name not in sizes:
            continue
        wl = wt.whitelist_with_neighbours(rng, sizes[name], K)
        keys, _ = wt.make_keys(rng, wl, K, n, p1=0.03, p2=0.0, pr=0.01, p_filt=0.0)      # the draw of shapes a and b
        quals = rng.integers(35, 74, size=(n, K), dtype=np.uint8)
        t0 = time.perf_counter()
        t_key, t_status, t_sm, t_nw = pt.posterior_np(keys, quals, filt, wl, K)
        t_truth = (time.perf_counter() - t0) * 1e3
        for d in (dp, dc, ds):
            d.set_whitelist(wl, K)
        d_key, d_q = to_dev(keys, np.int64), to_dev(quals, np.uint8)
        posterior = lambda: dp.run_keyed_posterior_device(d_w.data_ptr(), d_key.data_ptr(), d_q.data_ptr(), d_f.data_ptr(),  # noqa: E731
                                                          d_c.data_ptr(), d_k.data_ptr(), n, word_nt=24, distance=1)
        corrected = lambda: dc.run_keyed_corrected_device(d_w.data_ptr(), d_key.data_ptr(), d_f.data_ptr(), d_c.data_ptr(),  # noqa: E731
                                                          d_k.data_ptr(), n, word_nt=24, distance=1)
        kern, ok = {}, True
        uw = np.unique(wl)
        want_counts = np.asarray([t_nw.get(int(w), 0) for w in uw], np.uint32)
        for label, d in (("coop", dp), ("serial", ds)):
            kern[label] = lambda d=d: d.correct_keys_posterior_device(d_key.data_ptr(), d_q.data_ptr(), d_f.data_ptr(),
                                                                      d_ko.data_ptr(), d_st.data_ptr(), n)
            if a.which == "all":
                ok = ok and kern[label]() == t_sm
                ok = ok and bool(np.array_equal(d_ko.cpu().numpy().view(np.uint64), t_key))
                ok = ok and bool(np.array_equal(d_st.cpu().numpy(), t_status))
                ok = ok and bool(np.array_equal(d.whitelist_counts(uw), want_counts))
        tp, tc, tkc, tks = [], [], [], []
        for _ in range(a.warmup):
            posterior()
            if a.which == "all":
                corrected()
                kern["coop"]()
                kern["serial"]()
        for _ in range(a.passes):
            tp.append(timed_ms(posterior))
            if a.which == "all":
                tc.append(timed_ms(corrected))
                tkc.append(timed_ms(kern["coop"]))
                tks.append(timed_ms(kern["serial"]))
        info = dp.whitelist_info()
        line = dict(shape=name, what="10M metric words, 24 nt, d=1, 16-nt barcodes, a quality per base: 1e%d-barcode whitelist, "
                    "3 %% one substitution, 1 %% random" % (5 if name == "a" else 6), reads=n,
                    whitelist_distinct=int(info["n_distinct"]), table_log2=info["table_log2"], min_odds=39,
                    counts=dict(zip(("filtered", "exact", "corrected", "ambiguous", "unmatched"), t_sm["counts"])),
                    multi=t_sm["multi"], rescued=t_sm["rescued"], posterior=stats(tp))
        if a.which == "all":
            status, counts = dp.barcode_status()
            ok = ok and bool(np.array_equal(status, t_status)) and [int(c) for c in counts] == t_sm["counts"]
            ok = ok and dp.barcode_posterior() == dict(multi=t_sm["multi"], rescued=t_sm["rescued"])
            ok = ok and bool(np.all(np.isin(dp.group_keys(), wl)))
            sp, sc = stats(tp), stats(tc)
            line.update(corrected=sc, kernels_coop=stats(tkc), kernels_serial=stats(tks),
                        posterior_over_corrected=round(sp["median_ms"] / sc["median_ms"], 4),
                        posterior_extra_ms=round(sp["median_ms"] - sc["median_ms"], 4), truth_ms=round(t_truth, 1), verified=bool(ok))
        print(json.dumps(line), flush=True)
        del d_key, d_q
    for d in (dp, dc, ds):
        d.close()


if __name__ == "__main__":
    main()
