"""Cost of the barcode counter and the posterior's prior fed in chunks (humid_cells_*, humid_whitelist_prior_*) beside
the one-shot calls: 10 M reads, 16-nt barcodes (a few thousand cells with skewed sizes, their one-substitution errors
and ambient barcodes), keys, qualities and filter flags resident on the device.

    python tools/bench_cells_accum.py [--reads 10000000] [--cells 3000] [--chunks 1 4 16] [--repeat 3] [--json FILE]

One process, one build.  Per configuration one untimed pass and --repeat timed ones; a time is a host clock around
calls that end in a stream wait, the median over the repeats.  Every chunked result is compared with the one-shot's.
  discover   humid_whitelist_discover_device  |  humid_cells_begin + adds + humid_cells_finish, with the default table
             (2^16 slots at begin: it grows) and with a table sized in advance (option cells_table_log2)
  posterior  humid_whitelist_correct_posterior_device  |  prior_begin + prior adds + the corrections of all chunks
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--cells", type=int, default=3000)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch

    import humid_amd

    if not torch.cuda.is_available():
        sys.exit("bench_cells_accum.py needs a GPU: there is no CPU fallback")
    dev = torch.device("cuda", 0)
    n, k = a.reads, 16
    rng = np.random.default_rng(1003)
    cells = np.unique(rng.integers(0, 4 ** k, a.cells + 64).astype(np.uint64))[:a.cells]
    p = 1.0 / (np.arange(len(cells)) + 10.0)
    keys = cells[rng.choice(len(cells), n, p=p / p.sum())]
    u = rng.random(n)
    sub = rng.integers(1, 4, size=n).astype(np.uint64) << (np.uint64(2) * rng.integers(0, k, size=n).astype(np.uint64))
    keys = np.where(u < 0.05, keys ^ sub, keys)
    keys = np.where(u > 0.97, rng.integers(0, 4 ** k, size=n).astype(np.uint64), keys)
    filt = (rng.random(n) < 0.02).astype(np.uint8)
    quals = rng.integers(33 + 2, 33 + 41, size=(n, k), dtype=np.uint8)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.int64 if x.dtype == np.uint64 else x.dtype)).to(dev)

    d_k, d_f, d_q = up(keys), up(filt), up(quals)
    d_out = torch.zeros(n, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    dd = humid_amd.Dedup(device=0)
    rows = []

    def timed(name, chunks, fn):
        fn()
        ts = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            res = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        row = dict(run=name, chunks=chunks, ms=round(statistics.median(ts), 3))
        row.update(res[1] if isinstance(res, tuple) and isinstance(res[1], dict) else {})
        rows.append(row)
        print(json.dumps(row), flush=True)
        return res

    def pieces(c):
        size = (n + c - 1) // c
        return [(lo, min(lo + size, n)) for lo in range(0, n, size)]

    # ---- discover ----
    want = timed("discover one-shot", 0, lambda: (dd.discover_whitelist(d_k, d_f, barcode_nt=k, expected=a.cells, merge_ratio=3), {}))[0]
    want_cells = dd.discovered_cells()
    for sized in (0, 1):
        for c in a.chunks:
            def counter():
                dd.set_option("cells_table_log2", max(4, int(want["distinct"] * 3).bit_length()) if sized else 0)
                bc = dd.barcode_counter(barcode_nt=k)
                t0 = time.perf_counter()
                for lo, hi in pieces(c):
                    bc.add_device(d_k.data_ptr() + 8 * lo, d_f.data_ptr() + lo, hi - lo)
                t1 = time.perf_counter()
                sm = bc.finish(expected=a.cells, merge_ratio=3)
                t2 = time.perf_counter()
                info = bc.info()
                return sm, dict(adds_ms=round((t1 - t0) * 1e3, 3), finish_ms=round((t2 - t1) * 1e3, 3), n_grown=info["n_grown"],
                                table_log2=info["table_log2"])
            got = timed("counter, table %s" % ("sized in advance" if sized else "default"), c, counter)[0]
            assert got == want and all(np.array_equal(x, y) for x, y in zip(dd.discovered_cells(), want_cells))
    dd.set_option("cells_table_log2", 0)

    # ---- posterior ----
    def one_shot():
        return dd.correct_keys_posterior_device(d_k.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_out.data_ptr(), d_st.data_ptr(), n), {}
    want = timed("posterior one-shot", 0, one_shot)[0]
    want_out, want_st = d_out.clone(), d_st.clone()
    for c in a.chunks:
        def prior():
            dd.prior_begin()
            t0 = time.perf_counter()
            for lo, hi in pieces(c):
                dd.prior_add_device(d_k.data_ptr() + 8 * lo, d_f.data_ptr() + lo, hi - lo)
            t1 = time.perf_counter()
            tot = dict(counts=[0] * 5, multi=0, rescued=0)
            for lo, hi in pieces(c):
                s = dd.correct_keys_prior_device(d_k.data_ptr() + 8 * lo, d_q.data_ptr() + k * lo, d_f.data_ptr() + lo,
                                                 d_out.data_ptr() + 8 * lo, d_st.data_ptr() + lo, hi - lo)
                tot = dict(counts=[x + y for x, y in zip(tot["counts"], s["counts"])], multi=tot["multi"] + s["multi"],
                           rescued=tot["rescued"] + s["rescued"])
            t2 = time.perf_counter()
            return tot, dict(adds_ms=round((t1 - t0) * 1e3, 3), correct_ms=round((t2 - t1) * 1e3, 3))
        got = timed("prior + corrections", c, prior)[0]
        assert got == want and torch.equal(d_out, want_out) and torch.equal(d_st, want_st)
    dd.close()

    print("\n| run | chunks | total ms | adds | finish / corrections | growths | table |\n|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %.2f | %s | %s | %s | %s |" % (r["run"], r["chunks"] or "", r["ms"], r.get("adds_ms", ""),
                                                       r.get("finish_ms", r.get("correct_ms", "")), r.get("n_grown", ""),
                                                       ("2^%d" % r["table_log2"]) if "table_log2" in r else ""))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
