"""The whitelist from the data (humid_whitelist_discover_device) beside the correction against a whitelist
(humid_whitelist_correct_device) over the same reads: both make one table probe per read; the discovery also counts,
sorts the distinct barcodes, selects, merges and builds the whitelist's table.  One JSON line on stdout; times from
device events recorded on the context's stream around calls that end in a stream wait, warmed, median and quartiles over
--passes passes, the two calls alternated inside this process.

  shape: --reads reads (10 M), 16-nt barcodes, --cells cells (5 000) with geometric sizes, 1 % of the reads one
  substitution off, shuffled
  t_discover   humid_whitelist_discover_device, expected = --cells, merge ratio 5
  t_correct    humid_whitelist_correct_device against the whitelist the discovery installed
  t_truth      wall time of the numpy truth (tests/cells_truth.py)

"verified": cells, reads, summary and histogram equal the truth.  HUMID_KERNEL_TIMING=1 makes the library print the
time between the stages of every discovery on stderr (run it with few passes).

--sizes uniform (every cell the same share of the reads) and --order sorted (equal barcodes side by side: one probe and
one atomic add per wave and barcode) are the shape's two variations that tell the count kernel's costs apart.

  python tools/bench_cells.py [--passes 25] [--warmup 3] [--reads 10000000] [--cells 5000] [--sizes geometric|uniform]
                              [--order shuffled|sorted]
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


def make_reads(rng, n, n_cells, k, p_err, uniform=False):
    """cells with geometric sizes (the largest about 100 times the smallest), p_err of the reads one substitution off"""
    cells = rng.integers(0, 1 << (2 * k), size=n_cells, dtype=np.uint64)
    w = np.ones(n_cells) if uniform else np.exp(-np.log(100.0) * np.arange(n_cells) / max(n_cells - 1, 1))
    keys = cells[rng.choice(n_cells, size=n, p=w / w.sum())]
    sub = rng.integers(1, 4, size=n).astype(np.uint64) << (np.uint64(2) * rng.integers(0, k, size=n).astype(np.uint64))
    return np.where(rng.random(n) < p_err, keys ^ sub, keys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--cells", type=int, default=5000)
    ap.add_argument("--sizes", default="geometric", choices=("geometric", "uniform"))
    ap.add_argument("--order", default="shuffled", choices=("shuffled", "sorted"))
    a = ap.parse_args()
    import torch

    import humid_amd
    import cells_truth as ct

    K = 16
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    dd = humid_amd.Dedup(device=0, stream=stream.cuda_stream)
    rng = np.random.default_rng(77)
    keys = make_reads(rng, a.reads, a.cells, K, 0.01, uniform=a.sizes == "uniform")
    if a.order == "sorted":
        keys = np.sort(keys)
    filt = np.zeros(a.reads, np.uint8)
    t0 = time.perf_counter()
    t_cells, t_reads, t_sm, t_hist = ct.discover(keys, filt, K, ct.EXPECTED, a.cells, 5)
    t_truth = (time.perf_counter() - t0) * 1e3
    d_key = torch.from_numpy(keys.view(np.int64)).to(dev)
    d_filt = torch.from_numpy(filt).to(dev)
    d_out = torch.zeros(a.reads, dtype=torch.int64, device=dev)
    d_status = torch.zeros(a.reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def timed_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            fn()
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    discover = lambda: dd.discover_whitelist(d_key, d_filt, barcode_nt=K, expected=a.cells, merge_ratio=5)   # noqa: E731
    correct = lambda: dd.correct_keys_device(d_key.data_ptr(), d_filt.data_ptr(), d_out.data_ptr(), d_status.data_ptr(), a.reads)   # noqa: E731
    sm = discover()
    cells, reads = dd.discovered_cells()
    hn, hb = dd.barcode_count_hist()
    ok = sm == t_sm and np.array_equal(cells, t_cells) and np.array_equal(reads, t_reads) and \
        np.array_equal(hn, t_hist[0]) and np.array_equal(hb, t_hist[1])
    counts = correct()
    for _ in range(a.warmup):
        discover()
        correct()
    td, tc = [], []
    for _ in range(a.passes):
        td.append(timed_ms(discover))
        tc.append(timed_ms(correct))
    print(json.dumps(dict(reads=a.reads, barcode_nt=K, planted_cells=a.cells, sizes=a.sizes, order=a.order, summary=sm, verified=bool(ok),
                          correct_counts=[int(x) for x in counts], t_discover=stats(td), t_correct=stats(tc),
                          ratio=round(float(np.median(td) / np.median(tc)), 2), t_truth_ms=round(t_truth, 1))))
    dd.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
