"""Duplex consensus reads per cluster (humid_duplex_consensus_device) beside the plain consensus of the same layer with
the same ids (humid_consensus_device): what the two classes of voters cost.  One JSON line on stdout; device-event
times, warmed context, median and quartiles over --passes calls, the two calls alternated inside this process.

  the metric words (10 M reads, 24 nt, d = 1) as clusters; two layers of 150 nt reads from humid_amd.synth.synth_reads
  (seeds 71 and 72: one template pair per cluster, substitutions at --p-sub, qualities Phred 40 with probability 0.8,
  else uniform in 2 .. 39); every read but the representative is on the other strand with probability 1 / 2, and a
  read of the other strand carries the templates exchanged -- about half of each multi-read cluster votes from the
  other layer

  t_duplex_device      humid_duplex_consensus_device: two host waits inside, the results left in HBM
  t_consensus_device   humid_consensus_device on layer 1 with the same ids (the yardstick: same build, same run)
  bytes_read           what each call has to read: a member's vote is one base byte and one quality byte, from one blob
                       pair for the plain call and from two for the duplex call -- the same count -- plus the
                       representatives' records, off (twice for the duplex call), ids, keep (and strand)
  hbm_share            bytes_read + bytes written at 6.3 TB/s (the achievable HBM rate DESIGN.md uses) over the median

"verified": on --sample clusters (the largest ones and a random draw) out_off-relative bytes, depth, errors, depth_same,
depth_other and disagree equal the numpy truth of tests/duplex_truth.py.

  python tools/bench_duplex_consensus.py [--passes 15] [--warmup 2] [--reads 10000000] [--sample 3000]
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--p-sub", type=float, default=5e-3)
    ap.add_argument("--sample", type=int, default=3000, help="clusters verified against the truth (0: none)")
    a = ap.parse_args()
    import torch

    import humid_amd
    from humid_amd.synth import synth_reads, synth_words
    import duplex_truth as dt

    dev = torch.device("cuda:0")
    dd = humid_amd.Dedup(device=0)

    def to_dev(x, t):
        return torch.from_numpy(np.ascontiguousarray(x).view(t)).to(dev)

    def timed_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    words, filt = synth_words(a.reads, 1002, 24)                 # bench.py's metric words
    n, L = len(filt), a.read_len
    cid, keep, s0 = dd.run(words, filt, word_nt=24, distance=1)
    C = int(s0["clusters"])
    rng = np.random.default_rng(73)
    strand = rng.integers(0, 2, n, dtype=np.uint8)
    strand[cid == 0] = 2
    rs = dt.rep_strand(cid, keep, strand)
    other = np.flatnonzero((cid != 0) & (strand != rs))
    b1, q1 = synth_reads(cid, 71, read_len=L, p_sub=a.p_sub)
    b2, q2 = synth_reads(cid, 72, read_len=L, p_sub=a.p_sub)
    for x, y in ((b1, b2), (q1, q2)):                            # a read of the other strand: the two records exchanged
        for lo in range(0, len(other), 500_000):
            idx = other[lo:lo + 500_000]
            t = x[idx].copy()
            x[idx] = y[idx]
            y[idx] = t
    d_off = to_dev(np.arange(n + 1, dtype=np.uint64) * np.uint64(L), np.int64)
    d_c, d_k, d_s = to_dev(cid, np.int32), to_dev(keep, np.uint8), to_dev(strand, np.uint8)
    d_b1, d_q1 = to_dev(b1.reshape(-1), np.uint8), to_dev(q1.reshape(-1), np.uint8)
    d_b2, d_q2 = to_dev(b2.reshape(-1), np.uint8), to_dev(q2.reshape(-1), np.uint8)
    torch.cuda.synchronize()
    p = lambda t: t.data_ptr()  # noqa: E731
    dup = lambda: dd.duplex_consensus_device(p(d_b1), p(d_q1), p(d_off), n * L, p(d_b2), p(d_q2), p(d_off), n * L, p(d_c), p(d_k),  # noqa: E731
                                             p(d_s), n, C, min_q=10, strand_cap_q=40, cap_q=93)
    cons = lambda: dd.consensus_device(p(d_b1), p(d_q1), p(d_off), n * L, p(d_c), p(d_k), n, C, min_q=10, cap_q=93)  # noqa: E731
    sm = dup()
    members = int((cid != 0).sum())
    votes_bytes = 2 * members * L + 2 * C * L                    # every member's record in its layer, and the representatives'
    read_plain = votes_bytes + (n + 1) * 8 + n * 5
    read_duplex = votes_bytes + 2 * (n + 1) * 8 + n * 6
    written = 2 * sm["total_bytes"]
    line = dict(what="%d metric words as clusters, 2 x %d nt reads, p_sub %g, half of the members on the other strand" % (n, L, a.p_sub),
                reads=n, members=members, other_strand=int(len(other)), bytes_read_duplex=read_duplex, bytes_read_consensus=read_plain,
                bytes_written=written, **sm)
    ok = None
    if a.sample:
        res = dd._consensus_result(sm)
        extra = {k: np.zeros(C, np.uint32) for k in ("depth_same", "depth_other", "disagree")}
        dd._check(dd._lib.humid_get_duplex_consensus(dd._h, *[extra[k].ctypes.data for k in ("depth_same", "depth_other", "disagree")], None))
        depth = np.bincount(cid, minlength=C + 1)[1:]
        pick = np.unique(np.r_[np.argsort(depth)[-20:] + 1, rng.choice(np.arange(1, C + 1), min(a.sample, C), replace=False)])
        new_id = np.zeros(C + 1, np.int64)
        new_id[pick] = np.arange(1, len(pick) + 1)
        rows = np.flatnonzero(new_id[cid] != 0)
        off = np.arange(len(rows) + 1, dtype=np.uint64) * np.uint64(L)
        t = dt.duplex_numpy((b1[rows].reshape(-1), q1[rows].reshape(-1), off), (b2[rows].reshape(-1), q2[rows].reshape(-1), off),
                            new_id[cid[rows]], keep[rows], strand[rows], len(pick))
        ooff = res["out_off"].astype(np.int64)
        at = (ooff[pick - 1][:, None] + np.arange(L)[None, :]).reshape(-1)
        ok = bool(np.all(np.diff(ooff) == L) and np.array_equal(res["bases"][at], t["bases"]) and np.array_equal(res["quals"][at], t["quals"])
                  and np.array_equal(res["depth"][pick - 1], t["depth"]) and np.array_equal(res["errors"][pick - 1], t["errors"])
                  and all(np.array_equal(extra[k][pick - 1], t[k]) for k in extra))
        line.update(verified=ok, verified_clusters=int(len(pick)), largest_cluster=int(depth.max()))
        del res, t
    td, tc = [], []
    for _ in range(a.warmup):
        cons()
        dup()
    for _ in range(a.passes):
        tc.append(timed_ms(cons))
        td.append(timed_ms(dup))
    sd, sc = stats(td), stats(tc)
    line.update(t_duplex_device=sd, t_consensus_device=sc, duplex_over_consensus=round(sd["median_ms"] / sc["median_ms"], 3),
                hbm_share_duplex=round((read_duplex + written) / HBM_BYTES_PER_MS / sd["median_ms"], 4),
                hbm_share_consensus=round((read_plain + written) / HBM_BYTES_PER_MS / sc["median_ms"], 4))
    print(json.dumps(line), flush=True)
    dd.close()
    return 0 if ok in (None, True) else 1


if __name__ == "__main__":
    sys.exit(main())
