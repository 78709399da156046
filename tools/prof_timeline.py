#!/usr/bin/env python3
"""Timeline of ONE pass from a rocprofv3 --kernel-trace run (its *_kernel_trace.csv), as a markdown table laid out
like profiles/r03l_exchange_world1_timeline.md: start and duration of every kernel on the GPU's clock, and a `>> idle`
line for every stretch of more than IDLE_US in which the GPU ran nothing.

usage: prof_timeline.py KERNEL_TRACE_CSV [IDLE_US = 4] [FIRST_KERNEL = k_p8_scatter1<Reads8]

A pass is taken to start with the k_zero_many in front of FIRST_KERNEL; the second-last pass of the trace is printed
(the last one has no successor to end it)."""
import csv
import sys


def main():
    path = sys.argv[1]
    idle_us = float(sys.argv[2]) if len(sys.argv) > 2 else 4.0
    first = sys.argv[3] if len(sys.argv) > 3 else "k_p8_scatter1<Reads8"
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if first in r[2]]
    if len(starts) < 3:
        sys.exit("fewer than three passes in the trace")
    # (the zeroing launch in front of the pass's first scatter belongs to the pass)
    def begin(i):
        return i - 1 if i > 0 and "k_zero_many" in rows[i - 1][2] else i
    a, b = begin(starts[-2]), begin(starts[-1])
    one = rows[a:b]
    t0 = one[0][0]
    print("| start | us | kernel |\n|---:|---:|---|")
    busy = idle = 0.0
    n_idle = 0
    prev_end = t0
    for s, e, name in one:
        gap = (s - prev_end) / 1e3
        if gap > idle_us:
            print("| %.1f | %.1f | >> idle |" % ((prev_end - t0) / 1e3, gap))
            idle += gap
            n_idle += 1
        print("| %.1f | %.1f | `%s` |" % ((s - t0) / 1e3, (e - s) / 1e3, name[:72].replace("|", "/")))
        busy += (e - s) / 1e3
        prev_end = max(prev_end, e)
    print("\nkernels %.0f us in %d launches, %d idle stretches (> %g us) %.0f us, first kernel to last %.0f us"
          % (busy, len(one), n_idle, idle_us, idle, (prev_end - t0) / 1e3))


if __name__ == "__main__":
    main()
