"""-m gpu: `humid -w A -w B -w C --word-pattern P` end to end on a small SPLiT-seq-shaped FastQ pair: the barcode read
holds the UMI (10 nt), then three 8-nt segments with 12-nt linkers between them.  Expected words come from the Python
restatement of the pattern (test_cli_segments_host.pattern_words), expected keys, statuses and summaries from
tests/segments_truth.py, expected cluster ids and keep flags from the per-group truth on the corrected keys and from the
Python API; the same data with the linkers cut out and a contiguous -b 24 gives identical outputs."""
import os
import subprocess

import numpy as np
import pytest

import humid_amd
from cli_util import HUMID, read_fastq
from test_cli_keyed_gpu import check_outputs, split_words
from test_cli_segments_host import SPLIT, pattern_words

import grouped_truth as gt
import segments_truth as sg

pytestmark = pytest.mark.gpu

SEG_NT = [8, 8, 8]
K, N_WORD = 24, 44                                                  # word: barcode 24, UMI 10, 10 nt of the cDNA read


def letters(v, k):
    return "".join("ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def splitseq_files(tmp, n_reads, seed, n_umis=30):
    rng = np.random.default_rng(seed)
    lists = sg.make_lists(rng, [12, 10, 14], SEG_NT)
    keys, _ = sg.make_keys(rng, lists, SEG_NT, n_reads, p_high=0.0, p_filt=0.0)
    segs = [[letters((int(k) >> sh) & 0xFFFF, 8) for k in keys] for sh in sg.shifts(SEG_NT)]
    umis = ["".join("ACGT"[x] for x in rng.integers(0, 4, size=10)) for _ in range(n_umis)]
    cdna = ["".join("ACGT"[x] for x in rng.integers(0, 4, size=30)) for _ in range(8)]
    l1, l2 = "GTGGCCGATGTT", "ATCCACGTGCTT"
    bc, rd, cut = str(tmp / "bc.fastq"), str(tmp / "cdna.fastq"), str(tmp / "cut.fastq")
    with open(bc, "w") as fb, open(rd, "w") as fr, open(cut, "w") as fc:
        for i in range(n_reads):
            u, c = umis[rng.integers(0, n_umis)], cdna[rng.integers(0, 8)]
            if rng.random() < 0.02:
                u = u[:3] + "N" + u[4:]
            read = u + segs[0][i] + l1 + segs[1][i] + l2 + segs[2][i]
            if rng.random() < 0.02:
                read = read[:int(rng.integers(20, 57))]                # shorter than the pattern
            # the same letters with the linkers cut out, barcode first, in ONE file: -b 24 takes them as they stand
            flat = "".join(read[p] if p < len(read) else "N" for p in [j for j, ch in enumerate(SPLIT) if ch == "C"] +
                           [j for j, ch in enumerate(SPLIT) if ch == "N"]) + c[:10]
            fb.write("@r%d\n%s\n+\n%s\n" % (i, read, "I" * len(read)))
            fr.write("@r%d\n%s\n+\n%s\n" % (i, c, "I" * len(c)))
            fc.write("@r%d\n%s\n+\n%s\n" % (i, flat, "I" * len(flat)))
    wl = []
    for j, w in enumerate(lists):
        wl.append(str(tmp / ("seg%d.txt" % j)))
        with open(wl[-1], "w") as fh:
            fh.write("# segment %d\n" % j + "".join(letters(v, 8) + "\n" for v in w) + letters(w[0], 8).lower() + "\r\n")
    return [bc, rd], cut, wl, lists


def outputs(out, names=("barcodes.dat", "groups.dat", "stats.dat", "counts.dat", "neigh.dat", "clusters.dat")):
    return {n: open(os.path.join(out, n)).read() for n in names}


@pytest.mark.parametrize("mi", [None, 1])
def test_splitseq_pair(mi, tmp_path):
    files, cut, wl, lists = splitseq_files(tmp_path, 4000, 71)
    flags = ["-w", wl[0], "-w", wl[1], "-w", wl[2]] + (["--barcode-max-inexact", str(mi)] if mi is not None else [])
    out, log = str(tmp_path / "out"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-n", str(N_WORD), "--word-pattern", SPLIT, "-d", out, "-l", log, "-s", "-a"] + flags + files, timeout=300)
    words, filt = pattern_words(files, SPLIT, N_WORD)
    keys, rest = split_words(words, N_WORD, K)
    t_key, t_status, t_counts, t_seg, t_hist = sg.correct(keys, filt, lists, SEG_NT, mi)
    sg.assert_covers(sg.correct(keys, filt, lists, SEG_NT))
    filt2 = ((filt != 0) | (t_status >= 3)).astype(np.uint8)
    Ks, inv = np.unique(t_key[filt2 == 0], return_inverse=True)
    groups = np.full(len(filt), 0xFFFFFFFF, np.uint32)
    groups[filt2 == 0] = inv.astype(np.uint32)
    t = gt.per_group(rest, groups, filt2, N_WORD - K, 1, 0)
    check_outputs(out, files, t, [read_fastq(f) for f in files])    # _dedup, _annotated, the three histograms, stats.dat
    # ... and the Python API on the same words gives the same ids
    dd = humid_amd.Dedup()
    try:
        dd.set_whitelist_segments(lists, SEG_NT, mi)
        cid, keep, _ = dd.run_keyed(rest, keys, filt, word_nt=N_WORD - K, correct=True)
        assert np.array_equal(cid, t["cid"]) and np.array_equal(keep, t["keep"])
        st = dd.group_stats()
        sc, ih = dd.barcode_segments()
        assert np.array_equal(sc, t_seg) and np.array_equal(ih, t_hist) and np.array_equal(st["key"], Ks)
    finally:
        dd.close()
    got = outputs(out)
    assert got["groups.dat"] == "".join("%s %d %d %d\n" % (letters(k, K), r, u, c) for k, r, u, c in
                                        zip(st["key"], st["reads"], st["unique"], st["clusters"]))
    want = "exact: %d\ncorrected: %d\nambiguous: %d\nunmatched: %d\n" % tuple(int(c) for c in t_counts[1:])
    for s in range(3):
        want += "".join("segment%d.%s: %d\n" % (s, name, int(t_seg[s][j]))
                        for j, name in enumerate(("exact", "corrected", "ambiguous", "unmatched")))
    want += "".join("inexact%d: %d\n" % (m, int(t_hist[m])) for m in range(4))
    assert got["barcodes.dat"] == want
    text = open(log).read()
    assert "  barcodes: %d exact, %d corrected, %d ambiguous, %d unmatched\n" % tuple(int(c) for c in t_counts[1:]) in text
    assert text.count("  barcode segments (exact/corrected/ambiguous/unmatched): ") == 1
    # the linkers cut out, the barcode contiguous: the same statistics, the same records kept, the same ids
    out2 = str(tmp_path / "out2")
    subprocess.check_call([HUMID, "-n", str(N_WORD), "-b", str(K), "-d", out2, "-l", "/dev/null", "-s", "-a"] + flags + [cut], timeout=300)
    assert outputs(out2) == got
    names = lambda p: [r[0] for r in read_fastq(p)]                 # noqa: E731
    for kind in ("dedup", "annotated"):
        assert names(os.path.join(out2, "cut_%s.fastq" % kind)) == names(os.path.join(out, "bc_%s.fastq" % kind))


def test_one_list_is_the_plain_path(tmp_path):
    """one -w, with and without a pattern: the four lines of barcodes.dat and no segment line anywhere"""
    files, cut, wl, lists = splitseq_files(tmp_path, 1500, 73)
    product = str(tmp_path / "product.txt")
    open(product, "w").write("".join(letters(v, K) + "\n" for v in sg.product_list(lists, SEG_NT)))
    res = {}
    for name, args in (("pattern", ["--word-pattern", SPLIT] + files), ("cut", ["-b", str(K), cut])):
        out, log = str(tmp_path / name), str(tmp_path / (name + ".log"))
        subprocess.check_call([HUMID, "-n", str(N_WORD), "-w", product, "-d", out, "-l", log, "-s", "-q"] + args, timeout=300)
        res[name] = outputs(out)
        assert "segment" not in res[name]["barcodes.dat"] + open(log).read()
        assert len(res[name]["barcodes.dat"].strip().split("\n")) == 4
    assert res["pattern"] == res["cut"]
    # ... which is what the three lists with one inexact segment at the most give
    out = str(tmp_path / "seg")
    subprocess.check_call([HUMID, "-n", str(N_WORD), "-b", str(K), "-w", wl[0], "-w", wl[1], "-w", wl[2], "--barcode-max-inexact", "1",
                           "-d", out, "-l", "/dev/null", "-s", "-q", cut], timeout=300)
    seg = outputs(out)
    assert seg["barcodes.dat"].startswith(res["cut"]["barcodes.dat"])
    assert {k: v for k, v in seg.items() if k != "barcodes.dat"} == {k: v for k, v in res["cut"].items() if k != "barcodes.dat"}
