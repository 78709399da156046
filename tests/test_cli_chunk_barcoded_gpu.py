"""-m gpu: `humid --chunk-barcoded N` (a run with a barcode whose device part runs over chunks: the barcode counter, the
posterior's prior, the corrected chunks into a keyed accumulator) writes the files of the run without the flag, byte for
byte -- _dedup, _annotated, stats.dat, the three histograms, groups.dat, barcodes.dat, cells.dat, barcode_rank.dat -- and
the same log apart from its times."""
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID
from test_cli_segments_gpu import N_WORD, splitseq_files
from test_cli_segments_host import SPLIT

import whitelist_truth as wt

pytestmark = pytest.mark.gpu

K = 8


def letters(v, k=K):
    return "".join("ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def barcoded_fastq(tmp, n_reads, seed, n_cells=30, n_umis=40, umi=12, tail=16, p_sub=0.02, p_n=0.004):
    """one file as test_cli_whitelist_gpu.whitelisted_fastq writes it, with a barcode of 8 letters: read = cell barcode +
    UMI + cDNA, few cells of skewed sizes, few UMIs, substitutions in both; barcodes one and two substitutions off,
    random ones and midpoints of whitelist pairs; the barcode's qualities vary (--barcode-posterior reads them); and the
    whitelist file"""
    rng = np.random.default_rng(seed)
    os.makedirs(str(tmp), exist_ok=True)
    wl = wt.whitelist_with_neighbours(rng, n_cells, K)
    keys, _ = wt.make_keys(rng, wl, K, n_reads, p1=0.1, p2=0.04, pr=0.04, p_filt=0.0)
    heavy = rng.random(n_reads) < 0.5                                # half of the reads in the first few cells: a skew for --cells-*
    keys[heavy] = np.asarray(wl)[np.minimum(rng.geometric(0.3, size=int(heavy.sum())) - 1, n_cells - 1)]
    cells = np.asarray([[(int(v) >> (2 * (K - 1 - i))) & 3 for i in range(K)] for v in keys])
    umis = rng.integers(0, 4, size=(n_umis, umi))
    rest = np.concatenate([umis[rng.integers(0, n_umis, size=n_reads)], rng.integers(0, 4, size=(n_reads, tail))], 1)
    rest = np.where(rng.random(rest.shape) < p_sub, rng.integers(0, 4, size=rest.shape), rest)
    rows = np.concatenate([cells, rest], 1)
    rows = np.where(rng.random(rows.shape) < p_n, 4, rows)
    quals = rng.choice(np.asarray(list("#-:F")), size=rows.shape)    # Phred 2, 12, 25, 37
    path = str(tmp / "cells.fastq")
    with open(path, "w") as fh:
        for i, r in enumerate(rows):
            fh.write("@r%d\n%s\n+\n%s\n" % (i, "".join("ACGTN"[x] for x in r), "".join(quals[i])))
    wl_path = str(tmp / "wl.txt")
    with open(wl_path, "w") as fh:
        fh.write("".join(letters(v) + "\n" for v in wl))
    return [path], wl_path


def run(files, out, flags, log):
    subprocess.check_call([HUMID, "-d", out, "-l", log] + flags + files, timeout=300)
    return {fn: open(os.path.join(out, fn), "rb").read() for fn in sorted(os.listdir(out))}


def same_files(tmp_path, files, flags, chunkings, expect):
    os.makedirs(str(tmp_path), exist_ok=True)
    ref = run(files, str(tmp_path / "ref"), flags, str(tmp_path / "ref.log"))
    assert set(expect) <= set(ref), sorted(ref)
    strip = lambda t: [l.split("...")[0] for l in t.split("\n")]       # noqa: E731  (the lines without their times)
    ref_log = open(tmp_path / "ref.log").read()
    for c in chunkings:
        got = run(files, str(tmp_path / ("c%d" % c)), flags + ["--chunk-barcoded", str(c)], str(tmp_path / ("c%d.log" % c)))
        assert sorted(got) == sorted(ref)
        for fn in ref:
            assert got[fn] == ref[fn], (c, fn)
        assert strip(open(tmp_path / ("c%d.log" % c)).read()) == strip(ref_log)
    return ref, ref_log


@pytest.fixture(scope="module")
def fastq(tmp_path_factory):
    return barcoded_fastq(tmp_path_factory.mktemp("chunk_barcoded_in"), 3000, 131)


BASE = ["-n", "20", "-b", "8", "-s", "-a"]
STATS = ["stats.dat", "counts.dat", "neigh.dat", "clusters.dat", "groups.dat", "cells_dedup.fastq", "cells_annotated.fastq"]


@pytest.mark.parametrize("more,expect,in_log", [
    ([], [], []),
    (["-w", "WL"], ["barcodes.dat"], ["  barcodes: "]),
    (["-w", "WL", "--barcode-posterior"], ["barcodes.dat"], ["  barcode posterior: "]),
    (["--cells-top", "20", "--cells-merge-ratio", "3"], ["barcodes.dat", "cells.dat", "barcode_rank.dat"], ["  cells: "]),
    (["--cells-expected", "30", "--barcode-posterior"], ["barcodes.dat", "cells.dat", "barcode_rank.dat"], ["  cells: ", "  barcode posterior: "]),
    (["-w", "WL", "-e", "-m", "2"], ["barcodes.dat"], ["Levenshtein"]),
    (["-w", "WL", "-x", "-q"], ["barcodes.dat"], []),
], ids=["barcode_alone", "whitelist", "whitelist_posterior", "cells_top_merge", "cells_expected_posterior", "edit_distance_2",
        "maximum_no_dedup_file"])
def test_chunked_run_writes_the_same_files(fastq, more, expect, in_log, tmp_path):
    files, wl = fastq
    more = [wl if x == "WL" else x for x in more]
    want = [f for f in STATS if not ("-q" in more and f == "cells_dedup.fastq")] + expect
    ref, log = same_files(tmp_path, files, BASE + more, [700], want)
    for text in in_log:
        assert text in log, log
    if "barcodes.dat" in ref:
        counts = dict(l.split(": ") for l in ref["barcodes.dat"].decode().strip().split("\n"))
        assert int(counts["corrected"]) > 0 and int(counts["exact"]) > int(counts["corrected"])
        if "--barcode-posterior" in more:
            assert int(counts["multi"]) > 0
    assert len(ref["groups.dat"].decode().strip().split("\n")) >= 10


def test_segmented_word_pattern(tmp_path):
    files, _, wl, _ = splitseq_files(tmp_path, 3000, 71)
    flags = ["-n", str(N_WORD), "--word-pattern", SPLIT, "-s", "-a", "-w", wl[0], "-w", wl[1], "-w", wl[2], "--barcode-max-inexact", "1"]
    ref, log = same_files(tmp_path / "runs", files, flags, [700], ["barcodes.dat", "groups.dat", "stats.dat"])
    assert "  barcode segments (exact/corrected/ambiguous/unmatched):" in log
    counts = dict(l.split(": ") for l in ref["barcodes.dat"].decode().strip().split("\n"))
    assert sum(int(counts["segment%d.corrected" % g]) for g in range(3)) > 0 and int(counts["inexact1"]) > 0


def test_one_chunk_and_chunks_of_one_record(tmp_path):
    files, wl = barcoded_fastq(tmp_path / "in", 200, 137, n_cells=12)
    same_files(tmp_path / "a", files, BASE + ["-w", wl, "--barcode-posterior"], [1000000, 1], ["barcodes.dat", "groups.dat"])
    same_files(tmp_path / "b", files, BASE + ["--cells-min-reads", "3", "--cells-merge-ratio", "2"], [1000000, 1], ["cells.dat", "barcode_rank.dat"])


def test_no_cell_is_the_same_error(fastq, tmp_path):
    files, _ = fastq
    r = subprocess.run([HUMID, "-n", "20", "-b", "8", "-d", str(tmp_path / "out"), "-l", str(tmp_path / "log.txt"), "--cells-min-reads", "100000",
                        "--chunk-barcoded", "700"] + files, capture_output=True, timeout=300)
    assert r.returncode == 1 and b"no cell barcode was found" in r.stderr
    assert "  cells: 0 of " in open(tmp_path / "log.txt").read()
