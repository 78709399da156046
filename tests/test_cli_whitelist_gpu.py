"""-m gpu: `humid -b K -w FILE` end to end.  The barcode (the first K nucleotides of the word) is corrected against
the whitelist; reads whose barcode is ambiguous or unmatched are left out like reads the word filter excluded.
Expected words come from the oracle's word extraction (cli_util.expected_words), split at K; expected keys, statuses
and counts from tests/whitelist_truth.py; expected cluster ids and keep flags from the per-group truth
(tests/grouped_truth.py) on the corrected keys; the expected files are written from those."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, expected_words
from test_cli_keyed_gpu import check_outputs, split_words

import grouped_truth as gt
import whitelist_truth as wt

pytestmark = pytest.mark.gpu

K = 16


def letters(v, k=K):
    return "".join("ACGT"[(int(v) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def whitelisted_fastq(tmp, n_reads, seed, n_cells=30, n_umis=40, umi=12, tail=20, p_sub=0.02, p_n=0.004):
    """one file as test_cli_keyed_gpu.barcoded_fastq writes it -- read = cell barcode (16 nt) + UMI + cDNA, few cells,
    few UMIs, substitutions in both -- with the barcodes drawn by the generator of the whitelist tests (one and two
    substitutions, random barcodes, midpoints of whitelist pairs), and the whitelist file: 10x suffixes, lower case, a
    comment, an empty line, a CR, a duplicate"""
    rng = np.random.default_rng(seed)
    wl = wt.whitelist_with_neighbours(rng, n_cells, K)
    keys, _ = wt.make_keys(rng, wl, K, n_reads, p1=0.1, p2=0.04, pr=0.04, p_filt=0.0)
    cells = np.asarray([[(int(v) >> (2 * (K - 1 - i))) & 3 for i in range(K)] for v in keys])
    umis = rng.integers(0, 4, size=(n_umis, umi))
    rest = np.concatenate([umis[rng.integers(0, n_umis, size=n_reads)], rng.integers(0, 4, size=(n_reads, tail))], 1)
    rest = np.where(rng.random(rest.shape) < p_sub, rng.integers(0, 4, size=rest.shape), rest)
    rows = np.concatenate([cells, rest], 1)
    rows = np.where(rng.random(rows.shape) < p_n, 4, rows)
    path = str(tmp / "cells.fastq")
    with open(path, "w") as fh:
        for i, r in enumerate(rows):
            seq = "".join("ACGTN"[x] for x in r)
            fh.write("@r%d\n%s\n+\n%s\n" % (i, seq, "I" * len(seq)))
    wl_path = str(tmp / "wl.txt")
    with open(wl_path, "w") as fh:
        fh.write("# known barcodes\n\n")
        for j, v in enumerate(wl):
            s = letters(v)
            fh.write((s.lower() if j % 3 == 0 else s) + ("-1" if j % 2 else "") + ("\r\n" if j % 5 == 0 else "  \n"))
        fh.write(letters(wl[0]) + "\n")
    return [path], wl_path, wl


def truth_for(files, wl, word_nt, d, maximum=False, edit=False):
    words, filt, recs, _ = expected_words(files, word_nt)
    keys, rest = split_words(words, word_nt, K)
    key_out, status, counts = wt.correct(keys, filt, wl, K)
    filt2 = ((filt != 0) | (status >= 3)).astype(np.uint8)
    Ks, inv = np.unique(key_out[filt2 == 0], return_inverse=True)
    groups = np.full(len(filt), 0xFFFFFFFF, np.uint32)
    groups[filt2 == 0] = inv.astype(np.uint32)
    t = gt.per_group(rest, groups, filt2, word_nt - K, d, int(maximum), edit=edit)
    return t, recs, Ks, counts


def group_lines(t, Ks):
    """groups.dat of the truth: "<barcode> <reads> <unique> <clusters>" per barcode in ascending order"""
    lv = t["leaves"]
    out = []
    for g, key in enumerate(Ks):
        sel = np.asarray(lv["group"]) == g
        out.append("%s %d %d %d" % (letters(key), int(np.asarray(lv["count"])[sel].sum()), int(sel.sum()),
                                    len(np.unique(np.asarray(lv["cluster_id"])[sel]))))
    return out


def check_all(out, files, t, recs, Ks, counts, wl, gz=False):
    check_outputs(out, files, t, recs, gz=gz)                       # _dedup, _annotated, the three histograms, stats.dat
    got = open(os.path.join(out, "groups.dat")).read().split("\n")
    assert got[-1] == "" and got[:-1] == group_lines(t, Ks)
    assert set(l.split()[0] for l in got[:-1]) <= set(letters(v) for v in wl)
    assert open(os.path.join(out, "barcodes.dat")).read() == \
        "exact: %d\ncorrected: %d\nambiguous: %d\nunmatched: %d\n" % tuple(int(c) for c in counts[1:])


@pytest.mark.parametrize("flags,d", [([], 1), (["-x"], 1), (["-e", "-m", "2"], 2)])
def test_whitelisted_barcodes(flags, d, tmp_path):
    files, wl_path, wl = whitelisted_fastq(tmp_path, 4000, 61)
    out = str(tmp_path / "out")
    log = str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-w", wl_path, "-d", out, "-l", log, "-s", "-a"] + flags + files,
                          timeout=300)
    t, recs, Ks, counts = truth_for(files, wl, 28, d, maximum="-x" in flags, edit="-e" in flags)
    assert all(int(c) > 0 for c in counts) and (t["summary"]["edges"] > 0)
    check_all(out, files, t, recs, Ks, counts, wl)
    assert "  barcodes: %d exact, %d corrected, %d ambiguous, %d unmatched\n" % tuple(int(c) for c in counts[1:]) \
        in open(log).read()


def test_without_the_whitelist_there_are_more_groups(tmp_path):
    files, wl_path, wl = whitelisted_fastq(tmp_path, 4000, 63)
    n_lines = {}
    for name, flags in (("with", ["-w", wl_path]), ("without", [])):
        out = str(tmp_path / name)
        subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-d", out, "-l", "/dev/null", "-s", "-q"] + flags + files,
                              timeout=300)
        n_lines[name] = len(open(os.path.join(out, "groups.dat")).read().strip().split("\n"))
        assert os.path.exists(os.path.join(out, "barcodes.dat")) == (name == "with")
    assert n_lines["with"] <= len(np.unique(wl)) < n_lines["without"]


def test_gz_in_and_out(tmp_path):
    files, wl_path, wl = whitelisted_fastq(tmp_path, 3000, 65)
    gz = str(tmp_path / "cells.fastq.gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(open(files[0], "rb").read())
    t, recs, Ks, counts = truth_for(files, wl, 28, 1)
    for name, env in (("fast", {}), ("slow", {"HUMID_HOST_SLOW": "1"})):
        out = str(tmp_path / name)
        e = dict(os.environ)
        e.update(env)
        subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-w", wl_path, "-d", out, "-l", "/dev/null", "-s", "-a", gz],
                              env=e, timeout=300)
        check_all(out, [gz], t, recs, Ks, counts, wl, gz=True)
