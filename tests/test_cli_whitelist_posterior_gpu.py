"""-m gpu: `humid -b K -w FILE --barcode-posterior` end to end.  A barcode with several listed barcodes one
substitution away is decided by the qualities of its bases (the first K letters of the quality line) and by how often
each candidate occurs exactly in the input.  Expected words come from the oracle's word extraction
(cli_util.expected_words), split at K; expected keys, statuses and counters from tests/whitelist_posterior_truth.py on
the quality bytes of the file; expected cluster ids and keep flags from the per-group truth (tests/grouped_truth.py) on
the corrected keys; the expected files are written from those."""
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, expected_words
from test_cli_keyed_gpu import check_outputs, split_words
from test_cli_whitelist_gpu import group_lines, letters

import grouped_truth as gt
import whitelist_posterior_truth as pt
import whitelist_truth as wt

pytestmark = pytest.mark.gpu

K = 16
U64 = np.uint64


def posterior_fastq(tmp, n_reads, seed, flat=False, n_cells=30, n_umis=40, umi=12, tail=20, p_sub=0.02, p_n=0.004):
    """One file, read = cell barcode (16 nt) + UMI + cDNA.  The barcodes: listed ones, one and two substitutions,
    random ones, and every tenth read the midpoint of a listed pair at distance 2 (two candidates).
    flat=False: a quality per base from '#' to 'I', so that some midpoints are decided and some are not.
    flat=True: every quality 'I' and no exact read of the barcodes the midpoints lie between: every planted midpoint
    is an exact tie.  Returns (files, whitelist file, whitelist, indices of the planted reads)."""
    rng = np.random.default_rng(seed)
    wl = wt.whitelist_with_neighbours(rng, n_cells, K)
    m = min(n_cells // 4, 40)
    drawn = wl[2 * m:-2] if flat else wl                             # (wl[:2 m] hold the pairs, wl[-2:] a pair at distance 1)
    keys = drawn[rng.integers(0, len(drawn), size=n_reads)]
    u = rng.random(n_reads)
    one, two, rnd = np.flatnonzero(u < 0.14), np.flatnonzero((u >= 0.10) & (u < 0.14)), np.flatnonzero((u >= 0.14) & (u < 0.18))
    keys[one] = wt.substitute(rng, keys[one], K)
    keys[two] = wt.substitute(rng, keys[two], K)
    keys[rnd] = wt.random_barcodes(rng, len(rnd), K)
    mids = wt.midpoints(wl[:2 * m], K)
    assert len(mids)
    planted = np.sort(rng.choice(n_reads, size=n_reads // 10, replace=False))
    keys[planted] = mids[rng.integers(0, len(mids), size=len(planted))]
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
            if i % 500 == 7:
                seq = seq[:9]                                       # shorter than the barcode: filtered, its row never read
            qual = "I" * len(seq) if flat else "".join(chr(x) for x in rng.integers(35, 74, size=len(seq)))
            fh.write("@r%d\n%s\n+\n%s\n" % (i, seq, qual))
    wl_path = str(tmp / "wl.txt")
    with open(wl_path, "w") as fh:
        for v in wl:
            fh.write(letters(v) + "\n")
    return [path], wl_path, wl, planted


def truth_for(files, wl, word_nt, d, min_odds=39, maximum=False):
    words, filt, recs, _ = expected_words(files, word_nt)
    keys, rest = split_words(words, word_nt, K)
    quals = np.asarray([[ord(c) for c in (r[3][:K] + "!" * K)[:K]] for r in recs[0][:len(filt)]], np.uint8)
    key_out, status, sm, _ = pt.posterior(keys, quals, filt, wl, K, min_odds)
    filt2 = ((filt != 0) | (status >= 3)).astype(np.uint8)
    Ks, inv = np.unique(key_out[filt2 == 0], return_inverse=True)
    groups = np.full(len(filt), 0xFFFFFFFF, np.uint32)
    groups[filt2 == 0] = inv.astype(np.uint32)
    t = gt.per_group(rest, groups, filt2, word_nt - K, d, int(maximum))
    return t, recs, Ks, sm, status


def barcodes_dat(sm):
    return "exact: %d\ncorrected: %d\nambiguous: %d\nunmatched: %d\n" % tuple(sm["counts"][1:]) + \
        "multi: %d\nrescued: %d\n" % (sm["multi"], sm["rescued"])


def check_all(out, files, t, recs, Ks, sm, wl):
    check_outputs(out, files, t, recs)                              # _dedup, _annotated, the three histograms, stats.dat
    got = open(os.path.join(out, "groups.dat")).read().split("\n")
    assert got[-1] == "" and got[:-1] == group_lines(t, Ks)
    assert set(l.split()[0] for l in got[:-1]) <= set(letters(v) for v in wl)
    assert open(os.path.join(out, "barcodes.dat")).read() == barcodes_dat(sm)


@pytest.mark.parametrize("flags", [[], ["-x"]])
def test_posterior_barcodes(flags, tmp_path):
    files, wl_path, wl, _ = posterior_fastq(tmp_path, 3000, 71)
    out, log = str(tmp_path / "out"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-w", wl_path, "--barcode-posterior", "-d", out, "-l", log, "-s", "-a"]
                          + flags + files, timeout=300)
    t, recs, Ks, sm, status = truth_for(files, wl, 28, 1, maximum="-x" in flags)
    assert all(c > 0 for c in sm["counts"]) and 0 < sm["rescued"] < sm["multi"] and t["summary"]["edges"] > 0
    check_all(out, files, t, recs, Ks, sm, wl)
    text = open(log).read()
    assert "  barcodes: %d exact, %d corrected, %d ambiguous, %d unmatched\n" % tuple(sm["counts"][1:]) in text
    assert "  barcode posterior: %d reads with several candidates, %d of them corrected (odds >= 39)\n" % (sm["multi"], sm["rescued"]) \
        in text
    if not flags:
        # without the flag the same reads are ambiguous: fewer corrected reads, and barcodes.dat keeps its four lines
        plain = str(tmp_path / "plain")
        subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-w", wl_path, "-d", plain, "-l", "/dev/null", "-s", "-q"] + files,
                              timeout=300)
        c = sm["counts"]
        assert open(os.path.join(plain, "barcodes.dat")).read() == \
            "exact: %d\ncorrected: %d\nambiguous: %d\nunmatched: %d\n" % (c[1], c[2] - sm["rescued"], c[3] + sm["rescued"], c[4])


def test_min_odds_1_changes_exactly_the_tied_reads(tmp_path):
    files, wl_path, wl, planted = posterior_fastq(tmp_path, 3000, 73, flat=True)
    truths = {}
    for min_odds in (39, 1):
        out = str(tmp_path / ("odds%d" % min_odds))
        subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-w", wl_path, "--barcode-posterior", "--barcode-min-odds",
                               str(min_odds), "-d", out, "-l", "/dev/null", "-s", "-a"] + files, timeout=300)
        truths[min_odds] = truth_for(files, wl, 28, 1, min_odds=min_odds)
        t, recs, Ks, sm, status = truths[min_odds]
        check_all(out, files, t, recs, Ks, sm, wl)
    s39, s1 = truths[39][4], truths[1][4]
    changed = np.flatnonzero(s39 != s1)
    usable_planted = planted[s39[planted] != pt.FILTERED]
    assert len(changed) > 100 and np.array_equal(changed, usable_planted)
    assert np.all(s39[changed] == pt.AMBIGUOUS) and np.all(s1[changed] == pt.CORRECTED)
    assert truths[39][3]["rescued"] == 0 and truths[1][3]["rescued"] == truths[1][3]["multi"] == len(changed)
