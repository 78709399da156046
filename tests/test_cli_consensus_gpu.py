"""-m gpu: `humid -C -s -a` end to end, file by file.  Every kept record carries the consensus of its cluster's reads on
its sequence and quality lines.  Expected words come from the oracle's word extraction (cli_util.expected_words),
cluster ids and keep flags from the oracle run (tests/grouped_truth.py), with -Q the survivors from
tests/best_truth.py, and the consensus from tests/consensus_truth.py over a Python parse of every file; the
_annotated files and every .dat file are those of the same run without -C, byte for byte."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, expected_words, read_fastq
from humid_amd.synth import synth_fastq
from test_cli_best_gpu import best_keep, same_side_files
from test_cli_keyed_gpu import check_outputs
from test_cli_whitelist_gpu import check_all, truth_for as whitelist_truth_for, whitelisted_fastq

import best_truth as bt
import consensus_truth as ct
import grouped_truth as gt

pytestmark = pytest.mark.gpu


def expected(files, recs, cid, keep, n_clusters, min_q=10):
    """per file the _dedup records the truth asks for, and the log line's four numbers"""
    n = len(cid)
    want, changed, errors, multi = [], 0, 0, 0
    for r in recs:
        b, q, off = ct.flat([r[i][1].encode() for i in range(n)], [r[i][3].encode() for i in range(n)])
        t = ct.consensus_numpy(b, q, off, cid, keep, n_clusters, min_q, 93)
        if n <= 3000:
            ct.assert_same(t, ct.consensus_loop(b, q, off, np.asarray(cid), np.asarray(keep), n_clusters, min_q, 93))
        oo, tb, tq = t["out_off"].astype(np.int64), bytes(t["bases"]), bytes(t["quals"])
        out = []
        for i in np.flatnonzero(keep):
            c = int(cid[i])
            out.append((r[i][0], tb[oo[c - 1]:oo[c]].decode("latin-1"), r[i][2], tq[oo[c - 1]:oo[c]].decode("latin-1")))
            assert len(out[-1][1]) == len(r[i][1])
        want.append(out)
        changed += t["summary"]["bases_changed"]
        errors += t["summary"]["errors"]
        multi = t["summary"]["multi_read"]
    line = "  consensus: %d clusters, %d multi-read, %d bases changed, %d disagreeing votes\n" % (n_clusters, multi, changed, errors)
    return want, line, changed


def dedup_of(out, files, gz=False):
    ext = ".fastq.gz" if gz else ".fastq"
    return [read_fastq(os.path.join(out, os.path.basename(f).replace(ext, "_dedup" + ext))) for f in files]


@pytest.mark.parametrize("n_files,flags", [(1, []), (2, []), (1, ["-Q"]), (2, ["-Q", "--consensus-min-q", "20"])])
def test_plain_input(n_files, flags, tmp_path):
    files = synth_fastq(str(tmp_path / "in"), 3000, 17, n_files=n_files, umi_len=8, p_sub=2e-2, p_n=5e-3, read_len=40,
                        short_frac=0.02)
    scores = bt.rewrite_qualities(files, 17)
    words, filt, recs, _ = expected_words(files, 24)
    t = gt.per_group(words, np.zeros(len(filt), np.uint32), filt, 24, 1, 0)
    keep = best_keep(t, words, scores)[0] if "-Q" in flags else t["keep"]
    want, line, changed = expected(files, recs, t["cid"], keep, t["summary"]["clusters"], 20 if "20" in flags else 10)
    assert changed > 20
    out, plain, log = str(tmp_path / "out"), str(tmp_path / "plain"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-C", "-d", out, "-l", log, "-s", "-a"] + flags + files, timeout=300)
    subprocess.check_call([HUMID, "-d", plain, "-l", "/dev/null", "-s", "-a"] + [f for f in flags if f == "-Q"] + files,
                          timeout=300)
    tq = dict(t)
    tq["keep"] = keep
    check_outputs(plain, files, tq, recs)
    assert dedup_of(out, files) == want
    same_side_files(out, plain, files)
    assert line in open(log).read()


def test_gz_in_and_out_and_the_batch_loop(tmp_path):
    """gzip inputs inflated in memory, gzip members out; plain files through the batch loop instead of the mapping"""
    files = synth_fastq(str(tmp_path / "in"), 3000, 19, n_files=2, umi_len=8, p_sub=2e-2, read_len=40)
    bt.rewrite_qualities(files, 19)
    words, filt, recs, _ = expected_words(files, 24)
    t = gt.per_group(words, np.zeros(len(filt), np.uint32), filt, 24, 1, 0)
    want, line, _ = expected(files, recs, t["cid"], t["keep"], t["summary"]["clusters"])
    gz = []
    for f in files:
        gz.append(f + ".gz")
        with gzip.open(gz[-1], "wb") as fh:
            fh.write(open(f, "rb").read())
    out, plain, log = str(tmp_path / "out"), str(tmp_path / "plain"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-C", "-d", out, "-l", log, "-s", "-a"] + gz, timeout=300)
    subprocess.check_call([HUMID, "-d", plain, "-l", "/dev/null", "-s", "-a"] + gz, timeout=300)
    assert dedup_of(out, gz, gz=True) == want and line in open(log).read()
    names = sorted(os.listdir(plain))
    assert sorted(os.listdir(out)) == names
    for n in names:                                                     # (gzip members: compare what they hold)
        if "_annotated" in n:
            assert read_fastq(os.path.join(out, n)) == read_fastq(os.path.join(plain, n)), n
        elif n.endswith(".dat"):
            assert open(os.path.join(out, n), "rb").read() == open(os.path.join(plain, n), "rb").read(), n
    out2 = str(tmp_path / "out2")
    subprocess.check_call([HUMID, "-C", "-d", out2, "-l", "/dev/null"] + files, env=dict(os.environ, HUMID_NO_MAPPED_WRITE="1"),
                          timeout=300)
    assert dedup_of(out2, files) == want


def test_with_barcodes_and_a_whitelist(tmp_path):
    files, wl_path, wl = whitelisted_fastq(tmp_path, 4000, 61)
    bt.rewrite_qualities(files, 61)
    t, recs, Ks, counts = whitelist_truth_for(files, wl, 28, 1)
    _, filt, _, _ = expected_words(files, 28)
    assert np.any((t["cid"] == 0) & (filt == 0))                        # unmatched reads are no members
    want, line, changed = expected(files, recs, t["cid"], t["keep"], t["summary"]["clusters"])
    assert changed > 0
    out, plain, log = str(tmp_path / "out"), str(tmp_path / "plain"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-C", "-n", "28", "-b", "16", "-w", wl_path, "-d", out, "-l", log, "-s", "-a"] + files,
                          timeout=300)
    subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-w", wl_path, "-d", plain, "-l", "/dev/null", "-s", "-a"] + files,
                          timeout=300)
    check_all(plain, files, t, recs, Ks, counts, wl)
    assert dedup_of(out, files) == want
    same_side_files(out, plain, files)
    assert line in open(log).read()
