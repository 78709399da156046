"""-m gpu: `humid -Q -s -a` end to end, file by file.  Every cluster keeps the record with the best base qualities
among the records of its most abundant word.  Expected words come from the oracle's word extraction
(cli_util.expected_words), cluster ids and keep flags from the oracle run (tests/grouped_truth.py), the scores from a
Python sum over the quality lines and the survivors from tests/best_truth.py; the _annotated files and every .dat file
are those of the same run without -Q, byte for byte."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, expected_words
from humid_amd.synth import synth_fastq
from test_cli_keyed_gpu import check_outputs
from test_cli_whitelist_gpu import check_all, truth_for as whitelist_truth_for, whitelisted_fastq

import best_truth as bt
import grouped_truth as gt

pytestmark = pytest.mark.gpu


def best_keep(t, words, scores):
    """the truth's keep flags after the selection (scope LEAF), both ways; returns (keep_out, n_changed)"""
    a = bt.select_sort(words, t["cid"], t["keep"], scores, bt.LEAF)
    bt.assert_same(a, bt.select_loop(words, t["cid"], t["keep"], scores, bt.LEAF))
    assert a[2] > 0 and int(a[0].sum()) == t["summary"]["clusters"]
    return a[0], a[2]


def same_side_files(with_q, without_q, files):
    names = sorted(os.listdir(without_q))
    assert sorted(os.listdir(with_q)) == names
    side = [n for n in names if n.endswith(".dat") or "_annotated" in n]
    assert len(side) >= 4 + len(files)
    for n in side:
        assert filecmp.cmp(os.path.join(with_q, n), os.path.join(without_q, n), shallow=False), n
    assert any(not filecmp.cmp(os.path.join(with_q, n), os.path.join(without_q, n), shallow=False)
               for n in names if "_dedup" in n)


@pytest.mark.parametrize("n_files,flags,d", [(1, [], 1), (2, [], 1), (1, ["-x", "-m", "2"], 2)])
def test_plain_input(n_files, flags, d, tmp_path):
    files = synth_fastq(str(tmp_path / "in"), 4000, 17, n_files=n_files, umi_len=8, p_sub=4e-3, p_n=2e-3, read_len=40,
                        short_frac=0.01)
    scores = bt.rewrite_qualities(files, 17)
    words, filt, recs, _ = expected_words(files, 24)
    t = gt.per_group(words, np.zeros(len(filt), np.uint32), filt, 24, d, int("-x" in flags))
    keep_out, n_changed = best_keep(t, words, scores)
    out, plain, log = str(tmp_path / "out"), str(tmp_path / "plain"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-Q", "-d", out, "-l", log, "-s", "-a"] + flags + files, timeout=300)
    subprocess.check_call([HUMID, "-d", plain, "-l", "/dev/null", "-s", "-a"] + flags + files, timeout=300)
    check_outputs(plain, files, t, recs)
    tq = dict(t)
    tq["keep"] = keep_out
    check_outputs(out, files, tq, recs)
    same_side_files(out, plain, files)
    assert "  quality: %d clusters keep another record\n" % n_changed in open(log).read()


def test_streaming_path_gives_the_same_files(tmp_path):
    files = synth_fastq(str(tmp_path / "in"), 3000, 19, n_files=1, umi_len=8, p_sub=4e-3, read_len=40)
    bt.rewrite_qualities(files, 19)
    outs = []
    for name, env in (("fast", {}), ("slow", {"HUMID_HOST_SLOW": "1"})):
        e = dict(os.environ)
        e.update(env)
        outs.append(str(tmp_path / name))
        subprocess.check_call([HUMID, "-Q", "-d", outs[-1], "-l", "/dev/null", "-s", "-a"] + files, env=e, timeout=300)
    for n in os.listdir(outs[0]):
        assert filecmp.cmp(os.path.join(outs[0], n), os.path.join(outs[1], n), shallow=False), n


def test_with_barcodes_and_a_whitelist(tmp_path):
    files, wl_path, wl = whitelisted_fastq(tmp_path, 4000, 61)
    scores = bt.rewrite_qualities(files, 61)
    t, recs, Ks, counts = whitelist_truth_for(files, wl, 28, 1)
    words, filt, _, _ = expected_words(files, 28)
    rest = words & np.uint64((1 << 24) - 1)                             # the 12 nucleotides the run clusters
    # an unmatched read with the top score stays out: it has no cluster
    assert np.any((t["cid"] == 0) & (filt == 0))
    keep_out, n_changed = best_keep(t, rest, scores)
    out, plain, log = str(tmp_path / "out"), str(tmp_path / "plain"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-Q", "-n", "28", "-b", "16", "-w", wl_path, "-d", out, "-l", log, "-s", "-a"] + files,
                          timeout=300)
    subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-w", wl_path, "-d", plain, "-l", "/dev/null", "-s", "-a"] + files,
                          timeout=300)
    tq = dict(t)
    tq["keep"] = keep_out
    check_all(out, files, tq, recs, Ks, counts, wl)
    same_side_files(out, plain, files)
    assert "  quality: %d clusters keep another record\n" % n_changed in open(log).read()
