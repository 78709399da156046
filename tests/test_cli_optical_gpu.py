"""-m gpu: `humid -O 100 -s -a` end to end.  The names of the synthetic files are rewritten to Illumina form
(tests/optical_truth.rewrite_headers, which returns the positions it wrote); expected words come from the oracle's word
extraction (cli_util.expected_words), cluster ids and keep flags from the oracle run (tests/grouped_truth.py), with -Q
the survivors from tests/best_truth.py, and the split of the duplicates from tests/optical_truth.py.  optical.dat and
the two log lines must equal that truth; every other file is the one of the same run without -O, byte for byte."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, expected_words
from humid_amd.synth import synth_fastq
from test_cli_keyed_gpu import check_outputs

import best_truth as bt
import grouped_truth as gt
import optical_truth as ot

pytestmark = pytest.mark.gpu

D = 100


def make_input(tmp_path, n_files, style, seed=31):
    files = synth_fastq(str(tmp_path / "in"), 4000, seed, n_files=n_files, umi_len=8, p_sub=4e-3, p_n=2e-3, read_len=40,
                        short_frac=0.01, header_style=style)
    pos = ot.rewrite_headers(files, seed + 1, style)
    words, filt, recs, _ = expected_words(files, 24)
    t = gt.per_group(words, np.zeros(len(filt), np.uint32), filt, 24, 1, 0)
    return files, pos, words, t, recs


def expected_dat(t, keep, pos):
    o = ot.truth(t["cid"], keep, pos[0], pos[1], pos[2], D, t["summary"]["clusters"])
    s = o[3]
    assert s["optical"] > 20 and s["duplicates"] > s["optical"]          # the case says something
    lines = [("members", s["members"]), ("duplicates", s["duplicates"]), ("optical", s["optical"]),
             ("pcr", s["duplicates"] - s["optical"]), ("groups", s["groups"]), ("largest_group", s["largest_group"]),
             ("records_without_position", int((pos[0] == ot.NO_TILE).sum()))]
    return "".join("%s %d\n" % kv for kv in lines), s


def check_optical(out, log, t, keep, pos):
    want, s = expected_dat(t, keep, pos)
    assert open(os.path.join(out, "optical.dat")).read() == want
    text = open(log).read()
    assert "  optical: %d of %d duplicates in %d groups\n" % (s["optical"], s["duplicates"], s["groups"]) in text
    assert "  positions: %d of %d records\n" % (int((pos[0] != ot.NO_TILE).sum()), len(pos[0])) in text
    return s


def same_files_but_optical_dat(with_o, without_o):
    names = sorted(os.listdir(without_o))
    assert sorted(os.listdir(with_o)) == sorted(names + ["optical.dat"])
    for n in names:
        assert filecmp.cmp(os.path.join(with_o, n), os.path.join(without_o, n), shallow=False), n


@pytest.mark.parametrize("n_files,style", [(1, "_"), (2, "_"), (1, ":"), (2, ":")])
def test_optical_dat_and_log(n_files, style, tmp_path):
    files, pos, words, t, recs = make_input(tmp_path, n_files, style)
    out, plain, log = str(tmp_path / "out"), str(tmp_path / "plain"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-O", str(D), "-d", out, "-l", log, "-s", "-a"] + files, timeout=300)
    subprocess.check_call([HUMID, "-d", plain, "-l", "/dev/null", "-s", "-a"] + files, timeout=300)
    check_outputs(plain, files, t, recs)
    check_optical(out, log, t, t["keep"], pos)
    same_files_but_optical_dat(out, plain)


def test_with_best_quality_the_origin_follows_the_selected_read(tmp_path):
    files, pos, words, t, recs = make_input(tmp_path, 1, "_", seed=37)
    scores = bt.rewrite_qualities(files, 37)
    recs = expected_words(files, 24)[2]                                 # (the quality lines changed)
    keep_q = bt.select_sort(words, t["cid"], t["keep"], scores, bt.LEAF)
    assert keep_q[2] > 0
    out, plain, log = str(tmp_path / "out"), str(tmp_path / "plain"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-O", str(D), "-Q", "-d", out, "-l", log, "-s", "-a"] + files, timeout=300)
    subprocess.check_call([HUMID, "-Q", "-d", plain, "-l", "/dev/null", "-s", "-a"] + files, timeout=300)
    tq = dict(t)
    tq["keep"] = keep_q[0]
    check_outputs(plain, files, tq, recs)
    check_optical(out, log, t, keep_q[0], pos)
    same_files_but_optical_dat(out, plain)
    # the definition is what moved: the origins under the run's own keep are other reads
    a = ot.optical_sweep(t["cid"], t["keep"], *pos, D, t["summary"]["clusters"])
    b = ot.optical_sweep(t["cid"], keep_q[0], *pos, D, t["summary"]["clusters"])
    assert not np.array_equal(a[1], b[1])


def test_streaming_path_gives_the_same_files(tmp_path):
    files, pos, words, t, recs = make_input(tmp_path, 2, "_", seed=41)
    outs = []
    for name, env in (("fast", {}), ("slow", {"HUMID_HOST_SLOW": "1"})):
        e = dict(os.environ)
        e.update(env)
        outs.append(str(tmp_path / name))
        subprocess.check_call([HUMID, "-O", str(D), "-d", outs[-1], "-l", str(tmp_path / (name + ".log")), "-s", "-a"] + files,
                              env=e, timeout=300)
    assert sorted(os.listdir(outs[0])) == sorted(os.listdir(outs[1])) and "optical.dat" in os.listdir(outs[0])
    for n in os.listdir(outs[0]):
        assert filecmp.cmp(os.path.join(outs[0], n), os.path.join(outs[1], n), shallow=False), n
    check_optical(outs[1], str(tmp_path / "slow.log"), t, t["keep"], pos)


def test_refused_with_several_gpus(tmp_path):
    files = synth_fastq(str(tmp_path / "in"), 200, 3, n_files=1, umi_len=8, read_len=40)
    p = subprocess.run([HUMID, "-O", "100", "-g", "2", "-d", str(tmp_path / "out"), "-l", "/dev/null"] + files,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 1
    assert b"humid: -O runs on one GPU (not with -g, HUMID_GPUS or HUMID_FORCE_SHARDED)" in p.stderr
    assert not os.path.exists(str(tmp_path / "out" / "optical.dat"))
