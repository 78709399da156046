"""-m gpu: `humid --long-words` end to end (FastQ in -> _dedup / _annotated FastQ + .dat out) against outputs
constructed from tests/long_truth.py, in the shape of tests/test_cli_gpu.py::test_cli_end_to_end."""
import filecmp
import os
import subprocess

import pytest

import long_truth as lt
from cli_util import HUMID, read_fastq
from humid_amd.synth import synth_fastq
from test_cli_long_host import expected_long_words

pytestmark = pytest.mark.gpu


def dat(path):
    return [tuple(int(x) for x in l.split()) for l in open(path).read().strip().split("\n") if l]


@pytest.mark.parametrize("case", [
    dict(n_files=2, umi_len=8, umi_in_header=True, read_len=60, short_frac=0.01, word_nt=100, d=1, x=False, n=3000),
    dict(n_files=2, umi_len=0, umi_in_header=False, read_len=80, word_nt=150, d=2, x=True, n=2000),
])
def test_cli_long_end_to_end(case, tmp_path):
    case = dict(case)
    word_nt, d, x, n = case.pop("word_nt"), case.pop("d"), case.pop("x"), case.pop("n")
    files = synth_fastq(str(tmp_path / "in"), n, 123, p_sub=4e-3, p_n=2e-3, **case)
    out = str(tmp_path / "out" / "nested")
    cmd = [HUMID, "--long-words", "-n", str(word_nt), "-m", str(d), "-d", out, "-l", str(tmp_path / "log.txt"), "-s", "-a"]
    if x:
        cmd.append("-x")
    subprocess.check_call(cmd + files)
    words, filt, recs = expected_long_words(files, word_nt)
    t = lt.long_dedup(words, filt, d, x)
    cid, keep = t["cid"], t["keep"]
    assert t["summary"]["edges"] > 0 and t["summary"]["clusters"] < t["summary"]["unique"]
    for fi, f in enumerate(files):
        base = os.path.basename(f)
        dedup = read_fastq(os.path.join(out, base.replace(".fastq", "_dedup.fastq")))
        annot = read_fastq(os.path.join(out, base.replace(".fastq", "_annotated.fastq")))
        assert dedup == [recs[fi][i] for i in range(n) if keep[i]]
        assert annot == [(recs[fi][i][0] + ":%d" % cid[i],) + recs[fi][i][1:] for i in range(n)]
    h = t["hist"]
    assert dat(os.path.join(out, "counts.dat")) == h["counts"]
    assert dat(os.path.join(out, "neigh.dat")) == h["neigh"]
    assert dat(os.path.join(out, "clusters.dat")) == h["clusters"]
    stats = dict(l.split(": ") for l in open(os.path.join(out, "stats.dat")).read().strip().split("\n"))
    assert {k: int(v) for k, v in stats.items()} == h["stats"]
    log = open(tmp_path / "log.txt").read()
    assert "Calculating neighbours using Hamming distance... done." in log
    assert ("Calculating maximum clusters" if x else "Calculating directional clusters") in log
    assert "Writing filtered results... done." in log and "Writing annotated results... done." in log


def test_at_48_nt_the_flag_writes_identical_files(tmp_path):
    files = synth_fastq(str(tmp_path / "in"), 3000, 124, n_files=2, umi_len=8, read_len=36, p_sub=4e-3, p_n=2e-3, short_frac=0.01)
    outs = []
    for flag in ([], ["--long-words"]):
        out = str(tmp_path / ("out%d" % len(flag)))
        subprocess.check_call([HUMID] + flag + ["-n", "48", "-d", out, "-l", "/dev/null", "-s", "-a"] + files)
        outs.append(out)
    names = sorted(os.listdir(outs[0]))
    assert names == sorted(os.listdir(outs[1])) and len(names) == 8          # 2 x (_dedup, _annotated) + four .dat
    match, mismatch, errors = filecmp.cmpfiles(outs[0], outs[1], names, shallow=False)
    assert sorted(match) == names and not mismatch and not errors
