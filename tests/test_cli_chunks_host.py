"""CPU: `humid --chunk-reads N` is refused -- exit status 2, one line, before any GPU use -- together with what an
accumulated run does not do, and appears in the usage text."""
import os
import subprocess

import pytest

from cli_util import HUMID
from humid_amd import build
from humid_amd.synth import synth_fastq


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("chunks_in")
    files = synth_fastq(str(d), 50, 4, n_files=2, umi_len=0, umi_in_header=False, read_len=30)
    wl = str(d / "wl.txt")
    open(wl, "w").write("ACGTACGT\n")
    return files, wl


REFUSED = [
    (["-g", "2"], "-g"), (["-b", "8"], "-b"), (["-b", "8", "-w", "WL"], "-b"), (["-w", "WL"], "-w"),
    (["-b", "8", "--cells-top", "5"], "-b"), (["--cells-expected", "5"], "--cells"), (["--cells-min-reads", "5"], "--cells"),
    (["--cells-merge-ratio", "3"], "--cells"), (["--word-pattern", "NNNNNNNN"], "--word-pattern"), (["-P"], "-P"),
    (["-Q"], "-Q"), (["-C"], "-C"), (["-P", "-D"], "-P"), (["-D"], "-D"), (["-O", "100"], "-O"),
]


@pytest.mark.parametrize("extra,names", REFUSED)
def test_refused_combinations(extra, names, inputs, tmp_path):
    files, wl = inputs
    extra = [wl if x == "WL" else x for x in extra]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # (a GPU could not be opened anyway)
    out = str(tmp_path / "out")
    r = subprocess.run([HUMID, "--chunk-reads", "20", "-d", out, "-l", str(tmp_path / "log")] + extra + files, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 2, r.stderr
    lines = r.stderr.strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("humid: --chunk-reads") and names in lines[0], r.stderr
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "log"))


def test_sharded_by_environment_is_refused(inputs, tmp_path):
    files, _ = inputs
    for var in ("HUMID_GPUS", "HUMID_FORCE_SHARDED"):
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        env[var] = "2"
        r = subprocess.run([HUMID, "--chunk-reads", "20", "-d", str(tmp_path / "o")] + files, env=env, capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.startswith("humid: --chunk-reads runs on one GPU"), r.stderr


@pytest.mark.parametrize("value", ["0", "-3", "x", "12k", ""])
def test_chunk_reads_wants_a_number_of_one_or_more(value, inputs, tmp_path):
    files, _ = inputs
    r = subprocess.run([HUMID, "--chunk-reads", value, "-d", str(tmp_path / "o")] + files, capture_output=True, text=True)
    assert r.returncode == 2
    assert r.stderr.split("\n")[0] == "humid: --chunk-reads takes a number of records, 1 or more"
    if value == "0":
        assert r.stderr.count("\n") == 1


def test_usage_names_the_flag():
    r = subprocess.run([HUMID, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "[--chunk-reads N]" in r.stderr and "\n  --chunk-reads N  " in r.stderr
    r = subprocess.run([HUMID, "--chunk-reads"], capture_output=True, text=True)
    assert r.returncode == 2 and "--chunk-reads needs a value" in r.stderr
