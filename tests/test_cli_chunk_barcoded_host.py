"""CPU: `humid --chunk-barcoded N` is refused -- exit status 2, one line starting `humid: --chunk-barcoded`, before any
GPU use and before any file or directory is created -- without a barcode and together with what a keyed accumulated run
does not do; it appears in the usage text, and `--chunk-reads` keeps its own refusals."""
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
    d = tmp_path_factory.mktemp("chunk_barcoded_in")
    files = synth_fastq(str(d), 50, 4, n_files=2, umi_len=0, umi_in_header=False, read_len=60)
    wl = str(d / "wl.txt")
    open(wl, "w").write("ACGTACGT\n")
    return files, wl


NO_GPU = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")      # (a GPU could not be opened anyway)

REFUSED = [
    ([], "needs a barcode"), (["-n", "24"], "needs a barcode"), (["-n", "8", "--word-pattern", "NNNNNNNN"], "needs a barcode"),
    (["-b", "8", "--chunk-reads", "20"], "--chunk-reads"), (["-b", "8", "-g", "2"], "-g"),
    (["-b", "8", "-P"], "-P"), (["-b", "8", "-Q"], "-Q"), (["-b", "8", "-C"], "-C"), (["-b", "8", "-P", "-D"], "-P"),
    (["-b", "8", "-D"], "-D"), (["-b", "8", "-O", "100"], "-O"), (["-b", "8", "-w", "WL", "-Q"], "-Q"),
    (["-b", "8", "--cells-top", "5", "-C"], "-C"),
    (["-n", "41", "-b", "8"], "32 letters"), (["-n", "64", "-b", "31", "-w", "WL"], "32 letters"),
    (["-n", "41", "--word-pattern", "CCCCCCCC" + "N" * 33], "32 letters"),
]


@pytest.mark.parametrize("extra,names", REFUSED)
def test_refused_combinations(extra, names, inputs, tmp_path):
    files, wl = inputs
    extra = [wl if x == "WL" else x for x in extra]
    out = str(tmp_path / "out")
    r = subprocess.run([HUMID, "--chunk-barcoded", "20", "-d", out, "-l", str(tmp_path / "log")] + extra + files[:1],
                       env=dict(os.environ, **NO_GPU), capture_output=True, text=True)
    assert r.returncode == 2, r.stderr
    lines = r.stderr.strip().split("\n")
    assert len(lines) == 1 and lines[0].startswith("humid: --chunk-barcoded") and names in lines[0], r.stderr
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "log"))


def test_sharded_by_environment_is_refused(inputs, tmp_path):
    files, _ = inputs
    for var in ("HUMID_GPUS", "HUMID_FORCE_SHARDED"):
        env = dict(os.environ, **NO_GPU)
        env[var] = "2"
        r = subprocess.run([HUMID, "--chunk-barcoded", "20", "-b", "8", "-d", str(tmp_path / "o")] + files[:1], env=env,
                           capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.startswith("humid: --chunk-barcoded runs on one GPU"), r.stderr
        assert r.stderr.count("\n") == 1 and not os.path.exists(str(tmp_path / "o"))


@pytest.mark.parametrize("value", ["0", "-3", "x", "12k", ""])
def test_chunk_barcoded_wants_a_number_of_one_or_more(value, inputs, tmp_path):
    files, _ = inputs
    r = subprocess.run([HUMID, "--chunk-barcoded", value, "-b", "8", "-d", str(tmp_path / "o")] + files[:1], env=dict(os.environ, **NO_GPU),
                       capture_output=True, text=True)
    assert r.returncode == 2
    assert r.stderr.split("\n")[0] == "humid: --chunk-barcoded takes a number of records, 1 or more"
    if value == "0":
        assert r.stderr.count("\n") == 1
    assert not os.path.exists(str(tmp_path / "o"))


def test_usage_names_the_flag():
    r = subprocess.run([HUMID, "-h"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "[--chunk-barcoded N]" in r.stderr and "\n  --chunk-barcoded N  " in r.stderr
    assert "[--chunk-reads N]" in r.stderr and "\n  --chunk-reads N  " in r.stderr
    r = subprocess.run([HUMID, "--chunk-barcoded"], capture_output=True, text=True)
    assert r.returncode == 2 and "--chunk-barcoded needs a value" in r.stderr


def test_chunk_reads_keeps_refusing_a_barcode(inputs, tmp_path):
    files, wl = inputs
    for extra in (["-b", "8"], ["-w", wl], ["--cells-top", "5"], ["--word-pattern", "NNNNNNNN"]):
        r = subprocess.run([HUMID, "--chunk-reads", "20", "-d", str(tmp_path / "o")] + extra + files[:1], env=dict(os.environ, **NO_GPU),
                           capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.startswith("humid: --chunk-reads does not work with") and r.stderr.count("\n") == 1
