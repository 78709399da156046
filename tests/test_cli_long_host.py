"""Host side of `humid --long-words` without a GPU: word extraction beyond 64 nucleotides (--dump-words stops after
pass 1) against the oracle's restatement of src/fastq.cc, and every refused combination."""
import os
import subprocess

import numpy as np
import pytest

import long_truth as lt
from cli_util import HUMID, dump_words, read_fastq
from humid_amd import build
from humid_amd.synth import synth_fastq
from oracle import pyoracle as orc


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def expected_long_words(files, word_nt):
    """cli_util.expected_words for any length: preCompute + getNucleotides + makeWord per record, packed here into
    ceil(word_nt / 32) uint64"""
    recs = [read_fastq(f) for f in files]
    n = min(len(r) for r in recs)
    first_umi = len(orc.extract_umi(recs[0][0][0])) if n else 0
    hdr, take = orc.pre_compute(first_umi, len(files), word_nt)
    syms = np.zeros((n, word_nt), dtype=np.uint8)
    filt = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        nuc = orc.get_nucleotides(recs[0][i][0], [r[i][1] for r in recs], take, hdr)
        data, fl = orc.make_word(nuc)
        assert len(data) == word_nt
        syms[i] = data
        filt[i] = fl
    return lt.pack_syms(syms), filt, recs


def dump_long_words(files, word_nt, tmp, extra=()):
    out = os.path.join(tmp, "words_long.bin")
    subprocess.check_call([HUMID, "--long-words", "-n", str(word_nt), "-l", os.path.join(tmp, "log.txt"), "--dump-words", out] +
                          list(extra) + list(files))
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], dtype=np.uint64)[0])
    k = (word_nt + 31) // 32
    assert len(raw) == 8 + 8 * n * k + n
    return np.frombuffer(raw[8:8 + 8 * n * k], dtype=np.uint64).reshape(n, k), np.frombuffer(raw[8 + 8 * n * k:], dtype=np.uint8)


@pytest.mark.parametrize("word_nt", [65, 100, 150])
@pytest.mark.parametrize("case", [
    dict(n_files=1, umi_len=8, umi_in_header=True, read_len=160, short_frac=0.1),
    dict(n_files=2, umi_len=8, umi_in_header=True, read_len=80, short_frac=0.1),
    dict(n_files=2, umi_len=0, umi_in_header=False, read_len=60),                       # reads shorter than their share at 150
])
def test_long_words_match_the_python_extraction(case, word_nt, tmp_path):
    files = synth_fastq(str(tmp_path), 300, 99, p_sub=5e-3, p_n=3e-3, **case)
    w, f = dump_long_words(files, word_nt, str(tmp_path))
    ew, ef, _ = expected_long_words(files, word_nt)
    assert len(w) == 300 and 0 < int(ef.sum()) and (int(ef.sum()) < 300 or case["read_len"] == 60)
    assert np.array_equal(f, ef)
    assert np.array_equal(w, ew)


def test_streaming_path_packs_the_same_long_words(tmp_path):
    files = synth_fastq(str(tmp_path), 300, 98, n_files=2, umi_len=8, read_len=80, p_sub=5e-3, p_n=3e-3, short_frac=0.05)
    w, f = dump_long_words(files, 150, str(tmp_path))
    env = dict(os.environ, HUMID_HOST_SLOW="1")
    out = str(tmp_path / "slow.bin")
    subprocess.check_call([HUMID, "--long-words", "-n", "150", "-l", "/dev/null", "--dump-words", out] + files, env=env)
    raw = open(out, "rb").read()
    assert raw[8:8 + w.nbytes] == w.tobytes() and raw[8 + w.nbytes:] == f.tobytes()


@pytest.mark.parametrize("word_nt", [24, 32, 48, 64])
def test_up_to_64_nt_the_flag_dumps_the_same_words(word_nt, tmp_path):
    files = synth_fastq(str(tmp_path), 300, 97, n_files=2, umi_len=8, read_len=40, p_sub=5e-3, p_n=3e-3, short_frac=0.05)
    w, f = dump_words(files, word_nt, str(tmp_path))
    wl, fl = dump_long_words(files, word_nt, str(tmp_path))
    assert np.array_equal(wl, w.reshape(wl.shape)) and np.array_equal(fl, f)


REFUSED = [["-e"], ["-g", "2"], ["-b", "8"], ["-b", "8", "-w", "list.txt"], ["-w", "list.txt"], ["-P"], ["-Q"], ["-C"], ["-P", "-D"],
           ["-D"], ["-O", "10"],
           ["--chunk-reads", "100"], ["-b", "8", "--chunk-barcoded", "100"], ["--cells-top", "5"], ["--cells-expected", "5"],
           ["--cells-min-reads", "5"], ["--cells-merge-ratio", "3"], ["--word-pattern", "CCCCNNNN"], ["--barcode-posterior"],
           ["--barcode-min-odds", "10"], ["--barcode-max-inexact", "1"]]


@pytest.mark.parametrize("flags", REFUSED, ids=[" ".join(f) for f in REFUSED])
def test_refused_combinations_exit_2(flags, tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=2, read_len=80)
    r = subprocess.run([HUMID, "--long-words", "-n", "100", "-l", "/dev/null", "-d", str(tmp_path / "o")] + flags + files,
                       stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "--long-words" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "o")


@pytest.mark.parametrize("env", [{"HUMID_GPUS": "2"}, {"HUMID_FORCE_SHARDED": "1"}], ids=["HUMID_GPUS", "HUMID_FORCE_SHARDED"])
def test_sharding_from_the_environment_is_refused(env, tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=2, read_len=80)
    r = subprocess.run([HUMID, "--long-words", "-n", "100", "-l", "/dev/null", "-d", str(tmp_path / "o")] + files,
                       stderr=subprocess.PIPE, text=True, env=dict(os.environ, **env))
    assert r.returncode == 2 and "--long-words runs on one GPU" in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "o")


def test_word_length_limits(tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=30)
    r = subprocess.run([HUMID, "-n", "65"] + files, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and "--long-words" in r.stderr                # the message names the flag
    for n in ("513", "0"):
        r = subprocess.run([HUMID, "--long-words", "-n", n] + files, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 2, n
    w, _ = dump_long_words(files, 512, str(tmp_path))
    assert w.shape == (4, 16)
