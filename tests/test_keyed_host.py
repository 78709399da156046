"""CPU checks of keyed deduplication (include/humid_hip.h, humid_dedup_run_keyed) and of `humid -b K`: the Python
argument checks that need no device, the command line's refusals (before any device is opened) and the word
extraction under -b, which the split into key and word comes after."""
import os
import subprocess

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib
from humid_amd.synth import synth_fastq

from cli_util import HUMID, expected_words

NEW_SYMBOLS = ("humid_dedup_run_keyed", "humid_dedup_run_keyed_device", "humid_get_group_keys", "humid_keyed_rank_info")


def test_keyed_symbols_are_exported():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name), name
    assert lib.humid_abi_version() == 5


def test_null_context_is_refused():
    lib = _lib.load()
    assert lib.humid_dedup_run_keyed(None, None, None, None, 0, 24, 1, 0, None, None, None) == -1
    assert lib.humid_dedup_run_keyed_device(None, None, None, None, 0, 24, 1, 0, None, None, None) == -1
    assert lib.humid_get_group_keys(None, None, 0, None) == -1
    assert lib.humid_keyed_rank_info(None, None, None, None) == -1


def test_run_keyed_checks_its_arguments_before_the_library():
    """shape / dtype errors raise ValueError before the library is called: an object without a context is enough"""
    d = object.__new__(humid_amd.Dedup)
    w, f = np.zeros(10, np.uint64), np.zeros(10, np.uint8)
    k = np.arange(10, dtype=np.uint64)
    for words, keys, filt, word_nt in (
            (w, k[:9], f, 24),                                     # keys of another length
            (w, k.reshape(5, 2), f, 24),                           # keys not one-dimensional
            (w, k.astype(np.float64), f, 24),                      # keys not integers
            (w, np.arange(10) - 3, f, 24),                         # negative keys
            (w, k, f, 40),                                         # one uint64 per word at 40 nt
            (np.zeros((10, 2), np.uint64), k, f, 24),              # two at 24 nt
            (w, k, f.reshape(5, 2), 24)):
        with pytest.raises(ValueError):
            d.run_keyed(words, keys, filt, word_nt=word_nt)


@pytest.mark.parametrize("args", [["-n", "28", "-b", "0"], ["-n", "28", "-b", "33"], ["-n", "40", "-b", "33"],
                                  ["-n", "16", "-b", "16"], ["-n", "12", "-b", "20"], ["-b", "24"],
                                  ["-n", "28", "-b", "4", "-g", "2"], ["-n", "28", "-b"]])
def test_cli_refuses_bad_barcode_lengths(args, tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=40)
    if args[-1] == "-b":
        files = []                                                 # -b without a value
    r = subprocess.run([HUMID] + args + ["-d", str(tmp_path / "out"), "-l", "/dev/null"] + files, capture_output=True,
                       timeout=60)
    assert r.returncode == 2, r.stderr
    assert b"-b" in r.stderr
    assert not os.path.exists(tmp_path / "out")


@pytest.mark.parametrize("env", [{"HUMID_GPUS": "2"}, {"HUMID_FORCE_SHARDED": "1"}])
def test_cli_refuses_barcodes_on_several_ranks(env, tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=40)
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([HUMID, "-n", "28", "-b", "16", "-l", "/dev/null"] + files, capture_output=True, env=e, timeout=60)
    assert r.returncode == 2 and b"one GPU" in r.stderr


def test_usage_names_the_flag_and_the_g_line_is_current():
    r = subprocess.run([HUMID, "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0
    assert b"-b" in r.stderr and b"barcode" in r.stderr
    assert b"no -e beyond" not in r.stderr


@pytest.mark.parametrize("case", [
    dict(n_files=1, umi_len=0, umi_in_header=False, word_nt=28, b=16),          # barcode + UMI in the read
    dict(n_files=2, umi_len=8, umi_in_header=True, word_nt=24, b=8),            # header UMI first, then two files
    dict(n_files=2, umi_len=8, umi_in_header=True, word_nt=48, b=10),           # a wide word
    dict(n_files=2, umi_len=12, umi_in_header=False, umi_file=True, word_nt=64, b=32),
])
def test_word_extraction_under_b(case, tmp_path):
    """--dump-words with -b writes the n-nucleotide words the oracle's extraction gives, fast and streaming path"""
    case = dict(case)
    word_nt, b = case.pop("word_nt"), case.pop("b")
    files = synth_fastq(str(tmp_path / "in"), 3000, 5, p_sub=4e-3, p_n=3e-3, read_len=40, short_frac=0.02, **case)
    words, filt, _, _ = expected_words(files, word_nt)
    for env in ({}, {"HUMID_HOST_SLOW": "1"}, {"HUMID_DEVICE_PACK": "1"}):
        out = str(tmp_path / "words.bin")
        e = dict(os.environ)
        e.update(env)
        subprocess.check_call([HUMID, "-n", str(word_nt), "-b", str(b), "-l", "/dev/null", "--dump-words", out] + files,
                              env=e, timeout=120)
        raw = open(out, "rb").read()
        n = int(np.frombuffer(raw[:8], np.uint64)[0])
        wpr = 2 if word_nt > 32 else 1
        got = np.frombuffer(raw[8:8 + 8 * n * wpr], np.uint64)
        got_f = np.frombuffer(raw[8 + 8 * n * wpr:8 + 8 * n * wpr + n], np.uint8)
        assert n == len(filt) and np.array_equal(got_f, filt)
        assert np.array_equal(got.reshape(words.shape), words)
