"""No GPU: the two truths of tests/best_truth.py against each other (on the oracle's output and on hand cases), the
new symbols of the C ABI, the command line's refusal of -Q on several ranks, the usage text, and the -Q scores of
pass 1 (--dump-scores) against a Python sum on every input path."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib
from humid_amd.synth import synth_fastq, synth_words
from oracle import pyoracle as orc

import best_truth as bt
from cli_util import HUMID, ROOT

U64 = np.uint64


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("distance", [0, 1, 2])
def test_the_two_truths_agree_on_the_oracle(distance, method):
    words, filt = synth_words(20_000, 5, 24, p_sub=4e-3)
    cid, keep, s, _ = orc.dedup_run(words, filt, 24, distance, method)
    scores = np.random.default_rng(distance).integers(0, 12000, len(words)).astype(np.uint32)
    out = {}
    for scope in (bt.LEAF, bt.CLUSTER):
        a = bt.select_sort(words, cid, keep, scores, scope)
        bt.assert_same(a, bt.select_loop(words, cid, keep, scores, scope))
        assert int(a[0].sum()) == s["clusters"] and np.all(a[1][cid == 0] == bt.NO_READ)
        assert np.array_equal(cid[a[1][cid != 0]], cid[cid != 0])      # a representative is of the read's cluster
        out[scope] = a
    assert out[bt.LEAF][2] > 0
    if distance:
        assert np.count_nonzero(out[bt.LEAF][0] != out[bt.CLUSTER][0]) > 0
    const = bt.select_sort(words, cid, keep, np.full(len(words), 9, np.uint32), bt.LEAF)
    assert np.array_equal(const[0], keep) and const[2] == 0


def test_the_200k_case_is_not_degenerate():
    words, filt = synth_words(200_000, 5, 24)
    cid, keep, s, _ = orc.dedup_run(words, filt, 24, 1, 0)
    scores = np.random.default_rng(5).integers(0, 12000, len(words)).astype(np.uint32)
    leaf = bt.select_sort(words, cid, keep, scores, bt.LEAF)
    cluster = bt.select_sort(words, cid, keep, scores, bt.CLUSTER)
    assert s["clusters"] == 50_649
    assert leaf[2] > s["clusters"] // 4 and np.count_nonzero(leaf[0] != cluster[0]) > 100
    assert int(leaf[0].sum()) == int(cluster[0].sum()) == s["clusters"]


def test_hand_cases():
    A, B = 0x10, 0x11                                                   # two words of one cluster; A is the maxLeaf
    words = np.asarray([A, B, A, A, B, 0x77, 0x99], U64)
    cid = np.asarray([1, 1, 1, 1, 1, 0, 2], np.uint32)
    keep = np.asarray([1, 0, 0, 0, 0, 0, 1], np.uint8)

    def both(scores, scope):
        a = bt.select_loop(words, cid, keep, np.asarray(scores, np.uint32), scope)
        bt.assert_same(a, bt.select_sort(words, cid, keep, np.asarray(scores, np.uint32), scope))
        return list(a[0]), list(a[1]), a[2]

    NO = bt.NO_READ
    # a tie at the top: the smallest index
    assert both([1, 9, 5, 5, 9, 9, 0], bt.LEAF) == ([0, 0, 1, 0, 0, 0, 1], [2, 2, 2, 2, 2, NO, 6], 1)
    assert both([1, 9, 5, 5, 9, 9, 0], bt.CLUSTER) == ([0, 1, 0, 0, 0, 0, 1], [1, 1, 1, 1, 1, NO, 6], 1)
    # the best read outside the maxLeaf stays out under LEAF
    assert both([3, 8, 2, 1, 0, 0, 0], bt.LEAF) == ([1, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, NO, 6], 0)
    # score 0 everywhere and score 2^32 - 1
    assert both([0] * 7, bt.LEAF) == ([1, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, NO, 6], 0)
    top = 0xffffffff
    assert both([0, 0, 0, top, top, top, 0], bt.LEAF) == ([0, 0, 0, 1, 0, 0, 1], [3, 3, 3, 3, 3, NO, 6], 1)
    assert both([top - 1, 0, 0, top, top, top, 0], bt.CLUSTER) == ([0, 0, 0, 1, 0, 0, 1], [3, 3, 3, 3, 3, NO, 6], 1)
    # wide words: equal in one half only is another word
    wide = np.asarray([[1, 2], [1, 3], [0, 2], [1, 2]], U64)
    c2, k2 = np.asarray([1, 1, 1, 1], np.uint32), np.asarray([1, 0, 0, 0], np.uint8)
    a = bt.select_loop(wide, c2, k2, np.asarray([0, 9, 9, 5], np.uint32), bt.LEAF)
    bt.assert_same(a, bt.select_sort(wide, c2, k2, np.asarray([0, 9, 9, 5], np.uint32), bt.LEAF))
    assert list(a[0]) == [0, 0, 0, 1]


def test_symbols_are_declared_and_exported():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "humid_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("humid_select_best", "humid_select_best_device"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SYMBOLS and hasattr(lib, name)
    for macro in ("HUMID_BEST_LEAF", "HUMID_BEST_CLUSTER", "HUMID_NO_READ"):
        assert re.search(r"#define\s+%s\b" % macro, text)
    assert (humid_amd.BEST_LEAF, humid_amd.BEST_CLUSTER, humid_amd.NO_READ) == (0, 1, 0xffffffff)
    assert lib.humid_abi_version() == 5
    assert lib.humid_select_best(None, None, None, None, None, 0, 24, 0, None, None, None) == -1     # no context


@pytest.mark.parametrize("how", ["-g", "HUMID_GPUS", "HUMID_FORCE_SHARDED"])
def test_cli_refuses_q_on_several_ranks(how, tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=40)
    e = dict(os.environ)
    args = ["-Q"]
    if how == "-g":
        args += ["-g", "2"]
    else:
        e[how] = "2" if how == "HUMID_GPUS" else "1"
    r = subprocess.run([HUMID] + args + ["-d", str(tmp_path / "out"), "-l", "/dev/null"] + files, capture_output=True, env=e,
                       timeout=60)
    assert r.returncode == 2 and b"one GPU" in r.stderr and b"-Q" in r.stderr
    assert not os.path.exists(tmp_path / "out")


def test_usage_names_the_flag():
    r = subprocess.run([HUMID, "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"-Q" in r.stderr and b"qualit" in r.stderr


def dump_scores(files, tmp, env=None, extra=()):
    out = os.path.join(str(tmp), "scores.bin")
    e = dict(os.environ)
    e.update(env or {})
    subprocess.check_call([HUMID, "-l", "/dev/null", "--dump-scores", out] + list(extra) + list(files), env=e, timeout=120)
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], np.uint64)[0])
    assert len(raw) == 8 + 4 * n
    return np.frombuffer(raw[8:], np.uint32)


@pytest.mark.parametrize("n_files", [1, 2])
def test_dump_scores_on_every_input_path(n_files, tmp_path):
    """mapped, streaming, gzip inflated in memory, gzip streamed, CRLF; short reads; 1, 3 and 8 workers"""
    files = synth_fastq(str(tmp_path / "in"), 3000, 7, n_files=n_files, read_len=40, short_frac=0.05, p_n=3e-3)
    want = bt.rewrite_qualities(files, 7)
    assert len(want) == 3000 and want.min() < want.max() and len(set(want.tolist())) > 100
    for threads in ("1", "3", "8"):
        assert np.array_equal(dump_scores(files, tmp_path, {"HUMID_THREADS": threads}), want), threads
    assert np.array_equal(dump_scores(files, tmp_path, {"HUMID_HOST_SLOW": "1"}), want)
    assert np.array_equal(dump_scores(files, tmp_path, extra=["-Q", "-b", "8"]), want)
    gz, crlf = [], []
    for f in files:
        raw = open(f, "rb").read()
        gz.append(f + ".gz")
        with gzip.open(gz[-1], "wb") as fh:
            fh.write(raw)
        crlf.append(f.replace(".fastq", "_crlf.fastq"))
        open(crlf[-1], "wb").write(raw.replace(b"\n", b"\r\n"))
    for env in ({}, {"HUMID_THREADS": "3"}, {"HUMID_HOST_SLOW": "1"}):
        assert np.array_equal(dump_scores(gz, tmp_path, env), want), env
    assert np.array_equal(dump_scores(crlf, tmp_path), want)
    # with --dump-words beside it both files are written
    words_bin = str(tmp_path / "words.bin")
    assert np.array_equal(dump_scores(files, tmp_path, extra=["--dump-words", words_bin]), want)
    assert os.path.getsize(words_bin) == 8 + 3000 * 9


def test_without_q_nothing_is_scored(tmp_path):
    """--dump-words alone still writes exactly words and flags"""
    files = synth_fastq(str(tmp_path / "in"), 100, 3, n_files=1, read_len=40)
    out = str(tmp_path / "w.bin")
    subprocess.check_call([HUMID, "-l", "/dev/null", "--dump-words", out] + files, timeout=60)
    assert os.path.getsize(out) == 8 + 100 * 9 and not os.path.exists(tmp_path / "scores.bin")
