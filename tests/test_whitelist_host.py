"""CPU checks of the barcode whitelist correction (include/humid_hip.h, humid_whitelist_*) and of `humid -b K -w FILE`:
the two truths of tests/whitelist_truth.py against each other and against hand cases, the exported symbols, the
Python argument checks that need no device, and the command line's refusals (before any device is opened)."""
import os
import subprocess

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib
from humid_amd.synth import synth_fastq

from cli_util import HUMID
import whitelist_truth as wt

U64 = np.uint64
NEW_SYMBOLS = ("humid_whitelist_set", "humid_whitelist_info", "humid_whitelist_correct", "humid_whitelist_correct_device",
               "humid_dedup_run_keyed_corrected", "humid_dedup_run_keyed_corrected_device", "humid_get_barcode_status")


def enc(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16, 31, 32])
def test_the_two_truths_agree(k):
    rng = np.random.default_rng(k)
    for n_wl in (1, 2, 7, 60):
        wl = wt.whitelist_with_neighbours(rng, n_wl, k)
        keys, filt = wt.make_keys(rng, wl, k, 400, p1=0.15, p2=0.1, pr=0.1)
        if k < 32:
            keys[::37] |= U64(1) << U64(2 * k)                      # bits above 2 K
        a = wt.correct(keys, filt, wl, k)
        b = wt.correct_all_pairs(keys, filt, wl, k)
        c = wt.correct_np(keys, filt, wl, k)
        for x, y, z in zip(a, b, c):
            assert np.array_equal(x, y) and np.array_equal(x, z) and x.dtype == z.dtype
        assert int(a[2].sum()) == len(keys) and int(a[2][0]) == int(filt.sum())
        assert np.all(a[0][filt == 1] == 0) and np.all(a[1][filt == 1] == 0)
        changed = a[0] != keys
        assert np.array_equal(changed & (filt == 0), a[1] == wt.CORRECTED)


def test_generator_reaches_every_status():
    rng = np.random.default_rng(5)
    for k, n_wl in ((3, 5), (16, 200), (22, 200), (32, 200)):       # (4^3 = 64 keys: a small whitelist leaves room)
        wl = wt.whitelist_with_neighbours(rng, n_wl, k)
        keys, filt = wt.make_keys(rng, wl, k, 3000)
        _, status, _ = wt.correct(keys, filt, wl, k)
        assert wt.status_set(status) == {0, 1, 2, 3, 4}, k


def test_hand_cases():
    keys = np.asarray([enc(s) for s in ("AC", "CA", "AG", "GG", "AA", "CC", "TT")], U64)
    f = np.zeros(len(keys), np.uint8)
    f[-1] = 1
    for truth in (wt.correct, wt.correct_all_pairs):
        out, status, counts = truth(keys, f, [enc("AA"), enc("CC")], 2)
        assert list(status) == [3, 3, 2, 4, 1, 1, 0]
        assert list(out) == [enc("AC"), enc("CA"), enc("AA"), enc("GG"), enc("AA"), enc("CC"), 0]
        assert list(counts) == [1, 2, 1, 2, 1]
        # AC is a barcode itself: exact, although AA lies one nucleotide away
        out, status, _ = truth(np.asarray([enc("AC"), enc("AT")], U64), np.zeros(2, np.uint8), [enc("AA"), enc("AC")], 2)
        assert list(status) == [1, 3] and list(out) == [enc("AC"), enc("AT")]
        # a key with bits above 2 K is unmatched, whatever its low bits are
        out, status, _ = truth(np.asarray([enc("AA") | 16, enc("AG") | 16], U64), np.zeros(2, np.uint8), [enc("AA")], 2)
        assert list(status) == [4, 4]


def test_hash_copies_invert_each_other():
    for x in (0, 1, wt.TOP, 0x0123456789ABCDEF, 1 << 63):
        assert wt.unmix64(wt.mix64(x)) == x and wt.mix64(wt.unmix64(x)) == x


def test_whitelist_symbols_are_exported():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name), name
    assert (humid_amd.BC_FILTERED, humid_amd.BC_EXACT, humid_amd.BC_CORRECTED, humid_amd.BC_AMBIGUOUS,
            humid_amd.BC_UNMATCHED) == (0, 1, 2, 3, 4)
    hdr = open(os.path.join(os.path.dirname(HUMID), "..", "include", "humid_hip.h")).read()
    for i, name in enumerate(("FILTERED", "EXACT", "CORRECTED", "AMBIGUOUS", "UNMATCHED")):
        assert "#define HUMID_BC_%s" % name in hdr and ("HUMID_BC_%-9s %du" % (name, i)) in hdr


def test_null_context_is_refused():
    lib = _lib.load()
    one = np.zeros(1, U64)
    assert lib.humid_whitelist_set(None, one.ctypes.data, 1, 16) == -1
    assert lib.humid_whitelist_set(None, None, 0, 16) == -1
    assert lib.humid_whitelist_info(None, None, None, None) == -1
    assert lib.humid_whitelist_correct(None, None, None, 0, None, None, None) == -1
    assert lib.humid_whitelist_correct_device(None, None, None, 0, None, None, None) == -1
    assert lib.humid_dedup_run_keyed_corrected(None, None, None, None, 0, 24, 1, 0, None, None, None) == -1
    assert lib.humid_dedup_run_keyed_corrected_device(None, None, None, None, 0, 24, 1, 0, None, None, None) == -1
    assert lib.humid_get_barcode_status(None, None, 0, None) == -1


def test_python_checks_its_arguments_before_the_library():
    """shape / dtype errors raise ValueError before the library is called: an object without a context is enough"""
    d = object.__new__(humid_amd.Dedup)
    k = np.arange(10, dtype=U64)
    f = np.zeros(10, np.uint8)
    for barcodes, nt in ((k.reshape(5, 2), 16), (k.astype(np.float64), 16), (np.arange(10) - 3, 16), (k, 0), (k, 33),
                         (k, 1), (np.asarray([1 << 32], U64), 16), ("ACGT", 4)):
        with pytest.raises(ValueError):
            d.set_whitelist(barcodes, nt)
    for keys, filt in ((k[:9], f), (k.reshape(5, 2), f), (k.astype(np.float32), f), (np.arange(10) - 3, f),
                       (k, f.reshape(5, 2))):
        with pytest.raises(ValueError):
            d.correct_keys(keys, filt)
    with pytest.raises(ValueError):
        d.run_keyed(np.zeros(10, U64), k[:9], f, word_nt=24, correct=True)


def write_whitelist(path, lines):
    with open(path, "w") as fh:
        fh.write("".join(l + "\n" for l in lines))
    return str(path)


@pytest.mark.parametrize("case", ["no_b", "unreadable", "short_line", "long_line", "bad_letter", "gz_name", "no_barcode",
                                  "no_value"])
def test_cli_refuses_bad_whitelists(case, tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=40)
    good = ["ACGTACGT", "ttgcaagg-1", "# a comment", "", "GGGGCCCC\r"]
    args = ["-n", "28", "-b", "8"]
    if case == "no_b":
        args = ["-n", "28", "-w", write_whitelist(tmp_path / "wl.txt", good)]
    elif case == "unreadable":
        args += ["-w", str(tmp_path / "absent.txt")]
    elif case == "short_line":
        args += ["-w", write_whitelist(tmp_path / "wl.txt", good + ["ACGTACG"])]
    elif case == "long_line":
        args += ["-w", write_whitelist(tmp_path / "wl.txt", good + ["ACGTACGTA"])]
    elif case == "bad_letter":
        args += ["-w", write_whitelist(tmp_path / "wl.txt", good + ["ACGTNCGT"])]
    elif case == "gz_name":
        args += ["-w", write_whitelist(tmp_path / "wl.txt.gz", good)]
    elif case == "no_barcode":
        args += ["-w", write_whitelist(tmp_path / "wl.txt", ["# nothing", "", "   "])]
    else:
        args, files = ["-n", "28", "-b", "8", "-w"], []
    r = subprocess.run([HUMID, "-d", str(tmp_path / "out"), "-l", "/dev/null"] + files + args, capture_output=True,
                       timeout=60)
    assert r.returncode == 2, r.stderr
    assert b"-w" in r.stderr
    assert not os.path.exists(tmp_path / "out")


def test_cli_reads_a_good_whitelist_before_the_device(tmp_path):
    """a well-formed whitelist passes the checks: --dump-words (which never opens a device) then ends with status 0"""
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=40)
    wl = write_whitelist(tmp_path / "wl.txt", ["ACGTACGT", "ttgcaagg-1", "# a comment", "", "GGGGCCCC\r", "AAAAAAAA  "])
    r = subprocess.run([HUMID, "-n", "28", "-b", "8", "-w", wl, "-l", "/dev/null", "--dump-words", str(tmp_path / "w.bin")]
                       + files, capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr


def test_usage_names_the_flag():
    r = subprocess.run([HUMID, "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0
    assert b"-w" in r.stderr and b"whitelist" in r.stderr and b"barcodes.dat" in r.stderr
