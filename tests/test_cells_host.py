"""CPU checks of the whitelist taken from the data (include/humid_hip.h, humid_whitelist_discover) and of
`humid -b K --cells-*`: the two forms of the truth's merge against each other, the generator's planted cells recovered
by the definition, the new symbols in the binding, the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib

from cli_util import HUMID
import cells_truth as ct

U64 = np.uint64
NEW_SYMBOLS = ("humid_whitelist_discover", "humid_whitelist_discover_device", "humid_get_discovered_cells",
               "humid_get_barcode_count_hist")


def same(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3][0], b[3][0])
            and np.array_equal(a[3][1], b[3][1]))


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16, 32])
def test_the_two_truths_agree(k):
    """small alphabets make every selected barcode a neighbour of many others; ratios 1 .. 5; every mode"""
    rng = np.random.default_rng(300 + k)
    merged = 0
    for trial in range(6):
        if k <= 3:
            keys = rng.integers(0, 4 ** k, size=400).astype(U64)
            keys = np.where(rng.random(400) < 0.5, keys[0], keys)     # one heavy barcode
            filt = (rng.random(400) < 0.1).astype(np.uint8)
        else:
            keys, filt, _ = ct.planted(rng, k, 12, 20, 1.3, 0.2, 30)
        for mode, param in ((ct.TOP, 7), (ct.TOP, 10 ** 6), (ct.EXPECTED, 10), (ct.MIN_READS, 2)):
            for ratio in (1, 2, 5):
                a = ct.discover(keys, filt, k, mode, param, ratio)
                b = ct.discover(keys, filt, k, mode, param, ratio, all_pairs=True)
                assert same(a, b), (k, trial, mode, param, ratio)
                merged += a[2]["merged"]
                assert a[2]["cells"] + a[2]["merged"] == a[2]["selected"] <= a[2]["distinct"]
    assert merged > 0


def test_hand_cases_of_the_definition():
    enc = lambda s: sum("ACGT".index(ch) << (2 * (len(s) - 1 - i)) for i, ch in enumerate(s))    # noqa: E731
    a, b, c = enc("AAAA"), enc("AAAC"), enc("AACC")                   # a chain: a-b and b-c are one apart, a-c two
    keys, filt = ct.from_counts([(a, 1000), (b, 100), (c, 10)])
    cells, reads, sm, hist = ct.discover(keys, filt, 4, ct.TOP, 3, 5)
    assert list(cells) == [a] and list(reads) == [1000] and sm["merged"] == 2      # b is removed and still removes c
    assert [list(h) for h in hist] == [[10, 100, 1000], [1, 1, 1]]
    cells, _, sm, _ = ct.discover(keys, filt, 4, ct.TOP, 3, 0)
    assert list(cells) == [a, b, c] and sm["threshold_reads"] == 10 and sm["top_reads"] == 1000
    # equal counts, R = 1: only the larger value goes; TOP cuts a tie towards the smaller value
    keys, filt = ct.from_counts([(b, 5), (a, 5), (c, 5)])
    assert list(ct.discover(keys, filt, 4, ct.TOP, 3, 1)[0]) == [a]   # (b goes to a; c goes to b)
    assert list(ct.discover(keys, filt, 4, ct.TOP, 2, 0)[0]) == [a, b]
    # EXPECTED: b = (X + 50) // 100 capped at G - 1; 10 n >= m
    keys, filt = ct.from_counts([(enc("CAAA"), 100), (enc("GAAA"), 10), (enc("TAAA"), 9), (enc("ACCA"), 1)])
    assert ct.discover(keys, filt, 4, ct.EXPECTED, 1, 0)[2]["selected"] == 2       # b = 0, m = 100: 10 and up
    assert ct.discover(keys, filt, 4, ct.EXPECTED, 10 ** 9, 0)[2]["selected"] == 4  # b = G - 1, m = 1
    # an invalid key takes no part
    keys, filt = ct.from_counts([(enc("CAAA"), 3), (256, 7)])
    sm = ct.discover(keys, filt, 4, ct.MIN_READS, 1, 0)[2]
    assert (sm["usable"], sm["invalid_reads"], sm["distinct"], sm["cells"], sm["top_reads"]) == (10, 7, 1, 1, 3)


def test_planted_cells_come_back():
    """200 cells of 200 reads and more, 1 % of the reads one substitution off, 20 000 ambient barcodes of 1 .. 3 reads"""
    rng = np.random.default_rng(17)
    keys, filt, cells = ct.planted(rng, 16, 200, 200, 1.01, 0.01, 20_000)
    want = np.asarray(sorted(cells), U64)
    got, reads, sm, _ = ct.discover(keys, filt, 16, ct.EXPECTED, 200, 5)
    assert np.array_equal(got, want) and sm["distinct"] > 20_000 and int(reads.min()) >= 150
    got0, _, sm0, _ = ct.discover(keys, filt, 16, ct.EXPECTED, 200, 0)
    assert set(want) <= set(got0) and sm0["merged"] == 0
    near = set(w ^ (x << (2 * i)) for w in cells for i in range(16) for x in (1, 2, 3))
    assert set(int(x) for x in got0) - set(cells) <= near
    # every read counted: nothing but the merge separates the two
    assert sm0["cells"] == sm["cells"] + sm["merged"]
    # with a threshold low enough to let error barcodes in, the merge takes exactly those next to a cell out again
    low, _, sml, _ = ct.discover(keys, filt, 16, ct.MIN_READS, 2, 5)
    assert sml["merged"] > 0 and set(want) <= set(low)
    assert not (set(int(x) for x in low) - set(cells)) & near


def test_binding_lists_the_new_symbols():
    for n in NEW_SYMBOLS:
        assert n in _lib.SYMBOLS, n
    assert (humid_amd.CELLS_TOP, humid_amd.CELLS_EXPECTED, humid_amd.CELLS_MIN_READS) == (0, 1, 2)
    assert [f for f, _ in _lib.HumidCellsSummary._fields_] == list(ct.FIELDS)


def tiny_fastq(path):
    rng = np.random.default_rng(5)
    with open(path, "w") as fh:
        for i in range(8):
            seq = "".join("ACGT"[x] for x in rng.integers(0, 4, size=30))
            fh.write("@r%d\n%s\n+\n%s\n" % (i, seq, "I" * 30))
    return str(path)


@pytest.mark.parametrize("case,args,word", [
    ("two_modes", ["-b", "8", "--cells-top", "5", "--cells-expected", "5"], b"exclude each other"),
    ("two_modes_same", ["-b", "8", "--cells-min-reads", "5", "--cells-min-reads", "6"], b"exclude each other"),
    ("no_b", ["--cells-expected", "5"], b"need -b K"),
    ("with_w", ["-b", "8", "-w", "WL", "--cells-min-reads", "2"], b"do not work with -w"),
    ("with_P", ["-P", "--cells-top", "5"], b"do not work with -P"),
    ("with_g", ["-b", "8", "-g", "2", "--cells-top", "5"], b"run on one GPU"),
    ("sharded_env", ["-b", "8", "--cells-top", "5"], b"run on one GPU"),
    ("ratio_alone", ["-b", "8", "--cells-merge-ratio", "5"], b"--cells-merge-ratio needs"),
    ("zero", ["-b", "8", "--cells-top", "0"], b"--cells-top takes a number of 1 or more"),
    ("not_a_number", ["-b", "8", "--cells-expected", "many"], b"--cells-expected takes a number of 1 or more"),
    ("bad_ratio", ["-b", "8", "--cells-top", "5", "--cells-merge-ratio", "-1"], b"--cells-merge-ratio takes a ratio"),
])
def test_cli_refuses(case, args, word, tmp_path):
    """by message: an unknown flag exits 2 as well.  Nothing is written and no device is opened."""
    r1 = tiny_fastq(tmp_path / "r1.fastq")
    wl = tmp_path / "wl.txt"
    wl.write_text("ACGTACGT\n")
    args = [str(wl) if a == "WL" else a for a in args]
    files = [r1, tiny_fastq(tmp_path / "r2.fastq")] if case == "with_P" else [r1]
    env = dict(os.environ)
    env.pop("HUMID_GPUS", None)
    env.pop("HUMID_FORCE_SHARDED", None)
    if case == "sharded_env":
        env["HUMID_FORCE_SHARDED"] = "1"
    r = subprocess.run([HUMID, "-n", "20", "-d", str(tmp_path / "out"), "-l", "/dev/null"] + files + args, capture_output=True,
                       timeout=60, env=env)
    assert r.returncode == 2, r.stderr
    assert b"humid: " in r.stderr and word in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out")


def test_posterior_without_a_whitelist_is_refused_as_before(tmp_path):
    r1 = tiny_fastq(tmp_path / "r1.fastq")
    r = subprocess.run([HUMID, "-n", "20", "-b", "8", "--barcode-posterior", "-l", "/dev/null", r1], capture_output=True, timeout=60)
    assert r.returncode == 2
    assert b"humid: --barcode-posterior needs -w FILE (it decides between the listed barcodes near a read's barcode)\n" in r.stderr


def test_usage_names_the_flags():
    r = subprocess.run([HUMID, "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0
    for word in (b"--cells-top", b"--cells-expected", b"--cells-min-reads", b"--cells-merge-ratio", b"cells.dat", b"barcode_rank.dat"):
        assert word in r.stderr, word
