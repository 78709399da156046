"""CPU checks of the barcode correction by quality and abundance (include/humid_hip.h,
humid_whitelist_correct_posterior) and of `humid -b K -w FILE --barcode-posterior`: the two truths of
tests/whitelist_posterior_truth.py against each other, the weight table against its formula, the invariants the
header states, the odds boundary by hand, the exported symbols, the argument checks that need no device, and the
command line's refusals and --dump-barcode-quals (before any device is opened)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib

from cli_util import HUMID, ROOT
import whitelist_posterior_truth as pt
import whitelist_truth as wt

U64 = np.uint64
NEW_SYMBOLS = ("humid_whitelist_correct_posterior", "humid_whitelist_correct_posterior_device",
               "humid_dedup_run_keyed_posterior", "humid_dedup_run_keyed_posterior_device", "humid_get_barcode_posterior",
               "humid_whitelist_counts")


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


@pytest.mark.parametrize("k", [1, 2, 3, 8, 16, 21, 22, 32])
def test_the_two_truths_agree(k):
    rng = np.random.default_rng(100 + k)
    for n_wl, min_odds in ((2, 39), (7, 1), (60, 39), (60, 3)):
        wl, keys, quals, filt = pt.make_case(rng, 300, k, n_wl=n_wl)
        a = pt.posterior(keys, quals, filt, wl, k, min_odds)
        b = pt.posterior_all_pairs(keys, quals, filt, wl, k, min_odds)
        assert same(a, b) and same(a, pt.posterior_np(keys, quals, filt, wl, k, min_odds))
        out, status, sm, n_w = a
        assert sum(sm["counts"]) == len(keys) and sm["counts"][0] == int(filt.sum())
        assert np.all(out[filt == 1] == 0) and np.all(status[filt == 1] == 0)
        assert np.array_equal((out != keys) & (filt == 0), status == pt.CORRECTED)
        assert sm["rescued"] <= sm["multi"] and sum(n_w.values()) == sm["counts"][pt.EXACT]


def test_generator_reaches_every_status_and_both_outcomes():
    rng = np.random.default_rng(6)
    for k in (3, 16, 22, 32):
        wl, keys, quals, filt = pt.make_case(rng, 3000, k, n_wl=5 if k == 3 else 200)
        _, status, sm, _ = pt.posterior(keys, quals, filt, wl, k)
        assert wt.status_set(status) == {0, 1, 2, 3, 4}, k
        assert 0 < sm["rescued"] < sm["multi"], (k, sm)


def test_weight_table_is_the_formula():
    assert len(pt.E) == 41
    for q in range(41):
        assert pt.E[q] == pt.E_formula(q), q
        x = 2.0 ** 24 * 10.0 ** (-q / 10.0)
        assert pt.E[q] == math.floor(x + 0.5)
        assert abs((x + 0.5) - round(x + 0.5)) > 0.004, q      # far from a rounding boundary: no maths library disagrees
    # the header and the kernel file carry the same literal table
    for path in ("include/humid_hip.h", "humid_amd/csrc/kernels_wlpost.hip.h"):
        text = open(os.path.join(ROOT, path)).read()
        at = text.index("16777216")
        nums = [int(x) for x in re.findall(r"\d+", text[at:at + 700])][:41]
        assert nums == pt.E, path


def test_weights_stay_inside_64_bits():
    assert max(pt.E) == 1 << 24
    # at most 2^31 - 1 reads, one of them the query: n_w + 1 <= 2^31 - 1
    assert ((1 << 31) - 1) * max(pt.E) < 1 << 55 and 96 * ((1 << 31) - 1) * max(pt.E) < 1 << 62


def test_quality_difference_of_16_corrects_and_15_does_not():
    for q in range(0, 25):
        assert pt.E[q] >= 39 * pt.E[q + 16], q
    for q in range(0, 26):
        assert pt.E[q] < 39 * pt.E[q + 15], q


@pytest.mark.parametrize("case", pt.hand_cases(), ids=lambda c: c["name"])
def test_hand_cases(case):
    for truth in (pt.posterior, pt.posterior_all_pairs):
        out, status, sm, n_w = truth(case["keys"], case["quals"], case["filtered"], case["whitelist"], case["k"], case["min_odds"])
        assert int(status[-1]) == case["status"] and int(out[-1]) == case["key_out"]
        assert np.all(status[:-1] == pt.EXACT) and sm["multi"] == 1 and sm["rescued"] == (case["status"] == pt.CORRECTED)
        assert sum(n_w.values()) == len(status) - 1


def test_bits_above_2k_and_exact_beside_a_neighbour():
    AA, AC, AG = pt.key_of("AA"), pt.key_of("AC"), pt.key_of("AG")
    keys = np.asarray([AA | 16, AG | 16, AC, AG], U64)
    q = np.full((4, 2), 70, np.uint8)
    for truth in (pt.posterior, pt.posterior_all_pairs):
        out, status, sm, n_w = truth(keys, q, np.zeros(4, np.uint8), [AA, AC], 2)
        # AG has AA and AC one substitution away, both at nucleotide 1; AC holds one exact read: 2 : 1
        assert list(status) == [4, 4, 1, 3] and list(out) == [AA | 16, AG | 16, AC, AG]
        assert n_w == {AC: 1} and sm == dict(counts=[0, 1, 0, 1, 2], multi=1, rescued=0)
        out, status, sm, _ = truth(keys, q, np.zeros(4, np.uint8), [AA, AC], 2, min_odds=2)
        assert list(status) == [4, 4, 1, 2] and int(out[3]) == AC and sm["rescued"] == 1


@pytest.mark.parametrize("k,n_wl", [(3, 6), (16, 120), (22, 120)])         # (4^3 = 64 keys: a small whitelist leaves room)
def test_invariants_of_the_definition(k, n_wl):
    rng = np.random.default_rng(200 + k)
    wl, keys, quals, filt = pt.make_case(rng, 1500, k, n_wl=n_wl)
    plain_out, plain_st, _ = wt.correct(keys, filt, wl, k)
    out, status, sm, n_w = pt.posterior(keys, quals, filt, wl, k)
    # a read with one candidate is corrected exactly as the plain correction does
    one = plain_st == wt.CORRECTED
    assert one.any() and np.array_equal(out[one], plain_out[one]) and np.all(status[one] == pt.CORRECTED)
    # the statuses differ only on reads that are ambiguous there, and there only towards CORRECTED
    assert pt.plain_from_posterior(plain_st, status)
    differ = plain_st != status
    assert differ.any() and np.all(status[differ] == pt.CORRECTED)
    assert sm["multi"] == int((plain_st == wt.AMBIGUOUS).sum()) and sm["rescued"] == int(differ.sum())
    # equal quality bytes, no exact read, min_odds >= 2: the plain correction bit for bit
    W = set(int(w) for w in wl)
    f2 = filt.copy()
    f2[[int(x) in W for x in keys]] = 1
    flat = np.full_like(quals, 60)
    for min_odds in (2, 39):
        o2, s2, sm2, n2 = pt.posterior(keys, flat, f2, wl, k, min_odds)
        p_out, p_st, p_counts = wt.correct(keys, f2, wl, k)
        assert np.array_equal(o2, p_out) and np.array_equal(s2, p_st) and sm2["counts"] == [int(c) for c in p_counts]
        assert n2 == {} and sm2["rescued"] == 0
    # no order of the reads matters
    perm = rng.permutation(len(keys))
    o3, s3, sm3, n3 = pt.posterior(keys[perm], quals[perm], filt[perm], wl, k)
    assert np.array_equal(o3, out[perm]) and np.array_equal(s3, status[perm]) and sm3 == sm and n3 == n_w


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "humid_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint %s\(humid_ctx \*ctx" % name, hdr), name
    assert "typedef struct humid_bc_posterior_summary" in hdr
    assert lib.humid_abi_version() == 5
    import ctypes as C
    assert C.sizeof(_lib.HumidBcPosteriorSummary) == 56


def test_null_context_is_refused():
    lib = _lib.load()
    assert lib.humid_whitelist_correct_posterior(None, None, None, None, 0, 39, None, None, None) == -1
    assert lib.humid_whitelist_correct_posterior_device(None, None, None, None, 0, 39, None, None, None) == -1
    assert lib.humid_dedup_run_keyed_posterior(None, None, None, None, None, 0, 24, 1, 0, 39, None, None, None) == -1
    assert lib.humid_dedup_run_keyed_posterior_device(None, None, None, None, None, 0, 24, 1, 0, 39, None, None, None) == -1
    assert lib.humid_get_barcode_posterior(None, None, None) == -1
    assert lib.humid_whitelist_counts(None, None, 0, None) == -1


def test_python_checks_its_arguments_before_the_library():
    """shape / dtype / range errors raise ValueError before the library is called: an object without a context is enough"""
    d = object.__new__(humid_amd.Dedup)
    k = np.arange(10, dtype=U64)
    f = np.zeros(10, np.uint8)
    good = np.full((10, 16), 70, np.uint8)
    for quals in (good[:9], good.astype(np.int8), good.reshape(-1), good.astype(np.float32)):
        with pytest.raises(ValueError):
            d.correct_keys(k, f, quals=quals)
        with pytest.raises(ValueError):
            d.run_keyed(np.zeros(10, U64), k, f, word_nt=24, correct=True, barcode_quals=quals)
    for min_odds in (0, -1, 1 << 32):
        with pytest.raises(ValueError):
            d.correct_keys(k, f, quals=good, min_odds=min_odds)
        with pytest.raises(ValueError):
            d.run_keyed(np.zeros(10, U64), k, f, word_nt=24, correct=True, barcode_quals=good, min_odds=min_odds)
        with pytest.raises(ValueError):
            d.run_keyed_posterior_device(0, 0, 0, 0, 0, 0, 0, min_odds=min_odds)
    with pytest.raises(ValueError):
        d.run_keyed(np.zeros(10, U64), k, f, word_nt=24, correct=False, barcode_quals=good)
    for barcodes in (k.reshape(5, 2), k.astype(np.float64), np.arange(10) - 3):
        with pytest.raises(ValueError):
            d.whitelist_counts(barcodes)


# ---- the command line ---------------------------------------------------------------------------------------------
def write_fastq(path, rows, header_umi=False):
    """rows: (sequence, quality) per record"""
    with open(path, "w") as fh:
        for i, (seq, q) in enumerate(rows):
            fh.write("@r%d%s\n%s\n+\n%s\n" % (i, "_ACGTACGT" if header_umi else "", seq, q))
    return str(path)


def tiny_rows(rng, n=12, length=30):
    rows = []
    for i in range(n):
        ln = 5 if i == 3 else length                                 # one read shorter than the barcode
        rows.append(("".join("ACGT"[x] for x in rng.integers(0, 4, size=ln)),
                     "".join(chr(x) for x in rng.integers(35, 75, size=ln))))
    return rows


def write_whitelist(path):
    with open(path, "w") as fh:
        fh.write("ACGTACGT\nGGGGCCCC\n")
    return str(path)


@pytest.mark.parametrize("case", ["no_w", "no_b_dump", "header_umi", "short_take", "odds_0", "odds_word", "odds_missing"])
def test_cli_refuses(case, tmp_path):
    rng = np.random.default_rng(3)
    r1 = write_fastq(tmp_path / "r1.fastq", tiny_rows(rng), header_umi=case == "header_umi")
    wl = write_whitelist(tmp_path / "wl.txt")
    args, files, word = ["-n", "20", "-b", "8", "-w", wl, "--barcode-posterior"], [r1], b"--barcode-posterior"
    if case == "no_w":
        args = ["-n", "20", "-b", "8", "--barcode-posterior"]
    elif case == "no_b_dump":
        args, word = ["-n", "20", "--dump-barcode-quals", str(tmp_path / "q.bin")], b"--dump-barcode-quals"
    elif case == "header_umi":
        word = b"UMI"
    elif case == "short_take":                                        # two files share the 10 nucleotides: 5 < 8 from the first
        files, args, word = [r1, write_fastq(tmp_path / "r2.fastq", tiny_rows(rng))], ["-n", "10", "-b", "8", "-w", wl,
                                                                                        "--barcode-posterior"], b"fewer than"
    elif case == "odds_0":
        args, word = args + ["--barcode-min-odds", "0"], b"--barcode-min-odds"
    elif case == "odds_word":
        args, word = args + ["--barcode-min-odds", "many"], b"--barcode-min-odds"
    else:
        args, files, word = args + ["--barcode-min-odds"], [], b"--barcode-min-odds"
    r = subprocess.run([HUMID, "-d", str(tmp_path / "out"), "-l", "/dev/null"] + files + args, capture_output=True, timeout=60)
    assert r.returncode == 2, r.stderr
    assert word in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out") and not os.path.exists(tmp_path / "q.bin")


@pytest.mark.parametrize("slow", [False, True])
def test_cli_dumps_the_barcode_qualities(slow, tmp_path):
    """the first K letters of the first file's quality line per record, '!' behind the end of a shorter line; never
    opens a device.  Both input paths (mapped files, streaming reader)."""
    rng = np.random.default_rng(4)
    rows = tiny_rows(rng)
    r1 = write_fastq(tmp_path / "r1.fastq", rows)
    r2 = write_fastq(tmp_path / "r2.fastq", tiny_rows(rng))
    env = dict(os.environ)
    if slow:
        env["HUMID_HOST_SLOW"] = "1"
    for files, n in (([r1], "20"), ([r1, r2], "24")):                 # (24 over two files: 12 >= 8 from the first)
        dump = str(tmp_path / "q.bin")
        r = subprocess.run([HUMID, "-n", n, "-b", "8", "-l", "/dev/null", "--dump-barcode-quals", dump] + files,
                           capture_output=True, timeout=60, env=env)
        assert r.returncode == 0, r.stderr
        raw = open(dump, "rb").read()
        assert int(np.frombuffer(raw[:8], U64)[0]) == len(rows) and len(raw) == 8 + 8 * len(rows)
        got = np.frombuffer(raw[8:], np.uint8).reshape(len(rows), 8)
        want = np.asarray([[ord(c) for c in (q[:8] + "!" * 8)[:8]] for _, q in rows], np.uint8)
        assert np.array_equal(got, want)
        assert np.all(got[3, 5:] == ord("!")) and np.all(got[3, :5] != ord("!"))


def test_usage_names_the_flags():
    r = subprocess.run([HUMID, "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0
    assert b"--barcode-posterior" in r.stderr and b"--barcode-min-odds" in r.stderr and b"rescued" in r.stderr
