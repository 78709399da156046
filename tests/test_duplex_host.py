"""No GPU: the two truths of tests/duplex_truth.py against each other on random inputs, one hand-built column per row
of the decision table of humid_duplex_consensus (include/humid_hip.h) with the per-strand cap, the reduction to the
plain consensus for single-class clusters, invariance under flipping every strand, a planted strand-specific error, the
new symbols of the C ABI, the command line's refusals around -D, and what -P -D hands to the GPU
(--dump-consensus-input: the two layers, then one strand byte per read)."""
import os
import subprocess

import numpy as np
import pytest

import consensus_truth as ct
import duplex_truth as dt
import paired_truth as pt
from cli_util import HUMID, expected_words, read_fastq
from humid_amd import _lib, build


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


LENGTHS = np.asarray([0, 1, 63, 64, 65, 151])


def both(ls, lo, cid, keep, strand, C, **kw):
    a = dt.duplex_loop(ls, lo, cid, keep, strand, C, **kw)
    dt.assert_same(a, dt.duplex_numpy(ls, lo, cid, keep, strand, C, **kw), "the two truths")
    return a


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_two_truths_agree_on_random_inputs(seed):
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 2, 7, 20, 1, 40, 3]
    tops = [1, 1, 2, 3, 0, 0, 25, 1]
    cid, keep, strand = dt.sized_clusters(rng, sizes, tops, n_zero=5, shuffle=seed != 1)
    strand[cid == 0] = rng.integers(0, 256, int((cid == 0).sum()))      # not read
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS, len(cid)), rng.choice(LENGTHS, len(cid)),
                             p_err=0.15, odd_quals=True)
    for kw in (dict(), dict(min_q=0, strand_cap_q=93, cap_q=93), dict(min_q=20, strand_cap_q=1, cap_q=1),
               dict(min_q=93, strand_cap_q=40, cap_q=50)):
        a = both(l1, l2, cid, keep, strand, len(sizes), **kw)
        b = both(l2, l1, cid, keep, strand, len(sizes), **kw)           # the second call of the pair
        assert list(a["depth"]) == sizes and list(b["depth"]) == sizes
        assert np.array_equal(a["depth_same"], b["depth_same"])
    sm = both(l1, l2, cid, keep, strand, len(sizes))["summary"]
    assert sm["duplex_clusters"] == 4 and sm["both_called"] > sm["disagree"] > 0 and sm["agree"] > 0


def one(xs, ys, **kw):
    """one cluster: the records xs of class X (the first is the representative) vote in layer S, the records ys of
    class Y in layer O; what the other layer holds for them is never read.  Returns (bases, quals, summary, dict)"""
    n = len(xs) + len(ys)
    junk = [(b"", b"")] * len(xs)
    ls = ct.flat([r[0] for r in xs] + [b"TTTTTTTT"[:len(xs[0][0])] for _ in ys], [r[1] for r in xs] + [b"~~~~~~~~"[:len(xs[0][0])] for _ in ys])
    lo = ct.flat([j[0] for j in junk] + [r[0] for r in ys], [j[1] for j in junk] + [r[1] for r in ys])
    cid = np.ones(n, np.uint32)
    keep = np.zeros(n, np.uint8)
    keep[0] = 1
    strand = np.asarray([dt.BOTTOM] * len(xs) + [dt.TOP] * len(ys), np.uint8)
    t = both(ls, lo, cid, keep, strand, 1, **kw)
    return bytes(t["bases"]), bytes(t["quals"]), t["summary"], t


def q(p):
    return bytes([33 + p])


def test_one_column_per_row_of_the_table():
    # no vote in either class: the representative's own bytes, verbatim (N, lowercase, a quality below min_q)
    assert one([(b"Na", b"I#")], [(b"cA", b"I#")])[:2] == (b"Na", b"I#")
    # both call the same base: the margins add
    b, ql, sm, _ = one([(b"A", q(30))], [(b"A", q(20))])
    assert (b, ql) == (b"A", q(50)) and (sm["both_called"], sm["agree"], sm["disagree"], sm["masked"]) == (1, 1, 0, 0)
    assert one([(b"A", q(30))], [(b"A", q(20))], cap_q=45)[:2] == (b"A", q(45))
    assert one([(b"A", q(60))], [(b"A", q(50))], strand_cap_q=40)[:2] == (b"A", q(80))      # each capped, then added
    assert one([(b"A", q(60))], [(b"A", q(50))], strand_cap_q=93)[:2] == (b"A", q(93))      # 110, capped by cap_q
    # both call, bases differ, margins differ: the larger margin wins with the difference
    b, ql, sm, t = one([(b"A", q(30))], [(b"C", q(20))])
    assert (b, ql) == (b"A", q(10)) and (sm["both_called"], sm["agree"], sm["disagree"], sm["masked"]) == (1, 0, 1, 0)
    assert list(t["disagree"]) == [1] and sm["errors"] == 0 and sm["bases_changed"] == 0
    b, ql, sm, _ = one([(b"A", q(20))], [(b"C", q(30))])
    assert (b, ql) == (b"C", q(10)) and sm["bases_changed"] == 1
    # ... margins equal: N and !
    b, ql, sm, t = one([(b"A", q(30))], [(b"C", q(30))])
    assert (b, ql) == (b"N", b"!") and (sm["both_called"], sm["disagree"], sm["masked"]) == (1, 1, 1) and list(t["disagree"]) == [1]
    # exactly one class calls
    b, ql, sm, _ = one([(b"A", q(30))], [(b"N", q(40))])
    assert (b, ql) == (b"A", q(30)) and sm["both_called"] == 0 and sm["duplex_clusters"] == 1 and sm["votes"] == 1
    assert one([(b"n", q(30))], [(b"C", q(20))])[:2] == (b"C", q(20))
    assert one([(b"A", q(30))], [(b"C", q(5))])[:2] == (b"A", q(30))                         # below min_q: no vote
    assert one([(b"A", q(60))], [], strand_cap_q=40)[:2] == (b"A", q(40))                    # the strand cap on one class
    # a tie inside a class is no call: the other class decides alone
    b, ql, sm, _ = one([(b"A", q(30)), (b"C", q(30))], [(b"G", q(12))])
    assert (b, ql) == (b"G", q(12)) and sm["errors"] == 0 and sm["votes"] == 3
    # votes were cast, neither class calls
    b, ql, sm, _ = one([(b"A", q(30)), (b"C", q(30))], [(b"N", q(12))])
    assert (b, ql) == (b"N", b"!") and sm["masked"] == 1 and sm["both_called"] == 0
    # errors: per calling class its votes minus those for its called base
    b, ql, sm, _ = one([(b"A", q(30)), (b"A", q(30)), (b"C", q(10))], [(b"A", q(20)), (b"G", q(11))])
    assert (b, ql) == (b"A", q(40 + 9)) and sm["errors"] == 2 and sm["votes"] == 5
    # a shorter voting record stops voting; a longer one is cut to the representative's length
    b, ql, sm, _ = one([(b"AC", q(30) * 2)], [(b"A", q(20))])
    assert (b, ql) == (b"AC", q(50) + q(30))
    b, ql, sm, _ = one([(b"A", q(30))], [(b"ACGT", q(20) * 4)])
    assert (b, ql) == (b"A", q(50)) and sm["total_bytes"] == 1 and sm["votes"] == 2


def test_the_cap_keeps_a_deep_strand_from_outvoting_a_shallow_one():
    xs, ys = [(b"A", q(40))] * 50, [(b"C", q(40))] * 2
    assert one(xs, ys, strand_cap_q=40)[:2] == (b"N", b"!")               # 40 against 40
    assert one(xs, ys, strand_cap_q=93)[:2] == (b"A", q(93 - 80))         # min(2000, 93) - 80
    # the pooled consensus of the same 52 votes sees no conflict at all
    pb, pq, poff = ct.flat([r[0] for r in xs + ys], [r[1] for r in xs + ys])
    keep = np.zeros(52, np.uint8)
    keep[0] = 1
    p = ct.consensus_loop(pb, pq, poff, np.ones(52, np.uint32), keep, 1)
    assert (bytes(p["bases"]), bytes(p["quals"])) == (b"A", q(93))


def test_single_class_clusters_reduce_to_the_plain_consensus():
    rng = np.random.default_rng(5)
    sizes = [1, 2, 9, 30, 1, 4]
    tops = [1, 0, 9, 0, 0, 4]                                            # every cluster of one strand
    cid, keep, strand = dt.sized_clusters(rng, sizes, tops, n_zero=4)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS, len(cid)), rng.choice(LENGTHS, len(cid)),
                             p_err=0.2, odd_quals=True)
    garbage = (rng.integers(0, 256, len(l2[0])).astype(np.uint8), rng.integers(0, 256, len(l2[1])).astype(np.uint8), l2[2])
    for min_q, cap_q in ((10, 93), (0, 30), (50, 1)):
        d = both(l1, garbage, cid, keep, strand, len(sizes), min_q=min_q, strand_cap_q=93, cap_q=cap_q)
        p = ct.consensus_loop(l1[0], l1[1], l1[2], cid, keep, len(sizes), min_q, cap_q)
        ct.assert_same(p, d, "single class")                            # five arrays and the six shared summary fields
        assert d["summary"]["duplex_clusters"] == 0 and d["summary"]["both_called"] == 0
        assert np.array_equal(d["depth_same"], d["depth"]) and not d["depth_other"].any() and not d["disagree"].any()


def test_flipping_every_strand_changes_nothing():
    rng = np.random.default_rng(6)
    sizes, tops = [5, 12, 1, 8], [2, 12, 1, 3]
    cid, keep, strand = dt.sized_clusters(rng, sizes, tops, n_zero=3)
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, rng.choice(LENGTHS, len(cid)), rng.choice(LENGTHS, len(cid)), p_err=0.2)
    a = both(l1, l2, cid, keep, strand, 4)
    flipped = np.where(cid != 0, strand ^ 1, strand).astype(np.uint8)
    dt.assert_same(a, both(l1, l2, cid, keep, flipped, 4), "flipped")


def test_a_strand_specific_error_does_not_get_through():
    """12 reads of the other strand all carry the same wrong base at column 7, 3 reads of the representative's strand
    carry the right one: the pooled consensus of the oriented reads calls the error, the duplex consensus masks it at
    the default cap and calls the right base with a small quality when the cap lets the deep strand count for more"""
    rng = np.random.default_rng(7)
    cid, keep, strand = dt.sized_clusters(rng, [15], [3], rep_top=[True])
    n, L, col = 15, 20, 7
    l1, l2 = dt.duplex_reads(rng, cid, strand, keep, np.full(n, L), np.full(n, L), p_err=0, p_n=0, p_lower=0, q_lo=30, q_hi=30,
                             plant=("other", col))
    same = strand == dt.TOP
    right = l1[0].reshape(n, L)[np.flatnonzero(same)[0]]
    wrong = l2[0].reshape(n, L)[np.flatnonzero(~same)[0], col]
    assert wrong != right[col]
    # the oriented reads: every read's record that reads the representative's R1
    ob = np.where(same[:, None], l1[0].reshape(n, L), l2[0].reshape(n, L)).reshape(-1)
    oq = np.where(same[:, None], l1[1].reshape(n, L), l2[1].reshape(n, L)).reshape(-1)
    pooled = ct.consensus_loop(ob, oq, l1[2], cid, keep, 1)
    assert pooled["bases"][col] == wrong and pooled["quals"][col] == 33 + 93
    d = both(l1, l2, cid, keep, strand, 1)                              # 40 against 40
    assert d["bases"][col] == ord("N") and d["quals"][col] == ord("!") and d["summary"]["masked"] == 1
    assert np.array_equal(np.delete(d["bases"], col), np.delete(right, col)) and list(d["disagree"]) == [1]
    d = both(l1, l2, cid, keep, strand, 1, strand_cap_q=93)             # 90 against 93: the error wins by 3
    assert d["bases"][col] == wrong and d["quals"][col] == 33 + 3
    d = both(l1, l2, cid, keep, strand, 1, strand_cap_q=60)             # 60 against 60
    assert d["bases"][col] == ord("N")


def test_symbols_and_summary_layout():
    lib = _lib.load()
    for name in ("humid_duplex_consensus", "humid_duplex_consensus_device", "humid_get_duplex_consensus"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert tuple(k for k, _ in _lib.HumidDuplexSummary._fields_) == dt.KEYS
    assert dt.KEYS[:6] == ct.KEYS


def test_cli_refusals(tmp_path):
    files = pt.write_duplex_fastq(str(tmp_path / "in"), 4, 20)

    def refused(args, *words):
        p = subprocess.run([HUMID, "-d", str(tmp_path / "out"), "-l", "/dev/null"] + args, stderr=subprocess.PIPE, timeout=60)
        lines = p.stderr.decode().strip().split("\n")
        assert p.returncode != 0 and len(lines) == 1 and lines[0].startswith("humid: "), (args, p.returncode, lines)
        assert all(w in lines[0] for w in words), (args, lines[0])
        assert not os.path.exists(str(tmp_path / "out"))

    refused(["-D"] + files, "-D", "-P")                                 # -D without -P
    refused(["-D"] + files[:1], "-D", "-P")
    refused(["-C", "-D"] + files, "-C", "-D")                           # -C -D together
    refused(["-P", "-C"] + files, "-C", "-D")                           # -P -C stays refused and names -D
    refused(["-P", "-C", "-D"] + files, "-C", "-D")
    refused(["-P", "-D", "-g", "2"] + files, "one GPU")                 # several GPUs
    refused(["-P", "-D", "--duplex-strand-cap", "0"] + files, "--duplex-strand-cap")
    refused(["-P", "-D", "--duplex-strand-cap", "94"] + files, "--duplex-strand-cap")
    refused(["-P", "-D", "--consensus-min-q", "94"] + files, "--consensus-min-q")
    r = subprocess.run([HUMID, "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"-D" in r.stderr and b"--duplex-strand-cap" in r.stderr


@pytest.mark.parametrize("gz", [False, True])
def test_dump_consensus_input_under_p_d(gz, tmp_path):
    """the two layers as -C dumps them, then one strand byte per read: those of the canonical words, NONE for a filtered read"""
    n_nt = 24
    files = pt.write_duplex_fastq(str(tmp_path / "in"), 3, 600, n=n_nt, read_len=36, gz=gz)
    out = str(tmp_path / "cons.bin")
    subprocess.check_call([HUMID, "-P", "-D", "-n", str(n_nt), "-l", "/dev/null", "--dump-consensus-input", out] + files, timeout=120)
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], np.uint64)[0])
    assert n == 600
    at = 8
    for f in files:
        recs = read_fastq(f)
        b, ql, off = ct.flat([r[1].encode() for r in recs], [r[3].encode() for r in recs])
        got_off = np.frombuffer(raw[at:at + 8 * (n + 1)], np.uint64)
        at += 8 * (n + 1)
        t = int(got_off[n])
        assert np.array_equal(got_off, off)
        assert np.array_equal(np.frombuffer(raw[at:at + t], np.uint8), b) and np.array_equal(np.frombuffer(raw[at + t:at + 2 * t], np.uint8), ql)
        at += 2 * t
    strand = np.frombuffer(raw[at:], np.uint8)
    ew, ef, _, _ = expected_words(files, n_nt)
    _, es = pt.canonical(ew, ef, n_nt)
    assert len(strand) == n and np.array_equal(strand, es)
    assert (es == pt.NONE).sum() == ef.sum() > 0 and (es == pt.TOP).sum() > 100 and (es == pt.BOTTOM).sum() > 100
    # without -D the dump is what it was: no strand bytes
    subprocess.check_call([HUMID, "-n", str(n_nt), "-l", "/dev/null", "--dump-consensus-input", out] + files, timeout=120)
    assert open(out, "rb").read() == raw[:at]
