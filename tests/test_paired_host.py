"""Strand-symmetric (duplex) deduplication without a GPU: the truth of tests/paired_truth.py against itself and the
oracle, the hand-built case that canonicalising alone gets wrong, and the host side of `humid -P` (--dump-words stops
after pass 1; the refusals need no GPU either)."""
import os
import subprocess

import numpy as np
import pytest

import paired_truth as pt
from cli_util import HUMID, expected_words
from humid_amd import build
from oracle import pyoracle as orc


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


@pytest.mark.parametrize("n", [2, 8, 24, 32, 34, 64])
def test_mirror_and_canonical(n):
    rng = np.random.default_rng(n)
    vals = [pt.pack(rng.integers(0, 4, size=n)) for _ in range(200)]
    for v in vals[:50]:
        m = pt.mirror(v, n)
        assert pt.mirror(m, n) == v and m < (1 << (2 * n))
        seq = [(v >> (2 * (n - 1 - i))) & 3 for i in range(n)]
        assert m == pt.pack(seq[n // 2:] + seq[:n // 2])
        u = vals[0]
        assert pt.ham(pt.mirror(u, n), m) == pt.ham(u, v) and pt.ham(u, m) == pt.ham(pt.mirror(u, n), v)
    words = pt.from_ints(vals, n)
    filt = (rng.random(len(vals)) < 0.1).astype(np.uint8)
    cw, strand = pt.canonical(words, filt, n)
    assert np.array_equal(pt.to_ints(words, n), vals)
    for v, c, s, f in zip(vals, pt.to_ints(cw, n), strand, filt):
        if f:
            assert c == v and s == pt.NONE
        else:
            assert c == min(v, pt.mirror(v, n)) and s == (pt.TOP if c == v else pt.BOTTOM)


@pytest.mark.parametrize("n,d,method", [(8, 1, 0), (24, 1, 0), (24, 2, 1), (48, 1, 0), (64, 2, 1)])
def test_without_mirrors_the_truth_is_the_oracle_run(n, d, method):
    """words that start with AAA and whose second half starts with TTT are all top-strand reads, and the mirror of one
    differs from any other in those six places (asserted below): the paired truth is then the plain run"""
    rng = np.random.default_rng(10 * n + d)
    h = n // 2
    base = rng.integers(0, 4, size=(60, n))
    rows = base[rng.integers(0, 60, size=400)].copy()
    for r in rows:
        if rng.random() < 0.4:
            r[int(rng.integers(0, n))] = int(rng.integers(0, 4))
    rows[:, 0], rows[:, h] = 0, 3
    rows[:, 1], rows[:, h + 1] = 0, 3
    rows[:, 2 % h], rows[:, h + 2 % h] = 0, 3
    words = pt.from_ints([pt.pack(r) for r in rows], n)
    filt = (rng.random(len(rows)) < 0.05).astype(np.uint8)
    t = pt.run(words, filt, n, d, method)
    assert np.all(t["strand"][filt == 0] == pt.TOP)
    leaves = pt.to_ints(t["leaves"]["word"], n)
    assert min(pt.ham(u, pt.mirror(v, n)) for u in leaves[:80] for v in leaves[:80]) > d
    ocid, okeep, osum, _ = orc.dedup_run(words, filt, n, d, method)
    assert np.array_equal(t["cluster_id"], ocid) and np.array_equal(t["keep"], okeep)
    for k in ("total", "usable", "unique", "clusters", "edges"):
        assert t["summary"][k] == osum[k], k


@pytest.mark.parametrize("n,d,method", [(2, 1, 0), (8, 1, 1), (24, 1, 0), (24, 3, 0), (34, 2, 1), (64, 1, 0)])
def test_truth_of_the_mirrored_input(n, d, method):
    words, filt = pt.families(n + d, n, 500, d)
    t = pt.run(words, filt, n, d, method)
    m = pt.run(pt.mirror_words(words, n), filt, n, d, method)
    assert np.array_equal(t["cluster_id"], m["cluster_id"]) and np.array_equal(t["keep"], m["keep"])
    vals = pt.to_ints(words, n)
    pal = np.array([v == pt.mirror(v, n) for v in vals])
    usable = filt == 0
    assert np.array_equal(m["strand"][usable & ~pal], 1 - t["strand"][usable & ~pal])
    assert np.all(m["strand"][usable & pal] == pt.TOP) and np.all(t["strand"][usable & pal] == pt.TOP)
    assert np.array_equal(t["top"] + t["bottom"], m["top"] + m["bottom"])
    assert t["strands"]["duplex"] > 0 and t["strands"]["top_reads"] + t["strands"]["bottom_reads"] == int(usable.sum())
    c = pt.run(t["canonical"], filt, n, d, method)
    assert np.array_equal(t["cluster_id"], c["cluster_id"]) and np.array_equal(t["keep"], c["keep"])
    assert c["strands"]["bottom_reads"] == 0


@pytest.mark.parametrize("n", [2, 8, 24, 34, 64])
def test_orientation_flip_is_one_cluster_only_with_the_mirror_search(n):
    """a = A.B and b = B'.A, one error at the first nucleotide of B: ham(c(a), c(b)) > d, ham(a, m(b)) = 1"""
    a, b = pt.flip_pair(n)
    assert pt.ham(min(a, pt.mirror(a, n)), min(b, pt.mirror(b, n))) == n > 1 and pt.ham(a, pt.mirror(b, n)) == 1
    words, filt = pt.from_ints([a, b, a], n), np.zeros(3, np.uint8)
    t = pt.run(words, filt, n, 1)
    assert t["summary"]["clusters"] == 1 and t["summary"]["edges"] == 1
    assert t["keep"].tolist() == [1, 0, 0] and t["cluster_id"].tolist() == [1, 1, 1]
    cw, _ = pt.canonical(words, filt, n)
    ocid, okeep, osum, _ = orc.dedup_run(cw, filt, n, 1, 0)             # canonicalise, then the plain run
    assert osum["clusters"] == 2 and osum["edges"] == 0


def test_forced_cases_in_the_truth():
    n, d = 24, 1
    rng = np.random.default_rng(5)
    vals = pt.forced_reads(rng, n, d)
    t = pt.run(pt.from_ints(vals, n), np.zeros(len(vals), np.uint8), n, d)
    leaves = pt.to_ints(t["leaves"]["word"], n)
    off, idx = t["off"].astype(np.int64), t["idx"]
    for k in range(len(leaves)):
        row = idx[off[k]:off[k + 1]]
        assert k not in row and len(set(row.tolist())) == len(row)        # no self edge, every neighbour once
    pal = [k for k, v in enumerate(leaves) if v == pt.mirror(v, n)]
    assert len(pal) == 2
    both = [(k, j) for k in pal for j in idx[off[k]:off[k + 1]]
            if pt.ham(leaves[k], leaves[j]) <= d and pt.ham(leaves[k], pt.mirror(leaves[j], n)) <= d]
    assert both                                                          # a pair under both terms: listed once (above)


def dump_paired(files, n, tmp):
    out = os.path.join(tmp, "words.bin")
    subprocess.check_call([HUMID, "-P", "-n", str(n), "-l", os.path.join(tmp, "log.txt"), "--dump-words", out] + list(files))
    raw = open(out, "rb").read()
    N = int(np.frombuffer(raw[:8], np.uint64)[0])
    wpr = 2 if n > 32 else 1
    words = np.frombuffer(raw[8:8 + 8 * N * wpr], np.uint64)
    words = words.reshape(N, 2) if wpr == 2 else words
    filt = np.frombuffer(raw[8 + 8 * N * wpr:8 + 8 * N * wpr + N], np.uint8)
    strand = np.frombuffer(raw[8 + 8 * N * wpr + N:], np.uint8)
    return words, filt, strand


@pytest.mark.parametrize("n,gz", [(24, False), (40, False), (24, True), (64, False)])
def test_dump_words_are_the_canonical_words(n, gz, tmp_path):
    files = pt.write_duplex_fastq(str(tmp_path / "in"), 3, 600, n=n, read_len=36, gz=gz)
    words, filt, strand = dump_paired(files, n, str(tmp_path))
    ew, ef, _, (hdr, take) = expected_words(files, n)
    assert hdr == 0 and list(take) == [n // 2, n // 2]
    cw, es = pt.canonical(ew, ef, n)
    assert len(filt) == 600 and np.array_equal(filt, ef) and len(strand) == 600
    assert np.array_equal(strand, es) and (es == pt.BOTTOM).sum() > 100 and (es == pt.TOP).sum() > 100 and ef.sum() > 0
    assert np.array_equal(words[ef == 0], cw[ef == 0])


def test_cli_refusals(tmp_path):
    files = pt.write_duplex_fastq(str(tmp_path / "in"), 4, 20)

    def refused(args, word):
        p = subprocess.run([HUMID, "-P", "-d", str(tmp_path / "out"), "-l", "/dev/null"] + args, stderr=subprocess.PIPE)
        first = p.stderr.decode().split("\n")[0]
        assert p.returncode != 0 and first.startswith("humid: ") and word in first, (args, p.returncode, first)
        assert not os.path.exists(str(tmp_path / "out"))

    refused(files[:1], "two input files")
    refused(files + files[:1], "two input files")
    refused(["-n", "23"] + files, "even")
    refused(["-b", "8"] + files, "-b")
    refused(["-e"] + files, "-e")
    refused(["-C"] + files, "-C")
    refused(["-g", "2"] + files, "one GPU")
    # a UMI in the headers is refused as well
    umi = []
    for k, f in enumerate(files):
        umi.append(str(tmp_path / ("umi_R%d.fastq" % (k + 1))))
        with open(umi[-1], "w") as out:
            for i, line in enumerate(open(f)):
                out.write(line.replace("@read", "@read_ACGTACGT_", 1).replace("_ACGTACGT_", "x_ACGTACGT ", 1) if i % 4 == 0 else line)
    refused(umi, "UMI")
