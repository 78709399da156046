"""Host side of `humid --word-pattern` and of several -w without a GPU: the word extraction (--dump-words stops after
pass 1) against a Python restatement of the pattern, and the refusals, each one `humid:` line and exit code 1."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, dump_words, read_fastq
from humid_amd import build


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def write_fastq(path, n, seed, read_len=60, short=0.1, p_n=0.01, header_umi=False):
    rng = np.random.default_rng(seed)
    with open(path, "w") as fh:
        for i in range(n):
            ln = int(rng.integers(0, read_len)) if rng.random() < short else read_len
            seq = "".join("ACGTN"[4 if rng.random() < p_n else x] for x in rng.integers(0, 4, size=ln))
            fh.write("@r%d%s\n%s\n+\n%s\n" % (i, "_ACGTACGT" if header_umi else "", seq, "I" * ln))
    return path


def pattern_words(files, pattern, word_nt):
    """the restatement: the first file's C letters, then its N letters, then the other files' prefixes; a letter the
    read does not have, or one outside ACGT, is a G and filters the word"""
    recs = [read_fastq(f) for f in files]
    n = min(len(r) for r in recs)
    at = [i for i, ch in enumerate(pattern) if ch == "C"] + [i for i, ch in enumerate(pattern) if ch == "N"]
    rest = word_nt - len(at)
    others = len(files) - 1
    take = [rest // others + (rest % others if f == others - 1 else 0) for f in range(others)] if others else []
    words = np.zeros((n, 2) if word_nt > 32 else n, np.uint64)
    filt = np.zeros(n, np.uint8)
    for i in range(n):
        first = recs[0][i][1]
        sym = [first[p] if p < len(first) else "N" for p in at]
        for f in range(others):
            s = recs[f + 1][i][1]
            sym += [s[p] if p < len(s) else "N" for p in range(take[f])]
        v = 0
        for ch in sym:
            filt[i] |= ch not in "ACGT"
            v = (v << 2) | ("ACGT".index(ch) if ch in "ACGT" else 2)
        if word_nt > 32:
            words[i] = (v >> 64, v & ((1 << 64) - 1))
        else:
            words[i] = v
    return words, filt


def dump(files, word_nt, tmp, extra, env=None):
    out = os.path.join(tmp, "words.bin")
    e = dict(os.environ)
    e.update(env or {})
    subprocess.check_call([HUMID, "-n", str(word_nt), "-l", os.path.join(tmp, "log.txt"), "--dump-words", out] + extra + list(files),
                          env=e)
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], np.uint64)[0])
    wpr = 2 if word_nt > 32 else 1
    words = np.frombuffer(raw[8:8 + 8 * n * wpr], np.uint64)
    return (words.reshape(n, 2) if wpr == 2 else words), np.frombuffer(raw[8 + 8 * n * wpr:8 + 8 * n * wpr + n], np.uint8)


SPLIT = "N" * 10 + "C" * 8 + "X" * 12 + "C" * 8 + "X" * 12 + "C" * 8       # SPLiT-seq: UMI, three segments, two linkers
CASES = [
    (1, SPLIT, 34),                                                         # the wide path: 24 + 10 > 32
    (2, SPLIT, 50),                                                         # ... with 16 more from the second file
    (1, "XXX" + "C" * 6 + "XX" + "N" * 4 + "X" + "C" * 2 + "NN" + "XXXX", 14),   # leading, inner and trailing X; C and N interleaved
    (2, "XXCCCCXNNNCCX", 24),
    (3, "NNNNXXCC", 31),                                                    # 25 from two other files: 12 and 13
    (2, "XXXXNNNN", 12),                                                    # no barcode
]


@pytest.mark.parametrize("n_files,pattern,word_nt", CASES)
def test_pattern_words(n_files, pattern, word_nt, tmp_path):
    files = [write_fastq(str(tmp_path / ("r%d.fastq" % f)), 300, 10 * word_nt + f) for f in range(n_files)]
    want = pattern_words(files, pattern, word_nt)
    assert 0 < int(want[1].sum()) < 300                             # short reads and N: some words are filtered
    gz = str(tmp_path / "r0.fastq.gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(open(files[0], "rb").read())
    for fs, env in ((files, {}), (files, {"HUMID_HOST_SLOW": "1"}), ([gz] + files[1:], {}), (files, {"HUMID_DEVICE_PACK": "1"})):
        got = dump(fs, word_nt, str(tmp_path), ["--word-pattern", pattern], env)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    k = pattern.count("C")
    if k:                                                           # -b may repeat the pattern's K
        got = dump(files, word_nt, str(tmp_path), ["--word-pattern", pattern, "-b", str(k)])
        assert np.array_equal(got[0], want[0])
    log = open(tmp_path / "log.txt").read()
    assert "  header: 0" in log and "%s: %d" % (files[0], k + pattern.count("N")) in log


@pytest.mark.parametrize("n_files,word_nt,k", [(1, 28, 16), (2, 24, 8), (1, 40, 12), (2, 33, 5)])
def test_prefix_pattern_equals_dash_b(n_files, word_nt, k, tmp_path):
    """C x K then N x (the rest of the first file's share) is today's -b K, byte for byte"""
    files = [write_fastq(str(tmp_path / ("r%d.fastq" % f)), 200, 7 * word_nt + f, read_len=45) for f in range(n_files)]
    share = word_nt // n_files                                      # (the remainder goes to the last file)
    a = dump_words(files, word_nt, str(tmp_path))
    b = dump(files, word_nt, str(tmp_path), ["--word-pattern", "C" * k + "N" * ((word_nt if n_files == 1 else share) - k)])
    c = dump(files, word_nt, str(tmp_path), ["-b", str(k)])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], c[0])


def refused(args, must_say):
    p = subprocess.run([HUMID] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    lines = p.stderr.strip().split("\n")
    assert p.returncode == 1 and len(lines) == 1 and lines[0].startswith("humid: ") and must_say in lines[0], (args, p.returncode, p.stderr)


def test_refusals(tmp_path):
    f1 = write_fastq(str(tmp_path / "a.fastq"), 20, 1)
    f2 = write_fastq(str(tmp_path / "b.fastq"), 20, 2)
    umi = write_fastq(str(tmp_path / "u.fastq"), 20, 3, header_umi=True)
    wls = []
    for j, nt in enumerate((4, 4, 4)):
        wls.append(str(tmp_path / ("w%d.txt" % j)))
        open(wls[-1], "w").write("ACGT\nAAAA\n")
    three = ["-w", wls[0], "-w", wls[1], "-w", wls[2]]
    out = ["-d", str(tmp_path / "out"), "-l", "/dev/null"]
    pat = ["--word-pattern", "C" * 12 + "N" * 12, "-n", "24"]
    refused(pat + out + [umi], "UMI in its headers")
    refused(["--word-pattern", "C" * 12, "-n", "24", "-P"] + out + [f1, f2], "-P")
    refused(pat + ["-g", "2"] + out + [f1], "one GPU")
    e = dict(os.environ, HUMID_FORCE_SHARDED="1")
    p = subprocess.run([HUMID] + pat + out + [f1], env=e, stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 1 and p.stderr.count("\n") == 1 and "one GPU" in p.stderr
    refused(pat + ["-w", wls[0], "--barcode-posterior"] + out + [f1], "--barcode-posterior")
    refused(["-n", "24", "-b", "12", "--barcode-posterior"] + three + out + [f1], "--barcode-posterior")
    refused(["-n", "24", "-b", "12", "--cells-expected", "10"] + three + out + [f1], "--cells")
    refused(["-n", "24", "-b", "12", "--cells-top", "10", "--cells-merge-ratio", "3"] + three + out + [f1], "--cells")
    refused(["--word-pattern", "CCNZ", "-n", "3"] + out + [f1], "--word-pattern")
    refused(["--word-pattern", "CCNN", "-n", "5"] + out + [f1], "must add up to")         # one file: n = #C + #N
    refused(["--word-pattern", "CCNN", "-n", "3"] + out + [f1, f2], "exceed")
    refused(pat + ["-b", "11"] + out + [f1], "-b says 11")
    refused(["-n", "24", "-b", "12", "-w", wls[0], "--barcode-max-inexact", "1"] + out + [f1], "several -w")
    assert not os.path.exists(tmp_path / "out")                     # nothing was opened, nothing written
    # the segments' files: one length per file, the lengths add up to K, at most S inexact segments (as today's -w: exit 2)
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("ACGT\nACG\n")
    long = str(tmp_path / "long.txt")
    open(long, "w").write("ACGTACGTACG\n")
    for args, say in ((["-b", "12", "-w", wls[0], "-w", bad, "-w", wls[2]], "line 2 has 3 letters"),
                      (["-b", "13"] + three, "add up to 12 letters"),
                      (["-b", "15", "-w", wls[0], "-w", long], "1 .. 10"),
                      (["-b", "12", "--barcode-max-inexact", "4"] + three, "exceeds the 3 segments")):
        p = subprocess.run([HUMID, "-n", "24"] + args + out + [f1], stderr=subprocess.PIPE, text=True, timeout=60)
        assert p.returncode == 2 and p.stderr.startswith("humid: ") and say in p.stderr.split("\n")[0], (args, p.stderr)
