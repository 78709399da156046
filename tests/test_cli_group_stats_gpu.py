"""-m gpu: the groups.dat table of `humid -b K -s`: one line "<barcode> <reads> <unique> <clusters>" per distinct
barcode, ascending.  The expected table comes from the per-group truth (tests/grouped_truth.py, one oracle pass per
barcode) and the barcode letters from the reads themselves; the other outputs stay what test_cli_keyed_gpu.py
expects of them."""
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, expected_words, read_fastq

import grouped_truth as gt

pytestmark = pytest.mark.gpu


def dat(path):
    return [tuple(int(x) for x in l.split()) for l in open(path).read().strip().split("\n") if l]


def barcoded_fastq(path, n_reads, seed, n_cells=12, n_umis=40, k=16, umi=12, tail=20, p_sub=0.02, p_n=0.004):
    """one file, read = cell barcode (k nt) + UMI + cDNA: few cells, few UMIs, substitutions in both (the generator of
    test_cli_keyed_gpu.py)"""
    rng = np.random.default_rng(seed)
    cells = rng.integers(0, 4, size=(n_cells, k))
    cells[1] = cells[0]
    cells[1, 5] = (cells[0, 5] + 1) % 4                             # two cells one nucleotide apart
    umis = rng.integers(0, 4, size=(n_umis, umi))
    rows = np.concatenate([cells[rng.integers(0, n_cells, size=n_reads)], umis[rng.integers(0, n_umis, size=n_reads)],
                           rng.integers(0, 4, size=(n_reads, tail))], 1)
    sub = rng.random(rows.shape) < p_sub
    rows = np.where(sub, rng.integers(0, 4, size=rows.shape), rows)
    rows = np.where(rng.random(rows.shape) < p_n, 4, rows)
    with open(path, "w") as fh:
        for i, r in enumerate(rows):
            seq = "".join("ACGTN"[x] for x in r)
            fh.write("@r%d\n%s\n+\n%s\n" % (i, seq, "I" * len(seq)))
    return [path]


def split_words(words, word_nt, k):
    """packed n-nt words (u64[N] or [N, 2]) -> (key u64[N]: the first k nt, words of the remaining n - k nt)"""
    vals = [(int(w[0]) << 64) | int(w[1]) for w in words] if word_nt > 32 else [int(w) for w in words]
    rb = 2 * (word_nt - k)
    keys = np.asarray([v >> rb for v in vals], np.uint64)
    rest = [v & ((1 << rb) - 1) for v in vals]
    if word_nt - k > 32:
        return keys, np.asarray([[v >> 64, v & ((1 << 64) - 1)] for v in rest], np.uint64).reshape(-1, 2)
    return keys, np.asarray(rest, np.uint64)


def truth_for(files, word_nt, k, d, maximum=False):
    """(per-group truth, records, expected lines of groups.dat)"""
    words, filt, recs, _ = expected_words(files, word_nt)
    keys, rest = split_words(words, word_nt, k)
    K, inv = np.unique(keys[filt == 0], return_inverse=True)
    groups = np.full(len(filt), 0xFFFFFFFF, np.uint32)
    groups[filt == 0] = inv.astype(np.uint32)
    t = gt.per_group(rest, groups, filt, word_nt - k, d, int(maximum))
    usable = np.flatnonzero(filt == 0)
    lg = t["leaves"]["group"]
    lines = []
    for g, key in enumerate(K):
        members = usable[inv == g]
        letters = {recs[0][i][1][:k] for i in members}               # the barcode as the reads spell it
        assert len(letters) == 1
        letters = letters.pop()
        assert sum("ACGT".index(c) << (2 * (k - 1 - j)) for j, c in enumerate(letters)) == int(key)
        ids = np.unique(t["cid"][members])
        assert ids[0] > 0
        lines.append("%s %d %d %d" % (letters, len(members), int((lg == g).sum()), len(ids)))
    return t, recs, lines


def check_other_outputs(out, files, t, recs):
    n = len(t["cid"])
    for fi, f in enumerate(files):
        base = os.path.basename(f)
        dedup = read_fastq(os.path.join(out, base.replace(".fastq", "_dedup.fastq")))
        annot = read_fastq(os.path.join(out, base.replace(".fastq", "_annotated.fastq")))
        assert dedup == [recs[fi][i] for i in range(n) if t["keep"][i]]
        assert annot == [(recs[fi][i][0] + ":%d" % t["cid"][i],) + recs[fi][i][1:] for i in range(n)]
    h = t["hist"]
    assert dat(os.path.join(out, "counts.dat")) == h["counts"]
    assert dat(os.path.join(out, "neigh.dat")) == h["neigh"]
    assert dat(os.path.join(out, "clusters.dat")) == h["clusters"]
    st = dict(l.split(": ") for l in open(os.path.join(out, "stats.dat")).read().strip().split("\n"))
    s = t["summary"]
    assert {k: int(v) for k, v in st.items()} == dict(total=s["total"], usable=s["usable"], unique=s["unique"],
                                                      clusters=s["clusters"])


@pytest.mark.parametrize("word_nt,k,flags,gen", [
    (28, 16, [], dict()),
    (48, 10, ["-x"], dict(k=10, umi=12, tail=30, n_cells=9)),       # a wide word: 38 nt are clustered
])
def test_groups_dat(word_nt, k, flags, gen, tmp_path):
    files = barcoded_fastq(str(tmp_path / "cells.fastq"), 4000, 71 + k, **gen)
    out = str(tmp_path / "out")
    subprocess.check_call([HUMID, "-n", str(word_nt), "-b", str(k), "-d", out, "-l", "/dev/null", "-s", "-a"] + flags + files,
                          timeout=300)
    t, recs, lines = truth_for(files, word_nt, k, 1, maximum="-x" in flags)
    got = open(os.path.join(out, "groups.dat")).read()
    assert got.endswith("\n")
    got = got.split("\n")[:-1]
    assert len(got) == len(lines) > 5
    for a, b in zip(got, lines):
        assert a == b
    assert [l.split()[0] for l in got] == sorted(l.split()[0] for l in got)     # ascending by key = by letters (A < C < G < T)
    s = t["summary"]
    cols = np.asarray([[int(x) for x in l.split()[1:]] for l in got])
    assert cols.sum(0).tolist() == [s["usable"], s["unique"], s["clusters"]]
    check_other_outputs(out, files, t, recs)
    assert sorted(os.listdir(out)) == sorted(["cells_dedup.fastq", "cells_annotated.fastq", "counts.dat", "neigh.dat",
                                              "clusters.dat", "stats.dat", "groups.dat"])


def test_no_groups_dat_without_s_or_without_b(tmp_path):
    files = barcoded_fastq(str(tmp_path / "cells.fastq"), 1000, 5)
    for name, flags in (("no_s", ["-b", "16"]), ("no_b", ["-s"])):
        out = str(tmp_path / name)
        subprocess.check_call([HUMID, "-n", "28", "-d", out, "-l", "/dev/null"] + flags + files, timeout=300)
        assert os.path.exists(os.path.join(out, "cells_dedup.fastq"))
        assert not os.path.exists(os.path.join(out, "groups.dat"))
        assert os.path.exists(os.path.join(out, "stats.dat")) == (name == "no_b")
