"""-m gpu: `humid -b K` end to end.  The first K nucleotides of the word are matched exactly (the group key), the
remaining n - K are clustered by -m / -e / -x.  Expected words come from the oracle's word extraction
(cli_util.expected_words), split at K; expected cluster ids and keep flags from the per-group truth
(tests/grouped_truth.py, one oracle pass per key); the expected files are written from those."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, expected_words, read_fastq
from humid_amd.synth import synth_fastq

import grouped_truth as gt

pytestmark = pytest.mark.gpu


def dat(path):
    return [tuple(int(x) for x in l.split()) for l in open(path).read().strip().split("\n") if l]


def split_words(words, word_nt, k):
    """packed n-nt words (u64[N] or [N, 2]) -> (key u64[N]: the first k nt, words of the remaining n - k nt)"""
    vals = [(int(w[0]) << 64) | int(w[1]) for w in words] if word_nt > 32 else [int(w) for w in words]
    rb = 2 * (word_nt - k)
    keys = np.asarray([v >> rb for v in vals], np.uint64)
    rest = [v & ((1 << rb) - 1) for v in vals]
    if word_nt - k > 32:
        return keys, np.asarray([[v >> 64, v & ((1 << 64) - 1)] for v in rest], np.uint64).reshape(-1, 2)
    return keys, np.asarray(rest, np.uint64)


def truth_for(files, word_nt, k, d, maximum=False, edit=False):
    words, filt, recs, _ = expected_words(files, word_nt)
    keys, rest = split_words(words, word_nt, k)
    K, inv = np.unique(keys[filt == 0], return_inverse=True)
    groups = np.full(len(filt), 0xFFFFFFFF, np.uint32)
    groups[filt == 0] = inv.astype(np.uint32)
    return gt.per_group(rest, groups, filt, word_nt - k, d, int(maximum), edit=edit), recs


def check_outputs(out, files, t, recs, gz=False, stats=True):
    ext = ".fastq.gz" if gz else ".fastq"
    n = len(t["cid"])
    for fi, f in enumerate(files):
        base = os.path.basename(f)
        dedup = read_fastq(os.path.join(out, base.replace(ext, "_dedup" + ext)))
        annot = read_fastq(os.path.join(out, base.replace(ext, "_annotated" + ext)))
        assert dedup == [recs[fi][i] for i in range(n) if t["keep"][i]]
        assert annot == [(recs[fi][i][0] + ":%d" % t["cid"][i],) + recs[fi][i][1:] for i in range(n)]
    if stats:
        h = t["hist"]
        assert dat(os.path.join(out, "counts.dat")) == h["counts"]
        assert dat(os.path.join(out, "neigh.dat")) == h["neigh"]
        assert dat(os.path.join(out, "clusters.dat")) == h["clusters"]
        st = dict(l.split(": ") for l in open(os.path.join(out, "stats.dat")).read().strip().split("\n"))
        s = t["summary"]
        assert {k: int(v) for k, v in st.items()} == dict(total=s["total"], usable=s["usable"], unique=s["unique"],
                                                          clusters=s["clusters"])


def barcoded_fastq(path, n_reads, seed, n_cells=12, n_umis=40, k=16, umi=12, tail=20, p_sub=0.02, p_n=0.004):
    """one file, read = cell barcode (k nt) + UMI + cDNA: few cells, few UMIs, substitutions in both"""
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


@pytest.mark.parametrize("flags,d", [([], 1), (["-x"], 1), (["-e", "-m", "2"], 2), (["-m", "0"], 0)])
def test_barcode_and_umi_in_the_read(flags, d, tmp_path):
    files = barcoded_fastq(str(tmp_path / "cells.fastq"), 4000, 41)
    out = str(tmp_path / "out")
    subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-d", out, "-l", str(tmp_path / "log.txt"), "-s", "-a"] + flags
                          + files, timeout=300)
    t, recs = truth_for(files, 28, 16, d, maximum="-x" in flags, edit="-e" in flags)
    assert t["summary"]["edges"] > 0 or d == 0
    check_outputs(out, files, t, recs)
    log = open(tmp_path / "log.txt").read()
    assert ("Levenshtein" if "-e" in flags else "Hamming") in log and "Writing annotated results... done." in log


@pytest.mark.parametrize("word_nt,k", [(24, 8), (48, 10), (40, 4)])
def test_header_umi_and_two_files(word_nt, k, tmp_path):
    """the word starts with the header UMI: its first k nucleotides are the key; wide words split into a one-uint64
    or a two-uint64 rest"""
    files = synth_fastq(str(tmp_path / "in"), 3000, 123, n_files=2, umi_len=8, umi_in_header=True, p_sub=4e-3, p_n=2e-3,
                        read_len=36, short_frac=0.01)
    out = str(tmp_path / "out")
    subprocess.check_call([HUMID, "-n", str(word_nt), "-b", str(k), "-d", out, "-l", "/dev/null", "-s", "-a"] + files,
                          timeout=300)
    t, recs = truth_for(files, word_nt, k, 1)
    check_outputs(out, files, t, recs)


def test_gz_in_and_out_and_the_streaming_path(tmp_path):
    files = barcoded_fastq(str(tmp_path / "cells.fastq"), 3000, 43)
    gz = str(tmp_path / "cells.fastq.gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(open(files[0], "rb").read())
    t, recs = truth_for(files, 28, 16, 1)
    for name, env in (("fast", {}), ("slow", {"HUMID_HOST_SLOW": "1"}), ("devicepack", {"HUMID_DEVICE_PACK": "1"})):
        out = str(tmp_path / name)
        e = dict(os.environ)
        e.update(env)
        subprocess.check_call([HUMID, "-n", "28", "-b", "16", "-d", out, "-l", "/dev/null", "-s", "-a", gz], env=e, timeout=300)
        check_outputs(out, [gz], t, recs, gz=True)


def test_barcodes_one_nucleotide_apart_stay_apart(tmp_path):
    """the point of the flag: two cells whose barcodes differ in one nucleotide carry the same UMI.  -n 28 -b 16 keeps
    a read of each; plain -n 28 -m 1 merges them into one cluster and keeps one"""
    bc1, bc2, umi = "ACGTACGTACGTACGA", "ACGTACGTACGTACGT", "TTGCAAGGCTAC"
    path = str(tmp_path / "two_cells.fastq")
    with open(path, "w") as fh:
        for i, bc in enumerate([bc1, bc1, bc1, bc1, bc2, bc2]):           # (4 >= 2 x 2: the directional rule merges)
            seq = bc + umi + "GATTACAGATTACA"
            fh.write("@r%d\n%s\n+\n%s\n" % (i, seq, "I" * len(seq)))
    kept = {}
    for name, flags in (("keyed", ["-b", "16"]), ("plain", [])):
        out = str(tmp_path / name)
        subprocess.check_call([HUMID, "-n", "28", "-d", out, "-l", "/dev/null", "-a", "-s"] + flags + [path], timeout=300)
        kept[name] = [r[0] for r in read_fastq(os.path.join(out, "two_cells_dedup.fastq"))]
        ids = [r[0].rsplit(":", 1)[1] for r in read_fastq(os.path.join(out, "two_cells_annotated.fastq"))]
        assert ids == (["1", "1", "1", "1", "2", "2"] if name == "keyed" else ["1"] * 6)
    assert kept["keyed"] == ["@r0", "@r4"]
    assert kept["plain"] == ["@r0"]
    t, recs = truth_for([path], 28, 16, 1)
    check_outputs(str(tmp_path / "keyed"), [path], t, recs)
