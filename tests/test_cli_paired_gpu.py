"""-m gpu: `humid -P` end to end on a small two-file FastQ with reads of both strands.  Expected words come from the
oracle's word extraction (cli_util.expected_words), everything else from tests/paired_truth.py: the _dedup and
_annotated files byte for byte, stats.dat, strands.dat and the log line; with -Q the kept record of every cluster."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import paired_truth as pt
from cli_util import HUMID, expected_words, read_fastq
from humid_amd import build

pytestmark = pytest.mark.gpu

N_NT = 24


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def raw(path):
    return (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")).read()


def record_bytes(rec, tag=""):
    return ("%s%s\n%s\n%s\n%s\n" % (rec[0], tag, rec[1], rec[2], rec[3])).encode()


def check_outputs(out, files, recs, t, keep):
    for f, rs in zip(files, recs):
        base = os.path.basename(f)
        stem, ext = base.split(".", 1)
        dedup = b"".join(record_bytes(r) for r, k in zip(rs, keep) if k)
        assert raw(os.path.join(out, "%s_dedup.%s" % (stem, ext))) == dedup, base
        tags = [":%d%s" % (c, {pt.TOP: "/A", pt.BOTTOM: "/B", pt.NONE: ""}[s]) for c, s in zip(t["cluster_id"], t["strand"])]
        annot = b"".join(record_bytes(r, tag) for r, tag in zip(rs, tags))
        assert raw(os.path.join(out, "%s_annotated.%s" % (stem, ext))) == annot, base
    s, st = t["summary"], t["strands"]
    assert open(os.path.join(out, "stats.dat")).read() == \
        "total: %d\nusable: %d\nunique: %d\nclusters: %d\n" % (s["total"], s["usable"], s["unique"], s["clusters"])
    assert open(os.path.join(out, "strands.dat")).read() == \
        "clusters: %d\nduplex: %d\ntop_only: %d\nbottom_only: %d\ntop_reads: %d\nbottom_reads: %d\n" % (
            st["n_clusters"], st["duplex"], st["top_only"], st["bottom_only"], st["top_reads"], st["bottom_reads"])
    for name, key in (("counts.dat", "counts"), ("neigh.dat", "neigh"), ("clusters.dat", "clusters")):
        assert open(os.path.join(out, name)).read() == "".join("%d %d\n" % kv for kv in t["hist"][key]), name


@pytest.mark.parametrize("maximum,gz", [(False, False), (True, False), (False, True)])
def test_dedup_annotated_and_statistics(maximum, gz, tmp_path):
    files = pt.write_duplex_fastq(str(tmp_path / "in"), 11, 1500, n=N_NT, read_len=32, gz=gz)
    words, filt, recs, _ = expected_words(files, N_NT)
    t = pt.run(words, filt, N_NT, 1, int(maximum))
    assert t["strands"]["duplex"] > 50 and t["strands"]["top_only"] > 0 and t["strands"]["bottom_only"] > 0 and filt.sum() > 0
    out, log = str(tmp_path / "out"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-P", "-s", "-a", "-d", out, "-l", log] + (["-x"] if maximum else []) + files, timeout=300)
    check_outputs(out, files, recs, t, t["keep"])
    st = t["strands"]
    assert "  strands: %d clusters, %d duplex, %d top only, %d bottom only; %d top reads, %d bottom reads\n" % (
        st["n_clusters"], st["duplex"], st["top_only"], st["bottom_only"], st["top_reads"], st["bottom_reads"]) in open(log).read()
    # the molecules are counted once: the plain run on the same files sees about twice the clusters of the duplex ones
    plain = str(tmp_path / "plain")
    subprocess.check_call([HUMID, "-s", "-d", plain, "-l", "/dev/null"] + (["-x"] if maximum else []) + files, timeout=300)
    n_plain = int(open(os.path.join(plain, "stats.dat")).read().split("clusters: ")[1])
    assert n_plain >= t["summary"]["clusters"] + st["duplex"] // 2


def test_best_quality_keeps_a_bottom_strand_record(tmp_path):
    rng = np.random.default_rng(5)
    letters = rng.choice(list("5?I"), size=1200)                        # Phred 20, 30, 40
    files = pt.write_duplex_fastq(str(tmp_path / "in"), 13, 1200, n=N_NT, read_len=32, qual_of=lambda i: letters[i])
    words, filt, recs, _ = expected_words(files, N_NT)
    t = pt.run(words, filt, N_NT, 1)
    scores = np.zeros(len(filt), np.int64)                              # the sum of the qualities >= 15 over both files
    for rs in recs:
        scores += np.array([sum(ord(c) - 33 for c in r[3] if ord(c) >= 48) for r in rs], np.int64)
    cvals = pt.to_ints(t["canonical"], N_NT)
    keep = np.zeros(len(filt), np.uint8)
    moved_to_bottom = 0
    for k in np.flatnonzero(t["keep"]):
        cand = [i for i in np.flatnonzero(t["cluster_id"] == t["cluster_id"][k]) if cvals[i] == cvals[k]]
        b = max(cand, key=lambda i: (scores[i], -i))
        keep[b] = 1
        moved_to_bottom += int(b != k and t["strand"][b] == pt.BOTTOM)
    assert moved_to_bottom > 10                                          # the case says something
    out, log = str(tmp_path / "out"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID, "-P", "-Q", "-s", "-a", "-d", out, "-l", log] + files, timeout=300)
    check_outputs(out, files, recs, t, keep)
    assert "  quality: %d clusters keep another record\n" % int((keep & ~t["keep"] & 1).sum()) in open(log).read()
