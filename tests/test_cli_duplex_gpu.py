"""-m gpu: `humid -P -D` end to end on a small two-file FastQ with reads of both strands, plain and gzip, without and
with -Q.  Cluster ids and strands are read from the _annotated files, the kept records from the _dedup headers of a
`humid -P` run on the same files; both _dedup files then equal the truth of tests/duplex_truth.py record by record,
duplex.dat equals its summaries, and headers, order and every other output are those of the run without -D."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import consensus_truth as ct
import duplex_truth as dt
import paired_truth as pt
from cli_util import HUMID, read_fastq
from humid_amd import build

pytestmark = pytest.mark.gpu

N_NT, N_RECORDS = 24, 600


@pytest.fixture(scope="module", autouse=True)
def _built():
    build.build_host()


def raw(path):
    return (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")).read()


def out_name(out, f, kind):
    stem, ext = os.path.basename(f).split(".", 1)
    return os.path.join(out, "%s_%s.%s" % (stem, kind, ext))


@pytest.mark.parametrize("gz,best", [(False, False), (True, False), (False, True)])
def test_duplex_consensus_files(gz, best, tmp_path):
    rng = np.random.default_rng(5)
    letters = rng.choice(list("+5?I"), size=N_RECORDS)                  # Phred 10, 20, 30, 40
    files = pt.write_duplex_fastq(str(tmp_path / "in"), 17, N_RECORDS, n=N_NT, read_len=32, gz=gz, qual_of=lambda i: letters[i])
    flags = ["-P", "-s", "-a"] + (["-Q"] if best else [])
    plain, out, log = str(tmp_path / "plain"), str(tmp_path / "out"), str(tmp_path / "log.txt")
    subprocess.check_call([HUMID] + flags + ["-d", plain, "-l", "/dev/null"] + files, timeout=300)
    subprocess.check_call([HUMID] + flags + ["-D", "-d", out, "-l", log] + files, timeout=300)
    # every output but the _dedup files and duplex.dat is that of the run without -D
    assert sorted(os.listdir(out)) == sorted(os.listdir(plain) + ["duplex.dat"])
    for name in os.listdir(plain):
        if "_dedup" not in name:
            assert raw(os.path.join(out, name)) == raw(os.path.join(plain, name)), name
    recs = [read_fastq(f) for f in files]
    n = len(recs[0])
    assert n == N_RECORDS
    # cluster ids and strands from the annotated headers (":<id>/A", ":<id>/B", ":0"), the kept reads from the dedup headers
    cid, strand = np.zeros(n, np.uint32), np.full(n, dt.NONE, np.uint8)
    for i, r in enumerate(read_fastq(out_name(out, files[0], "annotated"))):
        m = re.search(r":(\d+)(/[AB])?$", r[0])
        cid[i] = int(m.group(1))
        if m.group(2):
            strand[i] = dt.TOP if m.group(2) == "/A" else dt.BOTTOM
    index = {r[0]: i for i, r in enumerate(recs[0])}
    kept = [index[r[0]] for r in read_fastq(out_name(plain, files[0], "dedup"))]
    keep = np.zeros(n, np.uint8)
    keep[kept] = 1
    C = int(cid.max())
    assert len(kept) == C and np.all((strand == dt.NONE) == (cid == 0)) and (cid == 0).sum() > 0
    layers = [ct.flat([r[1].encode() for r in rs], [r[3].encode() for r in rs]) for rs in recs]
    expect = []
    for f in (0, 1):
        t = dt.duplex_numpy(layers[f], layers[1 - f], cid, keep, strand, C)
        dt.assert_same(t, dt.duplex_loop(layers[f], layers[1 - f], cid, keep, strand, C), "the two truths")
        expect.append(t)
        off = t["out_off"].astype(np.int64)
        got = read_fastq(out_name(out, files[f], "dedup"))
        was = read_fastq(out_name(plain, files[f], "dedup"))
        assert len(got) == len(was) == C
        for g, w, i in zip(got, was, kept):                             # in file order: headers and '+' lines unchanged
            c = int(cid[i])
            assert g[0] == w[0] == recs[f][i][0] and g[2] == w[2]
            assert g[1].encode() == bytes(t["bases"][off[c - 1]:off[c]]), (f, i)
            assert g[3].encode() == bytes(t["quals"][off[c - 1]:off[c]]), (f, i)
    sm = [t["summary"] for t in expect]
    assert sm[0]["duplex_clusters"] > 20 and sm[0]["disagree"] + sm[1]["disagree"] > 0 and sm[0]["bases_changed"] > 0
    want = "".join("file%d.%s %d\n" % (f + 1, k, sm[f][k]) for f in (0, 1) for k in dt.KEYS)
    assert open(os.path.join(out, "duplex.dat")).read() == want
    line = "  duplex consensus: %d clusters, %d duplex, %d columns called by both strands, %d agree, %d disagree, %d masked, %d bases changed\n" % (
        C, sm[0]["duplex_clusters"], sm[0]["both_called"] + sm[1]["both_called"], sm[0]["agree"] + sm[1]["agree"],
        sm[0]["disagree"] + sm[1]["disagree"], sm[0]["masked"] + sm[1]["masked"], sm[0]["bases_changed"] + sm[1]["bases_changed"])
    assert line in open(log).read()
