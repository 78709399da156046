"""No GPU: the two truths of tests/consensus_truth.py against each other (on the oracle's clusters with random ragged
reads, and on hand cases), the new symbols of the C ABI, the command line's refusals of -C (several ranks, the
streaming input path), the usage text, and what -C hands to the GPU (--dump-consensus-input) against a Python parse
on every retained input path."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from humid_amd import _lib
from humid_amd.synth import synth_fastq, synth_words
from oracle import pyoracle as orc

import consensus_truth as ct
from cli_util import HUMID, ROOT, read_fastq


def both(bases, quals, off, cid, keep, C, min_q=10, cap_q=93):
    a = ct.consensus_loop(bases, quals, off, cid, keep, C, min_q, cap_q)
    ct.assert_same(a, ct.consensus_numpy(bases, quals, off, cid, keep, C, min_q, cap_q), "the two truths")
    return a


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("distance", [0, 1, 2])
def test_the_two_truths_agree_on_the_oracle(distance, method):
    words, filt = synth_words(3000, 5, 24, p_sub=4e-3)
    cid, keep, s, _ = orc.dedup_run(words, filt, 24, distance, method)
    rng = np.random.default_rng(10 * distance + method)
    lengths = rng.choice(np.asarray([0, 1, 30, 63, 64, 65, 80]), len(cid))
    b, q, off = ct.random_reads(rng, cid, lengths, odd_quals=True)
    for min_q, cap_q in ((10, 93), (0, 40), (93, 1)):
        a = both(b, q, off, cid, keep, s["clusters"], min_q, cap_q)
        sm = a["summary"]
        assert sm["n_clusters"] == s["clusters"] and int(a["depth"].sum()) == int((cid != 0).sum())
        assert sm["total_bytes"] == int(np.diff(off)[keep != 0].sum()) == len(a["bases"]) == int(a["out_off"][-1])
        assert sm["errors"] == int(a["errors"].sum()) and sm["multi_read"] == int((a["depth"] >= 2).sum())
    assert sm["multi_read"] > 100 and sm["votes"] > 0


def test_the_matrix_form_agrees_on_reads_of_one_length():
    from humid_amd.synth import synth_reads
    words, filt = synth_words(3000, 5, 24, p_sub=4e-3)
    cid, keep, s, _ = orc.dedup_run(words, filt, 24, 1, 0)
    b, q = synth_reads(cid, 3, read_len=70, p_sub=0.05)
    q[::7, ::7] = [0, 33, 40, 127, 255, 34, 43, 60, 200, 126]           # odd quality bytes
    b[5::11, 1::5] = ord("N")
    b[3::13, 2::7] |= 0x20
    off = np.arange(len(cid) + 1, dtype=np.uint64) * np.uint64(70)
    for min_q, cap_q, chunk in ((10, 93, 200_000), (0, 40, 100), (93, 1, 1)):
        a = both(b.reshape(-1), q.reshape(-1), off, cid, keep, s["clusters"], min_q, cap_q)
        ct.assert_same(a, ct.consensus_matrix(b, q, cid, keep, s["clusters"], min_q, cap_q, chunk=chunk), "the matrix form")
    assert a["summary"]["multi_read"] > 100


def one(reads, keep_at=0, **kw):
    """one cluster of the given (bases, quals) reads -> (consensus bases, quals, errors, summary)"""
    b, q, off = ct.flat([r[0] for r in reads], [r[1] for r in reads])
    cid = np.ones(len(reads), np.uint32)
    keep = np.zeros(len(reads), np.uint8)
    keep[keep_at] = 1
    a = both(b, q, off, cid, keep, 1, **kw)
    return bytes(a["bases"]), bytes(a["quals"]), int(a["errors"][0]), a["summary"]


def test_hand_cases():
    # a singleton is its own record: N, lowercase and a quality below min_q come back verbatim
    rec = (b"ACGTNacgtAC", b"III#I+5!#I~")
    assert one([rec])[:3] == (rec[0], rec[1], 0)
    assert one([rec])[3] == dict(n_clusters=1, total_bytes=11, multi_read=0, bases_changed=0, votes=5, errors=0)
    # 2 against 1: the majority base, the margin as quality, one disagreeing vote
    b, q, e, sm = one([(b"A", b"5"), (b"C", b"5"), (b"C", b"5")])      # '5' = Q20
    assert (b, q, e) == (b"C", bytes([33 + 20]), 1) and sm["bases_changed"] == 1 and sm["multi_read"] == 1
    # ... but one strong read beats two weak ones (sums of weights decide, not counts)
    assert one([(b"A", b"I"), (b"C", b"5"), (b"C", b"/")])[:3] == (b"A", bytes([33 + 40 - 20 - 14]), 2)
    # an exact tie gives N!
    assert one([(b"A", b"5"), (b"C", b"5")])[:3] == (b"N", b"!", 0)
    assert one([(b"A", b"5"), (b"C", b"5")])[3]["bases_changed"] == 1
    assert one([(b"A", b"5"), (b"C", b"5"), (b"G", b"+")])[:3] == (b"N", b"!", 0)   # a third, weaker base changes nothing
    # cap_q clips; without it the margin is the sum
    assert one([(b"G", b"I"), (b"G", b"I"), (b"G", b"I")], cap_q=93)[:2] == (b"G", bytes([33 + 93]))
    assert one([(b"G", b"I"), (b"G", b"I")], cap_q=93)[:2] == (b"G", bytes([33 + 80]))
    assert one([(b"G", b"I"), (b"G", b"I")], cap_q=40)[:2] == (b"G", bytes([33 + 40]))
    assert one([(b"G", b"I")], cap_q=1)[:2] == (b"G", bytes([34]))
    # a column where nothing votes copies the representative (here the second read is kept)
    assert one([(b"N", b"I"), (b"a", b"#"), (b"C", b"!")], keep_at=1)[:3] == (b"a", b"#", 0)
    assert one([(b"C", b"("), (b"T", b"I")], keep_at=0, min_q=41)[:3] == (b"C", b"(", 0)
    # min_q = 0 still needs a weight: quality 0 never votes
    assert one([(b"C", b"!"), (b"T", b"\"")], keep_at=0, min_q=0)[:3] == (b"T", b"\"", 0)
    # quality bytes below 33 count as 0, above 126 as 93
    assert one([(b"C", b"\x05"), (b"T", b"\xff")], keep_at=0, min_q=0)[:2] == (b"T", bytes([33 + 93]))
    # reads shorter and longer than the representative: the output has the representative's length
    b, q, e, sm = one([(b"ACGT", b"5555"), (b"AC", b"55"), (b"ATGTTTTT", b"55555555")], keep_at=0)
    assert (b, q, e) == (b"ACGT", bytes([33 + 60, 33 + 20, 33 + 40, 33 + 40]), 1) and sm["votes"] == 10
    # a length-0 representative: an empty record, whatever the others hold
    b, q, e, sm = one([(b"", b""), (b"ACGT", b"IIII")], keep_at=0)
    assert (b, q, e) == (b"", b"", 0) and sm["total_bytes"] == 0 and sm["votes"] == 0 and sm["multi_read"] == 1


def test_ids_zero_are_no_members_and_the_layout_is_by_cluster_id():
    b, q, off = ct.flat([b"TT", b"\x00\xff\x00", b"AAAA", b"C", b"AAAT"], [b"II", b"\x00\x00\x00", b"5555", b"I", b"5555"])
    cid = np.asarray([2, 0, 1, 2, 1], np.uint32)
    keep = np.asarray([0, 0, 1, 1, 0], np.uint8)
    a = both(b, q, off, cid, keep, 2)
    assert bytes(a["bases"]) == b"AAAN" + b"N" and list(a["out_off"]) == [0, 4, 5] and list(a["depth"]) == [2, 2]
    assert bytes(a["quals"]) == bytes([73, 73, 73, 33, 33])


def test_symbols_are_declared_and_exported():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "humid_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("humid_consensus", "humid_consensus_device", "humid_get_consensus", "humid_consensus_result_device"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SYMBOLS and hasattr(lib, name)
    assert re.search(r"\bhumid_consensus_summary\b", text)
    assert [k for k, _ in _lib.HumidConsensusSummary._fields_] == list(ct.KEYS)
    assert lib.humid_abi_version() == 5
    assert lib.humid_consensus(None, None, None, None, 0, None, None, 0, 0, 10, 93, None) == -1     # no context
    assert lib.humid_get_consensus(None, 0, None, None, None, None, None) == -1


@pytest.mark.parametrize("how", ["-g", "HUMID_GPUS", "HUMID_FORCE_SHARDED"])
def test_cli_refuses_c_on_several_ranks(how, tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=40)
    e = dict(os.environ)
    args = ["-C"]
    if how == "-g":
        args += ["-g", "2"]
    else:
        e[how] = "2" if how == "HUMID_GPUS" else "1"
    r = subprocess.run([HUMID] + args + ["-d", str(tmp_path / "out"), "-l", "/dev/null"] + files, capture_output=True, env=e,
                       timeout=60)
    assert r.returncode == 1 and b"one GPU" in r.stderr and b"-C" in r.stderr
    assert not os.path.exists(tmp_path / "out")


@pytest.mark.parametrize("how", ["crlf", "HUMID_HOST_SLOW", "HUMID_RETAIN_GB"])
def test_cli_refuses_c_on_the_streaming_path(how, tmp_path):
    files = synth_fastq(str(tmp_path / "in"), 1500, 8, n_files=1, read_len=40)   # (inflates beyond the smallest budget)
    e = dict(os.environ)
    if how == "crlf":
        raw = open(files[0], "rb").read()
        open(files[0], "wb").write(raw.replace(b"\n", b"\r\n"))
    elif how == "HUMID_HOST_SLOW":
        e[how] = "1"
    else:                                                                # a gzip file that inflates beyond the budget
        with gzip.open(files[0] + ".gz", "wb") as fh:
            fh.write(open(files[0], "rb").read())
        files = [files[0] + ".gz"]
        e[how] = "0.000001"
    r = subprocess.run([HUMID, "-C", "-d", str(tmp_path / "out"), "-l", "/dev/null"] + files, capture_output=True, env=e,
                       timeout=60)
    assert r.returncode == 1 and b"-C" in r.stderr and b"streaming" in r.stderr
    assert not os.path.exists(tmp_path / "out")


def test_cli_refuses_a_threshold_out_of_range(tmp_path):
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=40)
    r = subprocess.run([HUMID, "-C", "--consensus-min-q", "94", "-l", "/dev/null"] + files, capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--consensus-min-q" in r.stderr


def test_usage_names_the_flag():
    r = subprocess.run([HUMID, "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"-C" in r.stderr and b"consensus" in r.stderr and b"--consensus-min-q" in r.stderr


def parse_layers(files):
    """what --dump-consensus-input must hold: per file (off, bases, quals) from a Python parse"""
    recs = [read_fastq(f) for f in files]
    n = min(len(r) for r in recs)
    layers = [ct.flat([r[i][1].encode() for i in range(n)], [r[i][3].encode() for i in range(n)]) for r in recs]
    return n, [(off, b, q) for b, q, off in layers]


def dump_layers(files, tmp, env=None, extra=()):
    out = os.path.join(str(tmp), "cons.bin")
    e = dict(os.environ)
    e.update(env or {})
    subprocess.check_call([HUMID, "-l", "/dev/null", "--dump-consensus-input", out] + list(extra) + list(files), env=e,
                          timeout=120)
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], np.uint64)[0])
    at, layers = 8, []
    for _ in files:
        off = np.frombuffer(raw[at:at + 8 * (n + 1)], np.uint64)
        at += 8 * (n + 1)
        t = int(off[n])
        layers.append((off, np.frombuffer(raw[at:at + t], np.uint8), np.frombuffer(raw[at + t:at + 2 * t], np.uint8)))
        at += 2 * t
    assert at == len(raw)
    return n, layers


def same_layers(a, b):
    assert a[0] == b[0] and len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert all(np.array_equal(u, v) for u, v in zip(x, y))


@pytest.mark.parametrize("n_files", [1, 2])
def test_dump_consensus_input(n_files, tmp_path):
    """mapped and gzip inflated in memory; short reads (lengths 0 .. 7); 1, 3 and 8 workers"""
    from best_truth import rewrite_qualities
    files = synth_fastq(str(tmp_path / "in"), 3000, 7, n_files=n_files, read_len=40, short_frac=0.05, p_n=3e-3)
    rewrite_qualities(files, 7)
    want = parse_layers(files)
    assert want[0] == 3000 and len(set(np.diff(want[1][0][0]).tolist())) > 4
    for threads in ("1", "3", "8"):
        same_layers(dump_layers(files, tmp_path, {"HUMID_THREADS": threads}), want)
    same_layers(dump_layers(files, tmp_path, extra=["-C", "-Q"]), want)
    gz = []
    for f in files:
        gz.append(f + ".gz")
        with gzip.open(gz[-1], "wb") as fh:
            fh.write(open(f, "rb").read())
    for env in ({}, {"HUMID_THREADS": "3"}):
        same_layers(dump_layers(gz, tmp_path, env), want)
    # a file of a few records (below one worker's share) is held in memory too
    tiny = synth_fastq(str(tmp_path / "tiny"), 5, 3, n_files=n_files, read_len=40)
    same_layers(dump_layers(tiny, tmp_path, {"HUMID_THREADS": "8"}), parse_layers(tiny))
    # the streaming path holds no reads: refused
    r = subprocess.run([HUMID, "-l", "/dev/null", "--dump-consensus-input", str(tmp_path / "x.bin")] + files,
                       env=dict(os.environ, HUMID_HOST_SLOW="1"), capture_output=True, timeout=60)
    assert r.returncode == 1 and b"streaming" in r.stderr
