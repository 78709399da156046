"""No GPU: the two truths of tests/optical_truth.py against each other and against answers worked out by hand, and the
position parser of `humid -O` through --dump-positions (both header styles, text after a space, short names, fields
that are no numbers, the tile and lane limits, the mapped fast path against the streaming reader)."""
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID
from humid_amd.synth import synth_fastq

import optical_truth as ot

NT, NR = ot.NO_TILE, ot.NO_READ


def both(cid, keep, tile, x, y, D, C):
    a = ot.optical_sweep(cid, keep, tile, x, y, D, C)
    ot.assert_same(a, ot.optical_loop(cid, keep, tile, x, y, D, C), "the two truths")
    return a


def one_cluster(x, y, D, tile=None, keep_at=0):
    n = len(x)
    keep = np.zeros(n, np.uint8)
    keep[keep_at] = 1
    return both(np.ones(n, np.uint32), keep, np.full(n, 7, np.uint32) if tile is None else tile, x, y, D, 1)


def random_case(seed, n, n_clusters, D, side):
    rng = np.random.default_rng(seed)
    cid = rng.integers(0, n_clusters + 1, n).astype(np.uint32)
    cid[:n_clusters] = np.arange(1, n_clusters + 1)                    # every cluster has a read
    rng.shuffle(cid)
    keep = np.zeros(n, np.uint8)
    for c in range(1, n_clusters + 1):
        keep[rng.choice(np.flatnonzero(cid == c))] = 1
    keep[cid == 0] = rng.integers(0, 2, int((cid == 0).sum()))        # (ignored)
    tile, x, y = ot.make_positions(cid, keep, seed + 1, D=D, n_tiles=3, side=side, p_near=0.3, p_none=0.05)
    return cid, keep, tile, x, y


@pytest.mark.parametrize("seed,n,n_clusters,D,side", [(1, 400, 12, 100, 2000), (2, 900, 5, 40, 600), (3, 257, 257, 5, 50),
                                                       (4, 600, 1, 30, 900), (5, 300, 40, 0, 8)])
def test_the_two_truths_agree_on_random_inputs(seed, n, n_clusters, D, side):
    cid, keep, tile, x, y = random_case(seed, n, n_clusters, D, side)
    opt, org, pc, s = both(cid, keep, tile, x, y, D, n_clusters)
    m = cid != 0
    assert s["members"] == int(m.sum()) and s["duplicates"] == s["members"] - n_clusters
    assert np.all(opt[~m] == 0) and np.all(org[~m] == NR)
    assert np.all(cid[org[m]] == cid[m]) and np.all(opt[org[m]] == 0)            # an origin lies in the read's cluster
    assert np.all(opt[(keep != 0) & m] == 0)                                       # a kept read is never optical
    assert s["optical"] == int(opt.sum()) <= s["duplicates"]
    if seed in (1, 2, 4):
        assert s["optical"] > 0 and s["groups"] > 0 and s["largest_group"] >= 2


def test_thresholds_by_hand():
    D = 10
    u = np.array
    # |dx| and |dy| at D and at D + 1, each alone
    for dx, dy, close in ((D, 0, 1), (D + 1, 0, 0), (0, D, 1), (0, D + 1, 0), (D, D, 1), (D + 1, D + 1, 0)):
        opt, org, pc, s = one_cluster(u([100, 100 + dx]), u([50, 50 + dy]), D)
        assert opt.tolist() == [0, close] and org.tolist() == [0, 0 if close else 1] and pc.tolist() == [close]
        assert s == dict(n_clusters=1, members=2, duplicates=1, optical=close, groups=close, largest_group=1 + close)
    # D = 0: only equal positions; D = 0xffffffff: everything on a tile
    assert one_cluster(u([5, 5, 6]), u([9, 9, 9]), 0)[0].tolist() == [0, 1, 0]
    assert one_cluster(u([0, 0xffffffff, 7]), u([0xffffffff, 0, 7]), 0xffffffff)[0].tolist() == [0, 1, 1]
    # the wrap case: 0 and 0xffffffff are 2^32 - 1 apart, not 1
    opt, org, pc, s = one_cluster(u([0, 0xffffffff, 0xfffffff0, 3]), u([0, 0xffffffff, 0xfffffff8, 0xffffffff]), 16)
    assert opt.tolist() == [0, 0, 1, 0] and org.tolist() == [0, 1, 1, 3] and s["groups"] == 1
    # tile and x with bit 31 set
    t31 = np.full(3, 0x80000001, np.uint32)
    assert one_cluster(u([0x80000000, 0x80000005, 0x7ffffffb]), u([1, 1, 1]), 5, tile=t31)[0].tolist() == [0, 1, 1]
    # same position: another tile, another cluster, no tile at all
    assert one_cluster(u([4, 4]), u([4, 4]), 50, tile=u([7, 8], np.uint32))[0].tolist() == [0, 0]
    opt, org, pc, s = both(u([1, 2], np.uint32), u([1, 1], np.uint8), u([7, 7]), u([4, 4]), u([4, 4]), 50, 2)
    assert opt.tolist() == [0, 0] and s["optical"] == 0 and s["largest_group"] == 1
    opt, org, pc, s = one_cluster(u([4, 4]), u([4, 4]), 50, tile=u([NT, NT], np.uint32))
    assert opt.tolist() == [0, 0] and org.tolist() == [0, 1]
    # reads without a cluster carry the coordinates of members and keep == 1: ignored
    opt, org, pc, s = both(u([0, 1, 0, 1], np.uint32), u([1, 1, 1, 0], np.uint8), u([7] * 4), u([4] * 4), u([4] * 4), 50, 1)
    assert opt.tolist() == [0, 0, 0, 1] and org.tolist() == [NR, 1, NR, 1] and s["members"] == 2 and s["optical"] == 1


def test_transitivity_by_hand():
    D = 25
    x = np.arange(1000) * D
    opt, org, pc, s = one_cluster(x, np.zeros(1000, np.int64), D, keep_at=999)
    assert s["groups"] == 1 and s["largest_group"] == 1000 and s["optical"] == 999 and np.all(org == 999)
    x[500:] += 1                                                         # one step of D + 1
    opt, org, pc, s = one_cluster(x, np.zeros(1000, np.int64), D, keep_at=999)
    assert s["groups"] == 2 and s["largest_group"] == 500 and s["optical"] == 998
    assert np.all(org[:500] == 0) and np.all(org[500:] == 999)
    gx, gy = np.meshgrid(np.arange(40) * D, np.arange(40) * D)
    perm = np.random.default_rng(3).permutation(1600)
    opt, org, pc, s = one_cluster(gx.ravel()[perm], gy.ravel()[perm], D, keep_at=77)
    assert s["groups"] == 1 and s["largest_group"] == 1600 and np.all(org == 77)


def test_origin_by_hand():
    # cluster 1: reads 0 1 2 close together with the kept read 2; reads 3 4 close together without it; cluster 2:
    # its kept read 5 alone, 6 and 7 far from it and close to each other
    cid = np.array([1, 1, 1, 1, 1, 2, 2, 2], np.uint32)
    keep = np.array([0, 0, 1, 0, 0, 1, 0, 0], np.uint8)
    x = np.array([10, 12, 14, 900, 905, 10, 500, 501])
    y = np.array([10, 12, 14, 900, 905, 10, 500, 501])
    opt, org, pc, s = both(cid, keep, np.full(8, 3), x, y, 8, 2)
    assert org.tolist() == [2, 2, 2, 3, 3, 5, 6, 6] and opt.tolist() == [1, 1, 0, 0, 1, 0, 0, 1]
    assert pc.tolist() == [3, 1]
    assert s == dict(n_clusters=2, members=8, duplicates=6, optical=4, groups=3, largest_group=3)


def test_empty_inputs():
    z = np.zeros(0, np.uint32)
    for t in (ot.optical_sweep(z, z, z, z, z, 5, 0), ot.optical_loop(z, z, z, z, z, 5, 3)):
        assert all(v == 0 for v in t[3].values()) and len(t[0]) == 0
    opt, org, pc, s = both(np.zeros(3, np.uint32), np.ones(3, np.uint8), [1, 1, 1], [1, 1, 1], [1, 1, 1], 5, 0)
    assert opt.tolist() == [0, 0, 0] and org.tolist() == [NR] * 3 and all(v == 0 for v in s.values())


# ---- the parser of the command line ----------------------------------------------------------------------------------
def dump_positions(files, tmp, env=None):
    out = os.path.join(str(tmp), "pos.bin")
    e = dict(os.environ)
    e.update(env or {})
    subprocess.check_call([HUMID, "-l", os.path.join(str(tmp), "log.txt"), "--dump-positions", out] + list(files), env=e)
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:8], np.uint64)[0])
    assert len(raw) == 8 + 12 * n
    a = np.frombuffer(raw[8:], np.uint32).reshape(3, n)
    return a[0], a[1], a[2]


HEADERS = [
    ("@M1:7:FC:3:1101:4678:1110_AGTA 1:N:0", (3 << 24 | 1101, 4678, 1110)),
    ("@M1:7:FC:3:1101:4678:1110:AGTA", (3 << 24 | 1101, 4678, 1110)),
    ("@M1:7:FC:3:1101:4678:1110", (3 << 24 | 1101, 4678, 1110)),
    ("@M1:7:FC:3:1101:4678:1110 2:N:0:1:2:3:4", (3 << 24 | 1101, 4678, 1110)),
    ("@M1:7:FC:3:1101:4678 1:1:1", (NT, 0, 0)),                        # the fields after a space do not count
    ("@M1:7:FC:3:1101:4678", (NT, 0, 0)),
    ("@r17_ACGT", (NT, 0, 0)),
    ("@M1:7:FC:3:1101:4678:", (NT, 0, 0)),
    ("@M1:7:FC:3:1101:4678:_AGTA", (NT, 0, 0)),
    ("@M1:7:FC:x:1101:4678:1110", (NT, 0, 0)),
    ("@M1:7:FC:3:11a1:4678:1110", (NT, 0, 0)),
    ("@M1:7:FC:3:1101:46 78:1110", (NT, 0, 0)),
    ("@M1:7:FC:3:1101:-4:1110", (NT, 0, 0)),
    ("@M1:7:FC:3::4678:1110", (NT, 0, 0)),
    ("@M1:7:FC:3:16777215:1:2", (3 << 24 | 16777215, 1, 2)),
    ("@M1:7:FC:3:16777216:1:2", (NT, 0, 0)),
    ("@M1:7:FC:254:5:1:2", (254 << 24 | 5, 1, 2)),
    ("@M1:7:FC:255:5:1:2", (NT, 0, 0)),
    ("@M1:7:FC:0:0:0:0", (0, 0, 0)),
    ("@M1:7:FC:1:1:4294967295:4294967295x", (1 << 24 | 1, 0xffffffff, 0xffffffff)),
    ("@M1:7:FC:1:1:4294967296:1", (NT, 0, 0)),
    ("@M1:7:FC:1:1:1:99999999999999999999999", (NT, 0, 0)),
    ("@", (NT, 0, 0)),
]


def write_fastq(path, headers):
    with open(path, "w") as fh:
        for h in headers:
            fh.write("%s\nACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIII\n" % h)
    return [path]


@pytest.mark.parametrize("env", [{}, {"HUMID_HOST_SLOW": "1"}], ids=["mapped", "streaming"])
def test_header_cases(env, tmp_path):
    files = write_fastq(str(tmp_path / "h.fastq"), [h for h, _ in HEADERS])
    tile, x, y = dump_positions(files, tmp_path, env)
    for k, (h, want) in enumerate(HEADERS):
        assert (int(tile[k]), int(x[k]), int(y[k])) == want == ot.parse_name(h), h


@pytest.mark.parametrize("style,n_files", [("_", 1), (":", 1), ("_", 2)])
def test_rewritten_files_fast_path_equals_streaming_path(style, n_files, tmp_path):
    files = synth_fastq(str(tmp_path / "in"), 1500, 23, n_files=n_files, umi_len=8, read_len=40, header_style=style)
    umis = [l.split(" ")[0].split(style)[-1] for l in open(files[0]).read().split("\n")[0::4] if l]
    want = ot.rewrite_headers(files, 5, style)
    names = [l for l in open(files[0]).read().split("\n")[0::4] if l]
    assert [nm.split(" ")[0].split(style)[-1] for nm in names] == umis          # the UMI survives the rewriting
    assert int((want[0] == NT).sum()) > 0
    fast = dump_positions(files, tmp_path)
    slow = dump_positions(files, tmp_path, {"HUMID_HOST_SLOW": "1"})
    for a, b, c in zip(want, fast, slow):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert [ot.parse_name(nm) for nm in names] == [tuple(int(v[i]) for v in want) for i in range(len(names))]
