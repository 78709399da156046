"""-m gpu: the edit-distance (-e) search swept over every plan, shift and indel site.

The words are the placed pairs of tests/edit_truth.py (one edit in each damaged segment, at the first, last and an
interior position, every order of deletions and insertions, 4 and 2 letters, plus indels at the word's ends and at the
boundary between its two machine words); the truth is the all-pairs dynamic programme of the CPU oracle
(oracle.pyoracle.edit_adjacency_allpairs / lev_pairs), which shares nothing with the search.  Everything is compared
for equality.

  a. test_whole_path*    Dedup.run(edit=True) under every forced plan (d, s) and the automatic one
  b. test_join_by_join   humid_stage_pairs_edit share by share (one join per share)
  c. test_grouped*       run_grouped(edit=True) under forced plans: the group field stays put
  d. test_pieces         bucket_walk 1, 2, 5: runs of walk - 1 .. 2 walk + 1 equal keys, the long run first / last
  e. test_verifiers*     lev_band1 / lev_band2 / LevX<0> on the device on their own (tests/csrc/edit_harness.hip)

Key width of a plan = 2 bits x the nucleotides of its k = s - d untouched segments (the longest combination, cut to
64 bits); the joins take 32-bit keys up to 32 bits and 64-bit keys beyond.  Among the cases below:
  lev_band1 (d = 2, 3): (24, 2, 3) 1 x 8 nt = 16 bits and (24, 2, 6) 4 x 4 nt = 32 bits -> 32-bit keys;
                        (32, 2, 6) 6 + 6 + 5 + 5 nt = 44 bits and (64, 3, 6) 3 x 11 nt = 66 -> cut to 64 -> 64-bit keys
  lev_band2 (d = 4, 5): (24, 4, 5) 1 x 5 nt = 10 bits and (48, 4, 6) 2 x 8 nt = 32 bits -> 32-bit keys;
                        (64, 4, 6) 2 x 11 nt = 44 bits and (63, 4, 6) 11 + 11 nt = 44 bits -> 64-bit keys
  LevX<0>   (d >= 6):   every plain plan has k = 1 (s = d + 1 is the only legal s): (32, 6, 7) 5 nt = 10 bits,
                        (33, 7, 8) 5 nt = 10 bits -> 32-bit keys.  64-bit keys need the group field of a grouped run:
                        test_grouped_wide_group_field, 44 nt + 2^30 groups (15 nt = 30 bits) + 7 nt = 44 bits.
"""
import functools
import itertools
import json
import os

import numpy as np
import pytest

import humid_amd
from humid_amd.synth import synth_wide_words, synth_words
from oracle import pyoracle as orc

import edit_truth as et
from test_gpu_edit import check_edit

pytestmark = pytest.mark.gpu

# every legal (d, s): s = d + 1 .. with at most MAX_COMBOS = 20 combinations
DS = [(2, 3), (2, 4), (2, 5), (2, 6), (3, 4), (3, 5), (3, 6), (4, 5), (4, 6), (5, 6), (6, 7), (7, 8)]
N_NARROW = [8, 12, 16, 24, 31, 32]
N_WIDE = [33, 34, 48, 63, 64]
# d <= 5 at every word length; the many pairs of d = 6 (6 000 per length) and d = 7 (19 000) at the lengths where the
# word type, the one-nucleotide high word and the shortest segments (s = n) are met
N_OF_D = {6: [8, 16, 32, 33, 64], 7: [8, 32, 33]}
PAIRS_PER_RUN = 100            # 200 words: the all-pairs truth of a run costs (200^2 / 2) n^2 cells


def runs_per_test(n):
    return 40 if n <= 34 else 12


@functools.lru_cache(maxsize=2)
def packed_pairs(n, d, s):
    x, y, meta = et.all_pairs(1000 * n + 10 * d + s, n, d, s)
    return et.pack(x), et.pack(y), meta


def n_parts(n, d, s):
    runs = -(-et.n_placed(n, d, s) // PAIRS_PER_RUN)
    return -(-runs // runs_per_test(n))


WHOLE = [(n, d, s, part) for d, s in DS for n in N_OF_D.get(d, N_NARROW + N_WIDE) if s <= n
         for part in range(n_parts(n, d, s))]

_CTX = {}


@pytest.fixture(scope="module")
def forced():
    """contexts with plan_segments = s, made once"""
    def get(s, walk=None):
        if (s, walk) not in _CTX:
            dd = humid_amd.Dedup()
            dd.set_option("plan_segments", s)
            if walk is not None:
                dd.set_option("bucket_walk", walk)
            _CTX[(s, walk)] = dd
        return _CTX[(s, walk)]
    yield get
    for dd in _CTX.values():
        dd.close()
    _CTX.clear()


def edge_set(off, idx):
    off = np.asarray(off).astype(np.int64)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    idx = np.asarray(idx).astype(np.int64)
    keep = rows < idx
    return set(zip(rows[keep].tolist(), idx[keep].tolist()))


def describe(uw, n, pairs):
    return ["(%d, %d) %s %s d=%d" % (a, b, et.nt_string(uw[a], n), et.nt_string(uw[b], n),
                                    int(orc.lev_pairs(uw[a:a + 1], uw[b:b + 1], n)[0])) for a, b in sorted(pairs)[:4]]


def assert_adjacency(got, want, uw, n, what):
    goff, gidx = got
    woff, widx = want
    if np.array_equal(np.asarray(goff).astype(np.uint64), woff) and np.array_equal(gidx, widx):
        return
    g, w = edge_set(goff, gidx), edge_set(woff, widx)
    raise AssertionError("%s: %d pairs lost %s, %d pairs too many %s" %
                         (what, len(w - g), describe(uw, n, w - g), len(g - w), describe(uw, n, g - w)))


def run_and_compare(dd, words, n, d, what):
    """Dedup.run(edit=True) over `words` against the all-pairs truth; returns (adjacency, unique words)"""
    uw = et.unique_words(words)
    want = orc.edit_adjacency_allpairs(uw, n, d)
    _, _, sm = dd.run(words, np.zeros(len(words), np.uint8), word_nt=n, distance=d, edit=True)
    assert sm["unique"] == len(uw), what
    got = dd.adjacency()
    assert_adjacency(got, want, uw, n, what)
    assert sm["edges"] == len(want[1]) // 2, what
    return got, uw


def cat(a, b):
    return np.concatenate([a, b])


# ---- a. the whole path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d,s,part", WHOLE, ids=["n%d_d%d_s%d_p%d" % c for c in WHOLE])
def test_whole_path_forced_plan(forced, n, d, s, part):
    x, y, _ = packed_pairs(n, d, s)
    dd = forced(s)
    per = PAIRS_PER_RUN * runs_per_test(n)
    starts = range(part * per, min(len(x), (part + 1) * per), PAIRS_PER_RUN)
    found = 0
    for lo in starts:
        got, _ = run_and_compare(dd, cat(x[lo:lo + PAIRS_PER_RUN], y[lo:lo + PAIRS_PER_RUN]), n, d,
                                 "n=%d d=%d s=%d pairs %d.." % (n, d, s, lo))
        found += len(got[1])
    # (the parts are sized by an upper bound of the pairs: with segments of one or two nucleotides some placements
    # coincide, and the last part can be empty)
    assert found > 0 or len(starts) == 0


def noise_words(n, target, seed):
    """synth_words-style families (substitution errors) cut so that they hold `target` different words"""
    w, _ = (synth_wide_words if n > 32 else synth_words)(6 * target, seed, n, p_sub=5e-3, p_n=0.0)
    key = w if n <= 32 else w[:, 0].astype(object) * (1 << 64) + w[:, 1].astype(object)
    _, first = np.unique(key, return_index=True)
    return w[:np.sort(first)[target - 1] + 1]


# the automatic plan (s = 0): its choice follows the number of unique words -- about log4(U) nucleotides of key --
# so noise lifts U over 1024 and over 4096.  The truth is quadratic in U: 4096 words are affordable at 12 nt only,
# and there up to d = 4 (at d >= 5 most pairs of 12-nt words are neighbours).
AUTO = [(24, d, 1100) for d in (2, 3, 4, 5, 6, 7)] + [(12, d, 4200) for d in (2, 3, 4)] + \
       [(12, 2, 1100), (33, 2, 1100), (33, 4, 1100), (40, 6, 1100)]


@pytest.mark.parametrize("n,d,target", AUTO, ids=["n%d_d%d_u%d" % c for c in AUTO])
def test_whole_path_automatic_plan(n, d, target):
    plans = [s for dd_, s in DS if dd_ == d and s <= n]
    per = (100 if target > 4096 or n > 32 else 300) // len(plans)        # (the truth is quadratic in U)
    xs, ys = [], []
    for s in plans:
        x, y, _ = packed_pairs(n, d, s)
        pick = np.linspace(0, len(x) - 1, per).astype(int)
        xs += [x[pick]]
        ys += [y[pick]]
    words = np.concatenate(xs + ys + [noise_words(n, target, 40 + d)])
    dd = humid_amd.Dedup()
    try:
        _, uw = run_and_compare(dd, words, n, d, "auto plan n=%d d=%d" % (n, d))
        assert len(uw) > target
    finally:
        dd.close()


@pytest.mark.parametrize("n,d,s", [(24, 3, 5), (48, 3, 6), (24, 4, 5), (32, 6, 7)])
def test_cluster_ids_stay_tied_to_the_oracle(forced, n, d, s):
    """one forced-plan case per verifier through test_gpu_edit.check_edit: ids, flags, leaves, adjacency and clusters
    against the oracle's trie search (band 1 also on two-word words)"""
    x, y, _ = packed_pairs(n, d, s)
    pick = np.linspace(0, len(x) - 1, 150).astype(int)
    words = np.concatenate([x[pick], y[pick], x[pick[::3]]])
    check_edit(forced(s), words, np.zeros(len(words), np.uint8), n, d, False)
    check_edit(forced(s), words, np.zeros(len(words), np.uint8), n, d, True, deep=False)


# ---- b. join by join ------------------------------------------------------------------------------------
JOINS = [(n, d, s) for d, s in DS for n in ((8, 16, 24, 32) if d <= 4 else (16, 32)) if s <= n]
W_SHARES = 256                 # above every plan's number of joins (the largest seen: 125)


def census_line(rec):
    path = os.environ.get("HUMID_EDIT_CENSUS")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


@pytest.mark.parametrize("n,d,s", JOINS, ids=["n%d_d%d_s%d" % c for c in JOINS])
def test_join_by_join(n, d, s):
    """d <= 4: every placed pair, in runs of 400 pairs (a pair that only one offset vector finds is one of a dozen
    among 1 700); d >= 5: 400 pairs evenly sampled.  The shares of 2, 3 and 7 on the first run only."""
    import torch
    from humid_amd.sharded import HipStageOps
    x, y, _ = packed_pairs(n, d, s)
    if d <= 4:
        picks = [np.arange(lo, min(lo + 400, len(x))) for lo in range(0, len(x), 400)]
    else:
        picks = [np.linspace(0, len(x) - 1, 400).astype(int)]
    ops = HipStageOps(0)
    census = dict(n=n, d=d, s=s, pairs=0, pairs_with_one_finder=0)
    joins, sole = set(), set()
    try:
        ops.set_option("plan_segments", s)
        for run, pick in enumerate(picks):
            uw = et.unique_words(cat(x[pick], y[pick]))
            U = len(uw)
            woff, widx = orc.edit_adjacency_allpairs(uw, n, d)
            truth = np.asarray(sorted((a << 32) | b for a, b in edge_set(woff, widx)), np.uint64)
            g = torch.from_numpy(uw.view(np.int64)).to(ops.device)

            def share(rank, world):
                return ops.pairs_edit(g, n, d, rank, world).cpu().numpy().view(np.uint64).copy()

            whole = share(0, 1)
            for world in (W_SHARES, 2, 3, 7) if run == 0 else (W_SHARES,):
                shares = [share(r, world) for r in range(world)]
                for r, e in enumerate(shares):
                    where = "run %d, share %d of %d" % (run, r, world)
                    a, b = (e >> np.uint64(32)).astype(np.int64), (e & np.uint64(0xffffffff)).astype(np.int64)
                    bad = np.flatnonzero(~((a < b) & (b < U)))
                    assert len(bad) == 0, "%s: pair (%d, %d) out of order or range" % (where, a[bad[0]], b[bad[0]])
                    ue = np.unique(e)
                    ua, ub = (ue >> np.uint64(32)).astype(np.int64), (ue & np.uint64(0xffffffff)).astype(np.int64)
                    far = np.flatnonzero(orc.lev_pairs(uw[ua], uw[ub], n) > d)
                    assert len(far) == 0, "%s: %s further than %d" % (
                        where, describe(uw, n, [(int(ua[far[0]]), int(ub[far[0]]))]), d)
                assert np.array_equal(np.sort(np.concatenate(shares)), np.sort(whole)), \
                    "run %d: the shares of %d are not the whole list" % (run, world)
                if world == W_SHARES:
                    assert all(len(e) == 0 for e in shares[200:]), "a plan of 200 joins or more"
                    finders = {}
                    for r, e in enumerate(shares):
                        for v in np.unique(e).tolist():
                            finders.setdefault(v, []).append(r)
                    missing = set(truth.tolist()) - set(finders)
                    assert not missing, "run %d: no join finds %s" % (
                        run, describe(uw, n, [(v >> 32, v & 0xffffffff) for v in missing]))
                    joins |= {r for r, e in enumerate(shares) if len(e)}
                    sole |= {f[0] for f in finders.values() if len(f) == 1}
                    census["pairs"] += len(truth)
                    census["pairs_with_one_finder"] += sum(len(f) == 1 for f in finders.values())
            got = ops.unique_edges(torch.from_numpy(whole.view(np.int64)).to(ops.device), U).cpu().numpy().view(np.uint64)
            assert np.array_equal(got, truth), "run %d" % run
        census_line(dict(census, joins_with_pairs=len(joins), sole_finders=len(sole)))
    finally:
        ops.close()


# ---- c. grouped -------------------------------------------------------------------------------------------
def grouped_truth(words, groups, n, d):
    """the all-pairs adjacency taken per group, leaves in (group, word) order"""
    offs, idxs, base = [np.zeros(1, np.uint64)], [], 0
    for g in np.unique(groups):
        uw = et.unique_words(words[groups == g])
        off, idx = orc.edit_adjacency_allpairs(uw, n, d)
        offs.append(off[1:] + offs[-1][-1])
        idxs.append(idx + np.uint32(base))
        base += len(uw)
    return np.concatenate(offs), np.concatenate(idxs), base


def grouped_case(dd, x, y, ids, n_groups, n, d, what):
    """pairs [0, m) copied into every group; pairs [m, ..) split -- x into the first group, y into the second, and the
    other way round into the second and third: within d only if the group field is ignored"""
    m = len(x) * 3 // 4
    words = np.concatenate([x[:m], y[:m]] * 3 + [x[m:], y[m:], y[m:], x[m:]])
    groups = np.concatenate([np.full(2 * m, g, np.uint32) for g in ids] +
                            [np.full(len(x) - m, g, np.uint32) for g in (ids[0], ids[1], ids[1], ids[2])])
    woff, widx, u = grouped_truth(words, groups, n, d)
    _, _, sm = dd.run_grouped(words, groups, np.zeros(len(words), np.uint8), word_nt=n, n_groups=n_groups, distance=d,
                              edit=True)
    assert sm["unique"] == u, what
    goff, gidx = dd.adjacency()
    if not (np.array_equal(goff.astype(np.uint64), woff) and np.array_equal(gidx, widx)):
        g, w = edge_set(goff, gidx), edge_set(woff, widx)
        raise AssertionError("%s: %d pairs lost, %d too many (leaf indices in (group, word) order: lost %s, too many %s)"
                             % (what, len(w - g), len(g - w), sorted(w - g)[:4], sorted(g - w)[:4]))
    assert sm["edges"] == len(widx) // 2, what
    assert np.array_equal(np.unique(dd.leaves()["group"]), np.unique(groups))
    return len(widx)


GROUPED = [(n, d, s) for n in (16, 30, 44) for d, s in ((2, 3), (2, 6), (3, 4), (3, 6), (4, 5), (4, 6))]


@pytest.mark.parametrize("n,d,s", GROUPED, ids=["n%d_d%d_s%d" % c for c in GROUPED])
def test_grouped_forced_plan(forced, n, d, s):
    """16 and 30 nt + one group nucleotide: one-word internal words; 44 nt: two-word"""
    x, y, _ = packed_pairs(n, d, s)
    found = 0
    for lo in range(0, len(x), 100):
        found += grouped_case(forced(s), x[lo:lo + 100], y[lo:lo + 100], (0, 1, 2), 3, n, d,
                              "grouped n=%d d=%d s=%d pairs %d.." % (n, d, s, lo))
    assert found > 0


def test_grouped_wide_group_field(forced):
    """2^30 groups: a group field of 15 nucleotides in front of the 7-nt segment -- 44 key bits, the 64-bit joins with
    the bit-vector verifier (d = 6), which no plain run reaches; and with lev_band1 (d = 2, s = 3: 30 + 30 bits)"""
    for d, s in ((6, 7), (2, 3)):
        x, y, _ = packed_pairs(44, d, s)
        pick = np.linspace(0, len(x) - 1, 400).astype(int) if len(x) > 400 else np.arange(len(x))
        ids = (5, (1 << 29) + 12345, (1 << 30) - 1)
        for lo in range(0, len(pick), 200):
            assert grouped_case(forced(s), x[pick[lo:lo + 200]], y[pick[lo:lo + 200]], ids, 1 << 30, 44, d,
                                "2^30 groups d=%d pairs %d.." % (d, lo)) > 0


# ---- d. pieces ----------------------------------------------------------------------------------------------
def run_family(rng, n, d, seg, value, size):
    """`size` different words that hold `value` in segment seg = (start, length): one base word with up to d / 2
    substitutions, and now and then a deletion + insertion, outside that segment (members are mostly neighbours)"""
    start, ln = seg
    outside = [i for i in range(n) if not start <= i < start + ln]
    base = rng.integers(0, 4, size=n)
    base[start:start + ln] = value
    out = {}
    while len(out) < size:
        w = base.copy()
        for i in rng.choice(outside, size=int(rng.integers(1, d // 2 + 1)), replace=False):
            w[i] = (w[i] + int(rng.integers(1, 4))) % 4
        side = [i for i in outside if i < start] if rng.random() < 0.5 else [i for i in outside if i >= start + ln]
        if len(side) >= 3 and rng.random() < 0.4:                   # an indel pair on one side of the shared segment
            a, b = sorted(rng.choice(len(side), size=2, replace=False).tolist())
            part = w[side].tolist()
            del part[a]
            part.insert(b, int(rng.integers(0, 4)))
            w[side] = part
        out[tuple(w.tolist())] = w
    return list(out.values())


PIECES = [(24, 2), (24, 4), (24, 6), (64, 2), (40, 6)]      # (64, 2, s = 3): 22-nt segments, 64-bit keys; 40: W2 + u32


@pytest.mark.parametrize("walk", [1, 2, 5])
@pytest.mark.parametrize("n,d", PIECES, ids=["n%d_d%d" % c for c in PIECES])
def test_pieces(forced, n, d, walk):
    """s = d + 1: a join key is one whole segment.  Families that share one segment give runs of exactly walk - 1,
    walk, walk + 1, 2 walk and 2 walk + 1 equal keys in that segment's unshifted join (a run of walk + 1 is the
    shortest that k_edit_join hands to the pieces); the longest run holds the smallest key, then the largest, so that
    it ends at position U - 1 of the key order.  The shared segment is the first, a middle and the last one."""
    s = d + 1
    segs = et.segments(n, s)
    control = forced(s, 1024)
    dd = humid_amd.Dedup()
    try:
        dd.set_option("plan_segments", s)
        dd.set_option("bucket_walk", walk)
        for t in (0, s // 2, s - 1):
            for extreme in (0, 3):
                rng = np.random.default_rng(1000 * n + 100 * d + 10 * walk + t + extreme)
                lens = sorted({walk - 1, walk, walk + 1, 2 * walk, 2 * walk + 1} - {0})
                ln = segs[t][1]
                values = {tuple([extreme] * ln)}
                while len(values) < len(lens):
                    values.add(tuple(rng.integers(0, 4, size=ln).tolist()))
                values.discard(tuple([extreme] * ln))
                values = [tuple([extreme] * ln)] + sorted(values)        # the long run: the extreme key
                rows = []
                for size, v in zip(reversed(lens), values):
                    rows += run_family(rng, n, d, segs[t], np.asarray(v), size)
                noise = rng.integers(0, 4, size=(300 if n <= 32 else 120, n))
                taken = set(values)
                noise = [w for w in noise if tuple(w[segs[t][0]:segs[t][0] + ln].tolist()) not in taken]
                words = et.pack(np.asarray(rows + noise))
                what = "walk=%d n=%d d=%d shared segment %d, long run %s" % (walk, n, d, t, "first" if extreme == 0 else "last")
                got, uw = run_and_compare(dd, words, n, d, what)
                # the runs really are what the test says: segment t's values in the unique words
                seg_of = [tuple(r) for r in np.asarray(rows + noise)[:, segs[t][0]:segs[t][0] + ln].tolist()]
                counts = sorted(seg_of.count(v) for v in values)
                assert counts == lens, (what, counts, lens)
                assert (max(seg_of) if extreme == 3 else min(seg_of)) == values[0], what
                control.run(words, np.zeros(len(words), np.uint8), word_nt=n, distance=d, edit=True)
                ctl = control.adjacency()
                assert np.array_equal(got[0], ctl[0]) and np.array_equal(got[1], ctl[1]), what + ": bucket_walk 1024 differs"
                assert len(got[1]) > 0
    finally:
        dd.set_option("bucket_walk", 1024)
        dd.close()


# ---- e. the verifiers on their own ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    import prims_harness
    return prims_harness.load_edit()


def verify(harness, x, y, n, what):
    x = np.ascontiguousarray(x, np.uint64)
    y = np.ascontiguousarray(y, np.uint64)
    out = np.zeros((len(x), 3), np.uint32)
    rc = harness.eh_verify(x.ctypes.data, y.ctypes.data, len(x), n, out.ctypes.data)
    assert rc == 0, rc
    true = orc.lev_pairs(x, y, n).astype(np.uint32)
    for col, cap, name in ((0, 4, "lev_band1"), (1, 6, "lev_band2"), (2, 1 << 30, "LevX<0>")):
        bad = np.flatnonzero(np.minimum(out[:, col], cap) != np.minimum(true, cap))
        assert len(bad) == 0, "%s, %s: %s %s gives %d, the distance is %d (%d pairs differ)" % (
            what, name, et.nt_string(x[bad[0]], n), et.nt_string(y[bad[0]], n), out[bad[0], col], true[bad[0]], len(bad))
    return true


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_verifiers_every_pair_of_small_words(harness, n):
    w = np.arange(4 ** n, dtype=np.uint64)
    true = verify(harness, np.repeat(w, len(w)), np.tile(w, len(w)), n, "every pair at n=%d" % n)
    assert int(true.max()) == n


def random_pairs(rng, n, count):
    """x against x shifted by -2 .. 2 positions (indel pairs at the ends) with 0 .. 6 substitutions; every tenth
    pair two unrelated words; a tenth over two letters"""
    x = rng.integers(0, 4, size=(count, n))
    x[::10] = rng.integers(0, 2, size=x[::10].shape)
    y = x.copy()
    shift = rng.integers(-2, 3, size=count)
    for k in (-2, -1, 1, 2):
        rows = shift == k
        y[rows] = np.roll(x[rows], k, axis=1)
    subs = rng.random((count, n)) < (rng.integers(0, 7, size=count) / n)[:, None]
    y = np.where(subs, (y + rng.integers(1, 4, size=y.shape)) % 4, y)
    y[5::10] = rng.integers(0, 4, size=y[5::10].shape)
    return x, y


@pytest.mark.parametrize("n", [6, 7, 15, 16, 17, 31, 32, 33, 34, 47, 48, 63, 64])
def test_verifiers_generated_pairs(harness, n):
    """200 000 pairs: the placed pairs of every plan that fits n, and random ones"""
    xs, ys, have = [], [], 0
    for d, s in DS:
        if s <= n and d <= 5:
            x, y, _ = et.all_pairs(7 * n + d + s, n, d, s)
            xs.append(x)
            ys.append(y)
            have += len(x)
    x, y = random_pairs(np.random.default_rng(n), n, 200_000 - have)
    x, y = np.concatenate(xs + [x]), np.concatenate(ys + [y])
    assert len(x) == 200_000
    true = verify(harness, et.pack(x), et.pack(y), n, "generated pairs at n=%d" % n)
    hist = np.bincount(true, minlength=8)
    assert all(hist[:min(n, 7)] > 100), hist       # every distance the bands decide on is there


@pytest.mark.parametrize("n", [32, 33, 64])
def test_verifiers_special_words(harness, n):
    rng = np.random.default_rng(n)
    r = rng.integers(0, 4, size=(6, n))
    rows = [np.zeros(n, int), np.full(n, 3), np.arange(n) % 2, (np.arange(n) + 1) % 2, 3 * (np.arange(n) % 2),
            np.arange(n) % 4, (np.arange(n) // 2) % 4] + list(r) + [v[::-1] for v in r]
    rows = np.asarray(rows)
    a, b = zip(*itertools.product(range(len(rows)), repeat=2))
    true = verify(harness, et.pack(rows[list(a)]), et.pack(rows[list(b)]), n, "special words at n=%d" % n)
    assert int(true.max()) == n                    # all-A against all-T
