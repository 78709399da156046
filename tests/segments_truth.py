"""Two independent truths of the segmented barcode whitelist correction (include/humid_hip.h,
humid_whitelist_set_segments) in numpy / plain Python, and the generators the segment tests share.

TEST HELPER, never product code.

correct():            per segment and distinct subkey, a set lookup of the subkey and of its 3 L one-substitution
                      variants; the classes of a read's segments are then combined by the rule of the header.
correct_all_pairs():  per distinct key, the Hamming distance of every segment to that segment of EVERY member of the
                      product list W_0 x ... x W_(S-1): no variants, no sets, no per-segment lists.  The product and the
                      keys must be small.
Both return (key_out u64[N], status u8[N], counts u64[5], seg_counts u64[S, 4], inexact_hist u64[S + 1]).
"""
import itertools

import numpy as np

import whitelist_truth as wt

U64 = np.uint64
FILTERED, EXACT, CORRECTED, AMBIGUOUS, UNMATCHED = range(5)
LOW = 0x5555555555555555


def shifts(seg_nt):
    """bits below every segment: segment 0 is the most significant"""
    k = sum(seg_nt)
    out, below = [], k
    for nt in seg_nt:
        below -= nt
        out.append(2 * below)
    return out


def compose(subkeys, seg_nt):
    """subkeys: one integer array per segment -> the keys"""
    key = np.zeros(len(subkeys[0]), U64)
    for sub, sh in zip(subkeys, shifts(seg_nt)):
        key |= np.asarray(sub, U64) << U64(sh)
    return key


def product_list(lists, seg_nt):
    """W_0 x ... x W_(S-1) as keys (every combination of the distinct entries)"""
    grids = np.meshgrid(*[np.unique(np.asarray(w, U64)) for w in lists], indexing="ij")
    return compose([g.ravel() for g in grids], seg_nt)


def _combine(keys, filtered, seg_nt, max_inexact, cls, rep):
    """cls / rep: int[N, S] class (0 exact .. 3 unmatched) and replacement of every segment of every read (rows of
    filtered reads and of keys >= 4^K are not read)"""
    keys = np.asarray(keys, U64)
    f = np.asarray(filtered, np.uint8)
    n, S, K = len(f), len(seg_nt), sum(seg_nt)
    if max_inexact is None:
        max_inexact = S
    usable = f == 0
    valid = usable & ((keys >> U64(2 * K)) == 0 if K < 32 else True)
    m = (cls != 0).sum(1)
    worst = cls.max(1) if S else np.zeros(n, np.int64)
    status = np.full(n, FILTERED, np.uint8)
    status[usable] = UNMATCHED
    ok = valid & (m <= max_inexact)
    status[ok] = (EXACT + worst[ok]).astype(np.uint8)
    out = np.where(usable, keys, U64(0))
    fixed = status == CORRECTED
    out[fixed] = compose([rep[fixed, s] for s in range(S)], seg_nt)
    seg_counts = np.zeros((S, 4), U64)
    for s in range(S):
        seg_counts[s] = np.bincount(cls[valid, s], minlength=4)
    hist = np.bincount(m[valid], minlength=S + 1).astype(U64)
    return out, status, np.bincount(status, minlength=5).astype(U64), seg_counts, hist


def correct(keys, filtered, lists, seg_nt, max_inexact=None):
    """the definition through set lookups, segment by segment"""
    keys = np.asarray(keys, U64)
    n, S = len(keys), len(seg_nt)
    cls, rep = np.zeros((n, S), np.int64), np.zeros((n, S), np.int64)
    for s, (w, nt, sh) in enumerate(zip(lists, seg_nt, shifts(seg_nt))):
        W = set(int(x) for x in np.asarray(w, U64))
        sub = ((keys >> U64(sh)) & U64(4 ** nt - 1)).astype(np.int64)
        uniq, inv = np.unique(sub, return_inverse=True)
        c_u, r_u = np.zeros(len(uniq), np.int64), uniq.copy()
        for i, k in enumerate(int(x) for x in uniq):
            if k in W:
                continue
            hits = [k ^ (x << (2 * p)) for p in range(nt) for x in (1, 2, 3) if k ^ (x << (2 * p)) in W]
            c_u[i] = 1 if len(hits) == 1 else 2 if hits else 3
            if len(hits) == 1:
                r_u[i] = hits[0]
        cls[:, s], rep[:, s] = c_u[inv], r_u[inv]
    return _combine(keys, filtered, seg_nt, max_inexact, cls, rep)


def correct_all_pairs(keys, filtered, lists, seg_nt, max_inexact=None):
    """the definition through the distance of every distinct key to every member of the product list, split by
    segment: segment s of the key is exact when some member has distance 0 there, else its candidates are the distinct
    values of that segment among the members at distance 1 there"""
    keys = np.asarray(keys, U64)
    f = np.asarray(filtered, np.uint8)
    S, K = len(seg_nt), sum(seg_nt)
    members = [int(x) for x in product_list(lists, seg_nt)]
    sh = shifts(seg_nt)
    masks = [(4 ** nt - 1) << b for nt, b in zip(seg_nt, sh)]
    n = len(keys)
    cls, rep = np.zeros((n, S), np.int64), np.zeros((n, S), np.int64)
    seen = {}
    for r in range(n):
        k = int(keys[r])
        if f[r] or (K < 32 and k >> (2 * K)):
            continue
        if k not in seen:
            zero, near = [False] * S, [set() for _ in range(S)]
            for w in members:
                x = k ^ w
                d = (x | (x >> 1)) & LOW
                for s in range(S):
                    ds = bin(d & masks[s]).count("1")
                    if ds == 0:
                        zero[s] = True
                    elif ds == 1:
                        near[s].add((w & masks[s]) >> sh[s])
            c = [0 if zero[s] else 1 if len(near[s]) == 1 else 2 if near[s] else 3 for s in range(S)]
            p = [min(near[s]) if c[s] == 1 else (k & masks[s]) >> sh[s] for s in range(S)]
            seen[k] = (c, p)
        cls[r], rep[r] = seen[k]
    return _combine(keys, f, seg_nt, max_inexact, cls, rep)


def make_lists(rng, sizes, seg_nt):
    """one list per segment as whitelist_truth.whitelist_with_neighbours makes them: random entries, some pairs at
    distance 2 (their midpoints are ambiguous) and one at distance 1.  A size of 4^L or more gives all 4^L values."""
    return [np.arange(4 ** nt, dtype=U64) if n >= 4 ** nt else wt.whitelist_with_neighbours(rng, n, nt)
            for n, nt in zip(sizes, seg_nt)]


def make_keys(rng, lists, seg_nt, n, p1=0.08, p2=0.04, p3=0.02, pr=0.02, p_high=0.01, p_filt=0.03):
    """The generator of the issue, modelled on whitelist_truth.make_keys: n keys drawn from the product of the lists;
    about 8 % of them with one substitution in one segment, 4 % with one substitution in each of two segments, 2 % with
    two substitutions in one segment, 2 % random; planted midpoints of list pairs at distance 2 in one segment (that
    segment is ambiguous); keys >= 4^K (K < 32); filtered reads carrying garbage keys.
    Returns (keys u64[n], filtered u8[n])."""
    S, K = len(seg_nt), sum(seg_nt)
    subs = [np.asarray(w, U64)[rng.integers(0, len(w), size=n)] if n else np.zeros(0, U64) for w in lists]
    u = rng.random(n)
    one = u < p1
    two = (u >= p1) & (u < p1 + p2)
    dbl = (u >= p1 + p2) & (u < p1 + p2 + p3)
    rnd = (u >= p1 + p2 + p3) & (u < p1 + p2 + p3 + pr)
    first = rng.integers(0, S, size=n)
    second = (first + 1 + rng.integers(0, max(S - 1, 1), size=n)) % S if S > 1 else first
    for s in range(S):
        sel = np.flatnonzero(((one | two | dbl) & (first == s)) | (two & (second == s) & (S > 1)))
        subs[s][sel] = wt.substitute(rng, subs[s][sel], seg_nt[s])
        sel = np.flatnonzero(dbl & (first == s))
        subs[s][sel] = wt.substitute(rng, subs[s][sel], seg_nt[s])
    if n >= 8:
        for s in range(S):
            mids = wt.midpoints(lists[s], seg_nt[s])
            if len(mids):
                at = rng.choice(n, size=min(len(mids), max(n // (50 * S), 2)), replace=False)
                subs[s][at] = mids[rng.integers(0, len(mids), size=len(at))]
    keys = compose(subs, seg_nt)
    sel = np.flatnonzero(rnd)
    keys[sel] = wt.random_barcodes(rng, len(sel), K)
    if K < 32:
        sel = np.flatnonzero(rng.random(n) < p_high)
        keys[sel] |= U64(1) << rng.integers(2 * K, 64, size=len(sel)).astype(U64)
    filt = (rng.random(n) < p_filt).astype(np.uint8)
    sel = np.flatnonzero(filt)
    keys[sel] = rng.integers(0, 1 << 64, size=len(sel), dtype=U64)
    return keys.astype(U64, copy=False), filt


def assert_covers(truth, statuses=(0, 1, 2, 3, 4), inexact=(0, 1, 2)):
    """the input exercises what the test is about: these statuses occur in the truth, and reads with these numbers of
    segments that are not exact"""
    assert wt.status_set(truth[1]) >= set(statuses), (wt.status_set(truth[1]), statuses)
    assert all(int(truth[4][m]) > 0 for m in inexact), (truth[4], inexact)


def assert_same(truth, got, names=("key_out", "status", "counts", "seg_counts", "inexact_hist")):
    for name, a, b in zip(names, truth, got):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
