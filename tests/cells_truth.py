"""Truth of the whitelist taken from the data (include/humid_hip.h, humid_whitelist_discover), literally from the
definition, in numpy and Python integers.  Shares nothing with the product.

discover(keys, filtered, k, mode, param, merge_ratio) -> (cells u64[], reads u32[], summary dict, (hist_n u64[],
hist_barcodes u64[])).  The merge exists twice: through the 3 k variants of every selected barcode looked up in a dict
(the default), and over all pairs of selected barcodes (all_pairs=True, for small selections); the host tests hold
them against each other."""
import numpy as np

U64 = np.uint64
TOP, EXPECTED, MIN_READS = 0, 1, 2
ALL_T = 0xFFFFFFFFFFFFFFFF
FIELDS = ("usable", "invalid_reads", "distinct", "selected", "merged", "cells", "threshold_reads", "top_reads", "reads_in_cells")


def one_apart(v, w):
    """v and w differ in exactly one nucleotide"""
    x = v ^ w
    return bin((x | (x >> 1)) & 0x5555555555555555).count("1") == 1


def counts_in_order(keys, filtered, k):
    """(usable, invalid, barcodes in the ORDER, their counts): by count descending, barcode value ascending"""
    keys = np.asarray(keys, U64)
    use = np.asarray(filtered) == 0
    uk = keys[use]
    usable = int(use.sum())
    if k < 32:
        ok = uk < U64(1 << (2 * k))
        invalid = int((~ok).sum())
        uk = uk[ok]
    else:
        invalid = 0
    vals, cnt = np.unique(uk, return_counts=True)
    order = np.lexsort((vals, -cnt.astype(np.int64)))              # (the last key is the primary one)
    return usable, invalid, [int(v) for v in vals[order]], [int(c) for c in cnt[order]]


def select(okeys, ocnt, mode, param):
    """the number of ranks in S"""
    G = len(okeys)
    assert param >= 1
    if G == 0:
        return 0
    if mode == TOP:
        return min(param, G)
    if mode == EXPECTED:
        b = min((param + 50) // 100, G - 1)
        m = ocnt[b]
        return sum(1 for n in ocnt if 10 * n >= m)
    if mode == MIN_READS:
        return sum(1 for n in ocnt if n >= param)
    raise ValueError(mode)


def merged_variants(skeys, scnt, k, ratio):
    """the error barcodes of S (given in the ORDER), through the 3 k variants of each"""
    rank = {v: r for r, v in enumerate(skeys)}
    gone = set()
    for r, w in enumerate(skeys):
        for i in range(k):
            for x in (1, 2, 3):
                v = w ^ (x << (2 * i))
                rv = rank.get(v)
                if rv is not None and rv < r and scnt[rv] >= ratio * scnt[r]:
                    gone.add(w)
    return gone


def merged_all_pairs(skeys, scnt, k, ratio):
    """the same over all pairs (v before w in the ORDER)"""
    gone = set()
    for r, w in enumerate(skeys):
        for rv in range(r):
            if one_apart(skeys[rv], w) and scnt[rv] >= ratio * scnt[r]:
                gone.add(w)
                break
    return gone


def discover(keys, filtered, k, mode, param, merge_ratio=0, all_pairs=False):
    usable, invalid, okeys, ocnt = counts_in_order(keys, filtered, k)
    G = len(okeys)
    n_sel = select(okeys, ocnt, mode, int(param))
    skeys, scnt = okeys[:n_sel], ocnt[:n_sel]
    gone = set()
    if merge_ratio >= 1:
        gone = (merged_all_pairs if all_pairs else merged_variants)(skeys, scnt, k, int(merge_ratio))
    kept = sorted((v, n) for v, n in zip(skeys, scnt) if v not in gone)
    cells = np.asarray([v for v, _ in kept], U64)
    reads = np.asarray([n for _, n in kept], np.uint32)
    summary = dict(usable=usable, invalid_reads=invalid, distinct=G, selected=n_sel, merged=len(gone), cells=len(kept),
                   threshold_reads=scnt[-1] if n_sel else 0, top_reads=ocnt[0] if G else 0,
                   reads_in_cells=int(sum(n for _, n in kept)))
    hn, hb = np.unique(np.asarray(ocnt, U64), return_counts=True)
    return cells, reads, summary, (hn.astype(U64), hb.astype(U64))


# ---- generators ------------------------------------------------------------------------------------------------------
def random_barcodes(rng, n, k, apart=True):
    """n distinct k-nucleotide barcodes; apart: no two of them one substitution from each other"""
    out, seen = [], set()
    while len(out) < n:
        v = int(rng.integers(0, 1 << 62)) & ((1 << (2 * k)) - 1) if k < 32 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        if v in seen:
            continue
        if apart and any((v ^ (x << (2 * i))) in seen for i in range(k) for x in (1, 2, 3)):
            continue
        seen.add(v)
        out.append(v)
    return out


def substitute(rng, v, k):
    """v with one nucleotide replaced by another"""
    return v ^ (int(rng.integers(1, 4)) << (2 * int(rng.integers(0, k))))


def planted(rng, k, n_cells, first_reads, growth, p_err, n_ambient, p_filt=0.05, shuffle=True):
    """n_cells cells whose reads grow geometrically from first_reads by the factor `growth`, every read's barcode with
    probability p_err one substitution off, n_ambient more barcodes of 1 .. 3 reads, filtered reads (with keys that
    must not be read: all-ones) interleaved with probability p_filt.  Returns (keys u64[], filtered u8[], cells)."""
    cells = random_barcodes(rng, n_cells, k)
    reads = []
    for i, v in enumerate(cells):
        n = int(first_reads * growth ** i)
        for _ in range(n):
            reads.append(substitute(rng, v, k) if rng.random() < p_err else v)
    for v in random_barcodes(rng, n_ambient, k, apart=False):
        reads += [v] * int(rng.integers(1, 4))
    keys = np.asarray(reads, U64)
    if shuffle:
        keys = keys[rng.permutation(len(keys))]
    filt = (rng.random(len(keys)) < p_filt).astype(np.uint8)
    keys = np.where(filt != 0, U64(ALL_T), keys)
    return keys, filt, cells


def from_counts(pairs, rng=None, filtered_between=0):
    """reads of an explicit table [(barcode, reads), ...]; rng: shuffled; filtered_between: that many filtered reads in
    front of every barcode's reads"""
    keys, filt = [], []
    for v, n in pairs:
        keys += [ALL_T] * filtered_between + [v] * n
        filt += [1] * filtered_between + [0] * n
    keys, filt = np.asarray(keys, U64), np.asarray(filt, np.uint8)
    if rng is not None and len(keys):
        p = rng.permutation(len(keys))
        keys, filt = keys[p], filt[p]
    return keys, filt
