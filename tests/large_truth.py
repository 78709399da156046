"""Exact CPU truth of single-GPU passes over tens of millions of reads (tests/test_gpu_large.py), where the oracle's
trie -- one thread, one walk per read -- takes minutes per case.

TEST HELPER, never product code: numpy and the C oracle only, no device code.

PrefixTruth     one stable argsort of the usable reads of a read set; every prefix of it (its first n reads) then
                costs O(n): the unique words in walk order (ascending packed value), their counts, each word's first
                read and each read's leaf.
pairs_d1        every pair of unique words at nucleotide Hamming distance 1, complete: two such words agree exactly
                on one of their two halves, so only the words of a run of equal half value are compared.
check_pairs_d2  a device's lists at d = 2: sound everywhere (distance 1 or 2, symmetric, rows strictly ascending) and
                complete on a seeded sample of leaves (every word within distance 2 of the leaf looked up).
unique_level    the clusters from the oracle's own clustering code (orc_graph_*, src/cluster.cc) over the counts and
                the lists, with the six summary counts and the histograms; per_read() then follows orc_map_reads.
"""
import numpy as np

from oracle import pyoracle as orc

M55 = np.uint64(0x5555555555555555)
LO32 = np.uint64(0xFFFFFFFF)


def nt_distance(a, b):
    """nucleotide Hamming distance between packed words, row by row (u64[k], or [hi, lo] rows u64[k, 2])"""
    x = np.bitwise_xor(a, b)
    d = np.bitwise_count((x | (x >> np.uint64(1))) & M55).astype(np.int64)
    return d.sum(axis=-1) if d.ndim == 2 else d


def _differ(w):
    """w[i] != w[i - 1] for i >= 1 (rows of two-word words)"""
    ne = w[1:] != w[:-1]
    return ne.any(axis=1) if ne.ndim == 2 else ne


def stable_order(words, idx):
    """the read indices idx sorted by their words, stable (two-word words by [hi, lo])"""
    if words.ndim == 1:
        return idx[np.argsort(words[idx], kind="stable")]
    p = np.argsort(words[idx, 1], kind="stable")
    hi = words[idx[p], 0]
    if len(hi) and int(hi.max()) < 1 << 16:
        hi = hi.astype(np.uint16)                       # (sorted by radix)
    return idx[p[np.argsort(hi, kind="stable")]]


class PrefixTruth:
    """The count stage's exact results for every prefix of one read set (words u64[N] or u64[N, 2], filtered u8[N])."""

    def __init__(self, words, filtered):
        assert len(words) < 1 << 32
        self.words = words
        self.order = stable_order(words, np.flatnonzero(np.asarray(filtered) == 0).astype(np.uint32))

    def prefix(self, n):
        """the first n reads: dict(n, usable, unique, word, count u32[U], first_read u32[U], leaf i32[n] (-1: filtered))"""
        sel = self.order[self.order < n]              # still sorted by word, and (a stable sort) by read within a word
        w = self.words[sel]
        new = np.ones(len(sel), bool)
        new[1:] = _differ(w)
        starts = np.flatnonzero(new)
        leaf = np.full(n, -1, np.int32)
        leaf[sel] = np.cumsum(new, dtype=np.int32) - 1
        return dict(n=n, usable=len(sel), unique=len(starts), word=w[starts],
                    count=np.diff(np.append(starts, len(sel))).astype(np.uint32), first_read=sel[starts], leaf=leaf)


def per_read(t, leaf_cid, is_max_leaf):
    """orc_map_reads (src/humid.cc:220-234, 268-285) over prefix t: a filtered read gets cluster 0 and keep 0, a usable
    one its leaf's cluster id.  keep is 1 for the first read of a leaf that is its own cluster's max leaf -- said per
    leaf: after a steal a cluster's max leaf can sit in another cluster, and then that cluster keeps no read."""
    cid = np.concatenate([np.zeros(1, np.uint32), np.asarray(leaf_cid, np.uint32)])[t["leaf"] + 1]
    keep = np.zeros(t["n"], np.uint8)
    keep[t["first_read"][np.asarray(is_max_leaf).astype(bool)]] = 1
    return cid, keep


def _halves(word, word_nt):
    """(top, bottom) half of every word; the bottom one holds the last word_nt // 2 nucleotides"""
    nb = 2 * (word_nt // 2)
    if word.ndim == 1:
        return word >> np.uint64(nb), word & np.uint64((1 << nb) - 1)
    assert nb < 64
    hi, lo = word[:, 0], word[:, 1]
    return (hi << np.uint64(64 - nb)) | (lo >> np.uint64(nb)), lo & np.uint64((1 << nb) - 1)


def pairs_d1(word, word_nt):
    """every pair (a < b) of the unique words `word` (walk order) at nucleotide Hamming distance 1, in ascending
    (a, b) order.  Such a pair agrees on exactly one half: per half, the words of a run of equal half value are
    compared pair by pair, and every pair is found exactly once."""
    A, B = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for key in _halves(word, word_nt):
        o = np.argsort(key)
        k = key[o]
        i = np.flatnonzero(k[1:] == k[:-1])           # sorted: k[i] == k[i + s] for every i of this list
        s = 1
        while len(i):
            a, b = o[i], o[i + s]
            hit = nt_distance(word[a], word[b]) == 1
            A.append(np.minimum(a, b)[hit])
            B.append(np.maximum(a, b)[hit])
            s += 1
            i = i[i + s < len(k)]
            i = i[k[i + s] == k[i]]
    key = np.sort((np.concatenate(A).astype(np.uint64) << np.uint64(32)) | np.concatenate(B).astype(np.uint64))
    assert np.all(key[1:] > key[:-1]), "a pair was found twice"
    return (key >> np.uint64(32)).astype(np.uint32), (key & LO32).astype(np.uint32)


def sub_pairs(a, b, first_read, n):
    """the pairs of a prefix's words from those of a longer prefix (first_read: the longer prefix's first reads): a
    word is among the first n reads iff its first read is; the leaves keep their order and are numbered again"""
    present = first_read < n
    rank = np.cumsum(present, dtype=np.int64) - 1
    both = present[a] & present[b]
    return rank[a[both]].astype(np.uint32), rank[b[both]].astype(np.uint32)


def csr(a, b, u):
    """the neighbour lists of the pairs (a, b) in CSR form, every row ascending (the order of the oracle's lists, H1 +
    H2 of DESIGN.md section 5)"""
    a = np.asarray(a, np.uint64)
    b = np.asarray(b, np.uint64)
    key = np.sort(np.concatenate([(a << np.uint64(32)) | b, (b << np.uint64(32)) | a]))
    off = np.zeros(u + 1, np.uint64)
    np.cumsum(np.bincount((key >> np.uint64(32)).astype(np.int64), minlength=u), out=off[1:])
    return off, (key & LO32).astype(np.uint32)


def _hist(a):
    k, v = np.unique(np.asarray(a, dtype=np.uint64), return_counts=True)
    return [(int(x), int(y)) for x, y in zip(k, v)]


def unique_level(t, off, idx, maximum=False):
    """prefix t clustered over the lists (off, idx) by the oracle's clustering code: orc_graph_find_clusters numbers
    the clusters in leaf order = walk order, and a leaf's is_max_leaf is max_leaf[cluster_id - 1] == leaf, as
    orc_export_leaves defines it.  Returns the leaves' degree / cluster_id / is_max_leaf, the clusters, the six
    summary counts and the histograms in Dedup.histograms()'s form."""
    u = t["unique"]
    g = orc.Graph(t["count"])
    g.append_csr(off, idx)
    nc = g.find_clusters(maximum)
    lc, size, mc, ml = g.export(nc)
    del g
    is_max = (ml[lc.astype(np.int64) - 1] == np.arange(u)).astype(np.uint8)
    degree = np.diff(np.asarray(off, np.int64)).astype(np.uint32)
    summary = dict(total=t["n"], usable=t["usable"], unique=u, clusters=nc, edges=len(idx) // 2,
                   nonsingle=int(np.count_nonzero(degree)))
    hist = dict(counts=_hist(t["count"]), neigh=_hist(degree), clusters=_hist(size),
                stats=dict(total=t["n"], usable=t["usable"], unique=u, clusters=nc))
    return dict(summary=summary, off=off, idx=idx, degree=degree, cluster_id=lc, is_max_leaf=is_max,
                clusters=dict(size=size, max_count=mc, max_leaf=ml), hist=hist)


def variant_masks(word_nt):
    """XOR masks that change one or two nucleotides of a word: 3 n + 9 n (n - 1) / 2 of them (2 556 at 24 nt); u64[M]
    for one-word words, [hi, lo] rows for two-word words (nucleotide i sits at bit 2 (n - 1 - i) of hi << 64 | lo)"""
    ms = [d << (2 * p) for p in range(word_nt) for d in (1, 2, 3)]
    ms += [(d << (2 * p)) | (e << (2 * q)) for p in range(word_nt) for q in range(p + 1, word_nt)
           for d in (1, 2, 3) for e in (1, 2, 3)]
    if word_nt <= 32:
        return np.asarray(ms, np.uint64)
    return np.asarray([(m >> 64, m & ((1 << 64) - 1)) for m in ms], np.uint64)


def _keys(w):
    """words as keys that np.searchsorted orders like the walk ([hi, lo] rows as records)"""
    if w.ndim == 1:
        return w
    k = np.empty(len(w), dtype=[("hi", "<u8"), ("lo", "<u8")])
    k["hi"], k["lo"] = w[:, 0], w[:, 1]
    return k


def sampled_rows_d2(word, word_nt, sample, masks=None):
    """the complete d <= 2 rows of the leaves `sample` by enumeration: every word within distance 2 of the leaf,
    looked up among the unique words `word`.  Returns (row << 32 | neighbour) u64, ascending; row = the position in
    `sample`."""
    masks = variant_masks(word_nt) if masks is None else masks
    wk = _keys(word)
    v = word[sample][:, None] ^ masks[None]
    vk = _keys(v.reshape((-1, 2) if word.ndim == 2 else -1))
    pos = np.minimum(np.searchsorted(wk, vk), len(word) - 1)
    hit = wk[pos] == vk
    r = np.repeat(np.arange(len(sample), dtype=np.uint64), len(masks))[hit]
    return np.sort((r << np.uint64(32)) | pos[hit].astype(np.uint64))


def rows_of(off, idx, sample):
    """the CSR rows of the leaves `sample` as (row << 32 | neighbour) u64; row = the position in `sample`"""
    off = np.asarray(off, np.int64)
    beg = off[sample]
    lens = off[np.asarray(sample) + 1] - beg
    start = np.cumsum(lens) - lens
    pos = np.repeat(beg - start, lens) + np.arange(int(lens.sum()))
    return (np.repeat(np.arange(len(sample), dtype=np.uint64), lens) << np.uint64(32)) | \
        np.asarray(idx, np.uint64)[pos]


def check_pairs_d2(word, word_nt, off, idx, n_sample=20_000, seed=0, chunk=1024, also=None):
    """a device's lists at d = 2 (CSR over the unique words `word`): every pair is at distance 1 or 2 (so its two ends
    differ), the lists are symmetric and every row is strictly ascending; the rows of a seeded sample of n_sample
    leaves, and of the leaves `also`, equal the complete enumeration (sampled_rows_d2).  Raises AssertionError;
    returns the leaves checked."""
    u = len(word)
    off = np.asarray(off, np.int64)
    idx = np.asarray(idx, np.uint32)
    assert off[0] == 0 and off[-1] == len(idx) and np.all(np.diff(off) >= 0), "not a CSR"
    row = np.repeat(np.arange(u, dtype=np.uint64), np.diff(off))
    key = (row << np.uint64(32)) | idx.astype(np.uint64)
    assert np.all(key[1:] > key[:-1]), "a row is not strictly ascending"
    assert np.array_equal(np.sort((idx.astype(np.uint64) << np.uint64(32)) | row), key), "the lists are not symmetric"
    del key
    d = nt_distance(word[row.astype(np.int64)], word[idx])
    assert np.all((d >= 1) & (d <= 2)), "a pair is not at distance 1 or 2"
    del d, row
    sample = np.random.default_rng(seed).choice(u, size=min(n_sample, u), replace=False)
    sample = np.unique(np.concatenate([sample, np.asarray([] if also is None else also, np.int64)]))
    masks = variant_masks(word_nt)
    for c0 in range(0, len(sample), chunk):
        s = sample[c0:c0 + chunk]
        assert np.array_equal(rows_of(off, idx, s), sampled_rows_d2(word, word_nt, s, masks)), \
            "a row of the leaves %d..%d is not complete" % (s[0], s[-1])
    return sample
