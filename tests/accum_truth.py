"""CPU truth for accumulated runs (include/humid_hip.h, humid_accum_*): a read set fed in chunks, each chunk with the
global index of its first read.

  accum_leaves    the accumulator's list from numpy alone: np.unique over the concatenation of the usable words
                  (axis=0 for two-word words), the reads per word, the smallest global index per word
  accum_expected  (cluster_id, keep) per chunk and the summary of an accumulated run: the oracle
                  (oracle.pyoracle.Pipeline) over all reads sorted by global index; keep is RE-DERIVED from the oracle's
                  leaves and the global first indices -- a read is kept iff it is usable, its word is its cluster's
                  maxLeaf and its global index is that word's first index -- and the oracle's own keep (the first such
                  read in sorted order) is returned beside it for the host test to compare.

A chunk is (words, filtered, base): words u64[N] (word_nt <= 32) or u64[N, 2], filtered u8[N], base an int."""
import numpy as np

from oracle import pyoracle as orc


def _concat(chunks, word_nt):
    wpr = 2 if word_nt > 32 else 1
    ws = [np.asarray(w, dtype=np.uint64).reshape(-1, wpr) for w, _, _ in chunks]
    w = np.concatenate(ws) if ws else np.zeros((0, wpr), np.uint64)
    f = np.concatenate([np.asarray(f, dtype=np.uint8) for _, f, _ in chunks]) if chunks else np.zeros(0, np.uint8)
    g = np.concatenate([np.uint64(b) + np.arange(len(f), dtype=np.uint64) for _, f, b in chunks]) if chunks else np.zeros(0, np.uint64)
    assert len(np.unique(g)) == len(g), "the index ranges of the chunks must be disjoint"
    return w, f, g


def _unique(w):
    """ascending distinct rows of w (u64[M, wpr]) and the inverse"""
    if len(w) == 0:
        return w.reshape(0, w.shape[1]), np.zeros(0, np.int64)
    if w.shape[1] == 1:
        u, inv = np.unique(w[:, 0], return_inverse=True)
        return u.reshape(-1, 1), inv.reshape(-1)
    u, inv = np.unique(w, axis=0, return_inverse=True)
    return u, inv.reshape(-1)


def accum_leaves(chunks, word_nt):
    """dict(word u64[U] or u64[U, 2], count u64[U], first u64[U]) of the accumulated list"""
    w, f, g = _concat(chunks, word_nt)
    use = f == 0
    u, inv = _unique(w[use])
    count = np.bincount(inv, minlength=len(u)).astype(np.uint64)
    first = np.full(len(u), np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(first, inv, g[use])
    return dict(word=u if word_nt > 32 else u[:, 0], count=count, first=first)


def accum_expected(chunks, word_nt, distance=1, method=0, edit=False):
    """([(cluster_id, keep)] per chunk in the order given, summary dict, [oracle keep] per chunk)"""
    w, f, g = _concat(chunks, word_nt)
    order = np.argsort(g, kind="stable")
    ws, fs, gs = w[order], f[order], g[order]
    p = orc.Pipeline(word_nt)
    p.read_data(ws if word_nt > 32 else ws[:, 0], fs)
    if edit and distance >= 2:
        p.find_edit_neighbours(distance)
    else:
        p.find_hamming_neighbours(distance)
    p.find_clusters(bool(method & 1))
    cid_s, keep_orc_s = p.map_reads()
    lv = p.leaves()
    # keep from the leaves: the oracle walks them ascending, as np.unique orders them
    use = fs == 0
    u, inv = _unique(ws[use])
    assert np.array_equal(u, np.asarray(lv["word"], dtype=np.uint64).reshape(-1, u.shape[1]))
    first = np.full(len(u), np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(first, inv, gs[use])
    keep_s = np.zeros(len(fs), np.uint8)
    keep_s[use] = (lv["is_max_leaf"][inv] != 0) & (gs[use] == first[inv])
    assert np.array_equal(cid_s[use], lv["cluster_id"][inv]) and not cid_s[~use].any()
    cid = np.zeros(len(f), np.uint32)
    keep = np.zeros(len(f), np.uint8)
    keep_orc = np.zeros(len(f), np.uint8)
    cid[order], keep[order], keep_orc[order] = cid_s, keep_s, keep_orc_s
    out, out_orc, at = [], [], 0
    for _, fc, _ in chunks:
        out.append((cid[at:at + len(fc)], keep[at:at + len(fc)]))
        out_orc.append(keep_orc[at:at + len(fc)])
        at += len(fc)
    return out, p.summary(), out_orc
