"""CPU truth for keyed accumulated runs (include/humid_hip.h, humid_accum_*_keyed): a read set with 64-bit keys fed in
chunks, each chunk with the global index of its first read.

TEST HELPER, never product code.

  keyed_leaves    the accumulator's list from numpy alone: np.unique over the (key, word) rows of the usable reads,
                  the reads per row by bincount, the smallest global index per row by np.minimum.at
  keyed_expected  (cluster_id, keep) per chunk, the summary and the whole truth dict of a keyed accumulated run: the
                  reads sorted by global index, group = the rank of the key among the distinct usable keys,
                  grouped_truth.per_group (one oracle pass per group) for cluster ids, leaves and summary; keep is
                  RE-DERIVED from is_max_leaf and the global first index, exactly as accum_truth.accum_expected does.

A chunk is (words u64[N], keys u64[N], filtered u8[N], base int).  Keys of filtered reads are never looked at."""
import numpy as np

from grouped_truth import per_group

U64 = np.uint64


def _concat(chunks):
    cat = lambda j, dt: np.concatenate([np.asarray(c[j], dtype=dt) for c in chunks]) if chunks else np.zeros(0, dt)   # noqa: E731
    w, k, f = cat(0, U64), cat(1, U64), cat(2, np.uint8)
    g = np.concatenate([U64(c[3]) + np.arange(len(c[2]), dtype=U64) for c in chunks]) if chunks else np.zeros(0, U64)
    assert len(np.unique(g)) == len(g), "the index ranges of the chunks must be disjoint"
    return w, k, f, g


def _unique_rows(k, w):
    """ascending distinct (key, word) rows and the inverse"""
    if len(k) == 0:
        return np.zeros((0, 2), U64), np.zeros(0, np.int64)
    u, inv = np.unique(np.stack([k, w], 1), axis=0, return_inverse=True)
    return u, inv.reshape(-1)


def keyed_leaves(chunks):
    """dict(key u64[U], word u64[U], count u64[U], first u64[U]) of the accumulated list"""
    w, k, f, g = _concat(chunks)
    use = f == 0
    u, inv = _unique_rows(k[use], w[use])
    count = np.bincount(inv, minlength=len(u)).astype(U64)
    first = np.full(len(u), np.iinfo(U64).max, dtype=U64)
    np.minimum.at(first, inv, g[use])
    return dict(key=u[:, 0], word=u[:, 1], count=count, first=first)


def keyed_expected(chunks, word_nt, distance=1, method=0, edit=False):
    """([(cluster_id, keep)] per chunk in the order given, summary dict, truth dict of grouped_truth.per_group with
    "keys" = the distinct usable keys ascending)"""
    w, k, f, g = _concat(chunks)
    order = np.argsort(g, kind="stable")
    ws, ks, fs, gs = w[order], k[order], f[order], g[order]
    use = fs == 0
    keys = np.unique(ks[use])
    group = np.zeros(len(fs), np.uint32)
    group[use] = np.searchsorted(keys, ks[use]).astype(np.uint32)
    t = per_group(ws, group, fs, word_nt, distance, method, edit, first_read=False)
    lv = t["leaves"]
    u, inv = _unique_rows(ks[use], ws[use])
    # the leaves of per_group are in (group, word) order: the order of the rows
    assert np.array_equal(u[:, 0], keys[lv["group"]]) and np.array_equal(u[:, 1], np.asarray(lv["word"], U64))
    first = np.full(len(u), np.iinfo(U64).max, dtype=U64)
    np.minimum.at(first, inv, gs[use])
    keep_s = np.zeros(len(fs), np.uint8)
    keep_s[use] = (lv["is_max_leaf"][inv] != 0) & (gs[use] == first[inv])
    assert np.array_equal(t["cid"][use], lv["cluster_id"][inv]) and not t["cid"][~use].any()
    cid = np.zeros(len(f), np.uint32)
    keep = np.zeros(len(f), np.uint8)
    cid[order], keep[order] = t["cid"], keep_s
    out, at = [], 0
    for c in chunks:
        n = len(c[2])
        out.append((cid[at:at + n], keep[at:at + n]))
        at += n
    t["keys"] = keys
    return out, t["summary"], t
