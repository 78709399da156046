"""Pure-numpy truth for words of any length (Dedup.run_long): words are u64[N, k] rows, k = ceil(word_nt / 32), the
first column right-aligned.  Leaves come from np.unique(axis=0) (rows sort lexicographically = numeric order, most
significant first), neighbours from an all-pairs Hamming matrix summed over the k columns (bruteforce.nt_hamming),
clusters from the literal recursion of bruteforce.cluster.  Shares no code with the C oracle, which stops at 64
nucleotides; tests/test_long_truth_host.py pins the two to each other where both apply.  Small inputs only: the
matrix is U x U."""
import numpy as np

import bruteforce as bf

U64 = np.uint64


def head_mask(word_nt):
    """(k, mask of the significant bits of column 0)"""
    k = (word_nt + 31) // 32
    hbits = 2 * (word_nt - 32 * (k - 1))
    return k, U64((1 << hbits) - 1)


def hist(a):
    k, v = np.unique(np.asarray(a, dtype=U64), return_counts=True)
    return [(int(x), int(y)) for x, y in zip(k, v)]


def long_dedup(words, filtered, d, maximum, word_nt=None):
    """words u64[N, k]; word_nt (optional) masks the ignored upper bits of column 0 first.  Returns a dict: cid, keep,
    summary, leaves (word u64[U, k], count, degree, cluster_id, is_max_leaf), off / idx (CSR adjacency, rows
    ascending), clusters (size, max_count, max_leaf) and hist (the four .dat histograms, as oracle.pyoracle.histograms)."""
    w = np.array(words, dtype=U64)
    f = np.asarray(filtered, dtype=np.uint8)
    if w.ndim == 1:
        w = w.reshape(-1, 1)
    n, k = w.shape
    if word_nt is not None:
        kk, m = head_mask(word_nt)
        assert kk == k
        w[:, 0] &= m
    use = np.nonzero(f == 0)[0]
    if len(use):
        uw, inv, cnt = np.unique(w[use], axis=0, return_inverse=True, return_counts=True)
        inv = np.asarray(inv).reshape(-1)
    else:
        uw, inv, cnt = np.zeros((0, k), U64), np.zeros(0, np.int64), np.zeros(0, np.int64)
    u = len(uw)
    dist = np.zeros((u, u), dtype=np.int64)
    for j in range(k):
        col = uw[:, j]
        if u and (col == col[0]).all():
            continue                                   # a constant column adds no distance
        dist += bf.nt_hamming(col[:, None], col[None, :])
    adj = dist <= d
    if u:
        np.fill_diagonal(adj, False)
    nbrs = [np.nonzero(adj[i])[0].tolist() for i in range(u)]
    cl, info = bf.cluster(cnt, nbrs, bool(maximum))
    deg = np.array([len(x) for x in nbrs], dtype=np.uint32)
    off = np.zeros(u + 1, dtype=U64)
    off[1:] = np.cumsum(deg)
    idx = np.array([x for row in nbrs for x in row], dtype=np.uint32)
    c = len(info)
    size = np.array([info[i]["size"] for i in range(1, c + 1)], dtype=U64)
    max_count = np.array([info[i]["maxCount"] for i in range(1, c + 1)], dtype=U64)
    max_leaf = np.array([info[i]["maxLeaf"] for i in range(1, c + 1)], dtype=np.uint32)
    leaf_cid = np.array(cl, dtype=np.uint32)
    is_max = np.zeros(u, dtype=np.uint8)
    is_max[max_leaf] = 1
    cid = np.zeros(n, dtype=np.uint32)
    keep = np.zeros(n, dtype=np.uint8)
    cid[use] = leaf_cid[inv] if u else 0
    first = np.full(u, n, dtype=np.int64)
    np.minimum.at(first, inv, use)
    keep[first[max_leaf]] = 1
    summary = dict(total=n, usable=len(use), unique=u, clusters=c, edges=int(deg.sum()) // 2)
    return dict(cid=cid, keep=keep, summary=summary,
                leaves=dict(word=uw, count=cnt.astype(U64), degree=deg, cluster_id=leaf_cid, is_max_leaf=is_max,
                            first_read=first.astype(np.uint32)),
                off=off, idx=idx, clusters=dict(size=size, max_count=max_count, max_leaf=max_leaf),
                hist=dict(counts=hist(cnt), neigh=hist(deg), clusters=hist(size),
                          stats=dict(total=n, usable=len(use), unique=u, clusters=c)))


def with_filler(words2, n, fill_nt, seed):
    """Two-word words of n nucleotides (u64[N, 2]) with fill_nt constant nucleotides put between their first n - 32 and
    their last 32: words of n + fill_nt nucleotides, u64[N, ceil((n + fill_nt) / 32)].  Distances, and so every result,
    stay what they were; the order of the words too (the filler is the same everywhere)."""
    w2 = np.asarray(words2, dtype=U64)
    assert w2.ndim == 2 and w2.shape[1] == 2 and 33 <= n <= 64
    rng = np.random.default_rng(seed)
    nh = n - 32
    fill = rng.integers(0, 4, size=fill_nt).astype(U64)
    total = n + fill_nt
    k, _ = head_mask(total)
    r = total - 32 * (k - 1)                            # nucleotides of column 0
    out = np.zeros((len(w2), k), dtype=U64)
    # nucleotide p of the new word: p < nh from hi, p < nh + fill_nt the filler, else from lo
    for p in range(total):
        if p < nh:
            sym = (w2[:, 0] >> U64(2 * (nh - 1 - p))) & U64(3)
        elif p < nh + fill_nt:
            sym = np.full(len(w2), fill[p - nh], dtype=U64)
        else:
            sym = (w2[:, 1] >> U64(2 * (31 - (p - nh - fill_nt)))) & U64(3)
        col = 0 if p < r else 1 + (p - r) // 32
        sh = 2 * (r - 1 - p) if p < r else 2 * (31 - (p - r) % 32)
        out[:, col] |= sym << U64(sh)
    return out


def pack_syms(syms):
    """nucleotide codes u8[N, n] -> words u64[N, ceil(n / 32)] in the long layout"""
    syms = np.asarray(syms)
    n = syms.shape[1]
    k, _ = head_mask(n)
    r = n - 32 * (k - 1)
    out = np.zeros((len(syms), k), dtype=U64)
    for p in range(n):
        col = 0 if p < r else 1 + (p - r) // 32
        sh = 2 * (r - 1 - p) if p < r else 2 * (31 - (p - r) % 32)
        out[:, col] |= syms[:, p].astype(U64) << U64(sh)
    return out


def unpack_syms(words, n):
    """words u64[N, ceil(n / 32)] -> nucleotide codes u8[N, n]"""
    w = np.asarray(words, dtype=U64)
    k, _ = head_mask(n)
    r = n - 32 * (k - 1)
    out = np.zeros((len(w), n), dtype=np.uint8)
    for p in range(n):
        col = 0 if p < r else 1 + (p - r) // 32
        sh = 2 * (r - 1 - p) if p < r else 2 * (31 - (p - r) % 32)
        out[:, p] = ((w[:, col] >> U64(sh)) & U64(3)).astype(np.uint8)
    return out


def substitute(word, word_nt, pos, delta=1):
    """a copy of one word (u64[k]) with nucleotide pos (0 = first) replaced by (old + delta) % 4"""
    w = np.array(word, dtype=U64)
    k, _ = head_mask(word_nt)
    r = word_nt - 32 * (k - 1)
    col = 0 if pos < r else 1 + (pos - r) // 32
    sh = 2 * (r - 1 - pos) if pos < r else 2 * (31 - (pos - r) % 32)
    old = (int(w[col]) >> sh) & 3
    w[col] = U64((int(w[col]) & ~(3 << sh)) | (((old + delta) & 3) << sh))
    return w
