"""What a strand-symmetric (duplex) run has to return (include/humid_hip.h, humid_dedup_run_paired): TEST HELPER, never
product code.

Plain numpy and Python integers, written from the definitions alone.  A word of n = 2 h nucleotides is A.B; its mirror
is m(A.B) = B.A; the canonical word is min(w, m(w)); a usable read is a top-strand read when its word is its canonical
word and a bottom-strand read otherwise.  The leaves are the distinct canonical words in ascending order, two different
leaves u, v are neighbours when min(ham(u, v), ham(u, m(v))) <= d -- found by comparing every pair -- and the clusters
are those of the oracle's clustering code (oracle.pyoracle.Graph) over these leaves and lists.
"""
import numpy as np

from oracle import pyoracle as orc

TOP, BOTTOM, NONE = 0, 1, 2
_M64 = (1 << 64) - 1
_LUT = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def to_ints(words, n):
    """packed words (u64[N], or u64[N, 2] = [hi, lo] beyond 32 nt) -> Python integers of 2 n bits"""
    w = np.asarray(words, np.uint64)
    if n > 32:
        return [(int(h) << 64) | int(l) for h, l in w.reshape(-1, 2)]
    return [int(x) for x in w.reshape(-1)]


def from_ints(vals, n):
    """the inverse of to_ints"""
    if n > 32:
        return np.array([(v >> 64, v & _M64) for v in vals], np.uint64).reshape(-1, 2)
    return np.array(vals, np.uint64).reshape(-1)


def mirror(v, n):
    """m(A.B) = B.A on the packed 2 n-bit value"""
    return ((v & ((1 << n) - 1)) << n) | (v >> n)


def mirror_words(words, n):
    return from_ints([mirror(v, n) for v in to_ints(words, n)], n)


def canonical(words, filtered, n):
    """(canonical words in the layout of words, strand u8[N]); a filtered read keeps its word and has strand NONE"""
    vals = to_ints(words, n)
    f = np.asarray(filtered, np.uint8)
    out, strand = [], np.full(len(f), NONE, np.uint8)
    for i, v in enumerate(vals):
        if f[i]:
            out.append(v)
            continue
        m = mirror(v, n)
        out.append(min(v, m))
        strand[i] = TOP if v <= m else BOTTOM
    return from_ints(out, n), strand


def ham(a, b):
    """nucleotide mismatches of two packed values"""
    x = a ^ b
    return bin((x | (x >> 1)) & int("01" * 64, 2)).count("1")


def _halves(vals):
    return (np.array([v >> 64 for v in vals], np.uint64), np.array([v & _M64 for v in vals], np.uint64))


def _mismatch(x):
    """nucleotide mismatches per element of a u64 array of XORs"""
    y = (x | (x >> np.uint64(1))) & np.uint64(0x5555555555555555)
    return _LUT[y.view(np.uint8).reshape(-1, 8)].sum(1, dtype=np.uint32)


def neighbours(leaves, n, d):
    """(off u64[U + 1], idx u32[2 E]) over the ascending leaves (Python integers): every pair compared, both terms"""
    u = len(leaves)
    hi, lo = _halves(leaves)
    mhi, mlo = _halves([mirror(v, n) for v in leaves])
    rows = []
    for i in range(u):
        plain = _mismatch(hi ^ hi[i]) + _mismatch(lo ^ lo[i])
        mirr = _mismatch(mhi ^ hi[i]) + _mismatch(mlo ^ lo[i])          # ham(u_i, m(v)) for every v
        ok = np.minimum(plain, mirr) <= d
        ok[i] = False                                                   # never its own neighbour
        rows.append(np.flatnonzero(ok).astype(np.uint32))               # ascending, each once
    off = np.zeros(u + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate(rows) if rows else np.zeros(0, np.uint32)
    return off, idx.astype(np.uint32)


def _hist(a):
    k, v = np.unique(np.asarray(a, dtype=np.uint64), return_counts=True)
    return [(int(x), int(y)) for x, y in zip(k, v)]


def run(words, filtered, n, d, method=0):
    """everything a paired run returns, as a dict: cluster_id u32[N], keep u8[N], summary (total, usable, unique,
    clusters, edges, nonsingle), leaves (word, count, first_read, degree, cluster_id, is_max_leaf), off / idx,
    clusters (size, max_count, max_leaf), hist (counts, neigh, clusters, stats), strand u8[N], top / bottom u32[C],
    strands (the strand summary)"""
    assert n % 2 == 0 and 2 <= n <= 64
    f = np.asarray(filtered, np.uint8)
    N = len(f)
    cw, strand = canonical(words, f, n)
    cvals = to_ints(cw, n)
    usable = [i for i in range(N) if not f[i]]
    leaves = sorted(set(cvals[i] for i in usable))
    pos = {v: k for k, v in enumerate(leaves)}
    U = len(leaves)
    count = np.zeros(U, np.uint32)
    first = np.full(U, N, np.uint32)
    for i in usable:
        k = pos[cvals[i]]
        count[k] += 1
        first[k] = min(first[k], i)
    off, idx = neighbours(leaves, n, d)
    g = orc.Graph(count)
    g.append_csr(off, idx)
    nc = g.find_clusters(bool(method))
    lc, size, mc, ml = g.export(nc)
    del g
    degree = np.diff(off.astype(np.int64)).astype(np.uint32)
    is_max = (ml[lc.astype(np.int64) - 1] == np.arange(U)).astype(np.uint8) if U else np.zeros(0, np.uint8)
    cid = np.zeros(N, np.uint32)
    keep = np.zeros(N, np.uint8)
    top, bottom = np.zeros(nc, np.uint32), np.zeros(nc, np.uint32)
    for i in usable:
        k = pos[cvals[i]]
        cid[i] = lc[k]
        (top if strand[i] == TOP else bottom)[lc[k] - 1] += 1
    for c in range(nc):
        keep[first[ml[c]]] = 1                                          # the first read whose canonical word is the maxLeaf
    summary = dict(total=N, usable=len(usable), unique=U, clusters=nc, edges=len(idx) // 2,
                   nonsingle=int(np.count_nonzero(degree)))
    strands = dict(n_clusters=nc, duplex=int(np.count_nonzero((top > 0) & (bottom > 0))),
                   top_only=int(np.count_nonzero((top > 0) & (bottom == 0))),
                   bottom_only=int(np.count_nonzero((top == 0) & (bottom > 0))),
                   top_reads=int(top.sum()), bottom_reads=int(bottom.sum()))
    return dict(cluster_id=cid, keep=keep, summary=summary,
                leaves=dict(word=from_ints(leaves, n), count=count, first_read=first, degree=degree, cluster_id=lc,
                            is_max_leaf=is_max),
                off=off, idx=idx, clusters=dict(size=size, max_count=mc, max_leaf=ml),
                hist=dict(counts=_hist(count), neigh=_hist(degree), clusters=_hist(size),
                          stats=dict(total=N, usable=len(usable), unique=U, clusters=nc)),
                strand=strand, top=top, bottom=bottom, strands=strands, canonical=cw)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def pack(seq):
    """nucleotide codes (first one most significant) -> Python integer"""
    v = 0
    for s in seq:
        v = (v << 2) | int(s)
    return v


def flip_pair(n):
    """(a, b): a = A.B is a top-strand read of a molecule; b = B'.A is a read of its other strand with ONE error at the
    first nucleotide of B, in front of the first position where A and B differ.  The error makes B' < A, so b is its
    own canonical word: ham(c(a), c(b)) = n, but ham(a, m(b)) = 1.  A = 1 0 0 .., B = 2 3 3 .., B' = 0 3 3 .."""
    h = n // 2
    A, B, B1 = [1] + [0] * (h - 1), [2] + [3] * (h - 1), [0] + [3] * (h - 1)
    return pack(A + B), pack(B1 + A)


def forced_reads(rng, n, d):
    """Python-integer words of the cases every input carries: the orientation flip; palindromes A.A; a leaf A.A' with
    ham(u, m(u)) = 2 (ham(u, m(u)) is even: at d <= 1 only the palindromes have it <= d; never a self edge); a pair u = A.A, v = A.A'' that qualifies under both terms (one edge)"""
    h = n // 2
    out = list(flip_pair(n)) * 2
    A = rng.integers(0, 4, size=h).tolist()
    out += [pack(A + A)] * 3                                            # palindrome
    A1 = list(A)
    A1[h - 1] = (A1[h - 1] + 1) % 4
    out += [pack(A + A1), pack(A1 + A)]                                 # ham(u, m(u)) = 2 (1 per half); both strands
    C = rng.integers(0, 4, size=h).tolist()
    C1 = list(C)
    C1[0] = (C1[0] + 2) % 4
    out += [pack(C + C), pack(C + C1), pack(C + C1)]                    # ham(u, v) = ham(u, m(v)) = 1
    return out


def families(seed, n, n_reads, d=1, p_filtered=0.03):
    """(words, filtered): molecules read from both strands with random substitutions, plus forced_reads, shuffled"""
    rng = np.random.default_rng(seed)
    h = n // 2
    vals = []
    if n_reads >= 16:
        vals += forced_reads(rng, n, d)
    n_mol = max(1, n_reads // 6)
    mol = rng.integers(0, 4, size=(n_mol, n))
    while len(vals) < n_reads:
        s = mol[int(rng.integers(0, n_mol))].copy()
        for _ in range(int(rng.integers(0, 3)) if rng.random() < 0.5 else 0):
            s[int(rng.integers(0, n))] = int(rng.integers(0, 4))
        s = s.tolist()
        if rng.random() < 0.5:
            s = s[h:] + s[:h]                                           # the other strand
        vals.append(pack(s))
    vals = [vals[i] for i in rng.permutation(len(vals))][:n_reads]
    filt = (rng.random(n_reads) < p_filtered).astype(np.uint8)
    return from_ints(vals, n), filt


def long_run_words(seed, n=24, k=300):
    """k leaves X.R (R > X) and k leaves R'.X (R' < X): every X.R meets the mirrors X.R' of all the others under the key
    "first half", a run of k equal keys; a third of the R' are an R with its first nucleotide changed, so mirror pairs
    at distance 1 exist.  All words are their own canonical words."""
    rng = np.random.default_rng(seed)
    h = n // 2
    X = [1] + [2] * (h - 1)
    vals = []
    for j in range(k):
        R = [int(rng.integers(2, 4))] + rng.integers(0, 4, size=h - 1).tolist()
        vals.append(pack(X + R))
        R1 = [int(rng.integers(0, 2))] + (R[1:] if j % 3 == 0 else rng.integers(0, 4, size=h - 1).tolist())
        if R1 < X:
            vals.append(pack(R1 + X))
    vals = [vals[i] for i in rng.permutation(len(vals))]
    return from_ints(vals, n), np.zeros(len(vals), np.uint8)


def shared_prefix_words(seed, n, share, k=300):
    """k different words P.T: one prefix P of `share` nucleotides (more than half a word) in front of tails T, a third
    of them random and each of the others one of those with one nucleotide changed, so pairs at distance 1 exist.  P
    starts with 0 and holds 2 at position n / 2: every word is below its mirror, its own canonical word.  Every third
    one is given as its mirror, a read of the other strand."""
    rng = np.random.default_rng(seed)
    h = n // 2
    assert h < share < n
    P = [0] + rng.integers(0, 4, size=share - 1).tolist()
    P[h] = 2
    tails = {}
    while len(tails) < k:
        if len(tails) % 3 == 0:
            T = rng.integers(0, 4, size=n - share).tolist()
        else:
            T = list(list(tails)[int(rng.integers(0, len(tails)))])
            T[int(rng.integers(0, len(T)))] = int(rng.integers(0, 4))
        tails[tuple(T)] = True
    vals = [pack(P + list(T)) for T in tails]
    vals = [mirror(v, n) if j % 3 == 0 else v for j, v in enumerate(vals)]
    vals = [vals[i] for i in rng.permutation(len(vals))]
    return from_ints(vals, n), np.zeros(len(vals), np.uint8)


def write_duplex_fastq(dirpath, seed, n_reads, n=24, read_len=30, gz=False, qual_of=None):
    """two FastQ files R1 / R2 without a UMI in the headers: molecules (a pair of random reads) sequenced several
    times, about half of the records from the other strand (R1 and R2 exchanged), with substitutions inside the first
    n / 2 nucleotides of either read and a few N.  qual_of(i) -> the quality letter of record i (default 'I').
    Returns [path of R1, path of R2]."""
    import gzip
    import os
    rng = np.random.default_rng(seed)
    os.makedirs(dirpath, exist_ok=True)
    h = n // 2
    n_mol = max(1, n_reads // 5)
    mol = rng.integers(0, 4, size=(n_mol, 2, read_len))
    names = [os.path.join(dirpath, "in_R%d.fastq%s" % (k, ".gz" if gz else "")) for k in (1, 2)]
    op = gzip.open if gz else open
    with op(names[0], "wt") as f1, op(names[1], "wt") as f2:
        for i in range(n_reads):
            pair = mol[int(rng.integers(0, n_mol))].copy()
            if rng.random() < 0.3:
                pair[int(rng.integers(0, 2)), int(rng.integers(0, h))] = int(rng.integers(0, 4))
            seqs = ["".join("ACGT"[x] for x in r) for r in pair]
            if rng.random() < 0.02:
                k = int(rng.integers(0, h))
                seqs[0] = seqs[0][:k] + "N" + seqs[0][k + 1:]
            if rng.random() < 0.5:
                seqs.reverse()                                          # the other strand
            q = (qual_of(i) if qual_of else "I") * read_len
            f1.write("@read%d 1:N:0\n%s\n+\n%s\n" % (i, seqs[0], q))
            f2.write("@read%d 2:N:0\n%s\n+\n%s\n" % (i, seqs[1], q))
    return names
