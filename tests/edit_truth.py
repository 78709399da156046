"""Pairs of words placed on purpose for the edit-distance (-e) search: TEST HELPER, never product code.

Plain Python.  It knows one thing about the search: the documented segment layout -- a word of n nucleotides is cut
into s segments, the remainder n % s spread over the first ones.  For every choice of the d damaged segments (the other
k = s - d stay untouched) and every assignment of edit kinds to them -- p deletions and p insertions, 0 <= p <= d / 2,
in every order, substitutions for the rest -- a pair (x, y) with exactly ONE edit in each damaged segment, the edit at
the first, the last and an interior position of its segment.  Every offset vector the untouched segments can show
between two words within d edits occurs that way, (+1, -1) and (2, 1) at d = 4 included.

The truth these pairs are checked against is oracle.pyoracle.edit_adjacency_allpairs / lev_pairs (the literal two-row
dynamic programme), never anything in this file.
"""
import itertools

import numpy as np

MODES = ("first", "last", "interior")


def segments(n, s):
    """[(start, length)] of the s segments of an n-nucleotide word: lengths n // s, one more for the first n % s"""
    base, rem = divmod(n, s)
    out, pos = [], 0
    for t in range(s):
        ln = base + (1 if t < rem else 0)
        out.append((pos, ln))
        pos += ln
    return out


def kind_assignments(d):
    """every tuple over S(ubstitution) / D(eletion) / I(nsertion) of length d with as many D as I"""
    return [k for k in itertools.product("SDI", repeat=d) if k.count("D") == k.count("I")]


def _position(seg, mode):
    start, ln = seg
    return start if mode == "first" else start + ln - 1 if mode == "last" else start + ln // 2


def apply_edits(rng, x, ops, alphabet, after=False):
    """y = x with the edits ops {position of x: kind}: S changes the letter, D drops it, I puts a new letter in front
    of it (after = True: behind it)"""
    y = []
    for i, c in enumerate(x):
        k = ops.get(i)
        if k is None:
            y.append(c)
        elif k == "S":
            y.append((c + 1 + int(rng.integers(0, alphabet - 1))) % alphabet)
        elif k == "I":
            ins = int(rng.integers(0, alphabet))
            y.extend([c, ins] if after else [ins, c])
    return y


def placed_pairs(rng, n, d, s, alphabet=4):
    """(X u8[P, n], Y u8[P, n], meta): meta[r] = (damaged segments, kinds, mode) of pair r.  Every pair over a random
    x of its own."""
    segs = segments(n, s)
    X, Y, meta = [], [], []
    for damaged in itertools.combinations(range(s), d):
        for kinds in kind_assignments(d):
            seen = set()
            for mode in MODES:
                pos = tuple(_position(segs[t], mode) for t in damaged)
                after = mode == "last"
                key = (pos, after and "I" in kinds)
                if key in seen:                       # short segments: the interior position is the first or last one
                    continue
                seen.add(key)
                x = rng.integers(0, alphabet, size=n).tolist()
                y = apply_edits(rng, x, dict(zip(pos, kinds)), alphabet, after)
                assert len(y) == n
                X.append(x)
                Y.append(y)
                meta.append((damaged, kinds, mode))
    return np.asarray(X, np.uint8).reshape(-1, n), np.asarray(Y, np.uint8).reshape(-1, n), meta


def edge_indel_pairs(rng, n, alphabet=4):
    """one deletion + one insertion at the places where the word's ends and (n > 32) the boundary between its two
    machine words lie: positions 0 and n - 1, and n - 33, n - 32, n - 31"""
    sites = [(0, n - 1), (n - 1, 0), (0, n // 2), (n // 2, n - 1), (n - 1, n // 2), (n // 2, 0)]
    if n > 32:
        for q in (n - 33, n - 32, n - 31):
            if 0 <= q < n:
                sites += [(q, n - 1), (q, 0), (0, q), (n - 1, q), (q, q + 1 if q + 1 < n else q - 1)]
    X, Y = [], []
    for a, b in sites:
        x = rng.integers(0, alphabet, size=n).tolist()
        y = x[:a] + x[a + 1:]                          # x[a] deleted ...
        y.insert(b, int(rng.integers(0, alphabet)))    # ... a new letter at index b of the result
        X.append(x)
        Y.append(y)
    return np.asarray(X, np.uint8), np.asarray(Y, np.uint8)


def all_pairs(seed, n, d, s):
    """what the sweep feeds for (n, d, s): the placed pairs over 4 letters and over 2 letters (repeats give other
    alignments), and the edge indels over both"""
    rng = np.random.default_rng(seed)
    xs, ys, meta = [], [], []
    for alphabet in (4, 2):
        x, y, m = placed_pairs(rng, n, d, s, alphabet)
        xs.append(x)
        ys.append(y)
        meta += [(alphabet,) + t for t in m]
        x, y = edge_indel_pairs(rng, n, alphabet)
        xs.append(x)
        ys.append(y)
        meta += [(alphabet, (), ("D", "I"), "edge")] * len(x)
    return np.concatenate(xs), np.concatenate(ys), meta


def pack(rows):
    """rows of nucleotide codes u8[N, n] -> u64[N] (n <= 32) or u64[N, 2] ([:, 0] = the first n - 32 nucleotides)"""
    rows = np.asarray(rows)
    n = rows.shape[1]
    if n <= 32:
        w = np.zeros(len(rows), np.uint64)
        for t in range(n):
            w = (w << np.uint64(2)) | rows[:, t].astype(np.uint64)
        return w
    return np.stack([pack(rows[:, :n - 32]), pack(rows[:, n - 32:])], 1)


def unique_words(words):
    """the ascending unique words (rows [hi, lo] in lexicographic order)"""
    w = np.asarray(words, np.uint64)
    return np.unique(w, axis=0) if w.ndim == 2 else np.unique(w)


def nt_string(word, n):
    """a packed word (int, or [hi, lo]) as nucleotides, for messages"""
    v = (int(word[0]) << 64) | int(word[1]) if np.ndim(word) else int(word)
    return "".join("ACGT"[(v >> (2 * (n - 1 - i))) & 3] for i in range(n))


def n_placed(n, d, s):
    """an upper bound of the pairs all_pairs() makes (for sizing test cases without generating)"""
    combos = len(list(itertools.combinations(range(s), d)))
    return 2 * (combos * len(kind_assignments(d)) * 3 + (6 + (15 if n > 32 else 0)))
