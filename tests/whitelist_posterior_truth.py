"""Two independent truths of the barcode correction by quality and abundance (include/humid_hip.h,
humid_whitelist_correct_posterior) in Python integers, and the generators its tests share.

TEST HELPER, never product code.

posterior():            per read that missed, set lookups of its 3 K one-substitution variants.
posterior_all_pairs():  per read that missed, its Hamming distance (over the K nucleotides) to EVERY whitelist entry:
                        no variants, no sets.  Quadratic: small inputs only.
Both return (key_out u64[N], status u8[N], summary dict(counts, multi, rescued), n_w dict barcode -> exact reads).
"""
import numpy as np

from whitelist_truth import (AMBIGUOUS, CORRECTED, EXACT, FILTERED, UNMATCHED, U64, midpoints,  # noqa: F401
                             random_barcodes, substitute, whitelist_with_neighbours)

# the literal table of the header; test_whitelist_posterior_host.py holds it against E_formula()
E = [16777216, 13326616, 10585708, 8408526, 6679130, 5305422, 4214246, 3347495, 2659010, 2112126, 1677722,
     1332662, 1058571, 840853, 667913, 530542, 421425, 334749, 265901, 211213, 167772, 133266,
     105857, 84085, 66791, 53054, 42142, 33475, 26590, 21121, 16777, 13327, 10586,
     8409, 6679, 5305, 4214, 3347, 2659, 2112, 1678]


def E_formula(q):
    """floor(2^24 * 10^(-q / 10) + 0.5) in exact integers: the largest e with (2 e - 1)^10 * 10^q <= 2^250"""
    lo, hi = 0, 1 << 25
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if (2 * mid - 1) ** 10 * 10 ** q <= 1 << 250:      # mid - 1/2 <= 2^24 * 10^(-q/10)
            lo = mid
        else:
            hi = mid
    return lo


def q_of(byte):
    return min(min(max(int(byte) - 33, 0), 93), 40)


def decide(cands, min_odds):
    """cands: [(barcode, weight)], not empty -> (key_out or None, status)"""
    total = sum(w for _, w in cands)
    best_b, best_w = min(cands, key=lambda c: (-c[1], c[0]))
    if best_w >= min_odds * (total - best_w):
        return best_b, CORRECTED
    return None, AMBIGUOUS


def _priors(keys, usable, W):
    n_w = {}
    for r in usable:
        k = int(keys[r])
        if k in W:
            n_w[k] = n_w.get(k, 0) + 1
    return n_w


def _run(keys, quals, filtered, whitelist, k, min_odds, candidates):
    assert min_odds >= 1
    keys = np.asarray(keys, U64)
    f = np.asarray(filtered, np.uint8)
    quals = np.asarray(quals, np.uint8).reshape(len(f), k)
    W = set(int(w) for w in np.asarray(whitelist, U64))
    usable = np.flatnonzero(f == 0)
    n_w = _priors(keys, usable, W)
    out = np.zeros(len(f), U64)
    status = np.zeros(len(f), np.uint8)
    multi = rescued = 0
    for r in usable:
        key = int(keys[r])
        out[r] = key
        if key in W:
            status[r] = EXACT
            continue
        cands = [(w, (n_w.get(w, 0) + 1) * E[q_of(quals[r, j])]) for w, j in candidates(key)]
        if not cands:
            status[r] = UNMATCHED
            continue
        won, st = decide(cands, min_odds)
        status[r] = st
        if won is not None:
            out[r] = won
        if len(cands) >= 2:
            multi += 1
            rescued += st == CORRECTED
    counts = [int(x) for x in np.bincount(status, minlength=5)]
    return out, status, dict(counts=counts, multi=int(multi), rescued=int(rescued)), n_w


def posterior(keys, quals, filtered, whitelist, k, min_odds=39):
    """the definition through set lookups of the variants"""
    W = set(int(w) for w in np.asarray(whitelist, U64))

    def candidates(key):
        # nucleotide j sits at bits 2 (k - 1 - j)
        return [(key ^ (x << (2 * (k - 1 - j))), j) for j in range(k) for x in (1, 2, 3) if key ^ (x << (2 * (k - 1 - j))) in W]
    return _run(keys, quals, filtered, whitelist, k, min_odds, candidates)


def posterior_all_pairs(keys, quals, filtered, whitelist, k, min_odds=39):
    """the definition through the distance of the key to every whitelist entry"""
    Ws = sorted(set(int(w) for w in np.asarray(whitelist, U64)))

    def candidates(key):
        out = []
        for w in Ws:
            x = key ^ w
            if x >> (2 * k):                                # bits above 2 K: no barcode is near
                continue
            diff = [j for j in range(k) if (x >> (2 * (k - 1 - j))) & 3]
            if len(diff) == 1:
                out.append((w, diff[0]))
        return out
    return _run(keys, quals, filtered, whitelist, k, min_odds, candidates)


def plain_from_posterior(status_plain, status_post):
    """the superset rule: the statuses differ from the plain correction's only where that one says AMBIGUOUS"""
    differ = np.flatnonzero(np.asarray(status_plain) != np.asarray(status_post))
    return bool(np.all(np.asarray(status_plain)[differ] == AMBIGUOUS))


def make_case(rng, n, k, n_wl=300, p_filt=0.03):
    """A whitelist with neighbours, n keys (exact, one and two substitutions, random, planted midpoints, garbage under
    filtered reads, a few with bits above 2 K) and per-base quality bytes from the whole byte range's interesting
    parts (below 33, 33 .. 73, above 126); rows of filtered reads carry garbage too.  Returns (whitelist, keys,
    quals u8[n, k], filtered)."""
    n_wl = min(n_wl, max(4 ** k // 2, 1)) if k < 6 else n_wl
    wl = whitelist_with_neighbours(rng, n_wl, k)
    keys = wl[rng.integers(0, len(wl), size=n)] if n else np.zeros(0, U64)
    u = rng.random(n)
    one = np.flatnonzero(u < 0.25)
    two = np.flatnonzero((u >= 0.25) & (u < 0.30))
    rnd = np.flatnonzero((u >= 0.30) & (u < 0.33))
    keys[one] = substitute(rng, keys[one], k)
    keys[two] = substitute(rng, substitute(rng, keys[two], k), k)
    keys[rnd] = random_barcodes(rng, len(rnd), k)
    mids = midpoints(wl, k)
    if len(mids) and n >= 8:
        at = rng.choice(n, size=max(n // 6, 2), replace=False)
        keys[at] = mids[rng.integers(0, len(mids), size=len(at))]
    if k < 32 and n >= 16:
        at = rng.choice(n, size=2, replace=False)
        keys[at] |= U64(1) << U64(2 * k)                    # bits above 2 K
    quals = rng.integers(33, 74, size=(n, k), dtype=np.uint8)
    odd = rng.random((n, k))
    quals[odd < 0.02] = 5                                   # below 33: q = 0
    quals[odd > 0.98] = 200                                 # above 126: q = 40
    filt = (rng.random(n) < p_filt).astype(np.uint8)
    sel = np.flatnonzero(filt)
    keys[sel] = rng.integers(0, 1 << 64, size=len(sel), dtype=U64)
    quals[sel] = rng.integers(0, 256, size=(len(sel), k), dtype=np.uint8)
    return wl, keys.astype(U64, copy=False), quals, filt


def key_of(seq):
    """ACGT string -> packed word (A C G T = 0 1 2 3, first nucleotide most significant)"""
    v = 0
    for ch in seq:
        v = (v << 2) | "ACGT".index(ch)
    return v


def hand_cases():
    """The odds boundary by hand, K = 2: the key AC has AA one substitution away (at nucleotide 1) and CC (at
    nucleotide 0).  Every case: dict(name, whitelist, k, keys, quals, filtered, min_odds, status, key_out) with status
    and key_out of the LAST read (the query; the reads in front are the exact reads that make the priors)."""
    AA, AC, AG, CC = key_of("AA"), key_of("AC"), key_of("AG"), key_of("CC")

    def case(name, wl, exact, qrow, min_odds, status, key_out):
        keys = np.asarray(list(exact) + [AC], U64)
        quals = np.full((len(keys), 2), 33 + 30, np.uint8)
        quals[-1] = qrow
        return dict(name=name, whitelist=np.asarray(wl, U64), k=2, keys=keys, quals=quals, filtered=np.zeros(len(keys), np.uint8),
                    min_odds=min_odds, status=status, key_out=key_out)
    out = []
    # equal priors: AA's weight is E[q of nucleotide 1], CC's E[q of nucleotide 0]; E[q] >= 39 E[q + 16] > E[q] / 39 > E[q + 15] ...
    for q in (0, 7, 24):
        out.append(case("q%d_vs_q%d" % (q, q + 16), [AA, CC], [], [33 + q + 16, 33 + q], 39, CORRECTED, AA))
        out.append(case("q%d_vs_q%d" % (q, q + 15), [AA, CC], [], [33 + q + 15, 33 + q], 39, AMBIGUOUS, AC))
        out.append(case("q%d_vs_q%d_swapped" % (q, q + 16), [AA, CC], [], [33 + q, 33 + q + 16], 39, CORRECTED, CC))
    # equal qualities: 38 exact reads of AA against none of CC are 39 : 1
    out.append(case("38_exact", [AA, CC], [AA] * 38, [63, 63], 39, CORRECTED, AA))
    out.append(case("37_exact", [AA, CC], [AA] * 37, [63, 63], 39, AMBIGUOUS, AC))
    out.append(case("38_exact_of_the_larger", [AA, CC], [CC] * 38, [63, 63], 39, CORRECTED, CC))
    # a tie: ambiguous at 39, the smaller barcode at 1
    out.append(case("tie_39", [AA, CC], [], [63, 63], 39, AMBIGUOUS, AC))
    out.append(case("tie_1", [AA, CC], [], [63, 63], 1, CORRECTED, AA))
    out.append(case("tie_1_with_priors", [AA, CC], [AA, CC], [63, 63], 1, CORRECTED, AA))
    # three candidates (AA and AG at nucleotide 1, CC at nucleotide 0): 79 >= 39 * 2, 77 < 78 although 77 >= 39 * 1
    out.append(case("three_78_exact", [AA, AG, CC], [AA] * 78, [63, 63], 39, CORRECTED, AA))
    out.append(case("three_76_exact", [AA, AG, CC], [AA] * 76, [63, 63], 39, AMBIGUOUS, AC))
    out.append(case("two_76_exact", [AA, CC], [AA] * 76, [63, 63], 39, CORRECTED, AA))
    return out


def posterior_np(keys, quals, filtered, whitelist, k, min_odds=39):
    """posterior() over whole arrays (binary searches in the sorted whitelist; the weights in u64, the one product
    that may pass 64 bits in Python integers), for read sets the Python loops take too long over; the host tests
    hold it against the other two.  Returns the same four values."""
    Ws = np.unique(np.asarray(whitelist, U64))
    keys = np.asarray(keys, U64)
    f = np.asarray(filtered, np.uint8)
    n = len(f)
    quals = np.asarray(quals, np.uint8).reshape(n, k)
    Et = np.asarray(E, U64)

    def find(x):
        i = np.minimum(np.searchsorted(Ws, x), len(Ws) - 1)
        return i, Ws[i] == x
    out = np.zeros(n, U64)
    status = np.zeros(n, np.uint8)
    usable = np.flatnonzero(f == 0)
    ku = keys[usable]
    idx, exact = find(ku) if len(ku) else (np.zeros(0, np.int64), np.zeros(0, bool))
    n_per = np.bincount(idx[exact], minlength=len(Ws)).astype(U64)
    out[usable] = ku
    status[usable] = EXACT
    miss = usable[~exact]
    km = keys[miss]
    total = np.zeros(len(miss), U64)
    best_w = np.zeros(len(miss), U64)
    best_b = np.zeros(len(miss), U64)
    n_cand = np.zeros(len(miss), np.int64)
    if len(miss):
        q = np.minimum(np.maximum(quals[miss].astype(np.int64) - 33, 0), 40)
        for v in range(3 * k):
            var = km ^ (U64(1 + v % 3) << U64(2 * (v // 3)))
            i, hit = find(var)
            w = np.where(hit, (n_per[i] + U64(1)) * Et[q[:, k - 1 - v // 3]], U64(0))
            total += w
            n_cand += hit
            better = hit & ((w > best_w) | ((w == best_w) & (var < best_b)))
            best_w = np.where(better, w, best_w)
            best_b = np.where(better, var, best_b)
    rest = total - best_w
    wins = np.asarray([int(b) >= min_odds * int(r) for b, r in zip(best_w, rest)], bool) if len(miss) else np.zeros(0, bool)
    st = np.where(n_cand == 0, UNMATCHED, np.where(wins, CORRECTED, AMBIGUOUS)).astype(np.uint8)
    status[miss] = st
    out[miss] = np.where(st == CORRECTED, best_b, km)
    multi = n_cand >= 2
    summary = dict(counts=[int(x) for x in np.bincount(status, minlength=5)], multi=int(multi.sum()),
                   rescued=int((multi & (st == CORRECTED)).sum()))
    n_w = {int(w): int(c) for w, c in zip(Ws, n_per) if c}
    return out, status, summary, n_w
