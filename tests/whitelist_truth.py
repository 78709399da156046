"""Two independent truths of the barcode whitelist correction (include/humid_hip.h, humid_whitelist_correct) in
numpy / plain Python, and the generators the whitelist tests share.

TEST HELPER, never product code.

correct():            per distinct key, a set lookup of the key and of its 3 K one-substitution variants.
correct_np():         the same as correct() in whole-array numpy (binary searches in the sorted whitelist), for read
                      sets the Python loop takes minutes over; the host tests hold it against the other two.
correct_all_pairs():  per distinct key, its Hamming distance (over the K nucleotides) to EVERY whitelist entry: no
                      variants, no sets.  Quadratic: small inputs only.
All three return (key_out u64[N], status u8[N], counts u64[5]).
"""
import numpy as np

U64 = np.uint64
TOP = (1 << 64) - 1
FILTERED, EXACT, CORRECTED, AMBIGUOUS, UNMATCHED = range(5)


def _finish(keys, filtered, per_key):
    keys = np.asarray(keys, U64)
    f = np.asarray(filtered, np.uint8)
    out = np.zeros(len(f), U64)
    status = np.zeros(len(f), np.uint8)
    usable = np.flatnonzero(f == 0)
    if len(usable):
        uniq, inv = np.unique(keys[usable], return_inverse=True)
        res = [per_key(int(k)) for k in uniq]
        out[usable] = np.asarray([r[0] for r in res], U64)[inv]
        status[usable] = np.asarray([r[1] for r in res], np.uint8)[inv]
    return out, status, np.bincount(status, minlength=5).astype(U64)


def correct(keys, filtered, whitelist, k):
    """the definition through set lookups"""
    W = set(int(w) for w in np.asarray(whitelist, U64))

    def per_key(key):
        if key in W:
            return key, EXACT
        hits = [key ^ (x << (2 * p)) for p in range(k) for x in (1, 2, 3) if key ^ (x << (2 * p)) in W]
        if len(hits) == 1:
            return hits[0], CORRECTED
        return key, AMBIGUOUS if hits else UNMATCHED
    return _finish(keys, filtered, per_key)


def correct_np(keys, filtered, whitelist, k):
    """correct() over whole arrays: membership by binary search in the sorted distinct whitelist"""
    W = np.unique(np.asarray(whitelist, U64))
    keys = np.asarray(keys, U64)
    f = np.asarray(filtered, np.uint8)
    out = np.zeros(len(f), U64)
    status = np.zeros(len(f), np.uint8)
    usable = np.flatnonzero(f == 0)

    def member(x):
        i = np.minimum(np.searchsorted(W, x), len(W) - 1)
        return W[i] == x
    ku = keys[usable]
    exact = np.zeros(len(ku), bool)
    if len(ku):
        order = np.argsort(ku)                                      # (a binary search per SORTED needle is many times faster)
        exact[order] = member(ku[order])
    out[usable] = ku
    status[usable] = EXACT
    if not exact.all():
        miss, inv = np.unique(ku[~exact], return_inverse=True)     # (only the keys that missed are made distinct)
        n_hit = np.zeros(len(miss), np.int32)
        winner = np.zeros(len(miss), U64)
        for v in range(3 * k):
            var = miss ^ (U64(1 + v % 3) << U64(2 * (v // 3)))
            h = member(var)
            n_hit += h
            winner = np.where(h, var, winner)
        st = np.where(n_hit == 1, CORRECTED, np.where(n_hit >= 2, AMBIGUOUS, UNMATCHED)).astype(np.uint8)
        at = usable[~exact]
        out[at] = np.where(n_hit == 1, winner, miss)[inv]
        status[at] = st[inv]
    return out, status, np.bincount(status, minlength=5).astype(U64)


def correct_all_pairs(keys, filtered, whitelist, k):
    """the definition through the distance of every distinct key to every whitelist entry"""
    W = sorted(set(int(w) for w in np.asarray(whitelist, U64)))
    low = 0x5555555555555555

    def per_key(key):
        near = []
        for w in W:
            x = key ^ w
            d = bin((x | (x >> 1)) & low).count("1") if x < (1 << (2 * k)) else k + 1    # bits above 2 K: no barcode
            if d == 0:
                return key, EXACT
            if d == 1:
                near.append(w)
        if len(near) == 1:
            return near[0], CORRECTED
        return key, AMBIGUOUS if near else UNMATCHED
    return _finish(keys, filtered, per_key)


def mix64(x):
    """the table's hash (common.hip.h)"""
    x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & TOP
    x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & TOP
    return x ^ (x >> 31)


def unmix64(x):
    """its inverse"""
    x = ((x ^ (x >> 31) ^ (x >> 62)) * 0x319642b2d24d8ec3) & TOP
    x = ((x ^ (x >> 27) ^ (x >> 54)) * 0x96de1b173f119089) & TOP
    return x ^ (x >> 30) ^ (x >> 60)


def random_barcodes(rng, n, k):
    """n values below 4^k (duplicates possible)"""
    if k == 32:
        return rng.integers(0, 1 << 64, size=n, dtype=U64)
    return rng.integers(0, 1 << (2 * k), size=n, dtype=U64)


def substitute(rng, keys, k):
    """every key with one nucleotide replaced by another one"""
    pos = rng.integers(0, k, size=len(keys)).astype(U64)
    x = rng.integers(1, 4, size=len(keys)).astype(U64)
    return keys ^ (x << (U64(2) * pos))


def make_keys(rng, whitelist, k, n, p1=0.05, p2=0.02, pr=0.02, p_filt=0.03):
    """The generator of the issue: n keys drawn from the whitelist, about 5 % of them with one substitution, 2 % with
    two, 2 % random, plus planted midpoints of whitelist pairs at distance 2 (a midpoint has both at distance 1) and a
    few filtered reads carrying garbage keys.  Returns (keys u64[n], filtered u8[n])."""
    wl = np.asarray(whitelist, U64)
    keys = wl[rng.integers(0, len(wl), size=n)] if n else np.zeros(0, U64)
    u = rng.random(n)
    one = u < p1
    two = (u >= p1) & (u < p1 + p2)
    rnd = (u >= p1 + p2) & (u < p1 + p2 + pr)
    for sel in (np.flatnonzero(one | two), np.flatnonzero(two)):
        keys[sel] = substitute(rng, keys[sel], k)
    sel = np.flatnonzero(rnd)
    keys[sel] = random_barcodes(rng, len(sel), k)
    mids = midpoints(wl, k)
    if len(mids) and n >= 8:
        at = rng.choice(n, size=min(len(mids), max(n // 50, 2)), replace=False)
        keys[at] = mids[rng.integers(0, len(mids), size=len(at))]
    filt = (rng.random(n) < p_filt).astype(np.uint8)
    sel = np.flatnonzero(filt)
    keys[sel] = rng.integers(0, 1 << 64, size=len(sel), dtype=U64)
    return keys.astype(U64, copy=False), filt


def midpoints(whitelist, k, limit=64):
    """keys with two whitelist barcodes at distance 1: for a pair at distance 2 (positions p < q), the first with
    the second's nucleotide at p.  Pairs are looked for among the first hundred entries as given (where
    whitelist_with_neighbours plants them); none may exist."""
    wl = list(dict.fromkeys(int(w) for w in np.asarray(whitelist, U64)[:100]))
    low = 0x5555555555555555
    out = []
    for i, a in enumerate(wl):
        for b in wl[i + 1:]:
            x = a ^ b
            m = (x | (x >> 1)) & low
            if bin(m).count("1") == 2:
                p = (m & -m).bit_length() - 1                       # bit position of the lower differing nucleotide
                out.append(a ^ (x & (3 << p)))
                if len(out) >= limit:
                    return np.asarray(out, U64)
    return np.asarray(out, U64)


def whitelist_with_neighbours(rng, n, k):
    """n random barcodes of which some pairs lie at distance 2 (so that midpoints exist) and some at distance 1"""
    wl = random_barcodes(rng, n, k)
    m = min(n // 4, 40)
    if m and k >= 2:
        wl[:m] = substitute(rng, substitute(rng, wl[m:2 * m], k), k)      # distance <= 2 to wl[m : 2 m]
    if n >= 8:
        wl[-1] = substitute(rng, wl[-2:-1], k)[0]                     # a pair at distance 1
    return wl


def status_set(status):
    return set(int(s) for s in np.unique(status))
