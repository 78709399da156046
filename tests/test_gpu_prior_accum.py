"""-m gpu: the posterior's prior fed in chunks (humid_whitelist_prior_*, humid_whitelist_correct_posterior_prior;
Dedup.prior_begin / prior_add / correct_keys(prior=True)) against the truth of tests/whitelist_posterior_truth.py and
the one-shot correct_keys(quals=) over all reads.  Integer arithmetic: every comparison is exact.

The input is built so that a prior that forgets earlier chunks FAILS: the exact reads of barcodes that compete for the
same keys lie unevenly over the chunks, and the truth alone shows (asserted below) that reads with several candidates
exist and that some get another answer from the posterior over their chunk than from the posterior over all reads.

NOT tested here: the limit of 2^31 - 2 reads per barcode (HUMID_E_OVERFLOW, the invalid prior): it needs billions of
reads and is not simulated."""
import numpy as np
import pytest

import humid_amd

import whitelist_posterior_truth as pt

pytestmark = pytest.mark.gpu

U64 = np.uint64
K = 8
MIN_ODDS = 2
E_UNSUPPORTED, E_STATE = -2, -6
N_CHUNKS = 4


def sub(b, j, x):
    """barcode b with nucleotide j (0 = first) changed by x = 1 .. 3"""
    return int(b) ^ (x << (2 * (K - 1 - j)))


def build(seed=701, n=4000):
    """(whitelist, keys, quals, filtered, chunk bounds): 20 groups of three barcodes at mutual distance 2 -- b, and b
    changed at (i, j) and at (i, k) --; their midpoints are one substitution from two or three of them.  Barcode t of
    group g has nearly all of its exact reads in chunk (g + t) % 4."""
    rng = np.random.default_rng(seed)
    groups, seen = [], set()
    while len(groups) < 20:
        b = int(rng.integers(0, 4 ** K))
        i, j, k = (int(v) for v in rng.choice(K, size=3, replace=False))
        xi, xj, xk = (int(v) for v in rng.integers(1, 4, size=3))
        trio = [b, sub(sub(b, i, xi), j, xj), sub(sub(b, i, xi), k, xk)]
        near = set(trio) | {sub(t, p, x) for t in trio for p in range(K) for x in (1, 2, 3)}
        if near & seen:
            continue                                                 # (groups stay two substitutions apart at least)
        seen |= near
        # three candidates (b and both others), then two each: (b, second), (b, third), (second, third)
        groups.append((trio, [sub(b, i, xi), sub(b, j, xj), sub(b, k, xk), sub(sub(sub(b, i, xi), j, xj), k, xk)]))
    wl = np.asarray([t for trio, _ in groups for t in trio], U64)
    size = n // N_CHUNKS
    bounds = [(c * size, (c + 1) * size) for c in range(N_CHUNKS)]
    keys = np.zeros(n, U64)
    for c, (lo, hi) in enumerate(bounds):
        for r in range(lo, hi):
            g = int(rng.integers(0, len(groups)))
            trio, mids = groups[g]
            u = rng.random()
            if u < 0.62:                                             # an exact read: mostly the barcode at home in this chunk
                home = [t for t in range(3) if (g + t) % N_CHUNKS == c]
                t = home[0] if home and rng.random() < 0.95 else int(rng.integers(0, 3))
                keys[r] = trio[t]
            elif u < 0.90:                                           # a midpoint: two or three candidates
                keys[r] = mids[int(rng.integers(0, len(mids)))]
            elif u < 0.95:                                           # one substitution from one barcode
                keys[r] = sub(trio[int(rng.integers(0, 3))], int(rng.integers(0, K)), int(rng.integers(1, 4)))
            else:
                keys[r] = int(rng.integers(0, 4 ** K))
    quals = (rng.choice(np.asarray([2, 12, 25, 37]), size=(n, K)) + 33).astype(np.uint8)
    filt = (rng.random(n) < 0.03).astype(np.uint8)
    keys[filt != 0] = U64(0xFFFFFFFFFFFFFFFF)                         # (never read)
    return wl, keys, quals, filt, bounds


@pytest.fixture(scope="module")
def case():
    wl, keys, quals, filt, bounds = build()
    whole = pt.posterior(keys, quals, filt, wl, K, MIN_ODDS)
    # the condition, from the truth alone: several candidates exist, and the chunk's own prior gives other answers
    assert whole[2]["multi"] >= 20
    differ = []
    for lo, hi in bounds:
        alone = pt.posterior(keys[lo:hi], quals[lo:hi], filt[lo:hi], wl, K, MIN_ODDS)
        differ.append(int(((alone[0] != whole[0][lo:hi]) | (alone[1] != whole[1][lo:hi])).sum()))
    assert sum(differ) >= 5 and len(wl) == len(set(int(w) for w in wl)) == 60, differ
    bounds = [bounds[c] for c in sorted(range(len(bounds)), key=lambda c: -differ[c])]    # (the chunk that differs most comes first)
    return wl, keys, quals, filt, bounds, whole


@pytest.fixture(scope="module", params=[1, 0], ids=["wave_cooperative", "lane_serial"])
def dd(request):
    """the two forms of the decision kernel (option "whitelist_coop")"""
    d = humid_amd.Dedup()
    d.set_option("whitelist_coop", request.param)
    yield d
    d.close()


def n_w_of(truth, wl):
    return np.asarray([truth[3].get(int(w), 0) for w in wl], np.uint32)


def corrected_in_chunks(d, keys, quals, filt, pieces):
    """prior_begin, every chunk added, every chunk corrected against the accumulated prior -> (keys_out, status, summed
    summary)"""
    d.prior_begin()
    for lo, hi in pieces:
        d.prior_add(keys[lo:hi], filt[lo:hi])
    out, status = np.zeros(len(keys), U64), np.zeros(len(keys), np.uint8)
    total = dict(counts=np.zeros(5, np.uint64), multi=0, rescued=0)
    for lo, hi in pieces[::-1]:                                      # (the order is free)
        o, s, counts, extra = d.correct_keys(keys[lo:hi], filt[lo:hi], quals=quals[lo:hi], min_odds=MIN_ODDS, prior=True)
        out[lo:hi], status[lo:hi] = o, s
        assert list(counts) == list(extra["counts"]) == [int(x) for x in np.bincount(s, minlength=5)]
        total["counts"] += counts
        total["multi"] += extra["multi"]
        total["rescued"] += extra["rescued"]
    return out, status, total


def test_every_chunk_gets_what_the_one_shot_gives_over_all_reads(dd, case):
    wl, keys, quals, filt, bounds, whole = case
    dd.set_whitelist(wl, K)
    o1, s1, c1, x1 = dd.correct_keys(keys, filt, quals=quals, min_odds=MIN_ODDS)          # the one-shot over all reads
    assert np.array_equal(o1, whole[0]) and np.array_equal(s1, whole[1]) and x1 == whole[2]
    out, status, total = corrected_in_chunks(dd, keys, quals, filt, bounds)
    assert np.array_equal(out, o1) and np.array_equal(status, s1)
    assert [int(x) for x in total["counts"]] == whole[2]["counts"]
    assert total["multi"] == whole[2]["multi"] and total["rescued"] == whole[2]["rescued"]
    assert np.array_equal(dd.whitelist_counts(wl), n_w_of(whole, wl))


@pytest.mark.parametrize("size", [1, 64, 65])
def test_chunk_sizes_around_a_wave(dd, case, size):
    wl, keys, quals, filt, _, _ = case
    keys, quals, filt = keys[:300], quals[:300], filt[:300]
    want = pt.posterior(keys, quals, filt, wl, K, MIN_ODDS)
    dd.set_whitelist(wl, K)
    pieces = [(a, min(a + size, 300)) for a in range(0, 300, size)]
    out, status, total = corrected_in_chunks(dd, keys, quals, filt, pieces)
    assert np.array_equal(out, want[0]) and np.array_equal(status, want[1])
    assert [int(x) for x in total["counts"]] == want[2]["counts"] and total["multi"] == want[2]["multi"] \
        and total["rescued"] == want[2]["rescued"]
    assert np.array_equal(dd.whitelist_counts(wl), n_w_of(want, wl))


def test_the_one_shot_posterior_and_the_prior_leave_each_other_alone(dd, case):
    wl, keys, quals, filt, bounds, whole = case
    dd.set_whitelist(wl, K)
    dd.prior_begin()
    for lo, hi in bounds:
        dd.prior_add(keys[lo:hi], filt[lo:hi])
    dd.prior_add(keys[:0], filt[:0])                                 # a chunk of no reads
    dd.prior_add(keys[:100], np.ones(100, np.uint8))                 # a chunk of filtered reads only
    lo, hi = bounds[0]                                               # the chunk whose own prior differs most
    alone = pt.posterior(keys[lo:hi], quals[lo:hi], filt[lo:hi], wl, K, MIN_ODDS)
    o, s, _, x = dd.correct_keys(keys[lo:hi], filt[lo:hi], quals=quals[lo:hi], min_odds=MIN_ODDS)    # one-shot: the chunk's own prior
    assert np.array_equal(o, alone[0]) and np.array_equal(s, alone[1]) and x == alone[2]
    assert np.array_equal(dd.whitelist_counts(wl), n_w_of(alone, wl))                                # (the later call's counts)
    o, s, _, x = dd.correct_keys(keys[lo:hi], filt[lo:hi], quals=quals[lo:hi], min_odds=MIN_ODDS, prior=True)
    assert np.array_equal(o, whole[0][lo:hi]) and np.array_equal(s, whole[1][lo:hi])
    assert not (np.array_equal(o, alone[0]) and np.array_equal(s, alone[1]))
    assert np.array_equal(dd.whitelist_counts(wl), n_w_of(whole, wl))


def refused(code, fn, *args, **kw):
    with pytest.raises(humid_amd.HumidError) as ei:
        fn(*args, **kw)
    assert ei.value.code == code, ei.value


def test_lifetime_and_states(case):
    wl, keys, quals, filt, bounds, whole = case
    d = humid_amd.Dedup()
    try:
        k, q, f = keys[:500], quals[:500], filt[:500]
        refused(E_STATE, d.prior_begin)                              # no whitelist
        refused(E_STATE, d.prior_add, k, f)
        d.set_whitelist(wl, K)
        refused(E_STATE, d.prior_add, k, f)                          # a whitelist, but no prior yet
        refused(E_STATE, d.correct_keys, k, f, quals=q, min_odds=MIN_ODDS, prior=True)
        d.prior_begin()
        d.prior_add(k, f)
        d.correct_keys(k, f, quals=q, min_odds=MIN_ODDS, prior=True)
        with pytest.raises(ValueError):
            d.correct_keys(k, f, prior=True)
        d.set_whitelist(wl[:30], K)                                  # another list: the prior went with the table it indexed
        refused(E_STATE, d.prior_add, k, f)
        refused(E_STATE, d.correct_keys, k, f, quals=q, min_odds=MIN_ODDS, prior=True)
        refused(E_STATE, d.whitelist_counts, wl[:30])
        d.prior_begin()
        d.prior_add(k, f)
        want = pt.posterior(k, q, f, wl[:30], K, MIN_ODDS)
        o, s, _, x = d.correct_keys(k, f, quals=q, min_odds=MIN_ODDS, prior=True)
        assert np.array_equal(o, want[0]) and np.array_equal(s, want[1]) and x == want[2]
        d.discover_whitelist(k, f, barcode_nt=K, top=10)             # a discovered whitelist ends it as well
        refused(E_STATE, d.prior_add, k, f)
        bc = d.barcode_counter(barcode_nt=K)
        bc.add(k, f)
        d.prior_begin()
        bc.finish(top=10)                                            # ... and so does the counter's finish
        refused(E_STATE, d.prior_add, k, f)
        d.prior_begin()
        d.set_whitelist(None)                                        # ... and a clear
        refused(E_STATE, d.prior_add, k, f)
        refused(E_STATE, d.prior_begin)
        d.set_whitelist_segments([wl[:10] & U64(0xFF), wl[:10] >> U64(8)], [4, 4])
        refused(E_UNSUPPORTED, d.prior_begin)
        refused(E_UNSUPPORTED, d.prior_add, k, f)
    finally:
        d.close()


def test_device_pointers(dd, case):
    import torch
    wl, keys, quals, filt, bounds, whole = case
    dd.set_whitelist(wl, K)
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    dq = torch.from_numpy(quals).cuda()
    df = torch.from_numpy(filt).cuda()
    do = torch.zeros(len(keys), dtype=torch.int64, device="cuda")
    ds = torch.zeros(len(keys), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dd.prior_begin()
    for lo, hi in bounds:
        dd.prior_add_device(dk.data_ptr() + 8 * lo, df.data_ptr() + lo, hi - lo)
    multi = 0
    for lo, hi in bounds:
        multi += dd.correct_keys_prior_device(dk.data_ptr() + 8 * lo, dq.data_ptr() + K * lo, df.data_ptr() + lo,
                                              do.data_ptr() + 8 * lo, ds.data_ptr() + lo, hi - lo, min_odds=MIN_ODDS)["multi"]
    assert np.array_equal(do.cpu().numpy().view(U64), whole[0]) and np.array_equal(ds.cpu().numpy(), whole[1])
    assert multi == whole[2]["multi"]
