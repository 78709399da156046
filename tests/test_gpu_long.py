"""-m gpu: words beyond 64 nucleotides (Dedup.run_long, humid_dedup_run_long).  Up to 64 nucleotides the C oracle is
the reference; beyond it tests/long_truth.py (numpy, pinned to the oracle by tests/test_long_truth_host.py)."""
import numpy as np
import pytest

import humid_amd
import long_truth as lt
from humid_amd.synth import synth_long_words, synth_wide_words, synth_words
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

U64 = np.uint64


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    yield d
    d.close()


def segments(n, d):
    """(first, last) nucleotide of the d + 1 contiguous segments of the search (lengths differ by at most one)"""
    s = d + 1
    base, rem, pos, out = n // s, n % s, 0, []
    for t in range(s):
        ln = base + (1 if t < rem else 0)
        out.append((pos, pos + ln - 1))
        pos += ln
    return out


def check_against_truth(dd, t, cid, keep, s, k):
    """everything the parity tests compare with the oracle, against a long_truth.long_dedup result"""
    for key in ("total", "usable", "unique", "clusters", "edges"):
        assert s[key] == t["summary"][key], (key, s[key], t["summary"][key])
    assert s["count_mode_used"] == 3
    assert np.array_equal(cid, t["cid"])
    assert np.array_equal(keep, t["keep"])
    if not s["unique"]:
        return
    lv, tlv = dd.leaves(), t["leaves"]
    assert lv["word"].shape == (s["unique"], k)
    assert np.array_equal(lv["word"], tlv["word"])
    assert np.array_equal(lv["count"].astype(U64), tlv["count"])
    assert np.array_equal(lv["first_read"], tlv["first_read"])
    assert np.array_equal(lv["degree"], tlv["degree"])
    assert np.array_equal(lv["cluster_id"], tlv["cluster_id"])
    assert np.array_equal(lv["is_max_leaf"], tlv["is_max_leaf"])
    off, idx = dd.adjacency()
    assert np.array_equal(off.astype(U64), t["off"])
    assert np.array_equal(idx, t["idx"])
    cl = dd.clusters()
    assert np.array_equal(cl["size"], t["clusters"]["size"])
    assert np.array_equal(cl["max_count"].astype(U64), t["clusters"]["max_count"])
    assert np.array_equal(cl["max_leaf"], t["clusters"]["max_leaf"])
    assert dd.histograms() == t["hist"]


def run_and_check(dd, words, filt, n, d, method):
    t = lt.long_dedup(words, filt, d, method, word_nt=n)
    cid, keep, s = dd.run_long(words, filt, n, distance=d, method=method)
    info = dd.long_info()
    check_against_truth(dd, t, cid, keep, s, (n + 31) // 32)
    assert info["words_per_read"] == (n + 31) // 32
    assert info["edges"] == t["summary"]["edges"]
    return t, s, info


# ---- A. oracle-anchored: the long kernels where the existing entry point also answers -------------------------------
@pytest.fixture(scope="module")
def short_inputs():
    out = {}
    for n in (1, 24, 32, 33, 48, 64):
        out[n] = synth_words(3000, 4100 + n, n, 0.01, 0.01) if n <= 32 else synth_wide_words(3000, 4100 + n, n, 0.01, 0.01)
    return out


def check_against_oracle(dd, words, filt, n, d, maximum):
    """tests/test_gpu_parity.py's helper, through run_long"""
    cid, keep, s = dd.run_long(words, filt, n, distance=d, method=int(maximum))
    p = orc.Pipeline(n)
    p.read_data(words, filt)
    p.find_hamming_neighbours(d)
    p.find_clusters(maximum)
    ocid, okeep = p.map_reads()
    os_ = p.summary()
    for k in ("total", "usable", "unique", "clusters", "edges"):
        assert s[k] == os_[k], (k, s[k], os_[k])
    assert s["count_mode_used"] == 3
    assert np.array_equal(cid, ocid)
    assert np.array_equal(keep, okeep)
    if s["unique"]:
        lv, olv = dd.leaves(), p.leaves()
        assert np.array_equal(lv["word"], olv["word"].reshape(lv["word"].shape))
        assert np.array_equal(lv["count"].astype(U64), olv["count"])
        assert np.array_equal(lv["degree"], olv["degree"])
        assert np.array_equal(lv["cluster_id"], olv["cluster_id"])
        assert np.array_equal(lv["is_max_leaf"], olv["is_max_leaf"])
        off, idx = dd.adjacency()
        ooff, oidx = p.adjacency()
        assert np.array_equal(off.astype(U64), ooff)
        assert np.array_equal(idx, oidx)
        cl, ocl = dd.clusters(), p.clusters()
        assert np.array_equal(cl["size"], ocl["size"])
        assert np.array_equal(cl["max_count"].astype(U64), ocl["max_count"])
        assert np.array_equal(cl["max_leaf"], ocl["max_leaf"])
        assert dd.histograms() == orc.histograms(p)
    return s


@pytest.mark.parametrize("maximum", [False, True])
@pytest.mark.parametrize("d", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 24, 32, 33, 48, 64])
def test_up_to_64_nt_equals_the_oracle(dd, short_inputs, n, d, maximum):
    words, filt = short_inputs[n]
    s = check_against_oracle(dd, words, filt, n, d, maximum)
    assert s["unique"] > (1000 if n > 1 else 3)
    info = dd.long_info()
    assert info["words_per_read"] == (n + 31) // 32
    assert info["joins"] == (1 if d >= n else d + 1)


# ---- B. truth-anchored --------------------------------------------------------------------------------------------------
def planted(words, filt, n, d, seed):
    """The issue's inputs, synth_long_words(3000, ., n, 0.01, 0.01), hold NO neighbour pair at n = 512: a read survives
    p_n = 0.01 with probability 0.99^512 (14 usable reads of 3000), and two reads of a molecule differ in ~10 places.
    So that no case passes vacuously, every case appends the same few reads to them: copies of the first usable words,
    three of each word itself and one copy each with 1 and with max(d, 1) substitutions at random places."""
    rng = np.random.default_rng(seed)
    base = words[filt == 0][:6]
    extra = []
    for w in base:
        extra += [w, w, w]
        for m in sorted({1, max(d, 1)}):
            v = w
            for pos in rng.choice(n, size=m, replace=False):
                v = lt.substitute(v, n, int(pos), int(rng.integers(1, 4)))
            extra.append(v)
    extra = np.array(extra, dtype=U64).reshape(-1, words.shape[1])
    return np.concatenate([words, extra]), np.concatenate([filt, np.zeros(len(extra), np.uint8)])


@pytest.fixture(scope="module")
def long_inputs():
    return {n: synth_long_words(3000, 9000 + n, n, 0.01, 0.01) for n in (65, 96, 97, 128, 150, 512)}


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("d", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [65, 96, 97, 128, 150, 512])
def test_long_words_equal_the_truth(dd, long_inputs, n, d, method):
    words, filt = planted(*long_inputs[n], n, d, seed=n)
    t, s, info = run_and_check(dd, words, filt, n, d, method)
    print(n, d, method, t["summary"], info)
    if d >= 1:
        assert s["edges"] > 0
        assert np.bincount(t["leaves"]["cluster_id"]).max() >= 2         # a cluster of several leaves
    assert info["joins"] == d + 1
    assert info["piece_joins"] == 0


# ---- C. boundaries, hand-built ------------------------------------------------------------------------------------------
def boundary_case(n, d, seed):
    rng = np.random.default_rng(seed)
    k = (n + 31) // 32
    r = n - 32 * (k - 1)
    base = lt.pack_syms(rng.integers(0, 4, size=(1, n)))[0]
    segs = segments(n, d)
    singles = {0, r - 1, r, n - 1}
    for j in range(1, k - 1):
        singles |= {r + 32 * j - 1, r + 32 * j}
    for a, b in segs:
        singles |= {a, b}
    variants = [lt.substitute(base, n, p) for p in sorted(p for p in singles if 0 <= p < n)]
    mid = [int(rng.integers(a, b + 1)) for a, b in segs]
    for untouched in range(d + 1):                          # d substitutions: found through the untouched segment only
        v = base
        for t, p in enumerate(mid):
            if t != untouched:
                v = lt.substitute(v, n, p, 2)
        variants.append(v)
    v = base
    for p in mid:                                           # d + 1 substitutions, one per segment: no neighbour of the base
        v = lt.substitute(v, n, p, 3)
    variants.append(v)
    rows, counts = [base], [10]
    for i, v in enumerate(variants):
        rows.append(v)
        counts.append(1 + i % 3)
    words = np.repeat(np.array(rows, dtype=U64), counts, axis=0)
    words = words[rng.permutation(len(words))]
    filt = np.zeros(len(words), np.uint8)
    return words, filt, len(variants)


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n", [65, 96, 97, 150])
def test_seams_and_segment_boundaries(dd, n, d):
    words, filt, n_variants = boundary_case(n, d, 100 * n + d)
    for method in (0, 1):
        t, s, info = run_and_check(dd, words, filt, n, d, method)
        assert s["unique"] == n_variants + 1 and info["joins"] == d + 1
        # the base word's neighbours: all single substitutions and the d-substitution variants, not the last one
        base_leaf = int(np.argmax(t["leaves"]["count"]))
        assert t["leaves"]["count"][base_leaf] == 10
        assert t["leaves"]["degree"][base_leaf] == n_variants - 1
        if (2 * n) % 64:
            # garbage in the ignored upper bits of the first uint64 of some reads changes nothing
            dirty = words.copy()
            hbits = 2 * (n - 32 * ((n + 31) // 32 - 1))
            dirty[::3, 0] |= U64(((1 << 64) - 1) ^ ((1 << hbits) - 1))
            dirty[1::3, 0] |= U64(1 << hbits)
            cid, keep, s2 = dd.run_long(dirty, filt, n, distance=d, method=method)
            check_against_truth(dd, t, cid, keep, s2, (n + 31) // 32)


# ---- D. against the two-word path at size ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide_run(dd):
    words, filt = synth_wide_words(50_000, 6464, 64, p_sub=5e-3)
    cid, keep, s = dd.run(words, filt, word_nt=64, distance=1)
    off, idx = dd.adjacency()
    lv = dd.leaves()
    return dict(words=words, filt=filt, cid=cid, keep=keep, s=s, off=off, idx=idx, lv=lv)


@pytest.mark.parametrize("shape", ["fill1", "fill33", "fill86", "prefix_suffix40"])
def test_longer_copies_of_64_nt_words_equal_the_two_word_run(dd, wide_run, shape):
    w2 = wide_run["words"]
    if shape.startswith("fill"):
        fill = int(shape[4:])
        words, n = lt.with_filler(w2, 64, fill, seed=fill), 64 + fill
    else:
        rng = np.random.default_rng(40)
        syms = lt.unpack_syms(w2, 64)
        pre, suf = rng.integers(0, 4, size=40), rng.integers(0, 4, size=40)
        words = lt.pack_syms(np.concatenate([np.tile(pre, (len(syms), 1)), syms, np.tile(suf, (len(syms), 1))], axis=1))
        n = 144
    cid, keep, s = dd.run_long(words, wide_run["filt"], n, distance=1)
    assert np.array_equal(cid, wide_run["cid"]) and np.array_equal(keep, wide_run["keep"])
    for key in ("usable", "unique", "clusters", "edges"):
        assert s[key] == wide_run["s"][key], key
    assert s["edges"] > 1000
    off, idx = dd.adjacency()
    assert np.array_equal(off, wide_run["off"]) and np.array_equal(idx, wide_run["idx"])
    lv = dd.leaves()
    for key in ("count", "degree", "cluster_id"):
        assert np.array_equal(lv[key], wide_run["lv"][key]), key


# ---- E. forced key collisions -----------------------------------------------------------------------------------------------
def test_two_key_bits_and_a_short_walk_change_nothing(dd, long_inputs):
    n, d = 150, 2
    words, filt = planted(*long_inputs[n], n, d, seed=n)
    t, s, info = run_and_check(dd, words, filt, n, d, 0)
    assert info["piece_joins"] == 0 and info["key_bits"] == 64
    try:
        dd.set_option("long_key_bits", 2)
        dd.set_option("bucket_walk", 8)
        cid, keep, s2 = dd.run_long(words, filt, n, distance=d)
        forced = dd.long_info()
        check_against_truth(dd, t, cid, keep, s2, 5)
    finally:
        dd.set_option("long_key_bits", 64)
        dd.set_option("bucket_walk", 1024)
    print(info, forced)
    assert forced["key_bits"] == 2 and forced["joins"] == 3
    assert forced["candidates"] > forced["raw_edges"] >= forced["edges"] == info["edges"]
    assert forced["piece_joins"] > 0
    assert forced["candidates"] > info["candidates"]


# ---- F. small and degenerate --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reads", [0, 1, 2, 5, 257])
def test_few_reads(dd, n_reads):
    rng = np.random.default_rng(n_reads)
    n = 150
    base = rng.integers(0, 4, size=(max(n_reads // 3, 1), n))
    syms = base[rng.integers(0, len(base), size=n_reads)].copy()
    for r in range(0, n_reads, 2):
        syms[r, rng.integers(0, n)] ^= 1                    # every second read: one substitution
    words = lt.pack_syms(syms).reshape(n_reads, 5)
    filt = (rng.random(n_reads) < 0.1).astype(np.uint8)
    for d in (0, 1):
        run_and_check(dd, words, filt, n, d, 0)


def test_all_filtered_and_all_equal(dd):
    words, _ = synth_long_words(300, 1, 100, 0.01, 0.0)
    cid, keep, s = dd.run_long(words, np.ones(300, np.uint8), 100)
    assert s["usable"] == 0 and s["unique"] == 0 and s["clusters"] == 0 and not cid.any() and not keep.any()
    assert dd.long_info()["joins"] == 0
    same = np.tile(words[:1], (300, 1))
    t, s, _ = run_and_check(dd, same, np.zeros(300, np.uint8), 100, 1, 0)
    assert s["unique"] == 1 and s["clusters"] == 1 and int(np.sum(t["keep"])) == 1


@pytest.mark.parametrize("n", [96, 512])
def test_all_t_words_without_a_spare_flag_bit(dd, n):
    """word_nt a multiple of 32: the first uint64 has no bit to carry the filtered flag, and a filtered read that holds
    the largest word there is must still come behind every usable one"""
    k = n // 32
    rng = np.random.default_rng(n)
    words = np.full((400, k), U64(2 ** 64 - 1))
    filt = (rng.random(400) < 0.3).astype(np.uint8)
    t, s, _ = run_and_check(dd, words, filt, n, 1, 0)
    assert s["unique"] == 1 and s["usable"] == 400 - int(filt.sum())
    # and with a smaller word and a neighbour of the all-T word among them
    words[5] = lt.substitute(words[5], n, n - 1, 1)
    words[6] = lt.substitute(words[6], n, 0, 1)
    words[7] = 0
    filt[5:8] = 0
    t, s, _ = run_and_check(dd, words, filt, n, 1, 1)
    assert s["unique"] == 4 and s["edges"] == 2


def test_distance_beyond_the_word_compares_all_pairs(dd):
    words, filt = synth_long_words(300, 65, 65, 0.01, 0.001)
    for d in (65, 70):
        t, s, info = run_and_check(dd, words, filt, 65, d, 0)
        u = s["unique"]
        assert info["joins"] == 1 and s["edges"] == u * (u - 1) // 2 and info["candidates"] == s["edges"]


# ---- G. refusals and state ----------------------------------------------------------------------------------------------------
def test_refusals(dd):
    words, filt = synth_long_words(100, 3, 150, 0.01, 0.001)
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.run_long(words, filt, 0)
    assert ei.value.code == -1
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.run_long(np.zeros((100, 17), U64), filt, 513)
    assert ei.value.code == -2
    for bad in (words[:, :4], words.reshape(-1), np.zeros((100, 5, 1), U64)):
        with pytest.raises(ValueError):
            dd.run_long(bad, filt, 150)
    with pytest.raises(ValueError):
        dd.run_long(np.zeros(100, U64), filt, 33)          # one-dimensional words: k = 1 only
    try:
        dd.set_option("edit_distance", 1)
        with pytest.raises(humid_amd.HumidError) as ei:
            dd.run_long(words, filt, 150)
        assert ei.value.code == -2
    finally:
        dd.set_option("edit_distance", 0)
    run_and_check(dd, words, filt, 150, 1, 0)               # the next run works
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.group_stats()
    assert ei.value.code == -6
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.group_stats_device()
    assert ei.value.code == -6
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.packed_words()
    assert ei.value.code == -6
    w2, f2 = synth_wide_words(100, 3, 64)
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.run(np.zeros((100, 2), U64), f2, word_nt=65)
    assert ei.value.code == -2
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.long_info()                                      # the last call was no long run
    assert ei.value.code == -6


def test_select_best_refuses_long_runs(dd):
    """humid_select_best* read one or two uint64 per read: after a long run they refuse (-6) instead of reading k-uint64
    rows at a 16-byte stride, through the device form, the host form and for a long run of 48 nt alike; word_nt > 64
    after a plain run is -2; the next runs work"""
    import ctypes as C
    import torch
    n_reads = 400
    words, filt = synth_long_words(n_reads, 5, 150, 0.01, 0.001)
    cid, keep, _ = dd.run_long(words, filt, 150)
    scores = np.arange(n_reads, dtype=np.uint32)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_cid = torch.from_numpy(cid.view(np.int32)).to(dev)
    d_keep, d_sc = torch.from_numpy(keep).to(dev), torch.from_numpy(scores.view(np.int32)).to(dev)
    d_out = torch.zeros(n_reads, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for scope in ("leaf", "cluster"):
        with pytest.raises(humid_amd.HumidError) as ei:
            dd.select_best_device(d_w.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), d_sc.data_ptr(), d_out.data_ptr(), 0,
                                  n_reads, word_nt=150, scope=scope)
        assert ei.value.code == -6
    keep_out, changed = np.zeros(n_reads, np.uint8), C.c_uint64()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    rc = dd._lib.humid_select_best(dd._h, vp(words), vp(cid), vp(keep), vp(scores), n_reads, 150, 0, vp(keep_out), None,
                                   C.byref(changed))
    assert rc == -6 and not keep_out.any()
    assert not d_out.cpu().numpy().any()                      # nothing was written
    run_and_check(dd, words, filt, 150, 1, 0)                 # the next long run works
    w48, f48 = synth_wide_words(n_reads, 6, 48, 0.01, 0.001)
    cid48, keep48, _ = dd.run_long(w48, f48, 48)
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.select_best(w48, cid48, keep48, scores, word_nt=48)
    assert ei.value.code == -6
    cid_p, keep_p, _ = dd.run(w48, f48, word_nt=48)
    assert np.array_equal(cid_p, cid48) and np.array_equal(keep_p, keep48)
    rc = dd._lib.humid_select_best(dd._h, vp(words), vp(cid_p), vp(keep_p), vp(scores), n_reads, 150, 0, vp(keep_out), None,
                                   C.byref(changed))
    assert rc == -2
    keep_out, rep, _ = dd.select_best(w48, cid_p, keep_p, scores, word_nt=48)      # and after a plain run it answers
    assert int(keep_out.sum()) == int(keep_p.sum())


def test_long_and_plain_runs_share_a_context():
    """run(24 nt), run_long(150), run(48), run_long(65) in ONE context: each equals a fresh context's results, and the
    plain runs retry what they retry in a context that ran the same plain runs with no long run in between"""
    w24, f24 = synth_words(20_000, 24, 24, p_sub=5e-3)
    w150, f150 = synth_long_words(5000, 150, 150, 2e-3, 1e-4)
    w48, f48 = synth_wide_words(20_000, 48, 48, p_sub=5e-3)
    w65, f65 = synth_long_words(5000, 65, 65, 5e-3, 1e-4)
    steps = [("run", w24, f24, 24), ("run_long", w150, f150, 150), ("run", w48, f48, 48), ("run_long", w65, f65, 65)]

    def results(d, how, w, f, n):
        cid, keep, s = (d.run(w, f, word_nt=n) if how == "run" else d.run_long(w, f, n))
        roads = d.run_roads() if how == "run" else None
        lv = d.leaves()
        off, idx = d.adjacency()
        return cid, keep, {k: s[k] for k in ("total", "usable", "unique", "clusters", "edges", "count_mode_used")}, lv, off, idx, roads

    shared, plain_only = humid_amd.Dedup(), humid_amd.Dedup()
    try:
        got_all = [results(shared, *st) for st in steps]
        plain_roads = [results(plain_only, *st)[6] for st in steps if st[0] == "run"]
    finally:
        shared.close()
        plain_only.close()
    assert [g[6] for g in got_all if g[6] is not None] == plain_roads
    for st, got in zip(steps, got_all):
        fresh = humid_amd.Dedup()
        try:
            want = results(fresh, *st)
        finally:
            fresh.close()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), st[0]
        assert got[2] == want[2] and got[2]["edges"] > 0
        for key in want[3]:
            assert np.array_equal(got[3][key], want[3][key]), key
        assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5])
