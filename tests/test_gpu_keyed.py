"""-m gpu: keyed deduplication (humid_dedup_run_keyed: grouped runs whose groups are the ranks of arbitrary 64-bit keys,
ranked on the device) against the truths of tests/grouped_truth.py fed np.unique(keys[filtered == 0],
return_inverse=True), bit for bit: per-read outputs, summary, leaves with their groups and keys, adjacency, clusters,
histograms, and group_keys() against np.unique."""
import numpy as np
import pytest

import humid_amd
from humid_amd.synth import synth_words

import grouped_truth as gt

pytestmark = pytest.mark.gpu

U64 = np.uint64
TOP = (1 << 64) - 1


@pytest.fixture(scope="module", params=[(0, 0, 1), (0, 1, 1), (1, 0, 1), (0, 1, 0)],
                ids=["lds_hashed_buckets", "lds_ordered_buckets", "global_table", "lds_ordered_library_radix"])
def dd(request):
    """the four count settings of test_gpu_grouped.py's fixture (count_mode, count_order, tile_partition)"""
    d = humid_amd.Dedup()
    d.set_option("count_mode", request.param[0])
    d.set_option("count_order", request.param[1])
    d.set_option("tile_partition", request.param[2])
    yield d
    d.close()


@pytest.fixture(scope="module")
def plain():
    d = humid_amd.Dedup()
    yield d
    d.close()


def pack(rows):
    """rows of nucleotide codes -> u64[N] (<= 32 nt) or u64[N, 2]"""
    n = rows.shape[1]
    if n <= 32:
        w = np.zeros(len(rows), U64)
        for t in range(n):
            w = (w << U64(2)) | rows[:, t].astype(U64)
        return w
    return np.stack([pack(rows[:, :n - 32]), pack(rows[:, n - 32:])], 1)


def make_words(seed, n_reads, word_nt, n_base=60, p_sub=0.04, p_filt=0.03):
    """a few base words with substitutions (exact repeats and near neighbours under every key) and some filtered
    reads"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, size=(n_base, word_nt))
    rows = base[rng.integers(0, n_base, size=n_reads)] if n_reads else np.zeros((0, word_nt), np.int64)
    rows = np.where(rng.random(rows.shape) < p_sub, rng.integers(0, 4, size=rows.shape), rows)
    filt = (rng.random(n_reads) < p_filt).astype(np.uint8)
    return pack(rows), filt


def ranks_of(keys, filt):
    """the contract: K = np.unique over the usable reads' keys; group[r] = index of key[r] in K (filtered reads: a
    value no group has, never read)"""
    keys = np.asarray(keys, U64)
    K, inv = np.unique(keys[filt == 0], return_inverse=True)
    groups = np.full(len(filt), 0xFFFFFFFF, np.uint32)
    groups[filt == 0] = inv.astype(np.uint32)
    return K, groups


def keyed_result(d, words, keys, filt, word_nt, distance=1, method=0, edit=False):
    """Dedup.run_keyed + every accessor, in the truths' dict form (+ "K": group_keys())"""
    cid, keep, s = d.run_keyed(words, keys, filt, word_nt=word_nt, distance=distance, method=method, edit=edit)
    lv = d.leaves()
    off, idx = d.adjacency()
    return dict(cid=cid, keep=keep, summary=s, leaves=lv, off=off, idx=idx, clusters=d.clusters(), hist=d.histograms(),
                K=d.group_keys())


def check(d, words, keys, filt, word_nt, distance=1, method=0, edit=False, truth="per_group", engine=None):
    keys = np.asarray(keys, U64)
    K, groups = ranks_of(keys, filt)
    if truth == "per_group":
        t = gt.per_group(words, groups, filt, word_nt, distance, method, edit=edit)
    else:
        t = gt.repetition(words, groups, filt, word_nt, distance, method, engine=engine)
    got = keyed_result(d, words, keys, filt, word_nt, distance, method, edit)
    gt.assert_same(t, got, first_read="first_read" in t["leaves"])     # (the per-group truth and the device engine)
    assert got["K"].dtype == U64 and np.array_equal(got["K"], K)
    assert np.array_equal(got["leaves"]["key"], K[np.asarray(t["leaves"]["group"], np.int64)])
    assert d.keyed_rank_info()["n_keys"] == len(K)
    return t, got


def runs_of(lengths, keys):
    return np.concatenate([np.full(n, k, U64) for n, k in zip(lengths, keys)])


def key_shapes(n, rng):
    """(name, keys[n]) of the issue's key shapes"""
    special = np.asarray([0, 1, 1 << 63, TOP - 1, TOP], U64)
    yield "one_key", np.full(n, 0xDEADBEEF12345678, U64)
    yield "own_key_each", rng.permutation(n).astype(U64) * U64(0x9E3779B97F4A7C15)
    yield "special_values", special[rng.integers(0, 5, size=n)]
    yield "top_bits_only", rng.integers(0, 7, size=n).astype(U64) << U64(61)
    yield "bottom_bits_only", U64(0xABCDEF0000000000) | rng.integers(0, 3, size=n).astype(U64)
    yield "barcodes_32bit", rng.integers(0, 1 << 32, size=40).astype(U64)[rng.integers(0, 40, size=n)]


def test_key_shapes(dd):
    rng = np.random.default_rng(1)
    words, filt = make_words(2, 3000, 12)
    for name, keys in key_shapes(len(filt), rng):
        for d, method in ((1, 0), (2, 1)):
            check(dd, words, keys, filt, 12, d, method)


def test_sorted_runs_and_the_same_keys_shuffled(plain):
    """runs of equal keys of lengths 1, 63, 64, 65 and 10 000 (a wave collapses a run into one probe), aligned and not
    aligned to the waves, and the same keys shuffled"""
    rng = np.random.default_rng(3)
    lengths = [1, 63, 64, 65, 10000, 1, 1, 64, 64, 63, 65, 10000, 1]
    vals = rng.integers(0, 1 << 63, size=len(lengths)).astype(U64) * U64(2) + U64(1)
    vals[4] = TOP                                                   # a long run of the key ~0
    vals[7] = vals[1]                                               # a key that comes back later
    keys = runs_of(lengths, vals)
    words, filt = make_words(4, len(keys), 24, n_base=400)
    check(plain, words, keys, filt, 24, 1, 0)
    filt2 = filt.copy()
    filt2[::64] = 1                                                 # filtered reads at the head of every wave
    filt2[100:200] = 1
    check(plain, words, keys, filt2, 24, 1, 0)
    order = rng.permutation(len(keys))
    check(plain, words[order], keys[order], filt[order], 24, 1, 0)
    order = np.argsort(keys, kind="stable")
    check(plain, words[order], keys[order], filt[order], 24, 2, 1)


def unmix64(x):
    """inverse of the table's hash (common.hip.h, mix64)"""
    m = (1 << 64) - 1
    x = ((x ^ (x >> 31) ^ (x >> 62)) * 0x319642b2d24d8ec3) & m
    x = ((x ^ (x >> 27) ^ (x >> 54)) * 0x96de1b173f119089) & m
    return x ^ (x >> 30) ^ (x >> 60)


def test_keys_that_collide_in_the_table(plain):
    """keys whose hash starts with the same 40 bits: one home slot at every table size, a probe chain as long as the
    key set; and the same with a table of 16 slots to start with"""
    rng = np.random.default_rng(5)
    words, filt = make_words(6, 4000, 12)
    same_home = np.asarray([unmix64((0x5A5A5A5A5A << 24) | i) for i in range(150)], U64)
    keys = same_home[rng.integers(0, len(same_home), size=len(filt))]
    check(plain, words, keys, filt, 12, 1, 0)
    plain.set_option("keyrank_table_log2", 4)
    try:
        check(plain, words, keys, filt, 12, 1, 0)
        assert plain.keyed_rank_info()["n_redo"] >= 1
    finally:
        plain.set_option("keyrank_table_log2", 0)


def test_filtered_reads_spend_no_group(dd):
    rng = np.random.default_rng(7)
    words, filt = make_words(8, 5000, 24, p_filt=0.2)
    keys = rng.integers(0, 16, size=len(filt)).astype(U64) * U64(1000)
    keys[filt == 1] = rng.integers(1 << 40, 1 << 41, size=int(filt.sum())).astype(U64)   # keys no usable read has
    t, got = check(dd, words, keys, filt, 24, 1, 0)
    assert len(got["K"]) == 16 and int(got["K"].max()) == 15000
    # with those keys counted, 24 + group_nt would still fit; with 60 nt it would not: 5 usable keys, many filtered
    w60, f60 = make_words(9, 3000, 60, p_filt=0.5)
    k60 = rng.integers(0, 5, size=len(f60)).astype(U64)
    k60[f60 == 1] = np.arange(int(f60.sum()), dtype=U64) + U64(100)
    check(dd, w60, k60, f60, 60, 1, 0)


def test_all_filtered_and_tiny_inputs(plain):
    words, filt = make_words(10, 500, 24)
    keys = np.arange(500, dtype=U64)
    _, got = check(plain, words, keys, np.ones(500, np.uint8), 24)
    assert len(got["K"]) == 0 and got["summary"]["unique"] == 0
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 257):
        words, filt = make_words(12 + n, n, 24, n_base=3, p_filt=0.0)
        for keys in (np.zeros(n, U64), np.full(n, TOP, U64), rng.integers(0, 3, size=n).astype(U64) << U64(62)):
            _, got = check(plain, words, keys, filt, 24)
            assert len(got["K"]) == len(np.unique(keys))


@pytest.mark.parametrize("word_nt", [8, 12, 24, 32, 40, 48])
def test_word_lengths_distances_methods(dd, word_nt):
    rng = np.random.default_rng(word_nt)
    words, filt = make_words(100 + word_nt, 4000, word_nt)
    keys = rng.integers(0, 1 << 64, size=300, dtype=U64)[rng.integers(0, 300, size=len(filt))]
    for d in (0, 1, 2, 3):
        for method in (0, 1):
            check(dd, words, keys, filt, word_nt, d, method, truth="repetition" if word_nt <= 24 else "per_group")


@pytest.mark.parametrize("word_nt,n_keys", [(54, 1000), (64, 1)])
def test_long_words_with_few_keys(dd, word_nt, n_keys):
    rng = np.random.default_rng(word_nt)
    words, filt = make_words(200 + word_nt, 3000, word_nt)
    keys = rng.integers(0, 1 << 64, size=n_keys, dtype=U64)[rng.integers(0, n_keys, size=len(filt))]
    for d in (1, 2):
        check(dd, words, keys, filt, word_nt, d, 0)


@pytest.mark.parametrize("word_nt", [16, 30, 44])
def test_edit_distance(plain, word_nt):
    rng = np.random.default_rng(word_nt)
    words, filt = make_words(300 + word_nt, 1500, word_nt, n_base=25, p_sub=0.06)
    keys = rng.integers(0, 1 << 64, size=9, dtype=U64)[rng.integers(0, 9, size=len(filt))]
    check(plain, words, keys, filt, word_nt, 2, 0, edit=True)


def test_refusal_leaves_the_context_usable(plain):
    """word_nt = 60 with more than 4^4 distinct keys does not fit 64 nucleotides: HUMID_E_UNSUPPORTED (-2), and the
    same context then runs a legal case"""
    rng = np.random.default_rng(13)
    words, filt = make_words(14, 2000, 60, p_filt=0.0)
    keys = (np.arange(2000) % 257).astype(U64) << U64(50)
    with pytest.raises(humid_amd.HumidError) as ei:
        plain.run_keyed(words, keys, filt, word_nt=60)
    assert ei.value.code == -2
    with pytest.raises(humid_amd.HumidError) as ei:
        plain.group_keys()
    assert ei.value.code == -6                                   # HUMID_E_STATE
    check(plain, words, (np.arange(2000) % 256).astype(U64) << U64(50), filt, 60)      # 4^4 keys: 60 + 4 = 64
    w24, f24 = make_words(15, 3000, 24)
    check(plain, w24, rng.integers(0, 50, size=3000).astype(U64), f24, 24)


def test_equal_to_the_grouped_path(plain):
    """run_keyed(words, keys) == run_grouped(words, inverse, n_groups = G), bit for bit, first_read included"""
    rng = np.random.default_rng(17)
    other = humid_amd.Dedup()
    for word_nt, n_keys, d in ((24, 5000, 1), (28, 1024, 2), (40, 70000, 1), (12, 1, 1)):
        words, filt = make_words(word_nt, 100_000, word_nt, n_base=3000)
        keys = rng.integers(0, 1 << 64, size=n_keys, dtype=U64)[rng.integers(0, n_keys, size=len(filt))]
        K, groups = ranks_of(keys, filt)
        want = gt.device_result(other, words, groups, filt, word_nt, n_groups=len(K), distance=d)
        got = keyed_result(plain, words, keys, filt, word_nt, d)
        gt.assert_same(want, got, first_read=True)
        assert np.array_equal(got["K"], K)
    other.close()


def test_table_too_small_is_redone(plain):
    """the ranking starts with a table of 16 slots for 3000 keys: the device reports it full and the ranking is
    repeated with larger tables -- asserted, not assumed -- with the same results; the size is then remembered"""
    rng = np.random.default_rng(19)
    words, filt = make_words(20, 20000, 24, n_base=500)
    keys = rng.integers(0, 1 << 64, size=3000, dtype=U64)[rng.integers(0, 3000, size=len(filt))]
    plain.set_option("keyrank_table_log2", 4)
    try:
        t, got = check(plain, words, keys, filt, 24, truth="repetition")
        info = plain.keyed_rank_info()
        assert info["n_redo"] >= 2 and (1 << info["table_log2"]) >= len(got["K"])
    finally:
        plain.set_option("keyrank_table_log2", 0)
    got2 = keyed_result(plain, words, keys, filt, 24)
    gt.assert_same(t, got2)
    assert plain.keyed_rank_info()["n_redo"] == 0                   # remembered from the pass before


def test_no_state_leaks_into_plain_and_grouped_runs(plain):
    rng = np.random.default_rng(23)
    words, filt = make_words(24, 50000, 24, n_base=4000)
    keys = rng.integers(0, 1 << 64, size=700, dtype=U64)[rng.integers(0, 700, size=len(filt))]
    K, groups = ranks_of(keys, filt)
    cid, keep, s = plain.run(words, filt, word_nt=24, distance=1)
    grouped = gt.device_result(plain, words, groups, filt, 24, n_groups=len(K))
    for _ in range(2):
        check(plain, words, keys, filt, 24, truth="repetition")
        cid2, keep2, s2 = plain.run(words, filt, word_nt=24, distance=1)
        assert np.array_equal(cid, cid2) and np.array_equal(keep, keep2) and s2["edges"] == s["edges"]
        lv = plain.leaves()
        assert "group" not in lv and "key" not in lv
        with pytest.raises(humid_amd.HumidError) as ei:
            plain.group_keys()
        assert ei.value.code == -6                                   # HUMID_E_STATE
        again = gt.device_result(plain, words, groups, filt, 24, n_groups=len(K))
        gt.assert_same(grouped, again, first_read=True)
        assert "key" not in again["leaves"]
        with pytest.raises(humid_amd.HumidError):
            plain.group_keys()


def test_device_entry_point(plain):
    import torch
    rng = np.random.default_rng(29)
    words, filt = make_words(30, 30000, 28, n_base=2000)
    keys = rng.integers(0, 1 << 64, size=1024, dtype=U64)[rng.integers(0, 1024, size=len(filt))]
    K, groups = ranks_of(keys, filt)
    t = gt.repetition(words, groups, filt, 28, 1, 0)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_k = torch.from_numpy(keys.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_cid = torch.zeros(len(filt), dtype=torch.int32, device=dev)
    d_keep = torch.zeros(len(filt), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s = plain.run_keyed_device(d_w.data_ptr(), d_k.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(),
                               len(filt), word_nt=28, distance=1)
    assert np.array_equal(d_cid.cpu().numpy().view(np.uint32), t["cid"])
    assert np.array_equal(d_keep.cpu().numpy(), t["keep"])
    assert s["clusters"] == t["summary"]["clusters"]
    lv = plain.leaves()
    assert np.array_equal(lv["group"], t["leaves"]["group"]) and np.array_equal(plain.group_keys(), K)
    assert np.array_equal(lv["key"], K[lv["group"]])


@pytest.mark.parametrize("n_keys,bits", [(100_000, 32), (2_500_000, 64)])
def test_scale(plain, n_keys, bits):
    """the 10 M metric words x 10^5 32-bit keys and x 2.5 M 64-bit keys, against the repetition code on the plain
    device pass"""
    rng = np.random.default_rng(31)
    words, filt = synth_words(10_000_000, 1001, 24)
    pool = rng.integers(0, 1 << bits, size=n_keys, dtype=U64)
    keys = pool[rng.integers(0, n_keys, size=len(filt))]
    other = humid_amd.Dedup()
    try:
        check(plain, words, keys, filt, 24, 1, 0, truth="repetition", engine=gt.device_engine(other))
    finally:
        other.close()
