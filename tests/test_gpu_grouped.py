"""-m gpu: grouped deduplication (humid_dedup_run_grouped) against the truths of tests/grouped_truth.py, bit for bit:
per-read outputs, summary, leaves with their groups, adjacency, clusters and histograms."""
import numpy as np
import pytest

import humid_amd
from humid_amd.synth import synth_words

import grouped_truth as gt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[(0, 0, 1), (0, 1, 1), (1, 0, 1), (0, 1, 0)],
                ids=["lds_hashed_buckets", "lds_ordered_buckets", "global_table", "lds_ordered_library_radix"])
def dd(request):
    """the four count settings of test_gpu_parity.py's fixture (count_mode, count_order, tile_partition)"""
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
        w = np.zeros(len(rows), np.uint64)
        for t in range(n):
            w = (w << np.uint64(2)) | rows[:, t].astype(np.uint64)
        return w
    return np.stack([pack(rows[:, :n - 32]), pack(rows[:, n - 32:])], 1)


def grouped_input(seed, n_reads, word_nt, ids, n_base=60, p_sub=0.04, p_filt=0.03):
    """the same base words in every group (exact repeats and near neighbours across groups); group ids drawn from
    `ids`; a few filtered reads with out-of-range groups"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, size=(n_base, word_nt))
    rows = base[rng.integers(0, n_base, size=n_reads)]
    rows = np.where(rng.random(rows.shape) < p_sub, rng.integers(0, 4, size=rows.shape), rows)
    groups = np.asarray(ids, np.uint32)[rng.integers(0, len(ids), size=n_reads)]
    filt = (rng.random(n_reads) < p_filt).astype(np.uint8)
    groups[filt == 1] = 0xFFFFFFFF
    return pack(rows), groups, filt


def near_ids(n_groups, k=12):
    """k group ids below n_groups whose 2-bit codes differ in one nucleotide from their neighbours (and 0, the top)"""
    top = n_groups - 1
    ids = {0, top}
    b = top // 3
    for t in range(min(k, max(1, (n_groups.bit_length() + 1) // 2))):
        for v in (b, b ^ (1 << (2 * t)), b ^ (2 << (2 * t)), b ^ (3 << (2 * t))):
            if v < n_groups:
                ids.add(v)
    return sorted(ids)


def ids_for(n_groups):
    return list(range(n_groups)) if n_groups <= 16 else near_ids(n_groups)


def test_one_group_is_the_plain_pass(plain):
    """n_groups = 1 (group NULL or all zero) is bit-identical to Dedup.run in every output and accessor"""
    for word_nt in (24, 32, 48, 64):
        words, _, filt = grouped_input(word_nt, 20000, word_nt, [0])
        for d in (1, 2):
            cid, keep, s = plain.run(words, filt, word_nt=word_nt, distance=d)
            want = dict(cid=cid, keep=keep, summary=s, leaves=plain.leaves(), off=plain.adjacency()[0],
                        idx=plain.adjacency()[1], clusters=plain.clusters(), hist=plain.histograms())
            want["leaves"]["group"] = np.zeros(s["unique"], np.uint32)
            for groups in (None, np.zeros(len(filt), np.uint32)):
                got = gt.device_result(plain, words, groups, filt, word_nt, n_groups=1, distance=d)
                gt.assert_same(want, got, first_read=True)
                for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle"):
                    assert got["summary"][k] == s[k], k


# (word_nt, n_groups, distances): the issue's grid -- word lengths, group counts, one-nucleotide group codes, the
# promotion 28 nt + 1024 groups (33 nt internal) and the largest legal word_nt + group_nt = 64
CASES = [(8, 3, (0, 1, 2, 3)), (12, 16, (0, 1, 2)), (24, 2, (1, 3)), (28, 1024, (1, 2)), (32, 4096, (1,)),
         (40, 16, (1, 2)), (24, 1 << 16, (1, 2)), (12, 1 << 20, (1, 3)), (48, 0xFFFFFFFF, (1, 2)), (54, 1 << 20, (1,))]
_TRUTH = {}


def truth(word_nt, n_groups, d, method, per_group=False):
    key = (word_nt, n_groups, d, method, per_group)
    if key not in _TRUTH:
        words, groups, filt = grouped_input(word_nt * 7 + d, 6000, word_nt, ids_for(n_groups))
        f = gt.per_group if per_group else gt.repetition
        t = f(words, groups, filt, word_nt, d, method)
        _TRUTH[key] = (words, groups, filt, t)
    return _TRUTH[key]


@pytest.mark.parametrize("word_nt,n_groups,ds", CASES, ids=["%dnt_%dg" % (c[0], c[1]) for c in CASES])
def test_parity(dd, word_nt, n_groups, ds):
    for d in ds:
        for method in (0, 1):
            words, groups, filt, t = truth(word_nt, n_groups, d, method)
            got = gt.device_result(dd, words, groups, filt, word_nt, n_groups=n_groups, distance=d, method=method)
            gt.assert_same(t, got)
            assert t["summary"]["edges"] > 0 or d == 0


def test_parity_against_per_group_loop(plain):
    """the definition itself (one oracle pass per group), first_read included"""
    for word_nt, n_groups, d in ((12, 16, 1), (28, 1024, 2), (40, 3, 1)):
        words, groups, filt, t = truth(word_nt, n_groups, d, 0, per_group=True)
        got = gt.device_result(plain, words, groups, filt, word_nt, n_groups=n_groups, distance=d)
        gt.assert_same(t, got, first_read=True)


def test_tuning_options_keep_results():
    """forced plan segments, and a short bucket walk so that the tiles take over inside one large group"""
    words, groups, filt = grouped_input(5, 30000, 12, [0, 1, 2], n_base=400)
    groups = np.where(filt == 0, (np.arange(len(filt)) % 10 == 0).astype(np.uint32), groups).astype(np.uint32)
    big = (words, groups, filt, gt.repetition(words, groups, filt, 12, 2, 0))
    cases = [(24, 16, 1, truth(24, 16, 1, 0)), (40, 4096, 2, truth(40, 4096, 2, 0)), (12, 3, 2, big)]
    for opt, val in (("plan_segments", 3), ("plan_segments", 4), ("bucket_walk", 16), ("coop_big", 0),
                     ("padded_partition", 0)):
        d = humid_amd.Dedup()
        d.set_option(opt, val)
        for word_nt, n_groups, dist, (words, groups, filt, t) in cases:
            gt.assert_same(t, gt.device_result(d, words, groups, filt, word_nt, n_groups=n_groups, distance=dist))
        d.close()


@pytest.mark.parametrize("word_nt,n_groups", [(16, 5), (30, 40), (44, 9)])
def test_edit_distance(plain, word_nt, n_groups):
    """-e: Levenshtein between the words only, against the per-group loop"""
    for d in (2, 3, 6):
        words, groups, filt = grouped_input(word_nt + d, 1500 if d < 6 else 600, word_nt, list(range(n_groups)),
                                            n_base=25, p_sub=0.06)
        t = gt.per_group(words, groups, filt, word_nt, d, 0, edit=True)
        got = gt.device_result(plain, words, groups, filt, word_nt, n_groups=n_groups, distance=d, edit=True)
        gt.assert_same(t, got, first_read=True)


def test_scale(plain):
    """2 M reads in 10^5 groups (12-nt UMIs) against the oracle's repetition-code pass; 10 M reads in 4096 groups
    (24 nt, d = 1) against the repetition code on the plain device pass"""
    rng = np.random.default_rng(11)
    words, filt = synth_words(2_000_000, 1001, 12)
    groups = rng.integers(0, 100_000, size=len(filt)).astype(np.uint32)
    t = gt.repetition(words, groups, filt, 12, 1, 0)
    gt.assert_same(t, gt.device_result(plain, words, groups, filt, 12, n_groups=100_000, distance=1))
    words, filt = synth_words(10_000_000, 1001, 24)
    groups = rng.integers(0, 4096, size=len(filt)).astype(np.uint32)
    other = humid_amd.Dedup()
    t = gt.repetition(words, groups, filt, 24, 1, 0, engine=gt.device_engine(other))
    other.close()
    got = gt.device_result(plain, words, groups, filt, 24, n_groups=4096, distance=1)
    gt.assert_same(t, got, first_read=True)


def test_sparse_skewed_and_empty_groups(dd):
    rng = np.random.default_rng(3)
    words, _, filt = grouped_input(9, 40000, 24, [0], n_base=300)
    n = len(filt)
    groups = np.where(rng.random(n) < 0.9, 7, rng.choice([0, 3, 1000, 1001, 4095], size=n)).astype(np.uint32)
    filt[groups == 1001] = 1                                        # a group with every read filtered
    t = gt.per_group(words, groups, filt, 24, 1, 0)
    gt.assert_same(t, gt.device_result(dd, words, groups, filt, 24, n_groups=4096, distance=1), first_read=True)
    assert 1001 not in set(t["leaves"]["group"].tolist())


def test_errors_leave_the_context_usable(plain):
    words, groups, filt = grouped_input(1, 5000, 24, list(range(16)))
    t = gt.repetition(words, groups, filt, 24, 1, 0)
    bad = groups.copy()
    bad[np.flatnonzero(filt == 0)[1234]] = 16
    with pytest.raises(humid_amd.HumidError) as ei:
        plain.run_grouped(words, bad, filt, word_nt=24, n_groups=16)
    assert ei.value.code == -1
    gt.assert_same(t, gt.device_result(plain, words, groups, filt, 24, n_groups=16))
    huge = groups.copy()
    huge[filt == 1] = 0xFFFFFFFF                                    # filtered: never read
    gt.assert_same(t, gt.device_result(plain, words, huge, filt, 24, n_groups=16))
    with pytest.raises(humid_amd.HumidError) as ei:
        plain.run_grouped(np.zeros((len(filt), 2), np.uint64), groups, filt, word_nt=57, n_groups=1 << 16)
    assert ei.value.code == -2
    with pytest.raises(humid_amd.HumidError) as ei:
        plain.run_grouped(np.zeros((len(filt), 2), np.uint64), groups, filt, word_nt=49, n_groups=0xFFFFFFFF)
    assert ei.value.code == -2


def test_grouped_and_plain_runs_alternate(plain):
    """remembered per-shape decisions (ordered-bucket verdicts, pair-list room) do not leak between the two"""
    words, groups, filt = grouped_input(21, 200_000, 24, list(range(4096)), n_base=20000)
    t = gt.repetition(words, groups, filt, 24, 1, 0)
    cid, keep, s = plain.run(words, filt, word_nt=24, distance=1)
    for _ in range(2):
        gt.assert_same(t, gt.device_result(plain, words, groups, filt, 24, n_groups=4096))
        cid2, keep2, s2 = plain.run(words, filt, word_nt=24, distance=1)
        assert np.array_equal(cid, cid2) and np.array_equal(keep, keep2) and s2["edges"] == s["edges"]
        assert "group" not in plain.leaves()


def test_device_entry_point(plain):
    import torch
    words, groups, filt, t = truth(28, 1024, 1, 0)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_g = torch.from_numpy(groups.view(np.int32)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    d_cid = torch.zeros(len(filt), dtype=torch.int32, device=dev)
    d_keep = torch.zeros(len(filt), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s = plain.run_grouped_device(d_w.data_ptr(), d_g.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(),
                                 len(filt), 1024, word_nt=28, distance=1)
    assert np.array_equal(d_cid.cpu().numpy().view(np.uint32), t["cid"])
    assert np.array_equal(d_keep.cpu().numpy(), t["keep"])
    assert s["clusters"] == t["summary"]["clusters"]
    assert np.array_equal(plain.leaves()["group"], t["leaves"]["group"])
