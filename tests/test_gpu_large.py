"""-m gpu: the single-GPU pass from 16 M to 67 M reads against an exact CPU truth (tests/large_truth.py).

Above 16,777,216 reads the pass switches to code that no smaller read set launches, chosen from N alone
(humid_amd/csrc/pipeline.hip.h: unpermute_tiled, stage_count_rec, part_bits):

  reads N                  un-permute: window, bins, kernels                               count stage, 24-nt words
  <= 16,777,216            2^14, <= 1024, k_unperm_bins8<1024> + k_unperm_window<., 14>    records
  16,777,217-25,165,824    2^14, 1025-1536, k_unperm_bins8<1536, 7>                        records, 25 index bits
  25,165,825-33,554,432    2^14, 1537-2048, k_unperm_bins8<2048>                           records
  33,554,433-50,331,648    2^15, 1025-1536, <1536, 7> + k_unperm_window<., 15>             records, 10-bit first level
  45,875,201 and up        (as the rows around it)                                         2^18 buckets
  50,331,649-67,108,864    2^15, 1537-2048, <2048>                                         records, 10-bit first level
  67,108,865               the bin table is full: the one-kernel un-permute                stage_count_lds

Every size runs over the device copy of ONE read set of 67,108,865 reads with n_reads = N -- a kernel that reads
past N pulls in real reads, and the counts catch it -- into outputs N + 1 long with sentinels at [N]."""
import numpy as np
import pytest
import torch

import humid_amd
import large_truth as lt
from humid_amd.synth import synth_wide_words, synth_words

pytestmark = pytest.mark.gpu

N_MAX = 67_108_865
N_X = 33_554_433
# every size, growing and shrinking across the window (2^14 / 2^15 reads) and bin-count changes, so that the remembered
# per-shape decisions carry over from run to run.  The bins' cursors live behind the records, at rec + (bins << wshift),
# and a pass skips clearing them only when the last tiled pass left them clean at that same address (unpermute_tiled,
# ucur_clean): so N_X (1025 x 2^15) and 67,108,864 (2048 x 2^15) run twice back to back, and 33,554,432
# (2048 x 2^14) runs again after the one-kernel un-permute of 67,108,865, which must leave the cursors alone
ORDER = [16_777_216, 33_554_433, 33_554_433, 16_777_217, 25_165_825, 50_331_649, 25_165_824, 45_875_201, 33_554_432,
         67_108_865, 33_554_432, 50_331_648, 67_108_864, 67_108_864]
FULL = {16_777_217, 33_554_433, 67_108_865}          # the unique level in full, too
SENT_C, SENT_K = -7, 9


class Truth:
    """exact results of the prefixes of one read set at d = 1: the pairs of the whole set once, each prefix's cut
    from them"""

    def __init__(self, words, filt, word_nt):
        self.pt = lt.PrefixTruth(words, filt)
        self.word_nt = word_nt
        self.pairs = None
        self.kept = {}
        self.last = None

    def get(self, n, maximum=False, keep=False):
        """keep: held for later calls; the last result is held until the next call in any case"""
        if (n, maximum) in self.kept:
            return self.kept[(n, maximum)]
        if self.last is not None and self.last[0] == (n, maximum):
            return self.last[1]
        self.last = None
        if self.pairs is None:
            whole = self.pt.prefix(len(self.pt.words))
            self.pairs = lt.pairs_d1(whole["word"], self.word_nt) + (whole["first_read"],)
            del whole
        t = self.pt.prefix(n)
        off, idx = lt.csr(*lt.sub_pairs(*self.pairs, n), t["unique"])
        x = lt.unique_level(t, off, idx, maximum)
        x["t"] = t
        x["cid"], x["keep"] = lt.per_read(t, x["cluster_id"], x["is_max_leaf"])
        if keep:
            self.kept[(n, maximum)] = x
        else:
            self.last = ((n, maximum), x)
        return x


def run(dd, d_w, d_f, n, word_nt=24, distance=1, method=0):
    """one pass over the first n reads into outputs n + 1 long: the sentinels at [n] must survive"""
    d_c = torch.full((n + 1,), SENT_C, dtype=torch.int32, device=d_w.device)
    d_k = torch.full((n + 1,), SENT_K, dtype=torch.uint8, device=d_w.device)
    s = dd.run_device(d_w.data_ptr(), d_f.data_ptr(), d_c.data_ptr(), d_k.data_ptr(), n, word_nt, distance, method)
    torch.cuda.synchronize()
    c, k = d_c.cpu().numpy(), d_k.cpu().numpy()
    assert c[n] == SENT_C and k[n] == SENT_K, "N = %d: a kernel wrote behind the outputs" % n
    return s, c[:n].view(np.uint32), k[:n]


def check(dd, s, cid, keep, x, full=False):
    """the summary counts, the leaves' words / counts / first reads and the per-read results exactly; full: the
    adjacency, degrees, leaf cluster ids, max-leaf flags, clusters and histograms too"""
    n = x["t"]["n"]
    for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle"):
        assert s[k] == x["summary"][k], (n, k, s[k], x["summary"][k])
    lv = dd.leaves()
    for k in ("word", "count", "first_read"):
        assert np.array_equal(lv[k], x["t"][k]), (n, k)
    assert np.array_equal(cid, x["cid"]), (n, "cluster_id", int(np.count_nonzero(cid != x["cid"])))
    assert np.array_equal(keep, x["keep"]), (n, "keep", int(np.count_nonzero(keep != x["keep"])))
    if full:
        for k in ("degree", "cluster_id", "is_max_leaf"):
            assert np.array_equal(lv[k], x[k]), (n, k)
        off, idx = dd.adjacency()
        assert np.array_equal(off.astype(np.uint64), x["off"]) and np.array_equal(idx, x["idx"]), (n, "adjacency")
        cl = dd.clusters()
        for k in ("size", "max_count", "max_leaf"):
            assert np.array_equal(cl[k].astype(np.uint64), x["clusters"][k].astype(np.uint64)), (n, k)
        assert dd.histograms() == x["hist"], (n, "histograms")


@pytest.fixture
def dd():
    """a fresh context, closed (its device buffers freed) even when the test fails"""
    d = humid_amd.Dedup(device=0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def big():
    words, filt = synth_words(N_MAX, 1077, 24)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    yield dict(d_w=d_w, d_f=d_f, truth=Truth(words, filt, 24))


def test_genome_prefixes_d2(dd):
    """BASELINE config 5: 50,331,649 reads of genome prefixes at d = 2 on the record path.  Summary, leaves and reads
    exactly; the device's lists sound everywhere and complete on 20,000 sampled leaves, then clustered by the oracle"""
    n = 50_331_649
    words, filt = synth_words(n, 1005, 24, mode="genome")
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    s, cid, keep = run(dd, d_w, d_f, n, distance=2)
    del d_w, d_f
    assert s["records8"] and s["count_mode_used"] == 2, (s["records8"], s["count_mode_used"])
    t = lt.PrefixTruth(words, filt).prefix(n)
    del words, filt
    lv = dd.leaves()
    assert s["unique"] == t["unique"]
    for k in ("word", "count"):
        assert np.array_equal(lv[k], t[k]), k
    off, idx = dd.adjacency()
    # most leaves of genome prefixes have no neighbour at all (mean degree ~0.2): besides the uniform sample, 40,000
    # leaves drawn from those with a neighbour at distance 1 in the complete d = 1 pair set, whose rows cannot be empty
    near = np.unique(np.concatenate(lt.pairs_d1(t["word"], 24)))
    also = np.random.default_rng(6).choice(near, size=min(40_000, len(near)), replace=False)
    sample = lt.check_pairs_d2(t["word"], 24, off, idx, n_sample=20_000, seed=5, also=also)
    assert len(sample) >= 50_000 and len(lt.rows_of(off, idx, sample)) >= len(also), len(sample)
    x = lt.unique_level(t, off.astype(np.uint64), idx)
    x["t"] = t
    x["cid"], x["keep"] = lt.per_read(t, x["cluster_id"], x["is_max_leaf"])
    check(dd, s, cid, keep, x, full=True)


def test_two_word_words_36nt(dd):
    """config 3's full 12-nt UMI: 33,554,433 reads of 36-nt words (two uint64) at d = 1 on the wide record path,
    everything against the truth, the complete pairs included"""
    n = 33_554_433
    words, filt = synth_wide_words(n, 1003, 36)
    dev = torch.device("cuda:0")
    d_w = torch.from_numpy(words.view(np.int64)).to(dev)
    d_f = torch.from_numpy(filt).to(dev)
    s, cid, keep = run(dd, d_w, d_f, n, word_nt=36)
    del d_w, d_f
    assert s["records8"] and s["count_mode_used"] == 2, (s["records8"], s["count_mode_used"])
    check(dd, s, cid, keep, Truth(words, filt, 36).get(n), full=True)


def test_sizes_on_one_context(dd, big):
    """every size of the table on one context (kernel_timing on): the path taken, then every result exactly"""
    dd.set_option("kernel_timing", 1)
    for n in ORDER:
        s, cid, keep = run(dd, big["d_w"], big["d_f"], n)
        tiled = n <= 1 << 26           # beyond: more than 2048 windows of 2^15 reads, the bin table is full
        assert s["records8"] == tiled, (n, s["records8"], s["count_mode_used"])
        assert not tiled or s["count_mode_used"] == 2, (n, s["count_mode_used"])
        assert (s["ms_k_unperm"] > 0) == tiled, (n, s["ms_k_unperm"])
        check(dd, s, cid, keep, big["truth"].get(n), full=n in FULL)


def test_maximum(dd, big):
    """-x at 33,554,433 reads, every array"""
    s, cid, keep = run(dd, big["d_w"], big["d_f"], N_X, method=1)
    assert s["records8"]
    check(dd, s, cid, keep, big["truth"].get(N_X, maximum=True), full=True)


# option -> (count_mode_used, tiled un-permute) of the path it selects at N_X
OTHER_PATHS = {("records8", 0): (2, True),          # 12-byte (key, read) pairs, k_unperm_bins + k_unperm_window
               ("count_mode", 1): (1, False),       # the global table, k_read_map
               ("count_order", 0): (0, True),       # hashed LDS buckets
               ("tile_partition", 0): (2, False)}   # the library's radix passes, the one-kernel un-permute


@pytest.mark.parametrize("option,value", sorted(OTHER_PATHS))
def test_other_paths(dd, big, option, value):
    """at 33,554,433 reads, a fresh context with one other path against the same truth; the path it took is asserted
    (count_mode_used, and with kernel_timing whether the tiled un-permute ran)"""
    dd.set_option(option, value)
    dd.set_option("kernel_timing", 1)
    s, cid, keep = run(dd, big["d_w"], big["d_f"], N_X)
    mode, tiled = OTHER_PATHS[(option, value)]
    assert not s["records8"] and s["count_mode_used"] == mode, (s["records8"], s["count_mode_used"])
    assert (s["ms_k_unperm"] > 0) == tiled, s["ms_k_unperm"]
    check(dd, s, cid, keep, big["truth"].get(N_X, keep=True))
