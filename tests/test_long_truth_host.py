"""tests/long_truth.py, the numpy truth of the long-word GPU tests, pinned to the C oracle where both apply (up to 64
nucleotides), and to itself under constant fillers that make the same words longer.  CPU only."""
import numpy as np
import pytest

import long_truth as lt
from humid_amd.synth import synth_wide_words
from oracle import pyoracle as orc

CASES = [(48, 1, 0), (64, 2, 1), (40, 1, 0), (64, 1, 0)]       # (n, d, method)


@pytest.fixture(scope="module")
def inputs():
    return {n: synth_wide_words(3000, 7000 + n, n, 0.01, 0.01) for n in sorted({c[0] for c in CASES})}


def oracle_full(words, filt, n, d, maximum):
    p = orc.Pipeline(n)
    p.read_data(words, filt)
    p.find_hamming_neighbours(d)
    p.find_clusters(maximum)
    cid, keep = p.map_reads()
    return p, cid, keep


@pytest.mark.parametrize("n,d,method", CASES)
def test_truth_equals_the_oracle_on_every_read(inputs, n, d, method):
    words, filt = inputs[n]
    t = lt.long_dedup(words, filt, d, method)
    p, ocid, okeep = oracle_full(words, filt, n, d, bool(method))
    os_ = p.summary()
    print("U", os_["unique"], "E", os_["edges"])
    assert os_["unique"] > 1000 and os_["edges"] > 300
    assert t["summary"] == os_
    assert np.array_equal(t["cid"], ocid) and np.array_equal(t["keep"], okeep)
    lv, olv = t["leaves"], p.leaves()
    for key in ("word", "count", "degree", "cluster_id", "is_max_leaf"):
        assert np.array_equal(lv[key], olv[key]), key
    ooff, oidx = p.adjacency()
    assert np.array_equal(t["off"], ooff) and np.array_equal(t["idx"], oidx)
    ocl = p.clusters()
    for key in ("size", "max_count", "max_leaf"):
        assert np.array_equal(t["clusters"][key], ocl[key]), key
    assert t["hist"] == orc.histograms(p)


@pytest.mark.parametrize("fill_nt", [1, 33, 86, 448])
@pytest.mark.parametrize("n,d,method", CASES[:2])
def test_a_constant_filler_changes_nothing(inputs, n, d, method, fill_nt):
    words, filt = inputs[n]
    t = lt.long_dedup(words, filt, d, method)
    longer = lt.with_filler(words, n, fill_nt, seed=fill_nt)
    assert longer.shape == (len(words), (n + fill_nt + 31) // 32)
    f = lt.long_dedup(longer, filt, d, method, word_nt=n + fill_nt)
    assert np.array_equal(f["cid"], t["cid"]) and np.array_equal(f["keep"], t["keep"])
    assert f["summary"] == t["summary"] and f["summary"]["edges"] > 0
    assert np.array_equal(f["off"], t["off"]) and np.array_equal(f["idx"], t["idx"])
    for key in ("count", "degree", "cluster_id", "is_max_leaf"):
        assert np.array_equal(f["leaves"][key], t["leaves"][key]), key


def test_substitute_and_head_mask():
    assert lt.head_mask(65) == (3, np.uint64(3)) and lt.head_mask(64) == (2, np.uint64(2 ** 64 - 1))
    w = np.zeros(3, np.uint64)
    assert lt.substitute(w, 65, 0).tolist() == [1, 0, 0]
    assert lt.substitute(w, 65, 1, 2).tolist() == [0, 2 << 62, 0]
    assert lt.substitute(w, 65, 64, 3).tolist() == [0, 0, 3]
