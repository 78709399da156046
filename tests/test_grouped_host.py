"""CPU checks of grouped deduplication (include/humid_hip.h, humid_dedup_run_grouped): the two truths of
tests/grouped_truth.py agree with each other, the plan of a grouped run keeps its promises (host arithmetic of the
library, no GPU), and the new entry points are exported."""
import ctypes as C

import numpy as np
import pytest

from humid_amd import _lib

import bruteforce as bf
import grouped_truth as gt

NEW_SYMBOLS = ("humid_dedup_run_grouped", "humid_dedup_run_grouped_device", "humid_get_leaf_groups",
               "humid_grouped_plan_info")


def grouped_words(rng, n_reads, word_nt, n_groups, n_base=40, p_sub=0.05, p_filt=0.03):
    """the same few base words in every group, with substitutions: exact repeats and near neighbours within and
    across groups; group ids 0 .. n_groups - 1 with a gap or two"""
    base = rng.integers(0, 4, size=(n_base, word_nt))
    pick = base[rng.integers(0, n_base, size=n_reads)]
    sub = rng.random(pick.shape) < p_sub
    pick = np.where(sub, rng.integers(0, 4, size=pick.shape), pick)
    vals = [int("".join(str(int(x)) for x in row), 4) for row in pick]
    if word_nt > 32:
        words = np.asarray([[v >> 64, v & ((1 << 64) - 1)] for v in vals], dtype=np.uint64)
    else:
        words = np.asarray(vals, dtype=np.uint64)
    groups = rng.integers(0, n_groups, size=n_reads).astype(np.uint32)
    filt = (rng.random(n_reads) < p_filt).astype(np.uint8)
    groups[filt == 1] = 0xFFFFFFFF                                 # ignored for filtered reads
    return words, groups, filt


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("distance", [0, 1, 2, 3])
def test_the_two_truths_agree(distance, method):
    rng = np.random.default_rng(100 + 10 * distance + method)
    for word_nt, n_groups in ((8, 3), (12, 16), (24, 5), (30, 17), (40, 6)):
        words, groups, filt = grouped_words(rng, 1500, word_nt, n_groups)
        a = gt.per_group(words, groups, filt, word_nt, distance, method)
        b = gt.repetition(words, groups, filt, word_nt, distance, method)
        gt.assert_same(a, b)
        assert a["summary"]["unique"] > n_groups and a["summary"]["edges"] > 0 or distance == 0


@pytest.mark.parametrize("method", [0, 1])
def test_per_group_truth_against_bruteforce(method):
    """small cases: the per-group truth's read outputs against tests/bruteforce.py group by group, Hamming and
    Levenshtein"""
    rng = np.random.default_rng(7 + method)
    for word_nt, distance, edit in ((8, 1, False), (10, 2, False), (10, 2, True), (12, 3, True)):
        words, groups, filt = grouped_words(rng, 300, word_nt, 4, n_base=12, p_sub=0.08)
        t = gt.per_group(words, groups, filt, word_nt, distance, method, edit=edit)
        base = 0
        for g in np.unique(groups[filt == 0]):
            sel = np.flatnonzero((groups == g) & (filt == 0))
            cid, keep, _ = bf.dedup(words[sel], np.zeros(len(sel), np.uint8), distance, maximum=bool(method),
                                    edit_nt=word_nt if edit else 0)
            cid = np.asarray(cid, np.uint64)
            assert np.array_equal(t["keep"][sel], np.asarray(keep, np.uint8))
            assert np.array_equal(t["cid"][sel].astype(np.uint64), np.where(cid > 0, cid + base, 0))
            base += int(cid.max())
        assert np.all(t["cid"][filt == 1] == 0) and np.all(t["keep"][filt == 1] == 0)


def group_nt(n_groups):
    return 0 if n_groups <= 1 else ((int(n_groups - 1).bit_length()) + 1) // 2


def test_grouped_plan_info_host_arithmetic():
    lib = _lib.load()
    nc, kb, gn = C.c_uint32(), C.c_uint32(), C.c_uint32()
    nc1, pb1 = C.c_uint32(), C.c_uint32()
    for n_groups in (1, 2, 3, 4, 5, 16, 17, 1000, 4096, 1 << 16, 100_000, 1 << 20, 1 << 31, 0xFFFFFFFF):
        gnt = group_nt(n_groups)
        for word_nt in (1, 2, 8, 12, 24, 28, 31, 32, 33, 40, 48, 56, 60, 63, 64):
            for d in (0, 1, 2, 3, 5, 8, 20, 40):
                for u in (10, 3_000_000, 1 << 40):
                    rc = lib.humid_grouped_plan_info(None, word_nt, n_groups, d, u, C.byref(nc), C.byref(kb),
                                                     C.byref(gn))
                    if word_nt + gnt > 64:
                        assert rc == -2, (word_nt, n_groups)
                        continue
                    assert rc == 0, (word_nt, n_groups, d, u)
                    assert gn.value == gnt
                    assert 1 <= nc.value <= 20 and 2 * gnt <= kb.value <= 64, (word_nt, n_groups, d, u, nc.value, kb.value)
                    if n_groups == 1:
                        assert lib.humid_stage_plan_info(None, word_nt, d, u, C.byref(nc1), C.byref(pb1)) == 0
                        assert nc.value == nc1.value, (word_nt, d, u)
    # the issue's examples: 24 nt with 2^16 groups (32 nt), 12-nt UMIs with 10^5 cells (21 nt), 48 nt + any u32 group
    for word_nt, n_groups, want in ((24, 1 << 16, 8), (12, 100_000, 9), (48, 0xFFFFFFFF, 16)):
        assert lib.humid_grouped_plan_info(None, word_nt, n_groups, 1, 1000, C.byref(nc), C.byref(kb), C.byref(gn)) == 0
        assert gn.value == want
    assert lib.humid_grouped_plan_info(None, 49, 0xFFFFFFFF, 1, 1000, C.byref(nc), C.byref(kb), C.byref(gn)) == -2
    assert lib.humid_grouped_plan_info(None, 64, 2, 1, 1000, C.byref(nc), C.byref(kb), C.byref(gn)) == -2
    assert lib.humid_grouped_plan_info(None, 24, 0, 1, 1000, C.byref(nc), C.byref(kb), C.byref(gn)) == -1


def test_grouped_symbols_are_exported():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name), name
