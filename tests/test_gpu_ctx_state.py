"""-m gpu: what a context holds after a call is ONE record (pipeline.hip.h, CtxState).  A humid_stage_graph after a
grouped, keyed or corrected run leaves a stage graph and nothing of that run: the leaf accessors answer for the
stage graph's words, every accessor of the run returns HUMID_E_STATE; and a refused run leaves nothing at all.
The stage entry points are called through the library handle with torch tensors as device buffers."""
import ctypes as C

import numpy as np
import pytest

import humid_amd
from humid_amd import _lib

from test_gpu_keyed import make_words

pytestmark = pytest.mark.gpu

U64 = np.uint64
OK, E_INVALID, E_UNSUPPORTED, E_STATE = 0, -1, -2, -6
N = 2000
WHITELIST = (np.arange(1, 8, dtype=U64) * U64(0x9E3779B1)) & U64(0xFFFFFFFF)      # 7 barcodes of 16 nt
W12, F12 = make_words(42, N, 12)
KEYS7 = WHITELIST[np.random.default_rng(43).integers(0, 7, size=N)]
ACCESSORS = ("first_read", "leaf_groups", "group_stats", "group_keys", "keyed_rank_info", "barcode_status")


def vp(a):
    return C.c_void_p(a.ctypes.data)


@pytest.fixture(scope="module")
def dd():
    d = humid_amd.Dedup()
    d.set_whitelist(WHITELIST, 16)
    yield d
    d.close()


@pytest.fixture(scope="module")
def ref():
    """a plain 24-nt, distance-1 run on a context of its own: its leaves are the stage graph's input and its truth"""
    d = humid_amd.Dedup()
    words, filt = make_words(41, N, 24)
    cid, keep, s = d.run(words, filt, word_nt=24, distance=1)
    lv = d.leaves()
    d.close()
    assert s["unique"] > 100 and s["edges"] > 0 and s["clusters"] < s["unique"]
    return dict(words=words, filt=filt, cid=cid, keep=keep, summary=s, leaves=lv)


def run_grouped(d):
    groups = np.random.default_rng(44).integers(0, 5, size=N).astype(np.uint32)
    return d.run_grouped(W12, groups, F12, word_nt=12, n_groups=5)


def run_keyed(d):
    return d.run_keyed(W12, KEYS7 << U64(20), F12, word_nt=12)


def run_corrected(d):
    out = d.run_keyed(W12, KEYS7, F12, word_nt=12, correct=True)
    status, counts = d.barcode_status()
    assert counts[1] == np.count_nonzero(F12 == 0)                 # every usable read's barcode is exact
    return out


def run_accessors(d, n_leaves):
    """return codes of the accessors that belong to a run (ACCESSORS[:3]) and to its kind, by name"""
    lib, h = d._lib, d._h
    n64, t32, r32 = C.c_uint64(), C.c_uint32(), C.c_uint32()
    first = np.zeros(max(n_leaves, 1), np.uint32)
    grp = np.zeros(max(n_leaves, 1), np.uint32)
    status, counts = np.zeros(N, np.uint8), np.zeros(5, U64)
    return dict(
        first_read=lib.humid_get_leaves(h, None, None, vp(first), None, None, None),
        leaf_groups=lib.humid_get_leaf_groups(h, vp(grp)),
        group_keys=lib.humid_get_group_keys(h, None, 0, C.byref(n64)),
        keyed_rank_info=lib.humid_keyed_rank_info(h, C.byref(n64), C.byref(t32), C.byref(r32)),
        barcode_status=lib.humid_get_barcode_status(h, vp(status), N, vp(counts)),
        group_stats=lib.humid_get_group_stats(h, 0, C.byref(n64), None, None, None, None))


def select_best_refused(d, cid, keep):
    """humid_select_best with the arguments of the 12-nt run: refused as "no completed run" """
    scores, keep_out = np.zeros(N, np.uint32), np.zeros(N, np.uint8)
    rc = d._lib.humid_select_best(d._h, vp(W12), vp(cid), vp(keep), vp(scores), N, 12, 0, vp(keep_out), None, None)
    return rc == E_INVALID and b"needs a completed single-GPU humid_dedup_run" in d._lib.humid_last_error(d._h)


def same_as_ref(d, ref):
    cid, keep, s = d.run(ref["words"], ref["filt"], word_nt=24, distance=1)
    assert np.array_equal(cid, ref["cid"]) and np.array_equal(keep, ref["keep"])
    assert all(s[k] == ref["summary"][k] for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle"))
    lv = d.leaves()
    assert lv.keys() == ref["leaves"].keys() and all(np.array_equal(lv[k], ref["leaves"][k]) for k in lv)


@pytest.mark.parametrize("before,n_answer", [(run_grouped, 3), (run_keyed, 5), (run_corrected, 6)],
                         ids=["grouped", "keyed", "corrected"])
def test_stage_graph_after_a_run_of_another_word_length(dd, ref, before, n_answer):
    import torch
    cid12, keep12, s12 = before(dd)
    # the run's accessors answer from its kind on (PLAIN < GROUPED < KEYED < CORRECTED), and only those
    assert run_accessors(dd, s12["unique"]) == {k: OK if i < n_answer else E_STATE for i, k in enumerate(ACCESSORS)}
    lv = ref["leaves"]
    u = len(lv["count"])
    dev = torch.device("cuda:0")
    d_word = torch.from_numpy(lv["word"].view(np.int64)).to(dev)
    d_cnt = torch.from_numpy(lv["count"].view(np.int32)).to(dev)
    torch.cuda.synchronize()
    pc, pm, s = C.c_void_p(), C.c_void_p(), _lib.HumidSummary()
    dd._check(dd._lib.humid_stage_graph(dd._h, C.c_void_p(d_word.data_ptr()), C.c_void_p(d_cnt.data_ptr()), u, 24, 1, 0,
                                        C.byref(pc), C.byref(pm), C.byref(s)))
    assert s.clusters == ref["summary"]["clusters"] and s.edges == ref["summary"]["edges"]
    # the leaf accessors answer for the stage graph: its words bit for bit (no mask of the 12-nt run), counts, ids
    word, count, cid = np.zeros(u, U64), np.zeros(u, np.uint32), np.zeros(u, np.uint32)
    dd._check(dd._lib.humid_get_leaves(dd._h, vp(word), vp(count), None, None, vp(cid), None))
    assert np.array_equal(word, lv["word"]) and np.array_equal(count, lv["count"]) and np.array_equal(cid, lv["cluster_id"])
    # nothing of the run is left
    assert run_accessors(dd, u) == dict.fromkeys(ACCESSORS, E_STATE)
    assert select_best_refused(dd, cid12, keep12)
    del d_word, d_cnt
    same_as_ref(dd, ref)


def test_a_refused_run_leaves_nothing_behind(dd, ref):
    """a pin of the rule, not of a defect: the keyed entry point cleared enough before the record existed too"""
    cid12, keep12, s12 = run_corrected(dd)
    words, filt = make_words(14, N, 60, p_filt=0.0)
    keys = (np.arange(N) % 257).astype(U64) << U64(50)             # 257 keys: 60 + 5 group nucleotides > 64
    with pytest.raises(humid_amd.HumidError) as ei:
        dd.run_keyed(words, keys, filt, word_nt=60)
    assert ei.value.code == E_UNSUPPORTED
    assert run_accessors(dd, s12["unique"]) == dict.fromkeys(ACCESSORS, E_STATE)
    word = np.zeros(s12["unique"], U64)
    assert dd._lib.humid_get_leaves(dd._h, vp(word), None, None, None, None, None) == E_STATE
    assert select_best_refused(dd, cid12, keep12)
    same_as_ref(dd, ref)
