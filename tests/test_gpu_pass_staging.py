"""-m gpu: the staging pool that the host-buffer forms of the post-run passes share (STAGE_IN / STAGE_OUT,
pipeline.hip.h).  The pass suites use one pattern per pass; here DIFFERENT passes go through ONE context with sizes
that go up and down and element widths that change from call to call, which is what a shared pool can get wrong:
every result equal, array for array, to the truths the suite already has (whitelist_truth, best_truth through
test_gpu_best.truth, consensus_truth, optical_truth, paired_truth).  Then: what is no staging -- the packed words of a
run, its leaves, the results of a consensus call -- survives later passes of larger inputs; the paired host run, which
goes through the host road of every other run, answers as its device form; a refused host form moves nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import humid_amd
from oracle import pyoracle as orc

import best_truth as bt
import consensus_truth as ct
import optical_truth as ot
import paired_truth as pt
import whitelist_truth as wt
from test_gpu_best import truth as best_truth
from test_gpu_consensus import truth as consensus_truth
from test_gpu_group_stats import device_view
from test_gpu_keyed import make_words
from test_gpu_optical import clustered

pytestmark = pytest.mark.gpu

U64 = np.uint64
E_INVALID = -1
WL_NT = 16


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


# ---- the passes, each with inputs and a truth that are computed once and never written --------------------------------
def correct_case(seed, n, wl):
    keys, filt = wt.make_keys(np.random.default_rng(seed), wl, WL_NT, n)
    return dict(keys=keys, filt=filt, truth=wt.correct_np(keys, filt, wl, WL_NT))


def do_correct(d, c):
    for name, a, b in zip(("key_out", "status", "counts"), c["truth"], d.correct_keys(c["keys"], c["filt"])):
        assert a.dtype == b.dtype and np.array_equal(a, b), name


def best_case(seed, n, nt):
    words, filt = make_words(seed, n, nt, n_base=max(4, n // 12))
    cid, keep, s, _ = orc.dedup_run(words, filt, nt, 1, 0)
    scores = np.random.default_rng(seed).integers(0, 50, n).astype(np.uint32)
    return dict(words=words, filt=filt, nt=nt, cid=cid, keep=keep, clusters=s["clusters"], scores=scores,
                truth={sc: best_truth(words, cid, keep, scores, sc) for sc in (bt.LEAF, bt.CLUSTER)})


def do_best(d, c, run=True):
    if run:
        cid, keep, s = d.run(c["words"], c["filt"], word_nt=c["nt"])
        assert np.array_equal(cid, c["cid"]) and np.array_equal(keep, c["keep"]) and s["clusters"] == c["clusters"]
    for name, scope in (("leaf", bt.LEAF), ("cluster", bt.CLUSTER)):
        bt.assert_same(c["truth"][scope], d.select_best(c["words"], c["cid"], c["keep"], c["scores"], c["nt"], scope=name), name)


def optical_case(seed, n, n_cl, D=100):
    cid, keep = clustered(seed, n, n_cl)
    tile, x, y = ot.make_positions(cid, keep, seed + 1, D=D, n_tiles=4, side=3000)
    t = ot.truth(cid, keep, tile, x, y, D, n_cl)
    assert t[3]["optical"] > 0
    return dict(cid=cid, keep=keep, tile=tile, x=x, y=y, D=D, n_cl=n_cl, truth=t)


def do_optical(d, c):
    got = d.optical_duplicates(c["cid"], c["keep"], c["tile"], c["x"], c["y"], distance=c["D"], n_clusters=c["n_cl"])
    ot.assert_same(got, c["truth"], "optical")


def consensus_case(seed, n, n_cl, lengths):
    rng = np.random.default_rng(seed)
    cid, keep = clustered(seed, n, n_cl)
    b, q, off = ct.random_reads(rng, cid, rng.choice(np.asarray(lengths), n))
    return dict(b=b, q=q, off=off, cid=cid, keep=keep, n_cl=n_cl, truth=consensus_truth(b, q, off, cid, keep, n_cl))


def do_consensus(d, c):
    ct.assert_same(c["truth"], d.consensus(c["b"], c["q"], c["cid"], c["keep"], off=c["off"], n_clusters=c["n_cl"]), "consensus")


def canonical_case(seed, n, nt):
    words, filt = make_words(seed, n, nt)
    return dict(words=words, filt=filt, nt=nt, truth=pt.canonical(words, filt, nt))


def do_canonical(d, c):
    out, strand = d.canonical_words(c["words"], c["filt"], word_nt=c["nt"])
    assert np.array_equal(out, c["truth"][0]) and np.array_equal(strand, c["truth"][1])


@pytest.fixture(scope="module")
def whitelist():
    return wt.whitelist_with_neighbours(np.random.default_rng(3), 400, WL_NT)


@pytest.fixture(scope="module")
def steps(whitelist):
    """the list of the issue, in its order: (what, call, case)"""
    return [("correct_keys 5000", do_correct, correct_case(11, 5000, whitelist)),
            ("select_best 300 x 24 nt", do_best, best_case(12, 300, 24)),
            ("optical 20000", do_optical, optical_case(13, 20000, 900)),
            ("select_best 2000 x 48 nt", do_best, best_case(14, 2000, 48)),     # 16-byte words where 4-byte ids were
            ("consensus 64, lengths 1 and 151", do_consensus, consensus_case(15, 64, 5, [1, 151])),
            ("canonical_words 7000 x 48 nt", do_canonical, canonical_case(16, 7000, 48)),
            ("optical 64", do_optical, optical_case(17, 64, 5))]


@pytest.fixture(scope="module")
def big(whitelist):
    """the three other passes on 10 000 reads (select_best with the run it needs)"""
    return [("select_best 10000", do_best, best_case(21, 10000, 24)),
            ("optical 10000", do_optical, optical_case(22, 10000, 500)),
            ("correct_keys 10000", do_correct, correct_case(23, 10000, whitelist))]


# ---- 1. sizes up and down, element widths changing ----------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_passes_of_changing_sizes_share_one_context(steps, whitelist, order):
    d = humid_amd.Dedup()
    try:
        d.set_whitelist(whitelist, WL_NT)
        for what, call, case in (steps if order == "forward" else steps[::-1]):
            try:
                call(d, case)
            except AssertionError as e:
                raise AssertionError("%s (%s): %s" % (what, order, e)) from e
    finally:
        d.close()


# ---- 2. what is not staging survives the pool ---------------------------------------------------------------------------
def test_packed_words_and_leaves_survive_later_passes(big, whitelist):
    n, nt = 1000, 24
    rng = np.random.default_rng(31)
    rows = rng.integers(0, 4, size=(n, nt))
    rows[1::2] = rows[0::2]                                             # pairs of equal words
    bases = np.frombuffer(b"ACGT", np.uint8)[rows]
    bases[5, 3] = ord("N")                                              # a filtered read
    d = humid_amd.Dedup()
    try:
        d.set_whitelist(whitelist, WL_NT)
        cid, keep, s = d.run_bases(bases, word_nt=nt)
        w, f = d.packed_words()
        assert f[5] == 1 and int(f.sum()) == 1
        ocid, okeep, osum, _ = orc.dedup_run(w, f, nt, 1, 0)
        assert np.array_equal(cid, ocid) and np.array_equal(keep, okeep)
        leaves = d.leaves()
        # select_best answers for the last run only, so it runs on this run's 1 000 reads; the others on 10 000
        scores = rng.integers(0, 50, n).astype(np.uint32)
        bt.assert_same(best_truth(w, cid, keep, scores, bt.LEAF), d.select_best(w, cid, keep, scores, nt))
        for what, call, case in big[1:]:
            call(d, case)
        w2, f2 = d.packed_words()
        assert np.array_equal(w2, w) and np.array_equal(f2, f)
        got = d.leaves()
        assert all(np.array_equal(got[k], leaves[k]) for k in leaves)
    finally:
        d.close()


def test_consensus_results_survive_later_passes(big, whitelist):
    c = consensus_case(32, 500, 40, [0, 1, 63, 64, 65, 151])
    d = humid_amd.Dedup()
    try:
        d.set_whitelist(whitelist, WL_NT)
        first = d.consensus(c["b"], c["q"], c["cid"], c["keep"], off=c["off"], n_clusters=c["n_cl"])
        ct.assert_same(c["truth"], first, "consensus")
        sm = first["summary"]
        for what, call, case in big:
            call(d, case)
        ct.assert_same(c["truth"], d._consensus_result(sm), "humid_get_consensus after the other passes")
        p = d.consensus_result_device()
        n_cl, tot = sm["n_clusters"], sm["total_bytes"]
        got = dict(out_off=device_view(p["out_off"], n_cl + 1, "<i8", U64), bases=device_view(p["bases"], tot, "|u1", np.uint8),
                   quals=device_view(p["quals"], tot, "|u1", np.uint8), depth=device_view(p["depth"], n_cl, "<i4", np.uint32),
                   errors=device_view(p["errors"], n_cl, "<i8", U64), summary=sm)
        ct.assert_same(c["truth"], got, "humid_consensus_result_device after the other passes")
    finally:
        d.close()


# ---- 3. the paired host run goes the way of every host run ---------------------------------------------------------------
@pytest.mark.parametrize("nt", [24, 48])
def test_paired_host_run_equals_its_device_form(nt):
    n = 3000
    words, filt = make_words(40 + nt, n, nt, n_base=250)
    words[1::2] = pt.mirror_words(words[1::2], nt)                       # half the reads from the other strand
    t = pt.run(words, filt, nt, 1)
    assert t["strands"]["duplex"] > 0 and t["strands"]["bottom_reads"] > 0
    cw = t["canonical"]
    scores = np.random.default_rng(nt).integers(0, 50, n).astype(np.uint32)
    best = best_truth(cw, t["cluster_id"], t["keep"], scores, bt.LEAF)

    def answers(d, cid, keep, s):
        for k in ("total", "usable", "unique", "clusters", "edges", "nonsingle"):
            assert s[k] == t["summary"][k], k
        assert np.array_equal(cid, t["cluster_id"]) and np.array_equal(keep, t["keep"])
        strand, top, bottom, sm = d.strands()
        assert np.array_equal(strand, t["strand"]) and np.array_equal(top, t["top"]) and np.array_equal(bottom, t["bottom"])
        assert sm == t["strands"]
        sel = d.select_best(cw, cid, keep, scores, nt)
        bt.assert_same(best, sel)
        return cid, keep, strand, top, bottom, sel[0], sel[1]

    d = humid_amd.Dedup()
    try:
        cid, keep, s = d.run_paired(words, filt, word_nt=nt, distance=1)
        assert s["ms_h2d"] >= 0
        host = answers(d, cid, keep, s)
        dev = torch.device("cuda:0")
        d_w = torch.from_numpy(words.reshape(-1).view(np.int64).copy()).to(dev)
        d_f = torch.from_numpy(filt).to(dev)
        d_cid = torch.zeros(n, dtype=torch.int32, device=dev)
        d_keep = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s = d.run_paired_device(d_w.data_ptr(), d_f.data_ptr(), d_cid.data_ptr(), d_keep.data_ptr(), n, word_nt=nt, distance=1)
        device = answers(d, d_cid.cpu().numpy().view(np.uint32), d_keep.cpu().numpy(), s)
        for a, b in zip(host, device):
            assert np.array_equal(a, b)
    finally:
        d.close()


# ---- 4. a refused host form moves nothing --------------------------------------------------------------------------------
def test_a_null_input_is_refused_by_every_host_form(steps, whitelist):
    """(as test_every_refusal_leaves_the_context_usable of the pass suites: the code, then the next valid call)"""
    correct, best, consensus, optical = steps[0][2], steps[1][2], steps[4][2], steps[6][2]
    canon = canonical_case(51, 300, 24)
    d = humid_amd.Dedup()
    try:
        lib, h = d._lib, d._h
        d.set_whitelist(whitelist, WL_NT)

        def refused(fn, ins, rest):
            """every input in turn NULL with n > 0; rest(ins) completes the argument list"""
            for hole in range(len(ins)):
                bad = list(ins)
                bad[hole] = None
                assert fn(h, *rest(bad)) == E_INVALID, (fn.__name__, hole)
                assert b"null buffer" in lib.humid_last_error(h)

        n = len(correct["filt"])
        out, status, counts = np.zeros(n, U64), np.zeros(n, np.uint8), np.zeros(5, U64)
        refused(lib.humid_whitelist_correct, [vp(correct["keys"]), vp(correct["filt"])],
                lambda a: a + [n, vp(out), vp(status), vp(counts)])
        do_correct(d, correct)

        do_best(d, best)                                                # (the run select_best needs)
        n = len(best["cid"])
        kout = np.zeros(n, np.uint8)
        refused(lib.humid_select_best, [vp(best["words"]), vp(best["cid"]), vp(best["keep"]), vp(best["scores"])],
                lambda a: a + [n, 24, 0, vp(kout), None, None])
        do_best(d, best, run=False)
        leaves = d.leaves()

        n = len(consensus["cid"])
        refused(lib.humid_consensus, [vp(consensus[k]) for k in ("b", "q", "off", "cid", "keep")],
                lambda a: a[:3] + [len(consensus["b"])] + a[3:] + [n, consensus["n_cl"], 10, 93, None])
        assert lib.humid_get_consensus(h, 0, None, None, None, None, None) == -6      # HUMID_E_STATE: no result left behind
        do_consensus(d, consensus)

        n = len(optical["cid"])
        opt = np.zeros(n, np.uint8)
        refused(lib.humid_optical_duplicates, [vp(optical[k]) for k in ("cid", "keep", "tile", "x", "y")],
                lambda a: a + [n, optical["n_cl"], optical["D"], vp(opt), None, None, None])
        do_optical(d, optical)

        n = len(canon["filt"])
        wout, strand = np.zeros(n, U64), np.zeros(n, np.uint8)
        refused(lib.humid_paired_canonical, [vp(canon["words"]), vp(canon["filt"])], lambda a: a + [n, 24, vp(wout), vp(strand)])
        do_canonical(d, canon)

        got = d.leaves()                                                # none of this touched the run
        assert all(np.array_equal(got[k], leaves[k]) for k in leaves)
        do_best(d, best, run=False)

        cid, keep = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        refused(lib.humid_dedup_run_paired, [vp(canon["words"]), vp(canon["filt"])], lambda a: a + [n, 24, 1, 0, vp(cid), vp(keep), None])
        assert lib.humid_get_strands(h, None, 0, None, None, None) == -6                # ... which leaves no run behind
        t = pt.run(canon["words"], canon["filt"], 24, 1)
        cid, keep, s = d.run_paired(canon["words"], canon["filt"], word_nt=24, distance=1)
        assert np.array_equal(cid, t["cluster_id"]) and np.array_equal(keep, t["keep"]) and np.array_equal(d.strands()[0], t["strand"])
    finally:
        d.close()
