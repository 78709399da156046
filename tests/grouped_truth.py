"""Two independent truths of a grouped run (include/humid_hip.h, humid_dedup_run_grouped) from the CPU oracle.

TEST HELPER, never product code.

per_group():   the contract itself -- one oracle pass per group over the group's usable reads in input order,
               cluster ids raised by the clusters of the groups below, leaves / adjacency / clusters of the
               groups concatenated in group order with their leaf indices shifted.
repetition():  ONE oracle pass: the rank of every read's group in base 4, each digit written d + 1 times, in
               front of the word.  Two words of different groups then differ in at least d + 1 nucleotides (never
               Hamming neighbours) and the order of (group, word) is kept.  Hamming only.
Both return the same dict: cid, keep, summary, leaves (with "group"), off, idx, clusters, hist.
"""
import numpy as np

from oracle import pyoracle as orc


def _pack(words, n):
    """words as a plain Python int per read (u64 or [hi, lo] rows)"""
    w = np.asarray(words, dtype=np.uint64)
    if n > 32:
        w = w.reshape(-1, 2)
        return [(int(a) << 64) | int(b) for a, b in w]
    return [int(x) for x in w.reshape(-1)]


def _unpack(vals, n):
    if n > 32:
        out = np.zeros((len(vals), 2), np.uint64)
        for i, v in enumerate(vals):
            out[i, 0] = v >> 64
            out[i, 1] = v & ((1 << 64) - 1)
        return out
    return np.asarray(vals, dtype=np.uint64).reshape(-1)


def _hist(a):
    k, v = np.unique(np.asarray(a, dtype=np.uint64), return_counts=True)
    return [(int(x), int(y)) for x, y in zip(k, v)]


def _histograms(t):
    s = t["summary"]
    return dict(counts=_hist(t["leaves"]["count"]), neigh=_hist(t["leaves"]["degree"]),
                clusters=_hist(t["clusters"]["size"]),
                stats=dict(total=s["total"], usable=s["usable"], unique=s["unique"], clusters=s["clusters"]))


def _oracle(words, n, distance, method, edit, filtered=None):
    p = orc.Pipeline(n)
    p.read_data(words, np.zeros(len(words), np.uint8) if filtered is None else filtered)
    if edit and distance >= 2:
        p.find_edit_neighbours(distance)
    else:
        p.find_hamming_neighbours(distance)
    p.find_clusters(bool(method))
    return p


def per_group(words, groups, filtered, word_nt, distance=1, method=0, edit=False, first_read=True):
    """the definition: one oracle pass per group"""
    f = np.asarray(filtered, dtype=np.uint8)
    g = np.asarray(groups, dtype=np.uint32)
    w = np.asarray(words, dtype=np.uint64)
    w = w.reshape(-1, 2) if word_nt > 32 else w.reshape(-1)
    N = len(f)
    cid = np.zeros(N, np.uint32)
    keep = np.zeros(N, np.uint8)
    usable = np.flatnonzero(f == 0)
    summary = dict(total=N, usable=len(usable), unique=0, clusters=0, edges=0)
    parts = dict(word=[], count=[], degree=[], cluster_id=[], is_max_leaf=[], group=[], first_read=[])
    offs, idxs = [np.zeros(1, np.uint64)], []
    cl = dict(size=[], max_count=[], max_leaf=[])
    n_leaves = n_clusters = 0
    gu = g[usable]
    order = np.argsort(gu, kind="stable")
    bounds = np.flatnonzero(np.diff(gu[order])) + 1
    for sel_o in np.split(order, bounds) if len(order) else []:
        sel = usable[sel_o]                                      # the group's usable reads, input order
        grp = int(g[sel[0]])
        p = _oracle(w[sel], word_nt, distance, method, edit)
        c, k = p.map_reads()
        c = c.astype(np.uint64)
        c[c > 0] += n_clusters
        cid[sel] = c.astype(np.uint32)
        keep[sel] = k
        lv = p.leaves()
        u = p.unique
        for key in ("word", "count", "degree", "is_max_leaf"):
            parts[key].append(lv[key])
        lcid = lv["cluster_id"].astype(np.uint64)
        lcid[lcid > 0] += n_clusters
        parts["cluster_id"].append(lcid.astype(np.uint32))
        parts["group"].append(np.full(u, grp, np.uint32))
        if first_read:
            first = {}
            for j, v in zip(sel, _pack(w[sel], word_nt)):
                first.setdefault(v, int(j))
            parts["first_read"].append(np.asarray([first[v] for v in sorted(first)], np.uint32))
        off, idx = p.adjacency()
        offs.append(off[1:] + offs[-1][-1])
        idxs.append(idx.astype(np.uint32) + n_leaves)
        pc = p.clusters()
        cl["size"].append(pc["size"])
        cl["max_count"].append(pc["max_count"])
        cl["max_leaf"].append(pc["max_leaf"] + n_leaves)
        s = p.summary()
        for key in ("unique", "clusters", "edges"):
            summary[key] += s[key]
        n_leaves += u
        n_clusters += s["clusters"]
    cat = lambda l, dt, shape=(0,): np.concatenate(l).astype(dt) if l else np.zeros(shape, dt)   # noqa: E731
    leaves = dict(word=cat(parts["word"], np.uint64, (0, 2) if word_nt > 32 else (0,)),
                  count=cat(parts["count"], np.uint64), degree=cat(parts["degree"], np.uint32),
                  cluster_id=cat(parts["cluster_id"], np.uint32), is_max_leaf=cat(parts["is_max_leaf"], np.uint8),
                  group=cat(parts["group"], np.uint32))
    if first_read:
        leaves["first_read"] = cat(parts["first_read"], np.uint32)
    t = dict(cid=cid, keep=keep, summary=summary, leaves=leaves,
             off=np.concatenate(offs).astype(np.uint64), idx=cat(idxs, np.uint32),
             clusters=dict(size=cat(cl["size"], np.uint64), max_count=cat(cl["max_count"], np.uint64),
                           max_leaf=cat(cl["max_leaf"], np.uint32)))
    t["hist"] = _histograms(t)
    return t


def _oracle_engine(words, filtered, n, distance, method):
    p = _oracle(words, n, distance, method, False, filtered)
    cid, keep = p.map_reads()
    s = p.summary()
    off, idx = p.adjacency()
    return dict(cid=cid, keep=keep, summary=s, leaves=p.leaves(), off=off, idx=idx, clusters=p.clusters())


def _split128(hi, lo, wb):
    """(hi, lo) of 128-bit values -> (value >> wb, value & (2^wb - 1)) as (code u64, word hi u64, word lo u64)"""
    if wb >= 64:
        s = np.uint64(wb - 64)
        m = np.uint64((1 << (wb - 64)) - 1) if wb < 128 else np.uint64(0xFFFFFFFFFFFFFFFF)
        return (hi >> s) if wb < 128 else np.zeros_like(hi), hi & m, lo
    s = np.uint64(wb)
    code = (lo >> s) | (hi << np.uint64(64 - wb)) if wb else hi
    return code, np.zeros_like(lo), lo & np.uint64((1 << wb) - 1)


def repetition(words, groups, filtered, word_nt, distance=1, method=0, engine=None):
    """ONE pass over the group rank in a repetition code in front of the word (Hamming only).  engine(words,
    filtered, n, distance, method) -> the dict of _oracle_engine; default: the CPU oracle."""
    engine = engine or _oracle_engine
    f = np.asarray(filtered, dtype=np.uint8)
    g = np.asarray(groups, dtype=np.uint32)
    w = np.asarray(words, dtype=np.uint64)
    w = w.reshape(-1, 2) if word_nt > 32 else w.reshape(-1)
    N = len(f)
    usable = f == 0
    present = np.unique(g[usable])
    rank = np.zeros(N, np.uint64)
    rank[usable] = np.searchsorted(present, g[usable]).astype(np.uint64)
    digits = 1
    while 4 ** digits < max(len(present), 1):
        digits += 1
    rep = distance + 1
    n = word_nt + digits * rep
    assert n <= 64 and digits * rep <= 32, "the repetition code needs %d nt" % n
    code = np.zeros(N, np.uint64)
    for t in range(digits):                                    # digit t (least significant first) -> rep copies
        dgt = (rank >> np.uint64(2 * t)) & np.uint64(3)
        for q in range(rep):
            code |= dgt << np.uint64(2 * (t * rep + q))
    wb = 2 * word_nt
    whi, wlo = (w[:, 0], w[:, 1]) if word_nt > 32 else (np.zeros(N, np.uint64), w)
    if wb >= 64:
        hi, lo = whi | (code << np.uint64(wb - 64)), wlo
    else:
        lo = wlo | (code << np.uint64(wb))
        hi = (code >> np.uint64(64 - wb)) if wb else code
    full = np.stack([hi, lo], 1) if n > 32 else lo
    r = engine(full, f, n, distance, method)
    lw = np.asarray(r["leaves"]["word"], np.uint64)
    lhi, llo = (lw[:, 0], lw[:, 1]) if n > 32 else (np.zeros(len(lw), np.uint64), lw)
    lcode, ohi, olo = _split128(lhi, llo, wb)
    lrank = np.zeros(len(lw), np.int64)
    for t in range(digits):
        lrank += (((lcode >> np.uint64(2 * t * rep)) & np.uint64(3)).astype(np.int64)) << (2 * t)
    lv = r["leaves"]
    leaves = dict(word=np.stack([ohi, olo], 1) if word_nt > 32 else olo, count=lv["count"], degree=lv["degree"],
                  cluster_id=lv["cluster_id"], is_max_leaf=lv["is_max_leaf"],
                  group=present[lrank].astype(np.uint32) if len(lw) else np.zeros(0, np.uint32))
    if "first_read" in lv:
        leaves["first_read"] = lv["first_read"]
    s = r["summary"]
    t = dict(cid=r["cid"], keep=r["keep"], summary=dict(total=N, usable=s["usable"], unique=s["unique"],
                                                        clusters=s["clusters"], edges=s["edges"]),
             leaves=leaves, off=np.asarray(r["off"]).astype(np.uint64), idx=np.asarray(r["idx"]).astype(np.uint32),
             clusters=r["clusters"])
    t["hist"] = _histograms(t)
    return t


def assert_same(a, b, first_read=False):
    """two results (truths, or a truth and the device's) agree bit for bit"""
    for k in ("total", "usable", "unique", "clusters", "edges"):
        assert int(a["summary"][k]) == int(b["summary"][k]), (k, a["summary"][k], b["summary"][k])
    assert np.array_equal(a["cid"], b["cid"])
    assert np.array_equal(a["keep"], b["keep"])
    keys = ["word", "count", "degree", "cluster_id", "is_max_leaf", "group"] + (["first_read"] if first_read else [])
    for k in keys:
        assert np.array_equal(np.asarray(a["leaves"][k]).astype(np.uint64), np.asarray(b["leaves"][k]).astype(np.uint64)), k
    assert np.array_equal(np.asarray(a["off"]).astype(np.uint64), np.asarray(b["off"]).astype(np.uint64))
    assert np.array_equal(np.asarray(a["idx"]).astype(np.uint32), np.asarray(b["idx"]).astype(np.uint32))
    for k in ("size", "max_count", "max_leaf"):
        assert np.array_equal(np.asarray(a["clusters"][k]).astype(np.uint64),
                              np.asarray(b["clusters"][k]).astype(np.uint64)), k
    assert a["hist"] == b["hist"]


def device_result(dd, words, groups, filtered, word_nt, n_groups=None, distance=1, method=0, edit=False):
    """Dedup.run_grouped + every accessor, in the truths' dict form"""
    cid, keep, s = dd.run_grouped(words, groups, filtered, word_nt=word_nt, n_groups=n_groups, distance=distance,
                                  method=method, edit=edit)
    lv = dd.leaves()
    off, idx = dd.adjacency()
    return dict(cid=cid, keep=keep, summary=s, leaves=lv, off=off, idx=idx, clusters=dd.clusters(),
                hist=dd.histograms())


def device_engine(dd):
    """an engine for repetition(): the plain device pass (Dedup.run, itself bit-exact against the oracle) over the
    coded words -- for read sets the CPU oracle takes minutes over"""
    def run(words, filtered, n, distance, method):
        cid, keep, s = dd.run(words, filtered, word_nt=n, distance=distance, method=method)
        off, idx = dd.adjacency()
        return dict(cid=cid, keep=keep, summary=s, leaves=dd.leaves(), off=off, idx=idx, clusters=dd.clusters())
    return run
