"""The definition of the duplex consensus read of a cluster (include/humid_hip.h, humid_duplex_consensus), written
twice with nothing shared: a dict / loop form, cluster by cluster and column by column, and a whole-array numpy form
that scatters every vote into [2, C, Lmax, 4] tables with np.add.at.  TEST HELPER, never product code.  Both take two
layers of reads -- (bases, quals, off) of the SAME layer S and of the OTHER layer O -- with cluster_id / keep of any
run and strand u8[N], and return
  dict(out_off u64[C + 1], bases u8[total], quals u8[total], depth u32[C], errors u64[C], depth_same u32[C],
       depth_other u32[C], disagree u32[C], summary dict of KEYS)."""
import numpy as np

KEYS = ("n_clusters", "total_bytes", "multi_read", "bases_changed", "votes", "errors", "duplex_clusters", "both_called",
        "agree", "disagree", "masked")
ARRAYS = ("out_off", "bases", "quals", "depth", "errors", "depth_same", "depth_other", "disagree")
ACGT = b"ACGT"
TOP, BOTTOM, NONE = 0, 1, 2


def duplex_loop(layer_s, layer_o, cid, keep, strand, n_clusters, min_q=10, strand_cap_q=40, cap_q=93):
    layers = []
    for b, q, off in (layer_s, layer_o):
        layers.append((bytes(np.asarray(b, np.uint8)), bytes(np.asarray(q, np.uint8)), [int(x) for x in off]))
    cid, keep, strand = [np.asarray(x).tolist() for x in (cid, keep, strand)]
    members, rep = {}, {}
    for i, (c, k) in enumerate(zip(cid, keep)):
        if c == 0:
            continue
        assert 1 <= c <= n_clusters and strand[i] in (TOP, BOTTOM)
        members.setdefault(c, []).append(i)
        if k:
            assert c not in rep
            rep[c] = i
    ob, oq, out_off = bytearray(), bytearray(), [0]
    per = {k: [] for k in ("depth", "errors", "depth_same", "depth_other", "disagree")}
    sm = dict.fromkeys(KEYS, 0)
    sm["n_clusters"] = n_clusters
    thr = max(min_q, 1)
    sb, sq, soff = layers[0]
    for c in range(1, n_clusters + 1):
        r = rep[c]
        # class 0 (X): the representative's strand, voting with layer S; class 1 (Y): the others, with layer O
        cls = [[i for i in members[c] if strand[i] == strand[r]], [i for i in members[c] if strand[i] != strand[r]]]
        err = dis = 0
        for j in range(soff[r + 1] - soff[r]):
            calls, votes = [], 0
            for s in (0, 1):
                lb, lq, loff = layers[s]
                S, n = [0, 0, 0, 0], [0, 0, 0, 0]
                for i in cls[s]:
                    if j >= loff[i + 1] - loff[i]:
                        continue
                    b, p = lb[loff[i] + j], min(max(lq[loff[i] + j] - 33, 0), 93)
                    if b in ACGT and p >= thr:
                        S[ACGT.index(b)] += p
                        n[ACGT.index(b)] += 1
                votes += sum(n)
                order = sorted(S, reverse=True)
                m = min(order[0] - order[1], strand_cap_q)
                if m > 0:
                    w = S.index(order[0])
                    calls.append((ACGT[w], m))
                    err += sum(n) - n[w]
            rb, rq = sb[soff[r] + j], sq[soff[r] + j]
            sm["votes"] += votes
            if votes == 0:
                b, q = rb, rq
            else:
                b, m = ord("N"), 0
                if len(calls) == 2:
                    sm["both_called"] += 1
                    (b0, m0), (b1, m1) = calls
                    if b0 == b1:
                        sm["agree"] += 1
                        b, m = b0, m0 + m1
                    else:
                        dis += 1
                        if m0 != m1:
                            b, m = (b0 if m0 > m1 else b1), abs(m0 - m1)
                elif len(calls) == 1:
                    b, m = calls[0]
                if m == 0:
                    b, q = ord("N"), ord("!")
                    sm["masked"] += 1
                else:
                    q = 33 + min(m, cap_q)
            sm["bases_changed"] += b != rb
            ob.append(b)
            oq.append(q)
        out_off.append(len(ob))
        per["depth"].append(len(members[c]))
        per["depth_same"].append(len(cls[0]))
        per["depth_other"].append(len(cls[1]))
        per["errors"].append(err)
        per["disagree"].append(dis)
        sm["multi_read"] += len(members[c]) >= 2
        sm["duplex_clusters"] += len(cls[1]) > 0
        sm["errors"] += err
        sm["disagree"] += dis
    sm["total_bytes"] = len(ob)
    sm = {k: int(v) for k, v in sm.items()}
    out = dict(out_off=np.asarray(out_off, np.uint64), bases=np.frombuffer(bytes(ob), np.uint8),
               quals=np.frombuffer(bytes(oq), np.uint8), summary=sm)
    for k, v in per.items():
        out[k] = np.asarray(v, np.uint64 if k == "errors" else np.uint32).reshape(-1)
    return out


def duplex_numpy(layer_s, layer_o, cid, keep, strand, n_clusters, min_q=10, strand_cap_q=40, cap_q=93):
    cid, keep, strand = np.asarray(cid, np.int64), np.asarray(keep), np.asarray(strand, np.int64)
    C = int(n_clusters)
    member = cid != 0
    assert cid.max(initial=0) <= C and np.all(strand[member] <= 1)
    reps = np.flatnonzero(member & (keep != 0))
    assert len(reps) == C and np.array_equal(np.sort(cid[reps]), np.arange(1, C + 1))
    rep = np.zeros(C + 1, np.int64)
    rep[cid[reps]] = reps
    bs, qs, offs = np.asarray(layer_s[0], np.uint8), np.asarray(layer_s[1], np.uint8), np.asarray(layer_s[2], np.int64)
    rlen = np.diff(offs)[rep[1:]] if C else np.zeros(0, np.int64)
    out_off = np.zeros(C + 1, np.int64)
    out_off[1:] = np.cumsum(rlen)
    total, lmax = int(out_off[C]), int(rlen.max(initial=0))
    other = member & (strand != strand[rep[cid]])                      # class Y; (cid 0 indexes rep[0]: masked by member)
    depth = np.bincount(cid[member], minlength=C + 1)[1:]
    d_other = np.bincount(cid[other], minlength=C + 1)[1:]
    code = np.full(256, -1, np.int64)
    code[list(ACGT)] = np.arange(4)
    S = np.zeros((2, C + 1, lmax, 4), np.int64)
    n = np.zeros((2, C + 1, lmax, 4), np.int64)
    for s, (lb, lq, loff) in enumerate((layer_s, layer_o)):
        lb, lq, loff = np.asarray(lb, np.uint8), np.asarray(lq, np.uint8), np.asarray(loff, np.int64)
        mine = other if s else member & ~other
        use = np.where(mine, np.minimum(np.diff(loff), np.r_[0, rlen][cid]), 0)
        read = np.repeat(np.arange(len(cid)), use)
        col = np.arange(int(use.sum())) - np.repeat(np.cumsum(use) - use, use)
        b, p = lb[loff[read] + col], np.clip(lq[loff[read] + col].astype(np.int64) - 33, 0, 93)
        ok = (code[b] >= 0) & (p >= max(min_q, 1))
        at = (cid[read[ok]] * lmax + col[ok]) * 4 + code[b[ok]]
        np.add.at(S[s].reshape(-1), at, p[ok])
        np.add.at(n[s].reshape(-1), at, 1)
    oc = np.repeat(np.arange(1, C + 1), rlen)
    oj = np.arange(total) - np.repeat(out_off[:-1], rlen)
    S, n = S[:, oc, oj], n[:, oc, oj]                                  # [2, total, 4]
    rb, rq = bs[offs[rep[oc]] + oj], qs[offs[rep[oc]] + oj]
    srt = np.sort(S, axis=2)
    win = np.argmax(S, axis=2)                                         # [2, total]; the first of equals: A C G T
    m = np.minimum(srt[:, :, 3] - srt[:, :, 2], strand_cap_q)
    nv = n.sum(axis=2)
    nwin = np.take_along_axis(n, win[:, :, None], axis=2)[:, :, 0]
    call = m > 0
    err = np.where(call, nv - nwin, 0).sum(axis=0)
    votes = nv.sum(axis=0)
    both = call[0] & call[1]
    same = both & (win[0] == win[1])
    differ = both & ~same
    xbig = m[0] > m[1]
    margin = np.where(same, m[0] + m[1], np.where(differ, np.abs(m[0] - m[1]), np.where(call[0], m[0], np.where(call[1], m[1], 0))))
    who = np.where(same, win[0], np.where(differ, np.where(xbig, win[0], win[1]), np.where(call[0], win[0], win[1])))
    none = votes == 0
    masked = ~none & (margin == 0)
    letters = np.frombuffer(ACGT, np.uint8)
    ob = np.where(none, rb, np.where(masked, ord("N"), letters[who])).astype(np.uint8)
    oq = np.where(none, rq, np.where(masked, ord("!"), 33 + np.minimum(margin, cap_q))).astype(np.uint8)
    per = lambda x: np.bincount(oc, weights=x, minlength=C + 1)[1:]
    sm = dict(n_clusters=C, total_bytes=total, multi_read=int((depth >= 2).sum()), bases_changed=int((ob != rb).sum()),
              votes=int(votes.sum()), errors=int(err.sum()), duplex_clusters=int((d_other > 0).sum()),
              both_called=int(both.sum()), agree=int(same.sum()), disagree=int(differ.sum()), masked=int(masked.sum()))
    return dict(out_off=out_off.astype(np.uint64), bases=ob, quals=oq, depth=depth.astype(np.uint32),
                errors=per(err).astype(np.uint64), depth_same=(depth - d_other).astype(np.uint32),
                depth_other=d_other.astype(np.uint32), disagree=per(differ).astype(np.uint32), summary=sm)


def assert_same(a, b, what="", keys=ARRAYS, summary_keys=KEYS):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, "%s: %s has shapes %r and %r" % (what, k, x.shape, y.shape)
        if not np.array_equal(x, y):
            i = int(np.flatnonzero(x != y)[0])
            raise AssertionError("%s: %s differs first at %d: %r != %r (%d places)" % (what, k, i, x[i], y[i],
                                                                                        np.count_nonzero(x != y)))
    sa, sb = a["summary"], b["summary"]
    assert {k: int(sa[k]) for k in summary_keys} == {k: int(sb[k]) for k in summary_keys}, \
        "%s: summaries %r != %r" % (what, sa, sb)


def rep_strand(cid, keep, strand):
    """strand of the representative of every read's cluster (0 where cluster_id == 0)"""
    cid, strand = np.asarray(cid, np.int64), np.asarray(strand, np.uint8)
    reps = np.flatnonzero((cid != 0) & (np.asarray(keep) != 0))
    rs = np.zeros(int(cid.max(initial=0)) + 1, np.uint8)
    rs[cid[reps]] = strand[reps]
    return rs[cid]


def duplex_reads(rng, cid, strand, keep, lengths1, lengths2, p_err=0.02, p_n=0.01, p_lower=0.005, q_lo=2, q_hi=41,
                 odd_quals=False, plant=None):
    """Two layers of reads for the given cluster ids: one template pair (T1, T2) per cluster; a member of the
    representative's strand carries T1 in layer 1 and T2 in layer 2, a member of the other strand T2 in layer 1 and T1
    in layer 2; each record is cut to its length (lengths1 / lengths2 per read), with substitutions at rate p_err, some
    N and some lowercase bytes, qualities uniform in [q_lo, q_hi] and with odd_quals also bytes below 33 and above 126
    -- as consensus_truth.random_reads makes them.
    plant = (cls, column): a strand-specific error -- every member of class cls ("same" or "other") carries the SAME
    wrong base at that column of its T1 record (the one that votes when layer 1 is the same layer).
    Returns ((bases1, quals1, off1), (bases2, quals2, off2))."""
    cid = np.asarray(cid, np.int64)
    other = (cid != 0) & (np.asarray(strand, np.uint8) != rep_strand(cid, keep, strand))
    lengths = [np.asarray(lengths1, np.int64), np.asarray(lengths2, np.int64)]
    lmax = max(1, int(lengths[0].max(initial=0)), int(lengths[1].max(initial=0)))
    acgt = np.frombuffer(ACGT, np.uint8)
    tcode = rng.integers(0, 4, (2, int(cid.max(initial=0)) + 1, lmax))
    layers = []
    for layer in (0, 1):
        ln = lengths[layer]
        off = np.zeros(len(cid) + 1, np.uint64)
        off[1:] = np.cumsum(ln, dtype=np.uint64)
        read = np.repeat(np.arange(len(cid)), ln)
        col = np.arange(int(ln.sum())) - np.repeat(off[:-1].astype(np.int64), ln)
        which = np.where(other[read], 1 - layer, layer)                 # the template this record carries
        b = acgt[tcode[which, cid[read], col]]
        m = len(b)
        u = rng.random(m)
        sub = u < p_err
        b[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
        b[(u >= p_err) & (u < p_err + p_n)] = ord("N")
        b[(u >= p_err + p_n) & (u < p_err + p_n + p_lower)] |= 0x20
        q = (33 + rng.integers(q_lo, q_hi + 1, m, dtype=np.uint8)).astype(np.uint8)
        if odd_quals:
            odd = rng.random(m) < 0.02
            q[odd] = rng.choice(np.asarray([0, 10, 32, 127, 200, 255], np.uint8), int(odd.sum()))
        if plant is not None:
            cls, pcol = plant
            hit = (cid[read] != 0) & (which == 0) & (col == pcol) & (other[read] == (cls == "other"))
            b[hit] = acgt[(tcode[0, cid[read[hit]], pcol] + 1) % 4]
        layers.append((b, q, off))
    return layers[0], layers[1]


def sized_clusters(rng, sizes, tops, n_zero=0, shuffle=True, rep_top=None):
    """(cluster_id u32, keep u8, strand u8) for clusters of the given sizes (ids in the given order), tops[k] of whose
    members are TOP reads and the others BOTTOM reads, plus n_zero reads without a cluster (strand NONE); keep = a
    random member of every cluster, or with rep_top[k] True / False a random TOP / BOTTOM member"""
    cid, strand = [], []
    for k, (d, t) in enumerate(zip(sizes, tops)):
        assert 0 <= t <= d
        cid += [k + 1] * d
        strand += [TOP] * t + [BOTTOM] * (d - t)
    cid = np.asarray(cid + [0] * n_zero, np.uint32)
    strand = np.asarray(strand + [NONE] * n_zero, np.uint8)
    if shuffle:
        perm = rng.permutation(len(cid))
        cid, strand = cid[perm], strand[perm]
    keep = np.zeros(len(cid), np.uint8)
    for k in range(len(sizes)):
        who = np.flatnonzero(cid == k + 1)
        if rep_top is not None and rep_top[k] is not None:
            who = who[strand[who] == (TOP if rep_top[k] else BOTTOM)]
        keep[who[int(rng.integers(0, len(who)))]] = 1
    return cid, keep, strand
