"""The definition of the consensus read of a cluster (include/humid_hip.h, humid_consensus), written twice with
nothing shared (and a third time for reads of one length, consensus_matrix): a dict / loop form, cluster by cluster and column by column, and a whole-array numpy form that
scatters every vote into [C, Lmax, 4] tables with np.add.at.  Both take one layer of reads -- flat ASCII blobs bases /
quals and off u64[N + 1] -- with cluster_id / keep of any run, and return
  dict(out_off u64[C + 1], bases u8[total], quals u8[total], depth u32[C], errors u64[C], summary dict)."""
import numpy as np

KEYS = ("n_clusters", "total_bytes", "multi_read", "bases_changed", "votes", "errors")
ACGT = b"ACGT"


def flat(reads_b, reads_q):
    """lists of bytes objects -> (bases, quals, off)"""
    assert [len(x) for x in reads_b] == [len(x) for x in reads_q]
    off = np.zeros(len(reads_b) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in reads_b], dtype=np.uint64)
    return (np.frombuffer(b"".join(reads_b), np.uint8).copy(), np.frombuffer(b"".join(reads_q), np.uint8).copy(), off)


def consensus_loop(bases, quals, off, cid, keep, n_clusters, min_q=10, cap_q=93):
    bases, quals = bytes(np.asarray(bases, np.uint8)), bytes(np.asarray(quals, np.uint8))
    off = [int(x) for x in off]
    members, rep = {}, {}
    for i, (c, k) in enumerate(zip(cid.tolist(), keep.tolist())):
        if c == 0:
            continue
        assert 1 <= c <= n_clusters
        members.setdefault(c, []).append(i)
        if k:
            assert c not in rep
            rep[c] = i
    ob, oq, out_off = bytearray(), bytearray(), [0]
    depth, errors = [], []
    sm = dict.fromkeys(KEYS, 0)
    sm["n_clusters"] = n_clusters
    thr = max(min_q, 1)
    for c in range(1, n_clusters + 1):
        r = rep[c]
        length = off[r + 1] - off[r]
        err = 0
        for j in range(length):
            S, n = [0, 0, 0, 0], [0, 0, 0, 0]
            for i in members[c]:
                if j >= off[i + 1] - off[i]:
                    continue
                b, p = bases[off[i] + j], min(max(quals[off[i] + j] - 33, 0), 93)
                if b in ACGT and p >= thr:
                    S[ACGT.index(b)] += p
                    n[ACGT.index(b)] += 1
            rb, rq = bases[off[r] + j], quals[off[r] + j]
            sm["votes"] += sum(n)
            if sum(n) == 0:
                b, q = rb, rq
            else:
                order = sorted(S, reverse=True)
                if order[0] == order[1]:
                    b, q = ord("N"), ord("!")
                else:
                    w = S.index(order[0])
                    b, q = ACGT[w], 33 + min(order[0] - order[1], cap_q)
                    err += sum(n) - n[w]
            sm["bases_changed"] += b != rb
            ob.append(b)
            oq.append(q)
        out_off.append(len(ob))
        depth.append(len(members[c]))
        errors.append(err)
        sm["multi_read"] += len(members[c]) >= 2
        sm["errors"] += err
    sm["total_bytes"] = len(ob)
    sm = {k: int(v) for k, v in sm.items()}
    return dict(out_off=np.asarray(out_off, np.uint64), bases=np.frombuffer(bytes(ob), np.uint8),
                quals=np.frombuffer(bytes(oq), np.uint8), depth=np.asarray(depth, np.uint32).reshape(-1),
                errors=np.asarray(errors, np.uint64).reshape(-1), summary=sm)


def consensus_numpy(bases, quals, off, cid, keep, n_clusters, min_q=10, cap_q=93):
    bases, quals = np.asarray(bases, np.uint8), np.asarray(quals, np.uint8)
    off, cid, keep = np.asarray(off, np.int64), np.asarray(cid, np.int64), np.asarray(keep)
    C = int(n_clusters)
    lens = np.diff(off)
    member = cid != 0
    assert cid.max(initial=0) <= C
    reps = np.flatnonzero(member & (keep != 0))
    assert len(reps) == C and np.array_equal(np.sort(cid[reps]), np.arange(1, C + 1))
    rep = np.zeros(C + 1, np.int64)
    rep[cid[reps]] = reps
    rlen = lens[rep[1:]] if C else np.zeros(0, np.int64)
    out_off = np.zeros(C + 1, np.int64)
    out_off[1:] = np.cumsum(rlen)
    total, lmax = int(out_off[C]), int(rlen.max(initial=0))
    depth = np.bincount(cid[member], minlength=C + 1)[1:]
    # every byte of every member read, cut to its representative's length: (read, column)
    use = np.minimum(lens, np.where(member, np.r_[0, rlen][cid], 0))
    read = np.repeat(np.arange(len(cid)), use)
    col = np.arange(int(use.sum())) - np.repeat(np.cumsum(use) - use, use)
    b, q = bases[off[read] + col], quals[off[read] + col]
    p = np.clip(q.astype(np.int64) - 33, 0, 93)
    code = np.full(256, -1, np.int64)
    code[list(ACGT)] = np.arange(4)
    ok = (code[b] >= 0) & (p >= max(min_q, 1))
    S = np.zeros((C + 1, lmax, 4), np.int64)
    n = np.zeros((C + 1, lmax, 4), np.int64)
    at = (cid[read[ok]] * lmax + col[ok]) * 4 + code[b[ok]]              # (flat index: the tables are contiguous)
    np.add.at(S.reshape(-1), at, p[ok])
    np.add.at(n.reshape(-1), at, 1)
    # the output positions: (cluster, column) of every output byte
    oc = np.repeat(np.arange(1, C + 1), rlen)
    oj = np.arange(total) - np.repeat(out_off[:-1], rlen)
    S, n = S[oc, oj], n[oc, oj]                                        # [total, 4]
    rb, rq = bases[off[rep[oc]] + oj], quals[off[rep[oc]] + oj]
    srt = np.sort(S, axis=1)
    first, second, win = srt[:, 3], srt[:, 2], np.argmax(S, axis=1)
    nv = n.sum(axis=1)
    none, tie = nv == 0, (nv != 0) & (first == second)
    ob = np.where(none, rb, np.where(tie, ord("N"), np.frombuffer(ACGT, np.uint8)[win])).astype(np.uint8)
    oq = np.where(none, rq, np.where(tie, ord("!"), 33 + np.minimum(first - second, cap_q))).astype(np.uint8)
    err = np.where(none | tie, 0, nv - n[np.arange(total), win])
    errors = np.bincount(oc, weights=err, minlength=C + 1)[1:].astype(np.uint64)
    sm = dict(n_clusters=C, total_bytes=total, multi_read=int((depth >= 2).sum()), bases_changed=int((ob != rb).sum()),
              votes=int(nv.sum()), errors=int(err.sum()))
    return dict(out_off=out_off.astype(np.uint64), bases=ob, quals=oq, depth=depth.astype(np.uint32), errors=errors,
                summary=sm)


def consensus_matrix(bases, quals, cid, keep, n_clusters, min_q=10, cap_q=93, chunk=200_000):
    """A third form for reads of ONE length, u8[N, L] matrices (what tools/bench_consensus.py verifies 10 M reads
    with): the reads sorted by cluster, the sums as np.add.reduceat over each cluster's rows, `chunk` clusters at a
    time.  tests/test_consensus_host.py holds it against the other two."""
    B, Q = np.asarray(bases, np.uint8), np.asarray(quals, np.uint8)
    cid, keep = np.asarray(cid, np.int64), np.asarray(keep)
    C, L = int(n_clusters), B.shape[1]
    order = np.argsort(cid, kind="stable")
    first = np.searchsorted(cid[order], np.arange(1, C + 2))
    depth = np.diff(first)
    assert cid.max(initial=0) <= C and np.all(depth >= 1)
    reps = np.flatnonzero((cid != 0) & (keep != 0))
    assert len(reps) == C and np.array_equal(np.sort(cid[reps]), np.arange(1, C + 1))
    rep = np.zeros(C + 1, np.int64)
    rep[cid[reps]] = reps
    ob, oq = np.empty((C, L), np.uint8), np.empty((C, L), np.uint8)
    errors = np.zeros(C, np.uint64)
    sm = dict(n_clusters=C, total_bytes=C * L, multi_read=int((depth >= 2).sum()), bases_changed=0, votes=0, errors=0)
    letters = np.frombuffer(ACGT, np.uint8)
    for c0 in range(0, C, chunk):
        c1 = min(C, c0 + chunk)
        rows = order[first[c0]:first[c1]]
        Bc = B[rows]
        p = np.clip(Q[rows].astype(np.int32) - 33, 0, 93)
        ok = p >= max(min_q, 1)
        at = first[c0:c1] - first[c0]
        S = np.stack([np.add.reduceat(np.where(ok & (Bc == ch), p, 0), at, axis=0) for ch in letters], axis=2)
        n = np.stack([np.add.reduceat((ok & (Bc == ch)).astype(np.int32), at, axis=0) for ch in letters], axis=2)
        srt = np.sort(S, axis=2)
        top, second, win = srt[:, :, 3], srt[:, :, 2], np.argmax(S, axis=2)
        nv = n.sum(axis=2)
        none, tie = nv == 0, (nv != 0) & (top == second)
        rb, rq = B[rep[c0 + 1:c1 + 1]], Q[rep[c0 + 1:c1 + 1]]
        ob[c0:c1] = np.where(none, rb, np.where(tie, ord("N"), letters[win]))
        oq[c0:c1] = np.where(none, rq, np.where(tie, ord("!"), 33 + np.minimum(top - second, cap_q)))
        err = np.where(none | tie, 0, nv - np.take_along_axis(n, win[:, :, None], axis=2)[:, :, 0])
        errors[c0:c1] = err.sum(axis=1)
        sm["bases_changed"] += int((ob[c0:c1] != rb).sum())
        sm["votes"] += int(nv.sum())
        sm["errors"] += int(err.sum())
    return dict(out_off=np.arange(C + 1, dtype=np.uint64) * np.uint64(L), bases=ob.reshape(-1), quals=oq.reshape(-1),
                depth=depth.astype(np.uint32), errors=errors, summary=sm)


def assert_same(a, b, what=""):
    for k in ("out_off", "bases", "quals", "depth", "errors"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, "%s: %s has shapes %r and %r" % (what, k, x.shape, y.shape)
        if not np.array_equal(x, y):
            i = int(np.flatnonzero(x != y)[0])
            raise AssertionError("%s: %s differs first at %d: %r != %r (%d places)" % (what, k, i, x[i], y[i],
                                                                                        np.count_nonzero(x != y)))
    sa, sb = a["summary"], b["summary"]
    assert {k: int(sa[k]) for k in KEYS} == {k: int(sb[k]) for k in KEYS}, "%s: summaries %r != %r" % (what, sa, sb)


def random_reads(rng, cid, lengths, p_err=0.02, p_n=0.01, p_lower=0.005, q_lo=2, q_hi=41, odd_quals=False):
    """Reads for the given cluster ids: one random template per cluster (as long as the longest length), every read a
    copy of its cluster's template cut to its length with substitutions at rate p_err, some N and some lowercase
    bytes; qualities uniform in [q_lo, q_hi] (Phred), with odd_quals also bytes below 33 and above 126.
    Returns (bases, quals, off)."""
    cid, lengths = np.asarray(cid, np.int64), np.asarray(lengths, np.int64)
    lmax = int(lengths.max(initial=0))
    acgt = np.frombuffer(ACGT, np.uint8)
    tmpl = acgt[rng.integers(0, 4, (int(cid.max(initial=0)) + 1, max(lmax, 1)))]
    off = np.zeros(len(cid) + 1, np.uint64)
    off[1:] = np.cumsum(lengths, dtype=np.uint64)
    read = np.repeat(np.arange(len(cid)), lengths)
    col = np.arange(int(lengths.sum())) - np.repeat(off[:-1].astype(np.int64), lengths)
    b = tmpl[cid[read], col].copy()
    m = len(b)
    u = rng.random(m)                                                  # one draw decides what happens to a byte
    sub = u < p_err
    b[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    b[(u >= p_err) & (u < p_err + p_n)] = ord("N")
    b[(u >= p_err + p_n) & (u < p_err + p_n + p_lower)] |= 0x20
    q = (33 + rng.integers(q_lo, q_hi + 1, m, dtype=np.uint8)).astype(np.uint8)
    if odd_quals:
        odd = rng.random(m) < 0.02
        q[odd] = rng.choice(np.asarray([0, 10, 32, 127, 200, 255], np.uint8), int(odd.sum()))
    return b, q, off
