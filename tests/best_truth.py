"""The definition of humid_select_best (include/humid_hip.h), two independent ways, both pure Python / numpy:
  select_loop  a loop over the reads with one dict entry per cluster
  select_sort  one whole-array lexsort over (cluster_id, -score, index)
Inputs: words u64[N] or u64[N, 2], cluster_id u32[N] and keep u8[N] of a run, scores u32[N]; scope 0 = LEAF (the
candidates of a cluster are its reads whose word equals the word of the run's representative), 1 = CLUSTER (all its
reads).  Both return (keep_out u8[N], rep_out u32[N], n_changed)."""
import numpy as np

LEAF, CLUSTER = 0, 1
NO_READ = 0xffffffff


def _word_rows(words, n):
    w = np.ascontiguousarray(words, np.uint64)
    return w.reshape(n, -1) if n else w.reshape(0, 1)


def select_loop(words, cluster_id, keep, scores, scope):
    n = len(cluster_id)
    w = _word_rows(words, n)
    rep = {}
    for i in range(n):
        c = int(cluster_id[i])
        if c and keep[i]:
            assert c not in rep, "two kept reads in cluster %d" % c
            rep[c] = i
    best = {}
    for i in range(n):
        c = int(cluster_id[i])
        if c == 0:
            continue
        r = rep[c]
        if scope == LEAF and tuple(w[i]) != tuple(w[r]):
            continue
        s = int(scores[i])
        if c not in best or s > best[c][0]:                            # (ascending i: the first of equal scores stays)
            best[c] = (s, i)
    keep_out = np.zeros(n, np.uint8)
    rep_out = np.full(n, NO_READ, np.uint32)
    for i in range(n):
        c = int(cluster_id[i])
        if c:
            rep_out[i] = best[c][1]
            keep_out[i] = best[c][1] == i
    return keep_out, rep_out, sum(1 for c in rep if best[c][1] != rep[c])


def select_sort(words, cluster_id, keep, scores, scope):
    cid = np.asarray(cluster_id, np.uint32)
    n = len(cid)
    w = _word_rows(words, n)
    keep = np.asarray(keep, np.uint8)
    sc = np.asarray(scores, np.uint32).astype(np.int64)
    n_cl = int(cid.max()) if n else 0
    kept = np.flatnonzero((keep != 0) & (cid != 0))
    old = np.full(n_cl + 1, -1, np.int64)
    old[cid[kept]] = kept
    assert len(kept) == n_cl and np.all(old[1:] >= 0), "not one kept read per cluster"
    cand = cid != 0
    if scope == LEAF and n:
        cand &= np.all(w == w[old[cid]], axis=1)                       # (old[0] = -1: any row; masked by cid != 0)
    idx = np.flatnonzero(cand)
    order = idx[np.lexsort((idx, -sc[idx], cid[idx]))]
    first = np.ones(len(order), bool)
    first[1:] = cid[order[1:]] != cid[order[:-1]]
    new = np.full(n_cl + 1, NO_READ, np.int64)
    new[cid[order[first]]] = order[first]
    rep_out = new[cid].astype(np.uint32)
    rep_out[cid == 0] = NO_READ
    keep_out = (rep_out == np.arange(n, dtype=np.uint32)).astype(np.uint8)
    return keep_out, rep_out, int(np.count_nonzero(new[1:] != old[1:]))


def assert_same(a, b, what=""):
    for name, x, y in zip(("keep_out", "rep_out"), a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), (what, name)
    assert int(a[2]) == int(b[2]), (what, "n_changed", a[2], b[2])


def phred_score(quals):
    """Picard's SUM_OF_BASE_QUALITIES over the quality lines (bytes) of one record: q = byte - 33, summed for q >= 15"""
    t = 0
    for q in quals:
        a = np.frombuffer(q, np.uint8).astype(np.int64) - 33
        t += int(a[a >= 15].sum())
    return t


def rewrite_qualities(files, seed):
    """Gives every record of the FastQ files random Phred qualities 2 .. 41 in place of the generator's constant ones
    (in place); returns the records' scores u32[N] over all files, N = the shortest file's records"""
    rng = np.random.default_rng(seed)
    per_file = []
    for path in files:
        lines = open(path, "rb").read().split(b"\n")[:-1]
        sc = []
        for i in range(3, len(lines), 4):
            q = (rng.integers(2, 42, len(lines[i])) + 33).astype(np.uint8).tobytes()
            lines[i] = q
            sc.append(phred_score([q]))
        open(path, "wb").write(b"\n".join(lines) + b"\n")
        per_file.append(sc)
    n = min(len(s) for s in per_file)
    return np.asarray([sum(s[i] for s in per_file) for i in range(n)], np.uint32)
