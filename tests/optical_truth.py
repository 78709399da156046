"""The definition of humid_optical_duplicates (include/humid_hip.h), two independent ways, both pure Python / numpy:
  optical_loop   a literal loop over all pairs of members of a cluster with a Python union-find
  optical_sweep  the members sorted by (cluster, tile, x); position p is compared with p + 1, p + 2, ... as whole
                 arrays while the window lasts; components by repeated minimum-label hooking and pointer jumping
Inputs: cluster_id u32[N] and keep u8[N] of a run, tile / x / y u32[N], the distance D and the cluster count C.  Both
return (optical u8[N], origin u32[N], per_cluster u32[C], summary dict).  Two members are close when they share the
cluster and a tile other than NO_TILE and |dx| <= D and |dy| <= D; the groups are the connected components of close;
the origin of a group is the cluster's kept read when the group holds it, else its smallest read index.
Also: make_positions (positions for a given clustering, with a chosen share of near neighbours), rewrite_headers
(Illumina names for the records of FastQ files, the UMI kept) and parse_name (the CLI's rule for a name, restated)."""
import numpy as np

NO_TILE = 0xffffffff
NO_READ = 0xffffffff
KEYS = ("n_clusters", "members", "duplicates", "optical", "groups", "largest_group")


def _check_input(cid, keep, C):
    """what the device reports as HUMID_E_INVALID"""
    assert int(cid.max(initial=0)) <= C, "an id above C"
    kept = cid[(keep != 0) & (cid != 0)]
    assert len(kept) == C and len(np.unique(kept)) == C, "not one kept read per cluster"


def _finish(n, C, cid, keep, members, comp):
    """members: read indices; comp: a component label per member (any labels).  The outputs from the partition."""
    optical = np.zeros(n, np.uint8)
    origin = np.full(n, NO_READ, np.uint32)
    per_cluster = np.zeros(C, np.uint32)
    summary = dict.fromkeys(KEYS, 0)
    summary["n_clusters"] = C if n else 0
    if n == 0 or C == 0:
        summary["n_clusters"] = 0
        return optical, origin, per_cluster, summary
    _, lab = np.unique(comp, return_inverse=True)
    n_groups = int(lab.max()) + 1 if len(lab) else 0
    vote = np.where(keep[members] != 0, 0, 1).astype(np.int64) << 32 | members.astype(np.int64)
    best = np.full(n_groups, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(best, lab, vote)
    org = (best[lab] & 0xffffffff).astype(np.uint32)
    origin[members] = org
    optical[members] = org != members
    np.add.at(per_cluster, cid[members].astype(np.int64) - 1, optical[members].astype(np.uint32))
    sizes = np.bincount(lab, minlength=n_groups)
    summary.update(members=len(members), duplicates=len(members) - C, optical=int(optical.sum()),
                   groups=int(np.count_nonzero(sizes >= 2)), largest_group=int(sizes.max(initial=0)))
    assert summary["optical"] == int(per_cluster.sum()) == int((sizes - 1).sum())
    return optical, origin, per_cluster, summary


def _arrays(cluster_id, keep, tile, x, y):
    return (np.asarray(cluster_id, np.uint32), np.asarray(keep, np.uint8), np.asarray(tile, np.uint32).astype(np.int64),
            np.asarray(x, np.uint32).astype(np.int64), np.asarray(y, np.uint32).astype(np.int64))


def optical_loop(cluster_id, keep, tile, x, y, D, C):
    cid, keep, tile, x, y = _arrays(cluster_id, keep, tile, x, y)
    n, D = len(cid), int(D)
    if n == 0 or C == 0:
        return _finish(n, C, cid, keep, None, None)
    _check_input(cid, keep, C)
    by_cluster = {}
    for i in range(n):
        if cid[i]:
            by_cluster.setdefault(int(cid[i]), []).append(i)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    tl, xl, yl = tile.tolist(), x.tolist(), y.tolist()
    for reads in by_cluster.values():
        for ai, i in enumerate(reads):
            if tl[i] == NO_TILE:
                continue
            for j in reads[ai + 1:]:
                if tl[j] == tl[i] and abs(xl[i] - xl[j]) <= D and abs(yl[i] - yl[j]) <= D:
                    ri, rj = find(i), find(j)
                    if ri != rj:
                        parent[ri] = rj
    members = np.flatnonzero(cid != 0)
    comp = np.asarray([find(int(i)) for i in members], np.int64)
    return _finish(n, C, cid, keep, members, comp)


def _components(n, a, b):
    """labels of the connected components of the graph over 0 .. n - 1 with the edges (a[k], b[k])"""
    lab = np.arange(n, dtype=np.int64)
    while len(a):
        la, lb = lab[a], lab[b]
        live = la != lb
        a, b, la, lb = a[live], b[live], la[live], lb[live]
        if len(a) == 0:
            break
        lo, hi = np.minimum(la, lb), np.maximum(la, lb)
        np.minimum.at(lab, hi, lo)                                     # the larger label's root hooks below the smaller
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
    return lab


def optical_sweep(cluster_id, keep, tile, x, y, D, C):
    cid, keep, tile, x, y = _arrays(cluster_id, keep, tile, x, y)
    n, D = len(cid), int(D)
    if n == 0 or C == 0:
        return _finish(n, C, cid, keep, None, None)
    _check_input(cid, keep, C)
    members = np.flatnonzero(cid != 0)
    order = members[np.lexsort((x[members], tile[members], cid[members]))]
    sc, st, sx, sy = cid[order].astype(np.int64), tile[order], x[order], y[order]
    m = len(order)
    ea, eb = [], []
    p = np.flatnonzero(st != NO_TILE)
    k = 1
    while len(p):
        p = p[p + k < m]
        q = p + k
        inside = (sc[q] == sc[p]) & (st[q] == st[p]) & (sx[q] - sx[p] <= D)
        p, q = p[inside], q[inside]
        near = np.abs(sy[q] - sy[p]) <= D
        ea.append(p[near])
        eb.append(q[near])
        k += 1
    a = np.concatenate(ea) if ea else np.zeros(0, np.int64)
    b = np.concatenate(eb) if eb else np.zeros(0, np.int64)
    comp = _components(m, a, b)
    return _finish(n, C, cid, keep, order, comp)


def assert_same(a, b, what=""):
    for name, u, v in zip(("optical", "origin", "per_cluster"), a, b):
        u, v = np.asarray(u), np.asarray(v)
        assert u.shape == v.shape and np.array_equal(u.astype(np.int64), v.astype(np.int64)), (what, name)
    assert {k: int(a[3][k]) for k in KEYS} == {k: int(b[3][k]) for k in KEYS}, (what, a[3], b[3])


def truth(cluster_id, keep, tile, x, y, D, C, loop=None):
    """the sweep truth, cross-checked against the all-pairs loop unless a cluster is too large for it (the loop is
    quadratic per cluster in Python: clusters up to 1500 reads take it, about a second)"""
    t = optical_sweep(cluster_id, keep, tile, x, y, D, C)
    if loop is None:
        cid = np.asarray(cluster_id, np.uint32)
        sizes = np.bincount(cid[cid != 0]) if len(cid) else np.zeros(1, np.int64)
        loop = int((sizes.astype(np.int64) ** 2).sum()) <= 3_000_000
    if loop:
        assert_same(t, optical_loop(cluster_id, keep, tile, x, y, D, C), "the two truths")
    return t


def make_positions(cluster_id, keep, seed, D=100, n_tiles=8, side=20000, p_near=0.3, p_none=0.01, lanes=2):
    """Positions for the reads of a clustering: every member draws a tile (lane << 24 | 1101 + k over n_tiles tiles
    of `lanes` lanes) and a point of a side x side square; with probability p_near it then moves to within D / 2 of
    the first point of a random read of its own cluster (same tile), so that about that share of the duplicates is
    optical; with probability p_none it has no position.  Reads with cluster_id == 0 get positions like everybody
    else (nothing may depend on them).  Returns tile, x, y (u32[N])."""
    cid = np.asarray(cluster_id, np.uint32)
    n = len(cid)
    rng = np.random.default_rng(seed)
    k = rng.integers(0, n_tiles, n)
    tile = (((k % lanes) + 1) << 24 | (1101 + k // lanes)).astype(np.int64)
    x = rng.integers(0, side, n)
    y = rng.integers(0, side, n)
    order = np.argsort(cid, kind="stable")
    sc = cid[order]
    start = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]]) if n else np.zeros(0, np.int64)
    size = np.diff(np.r_[start, n])
    first = np.repeat(start, size)
    partner = order[first + (rng.random(n) * np.repeat(size, size)).astype(np.int64)]   # by sorted place
    near = np.zeros(n, bool)
    near[order] = (rng.random(n) < p_near) & (sc != 0)
    pick = np.zeros(n, np.int64)
    pick[order] = partner
    jx = rng.integers(-(D // 2), D // 2 + 1, n)
    jy = rng.integers(-(D // 2), D // 2 + 1, n)
    tile = np.where(near, tile[pick], tile)
    nx = np.where(near, np.maximum(x[pick] + jx, 0), x)
    ny = np.where(near, np.maximum(y[pick] + jy, 0), y)
    tile = np.where(rng.random(n) < p_none, NO_TILE, tile)
    return tile.astype(np.uint32), nx.astype(np.uint32), ny.astype(np.uint32)


def parse_name(header):
    """(tile, x, y) of a FastQ header line by the rule of `humid -O`: the text before the first space split on ':';
    fields 4 .. 7 are lane, tile, x, y; lane, tile and x all digits, y the digits its field starts with; lane < 255,
    tile < 2^24, x and y below 2^32; anything else: no position"""
    none = (NO_TILE, 0, 0)
    f = header.split(" ")[0].split(":")
    if len(f) < 7:
        return none
    lane, tl, fx, fy = f[3:7]
    ny = 0
    while ny < len(fy) and fy[ny] in "0123456789":
        ny += 1
    fy = fy[:ny]
    for s in (lane, tl, fx, fy):
        if not s or any(ch not in "0123456789" for ch in s):
            return none
    lane, tl, fx, fy = int(lane), int(tl), int(fx), int(fy)
    if lane >= 255 or tl >= 1 << 24 or fx >= 1 << 32 or fy >= 1 << 32:
        return none
    return (lane << 24 | tl, fx, fy)


def rewrite_headers(files, seed, style="_", side=600, n_tiles=4, p_none=0.02):
    """Gives the records of the FastQ files Illumina names (in place): record i of every file becomes
    @M01:7:FC1:<lane>:<tile>:<x>:<y> followed by what its name carried behind the read number -- the UMI with its
    separator (`style` "_" or ":": it must be the files' own) and the text after the first space.  A share p_none of
    the records gets a name of five fields instead (no position).  Positions are uniform over n_tiles tiles of 2
    lanes and a side x side square.  Returns what was written, tile, x, y (u32[N], NO_TILE where there is none)."""
    rng = np.random.default_rng(seed)
    out = None
    for path in files:
        lines = open(path, "rb").read().split(b"\n")[:-1]
        n = len(lines) // 4
        if out is None:
            k = rng.integers(0, n_tiles, n)
            lane, tl = (k % 2) + 1, 1101 + k // 2
            x, y = rng.integers(0, side, n), rng.integers(0, side, n)
            none = rng.random(n) < p_none
            out = (np.where(none, NO_TILE, lane << 24 | tl).astype(np.uint32), np.where(none, 0, x).astype(np.uint32),
                   np.where(none, 0, y).astype(np.uint32))
        for i in range(min(n, len(out[0]))):
            old = lines[4 * i].decode()
            name, _, rest = old.partition(" ")
            cut = name.find(style, 1)
            tail = name[cut:] if cut >= 0 else ""                       # separator + UMI ("" without one)
            new = "@M01:7:FC1" if none[i] else "@M01:7:FC1:%d:%d:%d:%d" % (lane[i], tl[i], x[i], y[i])
            if none[i]:
                new += ":%d:%d" % (lane[i], tl[i])                      # five fields
            lines[4 * i] = (new + tail + (" " + rest if rest else "")).encode()
        open(path, "wb").write(b"\n".join(lines) + b"\n")
    return out
