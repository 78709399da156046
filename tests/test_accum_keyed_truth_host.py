"""tests/accum_keyed_truth.py on hand-made cases (CPU only): the helper the GPU tests of keyed accumulated runs trust."""
import numpy as np

from accum_keyed_truth import keyed_expected, keyed_leaves

U64 = np.uint64
TOP = 2 ** 64 - 1


def chunk(words, keys, filtered, base):
    return (np.asarray(words, U64), np.asarray(keys, U64), np.asarray(filtered, np.uint8), base)


def test_the_same_word_under_two_keys_by_hand():
    """4-nt words.  In global order:
         index  key   word  filtered
         0      5     0x00
         1      9     0x00             the same word under another key: an entry and a cluster of its own
         2      5     0x01             one substitution from 0x00, once: joins the cluster of (5, 0x00), read twice
         3      5     0x00
         4      TOP   0x01  yes        a garbage key on a filtered read: no group
         5      9     0x00
    fed as two chunks, the later reads first."""
    chunks = [chunk([0x00, 0x01, 0x00], [5, TOP, 9], [0, 1, 0], 3), chunk([0x00, 0x00, 0x01], [5, 9, 5], [0, 0, 0], 0)]
    lv = keyed_leaves(chunks)
    assert lv["key"].tolist() == [5, 5, 9] and lv["word"].tolist() == [0, 1, 0]
    assert lv["count"].tolist() == [2, 1, 2] and lv["first"].tolist() == [0, 2, 1]
    for method in (0, 1):
        res, s, t = keyed_expected(chunks, 4, 1, method)
        assert [r[0].tolist() for r in res] == [[1, 0, 2], [1, 2, 1]]
        assert [r[1].tolist() for r in res] == [[0, 0, 0], [1, 1, 0]]
        assert s == dict(total=6, usable=5, unique=3, clusters=2, edges=1)
        assert t["keys"].tolist() == [5, 9] and t["leaves"]["group"].tolist() == [0, 0, 1]
    # distance 0: (5, 0x01) is a cluster of its own, between the two others in (key, word) order
    res, s, _ = keyed_expected(chunks, 4, 0, 0)
    assert [r[0].tolist() for r in res] == [[1, 0, 3], [1, 3, 2]]
    assert [r[1].tolist() for r in res] == [[0, 0, 0], [1, 1, 1]]
    assert s == dict(total=6, usable=5, unique=3, clusters=3, edges=0)


def test_keys_order_unsigned_and_the_order_of_the_chunks_does_not_matter():
    keys = [1 << 63, 0, TOP, (1 << 63) | 1, 1, 0]
    a = chunk([7, 7, 7], keys[:3], [0, 0, 0], 10)
    b = chunk([7, 7, 7], keys[3:], [0, 0, 0], 100)
    lv = keyed_leaves([a, b])
    assert lv["key"].tolist() == [0, 1, 1 << 63, (1 << 63) | 1, TOP]
    assert lv["count"].tolist() == [2, 1, 1, 1, 1] and lv["first"].tolist() == [11, 101, 10, 100, 12]
    lv2 = keyed_leaves([b, a])
    assert all(np.array_equal(lv[k], lv2[k]) for k in lv)
    r1, s1, _ = keyed_expected([a, b], 4)
    r2, s2, _ = keyed_expected([b, a], 4)
    assert s1 == s2 and s1["clusters"] == 5
    assert r1[0][0].tolist() == [3, 1, 5] and r1[1][0].tolist() == [4, 2, 1]
    assert r1[0][1].tolist() == [1, 1, 1] and r1[1][1].tolist() == [1, 1, 0]       # (0, 7): index 11 is the first, 102 is not
    assert np.array_equal(r1[0][0], r2[1][0]) and np.array_equal(r1[1][1], r2[0][1])


def test_against_a_dictionary():
    rng = np.random.default_rng(5)
    n = 400
    w = rng.integers(0, 16, n).astype(U64)
    k = rng.integers(0, 6, n).astype(U64)
    f = (rng.random(n) < 0.1).astype(np.uint8)
    chunks = [chunk(w[:150], k[:150], f[:150], 1000), chunk(w[150:], k[150:], f[150:], 0), chunk([], [], [], 7)]
    want = {}
    for (ws, ks, fs, base) in chunks:
        for i in range(len(fs)):
            if not fs[i]:
                c, first = want.get((int(ks[i]), int(ws[i])), (0, 1 << 70))
                want[(int(ks[i]), int(ws[i]))] = (c + 1, min(first, base + i))
    lv = keyed_leaves(chunks)
    rows = sorted(want)
    assert list(zip(lv["key"].tolist(), lv["word"].tolist())) == rows
    assert lv["count"].tolist() == [want[r][0] for r in rows] and lv["first"].tolist() == [want[r][1] for r in rows]
    res, s, t = keyed_expected(chunks, 2, 0, 0)                       # distance 0: one cluster per entry, ids in list order
    ids = {r: i + 1 for i, r in enumerate(rows)}
    for (ws, ks, fs, base), (cid, keep) in zip(chunks, res):
        for i in range(len(fs)):
            r = (int(ks[i]), int(ws[i]))
            assert cid[i] == (0 if fs[i] else ids[r])
            assert keep[i] == (0 if fs[i] else int(want[r][1] == base + i))
    assert s["unique"] == s["clusters"] == len(rows) and s["total"] == n
