"""Host-side mirror of the reference surface for the hot path, over the C ABI.

Names follow the reference (/root/reference/src/humid.cc, src/cluster.h):
  Dedup.run(words, filtered)            readData + findHammingNeighbours + findClusters +
                                        the writeFiltered/writeAnnotated lookups
  Dedup.leaves()/adjacency()/clusters() what Trie::walk() / NLeaf / Cluster expose
  ClusterGraph                          NLeaf graphs built with link() (tests/test_cluster.cc)
  at_least_double                       src/cluster.cc:31-33
Everything executes in libhumid_hip.so on the GPU; a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

DIRECTIONAL = 0
MAXIMUM = 1

# which reads of a cluster Dedup.select_best chooses among (include/humid_hip.h, HUMID_BEST_*); rep of a read without a cluster
BEST_LEAF, BEST_CLUSTER = 0, 1
NO_READ = 0xffffffff
NO_TILE = 0xffffffff   # tile of a read without a position (HUMID_NO_TILE, Dedup.optical_duplicates)
_BEST_SCOPES = {"leaf": BEST_LEAF, "cluster": BEST_CLUSTER, BEST_LEAF: BEST_LEAF, BEST_CLUSTER: BEST_CLUSTER}

# strand of a read in a strand-symmetric run (include/humid_hip.h, HUMID_STRAND_*)
STRAND_TOP, STRAND_BOTTOM, STRAND_NONE = 0, 1, 2

# per-read status of the barcode correction (include/humid_hip.h, HUMID_BC_*); also the index into its five counts
BC_FILTERED, BC_EXACT, BC_CORRECTED, BC_AMBIGUOUS, BC_UNMATCHED = range(5)

# how Dedup.discover_whitelist selects the cells (include/humid_hip.h, HUMID_CELLS_*)
CELLS_TOP, CELLS_EXPECTED, CELLS_MIN_READS = 0, 1, 2


class HumidError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("humid_hip error %d: %s" % (code, msg))
        self.code = code


def _vp(a):
    if a is None:
        return None
    return C.c_void_p(a.ctypes.data)


def _keys_u64(keys, shape, what="keys"):
    """integers of at most 64 bits, not negative, of the given shape (None: any one-dimensional) -> contiguous u64"""
    k = np.asarray(keys)
    if k.dtype.kind not in "ui" or k.dtype.itemsize > 8 or (k.shape != shape if shape is not None else k.ndim != 1):
        raise ValueError("%s must be integers of at most 64 bits with shape %r" % (what, shape if shape is not None else "(n,)"))
    if k.dtype.kind == "i" and len(k) and int(k.min()) < 0:
        raise ValueError("%s must not be negative" % what)
    return np.ascontiguousarray(k, dtype=np.uint64)


class Context:
    """Owns a humid_ctx (device workspace + stream)."""

    def __init__(self, device: int = -1, stream: int | None = None):
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.humid_ctx_create(C.byref(h), device, C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise HumidError(rc, self._lib.humid_last_error(None).decode())
        self._h = h

    def set_option(self, key: str, value: int):
        """tuning knobs of include/humid_hip.h (humid_ctx_set_option); never change results"""
        self._check(self._lib.humid_ctx_set_option(self._h, key.encode(), int(value)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.humid_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise HumidError(rc, self._lib.humid_last_error(self._h).decode())


class Dedup(Context):
    """The whole hot path on one GPU."""

    def run(self, words, filtered, word_nt=24, distance=1, method=DIRECTIONAL, edit=False):
        """Host numpy buffers in, (cluster_id u32[N], keep u8[N], summary dict) out.
        edit: neighbours under Levenshtein instead of Hamming distance (the reference's -e).

        word_nt <= 32: words is u64[N].  33 <= word_nt <= 64: words is u64[N, 2], [:, 0] = the
        first word_nt-32 nucleotides, [:, 1] = the last 32 (include/humid_hip.h)."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        want = (len(f), 2) if word_nt > 32 else (len(f),)
        if f.ndim != 1 or w.shape != want:
            raise ValueError("words must have shape %r for word_nt=%d (filtered: %r)" % (want, word_nt, f.shape))
        n = len(f)
        self._wide = word_nt > 32
        self.set_option("edit_distance", int(bool(edit)))
        cid = np.zeros(n, dtype=np.uint32)
        keep = np.zeros(n, dtype=np.uint8)
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run(self._h, _vp(w), _vp(f), n, word_nt, distance, method,
                                              _vp(cid), _vp(keep), C.byref(s)))
        self.summary = s.asdict()
        return cid, keep, self.summary

    def run_bases(self, bases, word_nt=24, distance=1, method=DIRECTIONAL, edit=False):
        """bases: uint8[N, word_nt] -- the symbols of every record as the ASCII of the FastQ (what
        getNucleotides, src/fastq.cc:116-144, assembles); the words are packed on the device.
        Returns (cluster_id, keep, summary) like run()."""
        b = np.ascontiguousarray(bases, dtype=np.uint8)
        if b.ndim != 2 or b.shape[1] != word_nt:
            raise ValueError("bases must have shape (N, %d)" % word_nt)
        n = b.shape[0]
        self._wide = word_nt > 32
        self.set_option("edit_distance", int(bool(edit)))
        cid = np.zeros(n, dtype=np.uint32)
        keep = np.zeros(n, dtype=np.uint8)
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_bases(self._h, _vp(b), n, word_nt, distance, method, _vp(cid),
                                                    _vp(keep), C.byref(s)))
        self.summary = s.asdict()
        return cid, keep, self.summary

    def packed_words(self):
        """words and filtered flags the device packed in the last run_bases()"""
        n = int(self.summary["total"])
        w = np.zeros((n, 2) if getattr(self, "_wide", False) else n, np.uint64)
        f = np.zeros(n, np.uint8)
        self._check(self._lib.humid_get_packed_words(self._h, _vp(w), _vp(f)))
        return w, f

    def run_device(self, d_words, d_filtered, d_cluster_id, d_keep, n_reads, word_nt=24,
                   distance=1, method=DIRECTIONAL):
        """Device pointers (ints, e.g. tensor.data_ptr()); results stay in HBM."""
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_filtered), n_reads, word_nt, distance,
            method, C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.byref(s)))
        self.summary = s.asdict()
        self._wide = word_nt > 32
        return self.summary

    def run_long(self, words, filtered, word_nt, distance=1, method=DIRECTIONAL):
        """Words of 1 .. 512 nucleotides (include/humid_hip.h, humid_dedup_run_long): words is u64[N, k] with
        k = ceil(word_nt / 32), [:, 0] = the first word_nt - 32 (k - 1) nucleotides right-aligned (bits above them are
        ignored), every following column the next 32; a one-dimensional array is accepted for k = 1.  Hamming
        neighbours only.  Returns (cluster_id, keep, summary) like run(); leaves()["word"] is then u64[U, k], and
        long_info() says what the search did.  Up to 64 nucleotides the results are those of run()."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        k = (int(word_nt) + 31) // 32
        if w.ndim == 1 and k == 1:
            w = w.reshape(-1, 1)
        if f.ndim != 1 or (k >= 1 and w.shape != (len(f), k)):
            raise ValueError("words must have shape %r for word_nt=%d (filtered: %r)" % ((len(f), k), word_nt, f.shape))
        n = len(f)
        cid = np.zeros(n, dtype=np.uint32)
        keep = np.zeros(n, dtype=np.uint8)
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_long(self._h, _vp(w), _vp(f), n, word_nt, distance, method,
                                                   _vp(cid), _vp(keep), C.byref(s)))
        self.summary = self._long_summary = s.asdict()
        self._long_k = k
        return cid, keep, self.summary

    def run_long_device(self, d_words, d_filtered, d_cluster_id, d_keep, n_reads, word_nt, distance=1,
                        method=DIRECTIONAL):
        """run_long() over device pointers (ints; the words need 8-byte alignment only); results stay in HBM."""
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_long_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_filtered), n_reads, word_nt, distance, method,
            C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.byref(s)))
        self.summary = self._long_summary = s.asdict()
        self._long_k = (int(word_nt) + 31) // 32
        return self.summary

    def long_info(self):
        """what the last long run's search did (humid_long_info): dict(words_per_read, joins, key_bits, piece_joins,
        candidates, raw_edges, edges)"""
        info = _lib.HumidLongInfo()
        self._check(self._lib.humid_long_info(self._h, C.byref(info)))
        return info.asdict()

    def run_grouped(self, words, groups, filtered, word_nt=24, n_groups=None, distance=1, method=DIRECTIONAL,
                    edit=False):
        """Deduplicate within groups (include/humid_hip.h, humid_dedup_run_grouped): the results are those of
        run() on every group's reads on their own, ids of group g raised by the clusters of the groups below it.
        groups: u32[N] (None: all reads in group 0); n_groups None: groups[filtered == 0].max() + 1.
        Returns (cluster_id, keep, summary) like run(); leaves() then also gives every leaf's "group"."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        want = (len(f), 2) if word_nt > 32 else (len(f),)
        if f.ndim != 1 or w.shape != want:
            raise ValueError("words must have shape %r for word_nt=%d (filtered: %r)" % (want, word_nt, f.shape))
        g = None
        if groups is not None:
            g = np.ascontiguousarray(groups, dtype=np.uint32)
            if g.shape != f.shape:
                raise ValueError("groups must have shape %r" % (f.shape,))
        if n_groups is None:
            usable = g[f == 0] if g is not None else np.zeros(0, np.uint32)
            n_groups = int(usable.max()) + 1 if len(usable) else 1
        n = len(f)
        self._wide = word_nt > 32
        self.set_option("edit_distance", int(bool(edit)))
        cid = np.zeros(n, dtype=np.uint32)
        keep = np.zeros(n, dtype=np.uint8)
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_grouped(self._h, _vp(w), _vp(g), _vp(f), n, word_nt, n_groups,
                                                      distance, method, _vp(cid), _vp(keep), C.byref(s)))
        self.summary = self._grouped_summary = s.asdict()
        return cid, keep, self.summary

    def run_grouped_device(self, d_words, d_groups, d_filtered, d_cluster_id, d_keep, n_reads, n_groups,
                           word_nt=24, distance=1, method=DIRECTIONAL):
        """run_grouped on device pointers (ints, e.g. tensor.data_ptr(); d_groups u32, 0 for none); results stay
        in HBM.  n_groups is required here."""
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_grouped_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_groups) if d_groups else None, C.c_void_p(d_filtered),
            n_reads, word_nt, n_groups, distance, method, C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.byref(s)))
        self.summary = self._grouped_summary = s.asdict()
        self._wide = word_nt > 32
        return self.summary

    def _barcode_quals(self, quals, n):
        """u8[N, K] Phred+33 bytes of the barcodes, K that of the whitelist now set"""
        q = np.asarray(quals)
        if q.dtype != np.uint8 or q.ndim != 2 or q.shape[0] != n:
            raise ValueError("barcode qualities must be uint8 of shape (%d, K)" % n)
        k = self.whitelist_info()["barcode_nt"]
        if k and q.shape[1] != k:                               # (no whitelist: the library refuses the call)
            raise ValueError("barcode qualities must be uint8 of shape %r" % ((n, k),))
        return np.ascontiguousarray(q)

    @staticmethod
    def _min_odds(min_odds):
        if not 1 <= int(min_odds) < 1 << 32:
            raise ValueError("min_odds must be 1 .. 2**32 - 1")
        return int(min_odds)

    def run_keyed(self, words, keys, filtered, word_nt=24, distance=1, method=DIRECTIONAL, edit=False, correct=False,
                  barcode_quals=None, min_odds=39):
        """Deduplicate within groups given by arbitrary 64-bit keys (include/humid_hip.h, humid_dedup_run_keyed):
        run_grouped with every usable read's group = the rank of its key among the distinct keys of the usable
        reads, ranked on the device.  keys: u64[N]; keys of filtered reads are not read.
        Returns (cluster_id, keep, summary) like run(); leaves() then also gives every leaf's "group" (the rank)
        and "key", and group_keys() the sorted distinct keys.
        correct=True: the keys are corrected against the whitelist of set_whitelist() first and reads whose key is
        ambiguous or unmatched count as filtered (humid_dedup_run_keyed_corrected); barcode_status() then gives
        every read's status.
        barcode_quals (u8[N, K] raw Phred+33 bytes of the barcode's nucleotides, with correct=True only): a key with
        several whitelist barcodes one substitution away goes to the one whose weight (exact reads + 1) * error
        probability of the differing base is at least min_odds times all the others' together, instead of being
        ambiguous (humid_dedup_run_keyed_posterior); barcode_posterior() and whitelist_counts() answer afterwards."""
        if barcode_quals is not None and not correct:
            raise ValueError("barcode_quals needs correct=True")
        w = np.ascontiguousarray(words, dtype=np.uint64)
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        want = (len(f), 2) if word_nt > 32 else (len(f),)
        if f.ndim != 1 or w.shape != want:
            raise ValueError("words must have shape %r for word_nt=%d (filtered: %r)" % (want, word_nt, f.shape))
        k = np.asarray(keys)
        if k.dtype.kind not in "ui" or k.dtype.itemsize > 8 or k.shape != f.shape:
            raise ValueError("keys must be integers of at most 64 bits with shape %r" % (f.shape,))
        if k.dtype.kind == "i" and len(k) and int(k.min()) < 0:
            raise ValueError("keys must not be negative")
        k = np.ascontiguousarray(k, dtype=np.uint64)
        n = len(f)
        if barcode_quals is not None:
            mo = self._min_odds(min_odds)
            q = self._barcode_quals(barcode_quals, n)
        self._wide = word_nt > 32
        self.set_option("edit_distance", int(bool(edit)))
        cid = np.zeros(n, dtype=np.uint32)
        keep = np.zeros(n, dtype=np.uint8)
        s = _lib.HumidSummary()
        if barcode_quals is not None:
            self._check(self._lib.humid_dedup_run_keyed_posterior(self._h, _vp(w), _vp(k), _vp(q), _vp(f), n, word_nt, distance,
                                                                  method, mo, _vp(cid), _vp(keep), C.byref(s)))
            self.summary = self._grouped_summary = self._keyed_summary = s.asdict()
            return cid, keep, self.summary
        fn = self._lib.humid_dedup_run_keyed_corrected if correct else self._lib.humid_dedup_run_keyed
        self._check(fn(self._h, _vp(w), _vp(k), _vp(f), n, word_nt, distance, method, _vp(cid), _vp(keep), C.byref(s)))
        self.summary = self._grouped_summary = self._keyed_summary = s.asdict()
        return cid, keep, self.summary

    def run_keyed_device(self, d_words, d_keys, d_filtered, d_cluster_id, d_keep, n_reads, word_nt=24, distance=1,
                         method=DIRECTIONAL):
        """run_keyed on device pointers (ints, e.g. tensor.data_ptr(); d_keys u64); results stay in HBM."""
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_keyed_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_keys), C.c_void_p(d_filtered), n_reads, word_nt, distance,
            method, C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.byref(s)))
        self.summary = self._grouped_summary = self._keyed_summary = s.asdict()
        self._wide = word_nt > 32
        return self.summary

    def run_keyed_corrected_device(self, d_words, d_keys, d_filtered, d_cluster_id, d_keep, n_reads, word_nt=24,
                                   distance=1, method=DIRECTIONAL):
        """run_keyed(correct=True) on device pointers (ints, e.g. tensor.data_ptr(); d_keys u64); results stay in
        HBM."""
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_keyed_corrected_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_keys), C.c_void_p(d_filtered), n_reads, word_nt, distance,
            method, C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.byref(s)))
        self.summary = self._grouped_summary = self._keyed_summary = s.asdict()
        self._wide = word_nt > 32
        return self.summary

    def run_keyed_posterior_device(self, d_words, d_keys, d_quals, d_filtered, d_cluster_id, d_keep, n_reads, word_nt=24,
                                   distance=1, method=DIRECTIONAL, min_odds=39):
        """run_keyed(correct=True, barcode_quals=...) on device pointers (ints; d_keys u64[N], d_quals u8[N * K]);
        results stay in HBM."""
        s, mo = _lib.HumidSummary(), self._min_odds(min_odds)
        self._check(self._lib.humid_dedup_run_keyed_posterior_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_keys), C.c_void_p(d_quals), C.c_void_p(d_filtered), n_reads, word_nt,
            distance, method, mo, C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.byref(s)))
        self.summary = self._grouped_summary = self._keyed_summary = s.asdict()
        self._wide = word_nt > 32
        return self.summary

    def run_paired(self, words, filtered, word_nt=24, distance=1, method=DIRECTIONAL):
        """Strand-symmetric (duplex) deduplication (include/humid_hip.h, humid_dedup_run_paired): a word A.B and its
        mirror B.A (halves of word_nt / 2 nucleotides exchanged) are one molecule read from its two strands.  The
        leaves are the canonical words min(w, mirror(w)); two leaves u, v are neighbours when
        min(ham(u, v), ham(u, mirror(v))) <= distance.  word_nt must be even.
        Returns (cluster_id, keep, summary) like run(); leaves() gives the canonical words, strands() the strand of
        every read and the reads of each strand per cluster."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        want = (len(f), 2) if word_nt > 32 else (len(f),)
        if f.ndim != 1 or w.shape != want:
            raise ValueError("words must have shape %r for word_nt=%d (filtered: %r)" % (want, word_nt, f.shape))
        n = len(f)
        self._wide = word_nt > 32
        cid = np.zeros(n, dtype=np.uint32)
        keep = np.zeros(n, dtype=np.uint8)
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_paired(self._h, _vp(w), _vp(f), n, word_nt, distance, method,
                                                     _vp(cid), _vp(keep), C.byref(s)))
        self.summary = s.asdict()
        return cid, keep, self.summary

    def run_paired_device(self, d_words, d_filtered, d_cluster_id, d_keep, n_reads, word_nt=24, distance=1,
                          method=DIRECTIONAL):
        """run_paired on device pointers (ints, e.g. tensor.data_ptr()); results stay in HBM."""
        s = _lib.HumidSummary()
        self._check(self._lib.humid_dedup_run_paired_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_filtered), n_reads, word_nt, distance, method,
            C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.byref(s)))
        self.summary = s.asdict()
        self._wide = word_nt > 32
        return self.summary

    def canonical_words(self, words, filtered, word_nt=24):
        """Canonical word and strand of every read without running anything else (humid_paired_canonical): returns
        (words_out like words, strand u8[N] of STRAND_TOP / STRAND_BOTTOM / STRAND_NONE).  A filtered read keeps its
        word.  The results of the last run stay untouched."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        want = (len(f), 2) if word_nt > 32 else (len(f),)
        if f.ndim != 1 or w.shape != want:
            raise ValueError("words must have shape %r for word_nt=%d (filtered: %r)" % (want, word_nt, f.shape))
        out = w.copy()
        strand = np.zeros(len(f), np.uint8)
        self._check(self._lib.humid_paired_canonical(self._h, _vp(out), _vp(f), len(f), word_nt, _vp(out), _vp(strand)))
        return out, strand

    def canonical_words_device(self, d_words, d_filtered, d_words_out, d_strand, n_reads, word_nt=24):
        """canonical_words on device pointers (ints; d_words_out may be d_words)"""
        self._check(self._lib.humid_paired_canonical_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_filtered), n_reads, word_nt, C.c_void_p(d_words_out),
            C.c_void_p(d_strand)))

    def strands(self):
        """after run_paired: (strand u8[N], top u32[C], bottom u32[C], summary dict) -- the strand of every read, the
        reads of each strand of cluster c at [c - 1], and dict(n_clusters, duplex, top_only, bottom_only, top_reads,
        bottom_reads); a cluster is duplex when it has reads of both strands (humid_get_strands)"""
        n, c = int(self.summary["total"]), int(self.summary["clusters"])
        strand, top, bottom = np.zeros(n, np.uint8), np.zeros(c, np.uint32), np.zeros(c, np.uint32)
        sm = _lib.HumidStrandSummary()
        self._check(self._lib.humid_get_strands(self._h, _vp(strand), n, _vp(top), _vp(bottom), C.byref(sm)))
        return strand, top, bottom, sm.asdict()

    def set_whitelist(self, barcodes, barcode_nt=16):
        """The known barcodes (include/humid_hip.h, humid_whitelist_set): integers of at most 64 bits, each a
        barcode_nt-nucleotide word (< 4 ** barcode_nt); duplicates collapse.  None or an empty array clears the
        whitelist.  It stays with this object through any number of runs until it is replaced or cleared."""
        if barcodes is None:
            b = np.zeros(0, np.uint64)
        else:
            b = _keys_u64(barcodes, None, "barcodes")
        if len(b):
            if not 1 <= int(barcode_nt) <= 32:
                raise ValueError("barcode_nt must be 1 .. 32")
            if barcode_nt < 32 and int(b.max()) >= 4 ** int(barcode_nt):
                raise ValueError("a barcode is not a %d-nucleotide word" % barcode_nt)
        self._check(self._lib.humid_whitelist_set(self._h, _vp(b) if len(b) else None, len(b), int(barcode_nt)))

    def whitelist_info(self):
        """dict(n_distinct, barcode_nt, table_log2) of the whitelist (n_distinct = 0: none is set)"""
        n, k, t = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.humid_whitelist_info(self._h, C.byref(n), C.byref(k), C.byref(t)))
        return dict(n_distinct=n.value, barcode_nt=k.value, table_log2=t.value)

    def set_whitelist_segments(self, lists, seg_nt, max_inexact=None):
        """A segmented whitelist (include/humid_hip.h, humid_whitelist_set_segments) for barcodes made of several short
        segments, each with a list of its own (SPLiT-seq, inDrop, BD Rhapsody, sci-RNA-seq): lists[s] holds the known
        values of segment s, integers below 4 ** seg_nt[s]; 1 .. 8 segments of 1 .. 10 nucleotides, 32 at the most
        together.  Segment 0 is the first seg_nt[0] nucleotides of the key.  Every segment is corrected on its own,
        one substitution at the most in each; a read with more than max_inexact (default: all) segments that are not
        exact is unmatched.  It takes the place of the whitelist this object holds and stays until set_whitelist,
        discover_whitelist or another call of this replaces it.  correct_keys and run_keyed(correct=True) then work
        as with any whitelist (not with quals / barcode_quals); barcode_segments() gives the per-segment summary.
        Split-pool data without a cell list composes from this: correct_keys with the segments, discover_whitelist on
        its keys_out (with the reads it left ambiguous or unmatched marked filtered), then run_keyed(correct=True) on
        keys_out against the cells found."""
        nts = [int(x) for x in seg_nt]
        if len(lists) != len(nts) or not 1 <= len(nts) <= 8:
            raise ValueError("1 .. 8 segments, and one length per list")
        ls = [_keys_u64(w, None, "barcodes") for w in lists]
        if max_inexact is None:
            max_inexact = len(nts)
        if not 0 <= int(max_inexact) <= len(nts):
            raise ValueError("max_inexact must be 0 .. the number of segments")
        nt = np.asarray(nts, np.uint32)
        n = np.asarray([len(w) for w in ls], np.uint64)
        b = np.ascontiguousarray(np.concatenate(ls + [np.zeros(1, np.uint64)]))      # (never an empty buffer)
        self._check(self._lib.humid_whitelist_set_segments(self._h, len(nts), _vp(nt), _vp(n), _vp(b), int(max_inexact)))

    def whitelist_segments_info(self):
        """dict(n_seg, seg_nt, seg_n, max_inexact) of the segmented whitelist: the nucleotides and the distinct values
        of every segment (n_seg = 0: the whitelist is a plain one or none is set)"""
        s, m = C.c_uint32(), C.c_uint32()
        nt, n = np.zeros(8, np.uint32), np.zeros(8, np.uint64)
        self._check(self._lib.humid_whitelist_segments_info(self._h, C.byref(s), _vp(nt), _vp(n), C.byref(m)))
        return dict(n_seg=s.value, seg_nt=[int(x) for x in nt[:s.value]], seg_n=[int(x) for x in n[:s.value]],
                    max_inexact=m.value)

    def barcode_segments(self):
        """after correct_keys or run_keyed(correct=True) over a segmented whitelist, whichever came later:
        (seg_counts u64[S, 4], inexact_hist u64[S + 1]): per segment the usable reads whose segment was exact /
        corrected / ambiguous / unmatched, and the reads by their number of segments that were not exact
        (humid_get_barcode_segments)"""
        s = self.whitelist_segments_info()["n_seg"]
        sc, ih = np.zeros((8, 4), np.uint64), np.zeros(9, np.uint64)
        self._check(self._lib.humid_get_barcode_segments(self._h, _vp(sc), _vp(ih)))
        return sc[:s].copy(), ih[:s + 1].copy()

    def correct_keys(self, keys, filtered, quals=None, min_odds=39, prior=False):
        """Correct keys against the whitelist without running anything else (humid_whitelist_correct): returns
        (keys_out u64[N], status u8[N] of BC_FILTERED .. BC_UNMATCHED, counts u64[5] indexed by status).  The
        results of the last run stay untouched.
        quals (u8[N, K] raw Phred+33 bytes of the barcode's nucleotides): ambiguous keys are decided by quality and
        abundance (humid_whitelist_correct_posterior, see run_keyed) and a fourth value is returned, dict(counts,
        multi, rescued): the reads with two or more candidates and those of them that were corrected.
        prior=True (with quals): the abundances are those fed by prior_add, not this call's -- every read gets what
        the correction over ALL reads given to prior_add gives it, the counts are those of this chunk
        (humid_whitelist_correct_posterior_prior)."""
        if prior and quals is None:
            raise ValueError("prior=True needs the barcode qualities (quals)")
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        if f.ndim != 1:
            raise ValueError("filtered must be one-dimensional")
        k = _keys_u64(keys, f.shape)
        n = len(f)
        out, status, counts = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(5, np.uint64)
        if quals is not None:
            mo = self._min_odds(min_odds)
            q, sm = self._barcode_quals(quals, n), _lib.HumidBcPosteriorSummary()
            call = self._lib.humid_whitelist_correct_posterior_prior if prior else self._lib.humid_whitelist_correct_posterior
            self._check(call(self._h, _vp(k), _vp(q), _vp(f), n, mo, _vp(out), _vp(status), C.byref(sm)))
            d = sm.asdict()
            return out, status, np.asarray(d["counts"], np.uint64), d
        self._check(self._lib.humid_whitelist_correct(self._h, _vp(k), _vp(f), n, _vp(out), _vp(status), _vp(counts)))
        return out, status, counts

    def prior_begin(self):
        """Opens the posterior's prior fed in chunks over the whitelist in place (humid_whitelist_prior_begin): reads per
        barcode of its own, zeroed.  It lasts until the whitelist changes."""
        self._check(self._lib.humid_whitelist_prior_begin(self._h))

    def prior_add(self, keys, filtered):
        """adds a chunk's usable reads per whitelist barcode to the prior (humid_whitelist_prior_add)"""
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        if f.ndim != 1:
            raise ValueError("filtered must be one-dimensional")
        k = _keys_u64(keys, f.shape)
        n = len(f)
        self._check(self._lib.humid_whitelist_prior_add(self._h, _vp(k) if n else None, _vp(f) if n else None, n))

    def prior_add_device(self, d_keys, d_filtered, n_reads):
        """the same with integer device pointers"""
        self._check(self._lib.humid_whitelist_prior_add_device(self._h, C.c_void_p(d_keys) if n_reads else None,
                                                               C.c_void_p(d_filtered) if n_reads else None, n_reads))

    def correct_keys_prior_device(self, d_keys, d_quals, d_filtered, d_keys_out, d_status, n_reads, min_odds=39):
        """correct_keys(quals=..., prior=True) on device pointers (ints; d_quals u8[N * K]; d_keys_out u64[N] and d_status
        u8[N] may be 0); returns dict(counts, multi, rescued)"""
        sm, mo = _lib.HumidBcPosteriorSummary(), self._min_odds(min_odds)
        self._check(self._lib.humid_whitelist_correct_posterior_prior_device(
            self._h, C.c_void_p(d_keys), C.c_void_p(d_quals), C.c_void_p(d_filtered), n_reads, mo,
            C.c_void_p(d_keys_out) if d_keys_out else None, C.c_void_p(d_status) if d_status else None, C.byref(sm)))
        return sm.asdict()

    def correct_keys_device(self, d_keys, d_filtered, d_keys_out, d_status, n_reads):
        """correct_keys on device pointers (ints; d_keys_out u64[N] and d_status u8[N] may be 0); returns counts"""
        counts = np.zeros(5, np.uint64)
        self._check(self._lib.humid_whitelist_correct_device(
            self._h, C.c_void_p(d_keys), C.c_void_p(d_filtered), n_reads, C.c_void_p(d_keys_out) if d_keys_out else None,
            C.c_void_p(d_status) if d_status else None, _vp(counts)))
        return counts

    def correct_keys_posterior_device(self, d_keys, d_quals, d_filtered, d_keys_out, d_status, n_reads, min_odds=39):
        """correct_keys(quals=...) on device pointers (ints; d_quals u8[N * K]; d_keys_out u64[N] and d_status u8[N]
        may be 0); returns dict(counts, multi, rescued)"""
        sm, mo = _lib.HumidBcPosteriorSummary(), self._min_odds(min_odds)
        self._check(self._lib.humid_whitelist_correct_posterior_device(
            self._h, C.c_void_p(d_keys), C.c_void_p(d_quals), C.c_void_p(d_filtered), n_reads, mo,
            C.c_void_p(d_keys_out) if d_keys_out else None, C.c_void_p(d_status) if d_status else None, C.byref(sm)))
        return sm.asdict()

    def barcode_posterior(self):
        """after run_keyed(correct=True, barcode_quals=...): dict(multi, rescued) of that run
        (humid_get_barcode_posterior)"""
        m, r = C.c_uint64(), C.c_uint64()
        self._check(self._lib.humid_get_barcode_posterior(self._h, C.byref(m), C.byref(r)))
        return dict(multi=int(m.value), rescued=int(r.value))

    def whitelist_counts(self, barcodes):
        """u32[len(barcodes)]: the usable reads of the last posterior correction (call or run) whose key WAS each of
        the given barcodes, before any correction; 0 for a value the whitelist does not hold
        (humid_whitelist_counts)"""
        b = _keys_u64(barcodes, None, "barcodes")
        out = np.zeros(len(b), np.uint32)
        self._check(self._lib.humid_whitelist_counts(self._h, _vp(b) if len(b) else None, len(b), _vp(out) if len(b) else None))
        return out

    @staticmethod
    def _cells_mode(top, expected, min_reads, merge_ratio):
        """(mode, param, merge_ratio) of discover_whitelist's and BarcodeCounter.finish's arguments"""
        given = [(m, v) for m, v in ((CELLS_TOP, top), (CELLS_EXPECTED, expected), (CELLS_MIN_READS, min_reads)) if v is not None]
        if len(given) != 1:
            raise ValueError("exactly one of top, expected and min_reads must be given")
        mode, param = given[0][0], int(given[0][1])
        merge_ratio = int(merge_ratio)
        if not 1 <= param < 2 ** 64:
            raise ValueError("top, expected and min_reads must be in [1, 2**64)")
        if not 0 <= merge_ratio < 2 ** 32:
            raise ValueError("merge_ratio must be in [0, 2**32)")
        return mode, param, merge_ratio

    def discover_whitelist(self, keys, filtered, barcode_nt=16, top=None, expected=None, min_reads=None, merge_ratio=0):
        """The whitelist taken from the data (include/humid_hip.h, humid_whitelist_discover): the reads per barcode are
        counted on the device, the abundant barcodes are the cells, and they become this object's whitelist as if by
        set_whitelist.  Exactly one of top (the T most abundant), expected (every barcode with at least a tenth of the
        reads of the barcode at rank (expected + 50) // 100) and min_reads (every barcode with that many reads) must be
        given.  merge_ratio R >= 1 removes a selected barcode one substitution away from another with at least R
        times its reads; 0 keeps all.  keys and filtered are numpy arrays, or both torch tensors on this object's device
        (8-byte and 1-byte elements).  Returns the summary as a dict (usable, invalid_reads, distinct, selected, merged,
        cells, threshold_reads, top_reads, reads_in_cells).  The results of the last run stay untouched."""
        mode, param, merge_ratio = self._cells_mode(top, expected, min_reads, merge_ratio)
        if not 1 <= int(barcode_nt) <= 32:
            raise ValueError("barcode_nt must be 1 .. 32")
        sm = _lib.HumidCellsSummary()
        if hasattr(keys, "data_ptr") and hasattr(filtered, "data_ptr"):
            import torch
            n = filtered.numel()
            for a, size in ((keys, 8), (filtered, 1)):
                if not a.is_cuda or not a.is_contiguous() or a.element_size() != size or a.numel() != n or a.dim() != 1:
                    raise ValueError("device tensors must be contiguous, one-dimensional, of %d elements: keys of 8 bytes "
                                     "each, filtered of 1" % n)
            torch.cuda.synchronize(keys.device)
            self._check(self._lib.humid_whitelist_discover_device(
                self._h, C.c_void_p(keys.data_ptr()) if n else None, C.c_void_p(filtered.data_ptr()) if n else None, n,
                int(barcode_nt), mode, param, merge_ratio, C.byref(sm)))
            return sm.asdict()
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        if f.ndim != 1:
            raise ValueError("filtered must be one-dimensional")
        k = _keys_u64(keys, f.shape)
        n = len(f)
        self._check(self._lib.humid_whitelist_discover(self._h, _vp(k) if n else None, _vp(f) if n else None, n, int(barcode_nt),
                                                       mode, param, merge_ratio, C.byref(sm)))
        return sm.asdict()

    def discovered_cells(self):
        """after discover_whitelist: (barcodes u64[cells] ascending, reads u32[cells]), the cells and their reads
        (humid_get_discovered_cells)"""
        n = C.c_uint64()
        self._check(self._lib.humid_get_discovered_cells(self._h, None, None, 0, C.byref(n)))
        b, r = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self._lib.humid_get_discovered_cells(self._h, _vp(b), _vp(r), n.value, C.byref(n)))
        return b, r

    def barcode_count_hist(self):
        """after discover_whitelist: (reads u64[H] ascending, barcodes u64[H]): how many distinct barcodes have exactly
        that many reads, over all barcodes of the call -- the data of a barcode-rank plot
        (humid_get_barcode_count_hist)"""
        n = C.c_uint64()
        self._check(self._lib.humid_get_barcode_count_hist(self._h, None, None, 0, C.byref(n)))
        r, b = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64)
        if n.value:
            self._check(self._lib.humid_get_barcode_count_hist(self._h, _vp(r), _vp(b), n.value, C.byref(n)))
        return r, b

    def barcode_status(self):
        """after run_keyed(correct=True): (status u8[N], counts u64[5]) of that run (humid_get_barcode_status)"""
        n = int(self.summary["total"])
        status, counts = np.zeros(n, np.uint8), np.zeros(5, np.uint64)
        self._check(self._lib.humid_get_barcode_status(self._h, _vp(status), n, _vp(counts)))
        return status, counts

    def select_best(self, words, cluster_id, keep, scores, word_nt=24, scope="leaf", rep=True):
        """After a run: the best-scoring read of every cluster instead of the first one (include/humid_hip.h,
        humid_select_best).  words, cluster_id and keep are that run's words and outputs, scores u32[N], larger is
        better, ties to the smallest read index.  scope "leaf" (BEST_LEAF): among the reads that carry the word of the
        run's representative; "cluster" (BEST_CLUSTER): among all reads of the cluster.
        Returns (keep_out u8[N], rep u32[N], n_changed): rep[i] is the representative of read i's cluster (NO_READ
        for cluster_id == 0; None with rep=False), n_changed the number of clusters whose representative changed."""
        if scope not in _BEST_SCOPES:
            raise ValueError('scope must be "leaf" or "cluster"')
        cid = np.ascontiguousarray(cluster_id, dtype=np.uint32)
        n = len(cid)
        w = np.ascontiguousarray(words, dtype=np.uint64)
        k = np.ascontiguousarray(keep, dtype=np.uint8)
        sc = np.asarray(scores)
        if sc.dtype.kind not in "ui" or sc.shape != (n,) or (n and (int(sc.min()) < 0 or int(sc.max()) > 0xffffffff)):
            raise ValueError("scores must be integers in [0, 2**32) with shape (%d,)" % n)
        sc = np.ascontiguousarray(sc, dtype=np.uint32)
        want = (n, 2) if word_nt > 32 else (n,)
        if cid.ndim != 1 or w.shape != want or k.shape != (n,):
            raise ValueError("words must have shape %r for word_nt=%d, keep %r" % (want, word_nt, (n,)))
        keep_out = np.zeros(n, np.uint8)
        rep_out = np.zeros(n, np.uint32) if rep else None
        changed = C.c_uint64()
        self._check(self._lib.humid_select_best(self._h, _vp(w), _vp(cid), _vp(k), _vp(sc), n, word_nt, _BEST_SCOPES[scope],
                                                _vp(keep_out), _vp(rep_out), C.byref(changed)))
        return keep_out, rep_out, changed.value

    def select_best_device(self, d_words, d_cluster_id, d_keep, d_scores, d_keep_out, d_rep_out, n_reads, word_nt=24,
                           scope="leaf"):
        """select_best on device pointers (ints, e.g. tensor.data_ptr(); d_rep_out may be 0, d_keep_out may be
        d_keep); results stay in HBM.  Returns n_changed."""
        if scope not in _BEST_SCOPES:
            raise ValueError('scope must be "leaf" or "cluster"')
        changed = C.c_uint64()
        self._check(self._lib.humid_select_best_device(
            self._h, C.c_void_p(d_words), C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.c_void_p(d_scores), n_reads,
            word_nt, _BEST_SCOPES[scope], C.c_void_p(d_keep_out), C.c_void_p(d_rep_out) if d_rep_out else None,
            C.byref(changed)))
        return changed.value

    def consensus(self, bases, quals, cluster_id, keep, off=None, n_clusters=None, min_q=10, cap_q=93):
        """One consensus record per cluster from all of its reads (include/humid_hip.h, humid_consensus): per column
        every read votes for its base (A C G T, quality >= max(min_q, 1)) with the weight of its Phred quality; the
        output is the base with the largest sum and 33 + min(margin to the second, cap_q) as quality, 'N' / '!' on a
        tie, the representative's own bytes where nobody voted.  bases / quals: u8[N, L] matrices (off is implied) or
        flat ASCII blobs with off u64[N + 1]; cluster_id / keep from any run (keep possibly from select_best); one
        call per FastQ file.  n_clusters defaults to cluster_id.max().
        Returns dict(out_off u64[C + 1], bases u8[total], quals u8[total], depth u32[C], errors u64[C], summary):
        the consensus of cluster c is bytes [out_off[c - 1], out_off[c]) of bases and quals."""
        cid = np.ascontiguousarray(cluster_id, dtype=np.uint32)
        n = len(cid)
        k = np.ascontiguousarray(keep, dtype=np.uint8)
        b = np.ascontiguousarray(bases, dtype=np.uint8)
        q = np.ascontiguousarray(quals, dtype=np.uint8)
        if cid.ndim != 1 or k.shape != (n,) or b.shape != q.shape:
            raise ValueError("cluster_id and keep must have shape (N,), bases and quals the same shape")
        if off is None:
            if b.ndim != 2 or b.shape[0] != n:
                raise ValueError("without off, bases and quals must be u8[N, L] matrices")
            o = np.arange(n + 1, dtype=np.uint64) * np.uint64(b.shape[1])
        else:
            o = np.ascontiguousarray(off, dtype=np.uint64)
            if b.ndim != 1 or o.shape != (n + 1,):
                raise ValueError("with off, bases and quals must be flat blobs and off u64[N + 1]")
        if n_clusters is None:
            n_clusters = int(cid.max()) if n else 0
        sm = _lib.HumidConsensusSummary()
        self._check(self._lib.humid_consensus(self._h, _vp(b), _vp(q), _vp(o), b.size, _vp(cid), _vp(k), n, int(n_clusters),
                                              int(min_q), int(cap_q), C.byref(sm)))
        return self._consensus_result(sm.asdict())

    def _consensus_result(self, sm):
        c, t = sm["n_clusters"], sm["total_bytes"]
        out = dict(out_off=np.zeros(c + 1, np.uint64), bases=np.zeros(t, np.uint8), quals=np.zeros(t, np.uint8),
                   depth=np.zeros(c, np.uint32), errors=np.zeros(c, np.uint64), summary=sm)
        self._check(self._lib.humid_get_consensus(self._h, t, _vp(out["out_off"]), _vp(out["bases"]), _vp(out["quals"]),
                                                  _vp(out["depth"]), _vp(out["errors"])))
        return out

    def consensus_device(self, d_bases, d_quals, d_off, n_bytes, d_cluster_id, d_keep, n_reads, n_clusters, min_q=10,
                         cap_q=93):
        """consensus on device pointers (ints, e.g. tensor.data_ptr()); the results stay in HBM
        (consensus_result_device).  Returns the summary dict."""
        sm = _lib.HumidConsensusSummary()
        self._check(self._lib.humid_consensus_device(
            self._h, C.c_void_p(d_bases), C.c_void_p(d_quals), C.c_void_p(d_off), n_bytes, C.c_void_p(d_cluster_id),
            C.c_void_p(d_keep), n_reads, n_clusters, int(min_q), int(cap_q), C.byref(sm)))
        return sm.asdict()

    def consensus_result_device(self):
        """The results of the last consensus call left in HBM: dict(out_off, bases, quals, depth, errors) of integer
        device pointers (u64[C + 1], u8[total], u8[total], u32[C], u64[C]).  The memory belongs to this object: it is
        valid until its next consensus call or close()."""
        p = [C.c_void_p() for _ in range(5)]
        self._check(self._lib.humid_consensus_result_device(self._h, *[C.byref(x) for x in p]))
        return dict(zip(("out_off", "bases", "quals", "depth", "errors"), [x.value or 0 for x in p]))

    @staticmethod
    def _layer(bases, quals, off, n, what):
        """one layer as consensus() takes it: u8[N, L] matrices (off implied) or flat blobs with off u64[N + 1]"""
        b = np.ascontiguousarray(bases, dtype=np.uint8)
        q = np.ascontiguousarray(quals, dtype=np.uint8)
        if b.shape != q.shape:
            raise ValueError("bases_%s and quals_%s must have the same shape" % (what, what))
        if off is None:
            if b.ndim != 2 or b.shape[0] != n:
                raise ValueError("without off_%s, bases_%s and quals_%s must be u8[N, L] matrices" % (what, what, what))
            o = np.arange(n + 1, dtype=np.uint64) * np.uint64(b.shape[1])
        else:
            o = np.ascontiguousarray(off, dtype=np.uint64)
            if b.ndim != 1 or o.shape != (n + 1,):
                raise ValueError("with off_%s, bases_%s and quals_%s must be flat blobs and off_%s u64[N + 1]"
                                 % (what, what, what, what))
        return b, q, o

    def duplex_consensus(self, bases_same, quals_same, bases_other, quals_other, cluster_id, keep, strand, off_same=None,
                         off_other=None, n_clusters=None, min_q=10, strand_cap_q=40, cap_q=93):
        """One duplex consensus record per cluster (include/humid_hip.h, humid_duplex_consensus): the members of the
        representative's strand vote with their record of the SAME layer (the file the output belongs to), the
        members of the other strand with their record of the OTHER layer; each class makes a call of its own with a
        margin capped at strand_cap_q, and the two calls add when they agree and subtract when they differ.  Each
        layer is given as u8[N, L] matrices or as flat blobs with off u64[N + 1], as in consensus(); cluster_id / keep
        from run_paired (keep possibly from select_best), strand from strands().  One call per FastQ file, with the
        layers exchanged.
        Returns consensus()'s dict plus depth_same, depth_other, disagree (u32[C] each); summary has eleven fields."""
        cid = np.ascontiguousarray(cluster_id, dtype=np.uint32)
        n = len(cid)
        k = np.ascontiguousarray(keep, dtype=np.uint8)
        st = np.ascontiguousarray(strand, dtype=np.uint8)
        if cid.ndim != 1 or k.shape != (n,) or st.shape != (n,):
            raise ValueError("cluster_id, keep and strand must have shape (N,)")
        bs, qs, os_ = self._layer(bases_same, quals_same, off_same, n, "same")
        bo, qo, oo = self._layer(bases_other, quals_other, off_other, n, "other")
        if n_clusters is None:
            n_clusters = int(cid.max()) if n else 0
        sm = _lib.HumidDuplexSummary()
        self._check(self._lib.humid_duplex_consensus(
            self._h, _vp(bs), _vp(qs), _vp(os_), bs.size, _vp(bo), _vp(qo), _vp(oo), bo.size, _vp(cid), _vp(k), _vp(st), n,
            int(n_clusters), int(min_q), int(strand_cap_q), int(cap_q), C.byref(sm)))
        out = self._consensus_result(sm.asdict())
        c = out["summary"]["n_clusters"]
        for name in ("depth_same", "depth_other", "disagree"):
            out[name] = np.zeros(c, np.uint32)
        self._check(self._lib.humid_get_duplex_consensus(self._h, _vp(out["depth_same"]), _vp(out["depth_other"]),
                                                         _vp(out["disagree"]), None))
        return out

    def duplex_consensus_device(self, d_bases_same, d_quals_same, d_off_same, n_bytes_same, d_bases_other, d_quals_other,
                                d_off_other, n_bytes_other, d_cluster_id, d_keep, d_strand, n_reads, n_clusters, min_q=10,
                                strand_cap_q=40, cap_q=93):
        """duplex_consensus on device pointers (ints, e.g. tensor.data_ptr()); the results stay in HBM
        (consensus_result_device).  Returns the summary dict."""
        sm = _lib.HumidDuplexSummary()
        self._check(self._lib.humid_duplex_consensus_device(
            self._h, C.c_void_p(d_bases_same), C.c_void_p(d_quals_same), C.c_void_p(d_off_same), n_bytes_same,
            C.c_void_p(d_bases_other), C.c_void_p(d_quals_other), C.c_void_p(d_off_other), n_bytes_other,
            C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.c_void_p(d_strand), n_reads, n_clusters, int(min_q),
            int(strand_cap_q), int(cap_q), C.byref(sm)))
        return sm.asdict()

    def optical_duplicates(self, cluster_id, keep, tile, x, y, distance=100, n_clusters=None):
        """After a run: which duplicates of every cluster are optical ones (include/humid_hip.h,
        humid_optical_duplicates).  Two reads of a cluster are close when they lie on the same tile (NO_TILE: the read
        has no position) and |dx| <= distance and |dy| <= distance; the connected groups of close reads each keep one
        origin -- the cluster's kept read where the group holds it, else its smallest read index -- and every other
        read of a group is optical.  cluster_id / keep from any run (keep possibly from select_best); tile, x, y
        u32[N].  n_clusters defaults to the last run's count.  All five arrays are numpy arrays, or all five torch
        tensors on this object's device (int32 / uint8 storage is read as u32 / u8): the results then stay there.
        Returns (optical u8[N], origin u32[N], per_cluster u32[C], summary dict): origin is NO_READ for
        cluster_id == 0; pcr duplicates are summary["duplicates"] - summary["optical"]."""
        if n_clusters is None:
            n_clusters = int(self.summary["clusters"])
        n_clusters = int(n_clusters)
        distance = int(distance)
        if not 0 <= distance <= 0xffffffff:
            raise ValueError("distance must be in [0, 2**32)")
        sm = _lib.HumidOpticalSummary()
        arrays = (cluster_id, keep, tile, x, y)
        if all(hasattr(a, "data_ptr") for a in arrays):
            import torch
            n = cluster_id.numel()
            for a, size in zip(arrays, (4, 1, 4, 4, 4)):
                if not a.is_cuda or not a.is_contiguous() or a.element_size() != size or a.numel() != n or a.dim() != 1:
                    raise ValueError("device tensors must be contiguous, one-dimensional, of %d elements: cluster_id, tile, "
                                     "x, y of 4 bytes each, keep of 1" % n)
            dev = cluster_id.device
            optical = torch.zeros(n, dtype=torch.uint8, device=dev)
            origin = torch.zeros(n, dtype=torch.int32, device=dev)
            per_cluster = torch.zeros(n_clusters, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            self._check(self._lib.humid_optical_duplicates_device(
                self._h, *[C.c_void_p(a.data_ptr()) for a in arrays], n, n_clusters, distance, C.c_void_p(optical.data_ptr()),
                C.c_void_p(origin.data_ptr()), C.c_void_p(per_cluster.data_ptr()) if n_clusters else None, C.byref(sm)))
            return optical, origin, per_cluster, sm.asdict()
        cid = np.ascontiguousarray(cluster_id, dtype=np.uint32)
        n = len(cid)
        k = np.ascontiguousarray(keep, dtype=np.uint8)
        pos = []
        for name, a in (("tile", tile), ("x", x), ("y", y)):
            a = np.asarray(a)
            if a.dtype.kind not in "ui" or a.shape != (n,) or (n and (int(a.min()) < 0 or int(a.max()) > 0xffffffff)):
                raise ValueError("%s must be integers in [0, 2**32) with shape (%d,)" % (name, n))
            pos.append(np.ascontiguousarray(a, dtype=np.uint32))
        if cid.ndim != 1 or k.shape != (n,):
            raise ValueError("cluster_id and keep must have shape (N,)")
        optical = np.zeros(n, np.uint8)
        origin = np.zeros(n, np.uint32)
        per_cluster = np.zeros(n_clusters, np.uint32)
        self._check(self._lib.humid_optical_duplicates(
            self._h, _vp(cid), _vp(k), _vp(pos[0]), _vp(pos[1]), _vp(pos[2]), n, n_clusters, distance, _vp(optical), _vp(origin),
            _vp(per_cluster) if n_clusters else None, C.byref(sm)))
        return optical, origin, per_cluster, sm.asdict()

    def group_keys(self):
        """after a keyed run: the distinct keys of the usable reads, ascending (u64[G]); group g is key [g]"""
        n = C.c_uint64()
        self._check(self._lib.humid_get_group_keys(self._h, None, 0, C.byref(n)))
        k = np.zeros(n.value, np.uint64)
        self._check(self._lib.humid_get_group_keys(self._h, _vp(k), n.value, C.byref(n)))
        return k

    def keyed_rank_info(self):
        """after a keyed run: dict(n_keys, table_log2, n_redo) of its key ranking (humid_keyed_rank_info)"""
        g, t, r = C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._check(self._lib.humid_keyed_rank_info(self._h, C.byref(g), C.byref(t), C.byref(r)))
        return dict(n_keys=g.value, table_log2=t.value, n_redo=r.value)

    def group_stats(self):
        """Per-group statistics of the last run (include/humid_hip.h, humid_get_group_stats), reduced on the device:
        dict(reads u64[G], unique u32[G], clusters u32[G], edges u32[G], leaf_off u32[G+1], cluster_off u32[G+1]).
        G = n_groups after a grouped run, the number of distinct keys after a keyed run, 1 after a plain run.
        Group g owns the leaves [leaf_off[g], leaf_off[g+1]) and the cluster ids cluster_off[g]+1 .. cluster_off[g+1];
        clusters[g] is its number of molecules.  After a keyed run "key" (u64[G]) is group_keys(), so
        (key, clusters) is the count table in coordinate form."""
        n = C.c_uint64()
        self._check(self._lib.humid_get_group_stats(self._h, 0, C.byref(n), None, None, None, None))
        g = n.value
        reads, edges = np.zeros(g, np.uint64), np.zeros(g, np.uint32)
        leaf_off, cluster_off = np.zeros(g + 1, np.uint32), np.zeros(g + 1, np.uint32)
        self._check(self._lib.humid_get_group_stats(self._h, g, C.byref(n), _vp(reads), _vp(leaf_off),
                                                    _vp(cluster_off), _vp(edges)))
        out = dict(reads=reads, unique=np.diff(leaf_off), clusters=np.diff(cluster_off), edges=edges,
                   leaf_off=leaf_off, cluster_off=cluster_off)
        if getattr(self, "_keyed_summary", None) is self.summary:        # the last run was a keyed one
            out["key"] = self.group_keys()
        return out

    def group_stats_device(self):
        """The arrays of group_stats() left in HBM: dict(n, reads, leaf_off, cluster_off, edges) with n = G and
        integer device pointers (reads u64[G], leaf_off u32[G+1], cluster_off u32[G+1], edges u32[G]), e.g. for
        a torch tensor over them without a download.  The memory belongs to this object: it is valid until its
        next run or close(), and complete when the call returns."""
        n = C.c_uint64()
        p = [C.c_void_p() for _ in range(4)]
        self._check(self._lib.humid_group_stats_device(self._h, C.byref(n), *[C.byref(x) for x in p]))
        return dict(n=n.value, reads=p[0].value or 0, leaf_off=p[1].value or 0, cluster_off=p[2].value or 0,
                    edges=p[3].value or 0)

    def leaves(self):
        u = int(self.summary["unique"])
        wshape = (u, 2) if getattr(self, "_wide", False) else u
        if getattr(self, "_long_summary", None) is self.summary:         # the last run was a long one
            wshape = (u, self._long_k)
        out = dict(word=np.zeros(wshape, np.uint64), count=np.zeros(u, np.uint32),
                   first_read=np.zeros(u, np.uint32), degree=np.zeros(u, np.uint32),
                   cluster_id=np.zeros(u, np.uint32), is_max_leaf=np.zeros(u, np.uint8))
        self._check(self._lib.humid_get_leaves(self._h, _vp(out["word"]), _vp(out["count"]),
                                               _vp(out["first_read"]), _vp(out["degree"]),
                                               _vp(out["cluster_id"]), _vp(out["is_max_leaf"])))
        if getattr(self, "_grouped_summary", None) is self.summary:      # the last run was a grouped one
            out["group"] = np.zeros(u, np.uint32)
            self._check(self._lib.humid_get_leaf_groups(self._h, _vp(out["group"])))
        if getattr(self, "_keyed_summary", None) is self.summary:        # ... a keyed one
            out["key"] = self.group_keys()[out["group"]] if u else np.zeros(0, np.uint64)
        return out

    def graph_split_info(self):
        """dict(pairs_direct, pairs_graph, full_graph_built) of the last run (humid_graph_split_info)"""
        a, b, f = C.c_uint64(), C.c_uint64(), C.c_uint32()
        self._check(self._lib.humid_graph_split_info(self._h, C.byref(a), C.byref(b), C.byref(f)))
        return dict(pairs_direct=a.value, pairs_graph=b.value, full_graph_built=f.value)

    def group_records_info(self):
        """dict(searched_on_records, orders_stored) of the last run's compact graph stage (humid_group_records_info)"""
        a, b = C.c_uint32(), C.c_uint32()
        self._check(self._lib.humid_group_records_info(self._h, C.byref(a), C.byref(b)))
        return dict(searched_on_records=a.value, orders_stored=b.value)

    def wait_overlap_info(self):
        """dict(host_waits, overlapped) of the last mutating call (humid_wait_overlap_info): the host's waits for
        counters, and those of them that had kernels queued between the publishing kernel and the wait"""
        a, b = C.c_uint32(), C.c_uint32()
        self._check(self._lib.humid_wait_overlap_info(self._h, C.byref(a), C.byref(b)))
        return dict(host_waits=a.value, overlapped=b.value)

    def stamp_info(self):
        """dict(used, stamps, event_records) of the last mutating call (humid_stamp_info): whether its ms_total and
        ms_k_insert came from device stamps, the four raw stamps in ticks of 10 ns (pass start, count kernel start and
        end, pass end; zeros where the pass stored none) and the number of event records the call made"""
        used, n = C.c_uint32(), C.c_uint32()
        st = (C.c_uint64 * 4)()
        self._check(self._lib.humid_stamp_info(self._h, C.byref(used), st, C.byref(n)))
        return dict(used=bool(used.value), stamps=[int(x) for x in st], event_records=n.value)

    def run_roads(self):
        """what the last mutating call retried (humid_get_run_roads): dict(events, n_events, graph_attempts).  events:
        the names of the first 32 events in order, of PART_PADDED_REDO, ORDERS_REDONE, REGIONS_REGROWN, FAR_TILES,
        CSR_TILES, JOIN_PIECES; graph_attempts: passes through the compact graph stage's retry loop (0: it did not run)"""
        r = _lib.HumidRunRoads()
        self._check(self._lib.humid_get_run_roads(self._h, C.byref(r)))
        return r.asdict()

    def adjacency(self):
        u = int(self.summary["unique"])
        e2 = 2 * int(self.summary["edges"])
        off = np.zeros(u + 1, np.uint32)
        idx = np.zeros(max(e2, 1), np.uint32)
        self._check(self._lib.humid_get_adjacency(self._h, _vp(off), _vp(idx)))
        return off, idx[:e2]

    def clusters(self):
        c = int(self.summary["clusters"])
        size = np.zeros(max(c, 1), np.uint64)
        mc = np.zeros(max(c, 1), np.uint32)
        ml = np.zeros(max(c, 1), np.uint32)
        self._check(self._lib.humid_get_clusters(self._h, _vp(size), _vp(mc), _vp(ml)))
        return dict(size=size[:c], max_count=mc[:c], max_leaf=ml[:c])

    def histogram(self, which: int):
        """which: 0 counts.dat, 1 neigh.dat, 2 clusters.dat -> sorted [(key, value)]"""
        n = C.c_uint64()
        self._check(self._lib.humid_get_histogram(self._h, which, None, None, 0, C.byref(n)))
        k = np.zeros(max(n.value, 1), np.uint64)
        v = np.zeros(max(n.value, 1), np.uint64)
        self._check(self._lib.humid_get_histogram(self._h, which, _vp(k), _vp(v), n.value, C.byref(n)))
        return [(int(a), int(b)) for a, b in zip(k[:n.value], v[:n.value])]

    def histograms(self):
        s = self.summary
        return dict(counts=self.histogram(0), neigh=self.histogram(1), clusters=self.histogram(2),
                    stats=dict(total=int(s["total"]), usable=int(s["usable"]),
                               unique=int(s["unique"]), clusters=int(s["clusters"])))

    def accumulator(self, word_nt=24):
        """A read set fed in chunks (include/humid_hip.h, humid_accum_*): empties any earlier accumulator of this
        object and returns the new one."""
        return Accumulator(self, word_nt)

    def barcode_counter(self, barcode_nt=16):
        """The reads per barcode of a read set fed in chunks (include/humid_hip.h, humid_cells_*): empties any earlier
        counter of this object and returns the new one."""
        return BarcodeCounter(self, barcode_nt)

    def keyed_accumulator(self, word_nt=12, key_nt=0):
        """A read set with 64-bit keys fed in chunks (include/humid_hip.h, humid_accum_*_keyed): empties any earlier
        accumulator of this object, of either kind, and returns the new one."""
        return KeyedAccumulator(self, word_nt, key_nt)


class Accumulator:
    """One read set deduplicated in chunks: add() every chunk, finish(), then map() every chunk.

    The results are those of Dedup.run over all added reads sorted by global index (base + position in the chunk),
    whatever the order of the chunks.  The accumulator lives in the Dedup object's context: after finish(),
    dd.adjacency(), dd.clusters() and dd.histogram() answer for the accumulated set (until the first map())."""

    def __init__(self, dd: Dedup, word_nt: int):
        self._dd = dd
        self._lib = dd._lib
        dd._check(self._lib.humid_accum_begin(dd._h, int(word_nt)))
        self.word_nt = int(word_nt)
        self._next = 0

    def _chunk(self, words, filtered):
        w = np.ascontiguousarray(words, dtype=np.uint64)
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        want = (len(f), 2) if self.word_nt > 32 else (len(f),)
        if f.ndim != 1 or w.shape != want:
            raise ValueError("words must have shape %r for word_nt=%d (filtered: %r)" % (want, self.word_nt, f.shape))
        return w, f

    def add(self, words, filtered, base=None):
        """adds a chunk whose first read has global index `base` (default: the reads added so far); returns the base used"""
        w, f = self._chunk(words, filtered)
        base = self._next if base is None else int(base)
        self._dd._check(self._lib.humid_accum_add(self._dd._h, _vp(w), _vp(f), len(f), base))
        self._next = max(self._next, base + len(f))
        return base

    def add_device(self, d_words, d_filtered, n_reads, base):
        """the same with integer device pointers"""
        self._dd._check(self._lib.humid_accum_add_device(self._dd._h, C.c_void_p(d_words), C.c_void_p(d_filtered), n_reads, int(base)))
        self._next = max(self._next, int(base) + n_reads)
        return int(base)

    def finish(self, distance=1, method=DIRECTIONAL, edit=False):
        """clusters the accumulated words; returns the summary dict of Dedup.run over all added reads"""
        dd = self._dd
        dd.set_option("edit_distance", int(bool(edit)))
        s = _lib.HumidSummary()
        dd._check(self._lib.humid_accum_finish(dd._h, distance, method, C.byref(s)))
        dd.summary = s.asdict()
        dd._wide = self.word_nt > 32
        return dd.summary

    def map(self, words, filtered, base):
        """(cluster_id u32[N], keep u8[N], n_unknown) of a chunk whose first read has global index `base`"""
        w, f = self._chunk(words, filtered)
        cid = np.zeros(len(f), dtype=np.uint32)
        keep = np.zeros(len(f), dtype=np.uint8)
        unknown = C.c_uint64()
        self._dd._check(self._lib.humid_accum_map(self._dd._h, _vp(w), _vp(f), len(f), int(base), _vp(cid), _vp(keep),
                                                  C.byref(unknown)))
        return cid, keep, unknown.value

    def map_device(self, d_words, d_filtered, n_reads, base, d_cluster_id, d_keep):
        """the same with integer device pointers; the results stay in HBM.  Returns n_unknown."""
        unknown = C.c_uint64()
        self._dd._check(self._lib.humid_accum_map_device(self._dd._h, C.c_void_p(d_words), C.c_void_p(d_filtered), n_reads,
                                                         int(base), C.c_void_p(d_cluster_id), C.c_void_p(d_keep),
                                                         C.byref(unknown)))
        return unknown.value

    def leaves(self):
        """dict(word u64[U] or u64[U, 2], count u32[U], first u64[U]) of the accumulated list, ascending"""
        n = C.c_uint64()
        self._dd._check(self._lib.humid_accum_get_leaves(self._dd._h, None, None, None, 0, C.byref(n)))
        u = n.value
        out = dict(word=np.zeros((u, 2) if self.word_nt > 32 else u, np.uint64), count=np.zeros(u, np.uint32),
                   first=np.zeros(u, np.uint64))
        self._dd._check(self._lib.humid_accum_get_leaves(self._dd._h, _vp(out["word"]), _vp(out["count"]), _vp(out["first"]),
                                                         u, C.byref(n)))
        return out

    def info(self):
        """dict(word_nt, chunks, total, usable, unique, finished)"""
        nt, fin = C.c_uint32(), C.c_uint32()
        v = [C.c_uint64() for _ in range(4)]
        self._dd._check(self._lib.humid_accum_info(self._dd._h, C.byref(nt), *[C.byref(x) for x in v], C.byref(fin)))
        return dict(word_nt=nt.value, chunks=v[0].value, total=v[1].value, usable=v[2].value, unique=v[3].value,
                    finished=bool(fin.value))

    def clear(self):
        self._dd._check(self._lib.humid_accum_clear(self._dd._h))


class KeyedAccumulator:
    """One read set deduplicated per key in chunks (include/humid_hip.h, humid_accum_*_keyed): add() every chunk with
    its keys, finish(), then map() every chunk.

    The results are those of Dedup.run_keyed over all added reads sorted by global index.  word_nt is 1 .. 32; key_nt = 0
    takes any 64-bit key, key_nt = 1 .. 32 promises keys < 4**key_nt (a 16-nt barcode and a 12-nt UMI then share one
    uint64 on the device).  After finish(), dd.group_keys(), dd.group_stats(), dd.adjacency(), dd.clusters() and
    dd.histogram() answer for the accumulated set (until the first map()); dd.leaves() does not (it asks for first_read,
    which only a complete run has: leaves() of this object gives the list with its global first indices).
    Whitelist correction composes per chunk: keys_out, status, _ = dd.correct_keys(keys, filtered), then add or map
    keys_out with filtered | (status >= BC_AMBIGUOUS)."""

    def __init__(self, dd: Dedup, word_nt: int, key_nt: int):
        self._dd = dd
        self._lib = dd._lib
        dd._check(self._lib.humid_accum_begin_keyed(dd._h, int(word_nt), int(key_nt)))
        self.word_nt, self.key_nt = int(word_nt), int(key_nt)
        self._next = 0

    @staticmethod
    def _chunk(words, keys, filtered):
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        if f.ndim != 1:
            raise ValueError("filtered must be one-dimensional")
        return _keys_u64(words, f.shape, "words"), _keys_u64(keys, f.shape), f

    def add(self, words, keys, filtered, base=None):
        """adds a chunk whose first read has global index `base` (default: the reads added so far); returns the base used"""
        w, k, f = self._chunk(words, keys, filtered)
        base = self._next if base is None else int(base)
        self._dd._check(self._lib.humid_accum_add_keyed(self._dd._h, _vp(w), _vp(k), _vp(f), len(f), base))
        self._next = max(self._next, base + len(f))
        return base

    def add_device(self, d_words, d_keys, d_filtered, n_reads, base):
        """the same with integer device pointers"""
        self._dd._check(self._lib.humid_accum_add_keyed_device(self._dd._h, C.c_void_p(d_words), C.c_void_p(d_keys),
                                                               C.c_void_p(d_filtered), n_reads, int(base)))
        self._next = max(self._next, int(base) + n_reads)
        return int(base)

    def finish(self, distance=1, method=DIRECTIONAL, edit=False):
        """clusters the accumulated entries; returns the summary dict of Dedup.run_keyed over all added reads"""
        dd = self._dd
        dd.set_option("edit_distance", int(bool(edit)))
        s = _lib.HumidSummary()
        dd._check(self._lib.humid_accum_finish(dd._h, distance, method, C.byref(s)))
        dd.summary = dd._grouped_summary = dd._keyed_summary = s.asdict()
        dd._wide = False
        return dd.summary

    def map(self, words, keys, filtered, base):
        """(cluster_id u32[N], keep u8[N], n_unknown) of a chunk whose first read has global index `base`"""
        w, k, f = self._chunk(words, keys, filtered)
        cid = np.zeros(len(f), dtype=np.uint32)
        keep = np.zeros(len(f), dtype=np.uint8)
        unknown = C.c_uint64()
        self._dd._check(self._lib.humid_accum_map_keyed(self._dd._h, _vp(w), _vp(k), _vp(f), len(f), int(base), _vp(cid),
                                                        _vp(keep), C.byref(unknown)))
        return cid, keep, unknown.value

    def map_device(self, d_words, d_keys, d_filtered, n_reads, base, d_cluster_id, d_keep):
        """the same with integer device pointers; the results stay in HBM.  Returns n_unknown."""
        unknown = C.c_uint64()
        self._dd._check(self._lib.humid_accum_map_keyed_device(self._dd._h, C.c_void_p(d_words), C.c_void_p(d_keys),
                                                               C.c_void_p(d_filtered), n_reads, int(base),
                                                               C.c_void_p(d_cluster_id), C.c_void_p(d_keep), C.byref(unknown)))
        return unknown.value

    def leaves(self):
        """dict(key u64[U], word u64[U], count u32[U], first u64[U]) of the accumulated list, ascending by (key, word)"""
        n = C.c_uint64()
        self._dd._check(self._lib.humid_accum_get_leaves_keyed(self._dd._h, None, None, None, None, 0, C.byref(n)))
        u = n.value
        out = dict(key=np.zeros(u, np.uint64), word=np.zeros(u, np.uint64), count=np.zeros(u, np.uint32),
                   first=np.zeros(u, np.uint64))
        self._dd._check(self._lib.humid_accum_get_leaves_keyed(self._dd._h, _vp(out["key"]), _vp(out["word"]),
                                                               _vp(out["count"]), _vp(out["first"]), u, C.byref(n)))
        return out

    def info(self):
        """dict(word_nt, key_nt, entry_words, n_keys, chunks, total, usable, unique, finished)"""
        nt, fin, knt, ew, nk = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        v = [C.c_uint64() for _ in range(4)]
        self._dd._check(self._lib.humid_accum_info(self._dd._h, C.byref(nt), *[C.byref(x) for x in v], C.byref(fin)))
        self._dd._check(self._lib.humid_accum_keyed_info(self._dd._h, C.byref(knt), C.byref(ew), C.byref(nk)))
        return dict(word_nt=nt.value, key_nt=knt.value, entry_words=ew.value, n_keys=nk.value, chunks=v[0].value,
                    total=v[1].value, usable=v[2].value, unique=v[3].value, finished=bool(fin.value))

    def clear(self):
        self._dd._check(self._lib.humid_accum_clear(self._dd._h))


class BarcodeCounter:
    """The whitelist taken from a read set fed in chunks (include/humid_hip.h, humid_cells_*): add() every chunk's keys,
    then finish() with discover_whitelist's arguments.

    finish() gives what Dedup.discover_whitelist gives over all added reads, whatever their order and cut: the same dict,
    the same whitelist in place, the same dd.discovered_cells() and dd.barcode_count_hist().  It does not consume the
    counter: it may be called again with other arguments, and more chunks may be added behind it.  The counter lives
    in the Dedup object's context, in memory of its own: runs, accumulators and one-shot discover calls leave it alone."""

    def __init__(self, dd: Dedup, barcode_nt: int):
        self._dd = dd
        self._lib = dd._lib
        dd._check(self._lib.humid_cells_begin(dd._h, int(barcode_nt)))
        self.barcode_nt = int(barcode_nt)

    def add(self, keys, filtered):
        """adds a chunk (numpy arrays: keys u64[N], filtered u8[N])"""
        f = np.ascontiguousarray(filtered, dtype=np.uint8)
        if f.ndim != 1:
            raise ValueError("filtered must be one-dimensional")
        k = _keys_u64(keys, f.shape)
        n = len(f)
        self._dd._check(self._lib.humid_cells_add(self._dd._h, _vp(k) if n else None, _vp(f) if n else None, n))

    def add_device(self, d_keys, d_filtered, n_reads):
        """the same with integer device pointers"""
        self._dd._check(self._lib.humid_cells_add_device(self._dd._h, C.c_void_p(d_keys) if n_reads else None,
                                                         C.c_void_p(d_filtered) if n_reads else None, n_reads))

    def finish(self, top=None, expected=None, min_reads=None, merge_ratio=0):
        """selects the cells over everything added and installs them as the whitelist; returns discover_whitelist's dict"""
        mode, param, merge_ratio = Dedup._cells_mode(top, expected, min_reads, merge_ratio)
        sm = _lib.HumidCellsSummary()
        self._dd._check(self._lib.humid_cells_finish(self._dd._h, mode, param, merge_ratio, C.byref(sm)))
        return sm.asdict()

    def info(self):
        """dict(barcode_nt, chunks, reads, usable, invalid_reads, distinct, table_log2, n_grown)"""
        nt, log2, grown = C.c_uint32(), C.c_uint32(), C.c_uint32()
        v = [C.c_uint64() for _ in range(5)]
        self._dd._check(self._lib.humid_cells_info(self._dd._h, C.byref(nt), *[C.byref(x) for x in v], C.byref(log2),
                                                   C.byref(grown)))
        return dict(barcode_nt=nt.value, chunks=v[0].value, reads=v[1].value, usable=v[2].value, invalid_reads=v[3].value,
                    distinct=v[4].value, table_log2=log2.value, n_grown=grown.value)

    def clear(self):
        self._dd._check(self._lib.humid_cells_clear(self._dd._h))


class ClusterGraph(Context):
    """NLeaf graphs built by hand, as tests/test_cluster.cc:11-14 does with link()."""

    def __init__(self, counts, device: int = -1):
        super().__init__(device)
        self.counts = [int(c) for c in counts]
        self.nbrs = [[] for _ in self.counts]

    def link(self, a, b):
        self.nbrs[a].append(b)
        self.nbrs[b].append(a)

    def find_clusters(self, maximum=False):
        """findClusters over the leaves in index order.  Returns dict(leaf_cluster, size,
        max_count, max_leaf, n_clusters)."""
        u = len(self.counts)
        cnt = np.asarray(self.counts, dtype=np.uint32)
        off = np.zeros(u + 1, dtype=np.uint32)
        for i, l in enumerate(self.nbrs):
            off[i + 1] = off[i] + len(l)
        idx = np.asarray([x for l in self.nbrs for x in l] or [0], dtype=np.uint32)
        lc = np.zeros(max(u, 1), np.uint32)
        size = np.zeros(max(u, 1), np.uint64)
        mc = np.zeros(max(u, 1), np.uint32)
        ml = np.zeros(max(u, 1), np.uint32)
        nc = C.c_uint32()
        self._check(self._lib.humid_cluster_graph(self._h, _vp(cnt), _vp(off), _vp(idx), u,
                                                  MAXIMUM if maximum else DIRECTIONAL, _vp(lc),
                                                  _vp(size), _vp(mc), _vp(ml), C.byref(nc)))
        c = nc.value
        return dict(leaf_cluster=lc[:u], size=size[:c], max_count=mc[:c], max_leaf=ml[:c],
                    n_clusters=c)


def at_least_double(a: int, b: int, ctx: Context | None = None) -> bool:
    own = ctx is None
    ctx = ctx or Context()
    r = C.c_int()
    ctx._check(ctx._lib.humid_at_least_double(ctx._h, a, b, C.byref(r)))
    if own:
        ctx.close()
    return bool(r.value)
