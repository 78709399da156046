/*
 * humid_hip.h -- C ABI of libhumid_hip.so: HUMID's neighbour-search-and-cluster hot
 * path on one MI355X (gfx950), hand-written HIP.
 *
 * The reference (jfjlaros/HUMID, /root/reference) has no FFI/plugin seam; the seam
 * this library fills is the C++ surface src/humid.cc uses between FastQ pass 1 and
 * pass 2: lib/trie's Trie<4,NLeaf> (add / walk /
 * asymmetricHamming / find) plus src/cluster.{h,cc} and src/leaf.h.  Each entry
 * point below names the reference interface it replaces (paths relative to
 * /root/reference).  Plain pointers and sizes only; nothing throws or aborts across
 * the ABI; every function returns HUMID_OK (0) or a negative HUMID_E_* code and
 * humid_last_error() gives the text.  There is NO CPU fallback in this library.
 *
 * Packed word: nucleotide i (A0 C1 G2 T3, src/fastq.cc:12) of an n-symbol word
 * (n = -n word length, src/humid.cc:419) occupies bits [2(n-1-i), 2(n-1-i)+1] of a
 * uint64, so unsigned integer order == lexicographic order == Trie::walk() order.
 * n <= 32: one uint64 per read (all BASELINE.json configs use n = 24).
 * 33 <= n <= 64 ("wide" words): TWO uint64 per read, [2r] = the first n-32 nucleotides packed the
 * same way (right-aligned), [2r+1] = the last 32; every words / word array of the single-GPU entry
 * points (humid_dedup_run, humid_dedup_run_device, humid_get_leaves) then holds 2 entries per
 * read / leaf, 16-byte aligned on the device.  n > 64 returns HUMID_E_UNSUPPORTED from the entry points below;
 * see humid_dedup_run_long (up to HUMID_LONG_MAX_NT nucleotides, ceil(n / 32) uint64 per read).  Several GPUs:
 * humid_dedup_run_exchange takes wide words; of the humid_stage_* entry points those of the all-gather mode do
 * (humid_stage_histogram, _count_dense with a filter array, _unique, _graph, _graph_edges,
 * humid_stage_owner_perm_wide: value ranges are then ranges of HEADS, the top 64 bits of a word's 2n-bit value, and
 * the histogram is that of 32-nt words over the heads); the others return HUMID_E_UNSUPPORTED for n > 32.
 */
#ifndef HUMID_HIP_H
#define HUMID_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HUMID_OK             0
#define HUMID_E_INVALID     -1   /* bad argument                                    */
#define HUMID_E_UNSUPPORTED -2   /* word_nt > 64 (stages: > 32)                      */
#define HUMID_E_NOMEM       -3   /* device or host allocation failed                */
#define HUMID_E_HIP         -4   /* HIP runtime error (text in humid_last_error)    */
#define HUMID_E_OVERFLOW    -5   /* an index exceeded 32 bits (reads, 2*edges)      */
#define HUMID_E_STATE       -6   /* accessor called before a successful run         */

#define HUMID_METHOD_DIRECTIONAL 0u  /* default; src/cluster.cc:82-87               */
#define HUMID_METHOD_MAXIMUM     1u  /* -x;      src/cluster.cc:72-80               */

#define HUMID_ABI_VERSION 5u   /* 5: humid_stage_owner_perm_wide, wide words in the all-gather stages; 4: humid_exchange_info.d_unique_degree replaces d_compact_edges (owner-local clustering, round 3); 3: humid_dedup_run_exchange, humid_comm, humid_shm_* (round 2); 2: humid_dedup_run_bases, humid_stage_route ... */

typedef struct humid_ctx humid_ctx;   /* device workspace + stream; not thread-safe */

/* total/usable/unique/clusters are the four lines of stats.dat
 * (src/humid.cc:351-355).  ms_* are device times (hipEvents on the ctx stream). */
typedef struct humid_summary {
  uint64_t total;       /* reads seen                    src/humid.cc:98          */
  uint64_t usable;      /* reads without non-ACGT        src/humid.cc:96          */
  uint64_t unique;      /* distinct words                src/humid.cc:125         */
  uint64_t clusters;    /* clusters.size()               src/humid.cc:403         */
  uint64_t edges;       /* undirected neighbour pairs                             */
  uint64_t nonsingle;   /* unique words with >= 1 neighbour                       */
  /* the four stage times: filled by humid_dedup_run* only with option "kernel_timing" (0 otherwise; round 3: an
   * event record between two kernels costs ~4-6 us of idle GPU); ms_total and ms_k_insert are always measured: on
   * the record road of a lean pass by device stamps (option "device_stamps": the 100 MHz wall clock read at the
   * entry of four kernels that run anyway, no marker in the stream), by four event records elsewhere              */
  float ms_count;       /* hash insert + unique sort     (Trie::add, walk order)  */
  float ms_neighbours;  /* bucket passes + CSR           (findHammingNeighbours)  */
  float ms_cluster;     /* components + cluster kernel   (findClusters)           */
  float ms_map;         /* per-read map                  (writeFiltered/Annotated)*/
  float ms_total;       /* first kernel to last kernel on the stream (device stamps: entry of the first to entry of the last) */
  float ms_h2d, ms_d2h; /* host-buffer entry point only                           */
  /* single kernels, HIP events directly around the launches on the ctx stream:      */
  float ms_k_insert;    /* the count kernel: k_dedup_rec / k_dedup_lds / k_hash_insert (one launch); device stamps: its
                         * entry to the entry of the launch behind it, so with the dispatch between the two */
  float ms_k_pairs;     /* sum over the 2(d+1) k_pairs launches (count + fill)      */
  float ms_k_cluster;   /* k_cluster_pairs + _small (+ _components): 2-3 launches   */
  float ms_k_map;       /* first kernel of the un-permute: k_unperm_bins (or k_read_map_bucket, _part, k_read_map) */
  float ms_k_part;      /* front partition: the second-level scatter k_pt_scatter<2> (0: library radix passes) */
  float ms_k_unperm;    /* second kernel of the un-permute: k_unperm_window (0: one-kernel forms)   */
  uint32_t count_mode_used;  /* 0 = LDS tables, hashed buckets; 2 = LDS tables, word-ordered buckets (words of
                              * 33-64 nt: buckets on their top 64 bits); 1 = global HBM table (option or
                              * fallback); 3 = sorted (words of 33-64 nt: small inputs, uneven top bits, fallback).
                              * Bit 8 (0x100) is set on top of 2 when the count ran on 8-byte records (round 3). */
} humid_summary;

uint32_t humid_abi_version(void);
int      humid_device_count(void);

/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for
 * a stream owned by the context.  device < 0: current device. */
int  humid_ctx_create(humid_ctx **out, int device, void *stream);
void humid_ctx_destroy(humid_ctx *ctx);
const char *humid_last_error(const humid_ctx *ctx);   /* ctx may be NULL */
/* Options.  All but "edit_distance" are tuning knobs that never change results.  "count_mode": 0 = exact counts in hash-partitioned
 * LDS-resident tables (default; falls back to 1 by itself when a bucket overflows), 1 = one
 * open-address table in HBM.  Environment HUMID_COUNT_MODE presets it.
 * "plan_segments": 0 = automatic choice of the pigeonhole plan (s segments, buckets on every
 * combination of s-d of them), else force s (ignored when illegal for the given n, d).
 * "count_order": LDS buckets formed on the word prefix instead of its hash, which makes the unique
 * sort unnecessary: -1 (default) = when a sampled histogram of the top word bits says the fullest
 * bucket fits its LDS table (UMI-first layouts), 0 = never, 1 = always (either way a bucket
 * overflow falls back to hashed buckets).  Words of 33-64 nt: the same choice between LDS tables over
 * buckets of their top 64 bits and the sorting count (0 = always sort; "count_mode" 1 sorts too).
 * "edit_distance": 1 = neighbours under Levenshtein instead of Hamming distance (-e,
 *   findEditNeighbours src/humid.cc:140-158 / Trie::asymmetricLevenshtein) in humid_dedup_run*.
 *   Between equal-length words distance <= 1 is the Hamming search itself; 2 and 3 add the pairs that
 *   need one deletion + one insertion, 4 and 5 those with two of each (banded dynamic programmes); beyond 5
 *   every candidate is verified with the whole dynamic programme (no limit on the distance; the joins' keys
 *   shrink to one segment of n / (d + 1) nucleotides, so the search approaches all pairs, as the trie's does).
 * "coop_big": 1 (default) = components of more than 32 leaves are clustered by one workgroup each
 * (parallel flood), 0 = by one lane each (the literal sequential loop).
 * "tile_partition": 1 (default) = reads reach their count buckets, and results their reads, through
 * the hand-written LDS-staged partition (two coalesced passes each way); 0 = library radix passes
 * in front and one scattered store per read at the end (the round-1 form, also taken by itself for
 * read sets beyond ~180 M / ~67 M reads).
 * "kernel_timing": 1 = HIP events around the single kernels and between the stages, so that
 * humid_summary.ms_k_pairs / ms_k_cluster / ms_k_map / ms_k_part / ms_k_unperm and the stage times ms_count ..
 * ms_map of humid_dedup_run* are filled (default 0, also HUMID_KERNEL_TIMING: the 17 extra event records cost
 * 30-50 us of a 0.7 ms pass; ms_k_insert and ms_total are always there).
 * "device_stamps": 1 (default) = a pass without "kernel_timing" that counts on 8-byte records (one-word words,
 * humid_dedup_run / _device) takes ms_total and ms_k_insert from four device stamps -- thread 0 of workgroup 0 of
 * the first k_zero_many, of k_dedup_rec, of the scan behind it and of the pass's last k_publish_counters stores the
 * 100 MHz wall clock, and the last host wait delivers the four with the counters -- and records no event; 0 = the
 * four event records ev[0], kev[0], kev[1], ev[4] on every road (each a marker the next kernel waits ~6 us behind).
 * Every other road and every pass with "kernel_timing" records its events with either value.  humid_stamp_info.
 * "padded_partition": 1 (default) = the first level of the tile partition scatters into coarse bins of a
 * fixed room and needs no histogram pass over the reads; a bin that outgrows its room (heavily duplicated
 * words) is detected, the run repeated with the histogram pass, and the option stays 0 for this context.
 * "force_comm": 1 = humid_dedup_run_exchange goes through the humid_comm callbacks even with one rank
 * (a transport can be exercised on a one-GPU box); default 0: with one rank nothing is called or copied.
 * "bucket_walk": how many following words of its pigeonhole bucket a position is compared with by
 * its own thread (default 1024); the pairs further apart inside longer buckets are compared as
 * 1024 x 1024 tiles by whole workgroups.  0 = no bound (every pair by the position's thread, the
 * round-1 form: quadratic per lane on buckets of 10^5 words).  Results do not depend on it.
 * "optical_walk": how many following reads of its window (same cluster and tile, x no more than the distance ahead)
 * a sorted position of humid_optical_duplicates* is compared with by its own lane (default 64); the rest of a longer
 * window is compared by the 64 lanes of the position's wave side by side.  0 = no bound (quadratic per lane on a
 * cluster of 10^5 reads on one spot).  Results do not depend on it.
 * "accum_tile": merge positions per workgroup of humid_accum_add*'s merge, a power of two from 64 to 2048 (default
 * 2048: the staged tile takes 16 KB of LDS for one-word words, 32 KB for two-word words).  Results do not depend on it;
 * small values make small inputs cross many tile boundaries (tests).
 * "long_key_bits": 1 .. 64 (default 64), the bits of the join keys of humid_dedup_run_long*'s neighbour search.  Results
 * do not depend on it; 2 makes nearly all leaves share a key, which sends small inputs through the long buckets (tests). */
int  humid_ctx_set_option(humid_ctx *ctx, const char *key, int64_t value);
/* Optional: one slab of device memory for a run over about n_reads reads, so that the first run does
 * not pay ~35 separate allocations (the `humid` host calls it while pass 1 still parses).  Never
 * fails for lack of memory: without a slab the buffers are allocated one by one as before. */
int  humid_ctx_reserve(humid_ctx *ctx, uint64_t n_reads, uint32_t word_nt);
/* Page-locked host memory for the buffers of humid_dedup_run*: copies from / to it run at the full
 * PCIe rate (pageable buffers are staged by the runtime at a fraction of it: 5 GB/s measured).
 * NULL when the allocation fails -- ordinary memory works everywhere, only slower. */
void *humid_host_alloc(uint64_t bytes);
void  humid_host_free(void *p);

/* ---- the whole hot path ----------------------------------------------------
 * Replaces, between FastQ pass 1 and pass 2:
 *   trie.add(word.data)                 src/humid.cc:94-97   (exact counts)
 *   findHammingNeighbours(trie, d)      src/humid.cc:113-130 (lib/trie walk x asymmetricHamming)
 *     or, option "edit_distance",
 *   findEditNeighbours(trie, d)         src/humid.cc:140-158 (walk x asymmetricLevenshtein)
 *   findClusters(trie, maximum)         src/humid.cc:167-193 + src/cluster.cc:10-87
 *   trie.find(word)->leaf->cluster ...  src/humid.cc:223-231 (keep), :276-277 (cluster id)
 * words[N] (2N uint64 when word_nt > 32), filtered[N] in; cluster_id[N] (0 = filtered, ids 1.. in the order
 * src/humid.cc:177-180 hands them out) and keep[N] (1 = the record writeFiltered
 * emits: the first read, in input order, whose word is its cluster's maxLeaf) out.
 * Host buffers, caller-owned; summary may be NULL. */
int humid_dedup_run(humid_ctx *ctx, const uint64_t *words, const uint8_t *filtered,
                    uint64_t n_reads, uint32_t word_nt, uint32_t distance, uint32_t method,
                    uint32_t *cluster_id, uint8_t *keep, humid_summary *summary);

/* Same contract with DEVICE pointers (inputs already resident in HBM, outputs left
 * in HBM); work is queued on the context's stream and the call returns after the
 * stream has drained.  summary (host) may be NULL. */
int humid_dedup_run_device(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered,
                           uint64_t n_reads, uint32_t word_nt, uint32_t distance,
                           uint32_t method, uint32_t *d_cluster_id, uint8_t *d_keep,
                           humid_summary *summary);

/* The same with the word packing on the device (makeWord, src/fastq.cc:146-161): bases[n_reads *
 * word_nt] holds, per record, the word_nt symbols getNucleotides (src/fastq.cc:116-144) assembles --
 * header UMI, then the leading bases of every file's read, 'N' where a read or UMI was short -- as
 * the ASCII bytes of the FastQ.  A/C/G/T -> 0/1/2/3; any other byte counts as 'G' and filters the
 * word (src/fastq.cc:151-158).  humid_get_packed_words returns the words and flags the device made
 * (u64[n_reads], or u64[2 n_reads] above 32 nt; u8[n_reads]). */
int humid_dedup_run_bases(humid_ctx *ctx, const uint8_t *bases, uint64_t n_reads, uint32_t word_nt,
                          uint32_t distance, uint32_t method, uint32_t *cluster_id, uint8_t *keep,
                          humid_summary *summary);
int humid_get_packed_words(humid_ctx *ctx, uint64_t *words, uint8_t *filtered);

/* ---- long words: the whole hot path beyond 64 nucleotides -------------------------------------
 * (reference-free deduplication on read prefixes: -n is a plain size_t in src/humid.cc:419-420.)
 * 1 <= word_nt <= HUMID_LONG_MAX_NT; 0 returns HUMID_E_INVALID, more HUMID_E_UNSUPPORTED.  k = ceil(word_nt / 32)
 * uint64 per read, words[k * r + j]: [k * r + 0] holds the first word_nt - 32 (k - 1) nucleotides right-aligned (the
 * bits above them are ignored), every following uint64 the next 32, packed as everywhere in this library.  For
 * word_nt <= 32 and 33 .. 64 that IS the one- and two-word layout above.  Device pointers need 8-byte alignment only.
 * The results are those of humid_dedup_run's contract with "word" read as the k-uint64 value in lexicographic
 * (= numeric, most significant first) order: leaves = the distinct usable words ascending, counts, Hamming neighbours
 * over all word_nt nucleotides, directional / maximum clusters, id numbering, keep = the first read of the cluster's
 * maxLeaf, summary (count_mode_used is 3: the count sorts).  For word_nt <= 64 the outputs equal humid_dedup_run's
 * bit for bit; the long kernels run there too, nothing is forwarded.
 * The search: pigeonhole over distance + 1 contiguous segments of the word; per segment the leaves are joined on a
 * 64-bit key of the segment's nucleotides (masked to option "long_key_bits", 1 .. 64, default 64: results never depend
 * on it, small values force key collisions) and every candidate pair is verified by the exact Hamming distance over
 * all k uint64.  distance >= word_nt, or more segments than the plan's combinations allow, compares all pairs
 * (HUMID_E_OVERFLOW beyond 2^18 distinct words).
 * Option "edit_distance" set returns HUMID_E_UNSUPPORTED.  After a long run humid_get_leaves writes k uint64 per leaf;
 * humid_get_adjacency, _clusters and _histogram answer as after any run; humid_get_group_stats / humid_group_stats_device
 * and humid_get_packed_words return HUMID_E_STATE, and so do humid_select_best / humid_select_best_device (they read one or
 * two uint64 per read; word_nt > 64 is HUMID_E_UNSUPPORTED there after any other run).  Grouped, keyed, paired, accumulated, sharded and stage runs,
 * humid_dedup_run_bases and humid_select_best stay at 64 nucleotides. */
#define HUMID_LONG_MAX_NT 512u
int humid_dedup_run_long(humid_ctx *ctx, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads,
                         uint32_t word_nt, uint32_t distance, uint32_t method, uint32_t *cluster_id, uint8_t *keep,
                         humid_summary *summary);
int humid_dedup_run_long_device(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                                uint32_t word_nt, uint32_t distance, uint32_t method, uint32_t *d_cluster_id,
                                uint8_t *d_keep, humid_summary *summary);
/* Which road the last long run took (tests assert it); HUMID_E_STATE unless the last run was a long one. */
typedef struct humid_long_info_t {
  uint32_t words_per_read;   /* k                                                            */
  uint32_t joins;            /* segments of the search: distance + 1 (1: all pairs, and distance 0, where the one segment is
                              * the whole word and distinct leaves share none: nothing is launched); 0: fewer than 2 leaves */
  uint32_t key_bits;         /* bits of the join keys                                         */
  uint32_t piece_joins;      /* joins whose runs of equal keys were cut into pieces           */
  uint64_t candidates;       /* pairs handed to the full-word verification, over all joins    */
  uint64_t raw_edges;        /* pairs that passed it, before duplicates were removed          */
  uint64_t edges;
} humid_long_info_t;
int humid_long_info(humid_ctx *ctx, humid_long_info_t *out);

/* ---- grouped deduplication: words are clustered only within caller-given groups ----------------
 * (per cell barcode, per alignment position, per sample: UMI-tools --per-cell / dedup, fgbio
 * GroupReadsByUmi).  group[n_reads] (u32) beside words and filtered; 1 <= n_groups.  The results are
 * DEFINED as: for each group g in ascending order, humid_dedup_run on the reads with group == g (input
 * order), its cluster_id / keep scattered back to the reads' positions, every non-zero cluster id
 * raised by the clusters of all groups below g.  So words in different groups are never neighbours;
 * the walk order (leaf i of humid_get_leaves / _adjacency / _clusters, the cluster ids) is (group,
 * word) ascending; first_read is a global read index; summary counts and the three histograms are
 * over all groups.  Filtered reads get cluster id 0 and keep 0 and their group is not read.
 * n_groups == 1 (group may then be NULL) is the plain pass, bit for bit.  The option "edit_distance"
 * applies (Levenshtein between the words only), and no tuning option changes results.
 * Let group_nt = ceil(ceil(log2(n_groups)) / 2) (0 for one group): word_nt + group_nt > 64 returns
 * HUMID_E_UNSUPPORTED.  A usable read with group >= n_groups returns HUMID_E_INVALID (the context stays
 * usable).  words keep the caller's layout (one uint64 per read up to 32 nt, two beyond).  Not for the
 * multi-GPU pass.
 *   humid_dedup_run_grouped_device: the same with DEVICE pointers, like humid_dedup_run_device.
 *   humid_get_leaf_groups: after a grouped run, the group of every leaf (u32[unique]); humid_get_leaves
 *     returns the words without it.  HUMID_E_STATE after any other run.
 *   humid_grouped_plan_info: the pigeonhole plan of a grouped run over n_unique unique words in total
 *     (combinations, bits of the longest combination key, which always starts with the whole group
 *     field) and group_nt.  Host arithmetic only: ctx may be NULL. */
int humid_dedup_run_grouped(humid_ctx *ctx, const uint64_t *words, const uint32_t *group,
                            const uint8_t *filtered, uint64_t n_reads, uint32_t word_nt,
                            uint32_t n_groups, uint32_t distance, uint32_t method,
                            uint32_t *cluster_id, uint8_t *keep, humid_summary *summary);
int humid_dedup_run_grouped_device(humid_ctx *ctx, const uint64_t *d_words, const uint32_t *d_group,
                                   const uint8_t *d_filtered, uint64_t n_reads, uint32_t word_nt,
                                   uint32_t n_groups, uint32_t distance, uint32_t method,
                                   uint32_t *d_cluster_id, uint8_t *d_keep, humid_summary *summary);
int humid_get_leaf_groups(humid_ctx *ctx, uint32_t *group);
int humid_grouped_plan_info(humid_ctx *ctx, uint32_t word_nt, uint32_t n_groups, uint32_t distance,
                            uint64_t n_unique, uint32_t *n_combos, uint32_t *key_bits,
                            uint32_t *group_nt);

/* ---- keyed deduplication: grouped runs whose groups are arbitrary 64-bit keys -------------------
 * (a 16-nt cell barcode as a 32-bit value, barcode + gene or (contig, position, strand) as a 64-bit
 * value).  key[n_reads] (u64) beside words and filtered.  Let K be the ascending (unsigned) list of
 * the distinct key[r] over the usable reads (filtered[r] == 0) and G = len(K).  The results --
 * cluster_id / keep, summary, humid_get_leaves, humid_get_leaf_groups, _adjacency, _clusters, the
 * three histograms -- are DEFINED as those of humid_dedup_run_grouped with group[r] = index of key[r]
 * in K and n_groups = max(G, 1).  Every 64-bit value is a legal key.  Keys of filtered reads are
 * never read: they may be anything and never become a group.  With group_nt as above for G groups,
 * word_nt + group_nt > 64 returns HUMID_E_UNSUPPORTED and leaves the context usable; G <= n_reads <
 * 2^31 gives group_nt <= 16, so every word_nt <= 48 is accepted whatever the keys are.  The option
 * "edit_distance" applies as in grouped runs; no tuning option changes results.  Not for the
 * multi-GPU pass.
 * The keys are ranked on the device (no host-side sort or hash): the distinct keys go into an
 * open-address table, are compacted and sorted (work proportional to G), and a second pass over the
 * reads writes every rank straight into the internal word of the grouped pass.  G chooses group_nt
 * and the pigeonhole plan, so the ranking has ONE host wait of its own (about 10 us of idle device,
 * in front of the three waits of the pass).  A table that turns out too small is seen at that wait
 * and the ranking is repeated with a larger one (16 times the slots, at most 2 n_reads rounded up
 * to a power of two, which cannot be too small); the size that fitted is remembered for the next
 * run of the context.  Option "keyrank_table_log2" (4 .. 32, 0 = automatic): every ranking starts
 * with a table of that many slots instead; results do not depend on it.
 *   humid_dedup_run_keyed_device: the same with DEVICE pointers, like humid_dedup_run_grouped_device.
 *   humid_get_group_keys: K of the last run, up to cap keys; *n_out = G (call with cap = 0 to size
 *     the buffer).  The key of a leaf is K[leaf group].  HUMID_E_STATE unless the last run was a
 *     keyed run.
 *   humid_keyed_rank_info: the ranking of the last keyed run: G, log2 of the table size it ended
 *     with, and how often it was repeated with a larger table.  Any pointer may be NULL. */
int humid_dedup_run_keyed(humid_ctx *ctx, const uint64_t *words, const uint64_t *key,
                          const uint8_t *filtered, uint64_t n_reads, uint32_t word_nt,
                          uint32_t distance, uint32_t method, uint32_t *cluster_id, uint8_t *keep,
                          humid_summary *summary);
int humid_dedup_run_keyed_device(humid_ctx *ctx, const uint64_t *d_words, const uint64_t *d_key,
                                 const uint8_t *d_filtered, uint64_t n_reads, uint32_t word_nt,
                                 uint32_t distance, uint32_t method, uint32_t *d_cluster_id,
                                 uint8_t *d_keep, humid_summary *summary);
int humid_get_group_keys(humid_ctx *ctx, uint64_t *keys, uint64_t cap, uint64_t *n_out);
int humid_keyed_rank_info(humid_ctx *ctx, uint64_t *n_keys, uint32_t *table_log2, uint32_t *n_redo);

/* ---- barcode whitelist: keys one substitution away from a known barcode are corrected ------------
 * (UMI-tools --per-cell with a whitelist, Cell Ranger, STARsolo 1MM.)  Let K = barcode_nt, 1 <= K <= 32.
 * A barcode is a K-nucleotide word packed like every word here (first nucleotide most significant,
 * value < 4^K); W is the set of distinct barcodes of the whitelist.  For a read r with k = key[r]:
 *   status               value  condition                                               key_out[r]
 *   HUMID_BC_FILTERED      0    filtered[r] != 0; the key is not read                   0
 *   HUMID_BC_EXACT         1    k in W                                                  k
 *   HUMID_BC_CORRECTED     2    k not in W, exactly one w in W at Hamming distance 1    that w
 *                               from k over the K nucleotides
 *   HUMID_BC_AMBIGUOUS     3    k not in W, two or more such w                          k
 *   HUMID_BC_UNMATCHED     4    k not in W, no such w                                   k
 * So a key with bits set above 2K is unmatched, and a key that IS a whitelist barcode is exact even
 * when another barcode lies one nucleotide away.  Distance 2, insertions / deletions, base qualities
 * (the next section decides ambiguous keys by them) and barcodes with N (the caller marks such a
 * read filtered) are not handled.
 * A CORRECTED KEYED RUN is humid_dedup_run_keyed on key_out with
 *   filtered'[r] = filtered[r] || status[r] is AMBIGUOUS or UNMATCHED;
 * cluster_id / keep, the summary (usable counts filtered' == 0), humid_get_group_keys (now a subset
 * of W), leaves, adjacency, clusters, histograms and humid_get_group_stats follow from the contracts
 * above.
 * On the device: the whitelist is an open-address table of keys in HBM, 2^ceil(log2(2 n)) slots for
 * the n barcodes passed (load <= 0.5: every probe ends at a free slot), built once by
 * humid_whitelist_set and owned by the context: it survives any number of runs of any kind until it
 * is replaced, cleared (n = 0) or the context destroyed.  The correction is one pass over the reads
 * in front of the unchanged keyed pass: every lane looks its own key up (one lookup per run of equal
 * keys inside a wave); for a key that missed, the 64 lanes of the wave look up its 3K one-substitution
 * variants side by side, and a ballot counts the hits.  Option "whitelist_coop" 0 selects the
 * lane-serial form of that kernel (every missing lane walks its own 3K variants; same results).  The
 * pass has no host wait of its own: the five counts are read by humid_get_barcode_status.
 *   humid_whitelist_set: barcodes[n] is a HOST array; duplicates collapse.  n = 0 clears the
 *     whitelist.  HUMID_E_INVALID when barcode_nt is outside 1 .. 32 or a barcode is >= 4^K,
 *     HUMID_E_OVERFLOW for n > 2^30, HUMID_E_NOMEM when an allocation fails; in all three cases the
 *     previous whitelist stays in place and the context usable.
 *   humid_whitelist_info: distinct barcodes (0: no whitelist), K, log2 of the table's slots.  Any
 *     pointer may be NULL.
 *   humid_whitelist_correct: key[n_reads], filtered[n_reads] in; key_out[n_reads] (u64),
 *     status[n_reads] (u8) and counts[5] (reads per status, indexed by the status value) out; host
 *     buffers; any of the three outputs may be NULL.
 *   humid_whitelist_correct_device: the same with DEVICE pointers for key, filtered, key_out and
 *     status; counts stays on the host.  Returns after the stream has drained.
 *     Both return HUMID_E_STATE without a whitelist, and neither touches the results of the last run:
 *     every accessor, humid_get_barcode_status included, still answers for that run afterwards.
 *   humid_dedup_run_keyed_corrected(_device): the corrected keyed run; arguments as
 *     humid_dedup_run_keyed(_device).  HUMID_E_STATE without a whitelist.  A keyed run for every
 *     accessor.
 *   humid_get_barcode_status: the status of the first min(cap, n_reads) reads and the five counts
 *     of the last corrected keyed run.  Either pointer may be NULL.  HUMID_E_STATE unless the last
 *     run was a corrected one. */
#define HUMID_BC_FILTERED  0u
#define HUMID_BC_EXACT     1u
#define HUMID_BC_CORRECTED 2u
#define HUMID_BC_AMBIGUOUS 3u
#define HUMID_BC_UNMATCHED 4u
int humid_whitelist_set(humid_ctx *ctx, const uint64_t *barcodes, uint64_t n, uint32_t barcode_nt);
int humid_whitelist_info(humid_ctx *ctx, uint64_t *n_distinct, uint32_t *barcode_nt,
                         uint32_t *table_log2);
int humid_whitelist_correct(humid_ctx *ctx, const uint64_t *key, const uint8_t *filtered,
                            uint64_t n_reads, uint64_t *key_out, uint8_t *status, uint64_t counts[5]);
int humid_whitelist_correct_device(humid_ctx *ctx, const uint64_t *d_key, const uint8_t *d_filtered,
                                   uint64_t n_reads, uint64_t *d_key_out, uint8_t *d_status,
                                   uint64_t counts[5]);
int humid_dedup_run_keyed_corrected(humid_ctx *ctx, const uint64_t *words, const uint64_t *key,
                                    const uint8_t *filtered, uint64_t n_reads, uint32_t word_nt,
                                    uint32_t distance, uint32_t method, uint32_t *cluster_id,
                                    uint8_t *keep, humid_summary *summary);
int humid_dedup_run_keyed_corrected_device(humid_ctx *ctx, const uint64_t *d_words,
                                           const uint64_t *d_key, const uint8_t *d_filtered,
                                           uint64_t n_reads, uint32_t word_nt, uint32_t distance,
                                           uint32_t method, uint32_t *d_cluster_id, uint8_t *d_keep,
                                           humid_summary *summary);
int humid_get_barcode_status(humid_ctx *ctx, uint8_t *status, uint64_t cap, uint64_t counts[5]);

/* ---- segmented barcode whitelist: one list per segment, every segment corrected on its own -------
 * (STARsolo CB_UMI_Complex with several --soloCBwhitelist, UMI-tools --bc-pattern, the split-pool
 * pipelines: SPLiT-seq, inDrop, BD Rhapsody, sci-RNA-seq.)  A segmented whitelist has S segments,
 * 1 <= S <= 8; segment s has L_s nucleotides, 1 <= L_s <= 10, and a set W_s of distinct packed
 * L_s-mers; K = sum of L_s <= 32.  Segment 0 is the first L_0 nucleotides of the K-nucleotide key
 * (its most significant bits), segment s follows segment s - 1.  For a usable read with key
 * k < 4^K and subkeys k_s, the class c_s of segment s is the correction of the section above of k_s
 * against W_s over L_s nucleotides:
 *   EXACT      k_s in W_s
 *   CORRECTED  exactly one w in W_s at Hamming distance 1: it replaces k_s
 *   AMBIGUOUS  two or more such w
 *   UNMATCHED  none
 * Let m be the number of segments whose class is not EXACT.  With max_inexact (0 .. S) the status is
 *   HUMID_BC_FILTERED   filtered[r] != 0; the key is not read, key_out[r] = 0
 *   HUMID_BC_UNMATCHED  k >= 4^K or m > max_inexact
 *   otherwise the worst class of its segments, UNMATCHED > AMBIGUOUS > CORRECTED > EXACT.
 * key_out[r] is the corrected segments one behind the other for an EXACT or CORRECTED read, k for an
 * AMBIGUOUS or UNMATCHED one.  So S = 1 is humid_whitelist_correct with that one list, and
 * max_inexact = 1 is humid_whitelist_correct against the product list W_0 x ... x W_(S-1), both bit for
 * bit; max_inexact = S allows one substitution in EVERY segment, which no product list expresses.
 * Beside counts[5] a correction leaves a per-segment summary over the usable reads with k < 4^K,
 * whatever max_inexact is: seg_counts[s][c] the reads whose segment s is EXACT / CORRECTED /
 * AMBIGUOUS / UNMATCHED (c = 0 .. 3), inexact_hist[m] the reads by m.
 * On the device: a segment has at most 4^10 values, so humid_whitelist_set_segments works out the
 * answer for EVERY value once, on the device, into one direct-index table per segment (32-bit
 * entries, class << 30 | subkey, at most 4 MB a segment, in HBM and for the usual chemistries in L2):
 * every list entry marks itself exact, adds itself to the hit count of its 3 L_s variants and offers
 * itself as their winner by an atomic minimum, and a second kernel turns the counts into classes.
 * A read is then S independent table reads and no probing, in one pass in front of the unchanged
 * keyed pass, with no host wait of its own.
 *   humid_whitelist_set_segments: seg_nt[n_seg], seg_n[n_seg] and barcodes (the lists one behind the
 *     other, seg_n[s] entries of segment s) are HOST arrays; duplicates in a list collapse.  It
 *     installs the segmented whitelist in place of whatever whitelist the context holds and survives
 *     runs as that of humid_whitelist_set does; humid_whitelist_set, humid_whitelist_discover and a
 *     clear replace it.  HUMID_E_INVALID for n_seg outside 1 .. 8, a segment outside 1 .. 10
 *     nucleotides, K > 32, an empty list, an entry >= 4^L_s or max_inexact > n_seg (HUMID_E_OVERFLOW
 *     for a list of more than 2^30 entries): the previous whitelist stays and the context usable.
 *   humid_whitelist_segments_info: n_seg (0: the whitelist in place is plain or absent), the
 *     nucleotides and the distinct entries of every segment (0 behind the last), max_inexact.  Any
 *     pointer may be NULL.  humid_whitelist_info answers K for a segmented whitelist, the product of
 *     the distinct entries as n_distinct (at most 2^64 - 1) and table_log2 = 0.
 *   With a segmented whitelist in place humid_whitelist_correct(_device) and
 *   humid_dedup_run_keyed_corrected(_device) follow the definition above, and humid_get_barcode_status
 *   answers as for any corrected run; the posterior calls and runs of the next section return
 *   HUMID_E_UNSUPPORTED and humid_whitelist_counts HUMID_E_STATE.
 *   humid_get_barcode_segments: seg_counts (8 rows of 4, rows behind the last segment zero) and
 *     inexact_hist (9 bins) of the last correct call or corrected run over the segmented whitelist in
 *     place, whichever came later.  Either pointer may be NULL.  HUMID_E_STATE before such a call or
 *     once the whitelist was replaced. */
int humid_whitelist_set_segments(humid_ctx *ctx, uint32_t n_seg, const uint32_t *seg_nt,
                                 const uint64_t *seg_n, const uint64_t *barcodes,
                                 uint32_t max_inexact);
int humid_whitelist_segments_info(humid_ctx *ctx, uint32_t *n_seg, uint32_t seg_nt[8],
                                  uint64_t seg_n[8], uint32_t *max_inexact);
int humid_get_barcode_segments(humid_ctx *ctx, uint64_t seg_counts[32], uint64_t inexact_hist[9]);

/* ---- barcode whitelist: ambiguous keys decided by base quality and barcode abundance -------------
 * (Cell Ranger, STARsolo 1MM_multi.)  W, K, key, filtered, the five statuses and key_out are those
 * of the section above; a whitelist must be set.  Three inputs are new:
 *   qual[n_reads * K]  u8, raw Phred+33 bytes: qual[r*K + j] belongs to barcode nucleotide j, j = 0
 *                      the first nucleotide (bits 2(K-1-j) of the key).  Rows of filtered reads are
 *                      never read.  p = min(max(byte - 33, 0), 93) as in humid_consensus, q = min(p, 40).
 *   min_odds           u32 >= 1; 39 is a posterior of at least 0.975.
 * The error weight of a base of quality q is E[q] = floor(2^24 * 10^(-q/10) + 0.5), q = 0 .. 40:
 *   16777216 13326616 10585708 8408526 6679130 5305422 4214246 3347495 2659010 2112126 1677722
 *   1332662 1058571 840853 667913 530542 421425 334749 265901 211213 167772 133266 105857 84085
 *   66791 53054 42142 33475 26590 21121 16777 13327 10586 8409 6679 5305 4214 3347 2659 2112 1678
 * Prior: for w in W, n_w = the usable reads of THIS call whose key equals w (its EXACT reads), and
 * pi_w = n_w + 1.  Per usable read with key k:
 *   k in W: EXACT, as above.
 *   otherwise (a key with bits above 2K included) the candidates are the w in W that differ from k
 *   in exactly one of the K nucleotides, j_w (so a key with bits above 2K has none);
 *     weight(w) = pi_w * E[q of nucleotide j_w]          (< 2^55)
 *     total     = the sum of the weights                 (< 2^62: at most 96 candidates)
 *     best      = the candidate of the largest weight, ties to the smallest barcode value
 *   no candidate: UNMATCHED, key_out = k;
 *   weight(best) >= min_odds * (total - weight(best)), in exact integers: CORRECTED, key_out = best;
 *   otherwise AMBIGUOUS, key_out = k.
 * Consequences: a read with ONE candidate is corrected exactly as by humid_whitelist_correct; the
 * statuses differ from the plain correction only on reads that are AMBIGUOUS there; with all quality
 * bytes equal, no EXACT read and min_odds >= 2 the result equals humid_whitelist_correct bit for
 * bit; the result is made of sums and a maximum over a total order and depends on no order of reads
 * or atomics.  Not handled: barcodes with N (the caller marks such a read filtered), distance 2,
 * insertions / deletions, caller-supplied priors, grouped or sharded runs.
 * On the device: two launches.  The first looks every key up once (one lookup per run of equal keys
 * inside a wave), keeps the slot per read and adds the run lengths into a count per table slot; the
 * second probes only for the reads that missed: the lanes of the wave look the 3K variants of one
 * read up side by side, a hit loads the one quality byte of its nucleotide, and a 64-bit sum and a
 * maximum over the wave decide.  Option "whitelist_coop" 0 selects the lane-serial form.
 *   humid_whitelist_correct_posterior: key, qual, filtered in; key_out, status, summary out; host
 *     buffers; any output may be NULL.  summary.counts are the reads per status, multi the reads
 *     with two or more candidates, rescued those of them that were CORRECTED.
 *   humid_whitelist_correct_posterior_device: the same with DEVICE pointers for key, qual, filtered,
 *     key_out and status.  Both: HUMID_E_STATE without a whitelist, HUMID_E_INVALID for min_odds == 0
 *     or a NULL key / qual / filtered with n_reads > 0; n_reads == 0 is fine.  Like
 *     humid_whitelist_correct they touch nothing of the last run.
 *   humid_dedup_run_keyed_posterior(_device): humid_dedup_run_keyed_corrected(_device) with this
 *     correction in front; a corrected keyed run for every accessor (humid_get_barcode_status
 *     answers for it).  No host wait of its own: the counters are read by the getters.
 *   humid_get_barcode_posterior: multi and rescued of the last run; either pointer may be NULL.
 *     HUMID_E_STATE unless the last run was a posterior one.
 *   humid_whitelist_counts: n_w of the last posterior call or run, whichever came later, for n
 *     caller-given barcodes (a HOST array); 0 for a value that is no whitelist barcode.  The reads
 *     per barcode BEFORE correction.  HUMID_E_STATE before such a call, or once the whitelist was
 *     replaced or cleared after it. */
typedef struct humid_bc_posterior_summary {
    uint64_t counts[5];
    uint64_t multi;
    uint64_t rescued;
} humid_bc_posterior_summary;
int humid_whitelist_correct_posterior(humid_ctx *ctx, const uint64_t *key, const uint8_t *qual,
                                      const uint8_t *filtered, uint64_t n_reads, uint32_t min_odds,
                                      uint64_t *key_out, uint8_t *status,
                                      humid_bc_posterior_summary *summary);
int humid_whitelist_correct_posterior_device(humid_ctx *ctx, const uint64_t *d_key,
                                             const uint8_t *d_qual, const uint8_t *d_filtered,
                                             uint64_t n_reads, uint32_t min_odds, uint64_t *d_key_out,
                                             uint8_t *d_status, humid_bc_posterior_summary *summary);
int humid_dedup_run_keyed_posterior(humid_ctx *ctx, const uint64_t *words, const uint64_t *key,
                                    const uint8_t *qual, const uint8_t *filtered, uint64_t n_reads,
                                    uint32_t word_nt, uint32_t distance, uint32_t method,
                                    uint32_t min_odds, uint32_t *cluster_id, uint8_t *keep,
                                    humid_summary *summary);
int humid_dedup_run_keyed_posterior_device(humid_ctx *ctx, const uint64_t *d_words,
                                           const uint64_t *d_key, const uint8_t *d_qual,
                                           const uint8_t *d_filtered, uint64_t n_reads,
                                           uint32_t word_nt, uint32_t distance, uint32_t method,
                                           uint32_t min_odds, uint32_t *d_cluster_id, uint8_t *d_keep,
                                           humid_summary *summary);
int humid_get_barcode_posterior(humid_ctx *ctx, uint64_t *multi, uint64_t *rescued);
int humid_whitelist_counts(humid_ctx *ctx, const uint64_t *barcodes, uint64_t n,
                           uint32_t *counts_out);

/* ---- barcode whitelist from the data: the abundant barcodes are the cells ------------------------
 * (UMI-tools whitelist, Cell Ranger 2's cell calling, alevin's initial whitelist: for chemistries that
 * ship no list of barcodes.)  Inputs: key[n_reads] (u64), filtered[n_reads] (u8), K = barcode_nt with
 * 1 <= K <= 32, a mode with its param, and merge_ratio.  Keys of filtered reads are never read.  For
 * K < 32 a usable read whose key is >= 4^K is an invalid-key read: it is counted in invalid_reads and
 * takes no further part.  Everything below is exact integer arithmetic.
 *   Counts     n_k = the usable, valid reads with key k; G = the number of distinct such keys.
 *   ORDER      the distinct keys by (n_k descending, key value ascending), ranks 0 .. G-1: a total
 *              order.  n(r) is the count at rank r.
 *   Selection  HUMID_CELLS_TOP, param T >= 1: S = the ranks [0, min(T, G)); a tie at the cut goes to
 *              the smaller barcode value.
 *              HUMID_CELLS_EXPECTED, param X >= 1, after the order-of-magnitude rule of Cell Ranger 2
 *              with rounding conventions of this library (it is NOT claimed to equal Cell Ranger's
 *              result): b = min((X + 50) / 100, G - 1) in integer division, m = n(b); S = every key
 *              with 10 n_k >= m (64-bit).
 *              HUMID_CELLS_MIN_READS, param T >= 1: S = every key with n_k >= T.
 *              G = 0: S is empty.
 *   Merge      merge_ratio R >= 1 (0: no merge).  w in S is an error barcode when some v in S differs
 *              from w in exactly one of the K nucleotides, ranks before w in the ORDER and has
 *              n_v >= R n_w (64-bit product).  All error barcodes are removed.  The rule is evaluated
 *              against S as selected, not iteratively: a barcode that is itself removed still removes
 *              its neighbours, and the result depends on no order of evaluation.
 *   Result     the cells = S minus the error barcodes.  They become the context's whitelist exactly
 *              as if humid_whitelist_set(cells, K) had been called: it survives runs,
 *              humid_whitelist_info answers for it, the reads per barcode of an earlier posterior
 *              call are gone (humid_whitelist_counts: HUMID_E_STATE), and humid_whitelist_correct*,
 *              humid_dedup_run_keyed_corrected* and the posterior forms follow unchanged.  Zero cells
 *              clears the whitelist and returns HUMID_OK.  More than 2^30 cells returns
 *              HUMID_E_OVERFLOW and the previous whitelist stays.
 *   Summary    usable          usable reads
 *              invalid_reads   usable reads with an invalid key
 *              distinct        G
 *              selected        |S| before the merge
 *              merged          error barcodes removed
 *              cells           cells after the merge
 *              threshold_reads the smallest n_k in S, 0 when S is empty
 *              top_reads       n(0), 0 when G = 0
 *              reads_in_cells  the sum of n_k over the cells
 * Refused on the host, before anything moves: HUMID_E_INVALID for K outside 1 .. 32, mode > 2, param 0,
 * or a NULL key or filtered with n_reads > 0; HUMID_E_OVERFLOW for n_reads > 2^31 - 1.  After every
 * refusal or failure the previous whitelist (and the result of an earlier discover call) stays and the
 * context stays usable.  n_reads = 0 is legal: zero cells, the whitelist is cleared.
 * Like humid_whitelist_correct the call touches nothing of the last run: it works in buffers of its
 * own, not in the table humid_keyed_rank_info and the keyed accessors answer from, and every accessor
 * still answers for the last run afterwards.
 * Not handled: knee or density estimates of the number of cells, EmptyDrops-style tests against the
 * ambient profile, distance 2, insertions / deletions, priors from outside, grouped or sharded runs.
 * On the device (kernels_cells.hip.h): one pass over the reads counts them in an open-address table
 * in HBM, the keys in one array and the reads per slot in another (one probe and one atomic add per
 * run of equal keys inside a wave; the table is sized and grown as the key table of a keyed run is; option "cells_table_log2", 4 .. 32, 0 =
 * automatic, sets the size it starts with and never changes a result); the occupied slots are
 * compacted and sorted twice (by key, then stable by the complemented count: the ORDER); the cut is
 * read off the ORDER on the device, and the runs of equal counts in it are the histogram; the members
 * of S are taken in key order, one wave per member looks its 3K variants up in the counting table
 * side by side (option "whitelist_coop" 0: one lane per member), and the survivors, ascending, are
 * inserted into a table built beside the old one.  Work after the first pass is proportional to G;
 * at most four host waits.
 *   humid_whitelist_discover: key and filtered are HOST arrays; summary may be NULL.
 *   humid_whitelist_discover_device: the same with DEVICE pointers for key and filtered (the summary
 *     is written on the host).
 *   humid_get_discovered_cells: the cells in ascending barcode value with their n_k.  *n_out = their
 *     number (call with cap = 0 to size the buffers); writes min(cap, cells) entries.  Any pointer may
 *     be NULL.
 *   humid_get_barcode_count_hist: the pairs (n, number of distinct valid barcodes with exactly n
 *     reads) in ascending n over all G barcodes -- the data of a barcode-rank ("knee") plot -- by the
 *     protocol of humid_get_histogram.
 *     Both getters return HUMID_E_STATE unless the whitelist in place (or, after a call that found no
 *     cell, its absence) was installed by a discover call: humid_whitelist_set and a clear end that,
 *     a discover call that failed or was refused changes nothing. */
#define HUMID_CELLS_TOP       0u
#define HUMID_CELLS_EXPECTED  1u
#define HUMID_CELLS_MIN_READS 2u
typedef struct humid_cells_summary {
    uint64_t usable;
    uint64_t invalid_reads;
    uint64_t distinct;
    uint64_t selected;
    uint64_t merged;
    uint64_t cells;
    uint64_t threshold_reads;
    uint64_t top_reads;
    uint64_t reads_in_cells;
} humid_cells_summary;
int humid_whitelist_discover(humid_ctx *ctx, const uint64_t *key, const uint8_t *filtered,
                             uint64_t n_reads, uint32_t barcode_nt, uint32_t mode, uint64_t param,
                             uint32_t merge_ratio, humid_cells_summary *summary);
int humid_whitelist_discover_device(humid_ctx *ctx, const uint64_t *d_key, const uint8_t *d_filtered,
                                    uint64_t n_reads, uint32_t barcode_nt, uint32_t mode,
                                    uint64_t param, uint32_t merge_ratio,
                                    humid_cells_summary *summary);
int humid_get_discovered_cells(humid_ctx *ctx, uint64_t *barcodes, uint32_t *reads, uint64_t cap,
                               uint64_t *n_out);
int humid_get_barcode_count_hist(humid_ctx *ctx, uint64_t *reads, uint64_t *barcodes, uint64_t cap,
                                 uint64_t *n_out);

/* ---- per-group statistics: how many molecules every group holds ---------------------------------
 * (the UMI count per cell, or per (cell, gene): the count matrix.)  After a successful single-GPU run let G be
 * its number of groups: n_groups as passed to humid_dedup_run_grouped*; after humid_dedup_run_keyed* the number
 * of distinct keys, what humid_get_group_keys reports (G may be 0); a plain run (humid_dedup_run, _device,
 * _bases) counts as ONE group, G = 1.  The leaves are in (group, word) walk order and the cluster ids are
 * numbered on across the groups in group order, so both are one contiguous range per group.  For 0 <= g < G:
 *   leaf_off[g]     walk index of the first leaf whose group is >= g; leaf_off[G] = summary.unique.  The leaves
 *                   of g are [leaf_off[g], leaf_off[g + 1]): an absent group is an empty range, and
 *                   unique[g] = leaf_off[g + 1] - leaf_off[g].
 *   cluster_off[g]  the cluster ids of g are cluster_off[g] + 1 .. cluster_off[g + 1]; cluster_off[0] = 0,
 *                   cluster_off[G] = summary.clusters.  clusters[g] = cluster_off[g + 1] - cluster_off[g], the
 *                   molecules of g, is also the number of reads of g with keep == 1.
 *   reads[g]        (u64) usable reads of g = the sum of count over its leaves.
 *   edges[g]        (u32) neighbour pairs inside g = half the sum of degree over its leaves.
 * The sums over g are summary.usable, .unique, .clusters and .edges.  After a keyed run group g is key
 * humid_get_group_keys()[g], so (key, clusters) is the count table in coordinate form.
 * The statistics are computed on the device by the first of these two calls after a run (an exclusive scan
 * over the leaves, a lower-bound search per group, read from the internal words where the run left them:
 * work proportional to unique + G log unique, whatever the sizes of the groups and the gaps between them)
 * and kept until the next run; the runs themselves do nothing for them.
 *   humid_get_group_stats: host copies.  *n_out = G (call with cap = 0 to size the buffers); writes
 *     min(cap, G) entries of reads / edges and min(cap, G) + 1 entries of leaf_off / cluster_off.  Any pointer
 *     may be NULL.
 *   humid_group_stats_device: the same arrays left in HBM (reads u64[G], leaf_off u32[G + 1],
 *     cluster_off u32[G + 1], edges u32[G]), owned by the context and valid until its next run or
 *     humid_ctx_destroy; complete when the call returns.  Any pointer may be NULL.
 * Both return HUMID_E_STATE before any run and after a multi-GPU pass, a humid_stage_* call or
 * humid_cluster_graph, HUMID_E_INVALID for a NULL context, and HUMID_E_NOMEM when an allocation fails (the
 * context stays usable). */
int humid_get_group_stats(humid_ctx *ctx, uint64_t cap, uint64_t *n_out, uint64_t *reads,
                          uint32_t *leaf_off, uint32_t *cluster_off, uint32_t *edges);
int humid_group_stats_device(humid_ctx *ctx, uint64_t *n_out, const uint64_t **d_reads,
                             const uint32_t **d_leaf_off, const uint32_t **d_cluster_off,
                             const uint32_t **d_edges);

/* ---- the best-scoring read of every cluster: which read of a family survives ---------------------
 * (Picard MarkDuplicates keeps the pair with the largest sum of base qualities, UMICollapse the highest average
 * quality, UMI-tools the highest MAPQ.)  A run's keep[i] marks the FIRST read, in input order, whose word is its
 * cluster's maxLeaf.  This pass, run after it, picks by a caller-defined score instead.  Per read i < n_reads:
 *   words[i]       the caller's words of the run that produced the ids: one uint64, or two when word_nt > 32, in
 *                  the layout of humid_dedup_run.
 *   cluster_id[i], keep[i]   that run's outputs, unmodified.
 *   score[i]       uint32, larger is better.
 * A read with cluster_id == 0 (filtered; after a corrected run also ambiguous and unmatched) is no candidate:
 * neither its score nor its word is read.  For every cluster c let r_c be the one read with keep == 1 and
 * cluster_id == c.  The candidates of c are
 *   scope HUMID_BEST_LEAF (0):     its reads whose word equals words[r_c] -- the reads of the cluster's maxLeaf,
 *                                  so the survivor still carries the most abundant word, as in the reference;
 *   scope HUMID_BEST_CLUSTER (1):  all its reads.
 * (No group array is needed: two reads of ONE cluster with equal words are in the same group.)  The new
 * representative b_c is the candidate with the largest score; ties go to the smallest read index.  Outputs:
 *   keep_out[i]  = (i == b_c) for c = cluster_id[i]; 0 for cluster_id == 0.
 *   rep_out[i]   = b_c, the read's pointer to its family's representative; HUMID_NO_READ for cluster_id == 0.
 *                  May be NULL.
 *   *n_changed   = the number of clusters with b_c != r_c.  May be NULL.
 * So equal scores under scope LEAF give back keep exactly, sum(keep_out) == summary.clusters, and the result is a maximum over a
 * total order: it does not depend on the order the device takes the reads in.
 * Both entry points are valid only after a successful single-GPU humid_dedup_run* (plain, bases, grouped, keyed
 * or corrected) on this context with the same n_reads and word_nt -- the cluster count is that run's; in any
 * other case (no run, a multi-GPU pass, a humid_stage_* call or humid_cluster_graph since) they return
 * HUMID_E_INVALID, as for scope > 1, a NULL buffer and wide words that are not 16-byte aligned on the device.
 * n_reads == 0 returns HUMID_OK.  keep_out may be the same buffer as keep.  Malformed input -- an id above the
 * run's cluster count, a cluster without a read with keep == 1, or with two -- is detected on the device and
 * reported as HUMID_E_INVALID at the pass's one host wait; nothing is then written and no unchecked index followed.
 * The pass launches nothing unless it is called, works in memory of its own, and leaves the context usable and
 * every accessor of the last run valid, whatever it returns.
 * On the device (kernels_best.hip.h): the kept reads claim a table u32[C + 1]; every candidate votes
 * score << 32 | (0xffffffff - i) into a table u64[C + 1] with a 64-bit atomic maximum (runs of equal ids inside
 * a wave vote once); one more pass writes the outputs.
 *   humid_select_best: host buffers.
 *   humid_select_best_device: DEVICE pointers for all arrays; n_changed stays a host pointer.  Returns after
 *     the stream has drained. */
#define HUMID_BEST_LEAF    0u
#define HUMID_BEST_CLUSTER 1u
#define HUMID_NO_READ 0xffffffffu
int humid_select_best(humid_ctx *ctx, const uint64_t *words, const uint32_t *cluster_id,
                      const uint8_t *keep, const uint32_t *score, uint64_t n_reads, uint32_t word_nt,
                      uint32_t scope, uint8_t *keep_out, uint32_t *rep_out, uint64_t *n_changed);
int humid_select_best_device(humid_ctx *ctx, const uint64_t *d_words, const uint32_t *d_cluster_id,
                             const uint8_t *d_keep, const uint32_t *d_score, uint64_t n_reads,
                             uint32_t word_nt, uint32_t scope, uint8_t *d_keep_out, uint32_t *d_rep_out,
                             uint64_t *n_changed);

/* ---- consensus reads: one record per cluster, built from all of its reads --------------------------------------
 * (fgbio CallMolecularConsensusReads, gencore: errors are voted out, qualities reflect the agreement.)  The
 * definition is exact, in integers.  One call handles one LAYER of reads -- one FastQ file; a paired run calls once
 * per file:
 *   bases[n_bytes], quals[n_bytes]   raw ASCII; qualities are Phred+33.
 *   off[n_reads + 1] (u64)           read i owns bytes [off[i], off[i + 1]) of both blobs; len_i = off[i + 1] - off[i].
 *                                    Lengths may differ and may be 0.
 *   cluster_id[n_reads], keep[n_reads]   from any run (also from a sharded pass), keep possibly rewritten by
 *                                    humid_select_best.
 *   n_clusters = C                   passed explicitly: the pass needs no prior run on the context.
 *   min_q in 0 .. 93, cap_q in 1 .. 93.
 * A read with cluster_id == 0 is no member; none of its bytes are read.  r_c is the one read with keep == 1 and
 * cluster_id == c.
 * Votes.  p(byte) = min(max(byte - 33, 0), 93).  Read i casts a vote at column j when j < len_i, its base byte is one
 * of the uppercase A C G T and p(quality byte) >= max(min_q, 1); the vote's weight is p.  Anything else (N, lowercase,
 * IUPAC codes, a quality below the threshold) casts nothing.
 * Output of cluster c: len(r_c) base bytes and as many quality bytes.  For column j let S_b be the sum of the weights
 * and n_b the number of the votes for base b over ALL reads of c (not only those that share the representative's
 * word; reads longer than r_c are cut, shorter ones stop voting):
 *   no vote was cast                     both bytes are r_c's own, verbatim;
 *   the largest S_b is reached twice     'N' and '!' (a tie carries no information; no tie-break rule exists);
 *   otherwise                            the base with the largest S_b, and 33 + min(S_first - S_second, cap_q).
 * So a singleton's consensus is its own record wherever cap_q >= p.
 *   depth[c - 1]  (u32) = reads of c.
 *   errors[c - 1] (u64) = over the decided columns (neither verbatim nor tie) the votes cast minus n_winner.
 *   out_off[C + 1] (u64): the consensus of cluster c is bytes [out_off[c - 1], out_off[c]) of both output blobs
 *                 (cluster-id order; a scan over len(r_c) on the device).
 *   summary: n_clusters = C; total_bytes = out_off[C]; multi_read = clusters with depth >= 2; bases_changed = output
 *     base bytes that differ from r_c's; votes = all votes cast at columns below len(r_c); errors = sum of errors[].
 * Sums are 32-bit: a cluster of more than 46 182 444 reads (93 x that reaches 2^32) returns HUMID_E_OVERFLOW, decided
 * from the member counts before anything is summed (the other of the two possible answers, 64-bit sums, would double
 * the registers of every column for a cluster size no data set has).
 * Malformed input -- an id above C, a cluster with no kept read or with two, off decreasing anywhere, off[n_reads] >
 * n_bytes -- is found on the device and reported as HUMID_E_INVALID at the pass's first host wait; nothing is then
 * written and no unchecked index followed.  min_q / cap_q out of range and a NULL buffer with n_reads > 0 are refused
 * on the host (HUMID_E_INVALID).  n_reads == 0 or C == 0 returns HUMID_OK with an empty result (n_clusters = 0).  The
 * context stays usable and every accessor of the last run valid, whatever the pass returns; it launches nothing
 * unless it is called.  Two host waits: the total that sizes the output (with the checks), and the summary.
 * On the device (kernels_consensus.hip.h): the kept reads claim their clusters as in humid_select_best; the read
 * indices are grouped by cluster (count, scan, cursor scatter -- the order inside a cluster is that of the atomics,
 * which integer sums do not see); one wave per cluster with lanes over 64 columns and a loop over the members; a
 * cluster of more than 1024 reads is cut into pieces of 1024 whose partial sums meet in a table through 32-bit
 * atomic adds before one workgroup decides its columns.
 *   humid_consensus: host buffers.   humid_consensus_device: DEVICE pointers (summary stays a host pointer; may be
 *     NULL); returns after the stream has drained.
 *   humid_get_consensus: host copies of the last successful call's results; any pointer may be NULL; cap_bytes is the
 *     room of cons_bases / cons_quals: cap_bytes < total_bytes with either given returns HUMID_E_INVALID.
 *   humid_consensus_result_device: the same arrays left in HBM (as humid_group_stats_device), owned by the context.
 * The results live in buffers of their own: they last until the next humid_consensus* or humid_duplex_consensus* call
 * (successful or not) or humid_ctx_destroy, and survive any run.  Both getters return HUMID_E_STATE before a successful call. */
typedef struct humid_consensus_summary {
  uint64_t n_clusters, total_bytes, multi_read, bases_changed, votes, errors;
} humid_consensus_summary;
int humid_consensus(humid_ctx *ctx, const uint8_t *bases, const uint8_t *quals, const uint64_t *off, uint64_t n_bytes,
                    const uint32_t *cluster_id, const uint8_t *keep, uint64_t n_reads, uint64_t n_clusters,
                    uint32_t min_q, uint32_t cap_q, humid_consensus_summary *summary);
int humid_consensus_device(humid_ctx *ctx, const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_off,
                           uint64_t n_bytes, const uint32_t *d_cluster_id, const uint8_t *d_keep, uint64_t n_reads,
                           uint64_t n_clusters, uint32_t min_q, uint32_t cap_q, humid_consensus_summary *summary);
int humid_get_consensus(humid_ctx *ctx, uint64_t cap_bytes, uint64_t *out_off, uint8_t *cons_bases,
                        uint8_t *cons_quals, uint32_t *depth, uint64_t *errors);
int humid_consensus_result_device(humid_ctx *ctx, const uint64_t **d_out_off, const uint8_t **d_bases,
                                  const uint8_t **d_quals, const uint32_t **d_depth, const uint64_t **d_errors);

/* ---- duplex consensus reads: the two strands of a cluster as two independent observations ------------------------
 * (fgbio CallDuplexConsensusReads: a base seen on both strands is real, a base seen on one strand only is damage or
 * a PCR error.)  After a strand-symmetric run a cluster holds the reads of both strands of a molecule.  Pooling their
 * votes (humid_consensus) lets a strand of 50 reads outvote a strand of 2; here each strand makes a CAPPED call of its
 * own and the two calls have to agree.  The definition is exact, in integers.  One call produces one output layer (one
 * FastQ file of the pair) from two input layers: the SAME layer S, the file the output belongs to, and the OTHER layer
 * O, the other file; a paired run calls it twice with S and O exchanged.
 *   bases_s / quals_s / off_s[n_reads + 1], n_bytes_s and bases_o / quals_o / off_o, n_bytes_o: raw ASCII, Phred+33,
 *       laid out as for humid_consensus; the lengths of the two layers are independent and may be 0.
 *   cluster_id[n_reads], keep[n_reads]   from any run, keep possibly rewritten by humid_select_best.
 *   strand[n_reads] (u8)                 as humid_get_strands / humid_paired_canonical give it.
 *   n_clusters = C;  min_q in 0 .. 93, strand_cap_q in 1 .. 93, cap_q in 1 .. 93.
 * A read with cluster_id == 0 is no member: none of its bytes and not its strand are read.  A member's strand must be
 * HUMID_STRAND_TOP or HUMID_STRAND_BOTTOM.  r_c is the one member of cluster c with keep == 1.  The cluster's frame is
 * its representative's: a member i with strand[i] == strand[r_c] is in class X and votes with its record of layer S;
 * any other member is in class Y and votes with its record of layer O.  No reverse complement is involved (the other
 * strand's R2 reads the same end in the same direction as this strand's R1), so flipping every strand value changes
 * nothing.
 * Votes are exactly those of humid_consensus: p = min(max(byte - 33, 0), 93), uppercase A C G T only, p >= max(min_q,
 * 1), weight p.  Per column j < L = len_S(r_c) and per class s in {X, Y}: S_b^s the sum of the weights and n_b^s the
 * number of the votes for base b (a member whose voting record is shorter than j + 1 casts nothing there); the class's
 * call is b_s, the base with the largest sum (A before C before G before T among equals), with the margin
 * m_s = min(first - second, strand_cap_q); m_s == 0 (no votes, or a tie) means the class makes no call.  Column j:
 *   no vote in either class                          r_c's own bytes of layer S, verbatim;
 *   m_X > 0, m_Y > 0, b_X == b_Y                     that base, 33 + min(m_X + m_Y, cap_q);
 *   m_X > 0, m_Y > 0, bases differ, m_X != m_Y       the base of the larger margin, 33 + min(|m_X - m_Y|, cap_q);
 *   m_X > 0, m_Y > 0, bases differ, m_X == m_Y       'N' and '!';
 *   exactly one of m_X, m_Y > 0                      that class's base, 33 + min(m_s, cap_q);
 *   votes were cast, neither class calls             'N' and '!'.
 * When every member of every cluster has its representative's strand and strand_cap_q == 93, the outputs and the six
 * shared summary fields are those of humid_consensus on layer S, bit for bit; no byte of layer O is then read.
 * Per cluster (slot c - 1): depth = all its reads; depth_same / depth_other = the sizes of classes X / Y; errors (u64)
 * = over the columns and the classes with m_s > 0 the class's votes minus n of its called base; disagree (u32) = the
 * columns where both classes call different bases; out_off[C + 1] as in humid_consensus.
 * humid_duplex_summary: the first six fields have the names and meanings of humid_consensus_summary (votes: of both
 * classes); duplex_clusters = clusters where both classes are non-empty; both_called = columns where both classes
 * call; agree / disagree = those with the same / with different bases; masked = columns where a vote was cast and 'N'
 * is written.
 * Refusals as in humid_consensus, found on the device and reported at the first host wait, nothing written and no
 * unchecked index followed: HUMID_E_INVALID for an id above C, a cluster without a kept read or with two, off
 * decreasing in either layer, off[n_reads] beyond the bytes given in either layer, a member with a strand above 1;
 * parameters out of range and NULL buffers with n_reads > 0 are refused on the host (HUMID_E_INVALID).
 * HUMID_E_OVERFLOW for a cluster of more than 46 182 444 reads.  n_reads == 0 or C == 0 returns HUMID_OK with an empty
 * result.  The context stays usable and the last run's accessors valid, whatever is returned.  Two host waits.
 * Not part of this pass (strand_cap_q = 40 is fgbio's post-UMI error rate, a convention, not a measurement):
 *   - a minimum number of reads per strand;
 *   - filtering to duplex-only clusters (callers have depth_same / depth_other);
 *   - indel-aware alignment of the members;
 *   - grouped, keyed and sharded runs (the strand-symmetric run has none).
 * On the device (kernels_dconsensus.hip.h): the pass of humid_consensus with the member list of a cluster ordered TOP
 * members first, BOTTOM members last, so that each class is one contiguous range read from one layer; two sets of
 * sums per column; large clusters meet in a table of 16 u32 per column.
 *   humid_duplex_consensus: host buffers.   humid_duplex_consensus_device: DEVICE pointers (summary stays a host
 *     pointer; may be NULL); returns after the stream has drained.
 *   The results go into the consensus result buffers: humid_get_consensus and humid_consensus_result_device answer for
 *   the last successful call of either kind, and "until the next humid_consensus* call" includes the duplex calls and
 *   vice versa.
 *   humid_get_duplex_consensus: depth_same, depth_other, disagree (u32[C] each) and the summary of the last call; any
 *     pointer may be NULL; HUMID_E_STATE unless the last successful consensus call on the context was a duplex one. */
typedef struct humid_duplex_summary {
  uint64_t n_clusters, total_bytes, multi_read, bases_changed, votes, errors;
  uint64_t duplex_clusters, both_called, agree, disagree, masked;
} humid_duplex_summary;
int humid_duplex_consensus(humid_ctx *ctx, const uint8_t *bases_s, const uint8_t *quals_s, const uint64_t *off_s,
                           uint64_t n_bytes_s, const uint8_t *bases_o, const uint8_t *quals_o, const uint64_t *off_o,
                           uint64_t n_bytes_o, const uint32_t *cluster_id, const uint8_t *keep, const uint8_t *strand,
                           uint64_t n_reads, uint64_t n_clusters, uint32_t min_q, uint32_t strand_cap_q, uint32_t cap_q,
                           humid_duplex_summary *summary);
int humid_duplex_consensus_device(humid_ctx *ctx, const uint8_t *d_bases_s, const uint8_t *d_quals_s,
                                  const uint64_t *d_off_s, uint64_t n_bytes_s, const uint8_t *d_bases_o,
                                  const uint8_t *d_quals_o, const uint64_t *d_off_o, uint64_t n_bytes_o,
                                  const uint32_t *d_cluster_id, const uint8_t *d_keep, const uint8_t *d_strand,
                                  uint64_t n_reads, uint64_t n_clusters, uint32_t min_q, uint32_t strand_cap_q,
                                  uint32_t cap_q, humid_duplex_summary *summary);
int humid_get_duplex_consensus(humid_ctx *ctx, uint32_t *depth_same, uint32_t *depth_other, uint32_t *disagree,
                               humid_duplex_summary *summary);

/* ---- optical duplicates: which duplicates of a cluster come from the instrument -------------------------------------
 * (Picard MarkDuplicates READ_PAIR_OPTICAL_DUPLICATES, clumpify dedupe optical: reads of the same tile within a few
 * hundred -- on patterned flowcells a few thousand -- pixels of each other.)  The definition is exact, in integers.
 * Per read i < n_reads:
 *   cluster_id[i], keep[i]   from any run (also from a sharded pass), keep possibly rewritten by humid_select_best.
 *   tile[i]  (u32)           any value is a key (e.g. lane << 24 | tile); HUMID_NO_TILE: the read has no position.
 *   x[i], y[i]  (u32)        every value is legal.
 *   n_clusters = C           passed explicitly: the pass needs no prior run on the context.
 *   distance = D  (u32)      every value is legal.
 * A read with cluster_id == 0 is no member; none of its other fields are read.  Two members i != j are CLOSE when
 *   cluster_id[i] == cluster_id[j],  tile[i] == tile[j] != HUMID_NO_TILE,  |x[i] - x[j]| <= D  and  |y[i] - y[j]| <= D
 * (absolute differences of unsigned values: nothing wraps, no x + D is ever formed).  The OPTICAL GROUPS are the
 * connected components of "close" among the members: the relation is taken transitively, as in Picard's graph form
 * for large duplicate sets, so a chain of reads each within D of the next is one group; a member without a position
 * is a group of its own.  r_c is the one read with keep == 1 and cluster_id == c.  The ORIGIN of a group is r_c when
 * the group holds it, else the smallest read index of the group.  Outputs:
 *   optical_out[i]  (u8)        1 when i is a member and not the origin of its group, else 0.
 *   origin_out[i]   (u32)       the origin of i's group; HUMID_NO_READ for cluster_id == 0.  May be NULL.
 *   per_cluster_out[c - 1] (u32[C])  the optical reads of cluster c.  May be NULL.
 *   summary (may be NULL): n_clusters = C; members = reads with cluster_id != 0; duplicates = members - C; optical =
 *     the sum of per_cluster = the sum over the groups of (size - 1); groups = groups of at least 2 reads;
 *     largest_group = the reads of the largest group (1 when no two members are close, 0 without members).
 *     pcr = duplicates - optical is the caller's to form.
 * The result is a set partition plus a minimum over a total order: it does not depend on the order the device takes
 * the reads or performs its atomics in.
 * Malformed input -- an id above C, a cluster in 1 .. C with no kept read or with two -- is found on the device and
 * reported as HUMID_E_INVALID at the pass's one host wait; nothing is then written and no unchecked index followed
 * (C > n_reads is such a case, refused at once).  n_reads == 0 returns HUMID_OK with a zero summary and so does
 * C == 0, where every read counts as no member (optical 0, origin HUMID_NO_READ).  n_reads > 2^31 - 1 returns
 * HUMID_E_OVERFLOW; a NULL required buffer with n_reads > 0 HUMID_E_INVALID.  The pass launches nothing unless it is
 * called, works in memory of its own, and leaves the context usable and every accessor of the last run valid, whatever
 * it returns.
 * On the device (kernels_optical.hip.h): the kept reads claim their clusters as in humid_select_best; the read indices
 * are sorted by (cluster_id, tile, x) (three stable radix sorts); every sorted position walks forward while cluster
 * and tile are equal and x is no more than D ahead, and joins what it meets with |dy| <= D in a lock-free forest; per
 * root a 64-bit atomic minimum of (kept ? 0 : 1) << 32 | read index picks the origin; one more pass writes the
 * outputs.  Option "optical_walk" bounds the walk of one lane (see humid_ctx_set_option).
 *   humid_optical_duplicates: host buffers.
 *   humid_optical_duplicates_device: DEVICE pointers for all arrays; summary stays a host pointer.  Returns after the
 *     stream has drained. */
#define HUMID_NO_TILE 0xffffffffu
typedef struct humid_optical_summary {
  uint64_t n_clusters, members, duplicates, optical, groups, largest_group;
} humid_optical_summary;
int humid_optical_duplicates(humid_ctx *ctx, const uint32_t *cluster_id, const uint8_t *keep, const uint32_t *tile,
                             const uint32_t *x, const uint32_t *y, uint64_t n_reads, uint64_t n_clusters,
                             uint32_t distance, uint8_t *optical_out, uint32_t *origin_out, uint32_t *per_cluster_out,
                             humid_optical_summary *summary);
int humid_optical_duplicates_device(humid_ctx *ctx, const uint32_t *d_cluster_id, const uint8_t *d_keep,
                                    const uint32_t *d_tile, const uint32_t *d_x, const uint32_t *d_y, uint64_t n_reads,
                                    uint64_t n_clusters, uint32_t distance, uint8_t *d_optical_out,
                                    uint32_t *d_origin_out, uint32_t *d_per_cluster_out, humid_optical_summary *summary);

/* ---- strand-symmetric (duplex) deduplication --------------------------------
 * For duplex UMIs and unstranded paired-end libraries: a molecule read from its other strand arrives with the two
 * halves of its word exchanged.  word_nt = n must be even, 2 <= n <= 64; h = n / 2; a word is A.B, the first h
 * nucleotides followed by the last h (word layout as everywhere: one uint64 for n <= 32, two for n > 32).
 *   mirror      m(A.B) = B.A: on the packed 2n-bit value v, m(v) = ((v & (2^n - 1)) << n) | (v >> n).
 *   canonical   c(w) = min(w, m(w)) by unsigned value.
 *   strand      of a usable read: HUMID_STRAND_TOP when w == c(w) (palindromes w == m(w) included), else
 *               HUMID_STRAND_BOTTOM; a filtered read has HUMID_STRAND_NONE and its word is not read.
 *   leaves      the distinct canonical words of the usable reads, ascending; count = the reads of either strand,
 *               first_read = the smallest read index.
 *   neighbours  two different leaves u, v with min(ham(u, v), ham(u, m(v))) <= distance; lists ascending, every
 *               neighbour once, a leaf never its own neighbour (even when ham(u, m(u)) <= distance).
 * Clusters, cluster_id, keep, the numbering and the summary are those of humid_dedup_run over these leaves and
 * neighbour lists: keep[r] = 1 for the first read whose CANONICAL word is its cluster's maxLeaf.  distance == 0 is the
 * plain run on the canonical words.  (min() in front of a plain run is not enough: an error near the start of a half
 * flips which of w and m(w) is smaller, and two reads one substitution apart then sit n / 2 apart.)
 *
 * humid_paired_canonical*: words_out (may be words; a filtered read's entry is left as it is) and strand_out (u8[N])
 * per read.  Stand-alone: needs no run and leaves the results of the last run alone.
 * humid_dedup_run_paired*: the whole pass.  It counts as a plain run for every accessor: humid_get_leaves (canonical
 * words), humid_get_adjacency, humid_get_clusters, humid_get_histogram and humid_get_group_stats (G = 1) answer for it,
 * and humid_select_best* is valid after it when given the CANONICAL words.  Odd word_nt returns HUMID_E_INVALID,
 * word_nt > 64 HUMID_E_UNSUPPORTED, option "edit_distance" together with distance >= 2 HUMID_E_UNSUPPORTED.
 * n_reads == 0 and an all-filtered input return HUMID_OK with empty results.  Not available for grouped or keyed
 * runs or the multi-GPU pass.  The context stays usable whatever is returned.  The host-buffer form goes the way of
 * humid_dedup_run: its summary carries ms_h2d and ms_d2h, the copies in and out (the device form leaves them 0).
 * On the device (kernels_paired.hip.h): canonical words; the count stage over them; per combination of the pigeonhole
 * plan two sorted-key joins over the leaves, one against themselves and one against their mirrors, verified by
 * popcount; the pairs made unique and given to the graph stage; per-read outputs; strand tallies per cluster.
 * humid_get_strands: after a paired run (HUMID_E_STATE otherwise) strand[i] of the first min(cap, n_reads) reads,
 * top[c - 1] / bottom[c - 1] (u32[clusters]) the reads of each strand of cluster c, and the summary: n_clusters;
 * duplex = clusters with both; top_only / bottom_only; top_reads / bottom_reads.  Any pointer may be NULL.
 *   *_device: DEVICE pointers for the per-read arrays; summary stays a host pointer. */
#define HUMID_STRAND_TOP 0u
#define HUMID_STRAND_BOTTOM 1u
#define HUMID_STRAND_NONE 2u
typedef struct humid_strand_summary {
  uint64_t n_clusters, duplex, top_only, bottom_only, top_reads, bottom_reads;
} humid_strand_summary;
int humid_paired_canonical(humid_ctx *ctx, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads,
                           uint32_t word_nt, uint64_t *words_out, uint8_t *strand_out);
int humid_paired_canonical_device(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                                  uint32_t word_nt, uint64_t *d_words_out, uint8_t *d_strand_out);
int humid_dedup_run_paired(humid_ctx *ctx, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads,
                           uint32_t word_nt, uint32_t distance, uint32_t method, uint32_t *cluster_id, uint8_t *keep,
                           humid_summary *summary);
int humid_dedup_run_paired_device(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                                  uint32_t word_nt, uint32_t distance, uint32_t method, uint32_t *d_cluster_id,
                                  uint8_t *d_keep, humid_summary *summary);
int humid_get_strands(humid_ctx *ctx, uint8_t *strand, uint64_t cap, uint32_t *top, uint32_t *bottom,
                      humid_strand_summary *summary);

/* ---- accumulated runs: one read set fed in chunks ---------------------------------------------------
 * For a read set that does not fit one call: more than 2^31 - 1 reads, more than the device holds at once, or reads
 * that arrive in pieces (a second lane, a top-up run).  An accumulator belongs to a context and has a fixed word_nt
 * (1 .. 64, word layout as everywhere).  Chunks are added; each carries base_index, the GLOBAL index of its first
 * read: read i of the chunk has global index base_index + i.  The index ranges of different chunks must be disjoint;
 * this is not checked (with overlapping ranges keep is unspecified, nothing faults).  The accumulator holds, per
 * distinct usable word, ascending (Trie::walk() order): word, count (summed over all chunks), first_index (u64: the
 * smallest global index of a usable read with that word).  count is a sum and first_index a minimum, so nothing below
 * depends on the order in which the chunks were added.
 * Results.  Let R be all added reads sorted by global index.
 *   humid_accum_finish  the summary (total, usable, unique, clusters, edges, nonsingle; times are 0) of humid_dedup_run
 *                       over R, and that run's leaves, adjacency, clusters and histograms: the context is left as
 *                       humid_stage_graph leaves it, so humid_get_leaves (without first_read: use
 *                       humid_accum_get_leaves), humid_get_adjacency, humid_get_clusters and humid_get_histogram answer
 *                       for the accumulated set, and everything that needs a complete single-GPU run returns
 *                       HUMID_E_STATE.  Option "edit_distance" applies here as in humid_dedup_run.
 *   humid_accum_map     per read of the chunk given: cluster_id = the id that run gives to its word; keep = 1 iff the
 *                       read is usable, its word is its cluster's maxLeaf and its global index equals that leaf's
 *                       first_index.  Filtered reads get 0 / 0.  A usable read whose word the accumulator never saw
 *                       gets 0 / 0 and is counted in *n_unknown (may be NULL); the call still returns HUMID_OK.  The
 *                       chunk need not be one that was added.  The first map after a finish ends the record finish
 *                       published (the chunk is counted in the context's buffers; map reads the accumulator's own
 *                       copy of the per-leaf results).
 * States.  add, finish, map, get_leaves and info return HUMID_E_STATE before humid_accum_begin; map also unless
 * finish succeeded after the last add.  An add after finish is legal: it re-opens the accumulator, and finish must be
 * called again.  get_leaves and info work in every state after begin.  A chunk of 0 reads and a chunk of filtered
 * reads only are legal.  add leaves the context's record as humid_stage_count does.  The accumulator lives in device
 * memory of its own and survives every other call on the context until humid_accum_begin (which empties any earlier
 * accumulator and keeps its memory for the new one), humid_accum_clear (which returns the memory) or humid_ctx_destroy.
 * Limits.  A chunk holds at most 2^31 - 1 reads, the accumulated list at most 2^31 - 1 words, a count at most
 * 2^32 - 1: HUMID_E_OVERFLOW otherwise.  The total number of reads is a u64 with no limit of its own.  word_nt == 0
 * returns HUMID_E_INVALID, word_nt > 64 HUMID_E_UNSUPPORTED, method > 1 HUMID_E_INVALID.  Any failing call leaves the
 * accumulator as it was and the context usable: the merge writes into the second of two buffer sets, and the sets
 * swap only on success.
 * On the device (kernels_accum.hip.h): add = the count stage over the chunk + a merge-path merge of its unique list
 * into the accumulated one (equal words combined; one host wait, for the new number of words); finish = the graph stage
 * over the accumulated list; map = the count stage over the chunk + one binary search per unique word of the chunk +
 * the un-permute of humid_dedup_run.  Every add rewrites the accumulated list.
 * The keyed form has accumulators of its own (next section; a corrected one composes from it, the posterior correction
 * and a whitelist from the data included: the section behind it).  Grouped, paired and multi-GPU forms and the post-run
 * passes are not available for accumulated runs.
 * humid_accum_get_leaves: the first min(cap, unique) entries; *n_out = unique; any pointer may be NULL.
 * humid_accum_info: word_nt, chunks added, reads and usable reads added, unique words, finished (0 / 1).
 *   *_device: DEVICE pointers for the per-read arrays; n_unknown stays a host pointer. */
int humid_accum_begin(humid_ctx *ctx, uint32_t word_nt);
int humid_accum_add(humid_ctx *ctx, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads, uint64_t base_index);
int humid_accum_add_device(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                           uint64_t base_index);
int humid_accum_finish(humid_ctx *ctx, uint32_t distance, uint32_t method, humid_summary *summary);
int humid_accum_map(humid_ctx *ctx, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads, uint64_t base_index,
                    uint32_t *cluster_id, uint8_t *keep, uint64_t *n_unknown);
int humid_accum_map_device(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                           uint64_t base_index, uint32_t *d_cluster_id, uint8_t *d_keep, uint64_t *n_unknown);
int humid_accum_get_leaves(humid_ctx *ctx, uint64_t *word, uint32_t *count, uint64_t *first_index, uint64_t cap,
                           uint64_t *n_out);
int humid_accum_info(humid_ctx *ctx, uint32_t *word_nt, uint64_t *chunks, uint64_t *total, uint64_t *usable,
                     uint64_t *unique, uint32_t *finished);
int humid_accum_clear(humid_ctx *ctx);

/* ---- keyed accumulated runs: per-key deduplication of a read set fed in chunks ---------------------------
 * humid_dedup_run_keyed for a read set that does not fit one call: every read carries a 64-bit key (a cell barcode)
 * beside its word, and words are compared within one key only.  humid_accum_begin_keyed opens the accumulator: word_nt
 * is 1 .. 32 (one uint64 per word; above 32 HUMID_E_UNSUPPORTED, 0 HUMID_E_INVALID); key_nt = 0 makes every 64-bit
 * value a legal key; with key_nt = 1 .. 32 the caller promises keys < 4^key_nt (key_nt > 32: HUMID_E_INVALID), which
 * lets a key and a word of key_nt + word_nt <= 32 nucleotides share one uint64 on the device.  A usable read with a
 * larger key makes add / map return HUMID_E_INVALID, the accumulator as it was and the context usable, as a group
 * >= n_groups does in a grouped run.  Keys of filtered reads are never read.
 * A context holds ONE accumulator: either begin empties the earlier one of either kind and keeps its memory.  The plain
 * add / map / get_leaves on a keyed accumulator, and the keyed ones on a plain accumulator, return HUMID_E_STATE;
 * humid_accum_finish, humid_accum_info (unique = distinct (key, word) pairs) and humid_accum_clear serve both kinds.
 * The list.  Per distinct (key, word) of the usable reads, ascending by key (unsigned), then word: count (summed over
 * all chunks) and first_index (the smallest global index, u64).  Nothing depends on the order of the adds.
 * Results.  Let R be all added reads sorted by global index.
 *   humid_accum_finish  the summary, leaves, adjacency, clusters and histograms of humid_dedup_run_keyed over R (option
 *                       "edit_distance" applies as there), left as after a plain finish: humid_get_leaves gives the
 *                       caller's words, the group field stripped, and no first_read.  Beyond a plain finish,
 *                       humid_get_group_keys, humid_get_leaf_groups and humid_get_group_stats / humid_group_stats_device
 *                       answer for that run, until the first map ends the record (as the adjacency does).  The group
 *                       statistics carry the reads in 32 bits: beyond 2^32 - 1 accumulated usable reads they return
 *                       HUMID_E_UNSUPPORTED.  After a PLAIN finish nothing changes: they return HUMID_E_STATE.
 *   humid_accum_map_keyed  per read of the chunk given: cluster_id = the id that run gives to its (key, word); keep = 1
 *                       iff the read is usable, its entry is its cluster's maxLeaf and its global index is the entry's
 *                       first_index.  Filtered reads get 0 / 0.  A usable read whose (key, word) was never added -- a
 *                       known word under an unseen key included -- gets 0 / 0 and is counted in *n_unknown.
 * States, limits and failures are those of the plain accumulator: 2^31 - 1 reads per chunk, 2^31 - 1 entries, counts
 * below 2^32; a failing call changes nothing.
 * Whitelist correction composes, chunk by chunk: humid_whitelist_correct* over the chunk's keys, then add / map key_out
 * with filtered | (status >= HUMID_BC_AMBIGUOUS).  The result is humid_dedup_run_keyed_corrected over R.  The posterior
 * correction and humid_whitelist_discover* need counts over the whole read set: those counts are fed in chunks as well
 * (next section: humid_cells_* gives the discovered whitelist, humid_whitelist_prior_* the posterior's prior), in a pass
 * over the chunks BEFORE the one that corrects and adds them.
 * On the device: one kernel per chunk packs (key, word) into an entry and checks the key; the count stage, the merge and
 * the lookup of the plain accumulator run over entries.  finish ranks the keys off the sorted list (a flag where the
 * key changes, one scan) at the cost of ONE more host wait -- the number of distinct keys chooses the group field --
 * and runs the graph stage as a keyed pass over rank << 2 * word_nt | word.
 * humid_accum_get_leaves_keyed: the first min(cap, unique) entries; *n_out = unique; any pointer may be NULL.
 * humid_accum_keyed_info: key_nt, uint64 per entry on the device (1 or 2), distinct keys (after a finish; 0 before).
 *   *_device: DEVICE pointers for the per-read arrays; n_unknown stays a host pointer. */
int humid_accum_begin_keyed(humid_ctx *ctx, uint32_t word_nt, uint32_t key_nt);
int humid_accum_add_keyed(humid_ctx *ctx, const uint64_t *words, const uint64_t *key, const uint8_t *filtered,
                          uint64_t n_reads, uint64_t base_index);
int humid_accum_add_keyed_device(humid_ctx *ctx, const uint64_t *d_words, const uint64_t *d_key, const uint8_t *d_filtered,
                                 uint64_t n_reads, uint64_t base_index);
int humid_accum_map_keyed(humid_ctx *ctx, const uint64_t *words, const uint64_t *key, const uint8_t *filtered,
                          uint64_t n_reads, uint64_t base_index, uint32_t *cluster_id, uint8_t *keep, uint64_t *n_unknown);
int humid_accum_map_keyed_device(humid_ctx *ctx, const uint64_t *d_words, const uint64_t *d_key, const uint8_t *d_filtered,
                                 uint64_t n_reads, uint64_t base_index, uint32_t *d_cluster_id, uint8_t *d_keep,
                                 uint64_t *n_unknown);
int humid_accum_get_leaves_keyed(humid_ctx *ctx, uint64_t *key, uint64_t *word, uint32_t *count, uint64_t *first_index,
                                 uint64_t cap, uint64_t *n_out);
int humid_accum_keyed_info(humid_ctx *ctx, uint32_t *key_nt, uint32_t *entry_words, uint64_t *n_keys);

/* ---- barcode counts fed in chunks: the whitelist from the data and the posterior's prior over all chunks ------------
 * What a chunked single-cell run needs beside the keyed accumulator: the reads per barcode over the WHOLE read set.
 *
 * The barcode counter.  Let R be the concatenation of all chunks added since humid_cells_begin, in any order.
 * humid_cells_finish(mode, param, merge_ratio) gives exactly what humid_whitelist_discover(R, barcode_nt, mode, param,
 * merge_ratio) gives: the summary, the installed whitelist (a segmented one dropped), humid_get_discovered_cells,
 * humid_get_barcode_count_hist and that call's consequences for humid_whitelist_info and humid_whitelist_counts.  Counts
 * are sums: no result depends on the order or the cut of the chunks.
 * States.  finish does not consume the counter: it may be called again with another mode, param or ratio (its work is
 * proportional to the distinct barcodes), and an add after a finish is legal.  Every call returns HUMID_E_STATE before
 * begin.  begin empties an earlier counter and keeps its memory, clear returns the memory.  The counter lives in
 * buffers of its own: a one-shot humid_whitelist_discover*, a run of any kind and a keyed or plain accumulator on the
 * same context do not disturb it, and it disturbs none of them; add and finish touch nothing of the last run, as
 * discover does.
 * Limits.  barcode_nt outside 1 .. 32, mode > 2, param == 0 or a NULL buffer with n_reads > 0 return HUMID_E_INVALID, a
 * chunk of more than 2^31 - 1 reads HUMID_E_OVERFLOW: refused on the host before anything moves, the counter as it was.
 * The total number of reads is a u64 with no limit.  One barcode's count may not exceed 2^31 - 1 (the merge's 64-bit
 * product and the posterior's weights rely on it): the add that passes it returns HUMID_E_OVERFLOW.  After that, or after
 * an allocation or HIP failure during an add, the counter is INVALID: add, finish and info return HUMID_E_STATE until
 * the next begin; the context and the whitelist in place stay usable and unchanged.  A chunk of 0 reads and a chunk of
 * filtered reads only are legal.
 * On the device (kernels_cells.hip.h): the counting table of humid_whitelist_discover, kept from add to add.  A run of
 * equal keys whose head finds no slot within the probe bound marks its reads pending instead of ending the pass; the
 * host's one wait per sweep reads the pending reads, the slots claimed and the overflow flag, grows the table into
 * fresh buffers (16 times the slots, at most to the smallest power of two at or above 2 (distinct + pending), where the
 * probe bound is the capacity) and sweeps the pending reads alone: every usable valid read is counted exactly once.
 * An add that leaves the table more than half full grows it as well.  Option "cells_table_log2" sets the size a counter
 * starts with (0: 2^16 slots) and never changes a result.  finish compacts the table and runs the rest of the discovery.
 *   humid_cells_info: barcode_nt, chunks, reads, usable reads and invalid reads added, distinct barcodes, log2 of the
 *     table's slots, growths since begin.  Any pointer may be NULL.
 *   humid_cells_add_device: DEVICE pointers for key and filtered.
 *
 * The prior.  humid_whitelist_prior_begin needs a plain whitelist in place (HUMID_E_STATE without one,
 * HUMID_E_UNSUPPORTED over a segmented one, as the posterior calls) and zeroes reads per barcode of its own -- not those
 * of the one-shot posterior calls and runs, which stay what they are.  humid_whitelist_prior_add adds, per whitelist
 * barcode w, the usable reads of the chunk whose key equals w; n_w <= 2^31 - 2, beyond it the add returns
 * HUMID_E_OVERFLOW and the prior is invalid (HUMID_E_STATE until the next begin).  Let R be the concatenation of the
 * chunks given to prior_add.  For a chunk C (usually one of them, in any order)
 * humid_whitelist_correct_posterior_prior(C) writes for every read of C the key_out and status that
 * humid_whitelist_correct_posterior(R) writes for that read; its summary counts the reads of C alone, so over a
 * partition of R the summaries add up to the one-shot summary (counts, multi, rescued).  humid_whitelist_counts then
 * answers the accumulated n_w (until a one-shot posterior call or run comes later: then that call's).
 * The prior dies with the table it indexes: once humid_whitelist_set, _set_segments, _discover*, humid_cells_finish or a
 * clear has run, the prior calls return HUMID_E_STATE until the next humid_whitelist_prior_begin.
 * On the device (kernels_wlpost.hip.h): add is the counting half of the prior pass (one atomic per run of equal keys,
 * whose old value guards the limit); the correction is its lookup half, then the decision pass unchanged over the
 * accumulated counts.
 *   *_device: DEVICE pointers for the per-read arrays (the summary is written on the host).
 *
 * A whole chunked single-cell run: humid_cells_begin / _add per chunk / _finish (only without a shipped whitelist);
 * humid_whitelist_prior_begin / _add per chunk (only for the posterior correction); per chunk the correction and
 * humid_accum_add_keyed; humid_accum_finish; per chunk humid_accum_map_keyed. */
int humid_cells_begin(humid_ctx *ctx, uint32_t barcode_nt);
int humid_cells_add(humid_ctx *ctx, const uint64_t *key, const uint8_t *filtered, uint64_t n_reads);
int humid_cells_add_device(humid_ctx *ctx, const uint64_t *d_key, const uint8_t *d_filtered, uint64_t n_reads);
int humid_cells_finish(humid_ctx *ctx, uint32_t mode, uint64_t param, uint32_t merge_ratio, humid_cells_summary *summary);
int humid_cells_info(humid_ctx *ctx, uint32_t *barcode_nt, uint64_t *chunks, uint64_t *reads, uint64_t *usable,
                     uint64_t *invalid_reads, uint64_t *distinct, uint32_t *table_log2, uint32_t *n_grown);
int humid_cells_clear(humid_ctx *ctx);
int humid_whitelist_prior_begin(humid_ctx *ctx);
int humid_whitelist_prior_add(humid_ctx *ctx, const uint64_t *key, const uint8_t *filtered, uint64_t n_reads);
int humid_whitelist_prior_add_device(humid_ctx *ctx, const uint64_t *d_key, const uint8_t *d_filtered, uint64_t n_reads);
int humid_whitelist_correct_posterior_prior(humid_ctx *ctx, const uint64_t *key, const uint8_t *qual, const uint8_t *filtered,
                                            uint64_t n_reads, uint32_t min_odds, uint64_t *key_out, uint8_t *status,
                                            humid_bc_posterior_summary *summary);
int humid_whitelist_correct_posterior_prior_device(humid_ctx *ctx, const uint64_t *d_key, const uint8_t *d_qual,
                                                   const uint8_t *d_filtered, uint64_t n_reads, uint32_t min_odds,
                                                   uint64_t *d_key_out, uint8_t *d_status,
                                                   humid_bc_posterior_summary *summary);

/* ---- results of the last run, per unique word in Trie::walk() order ---------
 * (what a caller would read through Result<NLeaf>{leaf,path}, src/humid.cc:117,178,307;
 * NLeaf src/leaf.h:6-9; Cluster src/cluster.h:12-18).  Host output buffers sized by
 * summary.unique / 2*summary.edges / summary.clusters; any pointer may be NULL. */
int humid_get_leaves(humid_ctx *ctx, uint64_t *word, uint32_t *count, uint32_t *first_read,
                     uint32_t *degree, uint32_t *cluster_id, uint8_t *is_max_leaf);
int humid_get_adjacency(humid_ctx *ctx, uint32_t *nbr_off /* unique+1 */,
                        uint32_t *nbr_idx /* 2*edges, each list ascending */);
int humid_get_clusters(humid_ctx *ctx, uint64_t *size, uint32_t *max_count,
                       uint32_t *max_leaf /* walk index of Cluster::maxLeaf */);

/* Histograms of the last run: runStatistics src/humid.cc:301-315 and clusterStats
 * src/cluster.cc:89-95 -> counts.dat / neigh.dat / clusters.dat.
 * which: 0 = leaf->count, 1 = neighbours.size(), 2 = Cluster::size.
 * Writes up to cap (key,value) pairs in ascending key order; *n_out = bins found
 * (call with cap = 0 to size the buffers). */
int humid_get_histogram(humid_ctx *ctx, uint32_t which, uint64_t *keys, uint64_t *values,
                        uint64_t cap, uint64_t *n_out);

/* ---- clustering over an explicit neighbour graph ----------------------------
 * Replaces findClusters (src/humid.cc:167-193) + assignDirectionalCluster /
 * assignMaxCluster (src/cluster.h:26-36) for a caller that built NLeaf::neighbours
 * itself (as tests/test_cluster.cc:11-14 does with link()): leaves are walked in
 * index order, neighbour lists are scanned in the order given.
 * count[U]; nbr_off[U+1], nbr_idx[nbr_off[U]] (CSR, host).  Out: leaf_cluster[U]
 * (ids 1..C), and per cluster id c at slot c-1: size, max_count, max_leaf.
 * cl_* buffers must hold U entries; *n_clusters = C.  Neighbour lists must be symmetric (b in
 * a's list <=> a in b's, as link() and src/humid.cc:121-122 produce) and two linked leaves may
 * not both have count 0 (the reference's maxNeighbour_ never terminates on that input):
 * HUMID_E_INVALID otherwise. */
int humid_cluster_graph(humid_ctx *ctx, const uint32_t *count, const uint32_t *nbr_off,
                        const uint32_t *nbr_idx, uint32_t n_leaves, uint32_t method,
                        uint32_t *leaf_cluster, uint64_t *cl_size, uint32_t *cl_max_count,
                        uint32_t *cl_max_leaf, uint32_t *n_clusters);

/* ---- stages of the same path, for the multi-GPU driver --------------------------
 * One process per GPU (humid_amd/sharded.py, torch.distributed over RCCL): the packed words of
 * all ranks are all-gathered, every rank counts the words of ONE value range
 * (humid_stage_count), the per-range unique arrays are all-gathered (ranges are disjoint and
 * ordered, so their concatenation is Trie::walk() order), neighbours + clusters run over that
 * array (humid_stage_graph) and every rank emits the per-read results of the words it owns
 * (humid_stage_map; 0 elsewhere, so a sum over ranks is the answer).  All pointers are DEVICE
 * pointers unless noted; every call returns after the context's stream has drained.  The
 * reference has no counterpart (it is single-process); semantics per read are those of
 * humid_dedup_run. */

/* usable reads per top-`bits` bin of the word -> d_hist[1 << bits] (u32), for range splitters */
int humid_stage_histogram(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered,
                          uint64_t n_reads, uint32_t word_nt, uint32_t bits, uint32_t *d_hist);
/* Trie::add for the reads whose word is in [range_lo, range_hi] (inclusive); expected_reads =
 * upper bound of such reads (0 = n_reads) sizes the table.  n_unique/n_usable: host outputs. */
int humid_stage_count(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered,
                      uint64_t n_reads, uint32_t word_nt, uint64_t range_lo, uint64_t range_hi,
                      uint64_t expected_reads, uint64_t *n_unique, uint64_t *n_usable);
/* device pointers (owned by ctx, valid until the next stage_count) of this range's unique words
 * in ascending order, their counts and first read indices */
int humid_stage_unique(humid_ctx *ctx, const uint64_t **d_word, const uint32_t **d_count,
                       const uint32_t **d_first);
/* findHammingNeighbours + findClusters over an ascending unique array; *d_cluster_id /
 * *d_is_max: device arrays (owned by ctx) in the same order.  summary: host. */
int humid_stage_graph(humid_ctx *ctx, const uint64_t *d_g_word, const uint32_t *d_g_count,
                      uint64_t n_unique, uint32_t word_nt, uint32_t distance, uint32_t method,
                      const uint32_t **d_cluster_id, const uint8_t **d_is_max,
                      humid_summary *summary);
/* per-read (cluster_id, keep) for the reads counted by the preceding humid_stage_count, given
 * the cluster ids / maxLeaf flags of ITS unique words (local order); other reads get 0 */
int humid_stage_map(humid_ctx *ctx, const uint32_t *d_local_cluster_id,
                    const uint8_t *d_local_is_max, uint64_t n_reads, uint32_t *d_cluster_id,
                    uint8_t *d_keep);

/* Dense variant of humid_stage_count for a rank of a multi-GPU run: the usable reads of the rank's
 * value range are compacted in read order and counted with the LDS-partitioned tables, exactly like
 * a single-GPU read set.  shard_begin[n_shards+1] (host): the home shards of the gathered reads;
 * counts[q] (host, out) = this rank's reads in shard q = split sizes of the result all-to-all.
 * humid_stage_unique / humid_stage_graph* follow as usual; humid_stage_map_dense then yields the
 * packed results (cluster_id | keep << 31) of those reads in the same dense order, i.e. already
 * laid out as the per-shard streams. */
int humid_stage_count_dense(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered,
                            uint64_t n_reads, uint32_t word_nt, uint64_t range_lo, uint64_t range_hi,
                            const uint64_t *shard_begin, uint32_t n_shards, uint64_t *counts,
                            uint64_t *n_unique, uint64_t *n_usable);
int humid_stage_map_dense(humid_ctx *ctx, const uint32_t *d_local_cluster_id,
                          const uint8_t *d_local_is_max, const uint32_t **d_packed,
                          uint64_t *n_packed);

/* Partitioned neighbour search.  Every rank holds the whole ascending unique array (after the
 * all-gather of the per-range arrays); rank part_rank of part_world finds the pairs whose first
 * element lies in its slice -- an equal slice of the positions for the prefix combination, the
 * words whose combination key falls into its part of the key space for the sorted combinations.
 * The union over the ranks is every neighbour pair exactly once.  *d_edges: device array (owned by
 * ctx) of (smaller index << 32 | larger index).  The shares are all-gathered and handed to
 * humid_stage_graph_edges, which is humid_stage_graph with the pairs given instead of searched. */
int humid_stage_pairs(humid_ctx *ctx, const uint64_t *d_g_word, uint64_t n_unique, uint32_t word_nt,
                      uint32_t distance, uint32_t part_rank, uint32_t part_world,
                      const uint64_t **d_edges, uint64_t *n_edges);
int humid_stage_graph_edges(humid_ctx *ctx, const uint64_t *d_g_word, const uint32_t *d_g_count,
                            uint64_t n_unique, const uint64_t *d_edges, uint64_t n_edges,
                            uint32_t word_nt, uint32_t distance, uint32_t method,
                            const uint32_t **d_cluster_id, const uint8_t **d_is_max,
                            humid_summary *summary);

/* Edit distance (-e) on several GPUs (all-gather mode): humid_stage_pairs_edit = this rank's share of
 * the Levenshtein neighbour search (every part_world-th join of the shifted-segment search) over the
 * replicated unique array; shares may repeat a pair, so the gathered list goes through
 * humid_stage_unique_edges (sorted, duplicate-free) before humid_stage_graph_edges. */
int humid_stage_pairs_edit(humid_ctx *ctx, const uint64_t *d_g_word, uint64_t n_unique, uint32_t word_nt,
                           uint32_t distance, uint32_t part_rank, uint32_t part_world,
                           const uint64_t **d_edges, uint64_t *n_edges);
int humid_stage_unique_edges(humid_ctx *ctx, const uint64_t *d_edges, uint64_t n_edges, uint64_t n_unique,
                             const uint64_t **d_unique_edges, uint64_t *n_unique_edges);

/* Result return without N-sized collectives.  The owner of a word computes the results of its
 * reads; the reads' home ranks need them.  Both sides know the same predicate (value ranges), so
 * the streams carry no indices:
 *   humid_stage_owned_results (owner):  packed results (cluster_id | keep << 31) of all reads this
 *     context counted, dense, in read order; counts[q] = how many fall into
 *     [shard_begin[q], shard_begin[q+1]) -- the split sizes of an all-to-all send.
 *   humid_stage_owner_perm (home rank): for its own reads, the owner of each (by range) and the
 *     stable owner-major order: *d_perm[k] = local read of the k-th received result,
 *     counts[o] = reads owned by rank o -- the split sizes of the all-to-all receive.
 *   humid_stage_scatter (home rank):    writes cluster_id/keep of the received stream (0 for
 *     filtered reads).
 * shard_begin, range_lo/hi, counts: host arrays; the rest device pointers (owned by ctx where
 * returned through **).  Requires the global-table count variant on the owner side. */
int humid_stage_owned_results(humid_ctx *ctx, const uint32_t *d_local_cluster_id,
                              const uint8_t *d_local_is_max, const uint64_t *shard_begin,
                              uint32_t n_shards, const uint32_t **d_packed, uint64_t *counts);
int humid_stage_owner_perm(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered,
                           uint64_t n_reads, const uint64_t *range_lo, const uint64_t *range_hi,
                           uint32_t n_ranks, const uint32_t **d_perm, uint64_t *counts);
/* the same for words of word_nt nucleotides (33 .. 64: two uint64 per read, ranges of heads; <= 32: as above) */
int humid_stage_owner_perm_wide(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered,
                                uint64_t n_reads, uint32_t word_nt, const uint64_t *range_lo, const uint64_t *range_hi,
                                uint32_t n_ranks, const uint32_t **d_perm, uint64_t *counts);
int humid_stage_scatter(humid_ctx *ctx, const uint32_t *d_perm, const uint32_t *d_packed,
                        uint64_t n_recv, uint64_t n_reads, uint32_t *d_cluster_id, uint8_t *d_keep);

/* ---- exchange mode: words travel to the owner of their VALUE range --------------------------
 * (humid_amd/sharded.py, mode "exchange".)  Instead of the all-gather of every word to every
 * rank, each usable read's word goes to the rank that owns its value range (all-to-all, ranges
 * from an all-reduced histogram), that rank counts it (humid_stage_count_dense over the received
 * array), and candidate neighbours meet per pigeonhole combination: the prefix combination is
 * local to a value range (ranges are cut at prefix boundaries: use at most *prefix_bits histogram
 * bits), for every other combination the unique words travel once more, to the rank that owns
 * their combination key (hash of the key; a bucket is never split).  Pairs carry GLOBAL unique
 * indices (rank offset + local walk index); only the pairs -- about 2 % of the reads -- and the
 * counts of their endpoints are replicated, and clustered as a compact graph.
 *   humid_stage_plan_info:   combinations of the pigeonhole plan for plan_unique words in total (all
 *     ranks pass the same number) and the bits of the shortest prefix combination.  Host arithmetic
 *     only: ctx may be NULL (then the automatic plan is reported and no GPU is needed).
 *   humid_stage_combo_route: (word, id | count << 32) items of this rank's ascending unique array
 *     (id = id_base + index) in destination-major order, *d_items[2k] = word, [2k+1] = id | count<<32;
 *     counts[q] = items for rank q.
 *   humid_stage_pairs_keyed: the neighbour pairs among n_items items that share the bucket of
 *     `combo` and were not already found by an earlier combination, as 16-byte records
 *     *d_records[2k] = (smaller id << 32 | larger id), [2k+1] = count(smaller) | count(larger) << 32.
 *     interleaved = 1: d_items as above (any order; d_count ignored); interleaved = 0: a plain
 *     ascending word array with ids id_base + index and counts d_count (combination 0 only).
 *   humid_stage_compact_nodes: the distinct endpoints of an edge list (ascending), the same edges
 *     over positions in that list and (record_stride 2: the records above) the endpoints' counts --
 *     the input of humid_stage_graph_edges for a graph that leaves out the singletons (every
 *     singleton is its own cluster and its own maxLeaf).  record_stride 1: plain (a << 32 | b) edges.
 *   humid_stage_route_words: the words of this rank's usable reads in the owner-major order of the
 *     preceding humid_stage_owner_perm (the all-to-all send buffer).
 *   humid_stage_exchange_ids: cluster id + maxLeaf flag of this rank's unique words (global walk
 *     indices id_base ..) from the compact graph's results; ids count the cluster-creating leaves
 *     before a leaf in the WHOLE walk (src/humid.cc:177-180): singletons + compact creators.
 * humid_stage_count_dense accepts d_filtered = NULL: every read is usable and lies in
 * [range_lo, range_hi] (checked); the array is counted as it stands and the range only shapes the
 * word-ordered LDS buckets. */
/* Which road the pairs of the last run / graph stage took (option "pair_split", default 1): a pair whose two ends have
 * no other pair is settled straight from the pair list (*pairs_direct), the others go through the compact graph
 * (*pairs_graph); pairs_direct + pairs_graph = the summary's edges.  *full_graph_built: the graph over ALL pairs exists
 * in the context -- 1 after a run that did not split, else 0 until an accessor (humid_get_leaves / _adjacency /
 * _clusters / _histogram) has asked for it; the run's results never depend on it.  Any pointer may be NULL. */
int humid_graph_split_info(humid_ctx *ctx, uint64_t *pairs_direct, uint64_t *pairs_graph, uint32_t *full_graph_built);
/* How the compact graph stage of the last run made its bucket orders (option "group_records", default 1), counted over
 * all attempts of the stage: *searched_on_records = groupings that moved 8-byte records (squeezed word, walk index), had
 * the combination's search in them and stored no order; *orders_stored = bucket orders written to memory (a grouping
 * on 12-byte pairs or a sort; with a search in it or without).  Any pointer may be NULL. */
int humid_group_records_info(humid_ctx *ctx, uint32_t *searched_on_records, uint32_t *orders_stored);
/* The host waits of the last mutating call (the calls humid_get_run_roads speaks of): *host_waits = how often the host
 * waited for counters the device published, over all attempts and retries of the call; *overlapped = those waits that
 * had kernels queued between the publishing kernel and the wait, so that the GPU had work while the host read and
 * decided.  With option "overlap_waits" (default 1) the wait behind the record count and the wait behind the split of
 * the pairs are of that kind; the fetch of the rest graph's node count beside the small-component kernel is with
 * either value.  Host stores only: no device work, no result depends on it.  Any pointer may be NULL.  HUMID_E_STATE
 * before the first successful mutating call and after a failed one. */
int humid_wait_overlap_info(humid_ctx *ctx, uint32_t *host_waits, uint32_t *overlapped);
/* How the last mutating call was timed.  stamps_used: 1 = its ms_total and ms_k_insert are differences of device
 * stamps and the call recorded none of the four events (option "device_stamps").  stamps[4]: the raw stamps, ticks of
 * 10 ns -- pass start, count kernel start, count kernel end, pass end; also filled (beside the summary's event times)
 * for a pass on the record road with "kernel_timing" = 1, whose kernels store them all the same; zeros where the pass
 * stored none.  event_records: the hipEventRecord calls the call made, counted on the host.  Any pointer may be NULL.
 * HUMID_E_STATE before the first successful mutating call and after a failed one. */
int humid_stamp_info(humid_ctx *ctx, uint32_t *stamps_used, uint64_t stamps[4], uint32_t *event_records);
/* Which attempts the last mutating call (a run, humid_accum_add / _finish / _map, a humid_stage_* call that counts or
 * builds a graph) threw away and took again, in the order they happened.  A record the host keeps while it decides:
 * it costs the GPU nothing and changes no result.  One event per occurrence:
 *   HUMID_ROAD_PART_PADDED_REDO  count stage: a padded coarse bin of the partition outgrew its room; the exact
 *                                partition from then on
 *   HUMID_ROAD_ORDERS_REDONE     compact graph stage: a padded coarse bin of a bucket order was full; every order
 *                                is made again with exact bins, from then on
 *   HUMID_ROAD_REGIONS_REGROWN   compact graph stage: an append region of the pair list was full; more room
 *   HUMID_ROAD_FAR_TILES         compact graph stage: a bucket is longer than the bounded walk; the tiles made the
 *                                list of its far pairs and the search was taken again behind them
 *   HUMID_ROAD_CSR_TILES         per-unique-word graph (option compact_graph 0, humid_accum_finish, humid_stage_graph):
 *                                the tiles completed the buckets beyond the walk
 *   HUMID_ROAD_JOIN_PIECES       a candidate join of the edit-distance or strand-symmetric search cut its runs of
 *                                equal keys into pieces (one event per such join)
 * n_events counts all of them; events[] holds the first HUMID_ROADS_MAX.  graph_attempts: passes through the retry
 * loop of the compact graph stage (1 = nothing was retried; 0 = that stage did not run).  The lazy full graph of the
 * accessors records nothing, and no accessor changes the record.  A stage call that leaves the context's state as it
 * is (humid_stage_pairs_edit) adds its events to the record of the call before it.  HUMID_E_STATE before the first
 * successful mutating call and after a failed one. */
#define HUMID_ROAD_PART_PADDED_REDO 1
#define HUMID_ROAD_ORDERS_REDONE    2
#define HUMID_ROAD_REGIONS_REGROWN  3
#define HUMID_ROAD_FAR_TILES        4
#define HUMID_ROAD_CSR_TILES        5
#define HUMID_ROAD_JOIN_PIECES      6
#define HUMID_ROADS_MAX 32
typedef struct humid_run_roads {
  uint32_t n_events;                 /* events of the call, also those beyond HUMID_ROADS_MAX     */
  uint32_t graph_attempts;
  uint8_t events[HUMID_ROADS_MAX];   /* HUMID_ROAD_*, in order; 0 behind the last                 */
} humid_run_roads;
int humid_get_run_roads(humid_ctx *ctx, humid_run_roads *out);
/* HIP-event durations of the dominant kernels of the last humid_stage_count_dense /
 * humid_stage_map_dense pair (k_dedup_lds or k_hash_insert; k_read_map_bucket, k_read_map_part or k_read_map_packed) */
int humid_stage_kernel_ms(humid_ctx *ctx, float *ms_k_insert, float *ms_k_map, uint32_t *count_mode_used);
int humid_stage_route_words(humid_ctx *ctx, const uint64_t *d_words, uint64_t n_send,
                            const uint64_t **d_routed);
/* The same routing without a host wait and without a sort: the caller already knows how many reads go
 * to every owner (send_counts[q]: from the all-gathered per-rank histograms, whose bins the value
 * ranges are cut at).  *d_routed = the usable words in owner-major order, INPUT ORDER inside every
 * owner's block (the owner derives "first read of a word" from it); *d_perm = routed position -> read
 * index, for humid_stage_scatter.  Queued on the context's stream.  humid_stage_route_check waits
 * for the stream and returns HUMID_E_INVALID if the counts did not match the reads. */
int humid_stage_route(humid_ctx *ctx, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                      const uint64_t *range_lo, const uint64_t *range_hi, uint32_t n_ranks,
                      const uint64_t *send_counts, const uint64_t **d_routed, const uint32_t **d_perm);
int humid_stage_route_check(humid_ctx *ctx);
int humid_stage_exchange_ids(humid_ctx *ctx, const uint32_t *d_nodes, const uint32_t *d_compact_cluster_id,
                             const uint8_t *d_compact_is_max, uint64_t n_nodes, uint64_t n_clusters,
                             uint64_t id_base, uint64_t u_local, const uint32_t **d_local_cluster_id,
                             const uint8_t **d_local_is_max);
int humid_stage_plan_info(humid_ctx *ctx, uint32_t word_nt, uint32_t distance, uint64_t plan_unique,
                          uint32_t *n_combos, uint32_t *prefix_bits);
int humid_stage_combo_route(humid_ctx *ctx, const uint64_t *d_word, const uint32_t *d_count,
                            uint64_t n_unique, uint64_t id_base, uint32_t word_nt, uint32_t distance,
                            uint64_t plan_unique, uint32_t combo, uint32_t n_ranks,
                            const uint64_t **d_items, uint64_t *counts);
int humid_stage_pairs_keyed(humid_ctx *ctx, const uint64_t *d_items, uint64_t n_items, int interleaved,
                            uint64_t id_base, const uint32_t *d_count, uint32_t word_nt,
                            uint32_t distance, uint64_t plan_unique, uint32_t combo,
                            const uint64_t **d_records, uint64_t *n_edges);
int humid_stage_compact_nodes(humid_ctx *ctx, const uint64_t *d_edges, uint64_t n_edges,
                              uint32_t record_stride, const uint32_t **d_nodes, uint64_t *n_nodes,
                              const uint64_t **d_compact_edges, const uint32_t **d_node_counts);

/* ---- the whole exchange-mode pass of one rank in ONE call --------------------------------------
 * humid_dedup_run_exchange runs, for this rank's shard of the reads (input order), the sequence the
 * stage entry points above make up -- histogram, value ranges, word exchange, counts, pairs per
 * combination, compact graph, result exchange, scatter -- with everything between the exchanges inside
 * the library (persistent buffers, no host language in between).  What only the caller can do, moving
 * bytes between ranks, it does through humid_comm:
 *   host_all_gather: every rank contributes `bytes` bytes of HOST memory; all[world * bytes] receives the
 *     contributions in rank order (blocking).
 *   exchange: DEVICE memory; rank q is sent d_send[send_off[q] .. + send_bytes[q]) and what rank q sends
 *     here arrives at d_recv[recv_off[q] ..), recv_bytes[q] long -- for every q including this rank
 *     itself.  Two shapes occur: an all-to-all (all_gather = 0: both sides laid out in rank order,
 *     send_off and recv_off the running sums of the sizes) and an all-gather (all_gather = 1: send_off
 *     all 0, send_bytes all equal: the same bytes go to everybody).  The transfer must be ordered after the work queued on `stream` (the
 *     context's stream) and either complete or be ordered before later work on that stream when the
 *     call returns (grouped ncclSend/ncclRecv on `stream` do exactly that).
 * Both return 0 or a negative value, which ends the run with HUMID_E_COMM.  With world == 1 neither is
 * called (comm may then be NULL).  Every rank must make the call with the same word_nt, distance and
 * method.  *summary receives the totals of the WHOLE read set (identical on all ranks; ms_* are this
 * rank's); *info what a caller needs for the statistics files.  word_nt 1 .. 64 (above 32: two uint64 per
 * read, as in humid_dedup_run).  Limits: at most 16 ranks, a pigeonhole plan with a prefix (distance <
 * word_nt): HUMID_E_UNSUPPORTED otherwise. */
#define HUMID_E_COMM        -7   /* a humid_comm callback failed                        */
typedef struct humid_comm {
  void *user;
  uint32_t rank, world;
  int (*host_all_gather)(void *user, const void *mine, uint64_t bytes, void *all);
  int (*exchange)(void *user, const void *d_send, const uint64_t *send_off, const uint64_t *send_bytes,
                  void *d_recv, const uint64_t *recv_off, const uint64_t *recv_bytes, int all_gather,
                  void *stream);
} humid_comm;
typedef struct humid_exchange_info {
  uint64_t unique_local;             /* unique words this rank owns (its value range)             */
  uint64_t id_base;                  /* walk index of the first of them                           */
  uint64_t n_nodes;                  /* unique words with neighbours, all ranks                   */
  uint64_t n_pairs;                  /* neighbour pairs, all ranks                                */
  const uint32_t *d_unique_count;    /* device: counts of this rank's unique words (counts.dat)   */
  const uint32_t *d_unique_degree;   /* device: neighbours of every one of them (neigh.dat); since ABI 4: every rank clusters
                                      * its own components (+ the replicated ones that cross value ranges), no rank holds all pairs */
} humid_exchange_info;
int humid_dedup_run_exchange(humid_ctx *ctx, const humid_comm *comm, const uint64_t *d_words,
                             const uint8_t *d_filtered, uint64_t n_local, uint32_t word_nt,
                             uint32_t distance, uint32_t method, uint32_t *d_cluster_id, uint8_t *d_keep,
                             humid_summary *summary, humid_exchange_info *info);

/* A ready-made humid_comm.host_all_gather for ranks that are PROCESSES OF ONE NODE: a POSIX shared-memory
 * segment with one slot and one arrival counter per rank (a gather is a store into the own slot, a
 * release of the counter and a spin on the others': a few microseconds, where a collective of the
 * process group costs ~100 us of launches and waits for a 16 KB table).  Rank 0 creates the segment
 * `name` (e.g. "/humid_<pid>"), the others attach to it (they wait up to ~30 s for it to appear); every
 * humid_shm_open is COLLECTIVE (rank 0 waits until every rank has attached to ITS segment: a rank that mapped a
 * stale segment of the same name, left by a crashed run, notices and maps again).  Every
 * rank then passes humid_shm_all_gather as host_all_gather and its handle as `user` -- or, when it needs
 * `user` for its own exchange callback, calls humid_shm_all_gather(handle, ...) from its own wrapper.
 * A gather is at most slot_bytes per rank (humid_dedup_run_exchange needs 16 KB: the histogram table). */
typedef struct humid_shm humid_shm;
int  humid_shm_open(humid_shm **out, const char *name, uint32_t rank, uint32_t world, uint64_t slot_bytes);
int  humid_shm_all_gather(void *shm, const void *mine, uint64_t bytes, void *all);
void humid_shm_abort(humid_shm *shm);    /* this rank gives the group up: every rank's gathers return -1 from now on */
void humid_shm_close(humid_shm *shm);

/* src/cluster.cc:31-33 atLeastDouble_, evaluated on the device (parity probe). */
int humid_at_least_double(humid_ctx *ctx, uint64_t a, uint64_t b, int *result);

#ifdef __cplusplus
}
#endif
#endif
