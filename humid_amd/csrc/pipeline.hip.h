// pipeline.hip.h -- the pipeline of libhumid_hip.so behind its C ABI: context, stage A (exact counts + walk order),
// stage B (neighbours + clusters), stage C (per-read outputs), the helpers around them.  Everything here has INTERNAL
// linkage (static functions, templates, static kernels in the headers below), so the two HIP translation units of the
// library -- humid_hip.hip (context, single-GPU entry points, accessors) and humid_exchange.hip (the exchange pass and
// the multi-GPU stage entry points) -- each compile what they use of it; round 3 split them (round 2: one file).
#ifndef HUMID_PIPELINE_HIP_H
#define HUMID_PIPELINE_HIP_H

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <type_traits>
#include <utility>

#include "common.hip.h"
#include "prims.hip.h"
#include "kernels_count.hip.h"
#include "kernels_part.hip.h"
#include "kernels_part8.hip.h"
#include "kernels_graph.hip.h"
#include "kernels_cluster.hip.h"
#include "kernels_cgraph.hip.h"
#include "kernels_map.hip.h"
#include "kernels_xchg.hip.h"
#include "kernels_wide.hip.h"
#include "kernels_gkey.hip.h"
#include "kernels_keyrank.hip.h"
#include "kernels_gstats.hip.h"
#include "kernels_whitelist.hip.h"
#include "kernels_wlpost.hip.h"
#include "kernels_segments.hip.h"
#include "kernels_cells.hip.h"
#include "kernels_paired.hip.h"
#include "kernels_accum.hip.h"
#include "kernels_long.hip.h"

// --------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------
// One slab of device memory a context may hold (humid_ctx_reserve): buffers are carved out of it
// with a bump pointer instead of one hipMalloc each -- a first run needs ~35 buffers and every
// hipMalloc costs about a millisecond, which is most of what the `humid` command line spends between
// "pass 1 done" and "device path done" on 10 M reads.  Nothing is returned to the slab; a buffer
// that outgrows its carving gets a new one (slab or hipMalloc).
struct Arena {
  char *base = nullptr;
  size_t size = 0, used = 0;
  void *take(size_t bytes) {
    const size_t at = (used + 255) & ~(size_t)255;
    if (!base || at + bytes > size) return nullptr;
    used = at + bytes;
    return base + at;
  }
};

// One device buffer, grown on demand.  It owns its block: move-only, freed by the destructor -- except a block carved
// from the slab, which is never freed one by one (the slab goes as a whole, humid_ctx_destroy).
struct DBuf {
  void *p = nullptr;
  size_t cap = 0;
  bool in_arena = false;
  DBuf() = default;
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  DBuf(DBuf &&o) noexcept { *this = std::move(o); }
  DBuf &operator=(DBuf &&o) noexcept {                       // the source ends empty; what the target owned is freed
    if (this != &o) { release(); p = o.p; cap = o.cap; in_arena = o.in_arena; o.p = nullptr; o.cap = 0; o.in_arena = false; }
    return *this;
  }
  ~DBuf() { release(); }
  hipError_t ensure(size_t bytes, Arena *arena = nullptr) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = bytes + bytes / 8 + 256;
    if (arena) {
      if (void *q = arena->take(bytes + 256)) { p = q; cap = bytes + 256; in_arena = true; return hipSuccess; }
    }
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = want;
    return hipSuccess;
  }
  // room for need_bytes with the first keep_bytes kept: a list that is appended to.  A new block of twice the need
  // (never from the slab), one copy, one stream wait.
  hipError_t grow_keeping(size_t keep_bytes, size_t need_bytes, hipStream_t stream) {
    if (need_bytes <= cap) return hipSuccess;
    DBuf bigger;
    hipError_t e = bigger.ensure(need_bytes * 2);
    if (e == hipSuccess && keep_bytes) e = hipMemcpyAsync(bigger.p, p, keep_bytes, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess) *this = std::move(bigger);
    return e;
  }
  void release() { if (p && !in_arena) (void)hipFree(p); p = nullptr; cap = 0; in_arena = false; }
  template <class T> T *as() const { return (T *)p; }
};
static_assert(!std::is_copy_constructible<DBuf>::value && !std::is_copy_assignable<DBuf>::value, "DBuf is move-only");
static_assert(std::is_nothrow_move_constructible<DBuf>::value && std::is_nothrow_move_assignable<DBuf>::value, "DBuf is move-only");

// ---- what a context holds: ONE record of what the last mutating call left behind ----------------------------------
// Every mutating entry point starts with state_reset and ends, on success only, with state_publish; a stage graph,
// which builds on the count before it, starts with state_begin_graph instead.  Accessors ask the predicates below.
//
//   holds        leaf accessors (a)   run accessors (b)   kind accessors (c)
//   NOTHING      E_STATE              E_STATE             E_STATE            (no call yet, or the last one failed)
//   COUNT        E_STATE              E_STATE             E_STATE            (humid_stage_count*, the exchange pass)
//   STAGE_GRAPH  answer               E_STATE             E_STATE            (humid_stage_graph*: leaves, no reads)
//   HAND_GRAPH   E_STATE              E_STATE             E_STATE            (humid_cluster_graph returns all it has: recorded, read by nobody)
//   RUN          answer               answer              answer from its kind on, E_STATE below it
//
//   (a) humid_get_leaves without first_read, humid_get_adjacency, humid_get_clusters, humid_get_histogram
//   (b) first_read of humid_get_leaves, humid_get_packed_words, humid_get_group_stats / humid_group_stats_device,
//       humid_select_best* (which refuses with HUMID_E_INVALID)
//   (c) humid_get_leaf_groups: RUN_GROUPED; humid_get_group_keys, humid_keyed_rank_info: RUN_KEYED;
//       humid_get_barcode_status: RUN_CORRECTED; humid_get_barcode_posterior: RUN_CORRECTED with bc_posterior.  The
//       data of a kind (gk_word_nt, gk_leaf_nt, gk_groups; kr_n; bc_N, bc_posterior) is valid exactly when the record
//       says the run is of that kind.
//   dense is orthogonal: humid_stage_map_dense and humid_stage_kernel_ms answer while it is set, whatever holds says.
//   One STAGE_GRAPH is of a kind: the finish of a keyed accumulator (state_publish_keyed_graph) is RUN_KEYED, and
//   humid_get_leaf_groups, humid_get_group_keys and humid_get_group_stats / humid_group_stats_device answer for it
//   (its keys are ac_keys, not kr_keys); first_read and everything else under (b) stay E_STATE.
// The results of humid_consensus* are no part of this: they survive runs (cs_valid).
enum RunKind : u8 { RUN_PLAIN, RUN_GROUPED, RUN_KEYED, RUN_CORRECTED };   // ordered: each kind is a case of the one before
enum : u32 { CC_NONE = 0, CC_ON, CC_INVALID };   // a count fed in chunks (humid_cells_*, humid_whitelist_prior_*)
struct CtxState {
  enum Holds : u8 { NOTHING, COUNT, STAGE_GRAPH, HAND_GRAPH, RUN } holds = NOTHING;
  RunKind kind = RUN_PLAIN;    // of a RUN
  bool dense = false;          // the last count ran on a compacted list of this rank's reads; a stage graph after it keeps this
  bool stats_current = false;  // derived on demand from a RUN: gs_* hold its group statistics for gs_G groups
  bool paired = false;         // the RUN was humid_dedup_run_paired*: pd_strand / pd_top / pd_bottom / pd_sum are its (humid_get_strands)
  bool long_words = false;     // the RUN was humid_dedup_run_long*: g_word holds g_wpr = ceil(word_nt / 32) uint64 per leaf, lg_info is its (humid_long_info)
};

// What the last count that was KEPT left behind (stage_count.hip.h): the road it took and what the stages behind it
// need of that road.  Assigned whole by count_publish, once per kept count -- a discarded record attempt and an
// overflowed LDS attempt publish nothing -- and replaced only by the next kept count: not by state_reset, for
// humid_stage_count* -> humid_stage_graph* -> humid_stage_map* are separate calls that rely on it.  Read through the
// predicates below only.
enum CountRoad : u8 {
  COUNT_GLOBAL,        // one hash table in HBM; slot_of_read maps the reads
  COUNT_LDS_HASHED,    // LDS tables over hashed buckets, (key, read) pairs
  COUNT_LDS_ORDERED,   // LDS tables over word-ordered buckets, (key, read) pairs (two-word words: keys + gather)
  COUNT_REC,           // word-ordered buckets on records; positions are (bucket << 9 | j), the un-permute reads p8_b
  COUNT_SORTED         // the sorting count of two-word and long words: no buckets
};
struct CountLeft {
  CountRoad road = COUNT_GLOBAL;
  u32 n_parts = 0;               // buckets (0: the road has none)
  bool part_tiled = false;       // KEV_PART_BEGIN .. KEV_PART_END bracket a second-level scatter
  const u32 *cursor2 = nullptr;  // COUNT_REC: reads per bucket
};
// The remembered answer of prefix_fits_ordered for (reads, word length, key map): the sampled histogram and its host
// wait run once per shape, not once per pass; an overflowing ordered run sets it to "no"
struct OrderedMemo {
  bool valid = false, fits = false;
  u32 n = 0, nt = 0;
  u64 lo = 0, scale = 0;
};

// ---- the timing of a pass: named event slots and two records (the functions over them: pass_timing.hip.h; the table
// of who records and who reads which slot: DESIGN.md, "The events of a pass") ----
#define STAMP_N 4
enum StageEvent : u32 {              // humid_ctx::ev
  EV_PASS_START, EV_COUNT_END, EV_GRAPH_BUILT, EV_CLUSTERS_DONE, EV_PASS_END,
  EV_HOST_FRAME,                     // the first of the four events around a host entry point's copies (HostFrame)
  EV_N
};
enum { KEV_PAIR_COMBOS = 8 };        // combinations of a neighbour search that have events of their own
enum KernelEvent : u32 {             // humid_ctx::kev
  KEV_INSERT_BEGIN, KEV_INSERT_END,  // the count kernel
  KEV_CLUSTER_BEGIN, KEV_CLUSTER_END,
  KEV_PAIRS_FILL,                    // (begin, end) per combination: kev_pairs()
  KEV_PAIRS_COUNT = KEV_PAIRS_FILL + 2 * KEV_PAIR_COMBOS,
  KEV_MAP_MID = KEV_PAIRS_COUNT + 2 * KEV_PAIR_COMBOS,   // behind the first kernel of the read map
  KEV_DENSE_MAP_BEGIN, KEV_DENSE_MAP_END,                // humid_stage_map_dense
  KEV_PART_BEGIN, KEV_PART_END,      // the count's second-level scatter
  KEV_UNPERM_END,                    // behind k_unperm_window
  KEV_DENSE_MAP_MID,                 // between the two kernels of the dense map's tiled un-permute
  KEV_N
};
static_assert(EV_N == 6 && KEV_PAIRS_COUNT == 20 && KEV_MAP_MID == 36 && KEV_N == 43, "the event slots");
// What the pass now running has decided about its timing.  All false between calls, but for the last two, which the
// stage calls behind a map read: PassTimingGuard opens and closes it.
struct PassTiming {
  bool lean = false;             // the per-kernel timing is off: of the stage events only pass start and pass end are recorded, and the count kernel's pair
                                 // (an event record between two kernels is a marker the second one waits behind: ~4 us of idle GPU each, 8 per pass)
  bool stamp_ok = false;         // before the first launch: this pass may take its times from device stamps (cleared when a count is discarded)
  bool stamp_live = false;       // stage_count_rec counted this pass: its kernels store the stamps
  bool stamp_timed = false;      // ... and the pass is lean: no frame mark is recorded, the summary's times are the stamps'
  bool kernels_quiet = false;    // cg_build_full: the kernel marks are off whatever the option says
  bool unperm_tiled = false;     // KEV_MAP_MID .. KEV_UNPERM_END bracket k_unperm_window of the last map
  bool dense_map_timed = false;  // KEV_DENSE_MAP_BEGIN .. _END bracket the last humid_stage_map_dense
};
// What the last mutating call left for humid_stamp_info: cleared whole by state_reset
struct TimingLeft {
  u64 stamps[STAMP_N] = {};
  bool stamp_live = false, stamp_timed = false;
  u32 event_records = 0;         // hipEventRecord calls of that call: host stores only (EVREC, HostFrame)
};

struct humid_ctx {
  int device = 0;
  CtxState state;
  humid_run_roads roads = {};      // what the last mutating call retried (humid_get_run_roads): cleared with the record, host stores only
  RunKind pass_kind = RUN_PLAIN;   // the kind of the pass now running (PassKind below); RUN_PLAIN between calls
  Arena arena;               // humid_ctx_reserve
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  ull *d_ctr = nullptr;
  PsChain *ps_chain = nullptr;   // behind the counters
  u32 ps_epoch = 0;
  ull *h_ctr = nullptr;   // pinned mirror (CTR_N counters + the sequence word of read_counters)
  ull *h_ctr_dev = nullptr;   // the same memory as the device sees it
  ull ctr_seq = 0;
  // Device stamps (option "device_stamps"): the four points a lean pass is timed between -- pass start, count kernel
  // start and end, pass end -- as the 100 MHz wall clock read by thread 0 of workgroup 0 of a kernel that runs there
  // anyway, where the four frame marks would put as many markers into the stream.  d_stamp: STAMP_N
  // u64 of their own (on no ZeroList); the pass's last k_publish_counters copies them to h_ctr[STAMP_AT ..].
  u64 *d_stamp = nullptr;
  bool device_stamps = true;   // the option
  PassTiming timing;           // of the pass now running
  TimingLeft timing_left;      // of the last mutating call
  const u32 *gf_valid = nullptr; // set by the last bucket order: device count of the words it holds (padded grouping), or null
  u32 *ucur_clean = nullptr;     // the un-permute's bin cursors at this address are all zero
  DBuf gf_cur;                    // cursors of the padded grouping (512 u32, kept at zero between uses)
  bool gf_padded = true;  // bucket orders of the compact graph stage through padded coarse bins (until one was full)
  bool no_chain = false;  // HUMID_NO_SCAN_CHAIN: scans without k_ps_scan_chain (experiment / cross-check)
  bool no_poll = false;   // HUMID_NO_POLL / a failed first try: blit copies + stream wait instead
  DBuf in_words, in_filt, in_bases, out_cid, out_keep;       // host entry point staging of a run (humid_get_packed_words reads it)
  DBuf stage_in[9], stage_out[3];                            // host entry point staging of every post-run pass (STAGE_IN / STAGE_OUT)
  DBuf table, slot_out, slot_of_read, uniq_slot;             // table (cap+1) and per-read
  DBuf pk_keys, pk_vals, pbeg, ucount, pusable, ubase, pad_word, pad_cf, pslot;   // partitioned counts
  DBuf opos, own_packed, owner, owner_sorted, perm, small;                        // multi-GPU result return
  DBuf pc, poff, share_edges;                                                     // multi-GPU pair-search share
  DBuf own_words;                                                                 // multi-GPU dense count
  DBuf heads;                                                                     // big-component heads
  DBuf small_roots;         // k_comp_count: roots of the components of 3 .. 32 leaves (k_cluster_small works off this list)
  DBuf big_runs;            // k_big_runs: (start, length, first tile) of the buckets beyond k_pairs' walk, per combination
  DBuf had;                 // k_pairs: per combination and position, pairs found in the first phase (<< 24) | distance to the first one
  DBuf e_kx, e_vx, e_ky, e_vy, e_raw, e_sorted, e_edges, e_head, e_hpos;   // edit-distance neighbour search
  DBuf e_runlo, e_nch, e_choff, e_pc2, e_poff2;                            // ... its long runs in pieces
  bool edit = false;         // option "edit_distance": Levenshtein instead of Hamming neighbours (-e)
  DBuf xr_heads, xr_send, xr_zero;                             // the same for two-word words: heads, routed words, an all-usable flag array
  DBuf xr_hist, xr_recv, xr_eloc, xr_got, xr_eall, xr_ret;   // humid_dedup_run_exchange: histogram, received words, pair records, received items, results
  DBuf x_slot, x_slot_s, x_cnt, x_cnts, x_rec, x_ncnt, x_route, x_creator, x_base, x_mark, x_markcr, x_scan, x_lcid, x_lismax,
       x_items, x_w, x_id, x_ids, x_ends, x_ends_s, x_head, x_hpos, x_nodes, x_cedges;   // multi-GPU exchange mode
  DBuf w_sorted, w_head, w_hpos, w_start, w_heads;                                         // wide-word (sorted) counts
  // compact graph (kernels_cgraph.hip.h): pair regions + cursors, the two bitmaps with their rank blocks, per-node arrays
  DBuf cg_edges, cg_cur, cg_far, cg_bits, cg_nbits, cg_blk, cg_nblk, cg_nodes, cg_ncnt, cg_deg, cg_off, cg_idx, cg_parent, cg_csize,
       cg_curs, cg_cl_of, cg_maxleaf, cg_cl_size;
  u64 cg_ecap = 0;                  // room for pairs in the append regions (remembered from pass to pass; grown on demand)
  bool use_compact = true;          // option "compact_graph": 0 = the per-unique-word graph of rounds 1-2
  bool cg_valid = false;            // the last graph stage left its results in the cg_* arrays ...
  bool cg_expanded = false;         // ... and the per-unique-word view of them has been built (accessors)
  u32 cg_M = 0, cg_nblocks = 0;
  // the pairs of a graph stage split (k_pairs_split): isolated pairs are settled from the pair list, the compact graph
  // holds the rest.  cg_multi: leaves with >= 2 pairs; cg_rbits: ends of the rest pairs; cg_rest: those pairs;
  // cg_pres: creator | maxLeaf flag of the ends of isolated pairs
  DBuf cg_multi, cg_rbits, cg_rest, cg_pres;
  bool pair_split = true;           // option "pair_split": 0 = every pair goes through the compact graph
  bool cg_split = false;            // the last graph stage split its pairs: cg_* hold the REST graph until cg_ensure_full
  bool cg_full = false;             // ... and the graph over all pairs has been built since (accessors; once per run)
  bool cg_broken = false;           // ... and building that graph failed halfway (the pair list is relabelled in place: no second try)
  bool cg_m_late = false;           // ... and the rest graph's node count comes with the pass's last wait (n_clusters_compact)
  u64 cg_iso = 0, cg_R = 0;         // isolated pairs, rest pairs of that stage
  EdgeRegs cg_er = {};              // its pair list (regions + far), untouched by the split
  u64 cg_pairs_bound = 0;
  u32 cg_method = 0;
  const u32 *ctr_x[3] = {nullptr, nullptr, nullptr};   // read_counters_begin without the mapped mirror: what _end copies
  // owner-local clustering of the exchange pass (kernels_xchg.hip.h): records by destination, interior / crossing /
  // flagged-interior records, the forest over own leaves, crossing-creator bitmap and ids, own results
  DBuf xo_gw, xo_gc;                // the edit-distance road: unique words / counts of all ranks
  DBuf xo_regs, xo_inv;             // record regions of the pair search; routed position of every read
  u64 xr_ecap = 0;                  // room for pair records in the regions (remembered from pass to pass)
  DBuf xo_send, xo_int, xo_cross, xo_sel, xo_selall, xo_parent, xo_flag, xo_xroot, xo_xcbits, xo_xcblk, xo_xcid, xo_xcall, xo_ldeg, xo_cnt;
  DBuf pw_a, pw_ai, pw_b, pw_bi;    // two-word words: (word, read index) records of the two partition levels
  DBuf p8_a, p8_b, p8_cur, p8_status;               // 8-byte records of the count stage: level-1 output, level-2 output (kernels_part8.hip.h)
  bool use_rec8 = true;             // option "records8": 0 = always the 12-byte (key, read) pairs of kernels_part.hip.h
  CountLeft count_left;             // what the last kept count left behind
  DBuf pt_work, unperm_rec, route_tiles;                                                     // LDS-staged partition / un-permute (kernels_part.hip.h)
  bool group_buckets = true;        // option "group_buckets": bucket order of stretch keys by two-level grouping instead of a library sort
  bool fused_search = true;         // option "fused_search": the compact graph's neighbour search of a grouped combination rides in k_group_fine (0: a launch of k_pairs_append per combination)
  bool group_records = true;        // option "group_records": a grouping whose search rides moves 8-byte records (squeezed word, walk index) and stores no order (0: the 12-byte pairs, the order stored)
  u32 gr_rides = 0, gr_orders = 0;  // the last compact graph stage: groupings searched on records; bucket orders stored (humid_group_records_info)
  bool overlap_waits = true;        // option "overlap_waits": the count stage's and the split graph stage's host waits stand behind their publishing kernel with work queued after it (0: publish and wait back to back)
  bool static_tiles = true;         // option "static_tiles": level 2 of the record count finds its tiles from the padded bins' cursors (0: the tile table of k_pt_scan1)
  u32 wo_waits = 0, wo_overlapped = 0;   // host waits of the last mutating call; those with work queued between publish and wait (humid_wait_overlap_info): host stores only
  bool pt_padded = true;            // level 1 of the tile partition into padded coarse bins (no histogram pass); false after an overflow
  bool use_tile_partition = true;   // option "tile_partition": 0 = library radix passes + one-kernel un-permute (round 1)
  int x_test_fail_after = -1, x_gathers = 0;   // option "test_fail_before_gather": this rank leaves the pass with an error in the compute phase before its k-th gather (tests)
  bool x_hist_done = false, x_peer_failed = false;   // humid_dedup_run_exchange: the pass's first gather is done; a peer's failure was seen
  bool route_checked = true;        // no humid_stage_route since the last humid_stage_route_check
  const u32 *route_bad = nullptr;   // device flag of the last humid_stage_route
  OrderedMemo ordered_memo;
  u32 g_wpr = 1;                                                                  // uint64 per word of g_word
  bool slots_done = false;   // slot_out already written by k_finalize_nodes (one-GPU fusion)
  int count_mode = 0;        // 0: hash-partitioned LDS tables (default), 1: one global HBM table
  u32 force_segments = 0;    // 0: automatic pigeonhole plan; else the number of segments s
  bool force_comm = false;   // humid_dedup_run_exchange: call the humid_comm callbacks even with one rank (transport tests)
  u32 walk_max = PT2_TILE;   // k_pairs compares a position with this many followers; longer buckets go to k_pairs_tiles (0: never)
  bool coop_big = true;      // big components: workgroup-cooperative kernel (directional method)
  int count_order = -1;      // LDS buckets by word prefix: -1 automatic (uniform prefix), 0 never, 1 always
  // grouped runs (humid_dedup_run_grouped*): the pass runs over internal words that carry the group ("gkey")
  // in gk_nt nucleotides above the caller's word; the count sorts them into (group, word) walk order and every
  // combination of the plan starts with the whole group field (make_plan), so buckets never mix groups
  u32 gk_nt = 0;             // the group field (nucleotides) of the pass now running; 0 unless pass_kind >= RUN_GROUPED
  u32 gk_epoch = 0;          // value k_gkey_words stores into h_ctr[CTR_N + 1] when a usable read's group is out of range
  u32 gk_word_nt = 0, gk_leaf_nt = 0;   // RUN_GROUPED on: the leaf arrays hold internal words of this caller word length and group field
  DBuf gk_words, gk_group_in, gk_bad;   // internal words (a keyed accumulator: a chunk's entries); host entry point staging of the groups; device flag (no mapped memory)
  // keyed runs (humid_dedup_run_keyed*): grouped runs whose groups are the ranks of 64-bit keys (kernels_keyrank.hip.h)
  u32 kr_n = 0;              // RUN_KEYED on: kr_keys holds the run's kr_n sorted distinct keys
  u32 kr_cap_log2 = 0;       // log2 of the table size of the next ranking (0: 16); remembered from pass to pass, grown on demand
  u32 kr_force_log2 = 0;     // option "keyrank_table_log2": every ranking starts with this table size (test hook)
  u32 kr_last_log2 = 0, kr_redo = 0;    // the last ranking: its final table size and how often it was repeated
  DBuf kr_table, kr_raw, kr_rawslot, kr_keys, kr_slot, kr_key_in;   // table; compacted and sorted (key, slot); host entry point staging
  // barcode whitelist (humid_whitelist_*, kernels_whitelist.hip.h): the table belongs to the context, in memory of its
  // own (never the slab, never a buffer a run carves), until it is replaced, cleared or the context destroyed
  DBuf wl_table;             // u64[cap + 2]: keys, the reserved slot of the key EMPTY_KEY, the number of distinct barcodes
  u64 wl_n = 0;              // distinct barcodes (0: no whitelist)
  u32 wl_nt = 0, wl_log2 = 0;   // nucleotides of a barcode; log2 of the table's slots
  bool wl_coop = true;       // option "whitelist_coop": 0 = the lane-serial correction kernel (measurement / cross-check)
  u64 bc_N = 0;              // RUN_CORRECTED: bc_status / bc_counts are those of the run's bc_N reads
  DBuf bc_key, bc_filt, bc_status, bc_counts;            // corrected run: key_out, filtered', status, u64[5]
  DBuf wc_counts;                                        // humid_whitelist_correct*: counts of its own
  // correction by quality and abundance (humid_whitelist_correct_posterior*, humid_dedup_run_keyed_posterior*,
  // kernels_wlpost.hip.h): bc_counts / wc_counts then hold WLP_CTRS counters; the reads per barcode belong to the last such
  // call or run, whichever came later, and go with the whitelist they index (humid_whitelist_counts)
  DBuf bc_qual_in;           // host entry point staging of a posterior run's qualities
  DBuf wp_cnt, wp_slot;      // u32[cap + 1] reads per table slot; u32[n_reads] the slot of every read's key
  bool wp_valid = false;     // wp_cnt holds the counts of a posterior call or run over the whitelist now set
  bool bc_posterior = false; // RUN_CORRECTED: the correction was the posterior one (humid_get_barcode_posterior)
  // segmented whitelist (humid_whitelist_set_segments, kernels_segments.hip.h): in place of wl_table; wl_n is then the
  // product of the lists' distinct entries (saturating), wl_nt the sum of the segments, wl_log2 0
  SegPlan sg = {};           // sg.n_seg = 0: the whitelist in place is plain or absent
  u64 sg_distinct[SEG_MAX] = {};   // distinct entries of every list
  DBuf sg_table;             // u32[sum of 4^L_s]: the resolution tables, one behind the other
  DBuf sg_sum;               // u64[SEG_SUM_N]: the per-segment summary of the last segmented correct call or corrected run
  bool sg_sum_valid = false; // ... which ran over the segmented whitelist now set (humid_get_barcode_segments)
  // whitelist from the data (humid_whitelist_discover*, kernels_cells.hip.h): buffers of its own, never the slab, never
  // kr_table or anything else a run or an accessor reads; the results of the last successful call are kept for the getters
  u32 cd_cap_log2 = 0;       // log2 of the counting table of the next call (0: 16); remembered from call to call, grown on demand
  u32 cd_force_log2 = 0;     // option "cells_table_log2": every call starts with this table size (test hook)
  DBuf cd_table, cd_cnt, cd_ctr, cd_k0, cd_c0, cd_kkey, cd_kccnt, cd_flag, cd_pos, cd_skey, cd_scnt, cd_tmp;   // table, counters, scratch lists
  DBuf cd_cells, cd_cellcnt, cd_hist_n, cd_hist_first;   // results: cells ascending u64 / u32; histogram bins u64 / u32 (first rank)
  bool cd_valid = false;     // the whitelist in place (or its absence: zero cells) was installed by a discover call
  u64 cd_n_cells = 0, cd_n_hist = 0, cd_G = 0;           // entries of the result buffers; distinct barcodes of that call
  // the barcode counter fed in chunks (humid_cells_*): a counting table of its own that outlives the adds and grows while it
  // holds counts; no discover call, run or accumulator touches it, and it touches none of them (finish shares the
  // discovery's scratch lists and installs its results as a discover call does)
  u32 cc_state = CC_NONE;    // CC_NONE before humid_cells_begin / after _clear, CC_ON, CC_INVALID after a failed add
  u32 cc_nt = 0, cc_log2 = 0, cc_grown = 0;               // barcode length; log2 of the table's slots; growths since begin
  u64 cc_chunks = 0, cc_reads = 0, cc_usable = 0, cc_invalid = 0, cc_distinct = 0;
  DBuf cc_table, cc_cnt, cc_ctr, cc_pend;                // u64[cap + 1], u32[cap + 1], ull[CA_CTRS], u8[reads of a chunk]
  // the posterior's prior fed in chunks (humid_whitelist_prior_*): reads per slot of wl_table in an array of its own (wp_cnt
  // is zeroed by every one-shot posterior call); it goes with the table it indexes
  u32 pr_state = CC_NONE;    // CC_NONE before humid_whitelist_prior_begin / once the whitelist changed, CC_ON, CC_INVALID
  bool wp_prior = false;     // humid_whitelist_counts answers from pr_cnt: a prior call came later than any one-shot posterior
  DBuf pr_cnt, pr_ctr;       // u32[cap + 1]; ull[1] the overflow flag
  // per-group statistics (humid_get_group_stats / humid_group_stats_device, kernels_gstats.hip.h): computed by the first
  // accessor call after a run, kept until the next one; the runs themselves launch nothing for them
  u32 gk_groups = 1;         // n_groups of the last grouped run
  u32 gs_G = 0;
  DBuf gs_reads, gs_loff, gs_coff, gs_edges, gs_ps;   // reads u64[G], leaf / cluster offsets u32[G + 1], pairs u32[G]; scan of (count | degree << 32)
  // best-scoring read per cluster (humid_select_best*, kernels_best.hip.h): memory of its own, read by no accessor
  DBuf bs_rep, bs_best, bs_ctr;                              // u32[C + 1] representatives, u64[C + 1] votes, the pass's counters
  // consensus reads (humid_consensus*, kernels_consensus.hip.h): results in memory of their own, kept until the next
  // humid_consensus* call; no run and no other accessor touches them
  DBuf cs_rep, cs_cnt, cs_moff, cs_cur, cs_mem, cs_ctr, cs_big, cs_piece, cs_tab;   // representatives, reads per cluster, member lists, large clusters
  DBuf cs_ooff, cs_ob, cs_oq, cs_depth, cs_errors;           // results: u64[C + 1], two byte blobs, u32[C], u64[C]
  bool cs_valid = false;     // a humid_consensus* or humid_duplex_consensus* call succeeded: cs_sum and the result buffers are its
  humid_consensus_summary cs_sum = {};
  // duplex consensus reads (humid_duplex_consensus*, kernels_dconsensus.hip.h): the same scratch and result buffers, and
  bool cs_duplex = false;    // cs_valid and that call was a duplex one: ds_* and ds_sum are its (humid_get_duplex_consensus)
  DBuf ds_top, ds_same, ds_other, ds_disagree;               // TOP members u32[C + 2]; results: three u32[C]
  humid_duplex_summary ds_sum = {};
  // optical duplicates (humid_optical_duplicates*, kernels_optical.hip.h): memory of its own, read by no accessor
  DBuf op_rep, op_bctr, op_ctr, op_k0, op_v0, op_v1, op_ct, op_xy, op_vote, op_parent, op_root, op_best, op_gsize;
  u32 op_walk = 64;          // option "optical_walk" (OPT_WALK_DEFAULT): followers a position walks before its wave takes over; 0 = no bound
  // strand-symmetric runs (humid_dedup_run_paired*, kernels_paired.hip.h): the pass runs over the canonical words
  bool pd_run = false;       // a paired pass is running: run_device takes its neighbour pairs from paired_edges
  DBuf pd_words, pd_strand, pd_mir, pd_top, pd_bottom, pd_ctr;   // canonical words, strands, mirrored leaves, tallies u32[C + 1], ull[PD_CTRS]
  u64 pd_N = 0;              // state.paired: pd_strand holds the strands of the run's pd_N reads
  humid_strand_summary pd_sum = {};
  // long words (humid_dedup_run_long*, kernels_long.hip.h)
  u32 lg_key_bits = 64;      // option "long_key_bits": the join keys are masked to this many bits (tests force collisions with 2)
  humid_long_info_t lg_info = {};   // state.long_words: what the run's search did
  DBuf lg_cand;              // ull[MAX_COMBOS][LONG_CAND_SLOTS]: candidates verified, per join
  // accumulated runs (humid_accum_*, kernels_accum.hip.h): a read set fed in chunks.  The list -- distinct words ascending,
  // reads per word, smallest global read index per word -- lives in TWO buffer sets of its own (never the slab): a merge
  // reads set ac_cur and writes the other, and the sets swap only when it succeeded.  Kept until humid_accum_begin,
  // humid_accum_clear or the end of the context; no run and no other accessor touches it.
  bool ac_on = false;        // humid_accum_begin was called
  bool ac_finished = false;  // humid_accum_finish succeeded after the last add: ac_cid / ac_ismax are those of the list
  u32 ac_nt = 0, ac_cur = 0; // word length; the set that holds the list
  u32 ac_tile = ACC_TILE;    // option "accum_tile": merge positions per tile
  u64 ac_U = 0, ac_chunks = 0, ac_total = 0, ac_usable = 0;   // words in the list; chunks, reads and usable reads added
  DBuf ac_word[2], ac_cnt[2], ac_first[2];                    // WT[U], u32[U], u64[U]
  DBuf ac_split, ac_tcnt, ac_toff, ac_flag;                   // the merge: tile splits, new words per tile, their scan; overflow flag + unknown reads
  DBuf ac_cid, ac_ismax, ac_lcid, ac_lismax;                  // finish's copy of cid / ismax per word; a mapped chunk's per-leaf results
  // keyed accumulators (humid_accum_begin_keyed): the list holds entries (key, word) of ac_ent_nt nucleotides as the count
  // stage sees them -- one u64 `key << 2 * ac_nt | word` up to 32, W2 {key, word} beyond; ac_nt stays the caller's word
  bool ac_keyed = false;
  u32 ac_key_nt = 0, ac_ent_nt = 0;
  u64 ac_G = 0;                                               // ac_finished: distinct keys of the list
  DBuf ac_head, ac_hpos, ac_keys, ac_iword;                   // finish: key heads u32[U + 1], their scan, the keys u64[G], the pass's internal words
  DBuf uniq_word, s_word, s_slot, s_cnt, s_first;            // unique words (walk order)
  DBuf deg, nbr_off, nbr_idx, seg_k0, seg_v0, seg_ks, seg_vs, seg_ws, csize, cur;
  DBuf parent, mk0, mk1, cl_of, maxleaf, cl_size, flag, pos, cid, ismax, stk, tmp, scratch;
  hipEvent_t ev[EV_N] = {};    // by StageEvent
  bool kev_on = false;         // option "kernel_timing": events around the single kernels beyond the count kernel's pair (13 more records per pass: 20-45 us)
  hipEvent_t kev[KEV_N] = {};  // by KernelEvent
  const void *g_word = nullptr;  // arrays stage B ran on (u64 or W2 per word)
  const u32 *g_cnt = nullptr;
  u32 gU = 0;
  u32 cap_log2 = 0;
  u64 N = 0, U = 0, E = 0, M = 0, C = 0, usable = 0;
  u32 word_nt = 0, distance = 0, method = 0;
};

// the error text of calls without a context lives in ONE place (humid_hip.hip): humid_last_error(NULL) reads it
extern "C" void humid_set_global_error(const char *text);

static int fail(humid_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else humid_set_global_error(buf);
  return code;
}

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return fail(c, _e == hipErrorOutOfMemory ? HUMID_E_NOMEM : HUMID_E_HIP, "%s: %s (%s:%d)", \
                  #expr, hipGetErrorString(_e), __FILE__, __LINE__);                        \
  } while (0)

#define STAMP_AT (CTR_N + 2)   // h_ctr: CTR_N counters, the sequence word, the grouped runs' check word, the stamps
// what the stages behind a count ask of its record
static inline bool count_in_partition_order(const humid_ctx *c) { return c->count_left.road != COUNT_GLOBAL; }   // stage C walks pk_vals / pslot (or the records), not slot_of_read
static inline bool count_bucketed(const humid_ctx *c) { return c->count_left.n_parts != 0; }                      // positions end at pbeg[n_parts]; the read map goes bucket by bucket
static inline bool count_on_records(const humid_ctx *c) { return c->count_left.road == COUNT_REC; }
static inline bool count_part_timed(const humid_ctx *c) { return c->count_left.part_tiled; }
// humid_summary::count_mode_used: 3 sorted, 2 ordered buckets, 0 hashed buckets, 1 global table; bit 8: on records
static inline u32 count_mode_used(const humid_ctx *c) {
  static const u32 mode[] = {1u, 0u, 2u, 2u | 0x100u, 3u};   // by CountRoad
  return mode[c->count_left.road];
}

enum { STAMP_START = 0, STAMP_K0, STAMP_K1, STAMP_END };

// Two memory rules.  A run's buffers and its own staging may be carved from the slab (ENSURE).  Every post-run pass
// allocates plainly (PASS_ENSURE): the slab is sized for one run and takes nothing back.
#define ENSURE(buf, bytes) HIPCHK((buf).ensure((bytes), &c->arena))
#define PASS_ENSURE(buf, bytes) HIPCHK((buf).ensure((bytes)))
#define D2H(dst, src, bytes)   /* null-tolerant: an output nobody asked for, or of no bytes, is not copied */ \
  do { if ((dst) && (bytes)) HIPCHK(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, c->stream)); } while (0)
// The host-buffer forms of the post-run passes share ONE staging pool: they run on one stream and each synchronises
// before it returns, so none overlap.  STAGE_OUT: d = room for `bytes` in output slot j.  STAGE_IN: d = input slot i
// with `bytes` copied from the host pointer h (no bytes: room only, h may be null).
#define STAGE_OUT(d, j, bytes) do { PASS_ENSURE(c->stage_out[j], (bytes) + 16); (d) = (decltype(d))c->stage_out[j].p; } while (0)
#define STAGE_IN(d, i, h, bytes)                                                              \
  do {                                                                                        \
    PASS_ENSURE(c->stage_in[i], (bytes) + 16);                                                \
    (d) = (decltype(d))c->stage_in[i].p;                                                      \
    if (bytes) HIPCHK(hipMemcpyAsync((d), (h), (bytes), hipMemcpyHostToDevice, c->stream));   \
  } while (0)

static inline u32 blocks_for(u64 n, u32 bs = 256) { return (u32)((n + bs - 1) / bs); }
static inline u32 grid_stride_blocks(u64 n, u32 bs = 256) {
  u64 b = (n + bs - 1) / bs;
  if (b > 256 * 8) b = 256 * 8;
  if (b == 0) b = 1;
  return (u32)b;
}
static inline u32 bits_for(u64 n) {  // bits needed to represent values < n
  u32 b = 0;
  while (b < 64 && ((u64)1 << b) < n) b++;
  return b ? b : 1;
}

// ---- sort / scan wrappers over prims.hip.h (temporary storage grown on demand) ----------
template <class K, class V, class KIn, class VIn>
static int sort_pairs_in(humid_ctx *c, KIn kin, K *kout, VIn vin, V *vout, u64 n, u32 b0, u32 b1) {
  if (n == 0) return HUMID_OK;
  if (n > 0xffffffffull) return fail(c, HUMID_E_OVERFLOW, "sort of more than 2^32-1 items");
  ENSURE(c->tmp, (rs_temp_bytes<K, V, true>(n)));
  HIPCHK((rs_sort<K, V, true>(c->tmp.p, kin, kout, vin, vout, n, b0, b1, c->stream)));
  return HUMID_OK;
}
template <class K, class V>
static int sort_pairs(humid_ctx *c, const K *kin, K *kout, const V *vin, V *vout, u64 n, u32 b0, u32 b1) {
  return sort_pairs_in<K, V>(c, PtrIn<K>{kin}, kout, PtrIn<V>{vin}, vout, n, b0, b1);
}
template <class K>
static int sort_keys(humid_ctx *c, const K *kin, K *kout, u64 n, u32 b0, u32 b1) {
  if (n == 0) return HUMID_OK;
  if (n > 0xffffffffull) return fail(c, HUMID_E_OVERFLOW, "sort of more than 2^32-1 items");
  ENSURE(c->tmp, (rs_temp_bytes<K, u32, false>(n)));
  HIPCHK((rs_sort<K, u32, false>(c->tmp.p, PtrIn<K>{kin}, kout, IotaIn{}, (u32 *)nullptr, n, b0, b1, c->stream)));
  return HUMID_OK;
}
template <class T, class In>
static int exscan_in(humid_ctx *c, In in, T *out, u64 n, u64 *stamp = nullptr) {
  ENSURE(c->tmp, ps_scan_scratch_items(n) * sizeof(T) + 256);
  HIPCHK((ps_exscan<T>(in, out, n, (T *)c->tmp.p, c->stream, c->no_chain ? nullptr : c->ps_chain, &c->ps_epoch, stamp)));
  return HUMID_OK;
}
static int exscan_u32(humid_ctx *c, const u32 *in, u32 *out, u64 n) { return exscan_in<u32>(c, PtrIn<u32>{in}, out, n); }

// device counters -> pinned mirror, one stream sync.  extra32 (device u32, may be null) lands
// in h_ctr[CTR_N - 1].
// One tiny kernel stores the counters (and the extra value) straight into the page-locked mirror and then
// a sequence number; the host watches that word.  Two blit copies + hipStreamSynchronize cost ~30 us of idle
// GPU per host wait, this ~10 (four waits per single-GPU pass, eight in the multi-GPU pass; three of the four have
// work queued behind the publishing kernel, which the GPU works through while the host reads: read_counters_begin /
// _end below, option overlap_waits).
static __global__ void k_publish_counters(const ull *__restrict__ ctr, const u32 *__restrict__ extra32, const u32 *__restrict__ extra32b,
                                   volatile ull *host, ull seq, const u32 *__restrict__ extra32c = nullptr, u64 *stamp = nullptr) {
  HUMID_GUARD_LAST_VGPR();
  if (stamp && threadIdx.x == 0) {   // the pass's last launch: its entry is the pass's end; the four stamps travel with the counters
    const u64 t = wall_clock64();
    stamp[STAMP_END] = t;
    host[STAMP_AT + STAMP_START] = stamp[STAMP_START];
    host[STAMP_AT + STAMP_K0] = stamp[STAMP_K0];
    host[STAMP_AT + STAMP_K1] = stamp[STAMP_K1];
    host[STAMP_AT + STAMP_END] = t;
  }
  if (threadIdx.x < CTR_N) {
    ull v = ctr[threadIdx.x];
    if (threadIdx.x == CTR_N - 1 && extra32) v = (v & ~0xffffffffull) | (ull)*extra32;
    if (threadIdx.x == CTR_N - 2 && extra32b) v = (ull)*extra32b;
    if (threadIdx.x == CTR_N - 3 && extra32c) v = (ull)*extra32c;
    host[threadIdx.x] = v;
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) { host[CTR_N] = seq; __threadfence_system(); }
}
// extra32 -> h_ctr[CTR_N - 1] (low half), extra32b -> h_ctr[CTR_N - 2], extra32c -> h_ctr[CTR_N - 3]
// The wait in two halves: _begin puts the publishing kernel into the stream, _end waits for it.  Kernels launched in
// between run while the host waits and decides (their results are not in the counters the host sees): a wait that
// costs the GPU no idle time.  read_counters is the two back to back.
// stamp (the pass's last wait only): the device stamps, see humid_ctx::d_stamp
static int read_counters_begin(humid_ctx *c, const u32 *extra32 = nullptr, const u32 *extra32b = nullptr, const u32 *extra32c = nullptr,
                               u64 *stamp = nullptr) {
  c->ctr_x[0] = extra32; c->ctr_x[1] = extra32b; c->ctr_x[2] = extra32c;
  if (c->h_ctr_dev && !c->no_poll) {
    const ull seq = ++c->ctr_seq;
    hipLaunchKernelGGL(k_publish_counters, dim3(1), dim3(64), 0, c->stream, (const ull *)c->d_ctr, extra32, extra32b,
                       (volatile ull *)c->h_ctr_dev, seq, extra32c, stamp);
    HIPCHK(hipGetLastError());
  }
  return HUMID_OK;
}
// work_queued: the caller has launched kernels since _begin (counted for humid_wait_overlap_info)
#define POLL_QUIET_US 2000   // with overlap_waits: the host asks the stream nothing for its first 2 ms at a wait
static int read_counters_end(humid_ctx *c, bool work_queued = false) {
  const u32 *extra32 = c->ctr_x[0], *extra32b = c->ctr_x[1], *extra32c = c->ctr_x[2];
  c->wo_waits++;
  if (work_queued) c->wo_overlapped++;
  if (c->h_ctr_dev && !c->no_poll) {
    const ull seq = c->ctr_seq;
    volatile ull *flag = (volatile ull *)&c->h_ctr[CTR_N];
    const auto t0 = std::chrono::steady_clock::now();
    u32 spins = 0;
    // (A query of a busy stream leaves a marker at its end: a kernel queued behind the publishing kernel was followed by
    // 5.7 us of idle GPU before the next launch started.  With overlap_waits the host watches 95-170 us ahead of the GPU
    // at two waits of a pass, so the first query comes only after POLL_QUIET_US of watching; from then on one every 4096
    // looks, 2.5 us, as without the option: profiles/r04e_device_stamps.md.)
    const auto quiet = std::chrono::microseconds(c->overlap_waits ? POLL_QUIET_US : 0);
    while (*flag != seq) {
      if ((++spins & 0xfffu) == 0) {
        const auto waited = std::chrono::steady_clock::now() - t0;
        if (waited < quiet) continue;
        if (hipStreamQuery(c->stream) != hipErrorNotReady) break;              // drained (the stores are done or lost) or failed: settled below
        if (waited > std::chrono::seconds(30)) break;
      }
    }
    if (*flag == seq) { std::atomic_thread_fence(std::memory_order_acquire); return HUMID_OK; }
    HIPCHK(hipStreamSynchronize(c->stream));                                   // an error of an earlier kernel surfaces here
    if (*flag == seq) return HUMID_OK;
    c->no_poll = true;                                                          // mapped stores not visible on this system: copies from now on
  }
  HIPCHK(hipMemcpyAsync(c->h_ctr, c->d_ctr, CTR_N * sizeof(ull), hipMemcpyDeviceToHost, c->stream));
  if (extra32)
    HIPCHK(hipMemcpyAsync(&c->h_ctr[CTR_N - 1], extra32, 4, hipMemcpyDeviceToHost, c->stream));
  if (extra32b || extra32c) {
    HIPCHK(hipStreamSynchronize(c->stream));
    if (extra32b) { c->h_ctr[CTR_N - 2] = 0; HIPCHK(hipMemcpyAsync(&c->h_ctr[CTR_N - 2], extra32b, 4, hipMemcpyDeviceToHost, c->stream)); }
    if (extra32c) { c->h_ctr[CTR_N - 3] = 0; HIPCHK(hipMemcpyAsync(&c->h_ctr[CTR_N - 3], extra32c, 4, hipMemcpyDeviceToHost, c->stream)); }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}
static int read_counters(humid_ctx *c, const u32 *extra32 = nullptr, const u32 *extra32b = nullptr, const u32 *extra32c = nullptr,
                         u64 *stamp = nullptr) {
  const int rc = read_counters_begin(c, extra32, extra32b, extra32c, stamp);
  return rc != HUMID_OK ? rc : read_counters_end(c);
}

#define TRY(...) do { int _rc = (__VA_ARGS__); if (_rc != HUMID_OK) return _rc; } while (0)

// exclusive scan of in[0 .. n] (n + 1 entries, the last a sentinel) and its total out[n], fetched with the counters:
// one host wait.  h_ctr holds the counters of that moment afterwards.
static int scan_total(humid_ctx *c, const u32 *in, u32 *out, u64 n, u64 *total) {
  TRY(exscan_u32(c, in, out, n + 1));
  HIPCHK(hipGetLastError());
  TRY(read_counters(c, out + n));
  *total = c->h_ctr[CTR_N - 1] & 0xffffffffull;
  return HUMID_OK;
}

// ---- the record of CtxState: one reset, one publish, the predicates ----------------------------------------------
static inline void state_reset(humid_ctx *c) {
  c->state = CtxState{}; c->roads = humid_run_roads{}; c->wo_waits = c->wo_overlapped = 0;
  c->timing_left = TimingLeft{};
}
// one retry of the call now running (HUMID_ROAD_*): behind the host wait that showed it, a store on the host
static inline void road_taken(humid_ctx *c, u8 road) {
  if (c->roads.n_events < HUMID_ROADS_MAX) c->roads.events[c->roads.n_events] = road;
  c->roads.n_events++;
}
static inline void state_begin_graph(humid_ctx *c) { const bool dense = c->state.dense; state_reset(c); c->state.dense = dense; }
// the last statement of a mutating entry point that succeeded (a RUN is of the kind of the pass that ran it)
static inline int state_publish(humid_ctx *c, CtxState::Holds holds) {
  const bool dense = holds == CtxState::STAGE_GRAPH && c->state.dense;   // (what state_begin_graph kept of the count)
  c->state = CtxState{holds, holds == CtxState::RUN ? c->pass_kind : RUN_PLAIN, dense, false};
  return HUMID_OK;
}
static inline int state_publish_count(humid_ctx *c, bool dense) { state_publish(c, CtxState::COUNT); c->state.dense = dense; return HUMID_OK; }
static inline bool state_has_leaves(const humid_ctx *c) { return c->state.holds == CtxState::RUN || c->state.holds == CtxState::STAGE_GRAPH; }
static inline bool state_has_run(const humid_ctx *c) { return c->state.holds == CtxState::RUN; }   // a complete single-GPU run
static inline bool state_dense_count(const humid_ctx *c) { return c->state.dense; }   // what humid_stage_map_dense builds on
static inline bool state_run_is(const humid_ctx *c, RunKind at_least) { return state_has_run(c) && c->state.kind >= at_least; }
// The finish of a keyed accumulator leaves a STAGE_GRAPH whose leaves carry groups as a keyed run's do: its record is of
// kind RUN_KEYED (every other STAGE_GRAPH is RUN_PLAIN).  What reads groups off the leaves asks this, not state_run_is.
static inline int state_publish_keyed_graph(humid_ctx *c) { state_publish(c, CtxState::STAGE_GRAPH); c->state.kind = RUN_KEYED; return HUMID_OK; }
static inline bool state_keyed_graph(const humid_ctx *c) { return c->state.holds == CtxState::STAGE_GRAPH && c->state.kind == RUN_KEYED; }
static inline bool state_groups_are(const humid_ctx *c, RunKind at_least) { return state_has_leaves(c) && c->state.kind >= at_least; }
// The kind of the pass now running: set by the outermost of run_grouped_device, run_keyed_device and
// run_keyed_corrected_device, read by gkey_check, copied into the record by run_device's state_publish.
struct PassKind {
  humid_ctx *c;
  const bool outermost;
  PassKind(humid_ctx *c_, RunKind k) : c(c_), outermost(c_->pass_kind == RUN_PLAIN) { if (outermost) c->pass_kind = k; }
  ~PassKind() { if (outermost) { c->pass_kind = RUN_PLAIN; c->gk_nt = 0; } }
};

// Plan of the generalised pigeonhole search (see ComboPlan).  s is chosen so that combo keys are
// long enough for buckets to be small at this U (>= ~log4(U) nucleotides) without exceeding
// MAX_COMBOS combinations; d >= n degenerates to one empty-mask combo (every pair compared).
static u64 n_choose_k(u32 n, u32 k) {
  if (k > n) return 0;
  u64 r = 1;
  for (u32 i = 1; i <= k; i++) r = r * (n - k + i) / i;
  return r;
}

// short_later: the keys of the combinations after the first (the ones whose bucket order has to be MADE;
// the first is a prefix of the sorted words) are cut to max(24, 2 * want) bits -- enough to tell U words
// apart, and at <= 24 bits the order comes from the two-level grouping instead of a library sort over
// every key bit (48 bits for two halves of a 48-nt word).  Only the one-GPU Hamming search asks for it:
// the shifted joins of the edit search and the exchange pass's routing keep whole segments.
// gnt > 0 (grouped runs): the words carry a group field of gnt nucleotides ABOVE their n nucleotides.  The segments
// are cut over the n word nucleotides only, and every combination starts with the whole group field, never cut
// (field 0; later word fields are cut to fit 64 key bits): buckets never mix groups, and the first combination is
// still a prefix of the (group, word)-sorted words.  The "all pairs" plan becomes all pairs within a group.
static ComboPlan make_plan(u32 n, u32 d, u64 U, u32 force_segments, bool short_later = false, u32 gnt = 0) {
  ComboPlan p;
  memset(&p, 0, sizeof p);
  const u32 gw = 2 * gnt, gsh = 2 * n;           // the group field: bits [gsh, gsh + gw)
  const unsigned __int128 gmask = gnt ? (((unsigned __int128)1 << gw) - 1) << gsh : 0;
  if (gnt && (d >= n || n_choose_k(d + 1, 1) > MAX_COMBOS)) {
    p.ncombo = 1; p.key_bits = gw; p.mask[0] = W2{(u64)(gmask >> 64), (u64)gmask};
    p.nfield[0] = 1; p.shift[0][0] = (u8)gsh; p.width[0][0] = (u8)gw;
    return p;
  }
  // d >= n: every pair is a neighbour pair.  d >= MAX_COMBOS: even the smallest plan, s = d + 1,
  // has d + 1 > MAX_COMBOS combinations (of ONE segment of at most n / (d + 1) <= 3 nucleotides at
  // n <= 64: buckets of a quarter of all words and more), so the search degenerates to the same
  // single combination with an empty mask: one bucket, every pair compared.
  if (d >= n || n_choose_k(d + 1, 1) > MAX_COMBOS) { p.ncombo = 1; p.key_bits = 0; p.mask[0] = W2{0, 0}; p.nfield[0] = 0; return p; }
  u32 want = 1;                                  // nucleotides of key wanted: 4^want >= U
  while (want < n + gnt && ((u64)1 << (2 * want)) < U) want++;
  const u32 want_all = want;                     // (the group field stands for gnt of them)
  if (gnt) want = std::min<u32>(n, want > gnt ? want - gnt : 1u);
  u32 best_s = d + 1, best_len = 0;
  u64 best_c = ~0ull;
  for (u32 sgm = d + 1; sgm <= n && sgm <= d + MAX_FIELDS - (gnt ? 1u : 0u); sgm++) {
    const u64 combos = n_choose_k(sgm, sgm - d);
    if (combos > MAX_COMBOS) break;
    if (force_segments) {                         // test hook: take exactly this s if it is legal
      if (sgm == force_segments) { best_s = sgm; best_len = (sgm - d) * (n / sgm); best_c = combos; break; }
      continue;
    }
    const u32 len = (sgm - d) * (n / sgm);       // guaranteed key length (short segments)
    const bool better = (best_len < want) ? (len > best_len) : (len >= want && combos < best_c);
    if (best_len == 0 || better) { best_s = sgm; best_len = len; best_c = combos; }
    if (best_len >= want) break;                 // smallest s that reaches the wanted length
  }
  const u32 sgm = best_s, k = sgm - d;
  u32 seg_shift[64], seg_width[64];
  {
    u32 base = n / sgm, rem = n % sgm, pos = 0;
    for (u32 t = 0; t < sgm; t++) {
      u32 len = base + (t < rem ? 1 : 0);
      seg_shift[t] = 2 * (n - pos - len);
      seg_width[t] = 2 * len;
      pos += len;
    }
  }
  // combinations of k segments in lexicographic order: the first is {0..k-1}, a prefix
  u32 idx[64];
  for (u32 t = 0; t < k; t++) idx[t] = t;
  u32 c = 0, maxbits = 0;
  while (true) {
    // A combo key holds at most 64 bits (only wide words can exceed that): the last field is cut
    // to its top bits and later fields are dropped.  Two words within distance d still agree on the
    // shortened mask of some combo, so the search stays complete; it only compares a few more pairs.
    unsigned __int128 m = gmask;
    u32 bits = gw, nf = 0;
    const u32 limit = (short_later && c > 0 && !force_segments) ? std::min<u32>(64u, std::max<u32>(std::max<u32>(24u, 2 * want_all), gw + 2)) : 64u;
    if (gnt) { p.shift[c][0] = (u8)gsh; p.width[c][0] = (u8)gw; nf = 1; }
    for (u32 t = 0; t < k && bits < limit; t++) {
      const u32 sg = idx[t];
      u32 wd = seg_width[sg], sh = seg_shift[sg];
      if (bits + wd > limit) { const u32 cut = bits + wd - limit; wd -= cut; sh += cut; }
      p.shift[c][nf] = (u8)sh;
      p.width[c][nf] = (u8)wd;
      m |= ((wd >= 64) ? (unsigned __int128)~0ull : (((unsigned __int128)1 << wd) - 1)) << sh;
      bits += wd;
      nf++;
    }
    p.mask[c] = W2{(u64)(m >> 64), (u64)m};
    p.nfield[c] = (u8)nf;
    if (bits > maxbits) maxbits = bits;
    c++;
    int t = (int)k - 1;
    while (t >= 0 && idx[t] == sgm - k + (u32)t) t--;
    if (t < 0) break;
    idx[t]++;
    for (u32 q = (u32)t + 1; q < k; q++) idx[q] = idx[q - 1] + 1;
    if (c >= MAX_COMBOS) {           // unreachable (C(best_s, k) <= MAX_COMBOS was checked above); never overrun
      memset(&p, 0, sizeof p);
      p.ncombo = 1;
      return p;
    }
  }
  p.ncombo = c;
  p.key_bits = maxbits;
  return p;
}

#include "pass_timing.hip.h"

// ---- cluster stage shared by the full pipeline and the explicit-graph entry point ------
// The arrays a graph lives in: per unique word (legacy view: deg / nbr_off / ... of the context) or per
// COMPACT node (cg_* buffers, kernels_cgraph.hip.h).  n nodes, cnt[n] their counts.
struct GraphArrays {
  u32 *deg, *parent, *csize, *off, *idx, *cl_of, *maxleaf;
  u64 *cl_size;
};
static GraphArrays legacy_arrays(humid_ctx *c) {
  return GraphArrays{c->deg.as<u32>(), c->parent.as<u32>(), c->csize.as<u32>(), c->nbr_off.as<u32>(), c->nbr_idx.as<u32>(),
                     c->cl_of.as<u32>(), c->maxleaf.as<u32>(), c->cl_size.as<u64>()};
}
// needs: cnt[n], deg[n], off[n+1], idx, parent[n] + csize[n] (k_comp_stats done), M = nodes with deg > 0,
// Mbig = those in components larger than SMALL_COMP; small_roots listed by k_comp_count.
// Leaves cl_of (creator + 1) / maxleaf / cl_size (at the creators) in `g`.
// trivial_done: the components of one and two nodes are done and the roots listed (k_cg_trivial)
// late_m (with trivial_done): U and M are bounds and Mbig is not known yet -- the device's node count (*late_m) and
// CTR_MEMBERS are fetched while k_cluster_small_lds runs (read_counters_begin / _end), before the kernels that need them
// exact; *late_m_out = the node count
static int cluster_kernels(humid_ctx *c, const GraphArrays &g, const u32 *g_cnt, u32 U, u64 M, u64 Mbig, u32 method,
                           bool trivial_done = false, const u32 *late_m = nullptr, u64 *late_m_out = nullptr) {
  hipStream_t st = c->stream;
  if (!trivial_done) TRY(mark_kernel(c, c->kev[KEV_CLUSTER_BEGIN]));
  if (trivial_done) {
  } else if (method == HUMID_METHOD_MAXIMUM)
    hipLaunchKernelGGL(k_cluster_trivial<true>, dim3(blocks_for(U)), dim3(256), 0, st, g.deg, g.parent, g.csize, U, g_cnt, g.off,
                       g.idx, g.cl_of, g.maxleaf, g.cl_size);
  else
    hipLaunchKernelGGL(k_cluster_trivial<false>, dim3(blocks_for(U)), dim3(256), 0, st, g.deg, g.parent, g.csize, U, g_cnt, g.off,
                       g.idx, g.cl_of, g.maxleaf, g.cl_size);
  if (M > 0) {
    const u64 small_cap = M / 3 + 1;                  // listed roots: components of >= 3 of the M leaves with neighbours
    if (late_m) TRY(read_counters_begin(c, nullptr, nullptr, late_m));
    if (method == HUMID_METHOD_MAXIMUM)
      hipLaunchKernelGGL(k_cluster_small_lds<true>, dim3(blocks_for(small_cap, 64)), dim3(64), 0, st, c->small_roots.as<u32>(),
                         (const ull *)c->d_ctr, g.parent, g.csize, U, g_cnt, g.off, g.idx, g.cl_of, g.maxleaf, g.cl_size);
    else
      hipLaunchKernelGGL(k_cluster_small_lds<false>, dim3(blocks_for(small_cap, 64)), dim3(64), 0, st, c->small_roots.as<u32>(),
                         (const ull *)c->d_ctr, g.parent, g.csize, U, g_cnt, g.off, g.idx, g.cl_of, g.maxleaf, g.cl_size);
    if (late_m) {
      TRY(read_counters_end(c, true));
      Mbig = c->h_ctr[CTR_MEMBERS];
      M = c->h_ctr[CTR_N - 3] & 0xffffffffull;
      U = (u32)M;
      if (late_m_out) *late_m_out = M;
    }
    if (Mbig > 0) {
      ENSURE(c->mk0, (size_t)Mbig * 8);
      ENSURE(c->mk1, (size_t)Mbig * 8);
      ENSURE(c->stk, (size_t)Mbig * 8);
      HIPCHK(hipMemsetAsync(&c->d_ctr[CTR_SPECIAL], 0, sizeof(ull), st));
      hipLaunchKernelGGL(k_member_keys, dim3(COMPACT_BLOCKS), dim3(256), 0, st, g.deg, g.parent, g.csize, U, c->mk0.as<u64>(), c->d_ctr);
      TRY(sort_keys<u64>(c, c->mk0.as<u64>(), c->mk1.as<u64>(), Mbig, 0, 32 + bits_for(U)));
      if (method == HUMID_METHOD_MAXIMUM) {
        // maxLeaf ties are broken by depth-first pre-order: one lane per component
        hipLaunchKernelGGL(k_cluster_components<true>, dim3(blocks_for(Mbig, 64)), dim3(64), 0, st,
                           c->mk1.as<u64>(), (u32)Mbig, g_cnt, g.off, g.idx, g.cl_of, g.maxleaf, g.cl_size, c->stk.as<u32>());
      } else if (c->coop_big) {
        // one workgroup per component, flood as a parallel BFS
        ENSURE(c->heads, (size_t)Mbig * 4);
        HIPCHK(hipMemsetAsync(&c->d_ctr[CTR_SPECIAL], 0, sizeof(ull), st));
        hipLaunchKernelGGL(k_comp_heads, dim3(COMPACT_BLOCKS), dim3(256), 0, st, c->mk1.as<u64>(), (u32)Mbig,
                           c->heads.as<u32>(), c->d_ctr);
        const u32 grid = (u32)(Mbig / (SMALL_COMP + 1) + 1 < 2048 ? Mbig / (SMALL_COMP + 1) + 1 : 2048);
        hipLaunchKernelGGL(k_cluster_big_coop, dim3(grid), dim3(256), 0, st, c->mk1.as<u64>(), (u32)Mbig,
                           c->heads.as<u32>(), c->d_ctr, g_cnt, g.off, g.idx, g.cl_of, g.maxleaf, g.cl_size, c->stk.as<u32>());
      } else {
        hipLaunchKernelGGL(k_cluster_components<false>, dim3(blocks_for(Mbig, 64)), dim3(64), 0, st,
                           c->mk1.as<u64>(), (u32)Mbig, g_cnt, g.off, g.idx, g.cl_of, g.maxleaf, g.cl_size, c->stk.as<u32>());
      }
    }
  }
  TRY(mark_kernel(c, c->kev[KEV_CLUSTER_END]));
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// the legacy view: clusters over all U unique words, then creator flags and their prefix sum
static int cluster_stage(humid_ctx *c, const u32 *g_cnt, u32 U, u64 M, u64 Mbig, u32 method) {
  hipStream_t st = c->stream;
  ENSURE(c->cl_of, (size_t)U * 4);
  ENSURE(c->maxleaf, (size_t)U * 4);
  ENSURE(c->cl_size, (size_t)U * 8);
  ENSURE(c->flag, (size_t)U * 4);
  ENSURE(c->pos, (size_t)(U + 1) * 4);
  ENSURE(c->cid, (size_t)U * 4);
  ENSURE(c->ismax, (size_t)U);
  TRY(cluster_kernels(c, legacy_arrays(c), g_cnt, U, M, Mbig, method));
  hipLaunchKernelGGL(k_creator_flags, dim3(blocks_for(U)), dim3(256), 0, st, c->cl_of.as<u32>(), U,
                     c->flag.as<u32>());
  TRY(exscan_u32(c, c->flag.as<u32>(), c->pos.as<u32>(), U));
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

static int n_clusters_from_scan(humid_ctx *c, u32 U, u64 *out) {
  // (the pass's last host wait: both values through the counters' mapped store)
  TRY(read_counters(c, c->pos.as<u32>() + (U - 1), c->flag.as<u32>() + (U - 1), nullptr, c->timing.stamp_live ? c->d_stamp : nullptr));
  *out = (c->h_ctr[CTR_N - 1] & 0xffffffffull) + (c->h_ctr[CTR_N - 2] & 0xffffffffull);
  return HUMID_OK;
}

#include "stage_count.hip.h"

// buckets longer than k_pairs' bounded walk, over the walked order W[0, n) of one combination: device list at
// c->big_runs + slot * cap (start, length, first tile), host copy in `runs` with the total as a last entry
template <class WT>
// cap_n (0: n): the array length the slots of the device list are sized by -- one value for all combinations of a
// caller that keeps several lists at once
static int find_big_runs(humid_ctx *c, const WT *W, u32 n, WT mask, u32 walk_max, u32 slot, std::vector<BigRun> &runs,
                         const BigRun **d_runs_out, u32 cap_n = 0) {
  hipStream_t st = c->stream;
  const u32 cap = (cap_n ? cap_n : n) / (walk_max + 2) + 1;       // runs are disjoint and longer than walk_max + 1
  ENSURE(c->big_runs, (size_t)MAX_COMBOS * cap * sizeof(BigRun) + 16);
  u32 *d_n = (u32 *)((char *)c->big_runs.p + (size_t)MAX_COMBOS * cap * sizeof(BigRun));
  BigRun *d_runs = c->big_runs.as<BigRun>() + (size_t)slot * cap;
  HIPCHK(hipMemsetAsync(d_n, 0, 4, st));
  hipLaunchKernelGGL(k_big_runs<WT>, dim3(blocks_for(n)), dim3(256), 0, st, W, n, mask, walk_max, d_runs, cap, d_n);
  u32 n_runs = 0;
  HIPCHK(hipMemcpyAsync(&n_runs, d_n, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (n_runs > cap) return fail(c, HUMID_E_INVALID, "more large buckets (%u) than fit the input (%u)", n_runs, cap);
  runs.resize(n_runs);
  if (n_runs) HIPCHK(hipMemcpy(runs.data(), d_runs, (size_t)n_runs * sizeof(BigRun), hipMemcpyDeviceToHost));
  std::sort(runs.begin(), runs.end(), [](const BigRun &x, const BigRun &y) { return x.start < y.start; });
  ull tiles = 0;
  for (BigRun &x : runs) {
    const ull nt = ((ull)x.len + PT2_TILE - 1) / PT2_TILE;
    x.tile0 = tiles;
    tiles += nt * (nt + 1) / 2;
  }
  runs.push_back(BigRun{0u, 0u, tiles});                          // sentinel: the total
  if (n_runs) HIPCHK(hipMemcpy(d_runs, runs.data(), (size_t)n_runs * sizeof(BigRun), hipMemcpyHostToDevice));
  *d_runs_out = d_runs;
  return HUMID_OK;
}

// Keys of at most 24 bits (any combination of one-word words): bucket order by GROUPING in two hand-written levels
// (kernels_part.hip.h: the tile partition by the top d1 <= 9 key bits, k_group_fine by the rest) instead
// of a library sort; only that equal keys end up next to each other matters.  *done = false: not this
// shape (the caller sorts).
// the fields of combination cb as a kernel argument
static ComboFields plan_fields(const ComboPlan &plan, u32 cb) {
  ComboFields cf;
  cf.nf = plan.nfield[cb];
  for (u32 f = 0; f < MAX_FIELDS; f++) { cf.shift[f] = plan.shift[cb][f]; cf.width[f] = plan.width[cb][f]; }
  return cf;
}
// A neighbour search that may ride in a grouping (stage_graph_compact): `group` is the search of the combination
// being grouped, walked inside k_group_fine.  Taken only where every coarse bin is certain to be a small one (padded
// bins of at most GF_SMALL words) -- did_group says whether; if not the caller launches k_pairs_append.
// ev_group: events around the launch the search rode in, as kernel marks (null: none).
struct GroupRide {
  PairSearchDev group;
  bool did_group = false;
  hipEvent_t ev_group[2] = {nullptr, nullptr};
  // option group_records: word_bits = the significant bits of a word (0: not known, the order is stored).  Where the
  // ride is taken and a word squeezed by its coarse bin fits an 8-byte record beside its walk index, the grouping moves
  // records and stores NO order (ws / vs untouched): no_order.
  u32 word_bits = 0;
  bool no_order = false;
};
static void group_fine_recs_with_search(humid_ctx *c, const FieldsSrc &src, const RecSqueeze &sq, const u64 *recs, u32 *cursor, u32 d1, u32 d2,
                                        u32 ibits, u32 cap1, const PairSearchDev &s);
// (the launch layer of the neighbour search, below)
static void group_fine_with_search(humid_ctx *c, const FieldsSrc &src, const u64 *k0, const u32 *v0, const u32 *cbase, u32 d1, u32 d2, u64 *ws,
                                   u32 *vs, u32 cap1, const PairSearchDev &s);
template <class SRC, class WT>
static int group_words_by_stretch(humid_ctx *c, const ComboPlan &plan, u32 cb, const WT *W, u32 n, u64 *ws, u32 *vs, bool *done,
                                  bool may_pad = false, GroupRide *ride = nullptr) {
  hipStream_t st = c->stream;
  u32 bit_n = 0;
  for (u32 f = 0; f < plan.nfield[cb]; f++) bit_n += plan.width[cb][f];
  *done = c->group_buckets && plan.nfield[cb] >= 1 && bit_n >= 2 && bit_n <= 24 && n >= 4096;
  c->gf_valid = nullptr;
  if (!*done) return HUMID_OK;
  const u32 d1 = bit_n >= 18 ? 9u : (bit_n + 1) / 2, d2 = bit_n - d1;          // d2 <= 15: 2^15 LDS counters at most
  const u32 nb1 = 1u << d1;
  // may_pad (the caller reads CTR_GOVER at its host wait and comes back without it when a bin was full): level 1
  // scatters into PADDED coarse bins (mean + 25 % + 1024, as the count stage's first level) -- no histogram pass
  // over the words in front, the bins' counts are the cursors left behind; and no bin can hold more than its
  // room, so the launches for bin sizes beyond it are left out
  const bool padded = may_pad && c->gf_padded;
  const u32 cap1 = padded ? n / nb1 + n / nb1 / 4 + 1024 : 0u;
  const size_t room = padded ? (size_t)nb1 * cap1 : (size_t)n;
  const SRC src{W, plan_fields(plan, cb), bit_n};
  const u32 tiles1 = (n + PT_TILE - 1) / PT_TILE;
  u32 *cursor1 = nullptr;
  if (padded) {                                              // its own cursors, cleared by the kernel that reads them
    if (!c->gf_cur.p) {
      ENSURE(c->gf_cur, 512 * 4);
      HIPCHK(hipMemsetAsync(c->gf_cur.p, 0, 512 * 4, st));
    }
    cursor1 = c->gf_cur.as<u32>();
  }
  ENSURE(c->seg_k0, room * 8);
  const bool ride_ok = ride && std::is_same<SRC, FieldsSrc>::value && padded && cap1 <= GF_SMALL;   // every bin is a SIZE-0 bin
  if constexpr (std::is_same<SRC, FieldsSrc>::value) {
    // the search rides and nobody else reads this order: 8-byte records through level 1 (8192 of them are 64 KB of LDS: two
    // workgroups per CU, the tiles of U = 2.7 M words in ONE round), no scan of the cursors (k_group_fine_recs reads and
    // clears its own), no order stored.  Needs none of the scratch below: no walk indices beside the records, no bin
    // bases, no tile table.
    const u32 ibits = bits_for(n), wb = ride_ok ? ride->word_bits : 0u;
    if (ride_ok && c->group_records && wb && plan.width[cb][0] >= d1 && wb - d1 + ibits <= 64) {
      const RecSqueeze sq{(u32)plan.shift[cb][0] + plan.width[cb][0] - d1, d1};
      const FieldsRecs rsrc{W, sq, wb - d1};
      hipLaunchKernelGGL((k_p8_scatter1<FieldsRecs, 1024, CTR_GOVER>), dim3(tiles1), dim3(1024), 0, st, rsrc, n, wb, d1, ibits, cap1, cursor1,
                         c->seg_k0.as<u64>(), c->d_ctr);
      if (ride->ev_group[0]) TRY(mark_kernel(c, ride->ev_group[0]));
      group_fine_recs_with_search(c, src, sq, c->seg_k0.as<u64>(), cursor1, d1, d2, ibits, cap1, ride->group);
      if (ride->ev_group[1]) TRY(mark_kernel(c, ride->ev_group[1]));
      ride->did_group = ride->no_order = true;
      HIPCHK(hipGetLastError());
      return HUMID_OK;
    }
  }
  ENSURE(c->seg_v0, room * 4);
  // scratch: [hist1 512 | cursor1 512] zeroed, then [cbase 513 | tprefix 513 | pbeg dummy 514]
  ENSURE(c->pt_work, (size_t)(1024 + 513 + 513 + 516) * 4);
  u32 *hist1 = c->pt_work.as<u32>(), *cbase = hist1 + 1024, *tprefix = cbase + 513, *dummy = tprefix + 513;
  if (!padded) {
    cursor1 = hist1 + 512;
    HIPCHK(hipMemsetAsync(c->pt_work.p, 0, 1024 * 4, st));
    hipLaunchKernelGGL(k_pt_hist1<SRC>, dim3(tiles1 < 512 ? tiles1 : 512), dim3(1024), 0, st, src, n, d1, hist1);
    hipLaunchKernelGGL(k_pt_scan1, dim3(1), dim3(1024), 0, st, (const u32 *)hist1, d1, 0u, cbase, tprefix, dummy, dummy + 513, 0u);
  }
  static const bool gs_small = getenv("HUMID_GS_THREADS") ? atoi(getenv("HUMID_GS_THREADS")) == 512 : false;  // (experiments: 512-thread tiles are 7 us slower -- shorter runs per bin)
  if (gs_small)
    hipLaunchKernelGGL((k_pt_scatter<1, SRC, 512>), dim3((n + 4095) / 4096), dim3(512), 0, st, src, n, (const u64 *)nullptr,
                       (const u32 *)nullptr, (const u32 *)nullptr, (const u32 *)nullptr, d1, d2, (const u32 *)cbase, cursor1,
                       c->seg_k0.as<u64>(), c->seg_v0.as<u32>(), (u32 *)nullptr, cap1, &c->d_ctr[CTR_GOVER]);
  else
    hipLaunchKernelGGL((k_pt_scatter<1, SRC>), dim3(tiles1), dim3(1024), 0, st, src, n, (const u64 *)nullptr,
                       (const u32 *)nullptr, (const u32 *)nullptr, (const u32 *)nullptr, d1, d2, (const u32 *)cbase, cursor1,
                       c->seg_k0.as<u64>(), c->seg_v0.as<u32>(), (u32 *)nullptr, cap1, &c->d_ctr[CTR_GOVER]);
  if (padded)
    hipLaunchKernelGGL(k_pt_scan1, dim3(1), dim3(1024), 0, st, (const u32 *)cursor1, d1, 0u, cbase, tprefix, dummy, dummy + 513, cap1, cursor1);
  // up to three launches over the coarse bins, by bin size; which sizes cannot occur is known from n alone only
  // roughly (the bins of a skewed key can be any size) unless the bins are padded, so only the impossible
  // ones are left out
  c->gf_valid = padded ? (const u32 *)(cbase + nb1) : (const u32 *)nullptr;    // words the order holds (< n: a bin was full)
  const u32 largest = padded ? cap1 : n;
  if (ride_ok) {
    if constexpr (std::is_same<SRC, FieldsSrc>::value) {
      if (ride->ev_group[0]) TRY(mark_kernel(c, ride->ev_group[0]));
      group_fine_with_search(c, src, c->seg_k0.as<u64>(), c->seg_v0.as<u32>(), cbase, d1, d2, ws, vs, cap1, ride->group);
      if (ride->ev_group[1]) TRY(mark_kernel(c, ride->ev_group[1]));
      ride->did_group = true;
    }
  } else
  hipLaunchKernelGGL((k_group_fine<SRC, 0>), dim3(nb1), dim3(GF_THREADS), 0, st, src,
                     (const u64 *)c->seg_k0.as<u64>(), (const u32 *)c->seg_v0.as<u32>(), (const u32 *)cbase, d1, d2, ws, vs, cap1);
  if (largest > GF_SMALL)
    hipLaunchKernelGGL((k_group_fine<SRC, 1>), dim3(nb1), dim3(GF_THREADS), 0, st, src,
                       (const u64 *)c->seg_k0.as<u64>(), (const u32 *)c->seg_v0.as<u32>(), (const u32 *)cbase, d1, d2, ws, vs, cap1);
  if (largest > GF_MID)
    hipLaunchKernelGGL((k_group_fine<SRC, 2>), dim3(nb1), dim3(GF_THREADS), 0, st, src,
                       (const u64 *)c->seg_k0.as<u64>(), (const u32 *)c->seg_v0.as<u32>(), (const u32 *)cbase, d1, d2, ws, vs, cap1);
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// A combination whose key is ONE stretch of the word (a single segment, or neighbouring segments):
// the words themselves are the sort keys over that bit range and come out in bucket order (ws), the
// positions ride along as values (vs) -- no key array, and no gather of the words afterwards (44 us
// and 320 MB of traffic at 10 M reads; the 8-byte keys cost the sort 19 us more: tools/sort_probe.hip).
// *done = false: the key is not one stretch, nothing was queued.
static int sort_words_by_stretch(humid_ctx *c, const ComboPlan &plan, u32 cb, const u64 *W, u32 n, u64 *ws, u32 *vs, bool *done) {
  u32 bit_lo = 0, bit_n = 0;
  bool stretch = plan.nfield[cb] >= 1;
  for (u32 f = 0; stretch && f < plan.nfield[cb]; f++) {
    if (f + 1 < plan.nfield[cb] && plan.shift[cb][f] != plan.shift[cb][f + 1] + plan.width[cb][f + 1]) stretch = false;
    bit_n += plan.width[cb][f];
    bit_lo = plan.shift[cb][f];
  }
  *done = stretch && bit_n >= 1 && bit_lo + bit_n <= 64;
  if (!*done) return HUMID_OK;
  return sort_pairs_in<u64, u32>(c, PtrIn<u64>{W}, ws, IotaIn{}, vs, n, bit_lo, bit_lo + bit_n);
}

// keys of the fields cf of src[0 .. n), sorted: kout = the keys ascending (u32 where key_bits <= 32, else u64),
// vout = the index in src of each.  Scratch: seg_k0 / seg_v0.  The only place that launches k_combo_keys.
template <class WT>
static int combo_keys_sorted(humid_ctx *c, const WT *src, u32 n, const ComboFields &cf, u32 key_bits, void *kout, u32 *vout) {
  auto go = [&](auto key) -> int {
    using KT = decltype(key);
    hipLaunchKernelGGL((k_combo_keys<KT, WT>), dim3(blocks_for(n)), dim3(256), 0, c->stream, src, n, cf, c->seg_k0.as<KT>(),
                       c->seg_v0.as<u32>());
    return sort_pairs<KT, u32>(c, c->seg_k0.as<KT>(), (KT *)kout, c->seg_v0.as<u32>(), vout, n, 0, key_bits);
  };
  return key_bits <= 32 ? go(u32{}) : go(u64{});
}

// words of the unique array in bucket order of combination `seg` (> 0): ws[i] = the word walked at
// position i, vs[i] = its walk index.  Keys of <= 24 bits: two-level grouping; one stretch of the word:
// the words themselves as sort keys; else keys + sort + gather.  Scratch: seg_k0 / seg_v0 / seg_ks.
template <class WT>
static int bucket_order(humid_ctx *c, const ComboPlan &plan, u32 seg, const WT *g_word, u32 U, WT *ws, u32 *vs, bool may_pad = false,
                        GroupRide *ride = nullptr) {
  hipStream_t st = c->stream;
  u32 kb = 0;                                            // key bits of THIS combination
  for (u32 f = 0; f < plan.nfield[seg]; f++) kb += plan.width[seg][f];
  if (kb == 0) kb = 1;
  bool stretch = false;
  if (std::is_same<WT, u64>::value) {
    TRY((group_words_by_stretch<FieldsSrc, u64>(c, plan, seg, (const u64 *)g_word, U, (u64 *)ws, vs, &stretch, may_pad, ride)));
    if (!stretch) TRY(sort_words_by_stretch(c, plan, seg, (const u64 *)g_word, U, (u64 *)ws, vs, &stretch));
  } else {
    // two-word words: the keys are grouped (scratch), the words follow through the grouped positions
    TRY((group_words_by_stretch<FieldsSrcW2, W2>(c, plan, seg, (const W2 *)g_word, U, c->seg_ks.as<u64>(), vs, &stretch, may_pad)));
    if (stretch) hipLaunchKernelGGL(k_gather_bucket_words<WT>, dim3(blocks_for(U)), dim3(256), 0, st, g_word, vs, U, ws, c->gf_valid);
  }
  if (stretch) return HUMID_OK;
  TRY(combo_keys_sorted<WT>(c, g_word, U, plan_fields(plan, seg), kb, c->seg_ks.p, vs));
  hipLaunchKernelGGL(k_gather_bucket_words<WT>, dim3(blocks_for(U)), dim3(256), 0, st, g_word, vs, U, ws);
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// ---- the launch layer of the Hamming neighbour search ------------------------------------
// A driver of the search (stage_graph, stage_graph_compact, emit_orders in humid_exchange.hip) says WHAT is
// walked (Walked) and WHERE a found pair goes (CsrSink, EmitSink); k_pairs, k_pairs_tiles, k_pairs_append and the
// k_group_fine / k_group_fine_recs that a search rides in (GroupRide) are launched by the seven functions below and nowhere else.  Each holds the one (PASS0, MODE) dispatch of its
// kernel and the only spelling of the null pointers for the sinks a mode does not use, so a change to how a
// bucket is walked -- a kernel argument, a bound, a bucket left out -- is made here.
template <class WT>
struct Walked {            // the walked order of one combination
  const WT *W;             // the words in the order walked
  const u32 *V;            // their walk indices; null: the positions themselves (the prefix combination, PASS0)
  u32 n;
  WT mask;                 // the combination's mask
  u32 cb;                  // and its number
};
template <class WT>
struct PairSearch { EarlierMasksT<WT> em; u32 distance, walk_max; };   // what the combinations of one search share
struct CsrSink { u32 *deg, *parent; const u32 *nbr_off; u32 *cur, *nbr_idx, *had; const u32 *join_cnt; };
struct EmitSink { u32 *pc; const u32 *poff; u64 *edges; ull *ecount; };

template <class WT>
static EarlierMasksT<WT> earlier_masks(const ComboPlan &plan) {   // masks of all combinations, for the first-combination rule
  EarlierMasksT<WT> em;
  for (u32 t = 0; t < MAX_COMBOS; t++) em.m[t] = w_from<WT>(plan.mask[t]);
  return em;
}
template <class WT>
static PairSearch<WT> pair_search(const humid_ctx *c, const ComboPlan &plan, u32 distance) {
  return PairSearch<WT>{earlier_masks<WT>(plan), distance, c->walk_max};
}
// a driver that keeps the orders of combinations 1 .. nseg-1 over U words: order seg at seg_ws / seg_vs + (seg-1) U
template <class WT>
static int ensure_seg_scratch(humid_ctx *c, u32 nseg, u32 U) {
  if (nseg < 2) return HUMID_OK;
  ENSURE(c->seg_k0, (size_t)U * 8);
  ENSURE(c->seg_v0, (size_t)U * 4);
  ENSURE(c->seg_ks, (size_t)U * 8);                          // sorted keys: scratch, not kept
  ENSURE(c->seg_vs, (size_t)(nseg - 1) * U * 4);             // walk indices in bucket order, per combination
  ENSURE(c->seg_ws, (size_t)(nseg - 1) * U * sizeof(WT));    // words in bucket order, per combination
  return HUMID_OK;
}
template <class WT>
static WT *seg_ws(humid_ctx *c, u32 seg, u32 U) { return c->seg_ws.as<WT>() + (size_t)(seg - 1) * U; }
static u32 *seg_vs(humid_ctx *c, u32 seg, u32 U) { return c->seg_vs.as<u32>() + (size_t)(seg - 1) * U; }
template <class WT>
static Walked<WT> walked_seg(humid_ctx *c, const ComboPlan &plan, u32 seg, const WT *g_word, u32 U) {
  return Walked<WT>{seg ? seg_ws<WT>(c, seg, U) : g_word, seg ? seg_vs(c, seg, U) : nullptr, U, w_from<WT>(plan.mask[seg]), seg};
}

// f(PASS0, MODE) as integral constants, MODE = fill ? M_FILL : M_COUNT
template <int M_COUNT, int M_FILL, class F>
static void for_pass_mode(bool pass0, bool fill, F f) {
  const std::integral_constant<int, M_COUNT> mc;
  const std::integral_constant<int, M_FILL> mf;
  if (pass0) { if (fill) f(std::true_type{}, mf); else f(std::true_type{}, mc); }
  else { if (fill) f(std::false_type{}, mf); else f(std::false_type{}, mc); }
}

// k_pairs over the positions [i0, i0 + n_i) of an order; mode PM_COUNT (`big`: where a bucket beyond the walk sets the
// combination's bit) or PM_FILL
template <class WT>
static void pairs_csr(humid_ctx *c, const PairSearch<WT> &s, const Walked<WT> &w, int mode, u32 i0, u32 n_i, const CsrSink &k, ull *big) {
  const bool fill = mode == PM_FILL;
  for_pass_mode<PM_COUNT, PM_FILL>(!w.V, fill, [&](auto p0, auto m) {
    hipLaunchKernelGGL((k_pairs<decltype(p0)::value, decltype(m)::value, WT>), dim3(blocks_for(n_i)), dim3(256), 0, c->stream, w.W, w.V,
                       w.n, i0, n_i, w.mask, s.em, w.cb, s.distance, fill ? nullptr : k.deg, fill ? nullptr : k.parent,
                       fill ? k.nbr_off : nullptr, fill ? k.cur : nullptr, fill ? k.nbr_idx : nullptr, (u32 *)nullptr,
                       (const u32 *)nullptr, (u64 *)nullptr, k.had, s.walk_max, fill ? nullptr : big, fill ? nullptr : k.join_cnt);
  });
}
// the same with mode PM_EMIT_COUNT or PM_EMIT_FILL
template <class WT>
static void pairs_emit(humid_ctx *c, const PairSearch<WT> &s, const Walked<WT> &w, int mode, u32 i0, u32 n_i, const EmitSink &k, ull *big) {
  const bool fill = mode == PM_EMIT_FILL;
  for_pass_mode<PM_EMIT_COUNT, PM_EMIT_FILL>(!w.V, fill, [&](auto p0, auto m) {
    hipLaunchKernelGGL((k_pairs<decltype(p0)::value, decltype(m)::value, WT>), dim3(blocks_for(n_i)), dim3(256), 0, c->stream, w.W, w.V,
                       w.n, i0, n_i, w.mask, s.em, w.cb, s.distance, (u32 *)nullptr, (u32 *)nullptr, (const u32 *)nullptr,
                       (u32 *)nullptr, (u32 *)nullptr, k.pc, k.poff, k.edges, (u32 *)nullptr, s.walk_max, fill ? nullptr : big,
                       (const u32 *)nullptr);
  });
}
// k_pairs_tiles over the large buckets of an order (find_big_runs: device list d_runs, host copy runs): the pairs
// further apart than the walk.  Nothing is launched where there is no such bucket.
template <class WT>
static void tiles_csr(humid_ctx *c, const PairSearch<WT> &s, const Walked<WT> &w, const BigRun *d_runs, const std::vector<BigRun> &runs,
                      int mode, const CsrSink &k) {
  if (runs.size() < 2) return;
  const ull tiles = runs.back().tile0;
  for_pass_mode<PM_COUNT, PM_FILL>(!w.V, mode == PM_FILL, [&](auto p0, auto m) {
    hipLaunchKernelGGL((k_pairs_tiles<decltype(p0)::value, decltype(m)::value, WT>), dim3((u32)std::min<ull>(tiles, 1u << 20)),
                       dim3(PT2_THREADS), 0, c->stream, w.W, w.V, d_runs, (u32)runs.size() - 1, tiles, s.em, w.cb, s.distance, s.walk_max,
                       k.deg, k.parent, k.nbr_off, k.cur, k.nbr_idx, k.join_cnt, (u64 *)nullptr, (ull *)nullptr, 0u, 0xffffffffu);
  });
}
// the same for the emit modes; [i_lo, i_hi): only pairs whose first position lies in that range
template <class WT>
static void tiles_emit(humid_ctx *c, const PairSearch<WT> &s, const Walked<WT> &w, const BigRun *d_runs, const std::vector<BigRun> &runs,
                       int mode, const EmitSink &k, u32 i_lo = 0, u32 i_hi = 0xffffffffu) {
  if (runs.size() < 2) return;
  const ull tiles = runs.back().tile0;
  for_pass_mode<PM_EMIT_COUNT, PM_EMIT_FILL>(!w.V, mode == PM_EMIT_FILL, [&](auto p0, auto m) {
    hipLaunchKernelGGL((k_pairs_tiles<decltype(p0)::value, decltype(m)::value, WT>), dim3((u32)std::min<ull>(tiles, 1u << 20)),
                       dim3(PT2_THREADS), 0, c->stream, w.W, w.V, d_runs, (u32)runs.size() - 1, tiles, s.em, w.cb, s.distance, s.walk_max,
                       (u32 *)nullptr, (u32 *)nullptr, (const u32 *)nullptr, (u32 *)nullptr, (u32 *)nullptr, (const u32 *)nullptr,
                       k.edges, k.ecount, i_lo, i_hi);
  });
}
// k_pairs_append over a whole order; n_valid: the words a padded grouping holds (bucket_order with may_pad)
template <class WT>
static void pairs_append(humid_ctx *c, const PairSearch<WT> &s, const Walked<WT> &w, const EdgeRegs &er, u32 *bits, u32 *multi, ull *big,
                         u32 *overflow, const u32 *n_valid) {
  const dim3 grid(blocks_for(w.n, PA_PPT * 256)), blk(256);
  const PairRule<WT> rule{w.mask, s.em, w.cb, s.distance, s.walk_max};
  if (w.V && multi)
    hipLaunchKernelGGL((k_pairs_append<false, WT, true>), grid, blk, 0, c->stream, w.W, w.V, w.n, rule, er, bits, multi, big, overflow, n_valid);
  else if (w.V)
    hipLaunchKernelGGL((k_pairs_append<false, WT>), grid, blk, 0, c->stream, w.W, w.V, w.n, rule, er, bits, multi, big, overflow, n_valid);
  else if (multi)
    hipLaunchKernelGGL((k_pairs_append<true, WT, true>), grid, blk, 0, c->stream, w.W, w.V, w.n, rule, er, bits, multi, big, overflow, n_valid);
  else
    hipLaunchKernelGGL((k_pairs_append<true, WT>), grid, blk, 0, c->stream, w.W, w.V, w.n, rule, er, bits, multi, big, overflow, n_valid);
}
// the same search as an argument of the kernel that holds the combination's words while it groups them (GroupRide)
static PairSearchDev pairs_append_dev(const PairSearch<u64> &s, u64 mask, u32 cb, const EdgeRegs &er, u32 *bits, u32 *multi, ull *big,
                                      u32 *overflow) {
  return PairSearchDev{PairRule<u64>{mask, s.em, cb, s.distance, s.walk_max}, er, bits, multi, big, overflow};
}
// level 2 of a grouping whose coarse bins all hold at most GF_SMALL words, with the grouped combination's search in it
static void group_fine_with_search(humid_ctx *c, const FieldsSrc &src, const u64 *k0, const u32 *v0, const u32 *cbase, u32 d1, u32 d2, u64 *ws,
                                   u32 *vs, u32 cap1, const PairSearchDev &s) {
  if (s.multi)
    hipLaunchKernelGGL((k_group_fine<FieldsSrc, 0, PairSearchDevT<true>>), dim3(1u << d1), dim3(GF_THREADS), 0, c->stream, src, k0, v0, cbase, d1, d2,
                       ws, vs, cap1, PairSearchDevT<true>{s.rule, s.er, s.bits, s.multi, s.big, s.overflow});
  else
    hipLaunchKernelGGL((k_group_fine<FieldsSrc, 0, PairSearchDev>), dim3(1u << d1), dim3(GF_THREADS), 0, c->stream, src, k0, v0, cbase, d1, d2, ws,
                       vs, cap1, s);
}
// the same over the 8-byte records of a padded level 1 (FieldsRecs), for the search alone: no order is stored
static void group_fine_recs_with_search(humid_ctx *c, const FieldsSrc &src, const RecSqueeze &sq, const u64 *recs, u32 *cursor, u32 d1, u32 d2,
                                        u32 ibits, u32 cap1, const PairSearchDev &s) {
  if (s.multi)
    hipLaunchKernelGGL((k_group_fine_recs<FieldsSrc, RecSqueeze, PairSearchDevT<true>>), dim3(1u << d1), dim3(GF_THREADS), 0, c->stream, src, sq, recs,
                       cursor, d1, d2, ibits, cap1, PairSearchDevT<true>{s.rule, s.er, s.bits, s.multi, s.big, s.overflow});
  else
    hipLaunchKernelGGL((k_group_fine_recs<FieldsSrc, RecSqueeze, PairSearchDev>), dim3(1u << d1), dim3(GF_THREADS), 0, c->stream, src, sq, recs, cursor,
                       d1, d2, ibits, cap1, s);
}
// component sizes and what is read from them (M, Mbig, 2E, the roots of the small components) for deg / parent over U nodes
static void comp_stats(humid_ctx *c, u32 U) {
  hipLaunchKernelGGL(k_comp_stats, dim3(blocks_for(U)), dim3(256), 0, c->stream, c->deg.as<u32>(), c->parent.as<u32>(), U, c->csize.as<u32>());
  hipLaunchKernelGGL(k_comp_count, dim3(512), dim3(256), 0, c->stream, c->deg.as<u32>(), c->parent.as<u32>(), c->csize.as<u32>(), U, c->d_ctr,
                     c->small_roots.as<u32>());
}

// ---- stage B: neighbours + clusters over a sorted unique array ---------------------------
// g_word[U] ascending, g_cnt[U] (device; the context's own arrays on one GPU, the gathered
// arrays of all ranks on several).  Leaves deg/nbr_off/nbr_idx/cl_of/maxleaf/cl_size/flag/
// pos/cid/ismax in the context.
// ext_edges != nullptr: the neighbour pairs are GIVEN (multi-GPU: every rank searched its share,
// humid_stage_pairs, and the shares were all-gathered); otherwise they are searched here.
// WT: u64 (n <= 32) or W2 (33 <= n <= 64, two uint64 per word).
template <class WT>
static int stage_graph(humid_ctx *c, const WT *g_word, const u32 *g_cnt, u32 U, u32 word_nt,
                       u32 distance, u32 method, humid_summary &s, u32 &n_pair_segs_out,
                       const u64 *ext_edges = nullptr, u64 n_ext_edges = 0) {
  hipStream_t st = c->stream;
  c->g_word = g_word;
  c->g_wpr = (u32)(sizeof(WT) / 8);
  c->g_cnt = g_cnt;
  c->gU = U;
  c->cg_valid = false;
  // ---------------- 3. neighbours -----------------
  // deg has U+1 entries (last stays 0) so that one exclusive scan yields nbr_off[U] = 2E
  ENSURE(c->deg, (size_t)(U + 1) * 4);
  ENSURE(c->nbr_off, (size_t)(U + 1) * 4);
  ENSURE(c->parent, (size_t)U * 4);
  ENSURE(c->csize, (size_t)U * 4);
  ENSURE(c->cur, (size_t)U * 4);
  ENSURE(c->small_roots, ((size_t)U / 3 + 2) * 4);
  HIPCHK(hipMemsetAsync(&c->d_ctr[CTR_EDGES], 0, (CTR_SMALLROOTS - CTR_EDGES + 1) * sizeof(ull), st));
  hipLaunchKernelGGL(k_graph_init, dim3(blocks_for((u64)U + 1)), dim3(256), 0, st, c->parent.as<u32>(),
                     c->deg.as<u32>(), c->csize.as<u32>(), c->cur.as<u32>(), U);
  u64 E = 0, M = 0, Mbig = 0;
  u32 n_pair_segs = 0;
  const ComboPlan plan = make_plan(word_nt - c->gk_nt, distance, U, c->force_segments, true, c->gk_nt);
  const PairSearch<WT> ps = pair_search<WT>(c, plan, distance);
  const bool given = ext_edges != nullptr;
  const bool search = !given && distance > 0 && U > 1;
  // directional method: only neighbour pairs a climb or a flood can cross join two components
  // (joins_for_clustering); maximum method: all of them
  const u32 *join_cnt = (method & 1) ? nullptr : g_cnt;

  // one bucket holding every word (d >= n, or d too large for any pigeonhole plan): U^2 / 2
  // comparisons and, at such distances, nearly as many pairs -- beyond a few 10^5 words the pair
  // list cannot fit 32-bit CSR offsets anyway; refuse before spending minutes to find that out
  if (search && plan.ncombo == 1 && plan.key_bits == 0 && U > (1u << 18))
    return fail(c, HUMID_E_OVERFLOW, "distance %u over %u-nt words compares all pairs of %u unique words: too many neighbour pairs",
                distance, word_nt, U);
  if (given && n_ext_edges) {
    hipLaunchKernelGGL(k_edges_apply<false>, dim3(grid_stride_blocks(n_ext_edges)), dim3(256), 0, st, ext_edges,
                       n_ext_edges, U, c->deg.as<u32>(), c->parent.as<u32>(), (const u32 *)nullptr,
                       (u32 *)nullptr, (u32 *)nullptr, c->d_ctr, join_cnt);
    comp_stats(c, U);
  }
  // buckets beyond k_pairs' bounded walk (c->walk_max words; 0 = walk to the end of the bucket)
  u64 big_mask = 0;
  std::vector<BigRun> h_runs[MAX_COMBOS];
  const BigRun *d_runs[MAX_COMBOS] = {nullptr};
  // where the pairs of combination seg go (the arrays as they are at the time of the launch)
  auto sink = [&](u32 seg) {
    return CsrSink{c->deg.as<u32>(), c->parent.as<u32>(), c->nbr_off.as<u32>(), c->cur.as<u32>(), c->nbr_idx.as<u32>(),
                   c->had.as<u32>() + (size_t)seg * U, join_cnt};
  };
  // one pass over the combinations: PM_COUNT makes the bucket orders and leaves degrees and the component forest,
  // PM_FILL walks the same orders again and writes the CSR rows, the tiles of the large buckets behind each
  auto search_pass = [&](int mode) -> int {
    const PairPhase phase = mode == PM_COUNT ? PAIRS_COUNT : PAIRS_FILL;
    for (u32 seg = 0; seg < plan.ncombo; seg++) {
      if (seg && mode == PM_COUNT) TRY(bucket_order<WT>(c, plan, seg, g_word, U, seg_ws<WT>(c, seg, U), seg_vs(c, seg, U)));
      const Walked<WT> w = walked_seg<WT>(c, plan, seg, g_word, U);
      TRY(mark_pairs(c, phase, seg, 0));
      pairs_csr<WT>(c, ps, w, mode, 0u, U, sink(seg), &c->d_ctr[CTR_BIGMASK]);
      if (mode == PM_FILL && (big_mask >> seg & 1)) tiles_csr<WT>(c, ps, w, d_runs[seg], h_runs[seg], PM_FILL, sink(seg));
      TRY(mark_pairs(c, phase, seg, 1));
    }
    HIPCHK(hipGetLastError());
    return HUMID_OK;
  };
  if (search) {
    n_pair_segs = plan.ncombo < 8 ? plan.ncombo : 8;
    ENSURE(c->had, (size_t)plan.ncombo * U * 4);            // per combination and position: pairs found, distance to the first
    TRY(ensure_seg_scratch<WT>(c, plan.ncombo, U));
    TRY(search_pass(PM_COUNT));
    comp_stats(c, U);
  }
  TRY(exscan_u32(c, c->deg.as<u32>(), c->nbr_off.as<u32>(), (u64)U + 1));
  if (search || (given && n_ext_edges)) {
    HIPCHK(hipGetLastError());
    TRY(read_counters(c, c->nbr_off.as<u32>() + U));   // h_ctr[CTR_N-1] = 2E
    if (c->h_ctr[CTR_OVERFULL]) return fail(c, HUMID_E_INVALID, "malformed edge list (node index out of range)");
    // the degrees summed in 64 bits (k_comp_count): the 32-bit scan below it may have wrapped
    if (c->h_ctr[CTR_EDGES] > 0xffffffffull)
      return fail(c, HUMID_E_OVERFLOW, "%llu neighbour pairs exceed the 32-bit adjacency offsets", (ull)(c->h_ctr[CTR_EDGES] / 2));
    big_mask = search ? c->h_ctr[CTR_BIGMASK] : 0;
    u64 twoE = c->h_ctr[CTR_N - 1] & 0xffffffffull;
    if (big_mask) {
      road_taken(c, HUMID_ROAD_CSR_TILES);
      // some bucket is longer than k_pairs walks: find those runs, count their remaining pairs as
      // tiles, and take the component statistics and the offsets again
      for (u32 seg = 0; seg < plan.ncombo; seg++)
        if (big_mask >> seg & 1) {
          const Walked<WT> w = walked_seg<WT>(c, plan, seg, g_word, U);
          TRY(find_big_runs<WT>(c, w.W, U, w.mask, ps.walk_max, seg, h_runs[seg], &d_runs[seg]));
          tiles_csr<WT>(c, ps, w, d_runs[seg], h_runs[seg], PM_COUNT, sink(seg));
          HIPCHK(hipGetLastError());
        }
      HIPCHK(hipMemsetAsync(&c->d_ctr[CTR_EDGES], 0, 3 * sizeof(ull), st));
      HIPCHK(hipMemsetAsync(&c->d_ctr[CTR_SMALLROOTS], 0, sizeof(ull), st));
      HIPCHK(hipMemsetAsync(c->csize.p, 0, (size_t)U * 4, st));
      comp_stats(c, U);
      TRY(scan_total(c, c->deg.as<u32>(), c->nbr_off.as<u32>(), U, &twoE));
      if (c->h_ctr[CTR_EDGES] > 0xffffffffull)
        return fail(c, HUMID_E_OVERFLOW, "%llu neighbour pairs exceed the 32-bit adjacency offsets", (ull)(c->h_ctr[CTR_EDGES] / 2));
    }
    E = twoE / 2;
    M = c->h_ctr[CTR_NONSINGLE];
    Mbig = c->h_ctr[CTR_MEMBERS];
  }
  s.edges = c->E = E;
  s.nonsingle = c->M = M;
  ENSURE(c->nbr_idx, (size_t)(2 * E + 1) * 4);
  if (E > 0) {
    if (given)
      hipLaunchKernelGGL(k_edges_apply<true>, dim3(grid_stride_blocks(n_ext_edges)), dim3(256), 0, st, ext_edges,
                         n_ext_edges, U, (u32 *)nullptr, (u32 *)nullptr, c->nbr_off.as<u32>(),
                         c->cur.as<u32>(), c->nbr_idx.as<u32>(), c->d_ctr);
    else
      TRY(search_pass(PM_FILL));
    hipLaunchKernelGGL(k_sort_lists, dim3(blocks_for(U)), dim3(256), 0, st, c->nbr_off.as<u32>(), U,
                       c->nbr_idx.as<u32>());
  }
  TRY(mark_stage(c, c->ev[EV_GRAPH_BUILT]));

  // clusters
  TRY(cluster_stage(c, g_cnt, U, M, Mbig, method));
  // one GPU: the graph is over this context's own unique words, so the per-slot result words can
  // be written in the same pass (stage C then skips k_slot_results)
  const bool own = ((const void *)g_word == c->s_word.p) && U == (u32)c->U && !given;
  hipLaunchKernelGGL(k_finalize_nodes, dim3(blocks_for(U)), dim3(256), 0, st, c->cl_of.as<u32>(),
                     c->pos.as<u32>(), c->maxleaf.as<u32>(), U, c->cid.as<u32>(), c->ismax.as<u8>(),
                     own ? c->s_first.as<u32>() : (const u32 *)nullptr,
                     own ? c->s_slot.as<u32>() : (const u32 *)nullptr,
                     own ? c->slot_out.as<u64>() : (u64 *)nullptr);
  c->slots_done = own;
  HIPCHK(hipGetLastError());
  n_pair_segs_out = n_pair_segs;
  return HUMID_OK;
}


// ---- the compact graph from marked ids + pairs (kernels_cgraph.hip.h): shared by the single-GPU search
// (pairs appended into regions, counts by id) and the multi-GPU pass (pair records in global ids) ----
struct CgSource {
  EdgeRegs er;                 // pairs in id space: regions + far list (recs == null); set to the compact pairs on return
  const ulonglong2 *recs;      // or: pair records {a << 32 | b, count a | count b << 32}
  u32 n_recs;
  const RecSegs *segs = nullptr;   // or: several record arrays (the multi-GPU pass: interior, crossing, flagged-interior of the others)
  const u32 *cnt_by_id;        // counts by id (with plain pairs)
  u32 n_ids;                   // id space = bits of the bitmap c->cg_bits (zeroed, then marked, by the caller)
  u64 pairs_bound;             // no more pairs than this can be in the source
  u32 *bits = nullptr;         // the bitmap of the marked ids if not c->cg_bits (the rest of a split stage: c->cg_rbits)
  bool no_wait = false;        // no host wait: the caller knows the pairs (er.e == null, a dense list of pairs_bound pairs),
                               // regions_max is not wanted and CgStatus is left alone
};
struct CgStatus {
  bool overflow = false;       // an append region was full: `wanted` says how much room the search wants in all
  bool group_over = false;     // a padded coarse bin of a bucket order was full (CTR_GOVER)
  u64 wanted = 0, big_mask = 0, E = 0, M = 0, Mbig = 0;
};
static GraphArrays cg_arrays(humid_ctx *c) {
  return GraphArrays{c->cg_deg.as<u32>(), c->cg_parent.as<u32>(), c->cg_csize.as<u32>(), c->cg_off.as<u32>(), c->cg_idx.as<u32>(),
                     c->cg_cl_of.as<u32>(), c->cg_maxleaf.as<u32>(), c->cg_cl_size.as<u64>()};
}
// rank structure, nodes, compact pairs, degrees, forest, CSR rows (ascending), component sizes, the trivial
// components; ONE host wait at the end (every launch before it is sized by bounds: nodes <= 2 x pairs).
// In two halves.  cg_build_front is what does not depend on the pairs, only on the bitmap of the marked ids: its rank
// blocks and the nodes with their per-node arrays, sized by `nodes_bound` >= the bits set.  cg_build_back is the rest,
// from the relabelling of the pairs on, sized by the pairs' bound.  cg_build is the two back to back; the split graph
// stage queues the front behind its publishing kernel, before the host knows the number of rest pairs, and the back
// once it does (stage_graph_compact).
static int cg_build_front(humid_ctx *c, const u32 *bits, u32 n_ids, const u32 *cnt_by_id, u64 nodes_bound) {
  hipStream_t st = c->stream;
  const u32 n_words = (((n_ids + 31) / 32) + 7) & ~7u, n_blk = n_words / 8;
  const size_t Mb = (size_t)std::min<u64>(n_ids, nodes_bound);
  ENSURE(c->cg_blk, ((size_t)n_blk + 1) * 4);
  ENSURE(c->cg_nodes, (Mb + 1) * 4);
  ENSURE(c->cg_ncnt, (Mb + 1) * 4);
  ENSURE(c->cg_deg, (Mb + 2) * 4);
  ENSURE(c->cg_parent, (Mb + 1) * 4);
  ENSURE(c->cg_csize, (Mb + 1) * 4);
  ENSURE(c->cg_curs, (Mb + 1) * 4);
  TRY(exscan_in<u32>(c, BitsBlockIn{bits, n_blk}, c->cg_blk.as<u32>(), (u64)n_blk + 1));
  const BitRank br{bits, c->cg_blk.as<u32>()};
  const GraphArrays g = cg_arrays(c);
  hipLaunchKernelGGL(k_nodes_init, dim3(blocks_for(n_words)), dim3(256), 0, st, br, n_words, cnt_by_id, c->cg_nodes.as<u32>(),
                     c->cg_ncnt.as<u32>(), g.deg, g.parent, g.csize, c->cg_curs.as<u32>(), n_blk);
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}
static int cg_build_back(humid_ctx *c, CgSource &src, u32 method, CgStatus &out) {
  hipStream_t st = c->stream;
  u32 *bits = src.bits ? src.bits : c->cg_bits.as<u32>();
  const u32 n_words = (((src.n_ids + 31) / 32) + 7) & ~7u, n_blk = n_words / 8;
  const u64 pb = std::max<u64>(src.pairs_bound, 1);
  if (2 * pb + 2 > 0xffffffffull) return fail(c, HUMID_E_OVERFLOW, "too many neighbour pairs");
  const u32 Mb = (u32)std::min<u64>(src.n_ids, 2 * pb);
  ENSURE(c->cg_off, ((size_t)Mb + 2) * 4);
  ENSURE(c->cg_idx, (size_t)(2 * pb + 1) * 4);
  ENSURE(c->cg_cl_of, ((size_t)Mb + 1) * 4);
  ENSURE(c->cg_maxleaf, ((size_t)Mb + 1) * 4);
  ENSURE(c->cg_cl_size, ((size_t)Mb + 1) * 8);
  ENSURE(c->small_roots, ((size_t)Mb / 3 + 2) * 4);
  ENSURE(c->small, 64);
  const BitRank br{bits, c->cg_blk.as<u32>()};
  const u32 *m_dev = c->cg_blk.as<u32>() + n_blk;
  const GraphArrays g = cg_arrays(c);
  const u32 r_first = src.er.e ? 0u : ER_REGIONS;        // no regions (one dense pair list): the `far` region alone
  const bool by_count = (method & 1) == 0;
  if (src.segs) {
    const u32 n_all = src.segs->first[REC_SEGS];
    u32 n_max = 1;
    for (u32 q = 0; q < REC_SEGS; q++) n_max = std::max(n_max, src.segs->n[q]);
    ENSURE(c->cg_far, ((size_t)n_all + 1) * 8);
    hipLaunchKernelGGL(k_segs_relabel, dim3(std::min<u32>(blocks_for(n_max), 4096), REC_SEGS), dim3(256), 0, st, *src.segs, src.n_ids, br,
                       c->cg_far.as<u64>(), c->cg_ncnt.as<u32>(), g.deg, g.parent, by_count);
    src.er.far = c->cg_far.as<u64>();
    src.er.n_far = n_all;
  } else if (src.recs) {
    ENSURE(c->cg_far, ((size_t)src.n_recs + 1) * 8);
    if (src.n_recs)
      hipLaunchKernelGGL(k_records_relabel, dim3(blocks_for(src.n_recs)), dim3(256), 0, st, src.recs, src.n_recs, src.n_ids, br,
                         c->cg_far.as<u64>(), c->cg_ncnt.as<u32>(), g.deg, g.parent, by_count);
    src.er.far = c->cg_far.as<u64>();
    src.er.n_far = src.n_recs;
  } else {
    const u32 gx = (u32)std::min<u64>(std::max<u64>(blocks_for(std::max<u64>(src.er.cap_r, src.er.n_far)), 1), 4096);
    hipLaunchKernelGGL(k_pairs_relabel, dim3(gx, ER_REGIONS + 1 - r_first), dim3(256), 0, st, src.er, br, (const u32 *)c->cg_ncnt.as<u32>(),
                       g.deg, g.parent, by_count, r_first);
  }
  TRY(exscan_in<u32>(c, DegIn{g.deg, m_dev}, g.off, (u64)Mb + 1));
  {
    // CSR rows and component sizes side by side (one launch: kernels_cgraph.hip.h)
    const u32 gx = (u32)std::min<u64>(std::max<u64>(blocks_for(std::max<u64>(src.er.cap_r, src.er.n_far)), 1), 4096);
    hipLaunchKernelGGL(k_fill_and_stats, dim3(gx * (ER_REGIONS + 1 - r_first) + blocks_for(Mb)), dim3(256), 0, st, src.er, (const u32 *)g.off,
                       c->cg_curs.as<u32>(), g.idx, src.no_wait ? (u32 *)nullptr : c->small.as<u32>(), gx, (const u32 *)g.deg, g.parent, Mb, g.csize, m_dev, r_first);
  }
  hipLaunchKernelGGL(k_sort_lists, dim3(blocks_for(Mb)), dim3(256), 0, st, (const u32 *)g.off, Mb, g.idx);
  TRY(mark_kernel(c, c->kev[KEV_CLUSTER_BEGIN]));
  const u32 tg = (u32)std::min<u64>(std::max<u64>(blocks_for(Mb), 1), 512);
  if (method == HUMID_METHOD_MAXIMUM)
    hipLaunchKernelGGL(k_cg_trivial<true>, dim3(tg), dim3(256), 0, st, (const u32 *)g.parent, (const u32 *)g.csize, m_dev,
                       (const u32 *)c->cg_ncnt.as<u32>(), (const u32 *)g.off, (const u32 *)g.idx, g.cl_of, g.maxleaf, g.cl_size, c->d_ctr,
                       c->small_roots.as<u32>());
  else
    hipLaunchKernelGGL(k_cg_trivial<false>, dim3(tg), dim3(256), 0, st, (const u32 *)g.parent, (const u32 *)g.csize, m_dev,
                       (const u32 *)c->cg_ncnt.as<u32>(), (const u32 *)g.off, (const u32 *)g.idx, g.cl_of, g.maxleaf, g.cl_size, c->d_ctr,
                       c->small_roots.as<u32>());
  HIPCHK(hipGetLastError());
  if (src.no_wait) return HUMID_OK;
  TRY(read_counters(c, g.off + Mb, c->small.as<u32>(), m_dev));              // 2E, pairs the fullest region wanted, M
  out.wanted = (c->h_ctr[CTR_N - 2] & 0xffffffffull) * ER_REGIONS;            // (as a total: every region has the same room)
  out.overflow = (c->h_ctr[CTR_EOVER] & 0xffffffffull) != 0;
  out.group_over = c->h_ctr[CTR_GOVER] != 0;
  out.big_mask = c->h_ctr[CTR_BIGMASK];
  out.E = (c->h_ctr[CTR_N - 1] & 0xffffffffull) / 2;
  out.M = c->h_ctr[CTR_N - 3] & 0xffffffffull;
  out.Mbig = c->h_ctr[CTR_MEMBERS];
  return HUMID_OK;
}
static int cg_build(humid_ctx *c, CgSource &src, u32 method, CgStatus &out) {
  const u64 pb = std::max<u64>(src.pairs_bound, 1);
  if (2 * pb + 2 > 0xffffffffull) return fail(c, HUMID_E_OVERFLOW, "too many neighbour pairs");
  TRY(cg_build_front(c, src.bits ? src.bits : c->cg_bits.as<u32>(), src.n_ids, src.cnt_by_id, 2 * pb));
  return cg_build_back(c, src, method, out);
}
// the components of 3 and more nodes, then the nodes that created no cluster as a bitmap over the ids with
// its rank structure (c->cg_nbits zeroed by the caller; cg_nblk)
// late_m: M is a bound, Mbig unknown (cluster_kernels); *late_m_out = the node count if the cluster kernels fetched it
static int cg_cluster_rest(humid_ctx *c, u32 n_ids, u64 M, u64 Mbig, u32 method, const u32 *late_m = nullptr, bool fetch = false,
                           u64 *late_m_out = nullptr) {
  hipStream_t st = c->stream;
  const u32 n_words = (((n_ids + 31) / 32) + 7) & ~7u, n_blk = n_words / 8;
  const GraphArrays g = cg_arrays(c);
  ENSURE(c->cg_nblk, ((size_t)n_blk + 1) * 4);
  if (M > 0) TRY(cluster_kernels(c, g, c->cg_ncnt.as<u32>(), (u32)M, M, Mbig, method, true, fetch ? late_m : (const u32 *)nullptr, late_m_out));
  else TRY(mark_kernel(c, c->kev[KEV_CLUSTER_END]));
  if (M > 0)
    hipLaunchKernelGGL(k_noncreator_bits, dim3(blocks_for(M)), dim3(256), 0, st, (const u32 *)g.cl_of, c->cg_nodes.as<u32>(), (u32)M,
                       c->cg_nbits.as<u32>(), late_m);
  TRY(exscan_in<u32>(c, BitsBlockIn{c->cg_nbits.as<u32>(), n_blk}, c->cg_nblk.as<u32>(), (u64)n_blk + 1));
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// ---- stage B on the COMPACT graph (kernels_cgraph.hip.h): the single-GPU pipeline's form ---------
// Same contract as stage_graph (neighbours + clusters of the ascending unique array g_word / g_cnt),
// but every graph and cluster array lives on the M leaves that have neighbours; the per-unique-word
// view (deg / nbr_off / nbr_idx / cl_of / ... of the context) is only built when an accessor asks for
// it (expand_compact).  Leaves: slot_out (own = the graph is over this context's unique words) or
// cid / ismax (own = false), c->cg_* and the cluster count on the device (n_clusters_compact).
// ext_edges != nullptr: the pairs are GIVEN as (smaller << 32 | larger) walk indices (edit distance).
// Option pair_split (the default): a pair whose two ends have no other pair is settled by k_pairs_split right behind
// the searches, and cg_build only sees the rest (a dense list, its ends in cg_rbits); the attempt's host wait stands
// behind k_pairs_split, the rest build has none.  The cg_* arrays then hold the rest graph: cg_ensure_full.
template <class WT>
static int stage_graph_compact(humid_ctx *c, const WT *g_word, const u32 *g_cnt, u32 U, u32 word_nt,
                               u32 distance, u32 method, humid_summary &s, u32 &n_pair_segs_out,
                               const u64 *ext_edges = nullptr, u64 n_ext_edges = 0) {
  hipStream_t st = c->stream;
  c->g_word = g_word;
  c->g_wpr = (u32)(sizeof(WT) / 8);
  c->g_cnt = g_cnt;
  c->gU = U;
  c->cg_valid = false;
  c->cg_expanded = false;
  c->cg_split = c->cg_full = c->cg_m_late = c->cg_broken = false;
  c->cg_iso = c->cg_R = 0;
  c->gr_rides = c->gr_orders = 0;
  const bool split = c->pair_split;
  const ComboPlan plan = make_plan(word_nt - c->gk_nt, distance, U, c->force_segments, true, c->gk_nt);
  const PairSearch<WT> ps = pair_search<WT>(c, plan, distance);
  const bool given = ext_edges != nullptr;
  const bool search = !given && distance > 0 && U > 1;
  if (search && plan.ncombo == 1 && plan.key_bits == 0 && U > (1u << 18))
    return fail(c, HUMID_E_OVERFLOW, "distance %u over %u-nt words compares all pairs of %u unique words: too many neighbour pairs",
                distance, word_nt, U);
  if (given && n_ext_edges > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "too many neighbour pairs");
  const u32 nseg = search ? plan.ncombo : 0;
  const u32 n_words = (((U + 31) / 32) + 7) & ~7u, n_blk = n_words / 8;
  c->cg_nblocks = n_blk;
  ENSURE(c->cg_bits, (size_t)n_words * 4);
  ENSURE(c->cg_nbits, (size_t)n_words * 4);
  ENSURE(c->cg_blk, ((size_t)n_blk + 1) * 4);
  ENSURE(c->cg_nblk, ((size_t)n_blk + 1) * 4);
  ENSURE(c->cg_cur, (size_t)(ER_REGIONS * ER_STRIDE + 8) * 4);
  ENSURE(c->small_roots, ((size_t)U / 3 + 2) * 4);
  ENSURE(c->small, 64);
  if (split) {
    ENSURE(c->cg_multi, (size_t)n_words * 4);
    ENSURE(c->cg_rbits, (size_t)n_words * 4);
    ENSURE(c->cg_pres, (size_t)U * 4 + 4);
  }
  u32 *multi = split ? c->cg_multi.as<u32>() : (u32 *)nullptr;
  u64 n_iso = 0, R = 0;
  TRY(ensure_seg_scratch<WT>(c, nseg, U));
  u32 *bad = c->cg_cur.as<u32>() + ER_REGIONS * ER_STRIDE;       // malformed given pair
  const u64 *far = given ? ext_edges : nullptr;
  u64 n_far = given ? n_ext_edges : 0;
  u64 E = 0, M = 0, Mbig = 0;
  CgStatus cgs;
  EdgeRegs er;
  // the bucket order of a combination is made ONCE: the grouping places equal keys with atomics, so a
  // second run may order a bucket differently -- and the near / far split of a large bucket (walk
  // distance) must be the same in the search that follows the tiles as in the one before them
  bool ordered_seg[MAX_COMBOS] = {false};
  const u32 *seg_valid[MAX_COMBOS] = {nullptr};
  for (int attempt = 0;; attempt++) {
    if (attempt > 5) return fail(c, HUMID_E_INVALID, "internal: the pair list does not settle");
    c->roads.graph_attempts = (u32)attempt + 1;
    if (search && c->cg_ecap == 0) c->cg_ecap = std::max<u64>((u64)U / 4, 4096);
    const u64 ecap = search ? c->cg_ecap : ER_REGIONS;
    if (ecap / ER_REGIONS + 1 > 0xfffffff0ull) return fail(c, HUMID_E_OVERFLOW, "too many neighbour pairs");
    er.cap_r = (u32)((ecap + ER_REGIONS - 1) / ER_REGIONS);
    ENSURE(c->cg_edges, (size_t)ER_REGIONS * er.cap_r * 8);
    er.e = c->cg_edges.as<u64>();
    er.cur = c->cg_cur.as<u32>();
    er.far = far;
    er.n_far = (u32)n_far;
    {
      ZeroList z;
      memset(&z, 0, sizeof z);
      z.p[0] = c->cg_bits.as<u32>(); z.n[0] = n_words;
      z.p[1] = c->cg_nbits.as<u32>(); z.n[1] = n_words;
      z.p[2] = c->cg_cur.as<u32>(); z.n[2] = ER_REGIONS * ER_STRIDE + 8;
      z.p[3] = (u32 *)&c->d_ctr[CTR_EDGES]; z.n[3] = 2 * (CTR_GOVER - CTR_EDGES + 1);
      if (split) {
        z.p[4] = multi; z.n[4] = n_words;
        z.p[5] = c->cg_rbits.as<u32>(); z.n[5] = n_words;
        z.p[6] = c->small.as<u32>(); z.n[6] = SPLIT_WORDS;
      }
      hipLaunchKernelGGL(k_zero_many, dim3(64), dim3(256), 0, st, z);
    }
    // a launch of k_pairs_append over the order of combination seg, between its two events
    auto search_alone = [&](u32 seg) -> int {
      TRY(mark_pairs(c, PAIRS_COUNT, seg, 0));
      pairs_append<WT>(c, ps, walked_seg<WT>(c, plan, seg, g_word, U), er, c->cg_bits.as<u32>(), multi, &c->d_ctr[CTR_BIGMASK],
                       (u32 *)&c->d_ctr[CTR_EOVER], seg_valid[seg]);
      TRY(mark_pairs(c, PAIRS_COUNT, seg, 1));
      return HUMID_OK;
    };
    // fused_search: while an order is MADE its search rides in the grouping (GroupRide; the events then bracket the
    // launch it rode in) -- where the grouping takes it.  An order kept from an earlier attempt, and the prefix
    // combination's (the walk order itself), are searched by k_pairs_append.
    const bool ride_on = c->fused_search && std::is_same<WT, u64>::value;
    // Only the first attempt rides.  Where every order is stored that is so by itself (a later attempt finds the orders of
    // the first, or exact bins, which no search rides in); a search on records stores none, and were it to ride again
    // behind a full region, the run would take FEWER attempts than with stored orders: a ride spreads a combination's
    // pairs over one region per coarse bin, k_pairs_append over one per 1024 positions, and at 4 858 words (5 such regions)
    // the second attempt fits the regrown regions with a ride and fills one again without.  The attempts of a run do not
    // depend on group_records: a later attempt makes the order and searches it with k_pairs_append.
    const bool ride_now = ride_on && attempt == 0;
    for (u32 seg = 0; seg < nseg; seg++) {
      bool searched = false;
      if (seg) {
        // the count of words a padded grouping holds (pt_work: the next grouping overwrites it only behind this search,
        // in stream order); an order kept from an earlier attempt is complete, or that attempt would have been discarded
        seg_valid[seg] = nullptr;
        if (!ordered_seg[seg]) {
          GroupRide ride;
          if constexpr (std::is_same<WT, u64>::value) {
            if (ride_now) {
              ride.group = pairs_append_dev(ps, w_from<u64>(plan.mask[seg]), seg, er, c->cg_bits.as<u32>(), multi, &c->d_ctr[CTR_BIGMASK], (u32 *)&c->d_ctr[CTR_EOVER]);
              if (seg < KEV_PAIR_COMBOS)                  // (kernel marks: recorded with the option only)
                for (u32 end = 0; end < 2; end++) ride.ev_group[end] = c->kev[kev_pairs(PAIRS_COUNT, seg, end)];
              ride.word_bits = word_nt <= 32 ? 2 * word_nt : 0u;
            }
          }
          TRY(bucket_order<WT>(c, plan, seg, g_word, U, seg_ws<WT>(c, seg, U), seg_vs(c, seg, U), true, ride_now ? &ride : nullptr));
          seg_valid[seg] = c->gf_valid;
          searched = ride.did_group;
          // a search that rode on records (group_records) stored NO order: a later attempt makes it (no ride then, see
          // ride_now), and so do the tiles below
          ordered_seg[seg] = !ride.no_order;
          if (ride.no_order) c->gr_rides++; else c->gr_orders++;
        }
      }
      if (!searched) TRY(search_alone(seg));
    }
    if (n_far)
      hipLaunchKernelGGL(k_mark_pairs, dim3(blocks_for(n_far)), dim3(256), 0, st, far, (u32)n_far, U, c->cg_bits.as<u32>(), bad, multi);
    if (split) {
      // the isolated pairs are settled here, the others listed; the attempt's ONE host wait follows at once (a retry has
      // built no graph)
      const u64 rest_cap = (u64)ER_REGIONS * er.cap_r + n_far;
      if (rest_cap > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "too many neighbour pairs");
      ENSURE(c->cg_rest, (size_t)(rest_cap + 1) * 8);
      const u32 gx = (u32)std::min<u64>(std::max<u64>(blocks_for(std::max<u64>(er.cap_r, er.n_far), SPLIT_PPT * 256), 1), 4096);
      u32 *sp = c->small.as<u32>();
      if (method == HUMID_METHOD_MAXIMUM)
        hipLaunchKernelGGL(k_pairs_split<true>, dim3(gx, ER_REGIONS + 1), dim3(256), 0, st, er, (const u32 *)multi, g_cnt, c->cg_pres.as<u32>(),
                           c->cg_nbits.as<u32>(), c->cg_rbits.as<u32>(), c->cg_rest.as<u64>(), (u32)rest_cap, U, sp);
      else
        hipLaunchKernelGGL(k_pairs_split<false>, dim3(gx, ER_REGIONS + 1), dim3(256), 0, st, er, (const u32 *)multi, g_cnt, c->cg_pres.as<u32>(),
                           c->cg_nbits.as<u32>(), c->cg_rbits.as<u32>(), c->cg_rest.as<u64>(), (u32)rest_cap, U, sp);
      HIPCHK(hipGetLastError());
      if (c->overlap_waits) {
        // the front of the rest build does not depend on R, only on cg_rbits: it runs while the host waits for R and
        // the retry flags and decides.  Its arrays are sized by a bound known now: k_pairs_split lists at most rest_cap
        // pairs (its own argument), so cg_rbits has at most min(U, 2 * rest_cap) bits set.  On a retry its output is
        // dead: the next attempt zeroes the bitmaps and makes it again.
        TRY(read_counters_begin(c, sp + SPLIT_REST, sp + SPLIT_RMAX, sp + SPLIT_ALL));
        TRY(cg_build_front(c, c->cg_rbits.as<u32>(), U, g_cnt, 2 * rest_cap));
        TRY(read_counters_end(c, true));
      } else
        TRY(read_counters(c, sp + SPLIT_REST, sp + SPLIT_RMAX, sp + SPLIT_ALL));
      cgs.wanted = (c->h_ctr[CTR_N - 2] & 0xffffffffull) * ER_REGIONS;
      cgs.overflow = (c->h_ctr[CTR_EOVER] & 0xffffffffull) != 0;
      cgs.group_over = c->h_ctr[CTR_GOVER] != 0;
      cgs.big_mask = c->h_ctr[CTR_BIGMASK];
      R = c->h_ctr[CTR_N - 1] & 0xffffffffull;
      n_iso = (c->h_ctr[CTR_N - 3] & 0xffffffffull) - std::min<u64>(R, c->h_ctr[CTR_N - 3] & 0xffffffffull);
    } else {
      CgSource src;
      src.er = er; src.recs = nullptr; src.n_recs = 0; src.cnt_by_id = g_cnt; src.n_ids = U;
      src.pairs_bound = ecap + n_far;
      TRY(cg_build(c, src, method, cgs));
      er = src.er;
    }
    if (cgs.group_over) {                                // a padded coarse bin of a grouping was full: words are missing
      c->gf_padded = false;                              // from a bucket order -- all of it again with exact bins
      road_taken(c, HUMID_ROAD_ORDERS_REDONE);
      for (u32 q = 0; q < MAX_COMBOS; q++) ordered_seg[q] = false;
      far = given ? ext_edges : nullptr;
      n_far = given ? n_ext_edges : 0;
      continue;
    }
    if (cgs.overflow) {                                  // a region was full: more room, once more
      c->cg_ecap = cgs.wanted + cgs.wanted / 2 + ER_REGIONS * 64;
      road_taken(c, HUMID_ROAD_REGIONS_REGROWN);
      // Without pair_split cg_build has relabelled the pairs of the tiles IN PLACE (k_pairs_relabel): that list cannot be
      // used again, the tiles make it once more behind the next search.  With pair_split no graph has been built and the
      // list is intact; it is dropped all the same, so that both paths take the same attempts.  (A search that rode in the groupings spreads its pairs
      // over one region per coarse bin, k_pairs_append over one per 1024 positions: the search behind the tiles can
      // fill a region where the one in front of them did not.)
      if (!given) { far = nullptr; n_far = 0; }
      continue;
    }
    if (given) {
      u32 h_bad = 0;
      HIPCHK(hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (h_bad) return fail(c, HUMID_E_INVALID, "malformed edge list (node index out of range)");
    }
    if (search && cgs.big_mask && !far) {
      // some bucket is longer than k_pairs_append walks: its remaining pairs (further apart than the
      // walk) come from the tiles, as one more region; then the search is taken again with them in place
      const u64 big_mask = cgs.big_mask;
      u64 got = 0;
      for (int phase = 0; phase < 2; phase++) {
        u64 at = 0;
        for (u32 seg = 0; seg < nseg; seg++) {
          if (!(big_mask >> seg & 1)) continue;
          if (seg && !ordered_seg[seg]) {
            // its search rode on records and stored no order: made now, without a ride, and searched by k_pairs_append
            // from here on.  The padded bins that held every word a moment ago hold them again: the order is complete.
            TRY(bucket_order<WT>(c, plan, seg, g_word, U, seg_ws<WT>(c, seg, U), seg_vs(c, seg, U), true));
            ordered_seg[seg] = true;
            c->gr_orders++;
          }
          const Walked<WT> w = walked_seg<WT>(c, plan, seg, g_word, U);
          std::vector<BigRun> runs;
          const BigRun *d_runs = nullptr;
          TRY(find_big_runs<WT>(c, w.W, U, w.mask, ps.walk_max, seg, runs, &d_runs));
          if (!runs.back().tile0) continue;
          const ull start = phase ? at : 0;
          HIPCHK(hipMemcpyAsync(&c->d_ctr[CTR_SPECIAL], &start, sizeof(ull), hipMemcpyHostToDevice, st));
          HIPCHK(hipStreamSynchronize(st));
          tiles_emit<WT>(c, ps, w, d_runs, runs, phase ? PM_EMIT_FILL : PM_EMIT_COUNT,
                         EmitSink{nullptr, nullptr, c->cg_far.as<u64>(), &c->d_ctr[CTR_SPECIAL]});
          HIPCHK(hipGetLastError());
          TRY(read_counters(c));
          if (phase == 0) got += c->h_ctr[CTR_SPECIAL]; else at = c->h_ctr[CTR_SPECIAL];
        }
        if (phase == 0) {
          if (got > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "%llu neighbour pairs exceed the 32-bit adjacency offsets", (ull)got);
          ENSURE(c->cg_far, (size_t)(got + 1) * 8);
        }
      }
      far = c->cg_far.as<u64>();
      n_far = got;
      if (n_far) { road_taken(c, HUMID_ROAD_FAR_TILES); continue; }   // (else nothing beyond the walk after all: the list stands)
    }
    if (split) {
      c->cg_er = er;
      c->cg_pairs_bound = ecap + n_far;
    } else { E = cgs.E; M = cgs.M; Mbig = cgs.Mbig; }
    // far too roomy for this input: the next pass gets what this one wanted + a quarter (launches are sized by it)
    if (search && 2 * (cgs.wanted + cgs.wanted / 4 + ER_REGIONS * 64) < c->cg_ecap) c->cg_ecap = cgs.wanted + cgs.wanted / 4 + ER_REGIONS * 64;
    break;
  }
  const u32 *late_m = nullptr;
  bool fetch = false;
  if (split) {
    // the compact graph over the R rest pairs (a dense list) and their ends (cg_rbits), sized by R (with overlap_waits
    // its front, sized by a bound, is in the stream already); no wait of its own
    c->cg_split = true;
    c->cg_method = method;
    c->cg_iso = n_iso; c->cg_R = R;
    E = n_iso + R;
    if (R > 0) {
      CgSource src;
      src.er.e = nullptr; src.er.cap_r = 0; src.er.cur = c->cg_cur.as<u32>(); src.er.far = c->cg_rest.as<u64>(); src.er.n_far = (u32)R;
      src.recs = nullptr; src.n_recs = 0; src.cnt_by_id = g_cnt; src.n_ids = U;
      src.pairs_bound = R;
      src.bits = c->cg_rbits.as<u32>();
      src.no_wait = true;
      if (c->overlap_waits) TRY(cg_build_back(c, src, method, cgs));   // (its front ran behind the last attempt's publishing kernel)
      else TRY(cg_build(c, src, method, cgs));
      late_m = c->cg_blk.as<u32>() + n_blk;
      // a component of more than SMALL_COMP nodes has at least SMALL_COMP pairs: with fewer, Mbig = 0 and the node
      // count can wait for the pass's last wait; else both come while k_cluster_small_lds runs
      fetch = R >= SMALL_COMP;
      c->cg_m_late = !fetch;
      M = std::min<u64>(U, 2 * R);                       // (a bound)
      Mbig = 0;
    } else TRY(mark_kernel(c, c->kev[KEV_CLUSTER_BEGIN]));   // (no rest pair, no cg_build: the cluster kernels' first event is its)
  }
  s.edges = c->E = E;
  TRY(mark_stage(c, c->ev[EV_GRAPH_BUILT]));
  u64 M_rest = 0;
  TRY(cg_cluster_rest(c, U, M, Mbig, method, late_m, fetch, &M_rest));
  if (split) M = 2 * n_iso + (fetch ? M_rest : 0);       // (cg_m_late: n_clusters_compact adds the rest graph's nodes)
  s.nonsingle = c->M = M;
  c->cg_M = split ? 0u : (u32)M;
  const GraphArrays g = cg_arrays(c);
  const bool own = ((const void *)g_word == c->s_word.p) && U == (u32)c->U;
  if (!own) { ENSURE(c->cid, (size_t)U * 4); ENSURE(c->ismax, (size_t)U); }
  hipLaunchKernelGGL(k_finalize_leaves, dim3(blocks_for(U)), dim3(256), 0, st,
                     BitRank{split ? c->cg_rbits.as<u32>() : c->cg_bits.as<u32>(), c->cg_blk.as<u32>()},
                     BitRank{c->cg_nbits.as<u32>(), c->cg_nblk.as<u32>()}, c->cg_nodes.as<u32>(), (const u32 *)g.cl_of,
                     (const u32 *)g.maxleaf, U, own ? c->s_first.as<u32>() : (const u32 *)nullptr,
                     own ? c->s_slot.as<u32>() : (const u32 *)nullptr, own ? c->slot_out.as<u64>() : (u64 *)nullptr,
                     own ? (u32 *)nullptr : c->cid.as<u32>(), own ? (u8 *)nullptr : c->ismax.as<u8>(),
                     split ? (const u32 *)c->cg_bits.as<u32>() : (const u32 *)nullptr,
                     split ? (const u32 *)c->cg_pres.as<u32>() : (const u32 *)nullptr);
  c->slots_done = own;
  c->cg_valid = true;
  HIPCHK(hipGetLastError());
  n_pair_segs_out = nseg < 8 ? nseg : 8;
  return HUMID_OK;
}

// clusters = unique words - graph nodes that created no cluster (the pass's last host wait)
static int n_clusters_compact(humid_ctx *c, u32 U, u64 *out) {
  TRY(read_counters(c, c->cg_nblk.as<u32>() + c->cg_nblocks, c->cg_m_late ? c->cg_blk.as<u32>() + c->cg_nblocks : (const u32 *)nullptr,
                    nullptr, c->timing.stamp_live ? c->d_stamp : nullptr));
  *out = (u64)U - (c->h_ctr[CTR_N - 1] & 0xffffffffull);
  if (c->cg_m_late) { c->M += c->h_ctr[CTR_N - 2] & 0xffffffffull; c->cg_m_late = false; }   // (the rest graph's nodes)
  return HUMID_OK;
}

// The per-unique-word view of a compact graph stage, for the accessors (humid_get_leaves / _adjacency /
// _clusters / _histogram): degrees, CSR rows in walk indices, cluster arrays, creator prefix sum, ids.
// The gate in front of every reader of c->cg_* outside the graph stage.  A stage that split its pairs left the REST
// graph there; the accessors want the graph over all pairs.  The regions and the far list are as the searches left them
// (k_pairs_split only reads), so the unsplit build and the cluster kernels run over them once, with cg_bits as the node
// bitmap.  Nothing the run delivered is touched: not slot_out, not cid / keep, not the summary (cg_nbits / cg_nblk, which
// the ids came from, stay as they are too).
// It runs after the pass: the pass's kernel marks (the cluster kernels' pair) are not recorded again, and d_ctr / h_ctr /
// c->small, which it overwrites, are read by nothing once a pass has returned.  The build relabels the pair list in
// place, so a failure halfway leaves nothing to build from: cg_broken, and the accessors fail from then on.
static int cg_build_full(humid_ctx *c) {
  hipStream_t st = c->stream;
  struct Quiet { PassTiming &t; ~Quiet() { t.kernels_quiet = false; } } quiet{c->timing};
  c->timing.kernels_quiet = true;
  // (nor does its wait count among the run's: humid_wait_overlap_info)
  struct RunsWaits { humid_ctx *c; u32 w, o; ~RunsWaits() { c->wo_waits = w; c->wo_overlapped = o; } } waits{c, c->wo_waits, c->wo_overlapped};
  {
    ZeroList z;
    memset(&z, 0, sizeof z);
    z.p[0] = (u32 *)&c->d_ctr[CTR_EDGES]; z.n[0] = 2 * (CTR_GOVER - CTR_EDGES + 1);
    hipLaunchKernelGGL(k_zero_many, dim3(1), dim3(256), 0, st, z);
  }
  CgSource src;
  src.er = c->cg_er; src.recs = nullptr; src.n_recs = 0; src.cnt_by_id = c->g_cnt; src.n_ids = c->gU;
  src.pairs_bound = c->cg_pairs_bound;
  CgStatus cgs;
  TRY(cg_build(c, src, c->cg_method, cgs));
  if (cgs.E != c->E) return fail(c, HUMID_E_INVALID, "internal: the full graph has %llu pairs, the run found %llu", (ull)cgs.E, (ull)c->E);
  if (cgs.M > 0) TRY(cluster_kernels(c, cg_arrays(c), c->cg_ncnt.as<u32>(), (u32)cgs.M, cgs.M, cgs.Mbig, c->cg_method, true));
  HIPCHK(hipStreamSynchronize(st));
  c->cg_M = (u32)cgs.M;
  c->cg_full = true;
  return HUMID_OK;
}
static int cg_ensure_full(humid_ctx *c) {
  if (!c->cg_valid || !c->cg_split || c->cg_full) return HUMID_OK;
  if (c->cg_broken) return fail(c, HUMID_E_STATE, "the graph of this run could not be built when it was first asked for; run again");
  const int rc = cg_build_full(c);
  if (rc != HUMID_OK) c->cg_broken = true;
  return rc;
}

static int expand_compact(humid_ctx *c) {
  if (!c->cg_valid || c->cg_expanded) return HUMID_OK;
  TRY(cg_ensure_full(c));
  hipStream_t st = c->stream;
  const u32 U = c->gU, M = c->cg_M;
  const u64 E = c->E;
  if (U == 0) { c->cg_expanded = true; return HUMID_OK; }
  ENSURE(c->deg, ((size_t)U + 1) * 4);
  ENSURE(c->nbr_off, ((size_t)U + 1) * 4);
  ENSURE(c->nbr_idx, (size_t)(2 * E + 1) * 4);
  ENSURE(c->cl_of, (size_t)U * 4);
  ENSURE(c->maxleaf, (size_t)U * 4);
  ENSURE(c->cl_size, (size_t)U * 8);
  ENSURE(c->flag, (size_t)U * 4);
  ENSURE(c->pos, ((size_t)U + 1) * 4);
  ENSURE(c->cid, (size_t)U * 4);
  ENSURE(c->ismax, (size_t)U);
  const BitRank br{c->cg_bits.as<u32>(), c->cg_blk.as<u32>()};
  hipLaunchKernelGGL(k_expand_leaves, dim3(blocks_for((u64)U + 1)), dim3(256), 0, st, br, c->cg_nodes.as<u32>(), c->cg_deg.as<u32>(),
                     c->cg_cl_of.as<u32>(), c->cg_maxleaf.as<u32>(), c->cg_cl_size.as<u64>(), c->g_cnt, U, c->deg.as<u32>(),
                     c->cl_of.as<u32>(), c->maxleaf.as<u32>(), c->cl_size.as<u64>());
  TRY(exscan_u32(c, c->deg.as<u32>(), c->nbr_off.as<u32>(), (u64)U + 1));
  if (M)
    hipLaunchKernelGGL(k_expand_rows, dim3(blocks_for(M)), dim3(256), 0, st, c->cg_nodes.as<u32>(), c->cg_off.as<u32>(),
                       c->cg_idx.as<u32>(), M, c->nbr_off.as<u32>(), c->nbr_idx.as<u32>());
  hipLaunchKernelGGL(k_creator_flags, dim3(blocks_for(U)), dim3(256), 0, st, c->cl_of.as<u32>(), U, c->flag.as<u32>());
  TRY(exscan_u32(c, c->flag.as<u32>(), c->pos.as<u32>(), U));
  hipLaunchKernelGGL(k_finalize_nodes, dim3(blocks_for(U)), dim3(256), 0, st, c->cl_of.as<u32>(), c->pos.as<u32>(),
                     c->maxleaf.as<u32>(), U, c->cid.as<u32>(), c->ismax.as<u8>(), (const u32 *)nullptr, (const u32 *)nullptr,
                     (u64 *)nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  c->cg_expanded = true;
  return HUMID_OK;
}

// sorted, duplicate-free copy of an edge list (smaller << 32 | larger) -> c->e_edges
static int unique_edges(humid_ctx *c, const u64 *d_edges, u64 raw, u32 U, u64 *n_edges_out) {
  hipStream_t st = c->stream;
  *n_edges_out = 0;
  if (raw == 0) return HUMID_OK;
  if (raw >= 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "too many edges");
  // ---- sort + unique ----
  const u32 R = (u32)raw;
  ENSURE(c->e_sorted, (size_t)R * 8);
  ENSURE(c->e_head, ((size_t)R + 1) * 4);
  ENSURE(c->e_hpos, ((size_t)R + 1) * 4);
  TRY(sort_keys<u64>(c, d_edges, c->e_sorted.as<u64>(), R, 0, 32 + bits_for(U)));
  hipLaunchKernelGGL(k_heads_u64, dim3(blocks_for((u64)R + 1)), dim3(256), 0, st, c->e_sorted.as<u64>(), R,
                     c->e_head.as<u32>());
  u64 E = 0;
  TRY(scan_total(c, c->e_head.as<u32>(), c->e_hpos.as<u32>(), R, &E));
  ENSURE(c->e_edges, (size_t)(E + 1) * 8);
  hipLaunchKernelGGL(k_compact_heads_u64, dim3(blocks_for(R)), dim3(256), 0, st, c->e_sorted.as<u64>(),
                     c->e_head.as<u32>(), c->e_hpos.as<u32>(), R, c->e_edges.as<u64>());
  HIPCHK(hipGetLastError());
  *n_edges_out = E;
  return HUMID_OK;
}

// ---- one candidate join: the driver of the edit (-e) and the strand-symmetric (-P) search -------------------------
// The two sides of a join, both sorted by key: entry t of X meets the run of entries of Y that hold its key.
template <class KT>
struct JoinKeys {
  using key_type = KT;
  const KT *kx; const u32 *vx;     // X: keys ascending, the word each came from
  const KT *ky; const u32 *vy;     // Y: the same (X itself where a search joins its keys with themselves)
  u32 U;                           // entries on either side
};
// The pairs of one join, appended to c->e_raw at raw; raw advances.  The protocol:
//   clear the sentinel pc[U] and CTR_BIGMASK; COUNT, one lane per X entry; scan, and wait for the number of pairs;
//   if the COUNT raised CTR_BIGMASK -- some run of equal keys in Y is longer than the c->walk_max candidates that one
//   lane verifies --: every run in pieces of that many (k_edit_chunks), scan, wait for the number of pieces; COUNT,
//   one lane per piece; scan, wait;
//   nothing found: done.  Else room in e_raw (what it holds is kept) and FILL, over the entries or over the pieces.
// Host waits: one per join, three where the runs are cut into pieces.
// launch(fill, keys, n_pieces, pc, poff, out) holds the kernel launches of a search: fill is std::bool_constant<FILL>,
// keys a JoinKeys<u32 | u64>; n_pieces == 0: the join over keys.U entries, else over the n_pieces pieces of e_runlo /
// e_choff.  search: the search's name in the two overflow messages.
template <class Launch>
static int join_append(humid_ctx *c, const char *search, const void *kx, const u32 *vx, const void *ky, const u32 *vy, u32 U,
                       bool k32, Launch launch, u64 &raw) {
  auto run = [&](auto key) -> int {
    using KT = decltype(key);
    hipStream_t st = c->stream;
    const JoinKeys<KT> k{(const KT *)kx, vx, (const KT *)ky, vy, U};
    const std::false_type count{};
    const std::true_type fill{};
    HIPCHK(hipMemsetAsync(c->pc.as<u32>() + U, 0, 4, st));
    HIPCHK(hipMemsetAsync(&c->d_ctr[CTR_BIGMASK], 0, sizeof(ull), st));
    launch(count, k, (u64)0, c->pc.as<u32>(), (const u32 *)nullptr, (u64 *)nullptr);
    u64 found = 0, n_pieces = 0;                   // n_pieces > 0: this join goes through the pieces
    TRY(scan_total(c, c->pc.as<u32>(), c->poff.as<u32>(), U, &found));
    if (c->h_ctr[CTR_BIGMASK]) {
      ENSURE(c->e_runlo, ((size_t)U + 1) * 4);
      ENSURE(c->e_nch, ((size_t)U + 1) * 4);
      ENSURE(c->e_choff, ((size_t)U + 1) * 4);
      hipLaunchKernelGGL(k_edit_chunks<KT>, dim3(blocks_for((u64)U + 1)), dim3(256), 0, st, k.kx, k.ky, U, c->walk_max,
                         c->e_runlo.as<u32>(), c->e_nch.as<u32>());
      TRY(scan_total(c, c->e_nch.as<u32>(), c->e_choff.as<u32>(), U, &n_pieces));
      if (n_pieces >= 0xfffffff0ull) return fail(c, HUMID_E_OVERFLOW, "too many candidate pieces in the %s search", search);
      if (n_pieces) road_taken(c, HUMID_ROAD_JOIN_PIECES);
      ENSURE(c->e_pc2, ((size_t)n_pieces + 1) * 4);
      ENSURE(c->e_poff2, ((size_t)n_pieces + 1) * 4);
      HIPCHK(hipMemsetAsync(c->e_pc2.as<u32>() + n_pieces, 0, 4, st));
      launch(count, k, n_pieces, c->e_pc2.as<u32>(), (const u32 *)nullptr, (u64 *)nullptr);
      TRY(scan_total(c, c->e_pc2.as<u32>(), c->e_poff2.as<u32>(), n_pieces, &found));
    }
    if (found == 0) return HUMID_OK;
    if (raw + found >= 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "too many candidate pairs in the %s search", search);
    HIPCHK(c->e_raw.grow_keeping((size_t)raw * 8, (size_t)(raw + found) * 8, st));
    launch(fill, k, n_pieces, (u32 *)nullptr, (const u32 *)(n_pieces ? c->e_poff2 : c->poff).as<u32>(), c->e_raw.as<u64>() + raw);
    raw += found;
    return HUMID_OK;
  };
  return k32 ? run(u32{}) : run(u64{});
}

// edit_edges below: the offset vectors o[0 .. k) in [-D, D] of a combination of k members, walk cost <= 2 D, first
// non-zero entry positive.  group_field: member 0 is the group field of a grouped run, which stays in place.
static std::vector<std::vector<int>> edit_offset_patterns(u32 k, int D, bool group_field) {
  std::vector<std::vector<int>> patterns;
  std::vector<int> o(k, 0);
  std::function<void(u32, int, bool)> rec = [&](u32 t, int cost, bool signed_yet) {
    if (t == k) {
      const int total = cost + (k ? (o[k - 1] < 0 ? -o[k - 1] : o[k - 1]) : 0);
      if (total <= 2 * D) patterns.push_back(o);
      return;
    }
    for (int v = -D; v <= D; v++) {
      if (!signed_yet && v < 0) continue;                 // canonical sign
      if (group_field && t == 0 && v != 0) continue;
      const int prev = t ? o[t - 1] : 0;
      const int step = v > prev ? v - prev : prev - v;
      if (cost + step > 2 * D) continue;
      o[t] = v;
      rec(t + 1, cost + step, signed_yet || v != 0);
    }
  };
  rec(0, 0, false);
  return patterns;
}

// ---- edit distance (-e): neighbour pairs under Levenshtein distance 2 .. 5 --------------------------
// (distance <= 1 is the Hamming search: equal lengths leave no room for a lone insertion.)
// Pigeonhole with shifts.  The plan of the Hamming search cuts the word into s segments and looks at
// every combination of k = s - d of them: d edits damage at most d segments, so some combination is
// untouched.  Untouched does not mean unmoved: between a deletion and an insertion the text is
// shifted by one position.  With at most one such pair (d <= 3) the untouched segments of a
// combination are, in order, unshifted / shifted by one / unshifted again; taking as "X" the word
// whose text reappears one position LATER in the other (the other has the insertion first), the
// shift is +1.  So for every combination and every pattern (a, b) --
// members [a, b) of the combination shifted, a == b: none -- the words' own segments (X) are joined
// with the segments read at the shifted positions (Y); candidates are verified by the dynamic
// programme (lev_band1).  Every unordered pair is found from one of its two sides;
// duplicates go away in a final sort + unique.
// d = 4, 5 allow TWO insertion/deletion pairs: every untouched member t of a combination then sits at
// an offset o_t in {-2 .. +2} of its own, and the offsets form a walk that starts and ends at 0 (equal
// lengths) with one unit step per insertion or deletion: |o_0| + sum |o_t - o_{t-1}| + |o_last| <= 4.
// All such offset vectors are joined (up to a global sign: the mirrored vector finds the same pairs
// from their other side); d <= 3 is the special case 0..0 1..1 0..0.  Verification: lev_band2.  Result: c->e_edges (ascending), *n_edges_out.
// part_rank / part_world: this caller's share of the joins (multi-GPU: every rank holds the whole
// unique array and runs every part_world-th join; the shares are gathered and made unique by
// humid_stage_unique_edges).  make_unique = false leaves the raw list in c->e_raw.
template <class WT>
static int edit_edges(humid_ctx *c, const WT *g_word, u32 U, u32 word_nt, u32 distance, u64 *n_edges_out,
                      u32 part_rank = 0, u32 part_world = 1, bool make_unique = true) {
  hipStream_t st = c->stream;
  *n_edges_out = 0;
  if (U < 2) return HUMID_OK;
  // grouped runs: field 0 of every combination is the group field, joined at offset 0 only (a common prefix does
  // not change the Levenshtein distance, so verifying the whole internal word stays exact); word fields never
  // shift into it
  const u32 gnt = c->gk_nt, wn = word_nt - gnt;
  const ComboPlan plan = make_plan(wn, distance, U, c->force_segments, false, gnt);
  const u32 kb = plan.key_bits ? plan.key_bits : 1;
  ENSURE(c->e_kx, (size_t)U * 8);
  ENSURE(c->e_vx, (size_t)U * 4);
  ENSURE(c->e_ky, (size_t)U * 8);
  ENSURE(c->e_vy, (size_t)U * 4);
  ENSURE(c->seg_k0, (size_t)U * 8);
  ENSURE(c->seg_v0, (size_t)U * 4);
  ENSURE(c->pc, ((size_t)U + 1) * 4);
  ENSURE(c->poff, ((size_t)U + 1) * 4);
  const int D = (int)(distance / 2);             // the offsets' range; the band of the verification
  auto launch = [&](auto fill, auto k, u64 n_pieces, u32 *pc, const u32 *poff, u64 *out) {
    auto banded = [&](auto band) {
      constexpr bool FILL = decltype(fill)::value;
      constexpr u32 BAND = decltype(band)::value;
      using KT = typename decltype(k)::key_type;
      if (n_pieces)
        hipLaunchKernelGGL((k_edit_join_chunks<FILL, KT, WT, BAND>), dim3(blocks_for(n_pieces)), dim3(256), 0, st, k.kx, k.vx, k.ky,
                           k.vy, k.U, (const u32 *)c->e_runlo.as<u32>(), (const u32 *)c->e_choff.as<u32>(), (u32)n_pieces,
                           c->walk_max, g_word, word_nt, distance, pc, poff, out);
      else
        hipLaunchKernelGGL((k_edit_join<FILL, KT, WT, BAND>), dim3(blocks_for(k.U)), dim3(256), 0, st, k.kx, k.vx, k.ky, k.vy, k.U,
                           g_word, word_nt, distance, pc, poff, out, c->walk_max, &c->d_ctr[CTR_BIGMASK]);
    };
    if (D <= 1) banded(std::integral_constant<u32, 1>{});
    else if (D == 2) banded(std::integral_constant<u32, 2>{});
    else banded(std::integral_constant<u32, 0>{});
  };
  u64 raw = 0;                                   // pairs collected so far (with duplicates)
  u32 join_no = 0;
  for (u32 cb = 0; cb < plan.ncombo; cb++) {
    const ComboFields cfx = plan_fields(plan, cb);
    TRY(combo_keys_sorted<WT>(c, g_word, U, cfx, kb, c->e_kx.p, c->e_vx.as<u32>()));
    for (const std::vector<int> &o : edit_offset_patterns(cfx.nf, D, gnt != 0)) {
      ComboFields cfy = cfx;
      bool valid = true, shifted = false;
      for (u32 t = 0; t < cfx.nf; t++) {
        // offset +1 = one nucleotide towards the end of the word = a field shift lower by 2 bits
        const int sh = (int)cfy.shift[t] - 2 * o[t];
        if (sh < 0 || sh + (int)cfy.width[t] > (int)(2 * ((gnt && t == 0) ? word_nt : wn))) { valid = false; break; }   // off the word
        cfy.shift[t] = (u8)sh;
        shifted = shifted || o[t] != 0;
      }
      if (!valid) continue;
      if (join_no++ % part_world != part_rank) continue;     // another rank's join
      // shifted: Y = the keys read at the shifted positions; else the X keys against themselves
      if (shifted) TRY(combo_keys_sorted<WT>(c, g_word, U, cfy, kb, c->e_ky.p, c->e_vy.as<u32>()));
      const DBuf &ky = shifted ? c->e_ky : c->e_kx, &vy = shifted ? c->e_vy : c->e_vx;
      TRY(join_append(c, "edit-distance", c->e_kx.p, c->e_vx.as<u32>(), ky.p, vy.as<u32>(), U, kb <= 32, launch, raw));
    }
  }
  HIPCHK(hipGetLastError());
  if (raw == 0) return HUMID_OK;
  if (!make_unique) { *n_edges_out = raw; return HUMID_OK; }
  TRY(unique_edges(c, c->e_raw.as<u64>(), raw, U, n_edges_out));
  return HUMID_OK;
}

// ---- strand-symmetric neighbours (humid_dedup_run_paired*, kernels_paired.hip.h) ----------------------------------
// Pairs of leaves u < v with min(ham(u, v), ham(u, m(v))) <= distance, as a duplicate-free ascending edge list in
// c->e_edges.  g_word: the U canonical leaves, ascending.  For every combination of the pigeonhole plan two joins
// over the leaves' keys X: against themselves (plain pairs) and against the keys of the mirrored leaves (mirror
// pairs, verified against m(v)).  The host waits are those of join_append.
template <class WT>
static int paired_edges(humid_ctx *c, const WT *g_word, u32 U, u32 word_nt, u32 distance, u64 *n_edges_out) {
  hipStream_t st = c->stream;
  *n_edges_out = 0;
  if (U < 2 || distance == 0) return HUMID_OK;
  const ComboPlan plan = make_plan(word_nt, distance, U, c->force_segments);
  if (plan.ncombo == 1 && plan.key_bits == 0 && U > (1u << 18))
    return fail(c, HUMID_E_OVERFLOW, "distance %u over %u-nt words compares all pairs of %u unique words: too many neighbour pairs",
                distance, word_nt, U);
  const u32 kb = plan.key_bits ? plan.key_bits : 1;
  ENSURE(c->pd_mir, (size_t)U * sizeof(WT) + 16);
  ENSURE(c->e_kx, (size_t)U * 8);
  ENSURE(c->e_vx, (size_t)U * 4);
  ENSURE(c->e_ky, (size_t)U * 8);
  ENSURE(c->e_vy, (size_t)U * 4);
  ENSURE(c->seg_k0, (size_t)U * 8);
  ENSURE(c->seg_v0, (size_t)U * 4);
  ENSURE(c->pc, ((size_t)U + 1) * 4);
  ENSURE(c->poff, ((size_t)U + 1) * 4);
  const WT *mir = c->pd_mir.as<WT>();
  hipLaunchKernelGGL(k_pd_mirror<WT>, dim3(blocks_for(U)), dim3(256), 0, st, g_word, U, word_nt, c->pd_mir.as<WT>());
  u64 raw = 0;                                   // pairs collected so far (with duplicates)
  for (u32 cb = 0; cb < plan.ncombo; cb++) {
    const ComboFields cf = plan_fields(plan, cb);
    TRY(combo_keys_sorted<WT>(c, g_word, U, cf, kb, c->e_kx.p, c->e_vx.as<u32>()));
    TRY(combo_keys_sorted<WT>(c, mir, U, cf, kb, c->e_ky.p, c->e_vy.as<u32>()));
    for (u32 side = 0; side < 2; side++) {       // 0: the leaves themselves, 1: their mirrors
      const WT *yw = side ? mir : g_word;
      auto launch = [&](auto fill, auto k, u64 n_pieces, u32 *pc, const u32 *poff, u64 *out) {
        constexpr bool FILL = decltype(fill)::value;
        using KT = typename decltype(k)::key_type;
        if (n_pieces)
          hipLaunchKernelGGL((k_pd_join_chunks<FILL, KT, WT>), dim3(blocks_for(n_pieces)), dim3(256), 0, st, k.kx, k.vx, k.ky, k.vy,
                             k.U, (const u32 *)c->e_runlo.as<u32>(), (const u32 *)c->e_choff.as<u32>(), (u32)n_pieces, c->walk_max,
                             g_word, yw, distance, pc, poff, out);
        else
          hipLaunchKernelGGL((k_pd_join<FILL, KT, WT>), dim3(blocks_for(k.U)), dim3(256), 0, st, k.kx, k.vx, k.ky, k.vy, k.U, g_word,
                             yw, distance, pc, poff, out, c->walk_max, &c->d_ctr[CTR_BIGMASK]);
      };
      const DBuf &ky = side ? c->e_ky : c->e_kx, &vy = side ? c->e_vy : c->e_vx;
      TRY(join_append(c, "strand-symmetric", c->e_kx.p, c->e_vx.as<u32>(), ky.p, vy.as<u32>(), U, kb <= 32, launch, raw));
    }
  }
  HIPCHK(hipGetLastError());
  if (raw == 0) return HUMID_OK;
  TRY(unique_edges(c, c->e_raw.as<u64>(), raw, U, n_edges_out));
  return HUMID_OK;
}

// The un-permute in two coalesced passes (kernels_part.hip.h): position i of the partition order
// (pk_vals = read, pslot = padded slot of its word) -> cluster_id / keep in read order, or, packed,
// cluster id | keep << 31 per read.  *done = false: the read set is too large for the bin table
// (more than 2048 windows of 32 K reads) or the option is off; the caller takes the one-kernel form.
// The stage mark ev_mid is recorded between the two kernels.
static int unpermute_tiled(humid_ctx *c, u32 N, bool packed, u32 *d_cid, u8 *d_keep, KernelEvent ev_mid, bool *done) {
  hipStream_t st = c->stream;
  *done = false;
  if (!c->use_tile_partition || N == 0) return HUMID_OK;
  static const u32 uw_pref = getenv("HUMID_UW_SHIFT") ? (u32)atoi(getenv("HUMID_UW_SHIFT")) : 14u;   // (experiments)
  u32 wshift = uw_pref == 15 ? 15u : 14u;
  if (((u64)N + (1u << wshift) - 1) >> wshift > UW_MAXBINS) wshift = UW_MAXSHIFT;
  const u32 n_bins = (u32)(((u64)N + (1u << wshift) - 1) >> wshift);
  if (n_bins > UW_MAXBINS) return HUMID_OK;
  ENSURE(c->unperm_rec, ((size_t)n_bins << wshift) * 8 + (size_t)UW_MAXBINS * 4);
  u64 *rec = c->unperm_rec.as<u64>();
  u32 *ucur = (u32 *)(rec + ((size_t)n_bins << wshift));
  // the bins' cursors: k_unperm_window leaves every cursor it read at zero, so only a new place needs a clear
  if (c->ucur_clean != ucur) HIPCHK(hipMemsetAsync(ucur, 0, (size_t)UW_MAXBINS * 4, st));
  c->ucur_clean = nullptr;
  // positions in use: all N for the sorted (wide-word) count, else up to pbeg[n_parts] (on the device)
  const CountLeft &cl = c->count_left;
  const u32 *n_pos_dev = count_bucketed(c) ? c->pbeg.as<u32>() + cl.n_parts : (const u32 *)nullptr;
  if (count_on_records(c)) {
    // buckets per workgroup: about 7/8 of a tile's worth of records (reads per bucket: usable / buckets)
    const u64 mean = std::max<u64>(1, c->usable / cl.n_parts);
    const u32 chunk = (n_bins > 1024 && n_bins <= 1536) ? 7u * PT_THREADS : PT_TILE;     // records the variant below stages at a time
    const u32 B = (u32)std::min<u64>(64, std::max<u64>(1, (chunk - chunk / 8) / mean));
    const u32 grid = (cl.n_parts + B - 1) / B;
    if (n_bins <= 1024)
      hipLaunchKernelGGL(k_unperm_bins8<1024>, dim3(grid), dim3(1024), 0, st, (const u64 *)c->p8_b.as<u64>(), cl.cursor2,
                         (const u64 *)c->slot_out.as<u64>(), cl.n_parts, B, N, wshift, n_bins, ucur, rec);
    else if (n_bins <= 1536)
      hipLaunchKernelGGL((k_unperm_bins8<1536, 7>), dim3(grid), dim3(1024), 0, st, (const u64 *)c->p8_b.as<u64>(), cl.cursor2,
                         (const u64 *)c->slot_out.as<u64>(), cl.n_parts, B, N, wshift, n_bins, ucur, rec);
    else
      hipLaunchKernelGGL(k_unperm_bins8<2048>, dim3(grid), dim3(1024), 0, st, (const u64 *)c->p8_b.as<u64>(), cl.cursor2,
                         (const u64 *)c->slot_out.as<u64>(), cl.n_parts, B, N, wshift, n_bins, ucur, rec);
  }
  else
  hipLaunchKernelGGL(k_unperm_bins, dim3((N + PT_TILE - 1) / PT_TILE), dim3(1024), 0, st, c->pk_vals.as<u32>(),
                     c->pslot.as<u32>(), c->slot_out.as<u64>(), n_pos_dev, N, N, wshift, n_bins, ucur, rec);
  TRY(mark_stage(c, c->kev[ev_mid]));
  if (packed) {
    if (wshift == 14) hipLaunchKernelGGL((k_unperm_window<true, 14>), dim3(n_bins), dim3(UW_THREADS), 0, st, rec, ucur, N, d_cid, d_keep);
    else hipLaunchKernelGGL((k_unperm_window<true, 15>), dim3(n_bins), dim3(UW_THREADS), 0, st, rec, ucur, N, d_cid, d_keep);
  } else {
    if (wshift == 14) hipLaunchKernelGGL((k_unperm_window<false, 14>), dim3(n_bins), dim3(UW_THREADS), 0, st, rec, ucur, N, d_cid, d_keep);
    else hipLaunchKernelGGL((k_unperm_window<false, 15>), dim3(n_bins), dim3(UW_THREADS), 0, st, rec, ucur, N, d_cid, d_keep);
  }
  TRY(mark_kernel(c, c->kev[KEV_UNPERM_END]));
  HIPCHK(hipGetLastError());
  c->ucur_clean = ucur;
  *done = true;
  return HUMID_OK;
}

// ---- stage C: per-read outputs -------------------------------------------------------------
// l_cid/l_ismax: cluster id and maxLeaf flag of THIS context's unique words in local walk order
// (on one GPU the arrays stage B left behind; on several, this rank's slice of them).
static int stage_map(humid_ctx *c, const u32 *l_cid, const u8 *l_ismax, u32 N, u32 *d_cid, u8 *d_keep) {
  hipStream_t st = c->stream;
  const u32 U = (u32)c->U;
  const bool fused = c->slots_done && l_cid == c->cid.as<u32>() && l_ismax == c->ismax.as<u8>();
  c->slots_done = false;
  if (U > 0 && !fused)
    hipLaunchKernelGGL(k_slot_results, dim3(blocks_for(U)), dim3(256), 0, st, l_cid, l_ismax,
                       c->s_first.as<u32>(), c->s_slot.as<u32>(), U, c->slot_out.as<u64>());
  TRY(mark_stage(c, c->ev[EV_CLUSTERS_DONE]));
  if (count_in_partition_order(c)) {
    bool tiled = false;
    // KEV_MAP_MID is a STAGE mark in the tiled form (unpermute_tiled: recorded unless the pass is lean) and a KERNEL mark
    // in the one-kernel form below (recorded with kernel_timing).  They differ with HUMID_ALL_EVENTS set and
    // kernel_timing off: the tiled form records it then, the one-kernel form does not; nobody reads it there.
    TRY(unpermute_tiled(c, N, false, d_cid, d_keep, KEV_MAP_MID, &tiled));
    c->timing.unperm_tiled = tiled;
    if (!tiled) {
      // round-1 form: one scattered 4-byte store per read, then a coalesced split.  pk_keys (the
      // partitioned keys) is dead by now: reuse it for the packed per-read results; reads that were
      // excluded from the partition are not in it, so the array starts as zeros
      u32 *packed = c->pk_keys.as<u32>();
      HIPCHK(hipMemsetAsync(packed, 0, (size_t)N * 4, st));
      if (count_bucketed(c))
        hipLaunchKernelGGL(k_read_map_bucket, dim3(c->count_left.n_parts), dim3(256), 0, st, c->pk_vals.as<u32>(),
                           c->pslot.as<u32>(), c->slot_out.as<u64>(), c->pbeg.as<u32>(), c->ucount.as<u32>(), N, packed);
      else
        hipLaunchKernelGGL(k_read_map_part, dim3(grid_stride_blocks(N)), dim3(256), 0, st, c->pk_vals.as<u32>(),
                           c->pslot.as<u32>(), c->slot_out.as<u64>(), N, packed);
      TRY(mark_kernel(c, c->kev[KEV_MAP_MID]));
      hipLaunchKernelGGL(k_split_out, dim3(grid_stride_blocks(N)), dim3(256), 0, st, packed, N, d_cid, d_keep);
    }
  } else
    hipLaunchKernelGGL(k_read_map, dim3(grid_stride_blocks(N)), dim3(256), 0, st, c->slot_of_read.as<u32>(),
                       c->slot_out.as<u64>(), N, d_cid, d_keep);
  TRY(mark_frame(c, c->ev[EV_PASS_END]));
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// grouped runs: did k_gkey_words see a usable read with group >= n_groups?  Read after a host wait that followed it.
static int gkey_check(humid_ctx *c) {
  if (c->pass_kind == RUN_PLAIN) return HUMID_OK;
  const u32 seen = *(volatile u32 *)&c->h_ctr[CTR_N + 1];
  if (seen == c->gk_epoch && c->pass_kind >= RUN_KEYED) return fail(c, HUMID_E_INVALID, "internal: a usable read's key was not ranked");
  if (seen == c->gk_epoch) return fail(c, HUMID_E_INVALID, "a usable read has a group >= n_groups");
  return HUMID_OK;
}

// Where a kernel that checks the reads of a pass (k_gkey_words, k_kr_words, k_acck_pack) stores c->gk_epoch: the
// host-mapped counter mirror the next host wait reads, or, without one, a device word that gkey_bad_fetch copies there
// behind the kernel.
static int gkey_bad_word(humid_ctx *c, u32 **bad) {
  if (c->h_ctr_dev && !c->no_poll) { *bad = (u32 *)&c->h_ctr_dev[CTR_N + 1]; return HUMID_OK; }
  if (!c->gk_bad.p) {
    ENSURE(c->gk_bad, 16);
    HIPCHK(hipMemsetAsync(c->gk_bad.p, 0, 16, c->stream));
  }
  *bad = c->gk_bad.as<u32>();
  return HUMID_OK;
}
static int gkey_bad_fetch(humid_ctx *c, const u32 *bad) {
  if (bad == c->gk_bad.as<u32>()) HIPCHK(hipMemcpyAsync(&c->h_ctr[CTR_N + 1], bad, 4, hipMemcpyDeviceToHost, c->stream));
  return HUMID_OK;
}

static int check_run_args(humid_ctx *c, u64 n_reads, u32 word_nt, u32 method, u32 max_nt = 32) {
  if (word_nt == 0) return fail(c, HUMID_E_INVALID, "word_nt must be >= 1");
  if (word_nt > max_nt) return fail(c, HUMID_E_UNSUPPORTED, "word_nt %u > %u is not supported by this entry point", word_nt, max_nt);
  if (method > 1) return fail(c, HUMID_E_INVALID, "method must be 0 (directional) or 1 (maximum)");
  if (n_reads > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "n_reads %llu exceeds 2^31-1", (ull)n_reads);
  return HUMID_OK;
}

// word_nt > 32 as the word type: f is called with a null pointer to u64 (one uint64 per word) or W2 (two)
template <class F>
static int with_word_type(u32 word_nt, F f) { return word_nt > 32 ? f((const W2 *)nullptr) : f((const u64 *)nullptr); }

// The pair list of a graph stage whose pairs are GIVEN: a null list means "search", so no pair is an empty list
static inline const u64 *edges_or_empty(const u64 *edges, u64 n_edges) {
  static const u64 no_edges = 0;
  return n_edges ? edges : &no_edges;
}
// The graph stage of a run: the compact one or the per-unique-word one (option compact_graph).  given: the n_edges
// pairs of `edges` are the neighbour pairs (duplicate-free, ascending); else the stage searches them.
template <class WT>
static int graph_stage(humid_ctx *c, const WT *g_word, const u32 *g_cnt, u32 U, u32 word_nt, u32 distance, u32 method, humid_summary &s,
                       u32 &n_pair_segs, bool given = false, const u64 *edges = nullptr, u64 n_edges = 0) {
  const u64 *ext = given ? edges_or_empty(edges, n_edges) : nullptr;
  if (!given) n_edges = 0;
  return c->use_compact ? stage_graph_compact<WT>(c, g_word, g_cnt, U, word_nt, distance, method, s, n_pair_segs, ext, n_edges)
                        : stage_graph<WT>(c, g_word, g_cnt, U, word_nt, distance, method, s, n_pair_segs, ext, n_edges);
}

// ---- the full pipeline on device buffers (one GPU) -------------------------------------------
// WT = u64: word_nt <= 32, one uint64 per read.  WT = W2: 33 <= word_nt <= 64, two per read.
template <class WT>
static int run_device(humid_ctx *c, const WT *d_words, const u8 *d_filt, u64 n_reads, u32 word_nt,
                      u32 distance, u32 method, u32 *d_cid, u8 *d_keep, humid_summary *sum) {
  if (!c) return HUMID_E_INVALID;
  constexpr bool WIDE = sizeof(WT) == 16;
  state_reset(c);
  TRY(check_run_args(c, n_reads, word_nt, method, 64));
  if (WIDE != (word_nt > 32)) return fail(c, HUMID_E_INVALID, "word layout does not match word_nt");
  if (WIDE && ((uintptr_t)d_words & 15)) return fail(c, HUMID_E_INVALID, "wide words must be 16-byte aligned on the device");
  if (n_reads && (!d_words || !d_filt || !d_cid || !d_keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const u32 N = (u32)n_reads;
  humid_summary s;
  memset(&s, 0, sizeof s);
  s.total = n_reads;
  pass_begin(c, n_reads, word_nt, distance, method);
  if (N == 0) { if (sum) *sum = s; return state_publish(c, CtxState::RUN); }
  // a plain run of one-word words whose counters reach the host through the mapped mirror may take its four times from
  // device stamps
  PassTimingGuard timing(c, !WIDE && c->device_stamps && c->d_stamp && c->pass_kind == RUN_PLAIN && !c->pd_run && !(c->edit && distance >= 2) &&
                            c->h_ctr_dev && !c->no_poll);
  if constexpr (WIDE) TRY(stage_count_wide(c, d_words, d_filt, N, word_nt, s));
  else TRY(stage_count(c, d_words, d_filt, N, word_nt, 0ull, ~0ull, 0, s));
  TRY(gkey_check(c));                                        // (the count stage's host wait has seen k_gkey_words)
  const u32 U = (u32)c->U;
  if (U == 0) {   // everything filtered
    HIPCHK(hipMemsetAsync(d_cid, 0, (size_t)N * 4, st));
    HIPCHK(hipMemsetAsync(d_keep, 0, (size_t)N, st));
    HIPCHK(hipStreamSynchronize(st));
    if (sum) *sum = s;
    return state_publish(c, CtxState::RUN);
  }
  u32 n_pair_segs = 0;
  u64 n_given = 0;
  const bool paired = c->pd_run && distance >= 1, edit = !paired && c->edit && distance >= 2;
  // strand-symmetric run: the pairs of the plain and of the mirror join (paired_edges), given to the graph stage
  if (paired) TRY(paired_edges<WT>(c, c->s_word.as<WT>(), U, word_nt, distance, &n_given));
  // -e: Levenshtein neighbours (src/humid.cc:140-158); distance <= 1 IS the Hamming search
  if (edit) TRY(edit_edges<WT>(c, c->s_word.as<WT>(), U, word_nt, distance, &n_given));
  TRY(graph_stage<WT>(c, c->s_word.as<WT>(), c->s_cnt.as<u32>(), U, word_nt, distance, method, s, n_pair_segs, paired || edit,
                      c->e_edges.as<u64>(), n_given));
  TRY(stage_map(c, c->cid.as<u32>(), c->ismax.as<u8>(), N, d_cid, d_keep));
  if (c->cg_valid) TRY(n_clusters_compact(c, U, &c->C));
  else TRY(n_clusters_from_scan(c, U, &c->C));
  s.clusters = c->C;
  s.nonsingle = c->M;
  s.count_mode_used = count_mode_used(c);
  TRY(timing_tail(c, s, n_pair_segs));
  if (sum) *sum = s;
  return state_publish(c, CtxState::RUN);
}

// ---- long words (humid_dedup_run_long*, kernels_long.hip.h): k = ceil(word_nt / 32) uint64 per read; their count: stage_count_long ----
// Pairs of leaves u < v within Hamming distance `distance` over all word_nt nucleotides, as a duplicate-free ascending
// edge list in c->e_edges.  leaf: the U leaves ascending, k uint64 each.  Pigeonhole over distance + 1 contiguous
// segments (lengths differ by at most one): two words within the distance agree on some segment, so per segment the
// leaves are joined with themselves on a key of the segment (k_long_seg_keys) and every candidate is verified over
// the whole word -- a key collision only adds candidates.  distance >= word_nt, or more segments than MAX_COMBOS:
// one join of all pairs.  The host waits are those of join_append; c->lg_info says what was done.
static int long_edges(humid_ctx *c, const u64 *leaf, u32 U, u32 k, u32 word_nt, u32 distance, u64 *n_edges_out) {
  hipStream_t st = c->stream;
  *n_edges_out = 0;
  if (U < 2) return HUMID_OK;
  // distance 0: the plan's one segment is the whole word, and distinct leaves share none: its join is empty, not launched
  if (distance == 0) { c->lg_info.joins = 1; return HUMID_OK; }
  const bool all_pairs = distance >= word_nt || distance + 1 > MAX_COMBOS;
  if (all_pairs && U > (1u << 18))
    return fail(c, HUMID_E_OVERFLOW, "distance %u over %u-nt words compares all pairs of %u unique words: too many neighbour pairs",
                distance, word_nt, U);
  const u32 nseg = all_pairs ? 1u : distance + 1;
  ENSURE(c->e_kx, (size_t)U * 8);
  ENSURE(c->e_vx, (size_t)U * 4);
  ENSURE(c->seg_k0, (size_t)U * 8);
  ENSURE(c->seg_v0, (size_t)U * 4);
  ENSURE(c->pc, ((size_t)U + 1) * 4);
  ENSURE(c->poff, ((size_t)U + 1) * 4);
  ENSURE(c->lg_cand, (size_t)MAX_COMBOS * LONG_CAND_SLOTS * sizeof(ull));
  HIPCHK(hipMemsetAsync(c->lg_cand.p, 0, (size_t)MAX_COMBOS * LONG_CAND_SLOTS * sizeof(ull), st));
  const u32 pad = 64 * k - 2 * word_nt;            // bits in front of the word in its string of 64 k bits
  const u32 base = word_nt / nseg, rem = word_nt % nseg;
  u64 raw = 0;                                     // pairs collected so far (with duplicates)
  u32 pos = 0;
  for (u32 seg = 0; seg < nseg; seg++) {
    const u32 len = all_pairs ? 0u : base + (seg < rem ? 1u : 0u);
    const u32 nbits = 2 * len;
    const u32 kb = std::min<u32>(c->lg_key_bits, nbits == 0 ? 1u : std::min<u32>(nbits, 64u));
    const u64 kmask = kb >= 64 ? ~0ull : ((1ull << kb) - 1ull);
    hipLaunchKernelGGL(k_long_seg_keys, dim3(blocks_for(U)), dim3(256), 0, st, leaf, U, k, pad + 2 * pos, nbits, kmask,
                       c->seg_k0.as<u64>(), c->seg_v0.as<u32>());
    TRY(sort_pairs<u64, u32>(c, c->seg_k0.as<u64>(), c->e_kx.as<u64>(), c->seg_v0.as<u32>(), c->e_vx.as<u32>(), U, 0, kb));
    ull *cand = c->lg_cand.as<ull>() + (size_t)seg * LONG_CAND_SLOTS;
    bool in_pieces = false;                        // join_append took this join through the pieces
    auto launch = [&](auto fill, auto keys, u64 n_pieces, u32 *pc, const u32 *poff, u64 *out) {
      constexpr bool FILL = decltype(fill)::value;
      using KT = typename decltype(keys)::key_type;
      if (n_pieces) {
        in_pieces = true;
        if (!FILL) (void)hipMemsetAsync(cand, 0, LONG_CAND_SLOTS * sizeof(ull), st);     // (what the join over the entries counted before it gave up)
        hipLaunchKernelGGL((k_long_join_chunks<FILL, KT>), dim3(blocks_for(n_pieces)), dim3(256), 0, st, keys.kx, keys.vx, keys.U,
                           (const u32 *)c->e_runlo.as<u32>(), (const u32 *)c->e_choff.as<u32>(), (u32)n_pieces, c->walk_max, leaf, k,
                           distance, pc, poff, out, cand);
      } else
        hipLaunchKernelGGL((k_long_join<FILL, KT>), dim3(blocks_for(keys.U)), dim3(256), 0, st, keys.kx, keys.vx, keys.U, leaf, k,
                           distance, pc, poff, out, c->walk_max, &c->d_ctr[CTR_BIGMASK], cand);
    };
    TRY(join_append(c, "long-word", c->e_kx.p, c->e_vx.as<u32>(), c->e_kx.p, c->e_vx.as<u32>(), U, false, launch, raw));
    if (in_pieces) c->lg_info.piece_joins++;
    c->lg_info.joins++;
    c->lg_info.key_bits = std::max<u32>(c->lg_info.key_bits, kb);
    pos += len;
  }
  HIPCHK(hipGetLastError());
  ull h_cand[MAX_COMBOS * LONG_CAND_SLOTS];
  HIPCHK(hipMemcpyAsync(h_cand, c->lg_cand.p, (size_t)nseg * LONG_CAND_SLOTS * sizeof(ull), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (u32 i = 0; i < nseg * LONG_CAND_SLOTS; i++) c->lg_info.candidates += h_cand[i];
  c->lg_info.raw_edges = raw;
  if (raw == 0) return HUMID_OK;
  TRY(unique_edges(c, c->e_raw.as<u64>(), raw, U, n_edges_out));
  c->lg_info.edges = *n_edges_out;
  return HUMID_OK;
}

// The full pipeline on device buffers for long words: stage_count_long, long_edges, the graph stage with the pairs
// GIVEN (as the strand-symmetric and edit-distance runs give theirs), then the unchanged stage_map.
static int run_device_long(humid_ctx *c, const u64 *d_words, const u8 *d_filt, u64 n_reads, u32 word_nt, u32 distance,
                           u32 method, u32 *d_cid, u8 *d_keep, humid_summary *sum) {
  if (!c) return HUMID_E_INVALID;
  state_reset(c);
  TRY(check_run_args(c, n_reads, word_nt, method, HUMID_LONG_MAX_NT));
  if (c->edit) return fail(c, HUMID_E_UNSUPPORTED, "option edit_distance is not supported for long words");
  if ((uintptr_t)d_words & 7) return fail(c, HUMID_E_INVALID, "long words must be 8-byte aligned on the device");
  if (n_reads && (!d_words || !d_filt || !d_cid || !d_keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const u32 N = (u32)n_reads, k = (word_nt + 31) / 32;
  humid_summary s;
  memset(&s, 0, sizeof s);
  s.total = n_reads;
  pass_begin(c, n_reads, word_nt, distance, method);
  c->lg_info = humid_long_info_t{};
  c->lg_info.words_per_read = k;
  auto publish = [&]() { if (sum) *sum = s; state_publish(c, CtxState::RUN); c->state.long_words = true; return HUMID_OK; };
  s.count_mode_used = 3u;
  if (N == 0) return publish();
  PassTimingGuard timing(c, false);                          // (no device stamps: the sorting count stores none)
  TRY(stage_count_long(c, d_words, d_filt, N, word_nt, s));
  const u32 U = (u32)c->U;
  if (U == 0) {   // everything filtered
    HIPCHK(hipMemsetAsync(d_cid, 0, (size_t)N * 4, st));
    HIPCHK(hipMemsetAsync(d_keep, 0, (size_t)N, st));
    HIPCHK(hipStreamSynchronize(st));
    return publish();
  }
  const u64 *leaf = c->s_word.as<u64>();
  u64 E = 0;
  TRY(long_edges(c, leaf, U, k, word_nt, distance, &E));
  u32 n_pair_segs = 0;
  // (the graph stage reads no word when its pairs are given: it runs as over one-uint64 leaves and the record is set right behind it)
  TRY(graph_stage<u64>(c, leaf, c->s_cnt.as<u32>(), U, std::min<u32>(word_nt, 32u), distance, method, s, n_pair_segs, true,
                       c->e_edges.as<u64>(), E));
  c->g_wpr = k;
  TRY(stage_map(c, c->cid.as<u32>(), c->ismax.as<u8>(), N, d_cid, d_keep));
  if (c->cg_valid) TRY(n_clusters_compact(c, U, &c->C));
  else TRY(n_clusters_from_scan(c, U, &c->C));
  s.clusters = c->C;
  s.nonsingle = c->M;
  TRY(timing_tail(c, s, n_pair_segs, false));                // (ms_k_insert: the k sorts)
  return publish();
}

// ---- accumulated runs (humid_accum_*): a read set fed in chunks (kernels_accum.hip.h) --------------------------
// add = the count stage over the chunk + accum_merge; finish = the graph stage over the accumulated list + a copy of
// its cid / ismax; map = the count stage over the chunk + accum_lookup + the unchanged stage_map.  Per-read work stays
// in the count and un-permute kernels; what is new is proportional to unique words.
// the count stage over one chunk, leaving the context as humid_stage_count does
template <class WT>
static int accum_count_chunk(humid_ctx *c, const WT *d_words, const u8 *d_filt, u64 n_reads) {
  humid_summary s;
  memset(&s, 0, sizeof s);
  const u32 nt = c->ac_keyed ? c->ac_ent_nt : c->ac_nt;       // (a keyed accumulator counts entries)
  pass_begin(c, n_reads, nt);
  if (n_reads == 0) return HUMID_OK;
  if constexpr (sizeof(WT) == 16) return stage_count_wide(c, d_words, d_filt, (u32)n_reads, nt, s);
  else return stage_count(c, d_words, d_filt, (u32)n_reads, nt, 0ull, ~0ull, 0, s);
}

// The list of set ac_cur merged with the chunk just counted (s_word / s_cnt / s_first of c->U words, first read
// = base + s_first) into the other set; the sets swap at the end.  ONE host wait: the new number of words sizes
// the buffers the fill pass writes (the same wait brings the overflow flag).  Every failure leaves ac_cur and
// ac_U as they were.
template <class WT>
static int accum_merge(humid_ctx *c, u64 base) {
  hipStream_t st = c->stream;
  const u32 nA = (u32)c->ac_U, nB = (u32)c->U, T = c->ac_tile;
  const u64 P = (u64)nA + nB;                                  // (both below 2^31)
  const u32 n_tiles = (u32)((P + T - 1) / T);
  const u32 cur = c->ac_cur, nxt = cur ^ 1u;
  PASS_ENSURE(c->ac_split, ((size_t)n_tiles + 1) * 4);
  PASS_ENSURE(c->ac_tcnt, ((size_t)n_tiles + 1) * 4);
  PASS_ENSURE(c->ac_toff, ((size_t)n_tiles + 1) * 4);
  PASS_ENSURE(c->ac_flag, 16);
  HIPCHK(hipMemsetAsync(c->ac_flag.p, 0, 16, st));
  HIPCHK(hipMemsetAsync(c->ac_tcnt.as<u32>() + n_tiles, 0, 4, st));      // (the scan's sentinel)
  const WT *a_word = c->ac_word[cur].as<WT>(), *b_word = c->s_word.as<WT>();
  const u32 *a_cnt = c->ac_cnt[cur].as<u32>(), *b_cnt = c->s_cnt.as<u32>(), *b_first = c->s_first.as<u32>();
  const u64 *a_first = c->ac_first[cur].as<u64>();
  const size_t lds = ((size_t)T + 2) * sizeof(WT);
  hipLaunchKernelGGL((k_accum_partition<WT>), dim3(blocks_for((u64)n_tiles + 1)), dim3(256), 0, st, a_word, nA, b_word, nB, T, n_tiles,
                     c->ac_split.as<u32>());
  hipLaunchKernelGGL((k_accum_tile<WT, 0>), dim3(n_tiles), dim3(ACC_THREADS), lds, st, a_word, a_cnt, a_first, nA, b_word, b_cnt, b_first,
                     nB, base, T, (const u32 *)c->ac_split.as<u32>(), c->ac_tcnt.as<u32>(), (const u32 *)nullptr, (WT *)nullptr,
                     (u32 *)nullptr, (u64 *)nullptr, c->ac_flag.as<u32>());
  TRY(exscan_u32(c, c->ac_tcnt.as<u32>(), c->ac_toff.as<u32>(), (u64)n_tiles + 1));
  HIPCHK(hipGetLastError());
  TRY(read_counters(c, c->ac_toff.as<u32>() + n_tiles, c->ac_flag.as<u32>()));
  const u64 nU = c->h_ctr[CTR_N - 1] & 0xffffffffull;
  if (c->h_ctr[CTR_N - 2] & 0xffffffffull) return fail(c, HUMID_E_OVERFLOW, "the reads of one word exceed 2^32-1");
  if (nU > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "%llu accumulated unique words exceed 2^31-1", (ull)nU);
  // (a set that must grow doubles: an allocation and the release of the old block cost more than a merge)
  auto room = [](const DBuf &b, size_t bytes) { return bytes <= b.cap ? bytes : std::max(bytes, 2 * b.cap); };
  PASS_ENSURE(c->ac_word[nxt], room(c->ac_word[nxt], (size_t)nU * sizeof(WT) + 16));
  PASS_ENSURE(c->ac_cnt[nxt], room(c->ac_cnt[nxt], (size_t)nU * 4 + 16));
  PASS_ENSURE(c->ac_first[nxt], room(c->ac_first[nxt], (size_t)nU * 8 + 16));
  hipLaunchKernelGGL((k_accum_tile<WT, 1>), dim3(n_tiles), dim3(ACC_THREADS), lds, st, a_word, a_cnt, a_first, nA, b_word, b_cnt, b_first,
                     nB, base, T, (const u32 *)c->ac_split.as<u32>(), (u32 *)nullptr, (const u32 *)c->ac_toff.as<u32>(),
                     c->ac_word[nxt].as<WT>(), c->ac_cnt[nxt].as<u32>(), c->ac_first[nxt].as<u64>(), (u32 *)nullptr);
  HIPCHK(hipGetLastError());
  c->ac_cur = nxt;
  c->ac_U = nU;
  return HUMID_OK;
}

// The graph stage over the accumulated list (not the context's own unique words: stage_graph's `own` is false), the
// cluster count, and the copy of cid / ismax a later map reads -- map counts its chunk in the context's buffers.
template <class WT>
static int accum_finish(humid_ctx *c, u32 distance, u32 method, humid_summary &s) {
  const u32 U = (u32)c->ac_U, cur = c->ac_cur;
  if (U == 0) return HUMID_OK;
  const WT *g_word = c->ac_word[cur].as<WT>();
  const u32 *g_cnt = c->ac_cnt[cur].as<u32>();
  u32 nps = 0;
  if (c->edit && distance >= 2) {
    u64 E = 0;
    TRY(edit_edges<WT>(c, g_word, U, c->ac_nt, distance, &E));
    TRY(stage_graph<WT>(c, g_word, g_cnt, U, c->ac_nt, distance, method, s, nps, edges_or_empty(c->e_edges.as<u64>(), E), E));
  } else
    TRY(stage_graph<WT>(c, g_word, g_cnt, U, c->ac_nt, distance, method, s, nps));
  TRY(n_clusters_from_scan(c, U, &c->C));
  s.clusters = c->C;
  PASS_ENSURE(c->ac_cid, (size_t)U * 4 + 16);
  PASS_ENSURE(c->ac_ismax, (size_t)U + 16);
  HIPCHK(hipMemcpyAsync(c->ac_cid.p, c->cid.p, (size_t)U * 4, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->ac_ismax.p, c->ismax.p, (size_t)U, hipMemcpyDeviceToDevice, c->stream));
  return HUMID_OK;
}

// Per-read results of the chunk just counted: its leaves looked up in the accumulated list, then stage_map.
// *h_unknown: usable reads whose word the accumulator never saw (they get 0 / 0).
template <class WT>
static int accum_map(humid_ctx *c, u64 base, u32 *d_cid, u8 *d_keep, u64 *h_unknown) {
  hipStream_t st = c->stream;
  const u32 N = (u32)c->N, nB = (u32)c->U, nA = (u32)c->ac_U, cur = c->ac_cur;
  *h_unknown = 0;
  if (N == 0) return HUMID_OK;
  if (nB == 0) {                                               // everything filtered
    HIPCHK(hipMemsetAsync(d_cid, 0, (size_t)N * 4, st));
    HIPCHK(hipMemsetAsync(d_keep, 0, (size_t)N, st));
    return HUMID_OK;
  }
  PASS_ENSURE(c->ac_lcid, (size_t)nB * 4 + 16);
  PASS_ENSURE(c->ac_lismax, (size_t)nB + 16);
  PASS_ENSURE(c->ac_flag, 16);
  HIPCHK(hipMemsetAsync(c->ac_flag.p, 0, 16, st));
  ull *unknown = c->ac_flag.as<ull>() + 1;
  hipLaunchKernelGGL((k_accum_lookup<WT>), dim3(grid_stride_blocks(nB)), dim3(256), 0, st, c->ac_word[cur].as<WT>(),
                     c->ac_first[cur].as<u64>(), c->ac_cid.as<u32>(), c->ac_ismax.as<u8>(), nA, c->s_word.as<WT>(), c->s_cnt.as<u32>(),
                     c->s_first.as<u32>(), nB, base, c->ac_lcid.as<u32>(), c->ac_lismax.as<u8>(), unknown);
  HIPCHK(hipGetLastError());
  TRY(stage_map(c, c->ac_lcid.as<u32>(), c->ac_lismax.as<u8>(), N, d_cid, d_keep));
  HIPCHK(hipMemcpyAsync(h_unknown, unknown, 8, hipMemcpyDeviceToHost, st));
  return HUMID_OK;
}

// ---- grouped runs (humid_dedup_run_grouped*): one pass over many groups ------------------------------------
// group nucleotides of n_groups groups: ceil(ceil(log2(n_groups)) / 2), 0 for one group
static inline u32 gkey_nt_for(u32 n_groups) { return n_groups <= 1 ? 0u : (bits_for(n_groups) + 1) / 2; }

static int check_grouped_args(humid_ctx *c, u32 word_nt, u32 n_groups) {
  if (n_groups == 0) return fail(c, HUMID_E_INVALID, "n_groups must be >= 1");
  if (word_nt >= 1 && word_nt <= 64 && word_nt + gkey_nt_for(n_groups) > 64)
    return fail(c, HUMID_E_UNSUPPORTED, "word_nt %u + %u group nucleotides (%u groups) > 64 is not supported", word_nt,
                gkey_nt_for(n_groups), n_groups);
  return HUMID_OK;
}

// The whole grouped pass: k_gkey_words writes the internal words (and checks the groups), run_device runs the
// pass over them with the group field in every combination of the plan.  group == null: all reads in group 0
// (n_groups must be 1), the plain pass itself.  WI: the caller's word type (word_nt <= 32: u64).
// d_key != null (run_keyed_device, which has ranked the keys into c->kr_table; d_group is null): the group of a read
// is the rank of its key, n_groups the number of distinct keys, and k_kr_words writes the internal words.
template <class WI>
static int run_grouped_device(humid_ctx *c, const WI *d_words, const u32 *d_group, const u8 *d_filt, u64 n_reads,
                              u32 word_nt, u32 n_groups, u32 distance, u32 method, u32 *d_cid, u8 *d_keep,
                              humid_summary *sum, const u64 *d_key = nullptr) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  state_reset(c);
  TRY(check_run_args(c, n_reads, word_nt, method, 64));
  TRY(check_grouped_args(c, word_nt, n_groups));
  if (!d_group && !d_key && n_groups > 1) return fail(c, HUMID_E_INVALID, "group is null with n_groups = %u > 1", n_groups);
  if (n_reads && (!d_words || !d_filt || !d_cid || !d_keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  if (sizeof(WI) == 16 && ((uintptr_t)d_words & 15)) return fail(c, HUMID_E_INVALID, "wide words must be 16-byte aligned on the device");
  HIPCHK(hipSetDevice(c->device));
  const u32 gnt = gkey_nt_for(n_groups), n_int = word_nt + gnt, N = (u32)n_reads;
  PassKind pass(c, RUN_GROUPED);
  c->gk_nt = gnt;
  c->gk_word_nt = word_nt;
  c->gk_leaf_nt = gnt;
  c->gk_groups = n_groups;
  c->gk_epoch = c->gk_epoch + 1 ? c->gk_epoch + 1 : 1;     // (a value a store of an earlier pass cannot match)
  int rc;
  if ((!d_group && !d_key) || N == 0 || (d_key && gnt == 0)) {
    rc = run_device<WI>(c, d_words, d_filt, n_reads, word_nt, distance, method, d_cid, d_keep, sum);
  } else {
    hipStream_t st = c->stream;
    const bool wide = n_int > 32, copy = gnt > 0;             // (one group: the caller's words are the internal ones)
    if (copy) ENSURE(c->gk_words, (size_t)N * (wide ? 16 : 8) + 16);
    u32 *bad = nullptr;
    TRY(gkey_bad_word(c, &bad));
    if (d_key && wide)
      hipLaunchKernelGGL((k_kr_words<WI, W2>), dim3(blocks_for(N)), dim3(256), 0, st, d_words, d_key, d_filt, N,
                         (const KrSlot *)c->kr_table.p, c->kr_last_log2, n_groups, word_nt, gnt, c->gk_words.as<W2>(), bad, c->gk_epoch);
    else if (d_key)
      hipLaunchKernelGGL((k_kr_words<WI, u64>), dim3(blocks_for(N)), dim3(256), 0, st, d_words, d_key, d_filt, N,
                         (const KrSlot *)c->kr_table.p, c->kr_last_log2, n_groups, word_nt, gnt, c->gk_words.as<u64>(), bad, c->gk_epoch);
    else if (wide)
      hipLaunchKernelGGL((k_gkey_words<WI, W2>), dim3(blocks_for(N)), dim3(256), 0, st, d_words, d_group, d_filt, N,
                         word_nt, gnt, n_groups, copy ? c->gk_words.as<W2>() : nullptr, bad, c->gk_epoch);
    else
      hipLaunchKernelGGL((k_gkey_words<WI, u64>), dim3(blocks_for(N)), dim3(256), 0, st, d_words, d_group, d_filt, N,
                         word_nt, gnt, n_groups, copy ? c->gk_words.as<u64>() : nullptr, bad, c->gk_epoch);
    HIPCHK(hipGetLastError());
    TRY(gkey_bad_fetch(c, bad));
    if (!copy) rc = run_device<WI>(c, d_words, d_filt, n_reads, word_nt, distance, method, d_cid, d_keep, sum);
    else if (wide) rc = run_device<W2>(c, c->gk_words.as<W2>(), d_filt, n_reads, n_int, distance, method, d_cid, d_keep, sum);
    else rc = run_device<u64>(c, c->gk_words.as<u64>(), d_filt, n_reads, n_int, distance, method, d_cid, d_keep, sum);
  }
  if (rc == HUMID_OK) c->word_nt = word_nt;
  return rc;
}

// ---- keyed runs (humid_dedup_run_keyed*): grouped runs whose groups are the ranks of 64-bit keys ---------------
// Ranks the distinct keys of the usable reads on the device (kernels_keyrank.hip.h): table insert, compaction, ONE
// host wait (the number of distinct keys G chooses group_nt and the plan; the same wait reports a table that was
// too small, and the ranking is then repeated with a larger one), a G-proportional sort, the ranks written back
// into the table.  Leaves c->kr_keys (G sorted keys), c->kr_n = G and c->kr_table / kr_last_log2 for k_kr_words.
static int rank_keys(humid_ctx *c, const u64 *d_key, const u8 *d_filt, u32 N) {
  hipStream_t st = c->stream;
  u32 full_log2 = 4;                                          // the size that cannot be too small: cap >= 2 N
  while (full_log2 < 32 && ((u64)1 << full_log2) < 2 * (u64)N) full_log2++;
  u32 cap_log2 = c->kr_force_log2 ? c->kr_force_log2 : (c->kr_cap_log2 ? c->kr_cap_log2 : 16u);
  cap_log2 = std::min(std::max(cap_log2, 4u), full_log2);
  c->kr_redo = 0;
  u32 G = 0;
  u64 bits = 0;
  while (true) {
    const u32 cap = 1u << cap_log2;
    const u32 out_cap = std::min<u64>((u64)cap + 1, N);         // (every distinct key is some read's key)
    ENSURE(c->kr_table, ((size_t)cap + 1) * sizeof(KrSlot));
    ENSURE(c->kr_raw, (size_t)out_cap * 8 + 16);
    ENSURE(c->kr_rawslot, (size_t)out_cap * 4 + 16);
    HIPCHK(hipMemsetAsync(c->kr_table.p, 0xff, ((size_t)cap + 1) * sizeof(KrSlot), st));
    HIPCHK(hipMemsetAsync(c->d_ctr, 0, CTR_N * sizeof(ull), st));
    hipLaunchKernelGGL(k_kr_insert, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_key, d_filt, N, c->kr_table.as<KrSlot>(),
                       cap_log2, cap_log2 == full_log2 ? cap : 128u, c->d_ctr);
    hipLaunchKernelGGL(k_kr_compact, dim3(std::min<u32>(COMPACT_BLOCKS, blocks_for((u64)cap + 1))), dim3(256), 0, st,
                       (const KrSlot *)c->kr_table.p, cap, c->kr_raw.as<u64>(), c->kr_rawslot.as<u32>(), out_cap, c->d_ctr);
    HIPCHK(hipGetLastError());
    TRY(read_counters(c));                                     // the host wait of the ranking
    const bool overfull = c->h_ctr[CTR_OVERFULL] != 0 || c->h_ctr[CTR_UNIQUE] > out_cap;
    if (!overfull) { G = (u32)c->h_ctr[CTR_UNIQUE]; bits = c->h_ctr[CTR_KEYBITS]; break; }
    if (cap_log2 >= full_log2) return fail(c, HUMID_E_INVALID, "internal: the key table of 2^%u slots overflowed", cap_log2);
    cap_log2 = std::min(cap_log2 + 4, full_log2);
    c->kr_redo++;
  }
  c->kr_last_log2 = cap_log2;
  c->kr_n = G;
  // the next ranking starts with a table at most a third full for as many keys as this one saw
  u32 next = 12;
  while (next < full_log2 && ((u64)1 << next) < 3 * (u64)G) next++;
  c->kr_cap_log2 = next;
  if (G == 0) return HUMID_OK;
  ENSURE(c->kr_keys, (size_t)G * 8 + 16);
  ENSURE(c->kr_slot, (size_t)G * 4 + 16);
  TRY((sort_pairs<u64, u32>(c, c->kr_raw.as<u64>(), c->kr_keys.as<u64>(), c->kr_rawslot.as<u32>(), c->kr_slot.as<u32>(), G, 0,
                            bits ? 64u - (u32)__builtin_clzll(bits) : 1u)));          // (key bits above the highest one set: all 0)
  hipLaunchKernelGGL(k_kr_ranks, dim3(blocks_for(G)), dim3(256), 0, st, (const u32 *)c->kr_slot.p, G, c->kr_table.as<KrSlot>(),
                     1u << cap_log2);
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// The whole keyed pass.  WI: the caller's word type (word_nt <= 32: u64).
template <class WI>
static int run_keyed_device(humid_ctx *c, const WI *d_words, const u64 *d_key, const u8 *d_filt, u64 n_reads, u32 word_nt,
                            u32 distance, u32 method, u32 *d_cid, u8 *d_keep, humid_summary *sum) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  state_reset(c);
  TRY(check_run_args(c, n_reads, word_nt, method, 64));
  if (n_reads && (!d_words || !d_key || !d_filt || !d_cid || !d_keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  PassKind pass(c, RUN_KEYED);
  c->kr_n = 0;
  if (n_reads) TRY(rank_keys(c, d_key, d_filt, (u32)n_reads));
  return run_grouped_device<WI>(c, d_words, nullptr, d_filt, n_reads, word_nt, std::max(c->kr_n, 1u), distance, method,
                                d_cid, d_keep, sum, n_reads ? d_key : nullptr);
}

// ---- keyed accumulators (humid_accum_*_keyed; the second half of kernels_accum.hip.h) -----------------------------
// add / map = k_acck_pack over the chunk + the plain accumulator's add / map over the entries; finish = the keys ranked
// off the sorted list + a keyed graph stage over the internal words.  ET: the entry type.
// The chunk's entries into c->gk_words and the count stage over them.  A usable key beyond key_nt is seen at the count
// stage's host wait, before anything of the accumulator is touched.
template <class ET>
static int accum_pack_count(humid_ctx *c, const u64 *d_words, const u64 *d_key, const u8 *d_filt, u64 n_reads) {
  const u32 N = (u32)n_reads;
  if (N) {
    ENSURE(c->gk_words, (size_t)N * sizeof(ET) + 16);
    c->gk_epoch = c->gk_epoch + 1 ? c->gk_epoch + 1 : 1;
    u32 *bad = nullptr;
    TRY(gkey_bad_word(c, &bad));
    hipLaunchKernelGGL((k_acck_pack<ET>), dim3(blocks_for(N)), dim3(256), 0, c->stream, d_words, d_key, d_filt, N, c->ac_nt,
                       c->ac_key_nt, c->gk_words.as<ET>(), bad, c->gk_epoch);
    HIPCHK(hipGetLastError());
    TRY(gkey_bad_fetch(c, bad));
  }
  TRY(accum_count_chunk(c, (const ET *)c->gk_words.p, d_filt, n_reads));
  if (N && *(volatile u32 *)&c->h_ctr[CTR_N + 1] == c->gk_epoch)
    return fail(c, HUMID_E_INVALID, "a usable read has a key >= 4^%u", c->ac_key_nt);
  return HUMID_OK;
}

// The distinct keys of the accumulated list: head flags and their scan (left in ac_head / ac_hpos for k_acck_ranks), and
// finish's ONE extra host wait: *G chooses the group field and with it the internal word type and the plan.
template <class ET>
static int accum_rank_keys(humid_ctx *c, u32 *G) {
  const u32 U = (u32)c->ac_U;
  PASS_ENSURE(c->ac_head, ((size_t)U + 1) * 4);
  PASS_ENSURE(c->ac_hpos, ((size_t)U + 1) * 4);
  hipLaunchKernelGGL((k_acck_heads<ET>), dim3(grid_stride_blocks((u64)U + 1)), dim3(256), 0, c->stream,
                     c->ac_word[c->ac_cur].as<ET>(), U, 2 * c->ac_nt, c->ac_head.as<u32>());
  u64 total = 0;
  TRY(scan_total(c, c->ac_head.as<u32>(), c->ac_hpos.as<u32>(), U, &total));
  *G = (u32)total;
  return HUMID_OK;
}

// The keyed graph stage over the accumulated list: internal words `rank << 2 * word_nt | word` (ascending, because
// (key, word) order is (rank, word) order) and the keys into the accumulator's buffers, then what accum_finish does,
// with the context set as run_grouped_device sets it for a keyed pass.  IT: the internal word type.
template <class ET, class IT>
static int accum_finish_keyed(humid_ctx *c, u32 G, u32 distance, u32 method, humid_summary &s) {
  const u32 U = (u32)c->ac_U, cur = c->ac_cur, gnt = gkey_nt_for(G), n_int = c->ac_nt + gnt;
  PASS_ENSURE(c->ac_keys, (size_t)G * 8 + 16);
  PASS_ENSURE(c->ac_iword, (size_t)U * sizeof(IT) + 16);
  hipLaunchKernelGGL((k_acck_ranks<ET, IT>), dim3(grid_stride_blocks(U)), dim3(256), 0, c->stream, c->ac_word[cur].as<ET>(),
                     (const u32 *)c->ac_head.p, (const u32 *)c->ac_hpos.p, U, 2 * c->ac_nt, c->ac_keys.as<u64>(), c->ac_iword.as<IT>());
  HIPCHK(hipGetLastError());
  PassKind pass(c, RUN_KEYED);
  c->gk_nt = gnt;
  c->gk_word_nt = c->ac_nt;
  c->gk_leaf_nt = gnt;
  c->gk_groups = G;
  c->kr_n = G;
  const IT *g_word = c->ac_iword.as<IT>();
  const u32 *g_cnt = c->ac_cnt[cur].as<u32>();
  u32 nps = 0;
  if (c->edit && distance >= 2) {
    u64 E = 0;
    TRY(edit_edges<IT>(c, g_word, U, n_int, distance, &E));
    TRY(stage_graph<IT>(c, g_word, g_cnt, U, n_int, distance, method, s, nps, edges_or_empty(c->e_edges.as<u64>(), E), E));
  } else
    TRY(stage_graph<IT>(c, g_word, g_cnt, U, n_int, distance, method, s, nps));
  TRY(n_clusters_from_scan(c, U, &c->C));
  s.clusters = c->C;
  PASS_ENSURE(c->ac_cid, (size_t)U * 4 + 16);
  PASS_ENSURE(c->ac_ismax, (size_t)U + 16);
  HIPCHK(hipMemcpyAsync(c->ac_cid.p, c->cid.p, (size_t)U * 4, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->ac_ismax.p, c->ismax.p, (size_t)U, hipMemcpyDeviceToDevice, c->stream));
  return HUMID_OK;
}

// finish of a keyed accumulator with a non-empty list
template <class ET>
static int accum_finish_keyed_any(humid_ctx *c, u32 distance, u32 method, humid_summary &s) {
  u32 G = 0;
  TRY(accum_rank_keys<ET>(c, &G));
  c->ac_G = G;
  if constexpr (sizeof(ET) == 16)                              // (a one-word entry holds key_nt >= group nucleotides)
    if (c->ac_nt + gkey_nt_for(G) > 32) return accum_finish_keyed<ET, W2>(c, G, distance, method, s);
  return accum_finish_keyed<ET, u64>(c, G, distance, method, s);
}

// The count stage over a chunk on the device -- over its entries (accum_pack_count) when the accumulator
// is a keyed one --, then f, called with a null pointer to the type of the list's entries.
template <class F>
static int accum_counted(humid_ctx *c, const u64 *d_words, const u64 *d_key, const u8 *d_filt, u64 n_reads, F f) {
  if (c->ac_keyed)
    return with_word_type(c->ac_ent_nt, [&](auto *w) {
      TRY(accum_pack_count<std::remove_cv_t<std::remove_pointer_t<decltype(w)>>>(c, d_words, d_key, d_filt, n_reads));
      return f(w);
    });
  return with_word_type(c->ac_nt, [&](auto *w) {
    TRY(accum_count_chunk(c, (decltype(w))d_words, d_filt, n_reads));
    return f(w);
  });
}

// ---- barcode whitelist (humid_whitelist_*, humid_dedup_run_keyed_corrected*; kernels_whitelist.hip.h) -----------
#define SEG_NO_POSTERIOR "the correction by quality and abundance does not work with a segmented whitelist (humid_whitelist_set_segments)"
// the whitelist in place stops being a segmented one (it is replaced by a plain one, or cleared)
static void seg_drop(humid_ctx *c) {
  c->sg_table.release();
  c->sg = SegPlan{};
  c->sg_sum_valid = false;
}

// the whitelist in place changed: the reads per slot of a posterior call, and a prior fed in chunks, went with the table
// they index
static void wl_counts_drop(humid_ctx *c) {
  c->wp_valid = false;
  c->wp_prior = false;
  c->pr_state = CC_NONE;
}

// The correction pass over device arrays: zeroes d_counts (u64[5]) and launches the kernel; nothing waits here.
static int wl_correct_launch(humid_ctx *c, const u64 *d_key, const u8 *d_filt, u32 N, u64 *d_key_out, u8 *d_status,
                             u8 *d_filt_out, ull *d_counts) {
  hipStream_t st = c->stream;
  HIPCHK(hipMemsetAsync(d_counts, 0, 5 * sizeof(ull), st));
  if (c->sg.n_seg) {                                                // a segmented whitelist: S table reads per read, no probing
    c->sg_sum_valid = false;
    PASS_ENSURE(c->sg_sum, SEG_SUM_N * sizeof(ull));
    HIPCHK(hipMemsetAsync(c->sg_sum.p, 0, SEG_SUM_N * sizeof(ull), st));
    if (N) {
      hipLaunchKernelGGL(k_seg_resolve, dim3(blocks_for(N)), dim3(256), 0, st, d_key, d_filt, N, (const u32 *)c->sg_table.p, c->sg,
                         d_key_out, d_status, d_filt_out, d_counts, c->sg_sum.as<ull>());
      HIPCHK(hipGetLastError());
    }
    c->sg_sum_valid = true;
    return HUMID_OK;
  }
  if (N == 0) return HUMID_OK;
  if (c->wl_coop)
    hipLaunchKernelGGL(k_wl_correct<true>, dim3(blocks_for(N)), dim3(256), 0, st, d_key, d_filt, N, (const u64 *)c->wl_table.p,
                       c->wl_log2, 3 * c->wl_nt, d_key_out, d_status, d_filt_out, d_counts);
  else
    hipLaunchKernelGGL(k_wl_correct<false>, dim3(blocks_for(N)), dim3(256), 0, st, d_key, d_filt, N, (const u64 *)c->wl_table.p,
                       c->wl_log2, 3 * c->wl_nt, d_key_out, d_status, d_filt_out, d_counts);
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// The posterior correction over device arrays: zeroes d_counts (u64[WLP_CTRS]) and the reads per slot, then the prior
// and the decision pass; nothing waits here.  The per-slot and per-read arrays are plain allocations of the context.
static int wl_posterior_launch(humid_ctx *c, const u64 *d_key, const u8 *d_filt, const u8 *d_qual, u32 N, u32 min_odds,
                               u64 *d_key_out, u8 *d_status, u8 *d_filt_out, ull *d_counts) {
  hipStream_t st = c->stream;
  const size_t cap = (size_t)1 << c->wl_log2;
  c->wp_valid = false;
  PASS_ENSURE(c->wp_cnt, (cap + 1) * 4);
  PASS_ENSURE(c->wp_slot, (size_t)N * 4 + 16);
  HIPCHK(hipMemsetAsync(d_counts, 0, WLP_CTRS * sizeof(ull), st));
  HIPCHK(hipMemsetAsync(c->wp_cnt.p, 0, (cap + 1) * 4, st));
  if (N) {
    const u64 *tab = (const u64 *)c->wl_table.p;
    const dim3 grid(blocks_for(N)), block(256);
    hipLaunchKernelGGL((k_wlp_prior<true, true>), grid, block, 0, st, d_key, d_filt, N, tab, c->wl_log2, c->wp_cnt.as<u32>(), c->wp_slot.as<u32>(),
                       (ull *)nullptr);
    if (c->wl_coop)
      hipLaunchKernelGGL(k_wlp_decide<true>, grid, block, 0, st, d_key, d_filt, d_qual, N, (const u32 *)c->wp_slot.p, tab, c->wl_log2,
                         (const u32 *)c->wp_cnt.p, c->wl_nt, min_odds, d_key_out, d_status, d_filt_out, d_counts);
    else
      hipLaunchKernelGGL(k_wlp_decide<false>, grid, block, 0, st, d_key, d_filt, d_qual, N, (const u32 *)c->wp_slot.p, tab, c->wl_log2,
                         (const u32 *)c->wp_cnt.p, c->wl_nt, min_odds, d_key_out, d_status, d_filt_out, d_counts);
    HIPCHK(hipGetLastError());
  }
  c->wp_valid = true;
  c->wp_prior = false;                                              // (humid_whitelist_counts answers this call's counts)
  return HUMID_OK;
}

// The prior fed in chunks (humid_whitelist_prior_*; state and arguments checked by the entry points).  begin: the
// counts per slot of the table in place, zeroed, in an array of their own.
static int wl_prior_begin(humid_ctx *c) {
  HIPCHK(hipSetDevice(c->device));
  const size_t cap = (size_t)1 << c->wl_log2;
  c->pr_state = CC_NONE;
  PASS_ENSURE(c->pr_cnt, (cap + 1) * 4);
  PASS_ENSURE(c->pr_ctr, sizeof(ull));
  HIPCHK(hipMemsetAsync(c->pr_cnt.p, 0, (cap + 1) * 4, c->stream));
  HIPCHK(hipMemsetAsync(c->pr_ctr.p, 0, sizeof(ull), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->pr_state = CC_ON;
  c->wp_prior = true;                                               // (humid_whitelist_counts answers the accumulated counts)
  return HUMID_OK;
}

// add: the counting half of k_wlp_prior over a chunk, and one host wait for the overflow flag
static int wl_prior_add_chunk(humid_ctx *c, const u64 *d_key, const u8 *d_filt, u32 N) {
  if (N == 0) return HUMID_OK;
  hipLaunchKernelGGL((k_wlp_prior<true, false>), dim3(blocks_for(N)), dim3(256), 0, c->stream, d_key, d_filt, N, (const u64 *)c->wl_table.p,
                     c->wl_log2, c->pr_cnt.as<u32>(), (u32 *)nullptr, c->pr_ctr.as<ull>());
  HIPCHK(hipGetLastError());
  ull over = 0;
  HIPCHK(hipMemcpyAsync(&over, c->pr_ctr.p, sizeof over, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (over) return fail(c, HUMID_E_OVERFLOW, "a barcode's reads exceed 2^31-2: the prior is invalid until humid_whitelist_prior_begin");
  return HUMID_OK;
}
static int wl_prior_add(humid_ctx *c, const u64 *d_key, const u8 *d_filt, u32 N) {
  const int rc = wl_prior_add_chunk(c, d_key, d_filt, N);
  if (rc != HUMID_OK) c->pr_state = CC_INVALID;
  else c->wp_prior = true;
  return rc;
}

// The posterior correction of a chunk against the accumulated prior: zeroes d_counts (u64[WLP_CTRS]), then the lookup
// half of k_wlp_prior and the decision pass, unchanged, over pr_cnt; nothing waits here.  wp_cnt is not touched.
static int wl_posterior_prior_launch(humid_ctx *c, const u64 *d_key, const u8 *d_filt, const u8 *d_qual, u32 N, u32 min_odds,
                                     u64 *d_key_out, u8 *d_status, ull *d_counts) {
  hipStream_t st = c->stream;
  PASS_ENSURE(c->wp_slot, (size_t)N * 4 + 16);
  HIPCHK(hipMemsetAsync(d_counts, 0, WLP_CTRS * sizeof(ull), st));
  if (N) {
    const u64 *tab = (const u64 *)c->wl_table.p;
    const dim3 grid(blocks_for(N)), block(256);
    hipLaunchKernelGGL((k_wlp_prior<false, true>), grid, block, 0, st, d_key, d_filt, N, tab, c->wl_log2, (u32 *)nullptr, c->wp_slot.as<u32>(),
                       (ull *)nullptr);
    if (c->wl_coop)
      hipLaunchKernelGGL(k_wlp_decide<true>, grid, block, 0, st, d_key, d_filt, d_qual, N, (const u32 *)c->wp_slot.p, tab, c->wl_log2,
                         (const u32 *)c->pr_cnt.p, c->wl_nt, min_odds, d_key_out, d_status, (u8 *)nullptr, d_counts);
    else
      hipLaunchKernelGGL(k_wlp_decide<false>, grid, block, 0, st, d_key, d_filt, d_qual, N, (const u32 *)c->wp_slot.p, tab, c->wl_log2,
                         (const u32 *)c->pr_cnt.p, c->wl_nt, min_odds, d_key_out, d_status, (u8 *)nullptr, d_counts);
    HIPCHK(hipGetLastError());
  }
  c->wp_prior = true;
  return HUMID_OK;
}

// The corrected keyed pass: key_out and filtered' (filtered, ambiguous or unmatched) into context buffers, then the
// keyed pass over them, unchanged.  The status counts are not waited for: humid_get_barcode_status reads them.
// d_qual != null: the posterior correction (min_odds >= 1) in place of the plain one.
template <class WI>
static int run_keyed_corrected_device(humid_ctx *c, const WI *d_words, const u64 *d_key, const u8 *d_filt, u64 n_reads,
                                      u32 word_nt, u32 distance, u32 method, u32 *d_cid, u8 *d_keep, humid_summary *sum,
                                      const u8 *d_qual = nullptr, u32 min_odds = 0, bool posterior = false) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  state_reset(c);
  if (!c->wl_n) return fail(c, HUMID_E_STATE, "no whitelist is set in this context (humid_whitelist_set)");
  if (posterior && c->sg.n_seg) return fail(c, HUMID_E_UNSUPPORTED, SEG_NO_POSTERIOR);
  if (posterior && min_odds == 0) return fail(c, HUMID_E_INVALID, "min_odds must be >= 1");
  if (posterior && n_reads && !d_qual) return fail(c, HUMID_E_INVALID, "null buffer");
  TRY(check_run_args(c, n_reads, word_nt, method, 64));
  if (n_reads && (!d_words || !d_key || !d_filt || !d_cid || !d_keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  const u32 N = (u32)n_reads;
  ENSURE(c->bc_key, (size_t)N * 8 + 16);
  ENSURE(c->bc_filt, (size_t)N + 16);
  ENSURE(c->bc_status, (size_t)N + 16);
  ENSURE(c->bc_counts, WLP_CTRS * sizeof(ull));
  if (posterior)
    TRY(wl_posterior_launch(c, d_key, d_filt, d_qual, N, min_odds, c->bc_key.as<u64>(), c->bc_status.as<u8>(), c->bc_filt.as<u8>(),
                            c->bc_counts.as<ull>()));
  else
    TRY(wl_correct_launch(c, d_key, d_filt, N, c->bc_key.as<u64>(), c->bc_status.as<u8>(), c->bc_filt.as<u8>(),
                          c->bc_counts.as<ull>()));
  PassKind pass(c, RUN_CORRECTED);
  c->bc_N = n_reads;
  c->bc_posterior = posterior;
  return run_keyed_device<WI>(c, d_words, c->bc_key.as<u64>(), c->bc_filt.as<u8>(), n_reads, word_nt, distance, method, d_cid,
                              d_keep, sum);
}

// ---- whitelist from the data (humid_whitelist_discover*; kernels_cells.hip.h) ---------------------------------------
// what both forms refuse before anything moves
static int cells_discover_args(humid_ctx *c, const void *key, const void *filtered, u64 n_reads, u32 barcode_nt, u32 mode,
                               u64 param) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (barcode_nt < 1 || barcode_nt > 32) return fail(c, HUMID_E_INVALID, "barcode_nt must be 1 .. 32");
  if (mode > HUMID_CELLS_MIN_READS) return fail(c, HUMID_E_INVALID, "mode %u is none of HUMID_CELLS_TOP, _EXPECTED, _MIN_READS", mode);
  if (param == 0) return fail(c, HUMID_E_INVALID, "the mode's parameter must be >= 1");
  if (n_reads && (!key || !filtered)) return fail(c, HUMID_E_INVALID, "null buffer");
  if (n_reads > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "n_reads %llu exceeds 2^31-1", (ull)n_reads);
  return HUMID_OK;
}

// a host wait of the discovery: its counters, and (extra != null) one more device word
static int cd_wait(humid_ctx *c, ull *h, const u32 *extra = nullptr, u32 *h_extra = nullptr) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, c->cd_ctr.p, CD_CTRS * sizeof(ull), hipMemcpyDeviceToHost, c->stream));
  if (extra) HIPCHK(hipMemcpyAsync(h_extra, extra, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

template <class K, class V>
static int cd_sort(humid_ctx *c, const K *kin, K *kout, const V *vin, V *vout, u64 n, u32 bits) {
  PASS_ENSURE(c->cd_tmp, (rs_temp_bytes<K, V, true>(n)));
  HIPCHK((rs_sort<K, V, true>(c->cd_tmp.p, PtrIn<K>{kin}, kout, PtrIn<V>{vin}, vout, n, 0, bits, c->stream)));
  return HUMID_OK;
}

// pos[0 .. n] = the exclusive scan of flag[0 .. n] (n + 1 entries, the last a sentinel): pos[n] is the total
static int cd_scan(humid_ctx *c, const u32 *flag, u32 *pos, u64 n) {
  PASS_ENSURE(c->cd_tmp, ps_scan_scratch_items(n + 1) * 4 + 256);
  HIPCHK((ps_exscan<u32>(PtrIn<u32>{flag}, pos, n + 1, (u32 *)c->cd_tmp.p, c->stream, c->no_chain ? nullptr : c->ps_chain, &c->ps_epoch)));
  return HUMID_OK;
}

// Option "kernel_timing" (HUMID_KERNEL_TIMING): an event behind every stage of the discovery, and one line on stderr
// with the milliseconds between them when the call ends (the host waits lie inside the stage they end)
struct CdMarks {
  bool on;
  hipStream_t st;
  std::vector<std::pair<const char *, hipEvent_t>> ev;
  void mark(const char *name) {
    hipEvent_t e;
    if (!on || hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    ev.push_back({name, e});
  }
  ~CdMarks() {
    if (ev.size() > 1 && hipEventSynchronize(ev.back().second) == hipSuccess) {
      fprintf(stderr, "[humid] whitelist discovery, ms:");
      for (size_t i = 1; i < ev.size(); i++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev[i - 1].second, ev[i].second);
        fprintf(stderr, " %s %.3f", ev[i].first, ms);
      }
      fprintf(stderr, "\n");
    }
    for (auto &e : ev) (void)hipEventDestroy(e.second);
  }
};

static int cells_tail(humid_ctx *c, const u64 *tab, const u32 *cnt, u32 cap_log2, u32 G, u64 n_reads, u32 K, u32 mode, u64 param,
                      u32 ratio, ull *h, CdMarks &marks, humid_cells_summary *sum);

// The whole discovery over device arrays (arguments checked).  Four host waits at most: the distinct barcodes (again
// after every table that was too small), the selection's size with the histogram's, the cells after the merge (only
// with a merge), the installed table.  Nothing of the context changes before the last one succeeded.  The count is
// here, everything behind it in cells_tail, which humid_cells_finish runs over its own table.
static int cells_discover_device(humid_ctx *c, const u64 *d_key, const u8 *d_filt, u64 n_reads, u32 K, u32 mode, u64 param,
                                 u32 ratio, humid_cells_summary *sum) {
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const u32 N = (u32)n_reads;
  const u64 lim = K < 32 ? (u64)1 << (2 * K) : 0ull;
  ull h[CD_CTRS] = {};
  PASS_ENSURE(c->cd_ctr, CD_CTRS * sizeof(ull));
  ull *ctr = c->cd_ctr.as<ull>();
  HIPCHK(hipMemsetAsync(ctr, 0, CD_CTRS * sizeof(ull), st));
  CdMarks marks{c->kev_on, st, {}};
  marks.mark("start");
  u32 G = 0, cap_log2 = 0;
  if (N) {
    u32 full_log2 = 4;                                        // the size that cannot be too small: cap >= 2 N
    while (full_log2 < 32 && ((u64)1 << full_log2) < 2 * (u64)N) full_log2++;
    cap_log2 = c->cd_force_log2 ? c->cd_force_log2 : (c->cd_cap_log2 ? c->cd_cap_log2 : 16u);
    cap_log2 = std::min(std::max(cap_log2, 4u), full_log2);
    while (true) {
      const u32 cap = 1u << cap_log2;
      const u32 out_cap = std::min<u64>((u64)cap + 1, N);       // (every distinct barcode is some read's key)
      PASS_ENSURE(c->cd_table, ((size_t)cap + 1) * 8);
      PASS_ENSURE(c->cd_cnt, ((size_t)cap + 1) * 4);
      PASS_ENSURE(c->cd_k0, (size_t)out_cap * 8 + 16);
      PASS_ENSURE(c->cd_c0, (size_t)out_cap * 4 + 16);
      HIPCHK(hipMemsetAsync(c->cd_table.p, 0xff, ((size_t)cap + 1) * 8, st));
      HIPCHK(hipMemsetAsync(c->cd_cnt.p, 0, ((size_t)cap + 1) * 4, st));
      HIPCHK(hipMemsetAsync(ctr, 0, CD_CTRS * sizeof(ull), st));
      hipLaunchKernelGGL(k_cd_count, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_key, d_filt, N, c->cd_table.as<u64>(), c->cd_cnt.as<u32>(),
                         cap_log2, cap_log2 == full_log2 ? cap : 128u, lim, ctr);
      marks.mark("memset+k_cd_count");
      hipLaunchKernelGGL(k_cd_compact, dim3(std::min<u32>(COMPACT_BLOCKS, blocks_for((u64)cap + 1))), dim3(256), 0, st,
                         (const u64 *)c->cd_table.p, (const u32 *)c->cd_cnt.p, cap, c->cd_k0.as<u64>(), c->cd_c0.as<u32>(), out_cap, ctr);
      TRY(cd_wait(c, h));                                       // host wait 1
      marks.mark("k_cd_compact+wait");
      if (h[CD_OVERFULL] == 0 && h[CD_G] <= out_cap) break;
      if (cap_log2 >= full_log2) return fail(c, HUMID_E_INVALID, "internal: the barcode table of 2^%u slots overflowed", cap_log2);
      cap_log2 = std::min(cap_log2 + 4, full_log2);
    }
    G = (u32)h[CD_G];
    // the next call starts with a table at most a third full for as many barcodes as this one saw
    u32 next = 12;
    while (next < full_log2 && ((u64)1 << next) < 3 * (u64)G) next++;
    c->cd_cap_log2 = next;
  }
  return cells_tail(c, (const u64 *)c->cd_table.p, (const u32 *)c->cd_cnt.p, cap_log2, G, N, K, mode, param, ratio, h, marks, sum);
}

// The discovery behind the count: tab / cnt (2^cap_log2 slots and the reserved one) hold the reads per barcode, cd_k0 /
// cd_c0 their G occupied slots as k_cd_compact left them, h that wait's counters with the usable and invalid reads.
// n_reads bounds the histogram's bins: the reads that were counted, or any number not below them.
static int cells_tail(humid_ctx *c, const u64 *tab, const u32 *cnt, u32 cap_log2, u32 G, u64 n_reads, u32 K, u32 mode, u64 param,
                      u32 ratio, ull *h, CdMarks &marks, humid_cells_summary *sum) {
  hipStream_t st = c->stream;
  ull *ctr = c->cd_ctr.as<ull>();
  humid_cells_summary s;
  memset(&s, 0, sizeof s);
  s.usable = h[CD_USABLE];
  s.invalid_reads = h[CD_INVALID];
  s.distinct = G;
  // the results are built beside those of the last call, which stay in place until this one is complete
  DBuf cells, cellcnt, hist_n, hist_first, fresh;
  u64 n_cells = 0, n_hist = 0;
  u32 wl_log2 = 0;
  if (G) {
    const u64 *k0 = c->cd_k0.as<u64>();
    const u32 *c0 = c->cd_c0.as<u32>();
    PASS_ENSURE(c->cd_kkey, (size_t)G * 8 + 16);
    PASS_ENSURE(c->cd_kccnt, (size_t)G * 4 + 16);
    PASS_ENSURE(c->cd_flag, ((size_t)G + 1) * 4 + 16);
    PASS_ENSURE(c->cd_pos, ((size_t)G + 1) * 4 + 16);
    // the ORDER: by key ascending, then stable by the complemented count (bits above the largest count's: all 1)
    const u64 bits = h[CD_KEYBITS];
    TRY((cd_sort<u64, u32>(c, k0, c->cd_kkey.as<u64>(), c0, c->cd_kccnt.as<u32>(), G, bits ? 64u - (u32)__builtin_clzll(bits) : 1u)));
    u64 *okey = c->cd_k0.as<u64>();
    u32 *occnt = c->cd_c0.as<u32>();
    TRY((cd_sort<u32, u64>(c, c->cd_kccnt.as<u32>(), occnt, c->cd_kkey.as<u64>(), okey, G, 64u - (u32)__builtin_clzll(h[CD_MAXCNT] | 1ull))));
    // a histogram bin per distinct count: H (H + 1) / 2 <= the reads
    u64 hist_cap = 1;
    while (hist_cap < G && hist_cap * (hist_cap + 1) / 2 <= n_reads) hist_cap++;   // (in 64 bits: hist_cap <= G < 2^32)
    hist_cap = std::min<u64>(hist_cap, G);
    HIPCHK(hist_n.ensure((size_t)hist_cap * 8 + 16));
    HIPCHK(hist_first.ensure((size_t)hist_cap * 4 + 16));
    u32 *flag = c->cd_flag.as<u32>(), *pos = c->cd_pos.as<u32>();
    marks.mark("two_sorts");
    hipLaunchKernelGGL(k_cd_cut, dim3(1), dim3(64), 0, st, (const u64 *)okey, (const u32 *)occnt, G, mode, param, ctr);
    hipLaunchKernelGGL(k_cd_heads, dim3(blocks_for((u64)G + 1)), dim3(256), 0, st, (const u32 *)occnt, G, flag);
    TRY(cd_scan(c, flag, pos, G));
    hipLaunchKernelGGL(k_cd_hist, dim3(blocks_for(G)), dim3(256), 0, st, (const u32 *)occnt, (const u32 *)flag, (const u32 *)pos, G,
                       hist_n.as<u64>(), hist_first.as<u32>(), (u32)hist_cap, ctr);
    hipLaunchKernelGGL(k_cd_members, dim3(blocks_for((u64)G + 1)), dim3(256), 0, st, (const u64 *)c->cd_kkey.p, (const u32 *)c->cd_kccnt.p,
                       G, (const ull *)ctr, flag);
    TRY(cd_scan(c, flag, pos, G));
    TRY(cd_wait(c, h));                                         // host wait 2
    marks.mark("cut+hist+members+wait");
    const u64 sel = h[CD_SEL];
    n_hist = h[CD_NHIST];
    if (n_hist > hist_cap || sel > G) return fail(c, HUMID_E_INVALID, "internal: the selection or the histogram left its bounds");
    s.selected = sel;
    s.threshold_reads = h[CD_CUTCNT];
    s.top_reads = h[CD_TOP];
    if (sel && ratio == 0) {
      if (sel > ((u64)1 << 30)) return fail(c, HUMID_E_OVERFLOW, "a whitelist of %llu barcodes exceeds 2^30", (ull)sel);
      n_cells = sel;
      HIPCHK(cells.ensure((size_t)sel * 8 + 16));
      HIPCHK(cellcnt.ensure((size_t)sel * 4 + 16));
      hipLaunchKernelGGL(k_cd_take, dim3(blocks_for(G)), dim3(256), 0, st, (const u64 *)c->cd_kkey.p, (const u32 *)c->cd_kccnt.p, NONE32,
                         (const u32 *)flag, (const u32 *)pos, G, cells.as<u64>(), cellcnt.as<u32>(), (u32)sel, &ctr[CD_CELLREADS]);
    } else if (sel) {
      const u32 S = (u32)sel;
      PASS_ENSURE(c->cd_skey, (size_t)S * 8 + 16);
      PASS_ENSURE(c->cd_scnt, (size_t)S * 4 + 16);
      hipLaunchKernelGGL(k_cd_take, dim3(blocks_for(G)), dim3(256), 0, st, (const u64 *)c->cd_kkey.p, (const u32 *)c->cd_kccnt.p, NONE32,
                         (const u32 *)flag, (const u32 *)pos, G, c->cd_skey.as<u64>(), c->cd_scnt.as<u32>(), S, (ull *)nullptr);
      // (flag and pos are free again: the decisions and their scan take them, S + 1 <= G + 1 entries)
      if (c->wl_coop)
        hipLaunchKernelGGL(k_cd_merge<true>, dim3(grid_stride_blocks((u64)S * 64)), dim3(256), 0, st, (const u64 *)c->cd_skey.p,
                           (const u32 *)c->cd_scnt.p, S, tab, cnt, cap_log2, 3 * K, ratio, flag);
      else
        hipLaunchKernelGGL(k_cd_merge<false>, dim3(blocks_for(S)), dim3(256), 0, st, (const u64 *)c->cd_skey.p,
                           (const u32 *)c->cd_scnt.p, S, tab, cnt, cap_log2, 3 * K, ratio, flag);
      TRY(cd_scan(c, flag, pos, S));
      u32 kept = 0;
      TRY(cd_wait(c, h, pos + S, &kept));                       // host wait 3
      marks.mark("take+k_cd_merge+wait");
      if (kept > S) return fail(c, HUMID_E_INVALID, "internal: the merge kept more barcodes than it was given");
      if (kept > (1u << 30)) return fail(c, HUMID_E_OVERFLOW, "a whitelist of %u barcodes exceeds 2^30", kept);
      n_cells = kept;
      if (kept) {
        HIPCHK(cells.ensure((size_t)kept * 8 + 16));
        HIPCHK(cellcnt.ensure((size_t)kept * 4 + 16));
        hipLaunchKernelGGL(k_cd_take, dim3(blocks_for(S)), dim3(256), 0, st, (const u64 *)c->cd_skey.p, (const u32 *)c->cd_scnt.p, 0u,
                           (const u32 *)flag, (const u32 *)pos, S, cells.as<u64>(), cellcnt.as<u32>(), kept, &ctr[CD_CELLREADS]);
      }
    }
  }
  u64 distinct = 0;
  if (n_cells) {                                                 // the table, as humid_whitelist_set builds it
    wl_log2 = 1;
    while (((u64)1 << wl_log2) < 2 * n_cells) wl_log2++;
    const size_t cap = (size_t)1 << wl_log2;
    HIPCHK(fresh.ensure((cap + 2) * 8));
    HIPCHK(hipMemsetAsync(fresh.p, 0xff, (cap + 1) * 8, st));
    HIPCHK(hipMemsetAsync(fresh.as<u64>() + cap + 1, 0, 8, st));
    hipLaunchKernelGGL(k_wl_insert, dim3(grid_stride_blocks(n_cells)), dim3(256), 0, st, (const u64 *)cells.p, (u32)n_cells, fresh.as<u64>(),
                       wl_log2);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&distinct, fresh.as<u64>() + cap + 1, 8, hipMemcpyDeviceToHost, st));
  }
  TRY(cd_wait(c, h));                                             // the last host wait
  marks.mark("take+k_wl_insert+wait");
  if (distinct != n_cells) return fail(c, HUMID_E_INVALID, "internal: %llu cells, %llu of them distinct", (ull)n_cells, (ull)distinct);
  s.cells = n_cells;
  s.merged = s.selected - n_cells;
  s.reads_in_cells = h[CD_CELLREADS];
  c->wl_table = std::move(fresh);                                 // (zero cells: an empty buffer, the whitelist is cleared)
  seg_drop(c);
  c->wl_n = n_cells;
  c->wl_nt = n_cells ? K : 0;
  c->wl_log2 = wl_log2;
  wl_counts_drop(c);                                            // (the reads per slot went with the table they index)
  c->cd_cells = std::move(cells);
  c->cd_cellcnt = std::move(cellcnt);
  c->cd_hist_n = std::move(hist_n);
  c->cd_hist_first = std::move(hist_first);
  c->cd_n_cells = n_cells;
  c->cd_n_hist = n_hist;
  c->cd_G = G;
  c->cd_valid = true;
  if (sum) *sum = s;
  return HUMID_OK;
}

// ---- the barcode counter fed in chunks (humid_cells_*; kernels_cells.hip.h) -----------------------------------------
// State and arguments are checked by the entry points.  begin: an empty table of the starting size in the counter's own
// buffers (an earlier counter's memory is kept).
static int cells_accum_begin(humid_ctx *c, u32 K) {
  HIPCHK(hipSetDevice(c->device));
  c->cc_state = CC_NONE;
  const u32 log2 = std::min(std::max(c->cd_force_log2 ? c->cd_force_log2 : 16u, 4u), 31u);
  const size_t cap = (size_t)1 << log2;
  PASS_ENSURE(c->cc_table, (cap + 1) * 8);
  PASS_ENSURE(c->cc_cnt, (cap + 1) * 4);
  PASS_ENSURE(c->cc_ctr, CA_CTRS * sizeof(ull));
  HIPCHK(hipMemsetAsync(c->cc_table.p, 0xff, (cap + 1) * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->cc_cnt.p, 0, (cap + 1) * 4, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->cc_nt = K;
  c->cc_log2 = log2;
  c->cc_grown = 0;
  c->cc_chunks = c->cc_reads = c->cc_usable = c->cc_invalid = c->cc_distinct = 0;
  c->cc_state = CC_ON;
  return HUMID_OK;
}

// the smallest power of two at or above n, as a logarithm, 4 at least (64: beyond 2^63)
static u32 cells_log2_for(u64 n) {
  u32 b = 4;
  while (b < 64 && ((u64)1 << b) < n) b++;
  return b;
}

// The table moves into fresh buffers of 2^new_log2 slots, which replace the old ones once the kernel has been queued
// without error (the stream orders it before whatever reads the new table; the old buffers are freed behind it).
static int cells_accum_grow(humid_ctx *c, u32 new_log2) {
  hipStream_t st = c->stream;
  const u32 cap = 1u << c->cc_log2;
  const size_t ncap = (size_t)1 << new_log2;
  DBuf ntab, ncnt;                                                  // (both free themselves on every early return)
  HIPCHK(ntab.ensure((ncap + 1) * 8));
  HIPCHK(ncnt.ensure((ncap + 1) * 4));
  HIPCHK(hipMemsetAsync(ntab.p, 0xff, (ncap + 1) * 8, st));
  HIPCHK(hipMemsetAsync(ncnt.p, 0, (ncap + 1) * 4, st));
  hipLaunchKernelGGL(k_cd_grow, dim3(grid_stride_blocks((u64)cap + 1)), dim3(256), 0, st, (const u64 *)c->cc_table.p, (const u32 *)c->cc_cnt.p,
                     cap, ntab.as<u64>(), ncnt.as<u32>(), new_log2, c->cc_ctr.as<ull>());
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));                                 // (the old buffers are read until here)
  c->cc_table = std::move(ntab);
  c->cc_cnt = std::move(ncnt);
  c->cc_log2 = new_log2;
  c->cc_grown++;
  return HUMID_OK;
}

// a host wait of an add: its counters
static int cells_accum_wait(humid_ctx *c, ull *h) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, c->cc_ctr.p, CA_CTRS * sizeof(ull), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

// One chunk (1 <= N <= 2^31 - 1).  The first sweep counts every read whose run finds a slot and marks the others
// pending; while reads are pending the table grows -- 16 times the slots, at most to the size that cannot be too small,
// the smallest power of two at or above 2 (distinct + pending), where max_probe is the capacity itself -- and the
// pending reads alone are swept again.  So every usable valid read is counted exactly once.  One host wait per sweep.
static int cells_accum_chunk(humid_ctx *c, const u64 *d_key, const u8 *d_filt, u32 N) {
  hipStream_t st = c->stream;
  const u32 K = c->cc_nt;
  const u64 lim = K < 32 ? (u64)1 << (2 * K) : 0ull;
  ull h[CA_CTRS] = {};
  ull *ctr = c->cc_ctr.as<ull>();
  PASS_ENSURE(c->cc_pend, (size_t)N + 16);
  HIPCHK(hipMemsetAsync(ctr, 0, CA_CTRS * sizeof(ull), st));
  const dim3 grid(grid_stride_blocks(N)), block(256);
  u32 probe = std::min<u32>(128u, 1u << c->cc_log2);
  hipLaunchKernelGGL(k_cd_accum<false>, grid, block, 0, st, d_key, d_filt, N, c->cc_table.as<u64>(), c->cc_cnt.as<u32>(), c->cc_log2, probe, lim,
                     c->cc_pend.as<u8>(), ctr);
  TRY(cells_accum_wait(c, h));
  while (h[CA_PENDING]) {
    const u64 need = 2 * (c->cc_distinct + h[CA_CLAIMED] + h[CA_PENDING]);
    const u32 ceil_log2 = cells_log2_for(need);
    if (ceil_log2 > 31) return fail(c, HUMID_E_OVERFLOW, "a counting table for %llu barcodes exceeds 2^31 slots", (ull)(need / 2));
    if (c->cc_log2 >= ceil_log2) return fail(c, HUMID_E_INVALID, "internal: the barcode table of 2^%u slots overflowed", c->cc_log2);
    const u32 next = std::min(c->cc_log2 + 4, ceil_log2);
    TRY(cells_accum_grow(c, next));
    HIPCHK(hipMemsetAsync(&ctr[CA_PENDING], 0, sizeof(ull), st));
    probe = next == ceil_log2 ? 1u << next : 128u;
    hipLaunchKernelGGL(k_cd_accum<true>, grid, block, 0, st, d_key, d_filt, N, c->cc_table.as<u64>(), c->cc_cnt.as<u32>(), next, probe, lim,
                       c->cc_pend.as<u8>(), ctr);
    TRY(cells_accum_wait(c, h));
    if (h[CA_LOST]) return fail(c, HUMID_E_INVALID, "internal: the growth of the barcode table lost %llu slots", (ull)h[CA_LOST]);
  }
  if (h[CA_OVERFLOW])
    return fail(c, HUMID_E_OVERFLOW, "a barcode's reads exceed 2^31-1: the counter is invalid until humid_cells_begin");
  c->cc_distinct += h[CA_CLAIMED];
  c->cc_usable += h[CA_USABLE];
  c->cc_invalid += h[CA_INVALID];
  // more than half full: later chunks would probe long chains.  At most a quarter full afterwards, 16 times the slots at most.
  if (2 * c->cc_distinct > ((u64)1 << c->cc_log2)) {
    const u32 next = std::min(std::min(c->cc_log2 + 4, cells_log2_for(4 * c->cc_distinct)), 31u);
    if (next > c->cc_log2) {
      TRY(cells_accum_grow(c, next));
      TRY(cells_accum_wait(c, h));
      if (h[CA_LOST]) return fail(c, HUMID_E_INVALID, "internal: the growth of the barcode table lost %llu slots", (ull)h[CA_LOST]);
    }
  }
  return HUMID_OK;
}

// add: after a failure the counter is invalid until the next begin (a chunk may be half counted)
static int cells_accum_add(humid_ctx *c, const u64 *d_key, const u8 *d_filt, u64 n_reads) {
  if (n_reads) {
    const int rc = cells_accum_chunk(c, d_key, d_filt, (u32)n_reads);
    if (rc != HUMID_OK) {
      c->cc_state = CC_INVALID;
      return rc;
    }
  }
  c->cc_chunks++;
  c->cc_reads += n_reads;
  return HUMID_OK;
}

// finish: the occupied slots of the counter's table into the discovery's lists (their number is known: one host wait
// checks it), then the discovery's tail.  The counter is read, not changed.
static int cells_accum_finish(humid_ctx *c, u32 mode, u64 param, u32 ratio, humid_cells_summary *sum) {
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  ull h[CD_CTRS] = {};
  PASS_ENSURE(c->cd_ctr, CD_CTRS * sizeof(ull));
  ull *ctr = c->cd_ctr.as<ull>();
  HIPCHK(hipMemsetAsync(ctr, 0, CD_CTRS * sizeof(ull), st));
  CdMarks marks{c->kev_on, st, {}};
  marks.mark("start");
  const u32 G = (u32)c->cc_distinct;
  if (G) {
    const u32 cap = 1u << c->cc_log2;
    PASS_ENSURE(c->cd_k0, (size_t)G * 8 + 16);
    PASS_ENSURE(c->cd_c0, (size_t)G * 4 + 16);
    hipLaunchKernelGGL(k_cd_compact, dim3(std::min<u32>(COMPACT_BLOCKS, blocks_for((u64)cap + 1))), dim3(256), 0, st,
                       (const u64 *)c->cc_table.p, (const u32 *)c->cc_cnt.p, cap, c->cd_k0.as<u64>(), c->cd_c0.as<u32>(), G, ctr);
    TRY(cd_wait(c, h));
    marks.mark("k_cd_compact+wait");
    if (h[CD_G] != G) return fail(c, HUMID_E_INVALID, "internal: %llu occupied slots for %u barcodes", (ull)h[CD_G], G);
  }
  h[CD_USABLE] = c->cc_usable;
  h[CD_INVALID] = c->cc_invalid;
  return cells_tail(c, (const u64 *)c->cc_table.p, (const u32 *)c->cc_cnt.p, c->cc_log2, G, c->cc_usable, c->cc_nt, mode, param, ratio, h,
                    marks, sum);
}

// ---- strand-symmetric runs (humid_dedup_run_paired*) ------------------------------------------------------------
static int check_paired_args(humid_ctx *c, u32 word_nt) {
  if (word_nt == 0) return fail(c, HUMID_E_INVALID, "word_nt must be >= 1");
  if (word_nt > 64) return fail(c, HUMID_E_UNSUPPORTED, "word_nt %u > 64 is not supported", word_nt);
  if (word_nt & 1u) return fail(c, HUMID_E_INVALID, "a strand-symmetric word has two halves: word_nt %u is odd", word_nt);
  return HUMID_OK;
}

// what a paired run refuses before anything moves, buffers aside (both of its forms: run_host, run_paired_device)
static int check_paired_run_args(humid_ctx *c, u64 n_reads, u32 word_nt, u32 distance, u32 method) {
  TRY(check_paired_args(c, word_nt));
  TRY(check_run_args(c, n_reads, word_nt, method, 64));
  if (c->edit && distance >= 2)
    return fail(c, HUMID_E_UNSUPPORTED, "edit distance %u against a mirrored word is not supported (option edit_distance)", distance);
  return HUMID_OK;
}

// canonical words and strands of device arrays; nothing waits here
template <class WT>
static int pd_canonical_launch(humid_ctx *c, const WT *d_words, const u8 *d_filt, u32 N, u32 word_nt, WT *d_out, u8 *d_strand) {
  if (N == 0) return HUMID_OK;
  hipLaunchKernelGGL(k_pd_canonical<WT>, dim3(blocks_for(N)), dim3(256), 0, c->stream, d_words, d_filt, N, word_nt, d_out, d_strand);
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// The whole paired pass: canonical words and strands into context buffers, run_device over the canonical words with
// the neighbour pairs of paired_edges, then the strand tallies of the clusters and their summary (one host wait).
template <class WT>
static int run_paired_device(humid_ctx *c, const WT *d_words, const u8 *d_filt, u64 n_reads, u32 word_nt, u32 distance,
                             u32 method, u32 *d_cid, u8 *d_keep, humid_summary *sum) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  state_reset(c);
  TRY(check_paired_run_args(c, n_reads, word_nt, distance, method));
  if (n_reads && (!d_words || !d_filt || !d_cid || !d_keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  if (sizeof(WT) == 16 && ((uintptr_t)d_words & 15)) return fail(c, HUMID_E_INVALID, "wide words must be 16-byte aligned on the device");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const u32 N = (u32)n_reads;
  ENSURE(c->pd_words, (size_t)N * sizeof(WT) + 16);
  ENSURE(c->pd_strand, (size_t)N + 16);
  TRY(pd_canonical_launch<WT>(c, d_words, d_filt, N, word_nt, c->pd_words.as<WT>(), c->pd_strand.as<u8>()));
  struct Running { humid_ctx *c; ~Running() { c->pd_run = false; } } running{c};
  c->pd_run = true;
  TRY(run_device<WT>(c, c->pd_words.as<WT>(), d_filt, n_reads, word_nt, distance, method, d_cid, d_keep, sum));
  c->pd_run = false;
  const u32 C = (u32)c->C;
  humid_strand_summary ps;
  memset(&ps, 0, sizeof ps);
  ps.n_clusters = C;
  auto undo = [&](int rc) { state_reset(c); return rc; };      // (a failure here leaves no run behind)
  if (N && C) {
    hipError_t e = c->pd_top.ensure(((size_t)C + 1) * 4, &c->arena);
    if (e == hipSuccess) e = c->pd_bottom.ensure(((size_t)C + 1) * 4, &c->arena);
    if (e == hipSuccess) e = c->pd_ctr.ensure(PD_CTRS * sizeof(ull), &c->arena);
    if (e == hipSuccess) e = hipMemsetAsync(c->pd_top.p, 0, ((size_t)C + 1) * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(c->pd_bottom.p, 0, ((size_t)C + 1) * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(c->pd_ctr.p, 0, PD_CTRS * sizeof(ull), st);
    if (e != hipSuccess) return undo(fail(c, e == hipErrorOutOfMemory ? HUMID_E_NOMEM : HUMID_E_HIP, "strand tally: %s", hipGetErrorString(e)));
    hipLaunchKernelGGL(k_pd_tally, dim3(blocks_for(N)), dim3(256), 0, st, (const u32 *)d_cid, (const u8 *)c->pd_strand.p, N, C,
                       c->pd_top.as<u32>(), c->pd_bottom.as<u32>());
    hipLaunchKernelGGL(k_pd_summary, dim3(grid_stride_blocks(C)), dim3(256), 0, st, (const u32 *)c->pd_top.p,
                       (const u32 *)c->pd_bottom.p, C, c->pd_ctr.as<ull>());
    ull h[PD_CTRS];
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, c->pd_ctr.p, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return undo(fail(c, HUMID_E_HIP, "strand tally: %s", hipGetErrorString(e)));
    ps.duplex = h[PD_DUPLEX]; ps.top_only = h[PD_TOP_ONLY]; ps.bottom_only = h[PD_BOTTOM_ONLY];
    ps.top_reads = h[PD_TOP_READS]; ps.bottom_reads = h[PD_BOTTOM_READS];
  }
  c->pd_sum = ps;
  c->pd_N = n_reads;
  c->state.paired = true;
  return HUMID_OK;
}

#endif  // HUMID_PIPELINE_HIP_H
