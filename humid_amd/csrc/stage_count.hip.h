// Stage A of the pass: the exact count of the unique words and their walk order, on every road.
// Included by pipeline.hip.h behind the context, the scans / sorts and the counter reads it uses.
#pragma once

// ---- stage A: exact counts + walk order ------------------------------------------------
// The one writer of humid_ctx::count_left: every road calls it once, when its count is kept (also when that count found
// no unique word), and a count that is discarded or overflowed never does.
static inline void count_publish(humid_ctx *c, CountRoad road, u32 n_parts = 0, bool part_tiled = false, const u32 *cursor2 = nullptr) {
  c->count_left = CountLeft{road, n_parts, part_tiled, cursor2};
}

// the walk-order arrays a count leaves: n words of wsize bytes, and slot, count and first read of each
static int ensure_walk_order(humid_ctx *c, size_t n, size_t wsize) {
  ENSURE(c->s_word, n * wsize);
  ENSURE(c->s_slot, n * 4);
  ENSURE(c->s_cnt, n * 4);
  ENSURE(c->s_first, n * 4);
  return HUMID_OK;
}

// Inserts the reads whose word lies in [range_lo, range_hi] (inclusive; the multi-GPU path
// gives every rank one range, a single GPU takes everything), compacts the table and sorts
// the unique words.  Leaves table/slot_of_read/s_word/s_slot/s_cnt/s_first in the context.
static int stage_count_global(humid_ctx *c, const u64 *d_words, const u8 *d_filt, u32 N, u32 word_nt,
                              u64 range_lo, u64 range_hi, u64 expected_reads, humid_summary &s) {
  hipStream_t st = c->stream;
  if (expected_reads == 0 || expected_reads > N) expected_reads = N;
  u32 cap_log2 = 10;
  while (((u64)1 << cap_log2) < expected_reads + expected_reads / 2) cap_log2++;
  const u64 cap = (u64)1 << cap_log2;
  c->cap_log2 = cap_log2;
  ENSURE(c->table, (cap + 1) * sizeof(Slot));
  ENSURE(c->slot_out, (cap + 1) * 8);
  ENSURE(c->slot_of_read, (size_t)N * 4);
  ENSURE(c->uniq_slot, (size_t)expected_reads * 4 + 4);
  ENSURE(c->uniq_word, (size_t)expected_reads * 8 + 8);
  TRY(mark_frame(c, c->ev[EV_PASS_START]));
  HIPCHK(hipMemsetAsync(c->d_ctr, 0, CTR_N * sizeof(ull), st));
  HIPCHK(hipMemsetAsync(c->table.p, 0xff, (cap + 1) * sizeof(Slot), st));
  TRY(mark_frame(c, c->kev[KEV_INSERT_BEGIN]));
  hipLaunchKernelGGL(k_hash_insert, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_words, d_filt, N,
                     c->table.as<Slot>(), cap_log2, c->slot_of_read.as<u32>(), range_lo, range_hi,
                     (u32)(cap - cap / 8), c->d_ctr);
  TRY(mark_frame(c, c->kev[KEV_INSERT_END]));
  hipLaunchKernelGGL(k_compact_table, dim3(COMPACT_BLOCKS), dim3(256), 0, st,
                     c->table.as<Slot>(), (u32)(cap + 1), c->uniq_word.as<u64>(), c->uniq_slot.as<u32>(),
                     (u32)expected_reads, c->d_ctr);
  HIPCHK(hipGetLastError());
  TRY(read_counters(c));
  if (c->h_ctr[CTR_OVERFULL])
    return fail(c, HUMID_E_INVALID, "hash table over-full: more reads fell into this range than expected_reads");
  count_publish(c, COUNT_GLOBAL);
  const u32 U = (u32)c->h_ctr[CTR_UNIQUE];
  s.usable = c->usable = c->h_ctr[CTR_USABLE];
  s.unique = c->U = U;
  if (U == 0) return mark_stage(c, c->ev[EV_COUNT_END]);
  TRY(ensure_walk_order(c, U, 8));
  TRY(sort_pairs<u64, u32>(c, c->uniq_word.as<u64>(), c->s_word.as<u64>(), c->uniq_slot.as<u32>(),
                           c->s_slot.as<u32>(), U, 0, 2 * word_nt));
  hipLaunchKernelGGL(k_post_sort, dim3(blocks_for(U)), dim3(256), 0, st, c->s_slot.as<u32>(),
                     c->table.as<Slot>(), U, c->s_cnt.as<u32>(), c->s_first.as<u32>());
  TRY(mark_stage(c, c->ev[EV_COUNT_END]));
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// bucket bits of the partitioned count: 2^pb buckets of about PART_TARGET reads
static inline u32 part_bits(u32 N) {
  static const u64 target = getenv("HUMID_PART_TARGET") ? (u64)std::max(32, atoi(getenv("HUMID_PART_TARGET"))) : (u64)PART_TARGET;   // experiments
  u32 pb = 1;
  while (pb < 26 && (target << pb) < (u64)N) pb++;
  return pb;
}

// Ordered partition key = (word - lo) * scale: the value range the reads lie in, stretched over the
// whole 64-bit key space (see PartKeyOp).  shift < 64 iff scale == 2^shift.
struct KeyMap {
  u64 lo, scale;
  u32 shift;
};
static KeyMap key_map(u32 word_nt, u64 lo, u64 hi, bool within) {
  const u64 top = word_nt >= 32 ? ~0ull : (((u64)1 << (2 * word_nt)) - 1);
  if (!within) { lo = 0; hi = top; }
  if (hi > top) hi = top;
  if (lo > hi) { lo = 0; hi = top; }
  KeyMap m;
  m.lo = lo;
  const u64 span = hi - lo;
  if (span == ~0ull) { m.scale = 1; m.shift = 0; return m; }
  const u64 cnt = span + 1;
  if ((cnt & (cnt - 1)) == 0 && cnt > 1) {
    const u32 k = (u32)__builtin_ctzll(cnt);
    m.shift = 64 - k;
    m.scale = (u64)1 << m.shift;
  } else {
    m.shift = 64;
    m.scale = ~0ull / cnt;
  }
  return m;
}

// Room of one padded coarse bin of the tile partitions' first level: the mean fill of the nb1 bins, 1 / pad_div of it
// as head room, and 1024; capped so that nb1 rooms are indexed in 32 bits.
static inline u32 coarse_bin_room(u32 N, u32 nb1) {
  static const u32 pad_div = getenv("HUMID_PAD_DIV") ? (u32)std::max(1, atoi(getenv("HUMID_PAD_DIV"))) : 4u;
  return (u32)std::min<u64>(0xffffffffull / nb1, (u64)N / nb1 + (u64)N / nb1 / pad_div + 1024);
}

// Partitioned variant of stage A (see section 1b of the kernels).  Returns HUMID_OK with
// *overflowed = true when a bucket held more unique words than its LDS table (the caller then
// runs the global-table variant; results are never taken from an overflowed run).
// The count stage's two-level tile partition of the reads `src` yields (kernels_part.hip.h) into pk_keys / pk_vals,
// bucket bounds in pbeg.  SRC: ReadsSrc (one-word words) or WideReadsSrc (the heads of two-word words).
template <class SRC>
static int count_partition(humid_ctx *c, const SRC &src, u32 N, u32 pb, bool *used_padded) {
  hipStream_t st = c->stream;
  const u32 n_parts = 1u << pb;
  // hand-written partition (kernels_part.hip.h): two levels of LDS-staged scatter; excluded reads
  // (filtered, or outside this rank's value range) never enter it
  const u32 d1 = (pb + 1) / 2, d2 = pb - d1;
  const u32 nb1 = 1u << d1;
  // pt_work, in u32: [hist1 512 | cursor1 512 | hist_fine n_parts + 1 | cursor2 n_parts] zeroed, then
  // [cbase 513 | tprefix 513]
  const size_t zero_words = 1024 + (size_t)n_parts + 1 + n_parts;
  ENSURE(c->pt_work, (zero_words + 1026) * 4);
  u32 *hist1 = c->pt_work.as<u32>(), *cursor1 = hist1 + 512, *hist_fine = cursor1 + 512,
      *cursor2 = hist_fine + n_parts + 1, *cbase = cursor2 + n_parts, *tprefix = cbase + 513;
  HIPCHK(hipMemsetAsync(c->pt_work.p, 0, zero_words * 4, st));
  const u32 tiles1 = (N + PT_TILE - 1) / PT_TILE, tiles2 = tiles1 + nb1;
  // Two levels and keys that spread evenly over the coarse bins (hashed keys always do, word-ordered
  // keys were only chosen because their prefix does): level 1 scatters into PADDED coarse bins of a
  // fixed room (mean + 25 % + 1024) and needs no histogram pass over the reads in front; the bins'
  // counts are the cursors it leaves behind.  A bin that outgrows its room (heavily duplicated words:
  // all reads of a word share a bin) is reported, the run discarded, and this context goes back to the
  // histogram form (pt_padded = false).
  const bool padded = d2 > 0 && c->pt_padded;
  const u32 cap1 = padded ? coarse_bin_room(N, nb1) : 0u;
  const size_t room1 = padded ? (size_t)nb1 * cap1 : (size_t)N;
  *used_padded = padded;
  if (padded) {
    ENSURE(c->pad_word, room1 * 8);
    ENSURE(c->pslot, room1 * 4);
  }
  // level-1 output: the final arrays when there is no second level, else scratch that is dead until
  // k_dedup_lds writes it (pad_word, pslot)
  u64 *k1 = d2 ? c->pad_word.as<u64>() : c->pk_keys.as<u64>();
  u32 *v1 = d2 ? c->pslot.as<u32>() : c->pk_vals.as<u32>();
  if (!padded) {
    hipLaunchKernelGGL(k_pt_hist1<SRC>, dim3(tiles1 < 512 ? tiles1 : 512), dim3(1024), 0, st, src, N, d1, hist1);
    hipLaunchKernelGGL(k_pt_scan1, dim3(1), dim3(1024), 0, st, hist1, d1, d2, cbase, tprefix, c->pbeg.as<u32>(),
                       c->ucount.as<u32>() + n_parts, 0u);
  }
  hipLaunchKernelGGL((k_pt_scatter<1, SRC>), dim3(tiles1), dim3(1024), 0, st, src, N, (const u64 *)nullptr,
                     (const u32 *)nullptr, (const u32 *)nullptr, (const u32 *)nullptr, d1, d2, cbase, cursor1, k1, v1,
                     (u32 *)nullptr, cap1, &c->d_ctr[CTR_SPECIAL]);
  if (padded)
    hipLaunchKernelGGL(k_pt_scan1, dim3(1), dim3(1024), 0, st, (const u32 *)cursor1, d1, d2, cbase, tprefix, c->pbeg.as<u32>(),
                       c->ucount.as<u32>() + n_parts, cap1);
  TRY(mark_kernel(c, c->kev[KEV_PART_BEGIN]));
  if (d2) {
    hipLaunchKernelGGL(k_pt_hist2<SRC>, dim3(tiles2), dim3(1024), 0, st, src, k1, tprefix, cbase, d1, d2, hist_fine, cap1);
    hipLaunchKernelGGL((k_pt_scatter<2, SRC>), dim3(tiles2), dim3(1024), 0, st, src, N, k1, v1, tprefix, cbase, d1, d2,
                       hist_fine, cursor2, c->pk_keys.as<u64>(), c->pk_vals.as<u32>(), c->pbeg.as<u32>(), cap1, &c->d_ctr[CTR_SPECIAL]);
  }
  TRY(mark_kernel(c, c->kev[KEV_PART_END]));
  return HUMID_OK;
}

// wide != null (33 <= word_nt <= 64, `ordered` and the tile partition only; d_words unused): buckets are cut
// by the words' heads (WideReadsSrc) and counted by k_dedup_lds_wide (kernels_wide.hip.h).
static int stage_count_lds(humid_ctx *c, const u64 *d_words, const u8 *d_filt, u32 N, u32 word_nt,
                           u64 range_lo, u64 range_hi, const KeyMap &km, bool ordered, humid_summary &s,
                           bool *overflowed, const W2 *wide = nullptr) {
  hipStream_t st = c->stream;
  if (wide && !(ordered && c->use_tile_partition && part_bits(N) <= 18))
    return fail(c, HUMID_E_INVALID, "wide words are counted in word-ordered buckets of the tile partition only");
  const size_t wsize = wide ? sizeof(W2) : 8;
  *overflowed = false;
  const u32 pb = part_bits(N);
  const u32 n_parts = 1u << pb;
  ENSURE(c->pk_keys, (size_t)N * 8);
  ENSURE(c->pk_vals, (size_t)N * 4);
  ENSURE(c->pbeg, (size_t)(n_parts + 1) * 4);
  ENSURE(c->ucount, (size_t)(n_parts + 1) * 4);
  ENSURE(c->pusable, (size_t)(n_parts + 1) * 4);
  ENSURE(c->ubase, (size_t)(n_parts + 1) * 4);
  // pad_word / pslot double as the output of the padded first partition level (below): sized for that at
  // once, so that they are carved from the context's slab a single time
  const size_t room_early = (size_t)N + (size_t)N / 4 + ((size_t)1024 << ((pb + 1) / 2));
  ENSURE(c->pad_word, std::max(room_early * 8, (size_t)N * wsize));
  ENSURE(c->pad_cf, (size_t)N * 8);
  ENSURE(c->pslot, room_early * 4);
  ENSURE(c->slot_out, ((size_t)N + 1) * 8);
  ENSURE(c->uniq_slot, (size_t)N * 4 + 4);
  ENSURE(c->uniq_word, (size_t)N * 8 + 8);
  TRY(mark_frame(c, c->ev[EV_PASS_START]));
  HIPCHK(hipMemsetAsync(c->d_ctr, 0, CTR_N * sizeof(ull), st));
  const bool check_range = !(range_lo == 0 && range_hi == ~0ull);
  const bool tiled = c->use_tile_partition && pb <= 2 * 9;
  bool used_padded = false;
  if (tiled) {
    PtInput in;
    in.words = d_words; in.filtered = d_filt; in.rlo = range_lo; in.rhi = range_hi;
    in.check_range = check_range ? 1u : 0u;
    in.key = PartKeyOp{ordered ? 1u : 0u, km.lo, km.scale};
    if (wide) TRY(count_partition(c, WideReadsSrc{wide, d_filt, 2 * (word_nt - 32), in.key}, N, pb, &used_padded));
    else TRY(count_partition(c, ReadsSrc{in}, N, pb, &used_padded));
  } else {
    // beyond 2^18 buckets (> ~90 M reads): radix passes over the top pb key bits (prims.hip.h)
    ComposeIn<PartKeyOp, PtrIn<u64>> kin{PartKeyOp{ordered ? 1u : 0u, km.lo, km.scale}, PtrIn<u64>{d_words}};
    ComposeIn<ReadTagOp, IotaIn> vin{ReadTagOp{check_range ? d_words : nullptr, d_filt, range_lo, range_hi}, IotaIn{}};
    TRY((sort_pairs_in<u64, u32>(c, kin, c->pk_keys.as<u64>(), vin, c->pk_vals.as<u32>(), N, 64 - pb, 64)));
    hipLaunchKernelGGL(k_part_bounds, dim3(blocks_for(n_parts + 1)), dim3(256), 0, st, c->pk_keys.as<u64>(), N,
                       pb, n_parts, c->pbeg.as<u32>(), c->ucount.as<u32>());
  }
  TRY(mark_frame(c, c->kev[KEV_INSERT_BEGIN]));
  if (wide) {
    auto count = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(n_parts), dim3(256), 0, st, c->pk_keys.as<u64>(), c->pk_vals.as<u32>(), c->pbeg.as<u32>(), wide,
                         2 * (word_nt - 32), N, pb, c->pad_word.as<W2>(), c->pad_cf.as<uint2>(), c->ucount.as<u32>(),
                         c->pusable.as<u32>(), c->pslot.as<u32>(), c->d_ctr);
    };
    count(k_dedup_lds_wide<9, 512, 0, WL_SMALL_LEN>);
    if (N > WL_SMALL_LEN) count(k_dedup_lds_wide<10, 1024, WL_SMALL_LEN, WL_STAGE>);
  } else {
    auto count = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(n_parts), dim3(256), 0, st, c->pk_keys.as<u64>(), c->pk_vals.as<u32>(), c->pbeg.as<u32>(), N, pb,
                         km.lo, km.scale, km.shift, c->pad_word.as<u64>(), c->pad_cf.as<uint2>(), c->ucount.as<u32>(),
                         c->pusable.as<u32>(), c->pslot.as<u32>(), c->d_ctr);
    };
    if (ordered) count(k_dedup_lds<true>);
    else count(k_dedup_lds<false>);
  }
  TRY(mark_frame(c, c->kev[KEV_INSERT_END]));
  hipLaunchKernelGGL(k_part_totals, dim3(n_parts >= 16384 ? 64 : 4), dim3(256), 0, st, c->ucount.as<u32>(),
                     c->pusable.as<u32>(), n_parts, c->d_ctr);
  TRY(exscan_u32(c, c->ucount.as<u32>(), c->ubase.as<u32>(), (u64)n_parts + 1));
  HIPCHK(hipGetLastError());
  TRY(read_counters(c));
  if (used_padded && c->h_ctr[CTR_SPECIAL]) {          // a coarse bin outgrew its padded room: once more, with the histogram pass
    c->pt_padded = false;
    road_taken(c, HUMID_ROAD_PART_PADDED_REDO);
    return stage_count_lds(c, d_words, d_filt, N, word_nt, range_lo, range_hi, km, ordered, s, overflowed, wide);
  }
  if (c->h_ctr[CTR_OVERFULL]) { *overflowed = true; return HUMID_OK; }
  count_publish(c, ordered ? COUNT_LDS_ORDERED : COUNT_LDS_HASHED, n_parts, tiled);
  const u32 U = (u32)c->h_ctr[CTR_UNIQUE];
  s.usable = c->usable = c->h_ctr[CTR_USABLE];
  s.unique = c->U = U;
  if (U == 0) return mark_stage(c, c->ev[EV_COUNT_END]);
  TRY(ensure_walk_order(c, (size_t)U + 1, wsize));
  if (wide) {
    hipLaunchKernelGGL(k_compact_padded_wide, dim3(blocks_for((u64)n_parts * 64)), dim3(256), 0, st,
                       c->pad_word.as<W2>(), c->pad_cf.as<uint2>(), c->pbeg.as<u32>(), c->ucount.as<u32>(),
                       c->ubase.as<u32>(), n_parts, c->s_word.as<W2>(), c->s_slot.as<u32>(),
                       c->s_cnt.as<u32>(), c->s_first.as<u32>());
  } else {
    auto squeeze = [&](auto kernel, u64 *word, u32 *slot, u32 *cnt, u32 *first) {
      hipLaunchKernelGGL(kernel, dim3(blocks_for((u64)n_parts * 64)), dim3(256), 0, st, c->pad_word.as<u64>(), c->pad_cf.as<uint2>(),
                         c->pbeg.as<u32>(), c->ucount.as<u32>(), c->ubase.as<u32>(), n_parts, word, slot, cnt, first);
    };
    if (ordered)     // buckets are runs of the word order and sorted inside: squeezing out the holes IS the sort
      squeeze(k_compact_padded<true>, c->s_word.as<u64>(), c->s_slot.as<u32>(), c->s_cnt.as<u32>(), c->s_first.as<u32>());
    else {
      squeeze(k_compact_padded<false>, c->uniq_word.as<u64>(), c->uniq_slot.as<u32>(), (u32 *)nullptr, (u32 *)nullptr);
      TRY(sort_pairs<u64, u32>(c, c->uniq_word.as<u64>(), c->s_word.as<u64>(), c->uniq_slot.as<u32>(),
                               c->s_slot.as<u32>(), U, 0, 2 * word_nt));
      hipLaunchKernelGGL(k_post_sort_padded, dim3(blocks_for(U)), dim3(256), 0, st, c->s_slot.as<u32>(),
                         c->pad_cf.as<uint2>(), U, c->s_cnt.as<u32>(), c->s_first.as<u32>());
    }
  }
  TRY(mark_stage(c, c->ev[EV_COUNT_END]));
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// ---- the record roads: word-ordered buckets only, both partition levels padded (kernels_part8.hip.h) ----
static RecKey rec_key(const KeyMap &km) {
  RecKey rk;
  rk.lo = km.lo; rk.scale = km.scale;
  rk.pow2 = km.shift < 64 ? 1u : 0u;
  rk.z = rk.pow2 ? km.shift : 63u - (u32)__builtin_clzll(km.scale);
  rk.kbits = 64 - rk.z;
  return rk;
}

// The partition of a record count: 2^pb buckets behind 2^d1 coarse bins with room for cap1 records each.
struct RecShape {
  u32 pb, d1, d2, nb1, n_parts;
  RecKey rk;
  u32 ibits, cap1;
  size_t room1, room2;          // records of level 1, of level 2
};
// false: not this shape -- the options, too few / too many buckets, a read set too large for the tiled un-permute, fewer
// key bits than bucket bits.  index_in_record (one-word words: the record is the key bits below the coarse bin + the
// read index; two-word words carry the index beside the word): the record must also fit 64 bits.
static bool rec_shape(const humid_ctx *c, u32 N, const KeyMap &km, bool index_in_record, RecShape *out) {
  if (!c->use_rec8 || !c->use_tile_partition || !c->pt_padded) return false;
  RecShape sh;
  sh.pb = part_bits(N);
  if (sh.pb < 6 || sh.pb > 18) return false;
  if ((((u64)N + (1u << UW_MAXSHIFT) - 1) >> UW_MAXSHIFT) > UW_MAXBINS) return false;
  sh.rk = rec_key(km);
  sh.ibits = bits_for(N);
  sh.d1 = (sh.pb + 1) / 2;
  if (sh.rk.kbits < sh.pb + 1) return false;
  if (index_in_record) {
    // kbits - d1 + ibits <= 64.  24-nt words over their whole range have 48 key bits: with the balanced split
    // d1 = pb / 2 <= 9 that ends at 2^25 = 33 M reads; one more bit in the FIRST level (1024 coarse bins: half as long
    // runs per bin and tile there) carries the record path to the 67 M reads of the un-permute's bin table (BASELINE
    // configs 3 and 5: 50 M reads)
    while (sh.d1 < 10 && sh.pb - sh.d1 > 1 && sh.rk.kbits - sh.d1 + sh.ibits > 64) sh.d1++;
    if (sh.rk.kbits - sh.d1 + sh.ibits > 64 || sh.pb - sh.d1 > 9 || sh.pb == sh.d1) return false;
  }
  sh.d2 = sh.pb - sh.d1; sh.nb1 = 1u << sh.d1; sh.n_parts = 1u << sh.pb;
  sh.cap1 = coarse_bin_room(N, sh.nb1);
  sh.room1 = (size_t)sh.nb1 * sh.cap1; sh.room2 = (size_t)sh.n_parts << P8_CAP2_LOG;
  *out = sh;
  return true;
}

// The work area of a record count.  p8_status: per bucket (reads << 32 | unique words) and its exclusive scan; entry
// n_parts = the scan's sentinel -> the totals.  p8_cur, in u32: [cursor1 1024 | cursor2 n_parts] zeroed, then
// [cbase 1025 | tprefix 1025].  (Not pt_work: the reads per bucket, cursor2, are read again by the un-permute at the end
// of the pass, and the graph stage's grouping uses pt_work in between.)
struct RecWork {
  u64 *agg, *abase;
  u32 *cursor1, *cursor2, *cbase, *tprefix;
};
// Sizes what both roads have behind their own record buffers -- level 2's positions (p8_b), the padded words of wsize
// bytes and their (count, first read), the slots' results, the buckets' bounds -- carves the work area and launches the
// kernel that zeroes the cursors, the counters and the scan's sentinel, the pass-start frame mark in front of that
// launch; stamp: null, or where it stores the pass's start.
static int rec_work(humid_ctx *c, const RecShape &sh, size_t wsize, u64 *stamp, RecWork *out) {
  hipStream_t st = c->stream;
  ENSURE(c->p8_b, sh.room2 * 8);
  ENSURE(c->pad_word, sh.room2 * wsize);
  ENSURE(c->pad_cf, sh.room2 * 8);
  ENSURE(c->slot_out, (sh.room2 + 1) * 8);
  ENSURE(c->pbeg, (size_t)(sh.n_parts + 1) * 4);
  ENSURE(c->ucount, (size_t)(sh.n_parts + 1) * 4);
  ENSURE(c->p8_status, ((size_t)sh.n_parts + 1) * 16);
  ENSURE(c->p8_cur, ((size_t)PT_MAXBINS1 + sh.n_parts + 2 * (PT_MAXBINS1 + 1)) * 4);
  RecWork w;
  w.agg = c->p8_status.as<u64>(); w.abase = w.agg + sh.n_parts + 1;
  w.cursor1 = c->p8_cur.as<u32>(); w.cursor2 = w.cursor1 + PT_MAXBINS1;
  w.cbase = w.cursor2 + sh.n_parts; w.tprefix = w.cbase + PT_MAXBINS1 + 1;
  TRY(mark_frame(c, c->ev[EV_PASS_START]));
  ZeroList z;
  memset(&z, 0, sizeof z);
  z.p[0] = w.cursor1; z.n[0] = PT_MAXBINS1 + sh.n_parts;
  z.p[1] = (u32 *)c->d_ctr; z.n[1] = 2 * CTR_N;
  z.p[2] = (u32 *)(w.agg + sh.n_parts); z.n[2] = 2;
  hipLaunchKernelGGL(k_zero_many, dim3(32), dim3(256), 0, st, z, stamp);
  *out = w;
  return HUMID_OK;
}

// Behind the count kernels of a record road: the scan of the buckets' aggregates, the squeeze of the padded arrays into
// the walk order (`squeeze` launches the road's kernel; wsize: bytes per word), the host wait, and the verdict.
// The walk-order arrays are squeezed out of the padded ones BEFORE the host knows how many unique words there are (at
// most N: a bucket never reports more words than records it holds).  Everything the host's wait reads -- U and the
// usable reads (the scan's totals), CTR_SPECIAL, CTR_OVERFULL -- is final behind the scan, so with overlap_waits the
// publishing kernel stands IN FRONT of the squeeze: the host sees U, which it needs to shape the graph stage, while the
// squeeze runs, and queues that stage behind it.  (Without the option the publishing kernel follows the squeeze in the
// stream, and the GPU is idle from the squeeze's end until the host has seen U and launched.)
// *done = false: a bin outgrew its room (CTR_SPECIAL) or a bucket its table (CTR_OVERFULL); the count is discarded and
// nothing is published.  own_redo (one-word words): the road behind is stage_count_lds with the exact partition, so a
// full bin ends the padded partition of this context, and the pass's four times are that road's events; the key +
// gather road behind the two-word count decides by itself what to do next.
template <class Squeeze>
static int rec_tail(humid_ctx *c, const RecShape &sh, const RecWork &w, u32 N, size_t wsize, u64 *stamp_k1, bool own_redo,
                    Squeeze squeeze, humid_summary &s, bool *done) {
  hipStream_t st = c->stream;
  TRY(exscan_in<u64>(c, PtrIn<u64>{w.agg}, w.abase, (u64)sh.n_parts + 1, stamp_k1));
  TRY(ensure_walk_order(c, (size_t)N + 1, wsize));
  const u32 *totals = (const u32 *)(w.abase + sh.n_parts);     // U, usable
  const bool early = c->overlap_waits;
  if (early) TRY(read_counters_begin(c, totals, totals + 1));
  squeeze();
  TRY(mark_stage(c, c->ev[EV_COUNT_END]));
  HIPCHK(hipGetLastError());
  if (early) TRY(read_counters_end(c, true));
  else TRY(read_counters(c, totals, totals + 1));
  const u64 special = c->h_ctr[CTR_SPECIAL], overfull = c->h_ctr[CTR_OVERFULL];
  const u32 U = (u32)(c->h_ctr[CTR_N - 1] & 0xffffffffull);
  const u64 usable = c->h_ctr[CTR_N - 2] & 0xffffffffull;
  if (getenv("HUMID_TRACE_COUNT"))
    fprintf(stderr, "[rec count%s] N %u pb %u kbits %u ibits %u cap1 %u special %llu overfull %llu unique %u usable %llu\n",
            wsize == 8 ? "" : ", wide", N, sh.pb, sh.rk.kbits, sh.ibits, sh.cap1, (ull)special, (ull)overfull, U, (ull)usable);
  if (special || overfull) {
    if (own_redo) {
      c->timing.stamp_ok = c->timing.stamp_live = c->timing.stamp_timed = false;
      if (special) { c->pt_padded = false; road_taken(c, HUMID_ROAD_PART_PADDED_REDO); }     // the exact kernels from now on
    }
    return HUMID_OK;
  }
  count_publish(c, COUNT_REC, sh.n_parts, true, w.cursor2);
  s.usable = c->usable = usable;
  s.unique = c->U = U;
  *done = true;
  return HUMID_OK;
}

// Stage A on 8-byte records.  *done = false: not this shape, or the count was discarded -- the caller takes
// stage_count_lds.
static int stage_count_rec(humid_ctx *c, const u64 *d_words, const u8 *d_filt, u32 N, u32 word_nt, u64 range_lo, u64 range_hi,
                           const KeyMap &km, humid_summary &s, bool *done) {
  hipStream_t st = c->stream;
  *done = false;
  RecShape sh;
  if (!rec_shape(c, N, km, true, &sh)) return HUMID_OK;
  const u32 pb = sh.pb, d1 = sh.d1, d2 = sh.d2, nb1 = sh.nb1, n_parts = sh.n_parts, ibits = sh.ibits, cap1 = sh.cap1;
  const RecKey &rk = sh.rk;
  ENSURE(c->p8_a, sh.room1 * 8);
  // the pass's four times from device stamps (humid_ctx::d_stamp)
  const bool stamp = c->timing.stamp_ok;
  u64 *const sp = stamp ? c->d_stamp : nullptr;
  // taken up in front of the first frame mark, which asks stamp_timed (a call that fails in the sizing behind it goes
  // out through the pass's guard, which clears them)
  c->timing.stamp_live = stamp;
  c->timing.stamp_timed = stamp && c->timing.lean;           // no frame mark here, none at the pass's end in stage_map
  RecWork w;
  TRY(rec_work(c, sh, 8, sp ? sp + STAMP_START : (u64 *)nullptr, &w));
  const bool check_range = !(range_lo == 0 && range_hi == ~0ull);
  const Reads8 src{d_words, d_filt, range_lo, range_hi, check_range ? 1u : 0u, rk};
  const u32 tiles1 = (N + PT_TILE - 1) / PT_TILE, tiles2 = tiles1 + nb1;
  hipLaunchKernelGGL((k_p8_scatter1<Reads8, 1024>), dim3(tiles1), dim3(1024), 0, st, src, N, rk.kbits, d1, ibits, cap1, w.cursor1,
                     c->p8_a.as<u64>(), c->d_ctr);
  // static_tiles: level 2 reads the padded bins' cursors itself -- no scan, no tile table (and nothing stores
  // pbeg[n_parts] / ucount[n_parts], which no kernel of the record road reads: its un-permute, k_unperm_bins8, takes
  // the buckets' fills from cursor2).  One workgroup per tile of every bin's ROOM: those beyond the fill leave at once.
  if (c->static_tiles) {
    TRY(mark_kernel(c, c->kev[KEV_PART_BEGIN]));
    hipLaunchKernelGGL(k_p8_scatter2<true>, dim3(nb1 * ((cap1 + PT_TILE - 1) / PT_TILE)), dim3(1024), 0, st, (const u64 *)c->p8_a.as<u64>(),
                       (const u32 *)w.cursor1, (const u32 *)nullptr, rk.kbits, d1, d2, ibits, cap1, w.cursor2, c->p8_b.as<u64>(), c->d_ctr);
  } else {
    hipLaunchKernelGGL(k_pt_scan1, dim3(1), dim3(1024), 0, st, (const u32 *)w.cursor1, d1, d2, w.cbase, w.tprefix, c->pbeg.as<u32>(),
                       c->ucount.as<u32>() + n_parts, cap1);
    TRY(mark_kernel(c, c->kev[KEV_PART_BEGIN]));
    hipLaunchKernelGGL(k_p8_scatter2<false>, dim3(tiles2), dim3(1024), 0, st, (const u64 *)c->p8_a.as<u64>(), (const u32 *)w.tprefix,
                       (const u32 *)w.cbase, rk.kbits, d1, d2, ibits, cap1, w.cursor2, c->p8_b.as<u64>(), c->d_ctr);
  }
  TRY(mark_kernel(c, c->kev[KEV_PART_END]));
  TRY(mark_frame(c, c->kev[KEV_INSERT_BEGIN]));
  hipLaunchKernelGGL(k_dedup_rec, dim3(n_parts), dim3(256), 0, st, c->p8_b.as<u64>(), (const u32 *)w.cursor2, N, pb, d1, ibits, rk,
                     c->pad_word.as<u64>(), c->pad_cf.as<uint2>(), w.agg, c->d_ctr, sp ? sp + STAMP_K0 : (u64 *)nullptr);
  TRY(mark_frame(c, c->kev[KEV_INSERT_END]));
  auto squeeze = [&] {
    hipLaunchKernelGGL(k_compact_padded8, dim3(blocks_for((u64)n_parts * 64)), dim3(256), 0, st, c->pad_word.as<u64>(),
                       c->pad_cf.as<uint2>(), (const u64 *)w.agg, (const u64 *)w.abase, n_parts, c->s_word.as<u64>(),
                       c->s_slot.as<u32>(), c->s_cnt.as<u32>(), c->s_first.as<u32>());
  };
  return rec_tail(c, sh, w, N, 8, sp ? sp + STAMP_K1 : (u64 *)nullptr, true, squeeze, s, done);
}

// Stage A for two-word words on records (kernels_part8.hip.h, second half): the 16-byte word + its read index travel
// through both padded partition levels, k_dedup_wide_rec reads its bucket as two contiguous streams.  No device stamps
// here: the frame marks are always recorded.  *done = false: not this shape, or the count was discarded -- the
// caller takes stage_count_lds (keys + gather) or the sort.
static int stage_count_rec_wide(humid_ctx *c, const W2 *d_words, const u8 *d_filt, u32 N, u32 word_nt, const KeyMap &km,
                                humid_summary &s, bool *done) {
  hipStream_t st = c->stream;
  *done = false;
  RecShape sh;
  if (!rec_shape(c, N, km, false, &sh)) return HUMID_OK;
  const u32 pb = sh.pb, d1 = sh.d1, d2 = sh.d2, nb1 = sh.nb1, n_parts = sh.n_parts, cap1 = sh.cap1;
  const RecKey &rk = sh.rk;
  const u32 hbits = 2 * (word_nt - 32);
  ENSURE(c->pw_a, sh.room1 * 16);
  ENSURE(c->pw_ai, sh.room1 * 4);
  ENSURE(c->pw_b, sh.room2 * 16);
  ENSURE(c->pw_bi, sh.room2 * 4);
  RecWork w;
  TRY(rec_work(c, sh, sizeof(W2), nullptr, &w));
  const u32 tiles1 = (N + PT_TILE - 1) / PT_TILE, tiles2 = tiles1 + nb1;
  hipLaunchKernelGGL(k_pw_scatter<1>, dim3(tiles1), dim3(1024), 0, st, d_words, d_filt, (const u32 *)nullptr, N, hbits, rk,
                     (const u32 *)nullptr, (const u32 *)nullptr, d1, d2, cap1, w.cursor1, c->pw_a.as<W2>(), c->pw_ai.as<u32>(), c->d_ctr);
  hipLaunchKernelGGL(k_pt_scan1, dim3(1), dim3(1024), 0, st, (const u32 *)w.cursor1, d1, d2, w.cbase, w.tprefix, c->pbeg.as<u32>(),
                     c->ucount.as<u32>() + n_parts, cap1);
  TRY(mark_kernel(c, c->kev[KEV_PART_BEGIN]));
  hipLaunchKernelGGL(k_pw_scatter<2>, dim3(tiles2), dim3(1024), 0, st, (const W2 *)c->pw_a.as<W2>(), (const u8 *)nullptr,
                     (const u32 *)c->pw_ai.as<u32>(), N, hbits, rk, (const u32 *)w.tprefix, (const u32 *)w.cbase, d1, d2, cap1, w.cursor2,
                     c->pw_b.as<W2>(), c->pw_bi.as<u32>(), c->d_ctr);
  TRY(mark_kernel(c, c->kev[KEV_PART_END]));
  TRY(mark_frame(c, c->kev[KEV_INSERT_BEGIN]));
  auto count = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(n_parts), dim3(256), 0, st, (const W2 *)c->pw_b.as<W2>(), (const u32 *)c->pw_bi.as<u32>(),
                       (const u32 *)w.cursor2, hbits, rk, N, pb, c->pad_word.as<W2>(), c->pad_cf.as<uint2>(), w.agg, c->p8_b.as<u64>(),
                       c->d_ctr);
  };
  count(k_dedup_wide_rec<9, 512, 0, WL_SMALL_LEN>);
  if (N > WL_SMALL_LEN) count(k_dedup_wide_rec<10, 1024, WL_SMALL_LEN, WL_STAGE>);
  TRY(mark_frame(c, c->kev[KEV_INSERT_END]));
  auto squeeze = [&] {
    hipLaunchKernelGGL(k_compact_padded8_wide, dim3(blocks_for((u64)n_parts * 64)), dim3(256), 0, st, (const W2 *)c->pad_word.as<W2>(),
                       (const uint2 *)c->pad_cf.as<uint2>(), (const u64 *)w.agg, (const u64 *)w.abase, n_parts, c->s_word.as<W2>(),
                       c->s_slot.as<u32>(), c->s_cnt.as<u32>(), c->s_first.as<u32>());
  };
  return rec_tail(c, sh, w, N, sizeof(W2), nullptr, false, squeeze, s, done);
}

// humid_ctx::ordered_memo, the remembered answer of prefix_fits_ordered: does it speak of this shape; make it do so
static inline bool memo_matches(const OrderedMemo &m, u32 N, u32 word_nt, const KeyMap &km) {
  return m.valid && m.n == N && m.nt == word_nt && m.lo == km.lo && m.scale == km.scale;
}
static inline void memo_set(OrderedMemo &m, u32 N, u32 word_nt, const KeyMap &km, bool fits) {
  m = OrderedMemo{true, fits, N, word_nt, km.lo, km.scale};
}

// Would word-ordered buckets fit their LDS tables?  Histogram of the top (up to 12) word bits over
// a sample of the reads, folded / scaled to the 2^pb buckets the partition will use: the fullest
// bucket, with a 1.5x margin, must stay below the table's fill limit (a bucket's unique words
// cannot exceed its reads).  UMI-first layouts pass; read-prefix-first amplicon or low-complexity
// data does not and keeps the hashed buckets.  A wrong "yes" only costs the overflow fallback.
static int prefix_fits_ordered(humid_ctx *c, const u64 *d_words, const u8 *d_filt, u32 N, u32 word_nt,
                               const KeyMap &km, bool *fits) {
  *fits = false;
  // the answer for this shape is remembered: the sample and its host wait are paid once, not per
  // pass (a wrong "yes" on other data of the same shape costs the overflow fallback and resets it)
  if (memo_matches(c->ordered_memo, N, word_nt, km)) {
    *fits = c->ordered_memo.fits;
    return HUMID_OK;
  }
  const u32 bits = 2 * word_nt < 12 ? 2 * word_nt : 12;
  const u32 n_bins = 1u << bits;
  if (N < 65536) return HUMID_OK;                              // small inputs: not worth a decision
  // a sample is enough: the first 512 K reads (FastQ order is unrelated to the word value)
  const u32 n_sample = N < (1u << 19) ? N : (1u << 19);
  ENSURE(c->small, (size_t)n_bins * 4);
  HIPCHK(hipMemsetAsync(c->small.p, 0, (size_t)n_bins * 4, c->stream));
  hipLaunchKernelGGL(k_top_hist, dim3(128), dim3(1024), n_bins * 4, c->stream, d_words, d_filt, n_sample,
                     km.lo, km.scale, bits, c->small.as<u32>());
  std::vector<u32> h(n_bins);
  HIPCHK(hipMemcpyAsync(h.data(), c->small.p, (size_t)n_bins * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  const u32 pb = part_bits(N);
  double worst = 0;
  if (pb >= bits) {                    // several buckets per bin: assume the bin splits evenly
    u32 mx = 0;
    for (u32 v : h) if (v > mx) mx = v;
    worst = (double)mx / (double)(1u << (pb - bits));
  } else {                             // several bins per bucket: fold
    const u32 per = 1u << (bits - pb);
    for (u32 b = 0; b < n_bins; b += per) {
      u64 t = 0;
      for (u32 k = 0; k < per; k++) t += h[b + k];
      if ((double)t > worst) worst = (double)t;
    }
  }
  worst *= (double)N / (double)n_sample;
  *fits = worst * 1.5 <= (double)LDS_FILL_LIMIT;
  memo_set(c->ordered_memo, N, word_nt, km, *fits);
  return HUMID_OK;
}

// stage A dispatcher: partitioned LDS tables when every usable read is counted here (one GPU; a
// multi-GPU rank in exchange mode, `within`: all reads lie in [range_lo, range_hi]), the global
// table for a partial range of a larger array or after a bucket overflow.
static int stage_count(humid_ctx *c, const u64 *d_words, const u8 *d_filt, u32 N, u32 word_nt,
                       u64 range_lo, u64 range_hi, u64 expected_reads, humid_summary &s, bool within = false) {
  const bool full_range = (range_lo == 0 && range_hi == ~0ull);
  if (c->count_mode == 0 && (full_range || within)) {
    const KeyMap km = key_map(word_nt, range_lo, range_hi, within);
    bool overflowed = false;
    bool ordered = c->count_order == 1;
    if (c->count_order < 0) TRY(prefix_fits_ordered(c, d_words, d_filt, N, word_nt, km, &ordered));
    if (ordered) {
      bool done = false;
      TRY(stage_count_rec(c, d_words, d_filt, N, word_nt, range_lo, range_hi, km, s, &done));
      if (done) return HUMID_OK;
      TRY(stage_count_lds(c, d_words, d_filt, N, word_nt, range_lo, range_hi, km, true, s, &overflowed));
      if (!overflowed) return HUMID_OK;
      // these words do not fit word-ordered buckets after all: remember that for this shape
      memo_set(c->ordered_memo, N, word_nt, km, false);
    }
    TRY(stage_count_lds(c, d_words, d_filt, N, word_nt, range_lo, range_hi, km, false, s, &overflowed));
    if (!overflowed) return HUMID_OK;
  }
  return stage_count_global(c, d_words, d_filt, N, word_nt, range_lo, range_hi, expected_reads, s);
}

// ---- the sorting counts (two-word words: kernels_wide.hip.h; long words: kernels_long.hip.h) ----
// Their frame around the key / sort passes, which stay with each road.  Front: the buffers of the sort and of the
// sorted words (word_bytes each), the counters cleared, the frame marks of the pass's start and the sorts' begin.
static int sorted_count_front(humid_ctx *c, u32 N, size_t word_bytes) {
  hipStream_t st = c->stream;
  ENSURE(c->pk_keys, (size_t)N * 8);
  ENSURE(c->pad_word, (size_t)N * 8);
  ENSURE(c->pk_vals, (size_t)N * 4);
  ENSURE(c->uniq_slot, (size_t)N * 4 + 4);
  ENSURE(c->pslot, (size_t)N * 4);
  ENSURE(c->w_sorted, (size_t)N * word_bytes);
  ENSURE(c->w_head, ((size_t)N + 1) * 4);
  ENSURE(c->w_hpos, ((size_t)N + 1) * 4);
  TRY(mark_frame(c, c->ev[EV_PASS_START]));
  HIPCHK(hipMemsetAsync(c->d_ctr, 0, CTR_N * sizeof(ull), st));
  TRY(mark_frame(c, c->kev[KEV_INSERT_BEGIN]));
  return HUMID_OK;
}
// Back, behind the last sort: the frame mark of the sorts' end; `heads` gathers the words in sorted order and flags the first of every run of
// equal words; their scan gives U (one host wait); `unique` writes a leaf per run and the partition-order arrays
// pk_vals / pslot that stage C walks (k_read_map_part); the counts; the stage mark of the count's end.
template <class Heads, class Unique>
static int sorted_count_back(humid_ctx *c, u32 N, size_t word_bytes, Heads heads, Unique unique, humid_summary &s) {
  hipStream_t st = c->stream;
  TRY(mark_frame(c, c->kev[KEV_INSERT_END]));
  heads();
  u64 n_unique = 0;
  TRY(scan_total(c, c->w_head.as<u32>(), c->w_hpos.as<u32>(), N, &n_unique));
  count_publish(c, COUNT_SORTED);
  const u32 U = (u32)n_unique;
  s.usable = c->usable = c->h_ctr[CTR_USABLE];
  s.unique = c->U = U;
  TRY(ensure_walk_order(c, (size_t)U + 1, word_bytes));
  ENSURE(c->w_start, (size_t)(U + 2) * 4);
  ENSURE(c->slot_out, (size_t)(U + 1) * 8);
  unique();
  if (U)
    hipLaunchKernelGGL(k_wide_counts, dim3(blocks_for(U)), dim3(256), 0, st, c->w_start.as<u32>(), U,
                       c->s_cnt.as<u32>(), c->s_slot.as<u32>());
  TRY(mark_stage(c, c->ev[EV_COUNT_END]));
  HIPCHK(hipGetLastError());
  return HUMID_OK;
}

// Stage A for wide words (two uint64 per read): counts by sorting, see kernels_wide.hip.h.
// Leaves s_word (W2)/s_cnt/s_first/s_slot and, for stage C, the partition-order arrays
// pk_vals/pslot in the context.
// head_lo / head_hi (within): every word's head lies in that range (a rank's value range in the exchange pass).
static int stage_count_wide(humid_ctx *c, const W2 *d_words, const u8 *d_filt, u32 N, u32 word_nt, humid_summary &s,
                            u64 head_lo = 0, u64 head_hi = ~0ull, bool within = false) {
  hipStream_t st = c->stream;
  // LDS tables over head-ordered buckets when the heads spread evenly (count_mode 0, as for one-word
  // words; count_order 0 keeps the sort); the sort below otherwise and after an overflow
  if (c->count_mode == 0 && c->count_order != 0 && c->use_tile_partition && (N >= 65536 || c->count_order == 1) &&
      part_bits(N) <= 18) {
    const KeyMap km = key_map(24, head_lo >> WIDE_KEY_DROP, head_hi >> WIDE_KEY_DROP, within);   // (the keys: 48-bit numbers, see WideReadsSrc)
    bool ordered = c->count_order == 1;
    if (c->count_order < 0) {
      // the decision samples the first 512 K reads (and is remembered for the shape): heads of those only;
      // the partition itself computes a word's head as it reads the word (WideReadsSrc)
      const u32 n_sample = N < (1u << 19) ? N : (1u << 19);
      ENSURE(c->w_heads, (size_t)n_sample * 8);
      hipLaunchKernelGGL(k_wide_head64, dim3(blocks_for(n_sample)), dim3(256), 0, st, d_words, n_sample, 2 * (word_nt - 32), c->w_heads.as<u64>(),
                         WIDE_KEY_DROP);
      TRY(prefix_fits_ordered(c, c->w_heads.as<u64>(), d_filt, N, word_nt, km, &ordered));
    }
    if (getenv("HUMID_TRACE_COUNT")) fprintf(stderr, "[wide count] N %u order %d fits %d lo %llx scale %llx shift %u\n", N, c->count_order, (int)ordered, (ull)km.lo, (ull)km.scale, km.shift);
    if (ordered) {
      bool done8 = false;
      TRY(stage_count_rec_wide(c, d_words, d_filt, N, word_nt, km, s, &done8));
      if (done8) return HUMID_OK;
      bool overflowed = false;
      TRY(stage_count_lds(c, nullptr, d_filt, N, word_nt, 0ull, ~0ull, km, true, s, &overflowed, d_words));
      if (getenv("HUMID_TRACE_COUNT")) fprintf(stderr, "[wide count] overflowed %d special %llu overfull %llu\n", (int)overflowed, (ull)c->h_ctr[CTR_SPECIAL], (ull)c->h_ctr[CTR_OVERFULL]);
      if (!overflowed) return HUMID_OK;
      memo_set(c->ordered_memo, N, word_nt, km, false);
    }
  }
  const u32 hbits = 2 * (word_nt - 32);
  const u32 grid = grid_stride_blocks(N);
  TRY(sorted_count_front(c, N, sizeof(W2)));
  u64 *k0 = c->pk_keys.as<u64>(), *k1 = c->pad_word.as<u64>();
  u32 *va = c->uniq_slot.as<u32>(), *vb = c->pk_vals.as<u32>();
  hipLaunchKernelGGL(k_wide_keys_lo, dim3(grid), dim3(256), 0, st, d_words, d_filt, N, k0, va, c->d_ctr);
  TRY(sort_pairs<u64, u32>(c, k0, k1, va, vb, N, 0, 64));                       // by lo
  hipLaunchKernelGGL(k_wide_keys_hi, dim3(grid), dim3(256), 0, st, d_words, d_filt, vb, N, hbits, k0);
  TRY(sort_pairs<u64, u32>(c, k0, k1, vb, va, N, 0, hbits < 64 ? hbits + 1 : 64));   // by (filtered,) hi
  u32 *v = va;
  if (hbits == 64) {                                                            // n = 64: no spare key bit
    hipLaunchKernelGGL(k_wide_keys_flag, dim3(grid), dim3(256), 0, st, d_filt, va, N, (u32 *)k0);
    TRY(sort_pairs<u32, u32>(c, (u32 *)k0, (u32 *)k1, va, vb, N, 0, 1));
    v = vb;
  }
  auto heads = [&] {
    hipLaunchKernelGGL(k_wide_gather, dim3(grid), dim3(256), 0, st, d_words, v, N, hbits, c->w_sorted.as<W2>());
    hipLaunchKernelGGL(k_wide_heads, dim3(grid), dim3(256), 0, st, c->w_sorted.as<W2>(), N, c->d_ctr,
                       c->w_head.as<u32>());
  };
  auto unique = [&] {
    hipLaunchKernelGGL(k_wide_unique, dim3(grid), dim3(256), 0, st, c->w_sorted.as<W2>(), v, c->w_head.as<u32>(),
                       c->w_hpos.as<u32>(), N, c->d_ctr, c->s_word.as<W2>(), c->s_first.as<u32>(),
                       c->w_start.as<u32>(), c->pslot.as<u32>(), c->pk_vals.as<u32>());
  };
  return sorted_count_back(c, N, sizeof(W2), heads, unique, s);
}

// ---- long words (humid_dedup_run_long*, kernels_long.hip.h): k = ceil(word_nt / 32) uint64 per read ----------------
// Stage A: the sorting count of stage_count_wide for k words.  Leaves s_word (k per leaf) / s_cnt / s_first / s_slot
// and, for stage C, the partition-order arrays pk_vals / pslot; count_mode_used is 3.
static int stage_count_long(humid_ctx *c, const u64 *d_words, const u8 *d_filt, u32 N, u32 word_nt, humid_summary &s) {
  hipStream_t st = c->stream;
  const u32 k = (word_nt + 31) / 32, hbits = 2 * (word_nt - 32 * (k - 1));
  const u32 grid = grid_stride_blocks(N);
  TRY(sorted_count_front(c, N, (size_t)k * 8));
  u64 *k0 = c->pk_keys.as<u64>(), *k1 = c->pad_word.as<u64>();
  u32 *v = c->uniq_slot.as<u32>(), *v_other = c->pk_vals.as<u32>();   // v: the order so far
  for (u32 pass = 0; pass < k; pass++) {                               // least significant uint64 first
    const u32 j = k - 1 - pass;
    hipLaunchKernelGGL(k_long_keys, dim3(grid), dim3(256), 0, st, d_words, d_filt, pass ? (const u32 *)v : (const u32 *)nullptr, N, k, j,
                       hbits, k0, v, c->d_ctr);
    TRY(sort_pairs<u64, u32>(c, k0, k1, v, v_other, N, 0, j ? 64 : (hbits < 64 ? hbits + 1 : 64)));   // the head: by (filtered,) head
    std::swap(v, v_other);
  }
  if (hbits == 64) {                                                   // word_nt a multiple of 32: no spare key bit
    hipLaunchKernelGGL(k_wide_keys_flag, dim3(grid), dim3(256), 0, st, d_filt, (const u32 *)v, N, (u32 *)k0);
    TRY(sort_pairs<u32, u32>(c, (u32 *)k0, (u32 *)k1, v, v_other, N, 0, 1));
    std::swap(v, v_other);
  }
  auto heads = [&] {
    u64 *sw = c->w_sorted.as<u64>();
    hipLaunchKernelGGL(k_long_gather, dim3(grid_stride_blocks((u64)N * k)), dim3(256), 0, st, d_words, (const u32 *)v, N, k, hbits, sw);
    hipLaunchKernelGGL(k_long_heads, dim3(grid), dim3(256), 0, st, (const u64 *)sw, N, k, c->d_ctr, c->w_head.as<u32>());
  };
  auto unique = [&] {
    hipLaunchKernelGGL(k_long_unique, dim3(grid), dim3(256), 0, st, (const u64 *)c->w_sorted.as<u64>(), (const u32 *)v, c->w_head.as<u32>(),
                       c->w_hpos.as<u32>(), N, k, c->d_ctr, c->s_word.as<u64>(), c->s_first.as<u32>(), c->w_start.as<u32>(),
                       c->pslot.as<u32>(), c->pk_vals.as<u32>());
  };
  return sorted_count_back(c, N, (size_t)k * 8, heads, unique, s);
}
