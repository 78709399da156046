// kernels_segments.hip.h -- segmented cell-barcode whitelists (humid_whitelist_set_segments; split-pool and bead
// chemistries: SPLiT-seq, inDrop, BD Rhapsody, sci-RNA-seq): the K-nucleotide key is S segments of L_s <= 10
// nucleotides, every segment with a small list of its own, and every segment is corrected on its own against its list
// (include/humid_hip.h has the definition).  A segment has only 4^L_s <= 2^20 possible values, so the answer for EVERY
// value is worked out once, when the lists are set, into a direct-index table; a read then costs S independent table
// reads and no probing.
//   k_seg_mark    one list -> exact marks, hit counts and winners of the list's one-substitution variants
//   k_seg_finish  counts and winners -> the table's entries, class << 30 | subkey
//   k_seg_resolve per read: key_out, status, filtered', the five status counts and the per-segment summary
// Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_SEGMENTS_HIP_H
#define HUMID_KERNELS_SEGMENTS_HIP_H

#include "common.hip.h"

#define SEG_MAX 8u                  // segments of a whitelist
#define SEG_MAX_NT 10u              // nucleotides of a segment: a table of at most 4^10 entries, 4 MB
// the class of a subkey, the top two bits of its entry: in the order of the statuses, HUMID_BC_EXACT + class
#define SEG_EXACT 0u
#define SEG_CORRECTED 1u
#define SEG_AMBIGUOUS 2u
#define SEG_UNMATCHED 3u
#define SEG_SUB_MASK 0x3fffffffu
// work word of the build, one per entry beside the table: bit 31 = the entry is in the list, below it the number of
// DISTINCT list entries one substitution away (at most 3 L_s = 30)
#define SEG_IN_LIST 0x80000000u
// the summary of a resolve pass (u64 each): seg_counts[SEG_MAX][4] by class, then inexact_hist[SEG_MAX + 1]
#define SEG_SUM_HIST (SEG_MAX * 4u)
#define SEG_SUM_N (SEG_MAX * 4u + SEG_MAX + 1u)

// what the resolve kernel knows of the whitelist (by value: 112 bytes of kernel arguments)
struct SegPlan {
  u32 n_seg, max_inexact, key_nt;
  u32 shift[SEG_MAX];               // bits below segment s in the key
  u32 mask[SEG_MAX];                // 4^L_s - 1
  u32 off[SEG_MAX];                 // first entry of segment s's table
};

// One list.  tab[0, 4^nt) starts as all ones, work[0, 4^nt) as zero.  The first copy of an entry marks it and then
// offers itself to its 3 nt variants: one more hit, and the winner is the SMALLEST neighbour (atomic min), so the
// table depends neither on the order of the list nor on that of the atomics; later copies of the entry do nothing.
// distinct: the number of first copies (one atomic per wave).
static __global__ void __launch_bounds__(256)
k_seg_mark(const u64 *__restrict__ list, u32 n, u32 nt, u32 *tab, u32 *work, ull *distinct) {
  HUMID_GUARD_LAST_VGPR();
  const u32 n_up = (n + 63u) & ~63u;                               // whole waves stay in the loop: the ballot needs every lane
  u32 fresh_total = 0;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += gridDim.x * blockDim.x) {
    bool fresh = false;
    if (i < n) {
      const u32 k = (u32)list[i];                                  // (< 4^nt: the host checked)
      fresh = (atomicOr(&work[k], SEG_IN_LIST) & SEG_IN_LIST) == 0u;
      if (fresh)
        for (u32 v = 0; v < 3u * nt; v++) {
          const u32 var = k ^ ((1u + v % 3u) << (2u * (v / 3u)));
          atomicAdd(&work[var], 1u);
          atomicMin(&tab[var], k);
        }
    }
    fresh_total += (u32)__popcll(__ballot(fresh));
  }
  if ((threadIdx.x & 63u) == 0 && fresh_total) atomicAdd(distinct, (ull)fresh_total);
}

// n = 4^nt entries: an entry of the list is exact whatever lies around it; else one neighbour corrects, two or more
// make it ambiguous, none unmatched.  Only a corrected entry holds another subkey than its own.
static __global__ void __launch_bounds__(256)
k_seg_finish(u32 *tab, const u32 *__restrict__ work, u32 n) {
  HUMID_GUARD_LAST_VGPR();
  for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const u32 w = work[k], hits = w & ~SEG_IN_LIST;
    u32 e;
    if (w & SEG_IN_LIST) e = (SEG_EXACT << 30) | k;
    else if (hits == 1u) e = (SEG_CORRECTED << 30) | (tab[k] & SEG_SUB_MASK);
    else if (hits >= 2u) e = (SEG_AMBIGUOUS << 30) | k;
    else e = (SEG_UNMATCHED << 30) | k;
    tab[k] = e;
  }
}

// One pass over the reads, one lane per read.  The S table reads of a read do not depend on one another: all are issued
// before the first is used, so a read costs one gather latency, not S (the tables of a common chemistry, a few hundred
// KB, stay in L2).  key_out / status / filt_out may be null.  counts[5] (u64, by status) and sum[SEG_SUM_N] are ADDED
// to: every counter is reduced over the wave by a ballot, over the workgroup in LDS, and costs the workgroup one
// atomic where it is not zero.  The grid covers whole waves; no lane leaves before the last ballot.
static __global__ void __launch_bounds__(256)
k_seg_resolve(const u64 *__restrict__ key, const u8 *__restrict__ filt, u32 n, const u32 *__restrict__ tab, const SegPlan p,
              u64 *__restrict__ key_out, u8 *__restrict__ status, u8 *__restrict__ filt_out, ull *counts, ull *sum) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 lds[4][5 + SEG_SUM_N];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = r < n;
  const bool usable = in && filt[r] == 0;
  const u64 k = usable ? key[r] : 0ull;
  const bool valid = usable && (p.key_nt >= 32u || (k >> (2u * p.key_nt)) == 0ull);   // seg_counts / inexact_hist cover these
  u32 e[SEG_MAX];
#pragma unroll
  for (u32 s = 0; s < SEG_MAX; s++)
    e[s] = s < p.n_seg ? tab[p.off[s] + ((u32)(k >> p.shift[s]) & p.mask[s])] : 0u;    // (s >= n_seg: exact, subkey 0)
  u64 res = 0;
  u32 cls = 0, m = 0, worst = 0;                                    // cls: two bits per segment
#pragma unroll
  for (u32 s = 0; s < SEG_MAX; s++) {
    const u32 c = e[s] >> 30;
    cls |= c << (2u * s);
    m += c != 0u;
    worst = c > worst ? c : worst;
    if (s < p.n_seg) res |= (u64)(e[s] & SEG_SUB_MASK) << p.shift[s];
  }
  u32 st = HUMID_BC_FILTERED;
  if (usable) st = (valid && m <= p.max_inexact) ? HUMID_BC_EXACT + worst : HUMID_BC_UNMATCHED;
  if (st >= HUMID_BC_AMBIGUOUS) res = k;
  if (!usable) res = 0;
  if (in) {
    if (key_out) key_out[r] = res;
    if (status) status[r] = (u8)st;
    if (filt_out) filt_out[r] = (u8)(st == HUMID_BC_FILTERED || st >= HUMID_BC_AMBIGUOUS);
  }
#pragma unroll
  for (u32 s = 0; s < 5; s++) {
    const u32 c = (u32)__popcll(__ballot(in && st == s));
    if (lane == 0) lds[wave][s] = c;
  }
  for (u32 s = 0; s < p.n_seg; s++)                                 // (uniform over the grid)
#pragma unroll
    for (u32 c4 = 0; c4 < 4; c4++) {
      const u32 c = (u32)__popcll(__ballot(valid && ((cls >> (2u * s)) & 3u) == c4));
      if (lane == 0) lds[wave][5 + 4 * s + c4] = c;
    }
  for (u32 j = 0; j <= p.n_seg; j++) {
    const u32 c = (u32)__popcll(__ballot(valid && m == j));
    if (lane == 0) lds[wave][5 + SEG_SUM_HIST + j] = c;
  }
  __syncthreads();
  const u32 t = threadIdx.x;
  // counter t of the workgroup: the statuses, then the 4 n_seg class counts, then the n_seg + 1 bins of the histogram
  const bool mine = t < 5u + 4u * p.n_seg || (t >= 5u + SEG_SUM_HIST && t <= 5u + SEG_SUM_HIST + p.n_seg);
  if (mine) {
    const u32 c = lds[0][t] + lds[1][t] + lds[2][t] + lds[3][t];
    if (c) atomicAdd(t < 5u ? &counts[t] : &sum[t - 5u], (ull)c);
  }
}

#endif  // HUMID_KERNELS_SEGMENTS_HIP_H
