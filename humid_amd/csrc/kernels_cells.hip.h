// kernels_cells.hip.h -- the cell-barcode whitelist taken from the data (humid_whitelist_discover*; include/humid_hip.h
// has the definition): the reads per barcode are counted, the abundant barcodes are selected as cells, those that look
// like one-substitution errors of a larger cell are removed, and the rest becomes the context's whitelist.
//   k_cd_count    per read: one probe per run of equal keys inside a wave, the run's length added to the key's count
//   k_cd_accum    the same count into a table that is KEPT (humid_cells_*: a read set fed in chunks): never leaves early, reads
//                 whose key found no slot are marked pending and swept again after k_cd_grow moved the table into a larger one
//   k_cd_compact  occupied slots -> (key, ~count) list, their number, the OR of the keys and the largest count
//   (rs_sort, prims.hip.h, twice: by key, then stable by ~count -- the ORDER of the definition)
//   k_cd_cut      the selection's size and its last member (count, key) from the ORDER; the summary's top and threshold
//   k_cd_heads / k_cd_hist   runs of equal counts in the ORDER -> the barcode-count histogram
//   k_cd_members  key order: which barcodes the selection holds
//   k_cd_take     flagged (key, count) entries -> a dense list in the order they stand in, and the sum of their counts
//   k_cd_merge    one wave per selected barcode: its 3 K variants looked up side by side; is one of them a larger cell?
// Everything after the count is proportional to the number of distinct barcodes.  Part of libhumid_hip.so; device
// code for gfx950 only.
#ifndef HUMID_KERNELS_CELLS_HIP_H
#define HUMID_KERNELS_CELLS_HIP_H

#include "common.hip.h"
#include "kernels_keyrank.hip.h"
#include "kernels_whitelist.hip.h"

// The counting table is two arrays: tab[cap + 1], the keys (a 0xff memset empties them; slots [0, cap) are claimed by a
// compare-and-swap, the barcode that EQUALS EMPTY_KEY -- all-T at K = 32 -- lives in the reserved slot `cap`), and
// cnt[cap + 1], the reads per slot (zero on entry; the reserved slot is occupied exactly when its count is not 0).
// Keys and counts do NOT share a slot: an atomic add executes at the memory side and drops its line from the L2, so a
// count beside its key made every later probe of that key miss the cache -- the first form of this file, 16-byte slots
// of (key, count), spent 1.83 ms in k_cd_count on 10 M shuffled reads where this one spends 1.22 (profiles/cells.md).

// the counters of one discover call (u64 each)
enum { CD_G = 0, CD_USABLE, CD_INVALID, CD_OVERFULL, CD_KEYBITS, CD_MAXCNT, CD_SEL, CD_CUTCNT, CD_CUTKEY, CD_TOP, CD_NHIST,
       CD_CELLREADS, CD_CTRS = 16 };

// ctr[CD_OVERFULL] = 1 when a key found no slot within max_probe steps: the host repeats the count with a larger
// table (the last size, cap >= 2 n_reads, always has room: max_probe is then cap itself).  lim: 4^K, 0 for K = 32; a
// usable read whose key is >= lim is counted in ctr[CD_INVALID] and takes no further part.
static __global__ void __launch_bounds__(256)
k_cd_count(const u64 *__restrict__ key, const u8 *__restrict__ filt, u32 n, u64 *tab, u32 *cnt, u32 cap_log2, u32 max_probe,
           u64 lim, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  const u32 cap = 1u << cap_log2, mask = cap - 1u, lane = threadIdx.x & 63u;
  const u32 n_up = (n + 63u) & ~63u;                               // whole waves stay in the loop: the shuffles need every lane
  u32 n_usable = 0, n_invalid = 0;                                 // (the wave's, kept in every lane)
  for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < n_up; r += gridDim.x * blockDim.x) {
    if (*(volatile ull *)&ctr[CD_OVERFULL]) return;                 // too small already: the pass is repeated anyway
    const bool usable = r < n && filt[r] == 0;
    const u64 k = usable ? key[r] : 0ull;
    const bool valid = usable && (lim == 0ull || k < lim);
    const u64 valid_m = __ballot(valid);
    n_usable += (u32)__popcll(__ballot(usable));
    n_invalid += (u32)__popcll(__ballot(usable && !valid));
    const bool head = kr_run_head(k, valid, lane);
    const u64 heads = __ballot(head);
    if (!head) continue;
    // the run: this head and the valid lanes up to the next head (an invalid lane ends a run: the valid lane behind
    // it is a head)
    const u64 above = lane == 63u ? 0ull : heads & ~((2ull << lane) - 1ull);
    const u64 upto = above ? (above & (0ull - above)) - 1ull : ~0ull;
    const u32 len = (u32)__popcll(valid_m & ~((1ull << lane) - 1ull) & upto);
    u32 s = cap;
    if (k != EMPTY_KEY) {
      s = kr_home(k, cap_log2) & mask;
      u32 probes = 0;
      while (true) {
        u64 t = tab[s];
        if (t == EMPTY_KEY) t = atomicCAS((ull *)&tab[s], EMPTY_KEY, (ull)k);
        if (t == EMPTY_KEY || t == k) break;
        s = (s + 1u) & mask;
        if (++probes > max_probe) { ctr[CD_OVERFULL] = 1; s = NOSLOT; break; }   // never spin forever
      }
    }
    if (s != NOSLOT) atomicAdd(&cnt[s], len);
  }
  if (lane == 0) {
    if (n_usable) atomicAdd(&ctr[CD_USABLE], (ull)n_usable);
    if (n_invalid) atomicAdd(&ctr[CD_INVALID], (ull)n_invalid);
  }
}

// ---- the counter fed in chunks (humid_cells_*): the same table, kept from add to add and grown while it holds counts --
// the counters of one add (u64 each)
enum { CA_USABLE = 0, CA_INVALID, CA_PENDING, CA_CLAIMED, CA_OVERFLOW, CA_LOST, CA_CTRS = 8 };

// the largest count a barcode may reach (the merge's 64-bit product and the posterior's weights rely on it)
#define CD_MAX_COUNT 0x7fffffffu

__device__ __forceinline__ u32 cd_wave_sum(u32 v) {
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) v += (u32)__shfl_xor((int)v, d);
  return v;
}

// k_cd_count for a table that is kept: nothing may be counted twice and nothing dropped, so the kernel never leaves
// early.  A run whose head finds no slot within max_probe steps is PENDING: pend[r] = 1 for its reads (the head hands
// the byte to its run by the shuffle k_wlp_prior hands the slot with) and its length goes to ctr[CA_PENDING]; the host
// grows the table and runs the SWEEP over the pending reads alone, as often as it takes.
//   !SWEEP  every read; pend[r] is written for every r < n; ctr[CA_USABLE] and ctr[CA_INVALID] are raised
//   SWEEP   the reads with pend[r] != 0 (usable, valid keys: the first pass saw to that); pend[r] is rewritten
// ctr[CA_CLAIMED] counts the slots this launch claimed (the compare-and-swap that wins, or the reserved slot's first
// add), ctr[CA_OVERFLOW] = 1 when a count passed CD_MAX_COUNT: the adding lane sees the old value from its atomic.
// A count never wraps: it is at most CD_MAX_COUNT before the add that raises the flag, and an add has n <= 2^31 - 1.
template <bool SWEEP>
__global__ void __launch_bounds__(256)
k_cd_accum(const u64 *__restrict__ key, const u8 *__restrict__ filt, u32 n, u64 *tab, u32 *cnt, u32 cap_log2, u32 max_probe,
           u64 lim, u8 *pend, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  const u32 cap = 1u << cap_log2, mask = cap - 1u, lane = threadIdx.x & 63u;
  const u32 n_up = (n + 63u) & ~63u;                               // whole waves stay in the loop: the shuffles need every lane
  u32 n_usable = 0, n_invalid = 0;                                 // (the wave's, kept in every lane)
  u32 n_pending = 0, n_claimed = 0;                                // (this lane's)
  bool over = false;
  for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < n_up; r += gridDim.x * blockDim.x) {
    bool usable, valid;
    u64 k;
    if (SWEEP) {
      usable = valid = r < n && pend[r] != 0;
      k = valid ? key[r] : 0ull;
    } else {
      usable = r < n && filt[r] == 0;
      k = usable ? key[r] : 0ull;
      valid = usable && (lim == 0ull || k < lim);
      n_usable += (u32)__popcll(__ballot(usable));
      n_invalid += (u32)__popcll(__ballot(usable && !valid));
    }
    const u64 valid_m = __ballot(valid);
    const bool head = kr_run_head(k, valid, lane);
    const u64 heads = __ballot(head);
    u32 left = 0;                                                  // 1: the run found no slot
    if (head) {
      const u64 above = lane == 63u ? 0ull : heads & ~((2ull << lane) - 1ull);
      const u64 upto = above ? (above & (0ull - above)) - 1ull : ~0ull;
      const u32 len = (u32)__popcll(valid_m & ~((1ull << lane) - 1ull) & upto);
      u32 s = cap;
      bool claimed = false;
      if (k != EMPTY_KEY) {
        s = kr_home(k, cap_log2) & mask;
        u32 probes = 0;
        while (true) {
          u64 t = tab[s];
          if (t == EMPTY_KEY) {
            t = atomicCAS((ull *)&tab[s], EMPTY_KEY, (ull)k);
            claimed = t == EMPTY_KEY;
          }
          if (t == EMPTY_KEY || t == k) break;
          s = (s + 1u) & mask;
          if (++probes > max_probe) { s = NOSLOT; break; }         // never spin forever
        }
      }
      if (s != NOSLOT) {
        const u32 old = atomicAdd(&cnt[s], len);
        if (s == cap) claimed = old == 0u;                         // (len >= 1: exactly one add sees the empty reserved slot)
        if ((u64)old + (u64)len > (u64)CD_MAX_COUNT) over = true;
        n_claimed += claimed ? 1u : 0u;
      } else {
        left = 1u;
        n_pending += len;
      }
    }
    const u64 below = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
    const int src = below ? 63 - __clzll((long long)below) : (int)lane;
    left = (u32)__shfl((int)left, src);
    if (r < n && (!SWEEP || valid)) pend[r] = (u8)(valid ? left : 0u);
  }
  n_pending = cd_wave_sum(n_pending);
  n_claimed = cd_wave_sum(n_claimed);
  const bool any_over = __ballot(over) != 0ull;
  if (lane == 0) {
    if (n_usable) atomicAdd(&ctr[CA_USABLE], (ull)n_usable);
    if (n_invalid) atomicAdd(&ctr[CA_INVALID], (ull)n_invalid);
    if (n_pending) atomicAdd(&ctr[CA_PENDING], (ull)n_pending);
    if (n_claimed) atomicAdd(&ctr[CA_CLAIMED], (ull)n_claimed);
    if (any_over) ctr[CA_OVERFLOW] = 1;
  }
}

// Growth: every occupied slot of the old table tab[0, cap) claims a slot of the new key array ntab (0xff-emptied,
// 2^ncap_log2 > cap slots: there is always room, the probe bound is only there so that nothing spins forever) and stores
// its count beside it in ncnt (zeroed); the reserved slot carries over.  The old keys are distinct, so every
// compare-and-swap on an empty slot wins or meets ANOTHER key.  ctr[CA_LOST] counts the slots that found no room (the
// host refuses anything but 0).
static __global__ void __launch_bounds__(256)
k_cd_grow(const u64 *__restrict__ tab, const u32 *__restrict__ cnt, u32 cap, u64 *ntab, u32 *__restrict__ ncnt, u32 ncap_log2,
          ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  const u32 ncap = 1u << ncap_log2, nmask = ncap - 1u;
  for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s <= (u64)cap; s += (u64)gridDim.x * blockDim.x) {
    if (s == (u64)cap) { ncnt[ncap] = cnt[cap]; continue; }
    const u64 k = tab[s];
    if (k == EMPTY_KEY) continue;
    u32 t = kr_home(k, ncap_log2) & nmask, probes = 0;
    while (true) {
      u64 o = ntab[t];
      if (o == EMPTY_KEY) o = atomicCAS((ull *)&ntab[t], EMPTY_KEY, (ull)k);
      if (o == EMPTY_KEY) { ncnt[t] = cnt[s]; break; }
      t = (t + 1u) & nmask;
      if (++probes > ncap) { atomicAdd(&ctr[CA_LOST], 1ull); break; }   // never spin forever
    }
  }
}

__device__ __forceinline__ bool cd_occupied(const u64 *tab, const u32 *cnt, u32 s, u32 cap) {
  return s < cap ? tab[s] != EMPTY_KEY : cnt[s] != 0u;
}

// the slot of k in tab[0, cap], cap being the reserved slot, or NOSLOT
__device__ __forceinline__ u32 cd_find(const u64 *__restrict__ tab, const u32 *__restrict__ cnt, u32 cap_log2, u64 k) {
  const u32 cap = 1u << cap_log2, mask = cap - 1u;
  if (k == EMPTY_KEY) return cnt[cap] != 0u ? cap : NOSLOT;
  u32 s = kr_home(k, cap_log2) & mask;
  for (u32 probes = 0; probes < cap; probes++) {                    // (a free slot ends it long before: never spin forever)
    const u64 t = tab[s];
    if (t == k) return s;
    if (t == EMPTY_KEY) return NOSLOT;
    s = (s + 1u) & mask;
  }
  return NOSLOT;
}

// occupied slots of tab[0 .. cap] -> keys[] / ccnt[] (the COMPLEMENT of the count: ascending ~count is descending
// count) in arbitrary order; k_kr_compact's two passes over a block's chunk.  ctr[CD_G] = the distinct barcodes,
// ctr[CD_KEYBITS] = the OR of all of them, ctr[CD_MAXCNT] = the largest count (the sorts' widths).  Nothing is written
// at or beyond out_cap (the count still runs on: the host refuses it).
static __global__ void __launch_bounds__(256)
k_cd_compact(const u64 *__restrict__ tab, const u32 *__restrict__ cnt, u32 cap, u64 *__restrict__ keys, u32 *__restrict__ ccnt,
             u32 out_cap, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 lds[8];
  const u32 n_slots = cap + 1u;
  const u32 chunk = (n_slots + gridDim.x - 1) / gridDim.x;
  const u32 lo = blockIdx.x * chunk;
  const u32 hi = (lo + chunk < n_slots) ? lo + chunk : n_slots;
  u32 mine = 0;
  for (u32 s = lo + threadIdx.x; s < hi; s += 256) mine += cd_occupied(tab, cnt, s, cap) ? 1u : 0u;
  const u32 total = block_sum(mine, lds);
  if (total == 0) return;                                           // (uniform over the block)
  if (threadIdx.x == 0) lds[4] = (u32)atomicAdd(&ctr[CD_G], (ull)total);
  __syncthreads();
  u32 base = lds[4];
  __syncthreads();
  u64 bits = 0;
  u32 big = 0;
  for (u32 s0 = lo; s0 < hi; s0 += 256) {
    const u32 s = s0 + threadIdx.x;
    const bool occ = s < hi && cd_occupied(tab, cnt, s, cap);
    u32 here;
    const u32 at = base + block_rank(occ, lds, &here);
    if (occ && at < out_cap) {
      const u64 k = s < cap ? tab[s] : EMPTY_KEY;
      const u32 reads = cnt[s];
      keys[at] = k;
      ccnt[at] = ~reads;
      bits |= k;
      big = reads > big ? reads : big;
    }
    base += here;
  }
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) {
    const u32 blo = (u32)__shfl_xor((int)(u32)bits, d), bhi = (u32)__shfl_xor((int)(u32)(bits >> 32), d);
    bits |= ((u64)bhi << 32) | blo;
    const u32 o = (u32)__shfl_xor((int)big, d);
    big = o > big ? o : big;
  }
  if ((threadIdx.x & 63u) == 0 && bits) atomicOr(&ctr[CD_KEYBITS], (ull)bits);
  if ((threadIdx.x & 63u) == 0 && big) atomicMax(&ctr[CD_MAXCNT], (ull)big);
}

// The cut, from the ORDER (okey / occnt: G entries by count descending, key ascending; G >= 1).  One thread:
//   TOP        |S| = min(T, G)
//   EXPECTED   b = min((X + 50) / 100, G - 1), m = n(b); |S| = the ranks r with 10 n(r) >= m
//   MIN_READS  |S| = the ranks r with n(r) >= T
// the last two by a binary search over the descending counts.  S is the ranks [0, |S|): ctr[CD_SEL] = |S|,
// ctr[CD_CUTCNT] / ctr[CD_CUTKEY] = count and key of rank |S| - 1 (a barcode is in S exactly when its (count
// descending, key ascending) is not behind that pair), ctr[CD_TOP] = n(0).
static __global__ void __launch_bounds__(256)
k_cd_cut(const u64 *__restrict__ okey, const u32 *__restrict__ occnt, u32 G, u32 mode, u64 param, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  u64 sel;
  if (mode == HUMID_CELLS_TOP) {
    sel = param < (u64)G ? param : (u64)G;
  } else {
    u64 need, mul;                                                  // rank r is in S when mul * n(r) >= need
    if (mode == HUMID_CELLS_EXPECTED) {
      const u64 b0 = param / 100ull + (param % 100ull + 50ull) / 100ull;   // (X + 50) / 100 without the overflow
      const u32 b = b0 < (u64)(G - 1u) ? (u32)b0 : G - 1u;
      need = (u64)(~occnt[b]);
      mul = 10ull;
    } else {
      need = param;
      mul = 1ull;
    }
    u32 lo = 0, hi = G;                                             // the first rank that is NOT in S
    while (lo < hi) {
      const u32 mid = lo + (hi - lo) / 2u;
      if (mul * (u64)(~occnt[mid]) >= need) lo = mid + 1u; else hi = mid;
    }
    sel = lo;
  }
  ctr[CD_SEL] = sel;
  ctr[CD_CUTCNT] = sel ? (ull)(~occnt[sel - 1]) : 0ull;
  ctr[CD_CUTKEY] = sel ? (ull)okey[sel - 1] : 0ull;
  ctr[CD_TOP] = (ull)(~occnt[0]);
}

// head[i] = 1 where a run of equal counts starts in the ORDER, i < G; head[G] = 0 (the scan's total lands there)
static __global__ void __launch_bounds__(256)
k_cd_heads(const u32 *__restrict__ occnt, u32 G, u32 *__restrict__ head) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > G) return;
  head[i] = (i < G && (i == 0 || occnt[i] != occnt[i - 1])) ? 1u : 0u;
}

// hpos = the exclusive scan of head, H = hpos[G] runs.  The runs stand in DESCENDING count: run j becomes bin H - 1 - j,
// so that the bins ascend.  hist_n[bin] = the count, hist_first[bin] = the rank the run starts at; the barcodes of a
// bin are the distance to the start of the run behind it (the host takes the differences).  ctr[CD_NHIST] = H.
static __global__ void __launch_bounds__(256)
k_cd_hist(const u32 *__restrict__ occnt, const u32 *__restrict__ head, const u32 *__restrict__ hpos, u32 G,
          u64 *__restrict__ hist_n, u32 *__restrict__ hist_first, u32 hist_cap, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G) return;
  const u32 H = hpos[G];
  if (i == 0) ctr[CD_NHIST] = (ull)H;
  if (!head[i]) return;
  const u32 bin = H - 1u - hpos[i];
  if (bin < H && bin < hist_cap) {                                  // (nothing is written at or beyond hist_cap: the host refuses H > hist_cap)
    hist_n[bin] = (u64)(~occnt[i]);
    hist_first[bin] = i;
  }
}

// in[i] of the KEY order (kkey / kccnt, G entries): flag[i] = 1 when barcode i is in S, flag[G] = 0
static __global__ void __launch_bounds__(256)
k_cd_members(const u64 *__restrict__ kkey, const u32 *__restrict__ kccnt, u32 G, const ull *__restrict__ ctr,
             u32 *__restrict__ flag) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > G) return;
  bool in = false;
  if (i < G && ctr[CD_SEL] != 0ull) {
    const u64 cnt = (u64)(~kccnt[i]), cut = ctr[CD_CUTCNT];
    in = cnt > cut || (cnt == cut && kkey[i] <= (u64)ctr[CD_CUTKEY]);
  }
  flag[i] = in ? 1u : 0u;
}

// flagged entries -> kout / cout at pos (the exclusive scan of flag), cnt_xor undoing the complement where the input
// carries one; *reads (may be null) takes the sum of the counts that were taken.  Nothing is written at or beyond
// out_cap.  The grid covers whole waves.
static __global__ void __launch_bounds__(256)
k_cd_take(const u64 *__restrict__ kin, const u32 *__restrict__ cin, u32 cnt_xor, const u32 *__restrict__ flag,
          const u32 *__restrict__ pos, u32 n, u64 *__restrict__ kout, u32 *__restrict__ cout, u32 out_cap, ull *reads) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u64 mine = 0;
  if (i < n && flag[i]) {
    const u32 at = pos[i], cnt = cin[i] ^ cnt_xor;
    if (at < out_cap) {
      kout[at] = kin[i];
      cout[at] = cnt;
      mine = cnt;
    }
  }
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) {
    const u32 lo = (u32)__shfl_xor((int)(u32)mine, d), hi = (u32)__shfl_xor((int)(u32)(mine >> 32), d);
    mine += ((u64)hi << 32) | lo;
  }
  if (reads && (threadIdx.x & 63u) == 0 && mine) atomicAdd(reads, (ull)mine);
}

// does v, which has n_v reads, remove w (n_w reads) of S?  v ranks before w in the ORDER -- S is the ORDER's first
// ranks, so v is then in S as well -- and n_v >= R n_w (R < 2^32, n_w < 2^31: the product stays below 2^63)
__device__ __forceinline__ bool cd_removes(u64 v, u64 n_v, u64 w, u64 n_w, u32 ratio) {
  const bool before = n_v > n_w || (n_v == n_w && v < w);
  return before && n_v >= (u64)ratio * n_w;
}

// The merge over the selected barcodes (skey / scnt, n_sel entries, key order).  keep[i] = 0 when some barcode of S one
// substitution away ranks before barcode i and has at least `ratio` times its reads, else 1; keep[n_sel] = 0.  Every
// decision reads S as selected, none reads another decision.
// COOP: one wave per barcode; lane l looks variant l up in the counting table (a second round when 3 K > 64) and a
// ballot of the lanes that found a larger cell decides.  !COOP (option "whitelist_coop" 0): one lane per barcode walks
// its own 3 K variants.  Whole waves stay inside the loop that ballots.
template <bool COOP>
__global__ void __launch_bounds__(256)
k_cd_merge(const u64 *__restrict__ skey, const u32 *__restrict__ scnt, u32 n_sel, const u64 *__restrict__ tab,
           const u32 *__restrict__ cnt, u32 cap_log2, u32 n_var, u32 ratio, u32 *__restrict__ keep) {
  HUMID_GUARD_LAST_VGPR();
  if (blockIdx.x == 0 && threadIdx.x == 0) keep[n_sel] = 0u;
  if (COOP) {
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (u32 i = wave; i < n_sel; i += n_waves) {                   // (uniform over the wave)
      const u64 w = skey[i], n_w = scnt[i];
      bool any = false;
      for (u32 v0 = 0; v0 < n_var; v0 += 64u) {
        const u32 v = v0 + lane;
        bool hit = false;
        if (v < n_var) {
          const u64 var = wl_variant(w, v);
          const u32 s = cd_find(tab, cnt, cap_log2, var);
          if (s != NOSLOT) hit = cd_removes(var, (u64)cnt[s], w, n_w, ratio);
        }
        const u64 hits = __ballot(hit);
        any = any || hits != 0ull;
      }
      if (lane == 0) keep[i] = any ? 0u : 1u;
    }
  } else {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_sel) return;
    const u64 w = skey[i], n_w = scnt[i];
    bool any = false;
    for (u32 v = 0; v < n_var && !any; v++) {
      const u64 var = wl_variant(w, v);
      const u32 s = cd_find(tab, cnt, cap_log2, var);
      if (s != NOSLOT) any = cd_removes(var, (u64)cnt[s], w, n_w, ratio);
    }
    keep[i] = any ? 0u : 1u;
  }
}

#endif  // HUMID_KERNELS_CELLS_HIP_H
