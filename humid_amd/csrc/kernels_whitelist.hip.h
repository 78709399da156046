// kernels_whitelist.hip.h -- cell-barcode whitelist correction (humid_whitelist_*, humid_dedup_run_keyed_corrected*):
// a read's key that is no whitelist barcode but has exactly ONE whitelist barcode at Hamming distance 1 (over the
// K nucleotides of a barcode) is replaced by that barcode; a key with two or more such barcodes is ambiguous, one
// with none unmatched (include/humid_hip.h has the table of the five statuses).
//   k_wl_insert   whitelist -> an open-address table of keys in HBM (once per whitelist; duplicates collapse)
//   k_wl_correct  per read: key_out, status, filtered' and the five status counts
// Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_WHITELIST_HIP_H
#define HUMID_KERNELS_WHITELIST_HIP_H

#include "common.hip.h"
#include "kernels_keyrank.hip.h"

// The table: tab[0, cap) holds keys, EMPTY_KEY marks a free slot (a 0xff memset empties it), cap = 2^cap_log2 >=
// 2 n, so at least half of the slots stay free and every linear probe ends at one.  The barcode that EQUALS
// EMPTY_KEY (all-T at K = 32) lives in the reserved slot tab[cap]: 0 = present.  tab[cap + 1] counts the distinct
// barcodes (k_wl_insert).
__device__ __forceinline__ bool wl_has(const u64 *__restrict__ tab, u32 cap_log2, u64 k) {
  const u32 cap = 1u << cap_log2, mask = cap - 1u;
  if (k == EMPTY_KEY) return tab[cap] == 0ull;
  u32 s = kr_home(k, cap_log2) & mask;
  for (u32 probes = 0; probes < cap; probes++) {                    // (a free slot ends it long before: never spin forever)
    const u64 t = tab[s];
    if (t == k) return true;
    if (t == EMPTY_KEY) return false;
    s = (s + 1u) & mask;
  }
  return false;
}

// wl_has that says WHERE: the slot of k in tab[0, cap], cap being the reserved slot, or NOSLOT (kernels_wlpost.hip.h
// keeps a count per slot)
__device__ __forceinline__ u32 wl_find(const u64 *__restrict__ tab, u32 cap_log2, u64 k) {
  const u32 cap = 1u << cap_log2, mask = cap - 1u;
  if (k == EMPTY_KEY) return tab[cap] == 0ull ? cap : NOSLOT;
  u32 s = kr_home(k, cap_log2) & mask;
  for (u32 probes = 0; probes < cap; probes++) {
    const u64 t = tab[s];
    if (t == k) return s;
    if (t == EMPTY_KEY) return NOSLOT;
    s = (s + 1u) & mask;
  }
  return NOSLOT;
}

static __global__ void __launch_bounds__(256)
k_wl_insert(const u64 *__restrict__ bc, u32 n, u64 *tab, u32 cap_log2) {
  HUMID_GUARD_LAST_VGPR();
  const u32 cap = 1u << cap_log2, mask = cap - 1u;
  const u32 n_up = (n + 63u) & ~63u;                               // whole waves stay in the loop: the ballot needs every lane
  u32 fresh_total = 0;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += gridDim.x * blockDim.x) {
    bool fresh = false;
    if (i < n) {
      const u64 k = bc[i];
      if (k == EMPTY_KEY) fresh = atomicExch((ull *)&tab[cap], 0ull) != 0ull;
      else {
        u32 s = kr_home(k, cap_log2) & mask;
        for (u32 probes = 0; probes < cap; probes++) {
          u64 t = tab[s];
          if (t == EMPTY_KEY) {
            t = atomicCAS((ull *)&tab[s], EMPTY_KEY, (ull)k);
            if (t == EMPTY_KEY) { fresh = true; break; }
          }
          if (t == k) break;
          s = (s + 1u) & mask;
        }
      }
    }
    fresh_total += (u32)__popcll(__ballot(fresh));
  }
  if ((threadIdx.x & 63u) == 0 && fresh_total) atomicAdd((ull *)&tab[cap + 1], (ull)fresh_total);
}

// variant v (0 <= v < 3 K) of a key: XOR with 1, 2 or 3 at nucleotide v / 3 gives the three other nucleotides there
__device__ __forceinline__ u64 wl_variant(u64 k, u32 v) { return k ^ ((u64)(1u + v % 3u) << (2u * (v / 3u))); }

__device__ __forceinline__ u64 wl_bcast(u64 x, int src) {
  const u32 lo = (u32)__shfl((int)(u32)x, src), hi = (u32)__shfl((int)(u32)(x >> 32), src);
  return ((u64)hi << 32) | lo;
}

// One pass over the reads.  Every run of equal keys inside a wave costs its head lane one lookup (kr_run_head).
// COOP: the heads that missed are taken in turn: the key is handed to all 64 lanes, lane l looks variant l up (a
// second round when 3 K > 64), a ballot of the hits counts the whitelist barcodes at distance 1 -- the variants are
// distinct keys and the table holds distinct keys -- and with one hit its lane hands the variant back.  A miss costs
// the wave one or two probe latencies instead of up to 96 dependent ones in one lane while 63 idle.
// !COOP: the lane-serial form, every missing head walks its own 3 K variants (measured against COOP: DESIGN 3i);
// the cooperative kernel takes it too for a wave with more missing heads than it has variants to look up.
// key_out / status / filt_out may be null.  counts[5] (u64, by status) is ADDED to: one atomic per workgroup and
// status.  The grid covers whole waves; no lane leaves before the last shuffle.
template <bool COOP>
__global__ void __launch_bounds__(256)
k_wl_correct(const u64 *__restrict__ key, const u8 *__restrict__ filt, u32 n, const u64 *__restrict__ tab, u32 cap_log2,
             u32 n_var, u64 *__restrict__ key_out, u8 *__restrict__ status, u8 *__restrict__ filt_out, ull *counts) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 lds[4][5];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = r < n;
  const bool usable = in && filt[r] == 0;
  const u64 k = usable ? key[r] : 0ull;
  const bool head = kr_run_head(k, usable, lane);
  u64 res = k;
  u32 st = HUMID_BC_UNMATCHED;
  const bool hit = head && wl_has(tab, cap_log2, k);
  if (hit) st = HUMID_BC_EXACT;
  // m missing heads cost the cooperative form m rounds of one probe latency each (twice that when 3 K > 64), the
  // lane-serial form 3 K probes in every missing lane side by side: a wave where nearly every lane misses (random
  // keys) is better off serial (measured: DESIGN 3i, shape c)
  u64 miss = __ballot(head && !hit);
  const bool coop = COOP && (u32)__popcll(miss) * ((n_var + 63u) >> 6) <= n_var;     // (uniform over the wave)
  if (coop) {
    while (miss) {                                                  // (uniform over the wave)
      const int src = __ffsll((long long)miss) - 1;
      miss &= miss - 1ull;
      const u64 kb = wl_bcast(k, src);
      u32 n_hit = 0;
      u64 winner = 0;
      for (u32 v0 = 0; v0 < n_var; v0 += 64u) {
        const u32 v = v0 + lane;
        const u64 var = wl_variant(kb, v < n_var ? v : 0u);
        const u64 hits = __ballot(v < n_var && wl_has(tab, cap_log2, var));
        n_hit += (u32)__popcll(hits);
        if (hits) winner = wl_bcast(var, __ffsll((long long)hits) - 1);
      }
      if ((int)lane == src) {
        if (n_hit == 1) { res = winner; st = HUMID_BC_CORRECTED; }
        else if (n_hit >= 2) st = HUMID_BC_AMBIGUOUS;
      }
    }
  } else if (head && !hit) {
    u32 n_hit = 0;
    u64 winner = 0;
    for (u32 v = 0; v < n_var && n_hit < 2; v++) {
      const u64 var = wl_variant(k, v);
      if (wl_has(tab, cap_log2, var)) { n_hit++; winner = var; }
    }
    if (n_hit == 1) { res = winner; st = HUMID_BC_CORRECTED; }
    else if (n_hit >= 2) st = HUMID_BC_AMBIGUOUS;
  }
  // every lane of a run takes the result of the run's head: the nearest head at or below it
  const u64 heads = __ballot(head);
  const u64 below = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
  const int from = below ? 63 - __clzll((long long)below) : (int)lane;
  res = wl_bcast(res, from);
  st = (u32)__shfl((int)st, from);
  if (!usable) { res = 0; st = HUMID_BC_FILTERED; }
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
  __syncthreads();
  if (threadIdx.x < 5) {
    const u32 c = lds[0][threadIdx.x] + lds[1][threadIdx.x] + lds[2][threadIdx.x] + lds[3][threadIdx.x];
    if (c) atomicAdd(&counts[threadIdx.x], (ull)c);
  }
}

#endif  // HUMID_KERNELS_WHITELIST_HIP_H
