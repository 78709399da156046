// kernels_wlpost.hip.h -- barcode correction by quality and abundance (humid_whitelist_correct_posterior*,
// humid_dedup_run_keyed_posterior*; include/humid_hip.h has the definition): a key that is no whitelist barcode is
// replaced by the whitelist barcode w one substitution away whose weight (n_w + 1) * E[q of the differing base] is at
// least min_odds times the weights of all the others together.  n_w, the reads of the call whose key IS w, has to be
// complete before the first decision, so the pass is two launches on the stream:
//   k_wlp_prior    per read: the slot of its key in the whitelist table (or NOSLOT), and the reads per slot
//   k_wlp_decide   per read that missed: its candidates, their weights, the decision; the seven counters
//   k_wlp_counts   caller-given barcodes -> their reads per slot (humid_whitelist_counts)
// The table is probed once per key (prior) and once per variant of a key that missed (decision): no key is looked up
// twice.  Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_WLPOST_HIP_H
#define HUMID_KERNELS_WLPOST_HIP_H

#include "kernels_whitelist.hip.h"

// counts[WLP_CTRS] (u64): reads per status, then the reads with two or more candidates and those of them corrected
enum { WLP_MULTI = 5, WLP_RESCUED = 6, WLP_CTRS = 7 };

// E[q] = floor(2^24 * 10^(-q / 10) + 0.5), q = 0 .. 40: the error probability of a base of Phred quality q in 24
// fractional bits (the table of include/humid_hip.h, held against the formula by tests/test_whitelist_posterior_host.py)
#define WLP_QMAX 40u
static __constant__ u32 WLP_E[WLP_QMAX + 1] = {
    16777216, 13326616, 10585708, 8408526, 6679130, 5305422, 4214246, 3347495, 2659010, 2112126, 1677722,
    1332662,  1058571,  840853,   667913,  530542,  421425,  334749,  265901,  211213,  167772,  133266,
    105857,   84085,    66791,    53054,   42142,   33475,   26590,   21121,   16777,   13327,   10586,
    8409,     6679,     5305,     4214,    3347,    2659,    2112,    1678};

__device__ __forceinline__ u64 wlp_xor64(u64 x, int d) {
  const u32 lo = (u32)__shfl_xor((int)(u32)x, d), hi = (u32)__shfl_xor((int)(u32)(x >> 32), d);
  return ((u64)hi << 32) | lo;
}

// Pass 1.  One lookup per run of equal keys inside a wave; the run's head adds the run's length to its slot's count
// with ONE atomic (a barcode that holds every read costs a wave one atomic, not 64) and hands the slot to the run.
// cnt[cap + 1] is zero on entry.  slot_out[r] = NOSLOT for a read that is filtered or whose key is no barcode.
// The grid covers whole waves; no lane leaves before the last shuffle.
// The prior fed in chunks (humid_whitelist_prior_*) splits the two halves: COUNT && !SLOTS adds a chunk to counts that
// are NOT zero on entry and raises *over when the atomic's old value shows a count beyond WLP_MAX_PRIOR (a count never
// wraps: it is at most WLP_MAX_PRIOR before the add that raises the flag, and a chunk has n <= 2^31 - 1 reads);
// !COUNT && SLOTS is the lookup alone, the decision pass then reads the accumulated counts.
#define WLP_MAX_PRIOR 0x7ffffffeu
template <bool COUNT, bool SLOTS>
__global__ void __launch_bounds__(256)
k_wlp_prior(const u64 *__restrict__ key, const u8 *__restrict__ filt, u32 n, const u64 *__restrict__ tab, u32 cap_log2,
            u32 *cnt, u32 *__restrict__ slot_out, ull *over) {
  HUMID_GUARD_LAST_VGPR();
  const u32 lane = threadIdx.x & 63u;
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = r < n;
  const bool usable = in && filt[r] == 0;
  const u64 k = usable ? key[r] : 0ull;
  const bool head = kr_run_head(k, usable, lane);
  u32 s = NOSLOT;
  if (head) s = wl_find(tab, cap_log2, k);
  // a run: its head and the usable lanes up to the next head (an unusable lane ends a run: the usable lane behind it
  // is a head)
  const u64 heads = __ballot(head), usable_m = __ballot(usable);
  if (COUNT && head && s != NOSLOT) {
    const u64 above = lane == 63u ? 0ull : heads & ~((2ull << lane) - 1ull);
    const u64 upto = above ? (above & (0ull - above)) - 1ull : ~0ull;         // lanes below the next head
    const u64 from = ~((1ull << lane) - 1ull);
    const u32 len = (u32)__popcll(usable_m & from & upto);
    const u32 old = atomicAdd(&cnt[s], len);
    if (over && (u64)old + (u64)len > (u64)WLP_MAX_PRIOR) *over = 1ull;
  }
  if (SLOTS) {
    const u64 below = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
    const int src = below ? 63 - __clzll((long long)below) : (int)lane;
    s = (u32)__shfl((int)s, src);
    if (in) slot_out[r] = usable ? s : NOSLOT;
  }
}

// weight of the candidate in slot s, reached from read r's key through variant v (the nucleotide at bits 2 (v / 3),
// which is nucleotide K - 1 - v / 3 of the barcode): (n_w + 1) * E[q], below 2^32 * 2^24
__device__ __forceinline__ u64 wlp_weight(const u32 *__restrict__ cnt, const u8 *__restrict__ qual, const u32 *e, u32 s, u32 r,
                                          u32 K, u32 v) {
  const u32 b = qual[(size_t)r * K + (K - 1u - v / 3u)];
  u32 p = b < 33u ? 0u : b - 33u;
  p = p > WLP_QMAX ? WLP_QMAX : p;                                   // (min(min(p, 93), 40))
  return ((u64)cnt[s] + 1ull) * (u64)e[p];
}

// best >= min_odds * (total - best) in exact arithmetic: a product beyond 64 bits is larger than any weight
__device__ __forceinline__ bool wlp_wins(u64 best, u64 total, u32 min_odds) {
  const u64 rest = total - best;
  if (__umul64hi((u64)min_odds, rest) != 0ull) return false;
  return best >= (u64)min_odds * rest;
}

// Pass 2.  slot[r] is pass 1's: a hit is EXACT without a probe.  Every read that missed is a query of its own (equal
// keys carry different qualities).  COOP: the missing lanes are taken in turn, key and read index handed to all 64
// lanes, lane l looks variant l up (a second round when 3 K > 64) and on a hit loads the ONE quality byte of the
// source read that belongs to its nucleotide.  One candidate wins whatever it weighs: its lane hands it back.  With
// two or more, a 64-bit sum and a maximum of (weight, smallest barcode) over the wave follow and the source lane
// decides.  !COOP, and a wave with more missing lanes than variants: every missing lane walks its own 3 K variants.
// key_out / status / filt_out may be null.  counts[WLP_CTRS] is ADDED to: one atomic per workgroup and counter.
// The grid covers whole waves; no lane leaves before the last shuffle.
template <bool COOP>
__global__ void __launch_bounds__(256)
k_wlp_decide(const u64 *__restrict__ key, const u8 *__restrict__ filt, const u8 *__restrict__ qual, u32 n,
             const u32 *__restrict__ slot, const u64 *__restrict__ tab, u32 cap_log2, const u32 *__restrict__ cnt, u32 K,
             u32 min_odds, u64 *__restrict__ key_out, u8 *__restrict__ status, u8 *__restrict__ filt_out, ull *counts) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 e[WLP_QMAX + 1];
  __shared__ u32 lds[4][WLP_CTRS];
  if (threadIdx.x <= WLP_QMAX) e[threadIdx.x] = WLP_E[threadIdx.x];
  __syncthreads();
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 n_var = 3u * K;
  const bool in = r < n;
  const bool usable = in && filt[r] == 0;
  const u64 k = usable ? key[r] : 0ull;
  const bool missing = usable && slot[r] == NOSLOT;
  u64 res = k;
  u32 st = missing ? HUMID_BC_UNMATCHED : HUMID_BC_EXACT;
  u32 n_cand = 0;
  u64 miss = __ballot(missing);
  const bool coop = COOP && (u32)__popcll(miss) * ((n_var + 63u) >> 6) <= n_var;     // (uniform over the wave)
  if (coop) {
    while (miss) {                                                  // (uniform over the wave)
      const int src = __ffsll((long long)miss) - 1;
      miss &= miss - 1ull;
      const u64 kb = wl_bcast(k, src);
      const u32 rb = (u32)__shfl((int)r, src);
      u64 total = 0, best_w = 0, best_b = 0;
      u32 nc = 0;
      for (u32 v = lane; v < n_var; v += 64u) {                     // (no collective inside)
        const u64 var = wl_variant(kb, v);
        const u32 s = wl_find(tab, cap_log2, var);
        if (s != NOSLOT) {
          const u64 w = wlp_weight(cnt, qual, e, s, rb, K, v);
          total += w;
          nc++;
          if (w > best_w || (w == best_w && var < best_b)) { best_w = w; best_b = var; }
        }
      }
      const u64 hit_lanes = __ballot(nc >= 1u);
      const u32 cands = (u32)__popcll(hit_lanes) + (u32)__popcll(__ballot(nc >= 2u));      // (uniform over the wave)
      if (cands == 1u) {                                            // the common case: nothing to weigh, its lane hands it back
        best_b = wl_bcast(best_b, __ffsll((long long)hit_lanes) - 1);
        if ((int)lane == src) { n_cand = 1u; res = best_b; st = HUMID_BC_CORRECTED; }
      } else if (cands >= 2u) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
          total += wlp_xor64(total, d);
          const u64 ow = wlp_xor64(best_w, d), ob = wlp_xor64(best_b, d);
          if (ow > best_w || (ow == best_w && ob < best_b)) { best_w = ow; best_b = ob; }
        }
        if ((int)lane == src) {
          n_cand = cands;
          if (wlp_wins(best_w, total, min_odds)) { res = best_b; st = HUMID_BC_CORRECTED; }
          else st = HUMID_BC_AMBIGUOUS;
        }
      }
    }
  } else if (missing) {
    u64 total = 0, best_w = 0, best_b = 0;
    for (u32 v = 0; v < n_var; v++) {
      const u64 var = wl_variant(k, v);
      const u32 s = wl_find(tab, cap_log2, var);
      if (s != NOSLOT) {
        const u64 w = wlp_weight(cnt, qual, e, s, r, K, v);
        total += w;
        n_cand++;
        if (w > best_w || (w == best_w && var < best_b)) { best_w = w; best_b = var; }
      }
    }
    if (n_cand) {
      if (wlp_wins(best_w, total, min_odds)) { res = best_b; st = HUMID_BC_CORRECTED; }
      else st = HUMID_BC_AMBIGUOUS;
    }
  }
  if (!usable) { res = 0; st = HUMID_BC_FILTERED; }
  if (in) {
    if (key_out) key_out[r] = res;
    if (status) status[r] = (u8)st;
    if (filt_out) filt_out[r] = (u8)(st == HUMID_BC_FILTERED || st >= HUMID_BC_AMBIGUOUS);
  }
#pragma unroll
  for (u32 s = 0; s < WLP_CTRS; s++) {
    const bool mine = s < 5u ? st == s : s == WLP_MULTI ? n_cand >= 2u : n_cand >= 2u && st == HUMID_BC_CORRECTED;
    const u32 c = (u32)__popcll(__ballot(in && mine));
    if (lane == 0) lds[wave][s] = c;
  }
  __syncthreads();
  if (threadIdx.x < WLP_CTRS) {
    const u32 c = lds[0][threadIdx.x] + lds[1][threadIdx.x] + lds[2][threadIdx.x] + lds[3][threadIdx.x];
    if (c) atomicAdd(&counts[threadIdx.x], (ull)c);
  }
}

// reads per caller-given barcode: the count of its slot, 0 for a barcode the whitelist does not hold
static __global__ void __launch_bounds__(256)
k_wlp_counts(const u64 *__restrict__ bc, u32 n, const u64 *__restrict__ tab, u32 cap_log2, const u32 *__restrict__ cnt,
             u32 *__restrict__ out) {
  HUMID_GUARD_LAST_VGPR();
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const u32 s = wl_find(tab, cap_log2, bc[i]);
    out[i] = s == NOSLOT ? 0u : cnt[s];
  }
}

#endif  // HUMID_KERNELS_WLPOST_HIP_H
