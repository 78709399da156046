// kernels_best.hip.h -- best-scoring read of every cluster (humid_select_best*, include/humid_hip.h): a pass AFTER
// a run, over that run's per-read (cluster_id, keep) and a caller-defined u32 score per read.  For every cluster the
// candidate with the largest score becomes the representative, ties to the smallest read index; the candidates are
// the reads of the cluster's maxLeaf (scope LEAF: the reads whose word equals the word of the run's representative)
// or all reads of the cluster (scope CLUSTER).
//   k_best_rep    rep[cid] = the run's representative (the one read with keep == 1), by compare-and-swap; checks
//   k_best_vote   best[cid] = max over the candidates of (score << 32 | ~index): one 64-bit atomicMax per run of
//                 equal ids inside a wave that can still raise the slot
//   k_best_write  keep_out / rep_out per read, the number of clusters whose representative changed
// The result is a maximum over a total order: it does not depend on the order of the atomics.
// Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_BEST_HIP_H
#define HUMID_KERNELS_BEST_HIP_H

#include "common.hip.h"

// the pass's four u32 counters
enum { BEST_ERR = 0 /* bit 0: an id above C; bit 1: a cluster with two kept reads */, BEST_CLAIMS /* kept reads that claimed a cluster */,
       BEST_CHANGED /* clusters whose representative changed */, BEST_CTRS = 4 };

__device__ __forceinline__ bool best_same(const u64 *__restrict__ w, u32 a, u32 b) { return w[a] == w[b]; }
__device__ __forceinline__ bool best_same(const W2 *__restrict__ w, u32 a, u32 b) { return w_eq(w[a], w[b]); }

__device__ __forceinline__ u64 best_shfl_up(u64 x, u32 d) {
  const u32 lo = (u32)__shfl_up((int)(u32)x, d), hi = (u32)__shfl_up((int)(u32)(x >> 32), d);
  return ((u64)hi << 32) | lo;
}

// Every kept read of a cluster claims rep[cid] (u32[C + 1], preset to NONE32).  A second claimant and an id above C
// set BEST_ERR; the claims are counted, so a cluster without a kept read shows as claims != C.  Whole waves stay in
// the loop (the ballot needs every lane).
static __global__ void __launch_bounds__(256)
k_best_rep(const u32 *__restrict__ cid, const u8 *__restrict__ keep, u32 n, u32 C, u32 *rep, u32 *ctr) {
  HUMID_GUARD_LAST_VGPR();
  const u32 n_up = (n + 63u) & ~63u;
  u32 claims = 0;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += gridDim.x * blockDim.x) {
    bool claim = false;
    if (i < n) {
      const u32 c = cid[i];
      if (c > C) atomicOr(&ctr[BEST_ERR], 1u);
      else if (c != 0 && keep[i] != 0) {
        claim = true;
        if (atomicCAS(&rep[c], NONE32, i) != NONE32) atomicOr(&ctr[BEST_ERR], 2u);
      }
    }
    claims += (u32)__popcll(__ballot(claim));
  }
  if ((threadIdx.x & 63u) == 0 && claims) atomicAdd(&ctr[BEST_CLAIMS], claims);
}

// One vote per candidate: v = score << 32 | (0xffffffff - i) >= 1, so the largest v is the largest score and, among
// equal scores, the smallest index.  Lanes of a wave that hold a run of equal ids (sorted input makes long runs)
// reduce with a segmented max-scan first and the run's last lane votes for all of them; a plain load of the slot lets
// it skip the atomic when v cannot raise what it saw -- the slot only grows, so a stale value costs a needless atomic,
// never a missed one.  Malformed input (BEST_ERR set or claims != C after k_best_rep) ends the kernel at once: no
// index that was not checked is followed.  The grid covers whole waves; no lane leaves before the last shuffle.
template <class WT, bool LEAF>
__global__ void __launch_bounds__(256)
k_best_vote(const WT *__restrict__ words, const u32 *__restrict__ cid, const u32 *__restrict__ score, u32 n, u32 C,
            const u32 *__restrict__ rep, const u32 *__restrict__ ctr, ull *best) {
  HUMID_GUARD_LAST_VGPR();
  if (ctr[BEST_ERR] != 0 || ctr[BEST_CLAIMS] != C) return;         // (uniform over the grid)
  const u32 lane = threadIdx.x & 63u;
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 c = i < n ? cid[i] : 0u;                                // (c <= C: checked by k_best_rep)
  u64 v = 0;
  if (c != 0) {
    bool cand = true;
    if constexpr (LEAF) {
      const u32 r = rep[c];                                         // (claims == C without a double claim: every slot is set)
      cand = r == i || best_same(words, i, r);
    }
    if (cand) v = ((u64)score[i] << 32) | (u64)(0xffffffffu - i);
  }
  const u32 pc = (u32)__shfl_up((int)c, 1);
  const u64 heads = __ballot(lane == 0 || pc != c);
  const u64 below = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));   // (never 0: lane 0 is a head)
  const u32 first = 63u - (u32)__clzll((long long)below);
#pragma unroll
  for (u32 d = 1; d < 64u; d <<= 1) {
    const u64 o = best_shfl_up(v, d);
    if (lane >= first + d && o > v) v = o;
  }
  const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
  if (tail && v != 0) {
    const u64 seen = __hip_atomic_load(&best[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v > seen) atomicMax(&best[c], (ull)v);
  }
}

// keep_out / rep_out (may be null) per read and BEST_CHANGED, one atomic per workgroup.  Reads nothing of keep, so
// keep_out may be the array k_best_rep read.  Malformed input: nothing is written.
static __global__ void __launch_bounds__(256)
k_best_write(const u32 *__restrict__ cid, u32 n, u32 C, const u32 *__restrict__ rep, const ull *__restrict__ best,
             u8 *keep_out, u32 *__restrict__ rep_out, u32 *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 lds[4];
  if (ctr[BEST_ERR] != 0 || ctr[BEST_CLAIMS] != C) return;         // (uniform over the grid)
  const u32 n_up = (n + 255u) & ~255u;
  u32 changed = 0;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += gridDim.x * blockDim.x) {
    bool moved = false;
    if (i < n) {
      const u32 c = cid[i];
      u32 b = HUMID_NO_READ;
      if (c != 0) {
        b = 0xffffffffu - (u32)best[c];
        moved = b == i && rep[c] != i;
      }
      keep_out[i] = (u8)(b == i);
      if (rep_out) rep_out[i] = b;
    }
    changed += (u32)__popcll(__ballot(moved));
  }
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = changed;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u32 t = lds[0] + lds[1] + lds[2] + lds[3];
    if (t) atomicAdd(&ctr[BEST_CHANGED], t);
  }
}

#endif  // HUMID_KERNELS_BEST_HIP_H
