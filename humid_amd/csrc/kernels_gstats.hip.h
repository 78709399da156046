// kernels_gstats.hip.h -- per-group statistics of the last single-GPU run (humid_get_group_stats /
// humid_group_stats_device): for every group its leaf range, cluster-id range, reads and neighbour pairs.
// Everything is read where the run left it: the leaves are in (group, word) walk order, so a group is one
// contiguous leaf range; its number sits above the caller's word in the internal word (kernels_gkey.hip.h);
// cluster ids run on across groups, so pos[] (the exclusive scan of the creator flags) at a group's first leaf
// is the number of clusters below the group.
//   k_gs_offsets   one lane per group boundary g in [0, G]: lower bound of g among the leaves' groups
//                  (log2 U probes whatever the group sizes and whatever gap of absent groups lies around g)
//   k_gs_sums      one lane per group: reads and pairs as differences of ONE exclusive scan over the leaves
//                  whose items carry count in the low and degree in the high half (GsPairIn: all counts together
//                  are below 2^31, so the low half never carries into the high one)
// Integers only; no atomics: the results do not depend on the schedule.
#ifndef HUMID_KERNELS_GSTATS_HIP_H
#define HUMID_KERNELS_GSTATS_HIP_H

#include "common.hip.h"

// the group of leaf i: the bits of its internal word above the wb = 2 * word_nt bits of the caller's word
// (only called with a group field: wb <= 62 for one uint64, wb <= 126 for two; the group has at most 32 bits)
__device__ __forceinline__ u32 gs_group(const u64 *__restrict__ w, u32 i, u32 wb) { return (u32)(w[i] >> wb); }
__device__ __forceinline__ u32 gs_group(const W2 *__restrict__ w, u32 i, u32 wb) {
  const u64 hi = w[i].hi;
  if (wb >= 64) return (u32)(hi >> (wb - 64));
  return (u32)((hi << (64 - wb)) | (w[i].lo >> wb));
}

// scan input: count | degree << 32 per leaf
struct GsPairIn {
  const u32 *cnt, *deg;
  __device__ __forceinline__ u64 operator()(u64 i) const { return (u64)cnt[i] | ((u64)deg[i] << 32); }
};

// leaf_off[g] = first walk index whose group is >= g (U behind the last group), cluster_off[g] = clusters of
// the groups below g, for g in [0, G].  gnt == 0: no group field, every leaf is in group 0.
template <class WT>
__global__ void k_gs_offsets(const WT *__restrict__ word, const u32 *__restrict__ pos, u32 U, u32 n_clusters, u32 wb,
                             u32 gnt, u32 G, u32 *__restrict__ leaf_off, u32 *__restrict__ cluster_off) {
  HUMID_GUARD_LAST_VGPR();
  for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g <= G; g += (u64)gridDim.x * blockDim.x) {
    u32 lo = 0, hi = U;
    if (gnt == 0 || g == G) lo = g == 0 ? 0u : U;
    else
      while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (gs_group(word, mid, wb) < (u32)g) lo = mid + 1; else hi = mid;
      }
    leaf_off[g] = lo;
    cluster_off[g] = lo < U ? pos[lo] : n_clusters;
  }
}

// reads[g], edges[g] from the scan ps[U] of (count | degree << 32); behind the last leaf the totals
// (usable reads, 2 * pairs) stand in for ps[U]
static __global__ void k_gs_sums(const u32 *__restrict__ leaf_off, const u64 *__restrict__ ps, u32 U, u64 total, u32 G,
                                 u64 *__restrict__ reads, u32 *__restrict__ edges) {
  HUMID_GUARD_LAST_VGPR();
  for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (u64)gridDim.x * blockDim.x) {
    const u32 a = leaf_off[g], b = leaf_off[g + 1];
    const u64 sa = a < U ? ps[a] : total, sb = b < U ? ps[b] : total;
    reads[g] = (u64)((u32)sb - (u32)sa);
    edges[g] = ((u32)(sb >> 32) - (u32)(sa >> 32)) >> 1;
  }
}

#endif  // HUMID_KERNELS_GSTATS_HIP_H
