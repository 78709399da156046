// kernels_optical.hip.h -- optical duplicates per cluster (humid_optical_duplicates*, include/humid_hip.h): a pass
// AFTER a run, over that run's per-read (cluster_id, keep) and a position (tile, x, y) per read.  Two members of a
// cluster are close when they lie on the same tile (not HUMID_NO_TILE) with |dx| <= D and |dy| <= D; the optical
// groups are the connected components of "close"; the origin of a group is the cluster's kept read when the group
// holds it, else the smallest read index of the group; every other read of the group is an optical duplicate.
//   k_best_rep (kernels_best.hip.h)  the kept reads claim their clusters: the check of the input
//   OptKeyX / OptKeyTile / OptKeyCid  keys of the three stable radix sorts that order the read indices by
//                   (cluster_id, tile, x); a read that is no member sorts as (0, 0, 0) and none of its fields are read
//   k_opt_gather    per sorted position: (cluster << 32 | tile), (x << 32 | y), the vote (kept ? 0 : 1) << 32 | read
//   k_opt_walk      every position joins the positions of its window (same cluster and tile, x no more than D ahead)
//                   whose y is no more than D away, in a forest over the sorted positions (uf_union); a window of
//                   more than `walk` positions is finished by the whole wave
//   k_opt_root      per member: its root, a 64-bit atomic minimum of the vote and a count at the root
//   k_opt_write     optical / origin per read, per_cluster (one atomic per run of equal ids inside a wave), summary
// All differences are taken between ordered unsigned values (the sort makes x ascend inside a window), so nothing
// wraps.  The result is a set partition plus a minimum over a total order: it does not depend on the order of the
// atomics.  Malformed input (BEST_ERR set or claims != C after k_best_rep) ends every kernel here at once: nothing
// is written to the caller's buffers and no index that was not checked is followed.
// Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_OPTICAL_HIP_H
#define HUMID_KERNELS_OPTICAL_HIP_H

#include "common.hip.h"
#include "kernels_best.hip.h"
#include "kernels_graph.hip.h"

#define OPT_WALK_DEFAULT 64u   // option "optical_walk": followers a position compares itself with before its wave takes over

// the pass's u64 counters (beside the u32 counters of k_best_rep)
enum { OPT_MEMBERS = 0, OPT_OPTICAL, OPT_GROUPS /* groups of at least 2 reads */, OPT_LARGEST, OPT_CTRS = 4 };

// sort keys, read through the permutation of the sort before (null: the identity)
struct OptKeyX {
  const u32 *cid, *x;
  __device__ __forceinline__ u32 operator()(u64 i) const { return cid[i] != 0 ? x[i] : 0u; }
};
struct OptKeyTile {
  const u32 *cid, *tile, *perm;
  __device__ __forceinline__ u32 operator()(u64 i) const { const u32 r = perm[i]; return cid[r] != 0 ? tile[r] : 0u; }
};
struct OptKeyCid {
  const u32 *cid, *perm;
  __device__ __forceinline__ u32 operator()(u64 i) const { return cid[perm[i]]; }
};

__device__ __forceinline__ u32 opt_absdiff(u32 a, u32 b) { return a > b ? a - b : b - a; }

__device__ __forceinline__ bool opt_bad(const u32 *__restrict__ bctr, u32 C) { return bctr[BEST_ERR] != 0 || bctr[BEST_CLAIMS] != C; }

// scid[p] (the last sort's keys) and perm[p] -> the three records of sorted position p; parent[p] = p.  A position
// that is no member gets a (cluster, tile) word no member shares.  per_cluster (may be null) is cleared here, behind
// the check, for k_opt_write to add to.
static __global__ void __launch_bounds__(256)
k_opt_gather(const u32 *__restrict__ scid, const u32 *__restrict__ perm, const u8 *__restrict__ keep, const u32 *__restrict__ tile,
             const u32 *__restrict__ x, const u32 *__restrict__ y, u32 n, u32 C, const u32 *__restrict__ bctr,
             u64 *__restrict__ ct, u64 *__restrict__ xy, u64 *__restrict__ vote, u32 *__restrict__ parent,
             u32 *__restrict__ per_cluster) {
  HUMID_GUARD_LAST_VGPR();
  if (opt_bad(bctr, C)) return;                                      // (uniform over the grid)
  if (per_cluster)
    for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < C; k += gridDim.x * blockDim.x) per_cluster[k] = 0;
  for (u32 p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
    const u32 c = scid[p], r = perm[p];
    u64 a = (u64)HUMID_NO_TILE, b = 0, v = ((u64)1 << 32) | r;
    if (c != 0) {
      a = ((u64)c << 32) | tile[r];
      b = ((u64)x[r] << 32) | y[r];
      if (keep[r] != 0) v = r;
    }
    ct[p] = a;
    xy[p] = b;
    vote[p] = v;
    parent[p] = p;
  }
}

// One lane per sorted position p.  Its window: the positions q > p with ct[q] == ct[p] and x[q] - x[p] <= D (x ascends
// inside equal ct, so the window is a stretch that starts at p + 1 and the difference never wraps).  The lane walks the
// first `walk` of them itself (walk == 0: all).  Lanes whose window goes on are then served one after the other by the
// whole wave: the 64 lanes stride the rest of the window and a ballot tells whether all 64 were still inside.  The grid
// covers whole waves and no lane leaves before the last ballot.
static __global__ void __launch_bounds__(256)
k_opt_walk(const u64 *__restrict__ ct, const u64 *__restrict__ xy, u32 n, u32 C, u32 D, u32 walk, const u32 *__restrict__ bctr,
           u32 *parent) {
  HUMID_GUARD_LAST_VGPR();
  if (opt_bad(bctr, C)) return;                                      // (uniform over the grid)
  const u32 lane = threadIdx.x & 63u;
  const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  u64 a = 0, b = 0;
  bool live = false;
  if (p < n) {
    a = ct[p];
    b = xy[p];
    live = (u32)a != HUMID_NO_TILE;                                  // (no member, or a member without a position)
  }
  const u32 px = (u32)(b >> 32), py = (u32)b;
  u32 q = p + 1;
  if (live) {
    const u32 stop = (walk == 0 || n - q < walk) ? n : q + walk;     // (q <= n)
    live = false;
    for (; q < n; q++) {
      if (q == stop) { live = true; break; }                         // the window goes on: the wave's
      if (ct[q] != a) break;
      const u64 o = xy[q];
      if ((u32)(o >> 32) - px > D) break;
      if (opt_absdiff((u32)o, py) <= D) uf_union(parent, p, q);
    }
  }
  u64 todo = __ballot(live);
  while (todo) {
    const u32 src = (u32)__ffsll((long long)todo) - 1u;
    todo &= todo - 1ull;
    const u32 sp = (u32)__shfl((int)p, (int)src);
    const u32 sa_lo = (u32)__shfl((int)(u32)a, (int)src), sa_hi = (u32)__shfl((int)(u32)(a >> 32), (int)src);
    const u32 sx = (u32)__shfl((int)px, (int)src), sy = (u32)__shfl((int)py, (int)src);
    const u64 sa = ((u64)sa_hi << 32) | sa_lo;
    u32 base = (u32)__shfl((int)q, (int)src);
    while (true) {
      const u32 qq = base + lane;                                    // (base < n < 2^31: no wrap)
      bool in = false;
      if (qq < n && ct[qq] == sa) {
        const u64 o = xy[qq];
        in = (u32)(o >> 32) - sx <= D;
        if (in && opt_absdiff((u32)o, sy) <= D) uf_union(parent, sp, qq);
      }
      if (__ballot(in) != ~0ull) break;
      base += 64u;
    }
  }
}

// Per member: root[p], the smallest vote of its group and the group's size at the root.  Lanes of a wave that hold a
// run of equal roots count once; a plain load lets a vote that cannot lower the slot skip its atomic (the slot only
// falls, so a stale value costs a needless atomic, never a missed one).  Whole waves.
static __global__ void __launch_bounds__(256)
k_opt_root(const u64 *__restrict__ ct, const u64 *__restrict__ vote, u32 n, u32 C, const u32 *__restrict__ bctr,
           const u32 *__restrict__ parent, u32 *__restrict__ root, ull *best, u32 *gsize) {
  HUMID_GUARD_LAST_VGPR();
  if (opt_bad(bctr, C)) return;                                      // (uniform over the grid)
  const u32 lane = threadIdx.x & 63u;
  const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  const bool mem = p < n && (ct[p] >> 32) != 0;
  u32 r = NONE32;
  if (mem) {
    r = uf_find(parent, p);
    root[p] = r;
    const u64 v = vote[p];
    const u64 seen = __hip_atomic_load(&best[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v < seen) atomicMin(&best[r], (ull)v);
  }
  const u32 pr = (u32)__shfl_up((int)r, 1);
  const u64 heads = __ballot(lane == 0 || pr != r);
  const u64 upto = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);
  const u32 first = 63u - (u32)__clzll((long long)(heads & upto));   // (never 0 bits: lane 0 is a head)
  const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
  if (tail && mem) atomicAdd(&gsize[r], lane - first + 1u);
}

// optical / origin (may be null) per read, per_cluster (may be null; cleared by k_opt_gather), the four sums.  The sorted order
// holds every read once, members and others, so every entry of the outputs is written.  Whole waves stay in the loop.
static __global__ void __launch_bounds__(256)
k_opt_write(const u64 *__restrict__ ct, const u64 *__restrict__ vote, const u32 *__restrict__ root, const ull *__restrict__ best,
            const u32 *__restrict__ gsize, u32 n, u32 C, const u32 *__restrict__ bctr, u8 *__restrict__ optical,
            u32 *__restrict__ origin, u32 *per_cluster, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  if (opt_bad(bctr, C)) return;                                      // (uniform over the grid)
  const u32 lane = threadIdx.x & 63u;
  const u32 n_up = (n + 63u) & ~63u;
  u32 members = 0, opticals = 0, groups = 0, largest = 0;
  for (u32 p = blockIdx.x * blockDim.x + threadIdx.x; p < n_up; p += gridDim.x * blockDim.x) {
    u32 c = 0;
    bool opt = false, big = false;
    if (p < n) {
      c = (u32)(ct[p] >> 32);
      const u32 i = (u32)vote[p];
      u32 org = HUMID_NO_READ;
      if (c != 0) {
        const u32 r = root[p];
        org = (u32)best[r];
        opt = org != i;
        if (r == p) {                                                // one position per group
          const u32 s = gsize[r];
          big = s >= 2u;
          largest = s > largest ? s : largest;
        }
      }
      optical[i] = (u8)opt;
      if (origin) origin[i] = org;
    }
    const u64 m_mem = __ballot(c != 0), m_opt = __ballot(opt);
    members += (u32)__popcll(m_mem);
    opticals += (u32)__popcll(m_opt);
    groups += (u32)__popcll(__ballot(big));
    if (per_cluster) {
      const u32 pc = (u32)__shfl_up((int)c, 1);
      const u64 heads = __ballot(lane == 0 || pc != c);
      const u64 upto = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);
      const u32 first = 63u - (u32)__clzll((long long)(heads & upto));
      const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
      const u32 k = (u32)__popcll(m_opt & upto & ~((1ull << first) - 1ull));
      if (tail && c != 0 && k) atomicAdd(&per_cluster[c - 1u], k);
    }
  }
#pragma unroll
  for (u32 d = 32; d; d >>= 1) {
    const u32 o = (u32)__shfl_xor((int)largest, (int)d);
    largest = o > largest ? o : largest;
  }
  if (lane == 0) {                                                   // (members, opticals and groups are wave sums already)
    if (members) atomicAdd(&ctr[OPT_MEMBERS], (ull)members);
    if (opticals) atomicAdd(&ctr[OPT_OPTICAL], (ull)opticals);
    if (groups) atomicAdd(&ctr[OPT_GROUPS], (ull)groups);
    if (largest) atomicMax(&ctr[OPT_LARGEST], (ull)largest);
  }
}

#endif  // HUMID_KERNELS_OPTICAL_HIP_H
