// kernels_paired.hip.h -- strand-symmetric (duplex) deduplication (humid_dedup_run_paired*, humid_paired_canonical*,
// humid_get_strands; include/humid_hip.h).  A word of n = 2 h nucleotides is A.B (two halves of h); its mirror is
// m(A.B) = B.A, the word the same molecule gives when it is read from its other strand.  The pass runs over the
// CANONICAL words c(w) = min(w, m(w)), and two leaves u, v are neighbours when min(ham(u, v), ham(u, m(v))) <= d.
//   k_pd_canonical     per read: canonical word + strand (top: w == c(w); bottom otherwise; none: filtered)
//   k_pd_mirror        m(leaf) for every leaf, materialised once (a field of the plan may cross the half boundary)
//   k_pd_join          candidate join of one combination of the pigeonhole plan: X = the leaves' keys, Y = the keys of
//                      the leaves (plain pairs) or of the mirrored leaves (mirror pairs), both sorted by key.  One thread
//                      per X entry finds its run of equal keys in Y by binary search and verifies every candidate by
//                      popcount: ham(x, yw[y]) with yw = the leaves or their mirrors.  Count pass, then fill pass.
//   k_pd_join_chunks   the same with every run cut into pieces of `walk` candidates (k_edit_chunks lists them)
//   k_pd_tally         top[c] / bottom[c]: reads of each strand per cluster, one atomic per run of equal ids in a wave
//   k_pd_summary       duplex / top-only / bottom-only clusters and the reads of each strand
// Why every pair is found with the SMALLER leaf as x: ham(u, m(v)) <= d leaves some combination of the plan untouched
// between u and m(v), so u's key equals the key of m(v) there, whichever of u and v is the smaller; the same holds
// for ham(u, v).  So both joins keep only rx < ry: a pair comes out at most once per combination and join, and a leaf
// never pairs with itself even when ham(u, m(u)) <= d.  What comes out twice goes away in unique_edges.
// Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_PAIRED_HIP_H
#define HUMID_KERNELS_PAIRED_HIP_H

#include "common.hip.h"

// m(w) of an n-nucleotide word, n even (2 <= n <= 32 in one u64, 34 <= n <= 64 in W2)
__host__ __device__ __forceinline__ u64 pd_mirror(u64 w, u32 n) {
  const u64 low = (n >= 64) ? ~0ull : ((1ull << n) - 1ull);          // the last h nucleotides: n bits
  return n >= 64 ? w : (((w & low) << n) | (w >> n));
}
__host__ __device__ __forceinline__ W2 pd_mirror(W2 w, u32 n) {
  const unsigned __int128 v = ((unsigned __int128)w.hi << 64) | w.lo;
  const unsigned __int128 low = (((unsigned __int128)1) << n) - 1;   // n <= 64
  const unsigned __int128 r = ((v & low) << n) | (v >> n);
  return W2{(u64)(r >> 64), (u64)r};
}
__host__ __device__ __forceinline__ bool pd_less(u64 a, u64 b) { return a < b; }
__host__ __device__ __forceinline__ bool pd_less(W2 a, W2 b) { return w_less(a, b); }

enum { PD_DUPLEX = 0, PD_TOP_ONLY, PD_BOTTOM_ONLY, PD_TOP_READS, PD_BOTTOM_READS, PD_CTRS = 8 };

// words_out may be words (every thread reads its word before it writes it); a filtered read's word is not read and
// its output word is left as it is
template <class WT>
__global__ void __launch_bounds__(256)
k_pd_canonical(const WT *words, const u8 *__restrict__ filt, u32 n_reads, u32 n, WT *words_out, u8 *__restrict__ strand) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_reads) return;
  if (filt[i]) { strand[i] = (u8)HUMID_STRAND_NONE; return; }
  const WT w = words[i];
  const WT m = pd_mirror(w, n);
  const bool bottom = pd_less(m, w);
  words_out[i] = bottom ? m : w;
  strand[i] = bottom ? (u8)HUMID_STRAND_BOTTOM : (u8)HUMID_STRAND_TOP;
}

template <class WT>
__global__ void __launch_bounds__(256)
k_pd_mirror(const WT *__restrict__ leaf, u32 U, u32 n, WT *__restrict__ mir) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < U) mir[i] = pd_mirror(leaf[i], n);
}

// COUNT: pc[t] = pairs found; FILL: (smaller rank << 32 | larger rank) from poff[t].  walk / big: as k_edit_join.
template <bool FILL, class KeyT, class WT>
__global__ void __launch_bounds__(256)
k_pd_join(const KeyT *__restrict__ KX, const u32 *__restrict__ VX, const KeyT *__restrict__ KY, const u32 *__restrict__ VY,
          u32 n, const WT *__restrict__ xw, const WT *__restrict__ yw, u32 distance, u32 *__restrict__ pc,
          const u32 *__restrict__ poff, u64 *__restrict__ edges, u32 walk, ull *big) {
  HUMID_GUARD_LAST_VGPR();
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const KeyT key = KX[t];
  const u32 rx = VX[t];
  const WT wx = xw[rx];
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (KY[mid] < key) lo = mid + 1; else hi = mid;
  }
  if (!FILL && walk && lo + walk < n && KY[lo + walk] == key) { atomicOr(big, 1ull); pc[t] = 0; return; }
  u32 found = 0;
  u64 e = FILL ? (u64)poff[t] : 0;
  for (u32 j = lo; j < n && KY[j] == key; j++) {
    const u32 ry = VY[j];
    if (ry <= rx) continue;
    if (w_mismatch(w_xor(wx, yw[ry])) > distance) continue;
    if (FILL) edges[e++] = ((u64)rx << 32) | ry;
    else found++;
  }
  if (!FILL) pc[t] = found;
}

// one thread per piece of k_edit_chunks (run_lo, chunk_off = exclusive scan of the pieces per X entry, n + 1 entries)
template <bool FILL, class KeyT, class WT>
__global__ void __launch_bounds__(256)
k_pd_join_chunks(const KeyT *__restrict__ KX, const u32 *__restrict__ VX, const KeyT *__restrict__ KY,
                 const u32 *__restrict__ VY, u32 n, const u32 *__restrict__ run_lo, const u32 *__restrict__ chunk_off,
                 u32 n_pieces, u32 walk, const WT *__restrict__ xw, const WT *__restrict__ yw, u32 distance,
                 u32 *__restrict__ pc, const u32 *__restrict__ poff, u64 *__restrict__ edges) {
  HUMID_GUARD_LAST_VGPR();
  const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pieces) return;
  u32 lo = 0, hi = n;                                  // the X entry of this piece: largest t with chunk_off[t] <= p
  while (hi - lo > 1) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (chunk_off[mid] <= p) lo = mid; else hi = mid;
  }
  const u32 t = lo;
  const KeyT key = KX[t];
  const u32 rx = VX[t];
  const WT wx = xw[rx];
  const u32 j0 = run_lo[t] + (p - chunk_off[t]) * walk;
  u32 found = 0;
  u64 e = FILL ? (u64)poff[p] : 0;
  for (u32 j = j0; j < n && j - j0 < walk && KY[j] == key; j++) {
    const u32 ry = VY[j];
    if (ry <= rx) continue;
    if (w_mismatch(w_xor(wx, yw[ry])) > distance) continue;
    if (FILL) edges[e++] = ((u64)rx << 32) | ry;
    else found++;
  }
  if (!FILL) pc[p] = found;
}

// top[c] / bottom[c] (u32[C + 1], zeroed; slot 0 unused): lanes of a wave that hold a run of equal ids add once -- the
// run's last lane adds the run's two sums (segmented by the ballot of the run heads, as k_best_vote).  An id above C
// is not followed.  The grid covers whole waves; no lane leaves before the ballots.
static __global__ void __launch_bounds__(256)
k_pd_tally(const u32 *__restrict__ cid, const u8 *__restrict__ strand, u32 n, u32 C, u32 *top, u32 *bottom) {
  HUMID_GUARD_LAST_VGPR();
  const u32 lane = threadIdx.x & 63u;
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  u32 c = i < n ? cid[i] : 0u;
  const u32 s = i < n ? (u32)strand[i] : HUMID_STRAND_NONE;
  if (c > C || s == HUMID_STRAND_NONE) c = 0;
  const u32 pc = (u32)__shfl_up((int)c, 1);
  const u64 heads = __ballot(lane == 0 || pc != c);
  const u64 is_bottom = __ballot(c != 0 && s == HUMID_STRAND_BOTTOM);
  const bool tail = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
  if (tail && c != 0) {
    const u64 below = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));   // (never 0: lane 0 is a head)
    const u32 first = 63u - (u32)__clzll((long long)below);
    const u64 run = (lane == 63u ? ~0ull : ((2ull << lane) - 1ull)) & ~((1ull << first) - 1ull);   // lanes first .. lane
    const u32 nb = (u32)__popcll(is_bottom & run), nt = (u32)__popcll(run) - nb;
    if (nt) atomicAdd(&top[c], nt);
    if (nb) atomicAdd(&bottom[c], nb);
  }
}

// ctr (ull[PD_CTRS], zeroed): one atomic per counter and workgroup
static __global__ void __launch_bounds__(256)
k_pd_summary(const u32 *__restrict__ top, const u32 *__restrict__ bottom, u32 C, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ ull lds[4][5];
  ull v[5] = {0, 0, 0, 0, 0};
  const u32 C_up = (C + 255u) & ~255u;
  for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < C_up; k += gridDim.x * blockDim.x) {
    const u32 t = k < C ? top[k + 1] : 0u, b = k < C ? bottom[k + 1] : 0u;
    v[PD_DUPLEX] += (t && b) ? 1u : 0u;
    v[PD_TOP_ONLY] += (t && !b) ? 1u : 0u;
    v[PD_BOTTOM_ONLY] += (!t && b) ? 1u : 0u;
    v[PD_TOP_READS] += t;
    v[PD_BOTTOM_READS] += b;
  }
#pragma unroll
  for (u32 q = 0; q < 5; q++) {
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) {
      const u32 lo = (u32)__shfl_xor((int)(u32)v[q], d), hi = (u32)__shfl_xor((int)(u32)(v[q] >> 32), d);
      v[q] += ((ull)hi << 32) | lo;
    }
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    const ull t = lds[0][threadIdx.x] + lds[1][threadIdx.x] + lds[2][threadIdx.x] + lds[3][threadIdx.x];
    if (t) atomicAdd(&ctr[threadIdx.x], t);
  }
}

#endif  // HUMID_KERNELS_PAIRED_HIP_H
