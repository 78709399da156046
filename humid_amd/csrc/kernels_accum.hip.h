// kernels_accum.hip.h -- accumulated runs (humid_accum_*): a read set fed in chunks.  The accumulator is an ascending
// list of distinct words with (count u32, first_index u64); a chunk arrives as the count stage's own ascending list
// (s_word, s_cnt, s_first).  Two pieces of device code, templated on the word type (u64 or W2):
//   the MERGE of the two lists, equal words combined (counts added, first = minimum), in merge-path form:
//     k_accum_partition  one lane per tile boundary: the split (entries of A) of the diagonal t * T of the A + B merge
//                        order, by binary search (ties: A first)
//     k_accum_tile<0>    one workgroup per tile of T merge positions: its A part and B part staged in LDS, every
//                        position found by a binary search IN LDS, the positions that start a new word counted
//     (one exclusive scan over the tiles, prims.hip.h, whose total is the new number of words)
//     k_accum_tile<1>    the same merge again; every new word written at (tile offset + its rank in the tile)
//   A duplicate is always an (a, b) pair of neighbours in merge order, a first.  The a of a pair writes the combined
//   entry and the b writes nothing, so a lane needs no other lane's result: the A part is staged with the entry BEFORE
//   it and the B part with the entry BEHIND it, which is all a pair cut by a tile boundary needs.
//   LDS: (T + 2) words, 16 KB (u64) or 32 KB (W2) at the default T = ACC_TILE = 2048: several workgroups per CU.
//   the LOOKUP of a chunk's unique words in the accumulated list (k_accum_lookup): one binary search per chunk leaf.
// A keyed accumulator (humid_accum_*_keyed) runs the same code over entries (key, word): the second half of this file.
// Integers only.  The only atomics are the overflow flag and the unknown-read counter: results do not depend on the schedule.
#ifndef HUMID_KERNELS_ACCUM_HIP_H
#define HUMID_KERNELS_ACCUM_HIP_H

#include "common.hip.h"
#include "kernels_gkey.hip.h"

#define ACC_TILE 2048u       // default merge positions per tile (option "accum_tile": a power of two, 64 .. ACC_TILE)
#define ACC_THREADS 256u

__host__ __device__ __forceinline__ bool acc_le(u64 a, u64 b) { return a <= b; }
__host__ __device__ __forceinline__ bool acc_le(W2 a, W2 b) { return !w_less(b, a); }
__host__ __device__ __forceinline__ bool acc_eq(u64 a, u64 b) { return a == b; }
__host__ __device__ __forceinline__ bool acc_eq(W2 a, W2 b) { return w_eq(a, b); }

// entries of A among the first d of the merge of a[0 .. na) and b[0 .. nb) (both ascending, ties: a first), d <= na + nb
template <class WT>
__device__ __forceinline__ u32 acc_split(const WT *a, u32 na, const WT *b, u32 nb, u32 d) {
  u32 lo = d > nb ? d - nb : 0u, hi = d < na ? d : na;
  while (lo < hi) {
    const u32 mid = lo + ((hi - lo) >> 1);
    if (acc_le(a[mid], b[d - 1 - mid])) lo = mid + 1; else hi = mid;     // a[mid] is among the first d
  }
  return lo;
}

// split[t] for t in [0, n_tiles]: entries of A before merge position min(t * T, nA + nB)
template <class WT>
__global__ void k_accum_partition(const WT *__restrict__ a_word, u32 nA, const WT *__restrict__ b_word, u32 nB, u32 T, u32 n_tiles,
                                  u32 *__restrict__ split) {
  HUMID_GUARD_LAST_VGPR();
  const u64 P = (u64)nA + nB;
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t <= n_tiles; t += (u64)gridDim.x * blockDim.x) {
    const u64 d = t * T < P ? t * T : P;
    split[t] = acc_split(a_word, nA, b_word, nB, (u32)d);
  }
}

// One tile of the merge.  FILL = 0: tile_cnt[tile] = positions of the tile that start a new word; a combined count
// beyond 2^32 - 1 raises *overflow.  FILL = 1: the new words of the tile written from tile_off[tile] on.
// Dynamic LDS: (T + 2) words.
template <class WT, int FILL>
__global__ void __launch_bounds__(ACC_THREADS)
k_accum_tile(const WT *__restrict__ a_word, const u32 *__restrict__ a_cnt, const u64 *__restrict__ a_first, u32 nA,
             const WT *__restrict__ b_word, const u32 *__restrict__ b_cnt, const u32 *__restrict__ b_first, u32 nB, u64 base,
             u32 T, const u32 *__restrict__ split, u32 *__restrict__ tile_cnt, const u32 *__restrict__ tile_off,
             WT *__restrict__ o_word, u32 *__restrict__ o_cnt, u64 *__restrict__ o_first, u32 *__restrict__ overflow) {
  HUMID_GUARD_LAST_VGPR();
  extern __shared__ __attribute__((aligned(16))) unsigned char acc_lds[];
  __shared__ u32 wave_sum[ACC_THREADS / 64];
  const u32 tile = blockIdx.x, tid = threadIdx.x;
  const u64 P = (u64)nA + nB;
  const u64 p0 = (u64)tile * T, p1 = p0 + T < P ? p0 + T : P;
  const u32 a0 = split[tile], a1 = split[tile + 1];
  const u32 b0 = (u32)(p0 - a0), b1 = (u32)(p1 - a1);
  const u32 na = a1 - a0, nb = b1 - b0, nt = na + nb;            // nt <= T
  const bool has_prev = a0 > 0, has_next = b1 < nB;
  // sa[0] = A[a0 - 1] (if any), sa[1 + i] = A[a0 + i]; sb[j] = B[b0 + j], sb[nb] = B[b1] (if any)
  WT *sa = (WT *)acc_lds, *sb = sa + na + 1;
  for (u32 i = tid; i < na + 1; i += ACC_THREADS)
    if (i > 0 || has_prev) sa[i] = a_word[a0 + i - 1];
  for (u32 j = tid; j < nb + 1; j += ACC_THREADS)
    if (j < nb || has_next) sb[j] = b_word[b0 + j];
  __syncthreads();
  u32 run = FILL ? tile_off[tile] : 0u;                          // new words before the round's first position
  for (u32 q0 = 0; q0 < nt; q0 += ACC_THREADS) {
    const u32 q = q0 + tid;
    bool head = false, from_a = false, paired = false;
    u32 i = 0, j = 0;
    if (q < nt) {
      i = acc_split(sa + 1, na, sb, nb, q);
      j = q - i;
      from_a = i < na && (j >= nb || acc_le(sa[1 + i], sb[j]));
      if (from_a) {
        head = true;
        paired = (j < nb || has_next) && acc_eq(sa[1 + i], sb[j]);
      } else
        head = !((i > 0 || has_prev) && acc_eq(sa[i], sb[j]));   // sa[i] = the last entry of A before this b
    }
    if (!FILL && paired && (u64)a_cnt[a0 + i] + b_cnt[b0 + j] > 0xffffffffull) atomicOr(overflow, 1u);
    // rank of the position among the round's new words: ballot inside the wave, the waves' totals through LDS
    const u64 bal = __ballot(head);
    const u32 lane = tid & 63u, wv = tid >> 6;
    const u32 below = (u32)__popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_sum[wv] = (u32)__popcll(bal);
    __syncthreads();
    u32 before = 0, total = 0;
    for (u32 w = 0; w < ACC_THREADS / 64; w++) {
      const u32 s = wave_sum[w];
      before += w < wv ? s : 0u;
      total += s;
    }
    if (FILL && head) {
      const u32 o = run + before + below;
      if (from_a) {
        u32 cnt = a_cnt[a0 + i];
        u64 first = a_first[a0 + i];
        if (paired) {
          const u64 fb = base + b_first[b0 + j];
          cnt += b_cnt[b0 + j];
          first = fb < first ? fb : first;
        }
        o_word[o] = sa[1 + i]; o_cnt[o] = cnt; o_first[o] = first;
      } else {
        o_word[o] = sb[j]; o_cnt[o] = b_cnt[b0 + j]; o_first[o] = base + b_first[b0 + j];
      }
    }
    run += total;
    __syncthreads();                                             // wave_sum is written again in the next round
  }
  if (!FILL && tid == 0) tile_cnt[tile] = run;
}

// Per leaf of the chunk just counted (words b_word ascending, reads b_cnt, first local read b_first): its place in the
// accumulated list a_word[0 .. nA), the cluster id there, and is-max only for the leaf whose first read IS the
// accumulated first read.  A word the accumulator never saw: 0 / 0, its reads added to *unknown.
template <class WT>
__global__ void k_accum_lookup(const WT *__restrict__ a_word, const u64 *__restrict__ a_first, const u32 *__restrict__ a_cid,
                               const u8 *__restrict__ a_ismax, u32 nA, const WT *__restrict__ b_word, const u32 *__restrict__ b_cnt,
                               const u32 *__restrict__ b_first, u32 nB, u64 base, u32 *__restrict__ l_cid, u8 *__restrict__ l_ismax,
                               ull *__restrict__ unknown) {
  HUMID_GUARD_LAST_VGPR();
  for (u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x; u < nB; u += (u64)gridDim.x * blockDim.x) {
    const WT w = b_word[u];
    u32 lo = 0, hi = nA;                                         // lower bound of w
    while (lo < hi) {
      const u32 mid = lo + ((hi - lo) >> 1);
      if (acc_le(w, a_word[mid])) hi = mid; else lo = mid + 1;
    }
    const bool found = lo < nA && acc_eq(a_word[lo], w);
    l_cid[u] = found ? a_cid[lo] : 0u;
    l_ismax[u] = (found && a_ismax[lo] && a_first[lo] == base + b_first[u]) ? (u8)1 : (u8)0;
    if (!found) atomicAdd(unknown, (ull)b_cnt[u]);
  }
}

// ---- keyed accumulators (humid_accum_*_keyed): an entry is the pair (key, word) in (key, word) order -------------------
// ET, the entry type: u64 `key << 2 * word_nt | word` when key_nt >= 1 and key_nt + word_nt <= 32, W2 {hi = key, lo = word}
// otherwise.  Either orders as (key, word) does, so the count stage, the merge and the lookup above run over entries as
// they do over words.  Three kernels of their own:
//   k_acck_pack    per read of a chunk: its entry (a filtered read's is 0: its key is not read); a usable key that does
//                  not fit key_nt stores `epoch` into *bad, as k_gkey_words does for a group, and is cut to the field
//   k_acck_heads   per entry of the accumulated list: 1 where the key differs from the entry before (finish; one
//                  exclusive scan over the flags ranks the keys, its total is the number of distinct keys)
//   k_acck_ranks   per entry: the internal word `rank << 2 * word_nt | word` of a keyed pass (IT: u64, or W2 beyond 32
//                  nucleotides), and at every head the key itself into keys[rank]
__device__ __forceinline__ u64 acck_key(u64 e, u32 wb) { return e >> wb; }             // (one-word entries: wb <= 62)
__device__ __forceinline__ u64 acck_key(W2 e, u32) { return e.hi; }
__device__ __forceinline__ u64 acck_word(u64 e, u32 wb) { return e & ((1ull << wb) - 1ull); }
__device__ __forceinline__ u64 acck_word(W2 e, u32) { return e.lo; }
__device__ __forceinline__ void acck_put(u64 *out, u64 key, u64 word, u32 wb) { *out = (key << wb) | word; }
__device__ __forceinline__ void acck_put(W2 *out, u64 key, u64 word, u32) { *out = W2{key, word}; }

template <class ET>
__global__ void k_acck_pack(const u64 *__restrict__ words, const u64 *__restrict__ key, const u8 *__restrict__ filt, u32 n,
                            u32 word_nt, u32 key_nt, ET *__restrict__ out, u32 *bad, u32 epoch) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  bool wrong = false;
  if (i < n) {
    u64 k = 0, w = 0;
    if (filt[i] == 0) {
      const u64 kmask = (key_nt == 0 || key_nt >= 32) ? ~0ull : (1ull << (2 * key_nt)) - 1ull;
      const u64 wmask = word_nt >= 32 ? ~0ull : (1ull << (2 * word_nt)) - 1ull;
      k = key[i];
      wrong = (k & ~kmask) != 0;
      k &= kmask;
      w = words[i] & wmask;
    }
    acck_put(&out[i], k, w, 2 * word_nt);
  }
  const u64 lanes = __ballot(wrong);
  if (lanes && (threadIdx.x & 63u) == (u32)(__ffsll((long long)lanes) - 1)) {
    __hip_atomic_store(bad, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
  }
}

// head[i] for i in [0, U]: entry i starts a key; head[U] = 0 is the scan's sentinel
template <class ET>
__global__ void k_acck_heads(const ET *__restrict__ ent, u32 U, u32 wb, u32 *__restrict__ head) {
  HUMID_GUARD_LAST_VGPR();
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= U; i += (u64)gridDim.x * blockDim.x)
    head[i] = (i < U && (i == 0 || acck_key(ent[i], wb) != acck_key(ent[i - 1], wb))) ? 1u : 0u;
}

// hpos: the exclusive scan of head.  The rank of entry i's key is the number of heads up to and including i, less one.
template <class ET, class IT>
__global__ void k_acck_ranks(const ET *__restrict__ ent, const u32 *__restrict__ head, const u32 *__restrict__ hpos, u32 U, u32 wb,
                             u64 *__restrict__ keys, IT *__restrict__ iword) {
  HUMID_GUARD_LAST_VGPR();
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < U; i += (u64)gridDim.x * blockDim.x) {
    const ET e = ent[i];
    const u32 h = head[i], rank = hpos[i] + h - 1u;
    if (h) keys[rank] = acck_key(e, wb);
    gk_put(&iword[i], ((unsigned __int128)rank << wb) | acck_word(e, wb));              // (wb <= 64)
  }
}

#endif  // HUMID_KERNELS_ACCUM_HIP_H
