// kernels_long.hip.h -- long words: 1 .. HUMID_LONG_MAX_NT nucleotides, k = ceil(n / 32) uint64 per read
// (humid_dedup_run_long*, include/humid_hip.h).  Part of libhumid_hip.so; device code for gfx950 only.
// k is a run-time argument of every kernel: nothing here is a template over the word length.
//
// Layout: word r is words[k r .. k r + k); [k r] holds the first n - 32 (k - 1) nucleotides right-aligned ("the head":
// hbits = 2 (n - 32 (k - 1)) significant bits, the bits above are ignored), every following uint64 the next 32.  Read
// as one string of 64 k bits, most significant first, the word starts at bit 64 k - 2 n and the bits in front are zero
// once the head is masked; numeric order of that string == lexicographic order of the nucleotides == Trie::walk() order.
//
// Count (the sorting count of kernels_wide.hip.h for k words): k stable LSD radix sorts of (u64 key, u32 read index),
// least significant uint64 first (k_long_keys makes the keys of one pass), the filtered reads behind all words by a flag
// bit above the head or, where the head has no spare bit, by a one-bit pass (k_wide_keys_flag).  Then the words in
// sorted order (k_long_gather), run heads (k_long_heads), a scan, and the leaves (k_long_unique, k_wide_counts).
//
// Neighbours: per segment of the pigeonhole plan one key per leaf (k_long_seg_keys), sorted, joined with itself:
// k_long_join / k_long_join_chunks verify every candidate by the exact Hamming distance over all k uint64
// (long_within).  The sort is stable over ascending leaf indices, so inside a run of equal keys the leaves ascend: the
// candidates of entry t are the entries behind it, and a pair comes out once per segment with the smaller leaf first.
#ifndef HUMID_KERNELS_LONG_HIP_H
#define HUMID_KERNELS_LONG_HIP_H

#include "common.hip.h"
#include "kernels_count.hip.h"

// The candidates a workgroup verified, added to one of LONG_CAND_SLOTS counters of its join (the host sums them): one
// atomic per workgroup, spread over the slots -- one per wave on ONE address was half a millisecond at 3 M entries, the
// whole of the join kernel's time (profiles/long.md).  All threads of the workgroup call it.
#define LONG_CAND_SLOTS 32u
__device__ __forceinline__ void long_block_add(ull x, ull *lsum, ull *slots) {
  if (threadIdx.x == 0) *lsum = 0;
  __syncthreads();
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
  if ((threadIdx.x & 63u) == 0 && x) atomicAdd(lsum, x);
  __syncthreads();
  if (threadIdx.x == 0 && *lsum) atomicAdd(&slots[blockIdx.x & (LONG_CAND_SLOTS - 1u)], *lsum);
}

// the keys of one sort pass: uint64 j of every word, in the order vin of the pass before (null: read order; that
// pass also writes val = the read indices and counts the usable reads).  j = 0 is the head: masked to hbits bits,
// and with a spare bit (hbits < 64) the filtered reads get the value above every head.
static __global__ void __launch_bounds__(256)
k_long_keys(const u64 *__restrict__ words, const u8 *__restrict__ filtered, const u32 *__restrict__ vin, u32 n, u32 k,
            u32 j, u32 hbits, u64 *__restrict__ key, u32 *__restrict__ val, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 lds[8];
  const u64 hmask = hbits >= 64 ? ~0ull : ((1ull << hbits) - 1ull);
  u32 usable = 0;
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const u32 r = vin ? vin[i] : i;
    u64 x = words[(size_t)k * r + j];
    if (j == 0) {
      x &= hmask;
      if (hbits < 64 && filtered && filtered[r]) x = 1ull << hbits;
    }
    key[i] = x;
    if (!vin) {
      val[i] = i;
      usable += (filtered && filtered[i]) ? 0u : 1u;
    }
  }
  if (!vin) {                                            // (uniform over the grid)
    const u32 t = block_sum(usable, lds);
    if (threadIdx.x == 0 && t) atomicAdd(&ctr[CTR_USABLE], (ull)t);
  }
}

// words in sorted order, heads masked: one thread per uint64, k consecutive lanes read one word
static __global__ void __launch_bounds__(256)
k_long_gather(const u64 *__restrict__ words, const u32 *__restrict__ v, u32 n, u32 k, u32 hbits, u64 *__restrict__ sw) {
  HUMID_GUARD_LAST_VGPR();
  const u64 hmask = hbits >= 64 ? ~0ull : ((1ull << hbits) - 1ull);
  const u64 total = (u64)n * k;
  for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (u64)gridDim.x * blockDim.x) {
    const u32 i = (u32)(e / k), j = (u32)(e - (u64)i * k);
    const u64 x = words[(size_t)k * v[i] + j];
    sw[e] = j == 0 ? (x & hmask) : x;
  }
}

__device__ __forceinline__ bool long_eq(const u64 *__restrict__ a, const u64 *__restrict__ b, u32 k) {
  for (u32 j = k; j-- > 0;)                              // neighbours in sorted order share their front: the tail differs first
    if (a[j] != b[j]) return false;
  return true;
}

// head[i] = 1 where a new word starts among the usable reads (the first ctr[CTR_USABLE] positions); head[n] = 0
static __global__ void __launch_bounds__(256)
k_long_heads(const u64 *__restrict__ sw, u32 n, u32 k, const ull *__restrict__ ctr, u32 *__restrict__ head) {
  HUMID_GUARD_LAST_VGPR();
  const u32 usable = (u32)ctr[CTR_USABLE];
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x)
    head[i] = (i < usable && i < n && (i == 0 || !long_eq(sw + (size_t)k * i, sw + (size_t)k * (i - 1), k))) ? 1u : 0u;
}

// k_wide_unique for k uint64 per word: per position the rank of its word and the read tag (bit 31 = filtered); per run
// head the leaf's word, first read and run start
static __global__ void __launch_bounds__(256)
k_long_unique(const u64 *__restrict__ sw, const u32 *v, const u32 *__restrict__ head, const u32 *__restrict__ hpos, u32 n,
              u32 k, const ull *__restrict__ ctr, u64 *__restrict__ s_word, u32 *__restrict__ s_first,
              u32 *__restrict__ start, u32 *__restrict__ pslot, u32 *vals) {
  HUMID_GUARD_LAST_VGPR();
  const u32 usable = (u32)ctr[CTR_USABLE];
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const u32 r = v[i];
    if (i < usable) {
      const u32 h = head[i];
      const u32 rank = hpos[i] + h - 1u;
      pslot[i] = rank;
      vals[i] = r;
      if (h) {
        for (u32 j = 0; j < k; j++) s_word[(size_t)k * rank + j] = sw[(size_t)k * i + j];
        s_first[rank] = r;
        start[rank] = i;
      }
    } else {
      pslot[i] = NOSLOT;
      vals[i] = r | 0x80000000u;
    }
    if (i == 0) start[hpos[n]] = usable < n ? usable : n;
  }
}

// bits [b, b + w) of a leaf read as one string of 64 k bits, most significant first; 1 <= w <= 64, b + w <= 64 k
__device__ __forceinline__ u64 long_bits(const u64 *__restrict__ p, u32 b, u32 w) {
  const u32 q = b >> 6, o = b & 63u;
  u64 x = p[q] << o;
  if (o + w > 64) x |= p[q + 1] >> (64 - o);             // (o > 0 here)
  return x >> (64 - w);
}

// the join key of every leaf for the segment [bit0, bit0 + nbits) of the bit string: the segment itself where it fits
// 64 bits, else a 64-bit mix of its 64-bit pieces; masked to kmask.  val = the leaf index.
static __global__ void __launch_bounds__(256)
k_long_seg_keys(const u64 *__restrict__ leaf, u32 U, u32 k, u32 bit0, u32 nbits, u64 kmask, u64 *__restrict__ key,
                u32 *__restrict__ val) {
  HUMID_GUARD_LAST_VGPR();
  const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const u64 *p = leaf + (size_t)k * u;
  u64 h = 0;
  if (nbits <= 64) h = nbits ? long_bits(p, bit0, nbits) : 0ull;
  else
    for (u32 off = 0; off < nbits; off += 64) {
      const u32 w = nbits - off < 64 ? nbits - off : 64u;
      h = mix64(h ^ long_bits(p, bit0 + off, w)) + off;
    }
  key[u] = h & kmask;
  val[u] = u;
}

// Hamming distance over all k uint64 <= distance?  Leaves as soon as it is exceeded.
__device__ __forceinline__ bool long_within(const u64 *__restrict__ a, const u64 *__restrict__ b, u32 k, u32 distance) {
  u32 d = 0;
  for (u32 j = 0; j < k; j++) {
    d += nt_mismatch(a[j] ^ b[j]);
    if (d > distance) return false;
  }
  return true;
}

// The join of the sorted keys K (leaf V) with themselves, one lane per entry t: its candidates are the entries behind
// it with the same key.  COUNT: pc[t] = pairs found, cand[LONG_CAND_SLOTS] += candidates verified; FILL: (smaller leaf << 32 | larger)
// from poff[t].  walk / big: an entry with more than `walk` followers of its key is not walked by one lane -- the
// COUNT pass raises *big and the caller takes the join through k_edit_chunks / k_long_join_chunks.
template <bool FILL, class KeyT>
__global__ void __launch_bounds__(256)
k_long_join(const KeyT *__restrict__ K, const u32 *__restrict__ V, u32 n, const u64 *__restrict__ leaf, u32 k, u32 distance,
            u32 *__restrict__ pc, const u32 *__restrict__ poff, u64 *__restrict__ edges, u32 walk, ull *big, ull *cand) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ ull lsum;
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  ull tried = 0;
  if (t < n) {
    const KeyT key = K[t];
    if (!FILL && walk && (u64)t + walk < n && K[t + walk] == key) { atomicOr(big, 1ull); pc[t] = 0; }
    else {
      const u32 rx = V[t];
      const u64 *wx = leaf + (size_t)k * rx;
      u32 found = 0;
      u64 e = FILL ? (u64)poff[t] : 0;
      for (u32 j = t + 1; j < n && K[j] == key; j++) {
        const u32 ry = V[j];
        tried++;
        if (!long_within(wx, leaf + (size_t)k * ry, k, distance)) continue;
        if (FILL) edges[e++] = rx < ry ? (((u64)rx << 32) | ry) : (((u64)ry << 32) | rx);
        else found++;
      }
      if (!FILL) pc[t] = found;
    }
  }
  if (!FILL) long_block_add(tried, &lsum, cand);
}

// one lane per piece of k_edit_chunks (run_lo = start of the entry's run, chunk_off = exclusive scan of the pieces per
// entry, n + 1 entries): the piece's candidates behind the entry itself
template <bool FILL, class KeyT>
__global__ void __launch_bounds__(256)
k_long_join_chunks(const KeyT *__restrict__ K, const u32 *__restrict__ V, u32 n, const u32 *__restrict__ run_lo,
                   const u32 *__restrict__ chunk_off, u32 n_pieces, u32 walk, const u64 *__restrict__ leaf, u32 k,
                   u32 distance, u32 *__restrict__ pc, const u32 *__restrict__ poff, u64 *__restrict__ edges, ull *cand) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ ull lsum;
  const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
  ull tried = 0;
  if (p < n_pieces) {
    u32 lo = 0, hi = n;                                  // the entry of this piece: largest t with chunk_off[t] <= p
    while (hi - lo > 1) {
      const u32 mid = lo + ((hi - lo) >> 1);
      if (chunk_off[mid] <= p) lo = mid; else hi = mid;
    }
    const u32 t = lo;
    const KeyT key = K[t];
    const u32 rx = V[t];
    const u64 *wx = leaf + (size_t)k * rx;
    const u64 j0 = (u64)run_lo[t] + (u64)(p - chunk_off[t]) * walk;
    u32 found = 0;
    u64 e = FILL ? (u64)poff[p] : 0;
    for (u64 j = j0 > t ? j0 : (u64)t + 1; j < n && j - j0 < walk && K[j] == key; j++) {
      const u32 ry = V[j];
      tried++;
      if (!long_within(wx, leaf + (size_t)k * ry, k, distance)) continue;
      if (FILL) edges[e++] = rx < ry ? (((u64)rx << 32) | ry) : (((u64)ry << 32) | rx);
      else found++;
    }
    if (!FILL) pc[p] = found;
  }
  if (!FILL) long_block_add(tried, &lsum, cand);
}

#endif  // HUMID_KERNELS_LONG_HIP_H
