// kernels_keyrank.hip.h -- keyed runs (humid_dedup_run_keyed*): every usable read's 64-bit key is replaced by its
// RANK among the distinct keys of the usable reads, on the device, and the rank is written straight into the group
// field of the read's internal word (kernels_gkey.hip.h), so that the grouped pass runs over it unchanged.
//   k_kr_insert   distinct keys -> an open-address table in HBM (one probe per run of equal keys inside a wave)
//   k_kr_compact  occupied slots -> (key, slot) list, their number and the OR of the keys (sort width)
//   (rs_sort, prims.hip.h: the G distinct keys, G-proportional)
//   k_kr_ranks    sorted position -> the key's slot
//   k_kr_words    per read: look the rank up, write the internal word
// Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_KEYRANK_HIP_H
#define HUMID_KERNELS_KEYRANK_HIP_H

#include "common.hip.h"
#include "kernels_gkey.hip.h"

// One 16-byte slot per distinct key: the probe and the rank lookup touch one line.  A 0xff memset empties the
// table: key = EMPTY_KEY, used = rank = 0xffffffff.  Slots [0, cap) are claimed by a compare-and-swap on the key;
// the key that EQUALS EMPTY_KEY lives in the reserved slot `cap`, whose occupancy is its `used` word and not a key
// value: every 64-bit value is a legal key.
struct __attribute__((aligned(16))) KrSlot {
  u64 key;
  u32 used;    // slot `cap` only: 0 once the key EMPTY_KEY was seen
  u32 rank;    // position of the key among the sorted distinct keys (k_kr_ranks)
};

// lanes of the wave whose read starts a run of equal keys: usable, and the lane before it (lane 0: nothing) is
// filtered or holds another key.  A run of equal keys costs its head lane one probe.
__device__ __forceinline__ bool kr_run_head(u64 key, bool usable, u32 lane) {
  const u32 plo = (u32)__shfl_up((int)(u32)key, 1);
  const u32 phi = (u32)__shfl_up((int)(u32)(key >> 32), 1);
  const int pus = __shfl_up((int)usable, 1);
  return usable && (lane == 0 || !pus || (((u64)phi << 32) | plo) != key);
}

// the first probe position of a key in a table of 2^cap_log2 slots (cap_log2 >= 1)
__device__ __forceinline__ u32 kr_home(u64 key, u32 cap_log2) { return (u32)(mix64(key) >> (64 - cap_log2)); }

// ctr[CTR_OVERFULL] = 1 when a key found no slot within max_probe steps: the host repeats the ranking with a larger
// table (the last size, cap >= 2 n_reads, always has room: max_probe is then cap itself).
static __global__ void __launch_bounds__(256)
k_kr_insert(const u64 *__restrict__ key, const u8 *__restrict__ filt, u32 n, KrSlot *tab, u32 cap_log2, u32 max_probe,
            ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  const u32 cap = 1u << cap_log2, mask = cap - 1u, lane = threadIdx.x & 63u;
  const u32 n_up = (n + 63u) & ~63u;                               // whole waves stay in the loop: the shuffles need every lane
  for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < n_up; r += gridDim.x * blockDim.x) {
    if (*(volatile ull *)&ctr[CTR_OVERFULL]) return;                // too small already: the pass is repeated anyway
    const bool usable = r < n && filt[r] == 0;
    const u64 k = usable ? key[r] : 0ull;
    if (!kr_run_head(k, usable, lane)) continue;
    if (k == EMPTY_KEY) { tab[cap].used = 0u; continue; }
    u32 s = kr_home(k, cap_log2) & mask, probes = 0;
    while (true) {
      u64 t = tab[s].key;
      if (t == EMPTY_KEY) t = atomicCAS((ull *)&tab[s].key, EMPTY_KEY, (ull)k);
      if (t == EMPTY_KEY || t == k) break;
      s = (s + 1u) & mask;
      if (++probes > max_probe) { ctr[CTR_OVERFULL] = 1; break; }   // never spin forever
    }
  }
}

__device__ __forceinline__ bool kr_occupied(const KrSlot *tab, u32 s, u32 cap) {
  return s < cap ? tab[s].key != EMPTY_KEY : tab[s].used == 0u;
}

// occupied slots of tab[0 .. cap] -> keys[] / slots[] in arbitrary order (they are sorted next).  A fixed small grid:
// a block counts its chunk, reserves its output with ONE atomic and writes in a second pass over the chunk
// (kernels_count.hip.h, k_compact_table).  ctr[CTR_UNIQUE] = the number of distinct keys, ctr[CTR_KEYBITS] = the OR
// of all of them.  Nothing is written at or beyond out_cap (the count still runs on: the host refuses it).
static __global__ void __launch_bounds__(256)
k_kr_compact(const KrSlot *__restrict__ tab, u32 cap, u64 *__restrict__ keys, u32 *__restrict__ slots, u32 out_cap,
             ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 lds[8];
  const u32 n_slots = cap + 1u;
  const u32 chunk = (n_slots + gridDim.x - 1) / gridDim.x;
  const u32 lo = blockIdx.x * chunk;
  const u32 hi = (lo + chunk < n_slots) ? lo + chunk : n_slots;
  u32 mine = 0;
  for (u32 s = lo + threadIdx.x; s < hi; s += 256) mine += kr_occupied(tab, s, cap) ? 1u : 0u;
  const u32 total = block_sum(mine, lds);
  if (total == 0) return;                                           // (uniform over the block)
  if (threadIdx.x == 0) lds[4] = (u32)atomicAdd(&ctr[CTR_UNIQUE], (ull)total);
  __syncthreads();
  u32 base = lds[4];
  __syncthreads();
  u64 bits = 0;
  for (u32 s0 = lo; s0 < hi; s0 += 256) {
    const u32 s = s0 + threadIdx.x;
    const bool occ = s < hi && kr_occupied(tab, s, cap);
    u32 here;
    const u32 at = base + block_rank(occ, lds, &here);
    if (occ && at < out_cap) {
      const u64 k = s < cap ? tab[s].key : EMPTY_KEY;
      keys[at] = k;
      slots[at] = s;
      bits |= k;
    }
    base += here;
  }
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) {
    const u32 blo = (u32)__shfl_xor((int)(u32)bits, d), bhi = (u32)__shfl_xor((int)(u32)(bits >> 32), d);
    bits |= ((u64)bhi << 32) | blo;
  }
  if ((threadIdx.x & 63u) == 0 && bits) atomicOr(&ctr[CTR_KEYBITS], (ull)bits);
}

// sorted position i -> the rank word of the key's slot
static __global__ void __launch_bounds__(256)
k_kr_ranks(const u32 *__restrict__ slot_sorted, u32 n_keys, KrSlot *tab, u32 cap) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_keys) return;
  const u32 s = slot_sorted[i];
  if (s <= cap) tab[s].rank = i;
}

// Per read: the rank of its key (one lookup per run of equal keys inside a wave, handed to the run's other lanes)
// and the internal word, the rank in the gnt nucleotides above the caller's word_nt: what k_gkey_words writes from a
// group array, without the array.  Filtered reads get rank 0 (their key is not read).  A key the table does not
// hold, or a rank >= n_keys, cannot happen after a complete insert pass; it is range-checked all the same: the
// read gets rank 0 and `epoch` is stored into *bad (as in k_gkey_words), which the host refuses at the count
// stage's wait.
template <class WI, class WO>
__global__ void __launch_bounds__(256)
k_kr_words(const WI *__restrict__ words, const u64 *__restrict__ key, const u8 *__restrict__ filt, u32 n,
           const KrSlot *__restrict__ tab, u32 cap_log2, u32 n_keys, u32 word_nt, u32 gnt, WO *__restrict__ out,
           u32 *bad, u32 epoch) {
  HUMID_GUARD_LAST_VGPR();
  const u32 cap = 1u << cap_log2, mask = cap - 1u, lane = threadIdx.x & 63u;
  const u32 r = blockIdx.x * blockDim.x + threadIdx.x;              // (the grid covers whole waves; no lane leaves early)
  const bool usable = r < n && filt[r] == 0;
  const u64 k = usable ? key[r] : 0ull;
  const bool head = kr_run_head(k, usable, lane);
  u32 rank = 0;
  bool wrong = false;
  if (head) {
    u32 s = cap;
    if (k != EMPTY_KEY) {
      s = kr_home(k, cap_log2) & mask;
      u32 probes = 0;
      while (true) {
        const u64 t = tab[s].key;
        if (t == k) break;
        s = (s + 1u) & mask;
        if (t == EMPTY_KEY || ++probes > cap) { s = NOSLOT; break; }
      }
    }
    rank = s == NOSLOT ? NONE32 : tab[s].rank;
    if (rank >= n_keys) { wrong = true; rank = 0; }
  }
  if (wrong) {
    __hip_atomic_store(bad, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
  }
  // every lane of a run takes the rank of the run's head: the nearest head at or below it
  const u64 heads = __ballot(head);
  const u64 below = heads & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
  const int src = below ? 63 - __clzll((long long)below) : (int)lane;
  rank = (u32)__shfl((int)rank, src);
  if (r >= n) return;
  if (!usable) rank = 0;
  const u32 wb = 2 * word_nt, gb = 2 * gnt;                         // wb <= 126, 2 <= gb <= 32
  const unsigned __int128 wmask = ((unsigned __int128)1 << wb) - 1;
  const unsigned __int128 v = (gk_wide(words[r]) & wmask) | ((unsigned __int128)((u64)rank & ((1ull << gb) - 1)) << wb);
  gk_put(&out[r], v);
}

#endif  // HUMID_KERNELS_KEYRANK_HIP_H
