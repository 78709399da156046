// kernels_gkey.hip.h -- grouped runs (humid_dedup_run_grouped*): every read's internal word is its group ("gkey")
// in the gnt nucleotides above the caller's word_nt nucleotides.  The count stage then sorts the unique words into
// (group, word) walk order, and make_plan puts the whole group field into every combination, so the rest of the
// pass runs unchanged over word_nt + gnt nucleotides.
#ifndef HUMID_KERNELS_GKEY_HIP_H
#define HUMID_KERNELS_GKEY_HIP_H

#include "common.hip.h"

__device__ __forceinline__ unsigned __int128 gk_wide(u64 w) { return w; }
__device__ __forceinline__ unsigned __int128 gk_wide(W2 w) { return ((unsigned __int128)w.hi << 64) | w.lo; }
__device__ __forceinline__ void gk_put(u64 *out, unsigned __int128 v) { *out = (u64)v; }
__device__ __forceinline__ void gk_put(W2 *out, unsigned __int128 v) { *out = W2{(u64)(v >> 64), (u64)v}; }

// WI: the caller's word (u64 up to 32 nt, W2 beyond), WO: the internal word (u64 while word_nt + gnt <= 32).
// A usable read whose group is >= n_groups stores `epoch` into *bad (one lane per wave; *bad is the host-mapped
// counter mirror the next host wait reads, or a device word); its internal word keeps only the field's bits, so
// the pass stays in bounds until the host refuses its result.  Filtered reads are never counted: their group is
// not read.  out == null (one group: the internal words ARE the caller's): the groups are only checked.
template <class WI, class WO>
__global__ void k_gkey_words(const WI *__restrict__ words, const u32 *__restrict__ group, const u8 *__restrict__ filt,
                             u32 n, u32 word_nt, u32 gnt, u32 n_groups, WO *__restrict__ out, u32 *bad, u32 epoch) {
  HUMID_GUARD_LAST_VGPR();
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  bool wrong = false;
  if (i < n) {
    const u32 g = filt[i] == 0 ? group[i] : 0u;
    wrong = g >= n_groups;
    if (out) {
      unsigned __int128 v = gk_wide(words[i]);
      if (gnt) {
        const u32 wb = 2 * word_nt, gb = 2 * gnt;                  // wb <= 126, gb <= 32
        const unsigned __int128 wmask = ((unsigned __int128)1 << wb) - 1;
        v = (v & wmask) | ((unsigned __int128)((u64)g & ((1ull << gb) - 1)) << wb);
      }
      gk_put(&out[i], v);
    }
  }
  const u64 lanes = __ballot(wrong);
  if (lanes && (threadIdx.x & 63u) == (u32)(__ffsll((long long)lanes) - 1)) {
    __hip_atomic_store(bad, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
  }
}

#endif  // HUMID_KERNELS_GKEY_HIP_H
