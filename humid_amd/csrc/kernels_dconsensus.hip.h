// kernels_dconsensus.hip.h -- one DUPLEX consensus record per cluster (humid_duplex_consensus*, include/humid_hip.h):
// the pass of kernels_consensus.hip.h with two classes of voters instead of one.  The members of the representative's
// strand (class X) vote with their record of the same layer S, the members of the other strand (class Y) with their
// record of the other layer O; each class makes a capped call of its own and dcons_decide combines the two.  All sums
// are integers, so the result does not depend on the order the members are taken in.
//   k_dcons_rep     k_cons_rep plus: the TOP members per cluster, both layers' `off`, the strand byte of every member
//   ConsLenIn, k_cons_big_list   (kernels_consensus.hip.h, unchanged) out_off over layer S; the large clusters
//   k_dcons_scatter read indices grouped by cluster, TOP members from the front of the cluster's range and BOTTOM
//                   members from its back: the two classes are two contiguous sub-ranges
//   k_dcons_small   one wave per cluster of at most CONS_BIG reads: two loops, one per class and layer
//   k_dcons_piece   one workgroup per piece of a large cluster, its range split at the class boundary: partial sums into
//                   the cluster's table of 16 u32 per column (u32 atomics)
//   k_dcons_final   one workgroup per large cluster decides its columns from the table
// Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_DCONSENSUS_HIP_H
#define HUMID_KERNELS_DCONSENSUS_HIP_H

#include "kernels_consensus.hip.h"

// the pass's u64 counters: those of the plain pass (ConsLenIn, k_cons_big_list and cons_valid read them) and five more.
// CONS_ERR takes one more bit here, 5: a member whose strand is neither TOP nor BOTTOM.
enum { DCONS_DUPLEX = CONS_CTRS /* clusters with both classes */, DCONS_BOTH /* columns both classes call */,
       DCONS_DISAGREE /* ... with different bases */, DCONS_MASKED /* columns with votes that come out as N */, DCONS_CTRS = 16 };
// k_dcons_small adds its eight workgroup sums to two runs of four counters: their order is part of the kernel
static_assert(CONS_CHANGED == CONS_MULTI + 1 && CONS_VOTES == CONS_MULTI + 2 && CONS_ERRORS == CONS_MULTI + 3, "k_dcons_small: counter order");
static_assert(DCONS_BOTH == DCONS_DUPLEX + 1 && DCONS_DISAGREE == DCONS_DUPLEX + 2 && DCONS_MASKED == DCONS_DUPLEX + 3, "k_dcons_small: counter order");
static_assert(DCONS_MASKED < DCONS_CTRS, "the duplex counters fit");
#define DCONS_STRAND_TOP 0u       // HUMID_STRAND_TOP / _BOTTOM of include/humid_hip.h (passes.hip.h asserts it)
#define DCONS_STRAND_BOTTOM 1u

// k_cons_rep for two layers: top[c] = the members of cluster c with strand TOP (cnt[c] = all of them); off_s and off_o
// are checked for EVERY read, the strand byte for every member (an id of 0 or above C: not read).
static __global__ void __launch_bounds__(256)
k_dcons_rep(const u32 *__restrict__ cid, const u8 *__restrict__ keep, const u8 *__restrict__ strand, const u64 *__restrict__ off_s,
            const u64 *__restrict__ off_o, u32 n, u64 n_bytes_s, u64 n_bytes_o, u32 C, u32 *rep, u32 *cnt, u32 *top, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  const u32 n_up = (n + 63u) & ~63u;
  u32 claims = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && (off_s[n] > n_bytes_s || off_o[n] > n_bytes_o)) atomicOr(&ctr[CONS_ERR], 8ull);
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += gridDim.x * blockDim.x) {
    bool claim = false;
    if (i < n) {
      const u32 c = cid[i];
      if (off_s[i] > off_s[i + 1] || off_o[i] > off_o[i + 1]) atomicOr(&ctr[CONS_ERR], 4ull);
      if (c > C) atomicOr(&ctr[CONS_ERR], 1ull);
      else if (c != 0) {
        const u32 s = strand[i];
        atomicAdd(&cnt[c], 1u);
        if (s == DCONS_STRAND_TOP) atomicAdd(&top[c], 1u);
        else if (s != DCONS_STRAND_BOTTOM) atomicOr(&ctr[CONS_ERR], 32ull);
        if (keep[i] != 0) {
          claim = true;
          if (atomicCAS(&rep[c], NONE32, i) != NONE32) atomicOr(&ctr[CONS_ERR], 2ull);
        }
      }
    }
    claims += (u32)__popcll(__ballot(claim));
  }
  if ((threadIdx.x & 63u) == 0 && claims) atomicAdd(&ctr[CONS_CLAIMS], (ull)claims);
}

// cur[2 * c] and cur[2 * c + 1] are zero on entry: the cursor of the TOP members runs up from the front of the cluster's
// range, that of the BOTTOM members down from its back; the two meet at mem_off[c - 1] + top[c] (input checked: every
// member's strand is one of the two).
static __global__ void __launch_bounds__(256)
k_dcons_scatter(const u32 *__restrict__ cid, const u8 *__restrict__ strand, u32 n, const u32 *__restrict__ mem_off, u32 *cur,
                u32 *__restrict__ mem) {
  HUMID_GUARD_LAST_VGPR();
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const u32 c = cid[i];
    if (c == 0) continue;
    if (strand[i] == DCONS_STRAND_TOP) mem[mem_off[c - 1] + atomicAdd(&cur[2 * (size_t)c], 1u)] = i;
    else mem[mem_off[c] - 1u - atomicAdd(&cur[2 * (size_t)c + 1], 1u)] = i;
  }
}

// One class's call from its sums: the base with the largest sum (A before C before G before T, as cons_decide), the
// margin to the second capped at strand_cap_q (0: no votes or a tie -- the class makes no call), its votes and those
// for the called base.
struct DconsCall { u32 base, m, nv, nb; };
__device__ __forceinline__ DconsCall dcons_call(const ConsAcc a, u32 strand_cap_q) {
  const u32 m01 = max(a.s0, a.s1), m23 = max(a.s2, a.s3), best = max(m01, m23);
  const u32 second = max(min(m01, m23), m01 >= m23 ? min(a.s0, a.s1) : min(a.s2, a.s3));
  DconsCall k;
  k.nv = a.n0 + a.n1 + a.n2 + a.n3;
  k.base = a.s0 == best ? 'A' : a.s1 == best ? 'C' : a.s2 == best ? 'G' : 'T';
  k.nb = a.s0 == best ? a.n0 : a.s1 == best ? a.n1 : a.s2 == best ? a.n2 : a.n3;
  k.m = min(best - second, strand_cap_q);
  return k;
}

// The column's output from the sums of the two classes and the representative's own bytes (the table of
// include/humid_hip.h): two calls of one base add their margins, two calls of different bases subtract them.
struct DconsOut { u32 base, qual, votes, errs, changed, both, disagree, masked; };
__device__ __forceinline__ DconsOut dcons_decide(const ConsAcc x, const ConsAcc y, u32 rb, u32 rq, u32 strand_cap_q, u32 cap_q) {
  const DconsCall kx = dcons_call(x, strand_cap_q), ky = dcons_call(y, strand_cap_q);
  const bool cx = kx.m != 0, cy = ky.m != 0, both = cx && cy;
  u32 base = 'N', m = 0;
  if (both) {
    if (kx.base == ky.base) { base = kx.base; m = kx.m + ky.m; }
    else if (kx.m != ky.m) { base = kx.m > ky.m ? kx.base : ky.base; m = kx.m > ky.m ? kx.m - ky.m : ky.m - kx.m; }
  } else if (cx) { base = kx.base; m = kx.m; }
  else if (cy) { base = ky.base; m = ky.m; }
  DconsOut o;
  o.votes = kx.nv + ky.nv;
  o.errs = (cx ? kx.nv - kx.nb : 0u) + (cy ? ky.nv - ky.nb : 0u);
  o.both = both ? 1u : 0u;
  o.disagree = both && kx.base != ky.base ? 1u : 0u;
  o.masked = 0;
  if (o.votes == 0) { o.base = rb; o.qual = rq; }                        // verbatim
  else if (m == 0) { o.base = 'N'; o.qual = '!'; o.masked = 1; }         // no class calls, or two equal calls of different bases
  else { o.base = base; o.qual = 33u + (m < cap_q ? m : cap_q); }
  o.changed = o.base != rb ? 1u : 0u;
  return o;
}

// The votes of the members at positions [lo, hi) of a cluster's list (m0 its start in mem) at this lane's column, taken
// from one layer: 64 byte ranges per step, broadcast by cons_vote_batch.  The range and the layer are wave-uniform.
__device__ __forceinline__ void dcons_vote_range(ConsAcc &a, const u8 *__restrict__ bases, const u8 *__restrict__ quals,
                                                 const u64 *__restrict__ off, const u32 *__restrict__ mem, u32 m0, u32 lo, u32 hi,
                                                 u32 lane, u64 col, bool in, u32 min_q1) {
  for (u32 t0 = lo; t0 < hi; t0 += 64) {
    const u32 tn = hi - t0 < 64u ? hi - t0 : 64u;
    u64 mo = 0, ml = 0;
    if (lane < tn) { const u32 i = mem[m0 + t0 + lane]; mo = off[i]; ml = off[i + 1] - mo; }
    cons_vote_batch(a, bases, quals, mo, ml, tn, col, in, min_q1);
  }
}

// k_cons_small with two classes: one wave per cluster c = 1 + global wave index, lanes over 64 columns per step, two
// sets of eight sums per lane.  Class X, the representative's strand, is one sub-range of the cluster's list and votes
// from layer S; class Y is the other and votes from layer O.  A singleton follows no list.
// depth / depth_same / depth_other / disagree / errors [c - 1] per cluster; the eight summary counters by one atomic
// each per workgroup.
static __global__ void __launch_bounds__(256)
k_dcons_small(const u8 *__restrict__ bases_s, const u8 *__restrict__ quals_s, const u64 *__restrict__ off_s,
              const u8 *__restrict__ bases_o, const u8 *__restrict__ quals_o, const u64 *__restrict__ off_o,
              const u8 *__restrict__ strand, const u32 *__restrict__ rep, const u32 *__restrict__ top, const u32 *__restrict__ mem_off,
              const u32 *__restrict__ mem, const u64 *__restrict__ out_off, u32 C, u32 min_q1, u32 strand_cap_q, u32 cap_q,
              u8 *__restrict__ ob, u8 *__restrict__ oq, u32 *__restrict__ depth, u32 *__restrict__ depth_same,
              u32 *__restrict__ depth_other, u32 *__restrict__ disagree, u64 *__restrict__ errors, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 lds[4][8];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u64 cw = (u64)blockIdx.x * 4u + wave + 1u;
  u32 votes = 0, errs = 0, changed = 0, multi = 0, duplex = 0, both = 0, dis = 0, masked = 0;
  if (cw <= C) {                                                // (uniform per wave)
    const u32 c = (u32)cw;
    const u32 m0 = mem_off[c - 1], d = mem_off[c] - m0;
    if (d <= CONS_BIG) {
      const u32 r = rep[c], nt = top[c];
      const bool rtop = strand[r] == DCONS_STRAND_TOP;
      const u32 x0 = rtop ? 0u : nt, x1 = rtop ? nt : d, y0 = rtop ? nt : 0u, y1 = rtop ? d : nt;
      const u64 ro = off_s[r], L = off_s[r + 1] - ro, oo = out_off[c - 1];
      multi = d >= 2 ? 1u : 0u;
      duplex = y1 != y0 ? 1u : 0u;                               // (class X holds the representative)
      u32 cl_err = 0, cl_dis = 0;
      for (u64 j0 = 0; j0 < L; j0 += 64) {
        const u64 col = j0 + lane;
        const bool in = col < L;
        const u8 rb = in ? bases_s[ro + col] : (u8)0, rq = in ? quals_s[ro + col] : (u8)0;
        ConsAcc x, y;
        x.clear();
        y.clear();
        if (d == 1) { if (in) x.vote(rb, rq, min_q1); }
        else {
          dcons_vote_range(x, bases_s, quals_s, off_s, mem, m0, x0, x1, lane, col, in, min_q1);
          dcons_vote_range(y, bases_o, quals_o, off_o, mem, m0, y0, y1, lane, col, in, min_q1);
        }
        if (in) {
          const DconsOut o = dcons_decide(x, y, rb, rq, strand_cap_q, cap_q);
          ob[oo + col] = (u8)o.base; oq[oo + col] = (u8)o.qual;
          votes += o.votes; changed += o.changed; cl_err += o.errs; cl_dis += o.disagree; both += o.both; masked += o.masked;
        }
      }
      cl_err = cons_wave_sum(cl_err);
      cl_dis = cons_wave_sum(cl_dis);
      errs = lane == 0 ? cl_err : 0u;
      dis = lane == 0 ? cl_dis : 0u;
      if (lane == 0) {
        depth[c - 1] = d; depth_same[c - 1] = x1 - x0; depth_other[c - 1] = y1 - y0; disagree[c - 1] = cl_dis; errors[c - 1] = cl_err;
      }
    }
  }
  votes = cons_wave_sum(votes);
  changed = cons_wave_sum(changed);
  both = cons_wave_sum(both);
  masked = cons_wave_sum(masked);
  if (lane == 0) {
    lds[wave][0] = multi; lds[wave][1] = changed; lds[wave][2] = votes; lds[wave][3] = errs;
    lds[wave][4] = duplex; lds[wave][5] = both; lds[wave][6] = dis; lds[wave][7] = masked;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const u32 t = lds[0][threadIdx.x] + lds[1][threadIdx.x] + lds[2][threadIdx.x] + lds[3][threadIdx.x];
    // (CONS_MULTI .. CONS_ERRORS are 5 .. 8, DCONS_DUPLEX .. DCONS_MASKED 10 .. 13)
    if (t) atomicAdd(&ctr[threadIdx.x < 4 ? CONS_MULTI + threadIdx.x : DCONS_DUPLEX + threadIdx.x - 4u], (ull)t);
  }
}

__device__ __forceinline__ void dcons_tab_add(u32 *t8, u64 L, u64 col, const ConsAcc &a) {
  if (a.n0) { atomicAdd(&t8[0 * L + col], a.s0); atomicAdd(&t8[4 * L + col], a.n0); }
  if (a.n1) { atomicAdd(&t8[1 * L + col], a.s1); atomicAdd(&t8[5 * L + col], a.n1); }
  if (a.n2) { atomicAdd(&t8[2 * L + col], a.s2); atomicAdd(&t8[6 * L + col], a.n2); }
  if (a.n3) { atomicAdd(&t8[3 * L + col], a.s3); atomicAdd(&t8[7 * L + col], a.n3); }
}

// k_cons_piece with two classes: a wave's 256 positions [lo, hi) of the cluster's list are split at the class boundary
// top[c]; the TOP part and the BOTTOM part each vote from the layer their class reads and add to their class's half of
// the table tab[(first column * 16) + (class * 8 + q) * L + column].
static __global__ void __launch_bounds__(256)
k_dcons_piece(const u8 *__restrict__ bases_s, const u8 *__restrict__ quals_s, const u64 *__restrict__ off_s,
              const u8 *__restrict__ bases_o, const u8 *__restrict__ quals_o, const u64 *__restrict__ off_o,
              const u8 *__restrict__ strand, const u32 *__restrict__ rep, const u32 *__restrict__ top, const u32 *__restrict__ mem_off,
              const u32 *__restrict__ mem, const u64 *__restrict__ out_off, const ConsBig *__restrict__ big,
              const ConsPiece *__restrict__ piece, u32 min_q1, u32 *tab) {
  HUMID_GUARD_LAST_VGPR();
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const ConsPiece pc = piece[blockIdx.x];
  const ConsBig bg = big[pc.big];
  const u32 c = bg.c, m0 = mem_off[c - 1], d = mem_off[c] - m0, nt = top[c];
  const u64 L = out_off[c] - out_off[c - 1];
  const u32 lo = pc.k * CONS_PIECE + wave * (CONS_PIECE / 4u);
  if (lo >= d) return;                                          // (uniform per wave; no barrier below)
  const u32 hi = lo + CONS_PIECE / 4u < d ? lo + CONS_PIECE / 4u : d;
  const bool rtop = strand[rep[c]] == DCONS_STRAND_TOP;
  // the TOP positions [lo, th) and the BOTTOM positions [th, hi) of this wave; the class of the representative's
  // strand reads layer S and the first half of the table
  const u32 th = nt < lo ? lo : nt > hi ? hi : nt;
  u32 *t16 = tab + bg.tab * 16u;
  u32 *t_top = t16 + (rtop ? 0u : 8u) * L, *t_bot = t16 + (rtop ? 8u : 0u) * L;
  const u8 *b_top = rtop ? bases_s : bases_o, *q_top = rtop ? quals_s : quals_o;
  const u8 *b_bot = rtop ? bases_o : bases_s, *q_bot = rtop ? quals_o : quals_s;
  const u64 *o_top = rtop ? off_s : off_o, *o_bot = rtop ? off_o : off_s;
  for (u64 j0 = 0; j0 < L; j0 += 64) {
    const u64 col = j0 + lane;
    const bool in = col < L;
    ConsAcc a, b;
    a.clear();
    b.clear();
    dcons_vote_range(a, b_top, q_top, o_top, mem, m0, lo, th, lane, col, in, min_q1);
    dcons_vote_range(b, b_bot, q_bot, o_bot, mem, m0, th, hi, lane, col, in, min_q1);
    if (in) {
      dcons_tab_add(t_top, L, col, a);
      dcons_tab_add(t_bot, L, col, b);
    }
  }
}

__device__ __forceinline__ u64 dcons_wave_sum64(u64 x) {
#pragma unroll
  for (u32 s = 32; s >= 1; s >>= 1) x += ((u64)(u32)__shfl_xor((int)(u32)(x >> 32), (int)s) << 32) | (u32)__shfl_xor((int)(u32)x, (int)s);
  return x;
}

// One workgroup per large cluster: threads over its columns.
static __global__ void __launch_bounds__(256)
k_dcons_final(const u8 *__restrict__ bases_s, const u8 *__restrict__ quals_s, const u64 *__restrict__ off_s,
              const u8 *__restrict__ strand, const u32 *__restrict__ rep, const u32 *__restrict__ top, const u32 *__restrict__ mem_off,
              const u64 *__restrict__ out_off, const ConsBig *__restrict__ big, const u32 *__restrict__ tab, u32 strand_cap_q,
              u32 cap_q, u8 *__restrict__ ob, u8 *__restrict__ oq, u32 *__restrict__ depth, u32 *__restrict__ depth_same,
              u32 *__restrict__ depth_other, u32 *__restrict__ disagree, u64 *__restrict__ errors, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u64 lds[4][6];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const ConsBig bg = big[blockIdx.x];
  const u32 c = bg.c, r = rep[c];
  const u64 ro = off_s[r], L = off_s[r + 1] - ro, oo = out_off[c - 1];
  const u32 *t16 = tab + bg.tab * 16u;
  u64 v[6] = {0, 0, 0, 0, 0, 0};                                 // changed, votes, errors, both, disagree, masked
  for (u64 col = threadIdx.x; col < L; col += 256) {
    ConsAcc x, y;
    x.s0 = t16[0 * L + col]; x.s1 = t16[1 * L + col]; x.s2 = t16[2 * L + col]; x.s3 = t16[3 * L + col];
    x.n0 = t16[4 * L + col]; x.n1 = t16[5 * L + col]; x.n2 = t16[6 * L + col]; x.n3 = t16[7 * L + col];
    y.s0 = t16[8 * L + col]; y.s1 = t16[9 * L + col]; y.s2 = t16[10 * L + col]; y.s3 = t16[11 * L + col];
    y.n0 = t16[12 * L + col]; y.n1 = t16[13 * L + col]; y.n2 = t16[14 * L + col]; y.n3 = t16[15 * L + col];
    const DconsOut o = dcons_decide(x, y, bases_s[ro + col], quals_s[ro + col], strand_cap_q, cap_q);
    ob[oo + col] = (u8)o.base; oq[oo + col] = (u8)o.qual;
    v[0] += o.changed; v[1] += o.votes; v[2] += o.errs; v[3] += o.both; v[4] += o.disagree; v[5] += o.masked;
  }
#pragma unroll
  for (u32 k = 0; k < 6; k++) {
    v[k] = dcons_wave_sum64(v[k]);
    if (lane == 0) lds[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t[6];
#pragma unroll
    for (u32 k = 0; k < 6; k++) t[k] = lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k];
    const u32 d = mem_off[c] - mem_off[c - 1], nt = top[c];
    const u32 same = strand[r] == DCONS_STRAND_TOP ? nt : d - nt;
    depth[c - 1] = d; depth_same[c - 1] = same; depth_other[c - 1] = d - same;
    disagree[c - 1] = (u32)t[4];
    errors[c - 1] = t[2];
    atomicAdd(&ctr[CONS_MULTI], 1ull);
    if (t[0]) atomicAdd(&ctr[CONS_CHANGED], (ull)t[0]);
    if (t[1]) atomicAdd(&ctr[CONS_VOTES], (ull)t[1]);
    if (t[2]) atomicAdd(&ctr[CONS_ERRORS], (ull)t[2]);
    if (same != d) atomicAdd(&ctr[DCONS_DUPLEX], 1ull);
    if (t[3]) atomicAdd(&ctr[DCONS_BOTH], (ull)t[3]);
    if (t[4]) atomicAdd(&ctr[DCONS_DISAGREE], (ull)t[4]);
    if (t[5]) atomicAdd(&ctr[DCONS_MASKED], (ull)t[5]);
  }
}

#endif  // HUMID_KERNELS_DCONSENSUS_HIP_H
