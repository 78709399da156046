// kernels_consensus.hip.h -- one consensus record per cluster (humid_consensus*, include/humid_hip.h): a pass AFTER a
// run, over per-read (cluster_id, keep) and the reads themselves (ASCII bases and Phred+33 qualities of one FastQ
// file).  Every read of a cluster votes, per column, for its base with the weight of its quality; the column's output
// is the base with the largest sum and the margin to the second largest as its quality.  All sums are integers, so
// the result does not depend on the order the members are taken in.
//   k_cons_rep      rep[c] = the cluster's one kept read (compare-and-swap, the scheme of k_best_rep), cnt[c] = its
//                   reads; checks the ids, the claims and `off`
//   ConsLenIn       (a scan input) len(r_c) per cluster -> out_off
//   k_cons_big_list the clusters of more than CONS_BIG reads: (cluster, table offset) records and one record per
//                   piece of CONS_PIECE members
//   k_cons_scatter  read indices grouped by cluster: mem[mem_off[c - 1] + cursor]
//   k_cons_small    one wave per cluster of at most CONS_BIG reads: lanes over 64 columns, a loop over the members
//   k_cons_piece    one workgroup per piece of a large cluster: partial sums into the cluster's table (u32 atomics)
//   k_cons_final    one workgroup per large cluster decides its columns from the table
// Part of libhumid_hip.so; device code for gfx950 only.
#ifndef HUMID_KERNELS_CONSENSUS_HIP_H
#define HUMID_KERNELS_CONSENSUS_HIP_H

#include "common.hip.h"

#define CONS_BIG 1024u     // a cluster of more reads than this is cut into pieces (no wave walks a longer list alone)
#define CONS_PIECE 1024u   // members per piece: 256 per wave of k_cons_piece
#define CONS_MAX_DEPTH 46182444u   // 93 * this < 2^32: the u32 sums cannot wrap

// the pass's u64 counters
enum { CONS_ERR = 0 /* bit 0: an id above C; 1: two kept reads in a cluster; 2: off decreasing; 3: off[n] > n_bytes; 4: a cluster beyond CONS_MAX_DEPTH; 5: taken by the duplex pass, kernels_dconsensus.hip.h */,
       CONS_CLAIMS /* kept reads that claimed a cluster */, CONS_NBIG /* large clusters */, CONS_NPIECES /* their pieces */,
       CONS_TABCOLS /* columns of all their tables */, CONS_MULTI, CONS_CHANGED, CONS_VOTES, CONS_ERRORS, CONS_CTRS = 10 };

struct ConsBig { u32 c, pad; u64 tab; };       // a large cluster and the first column of its table
struct ConsPiece { u32 big, k; };              // piece k of large cluster big[]

// Claims as in k_best_rep; beside them the reads of every cluster are counted and off[i] <= off[i + 1] is checked for
// EVERY read (so, with off[n] <= n_bytes, every byte range a later kernel follows lies inside the blobs).
static __global__ void __launch_bounds__(256)
k_cons_rep(const u32 *__restrict__ cid, const u8 *__restrict__ keep, const u64 *__restrict__ off, u32 n, u64 n_bytes, u32 C,
           u32 *rep, u32 *cnt, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  const u32 n_up = (n + 63u) & ~63u;
  u32 claims = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && off[n] > n_bytes) atomicOr(&ctr[CONS_ERR], 8ull);
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += gridDim.x * blockDim.x) {
    bool claim = false;
    if (i < n) {
      const u32 c = cid[i];
      if (off[i] > off[i + 1]) atomicOr(&ctr[CONS_ERR], 4ull);
      if (c > C) atomicOr(&ctr[CONS_ERR], 1ull);
      else if (c != 0) {
        atomicAdd(&cnt[c], 1u);
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

__device__ __forceinline__ bool cons_valid(const ull *__restrict__ ctr, u32 C) { return ctr[CONS_ERR] == 0 && ctr[CONS_CLAIMS] == (ull)C; }

// scan input: item i < C is len(r_c) of cluster c = i + 1, item C is 0.  Malformed input: all 0, no index followed.
struct ConsLenIn {
  const u32 *rep;
  const u64 *off;
  const ull *ctr;
  u32 C;
  __device__ __forceinline__ u64 operator()(u64 i) const {
    if (i >= C || !cons_valid(ctr, C)) return 0;
    const u32 r = rep[i + 1];
    return off[r + 1] - off[r];
  }
};

// Every cluster of more than CONS_BIG reads takes a record, the columns of its table and its piece records.  The
// order of the records is that of the atomics: it decides where the scratch lies, never a result.
static __global__ void __launch_bounds__(256)
k_cons_big_list(const u32 *__restrict__ cnt, const u64 *__restrict__ out_off, u32 C, ConsBig *__restrict__ big,
                ConsPiece *__restrict__ piece, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  if (!cons_valid(ctr, C)) return;
  for (u32 c = 1u + blockIdx.x * blockDim.x + threadIdx.x; c <= C && c != 0; c += gridDim.x * blockDim.x) {
    const u32 d = cnt[c];
    if (d <= CONS_BIG) continue;
    if (d > CONS_MAX_DEPTH) { atomicOr(&ctr[CONS_ERR], 16ull); continue; }
    const u32 np = (d + CONS_PIECE - 1u) / CONS_PIECE;
    const u32 b = (u32)atomicAdd(&ctr[CONS_NBIG], 1ull);
    const u32 p0 = (u32)atomicAdd(&ctr[CONS_NPIECES], (ull)np);
    big[b] = ConsBig{c, 0u, (u64)atomicAdd(&ctr[CONS_TABCOLS], (ull)(out_off[c] - out_off[c - 1]))};
    for (u32 k = 0; k < np; k++) piece[p0 + k] = ConsPiece{b, k};
  }
}

// cur[c] is zero on entry; the place inside a cluster's list is whatever the atomics hand out.
static __global__ void __launch_bounds__(256)
k_cons_scatter(const u32 *__restrict__ cid, u32 n, const u32 *__restrict__ mem_off, u32 *cur, u32 *__restrict__ mem) {
  HUMID_GUARD_LAST_VGPR();
  for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const u32 c = cid[i];
    if (c != 0) mem[mem_off[c - 1] + atomicAdd(&cur[c], 1u)] = i;
  }
}

// eight sums of one column: weight and votes per base
struct ConsAcc {
  u32 s0, s1, s2, s3, n0, n1, n2, n3;
  __device__ __forceinline__ void clear() { s0 = s1 = s2 = s3 = n0 = n1 = n2 = n3 = 0; }
  // one read's byte pair: p = clamp(q - 33, 0, 93); a vote of weight p when the base is A C G T and p >= min_q1 (>= 1)
  __device__ __forceinline__ void vote(u32 b, u32 q, u32 min_q1) {
    u32 p = q < 33u ? 0u : q - 33u;
    p = p > 93u ? 93u : p;
    const bool ok = p >= min_q1;
    const bool a = ok && b == 'A', c = ok && b == 'C', g = ok && b == 'G', t = ok && b == 'T';
    s0 += a ? p : 0u; n0 += a ? 1u : 0u;
    s1 += c ? p : 0u; n1 += c ? 1u : 0u;
    s2 += g ? p : 0u; n2 += g ? 1u : 0u;
    s3 += t ? p : 0u; n3 += t ? 1u : 0u;
  }
};

// The column's output from its sums and the representative's own bytes.
struct ConsOut { u32 base, qual, votes, errs, changed; };
__device__ __forceinline__ ConsOut cons_decide(const ConsAcc a, u32 rb, u32 rq, u32 cap_q) {
  const u32 nv = a.n0 + a.n1 + a.n2 + a.n3;
  const u32 m01 = max(a.s0, a.s1), m23 = max(a.s2, a.s3), best = max(m01, m23);
  const u32 second = max(min(m01, m23), m01 >= m23 ? min(a.s0, a.s1) : min(a.s2, a.s3));
  const u32 base = a.s0 == best ? 'A' : a.s1 == best ? 'C' : a.s2 == best ? 'G' : 'T';
  const u32 nb = a.s0 == best ? a.n0 : a.s1 == best ? a.n1 : a.s2 == best ? a.n2 : a.n3;
  const u32 m = best - second;
  ConsOut o;
  o.votes = nv;
  if (nv == 0) { o.base = rb; o.qual = rq; o.errs = 0; }                  // verbatim
  else if (m == 0) { o.base = 'N'; o.qual = '!'; o.errs = 0; }           // a tie (a base with a vote has a sum >= 1: best > 0)
  else { o.base = base; o.qual = 33u + (m < cap_q ? m : cap_q); o.errs = nv - nb; }
  o.changed = o.base != rb ? 1u : 0u;
  return o;
}

__device__ __forceinline__ u64 cons_shfl64(u64 x, u32 src) {
  return ((u64)(u32)__shfl((int)(u32)(x >> 32), (int)src) << 32) | (u32)__shfl((int)(u32)x, (int)src);
}

// The votes of up to 64 members at this lane's column: lane t < tn holds member t's byte range (mo, ml).  Four members
// per step: their eight loads are issued before the first vote needs one.  All lanes of the wave call this together.
__device__ __forceinline__ void cons_vote_batch(ConsAcc &a, const u8 *__restrict__ bases, const u8 *__restrict__ quals, u64 mo, u64 ml,
                                                u32 tn, u64 col, bool in, u32 min_q1) {
  for (u32 t = 0; t < tn; t += 4) {
    u32 b[4], q[4];
#pragma unroll
    for (u32 k = 0; k < 4; k++) {
      const u64 bo = cons_shfl64(mo, (t + k) & 63u), bl = cons_shfl64(ml, (t + k) & 63u);
      const bool on = in && t + k < tn && col < bl;
      b[k] = on ? bases[bo + col] : 0u;                        // (0 is no base: it casts nothing)
      q[k] = on ? quals[bo + col] : 0u;
    }
#pragma unroll
    for (u32 k = 0; k < 4; k++) a.vote(b[k], q[k], min_q1);
  }
}

__device__ __forceinline__ u32 cons_wave_sum(u32 x) {
#pragma unroll
  for (u32 d = 32; d >= 1; d >>= 1) x += (u32)__shfl_xor((int)x, (int)d);
  return x;
}

// One wave per cluster c = 1 + global wave index, lanes over 64 columns per step, so that one member's bases and
// qualities arrive as coalesced 64-byte rows; registers do not depend on the read length.  A singleton (most clusters)
// follows no member list: its one read is the representative.  Larger clusters take 64 member indices and their byte
// ranges per lane and broadcast them inside the wave.  Clusters beyond CONS_BIG are left to k_cons_piece / _final.
// depth[c - 1], errors[c - 1] per cluster; the four summary counters by one atomic each per workgroup.
static __global__ void __launch_bounds__(256)
k_cons_small(const u8 *__restrict__ bases, const u8 *__restrict__ quals, const u64 *__restrict__ off, const u32 *__restrict__ rep,
             const u32 *__restrict__ mem_off, const u32 *__restrict__ mem, const u64 *__restrict__ out_off, u32 C, u32 min_q1,
             u32 cap_q, u8 *__restrict__ ob, u8 *__restrict__ oq, u32 *__restrict__ depth, u64 *__restrict__ errors, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u32 lds[4][4];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u64 cw = (u64)blockIdx.x * 4u + wave + 1u;
  u32 votes = 0, errs = 0, changed = 0, multi = 0;
  if (cw <= C) {                                                // (uniform per wave)
    const u32 c = (u32)cw;
    const u32 m0 = mem_off[c - 1], d = mem_off[c] - m0;
    if (d <= CONS_BIG) {
      const u32 r = rep[c];
      const u64 ro = off[r], L = off[r + 1] - ro, oo = out_off[c - 1];
      multi = d >= 2 ? 1u : 0u;
      u32 cl_err = 0;
      for (u64 j0 = 0; j0 < L; j0 += 64) {
        const u64 col = j0 + lane;
        const bool in = col < L;
        const u8 rb = in ? bases[ro + col] : (u8)0, rq = in ? quals[ro + col] : (u8)0;
        ConsAcc a;
        a.clear();
        if (d == 1) { if (in) a.vote(rb, rq, min_q1); }
        else {
          for (u32 t0 = 0; t0 < d; t0 += 64) {
            const u32 tn = d - t0 < 64u ? d - t0 : 64u;
            u64 mo = 0, ml = 0;
            if (lane < tn) { const u32 i = mem[m0 + t0 + lane]; mo = off[i]; ml = off[i + 1] - mo; }
            cons_vote_batch(a, bases, quals, mo, ml, tn, col, in, min_q1);
          }
        }
        if (in) {
          const ConsOut o = cons_decide(a, rb, rq, cap_q);
          ob[oo + col] = (u8)o.base; oq[oo + col] = (u8)o.qual;
          votes += o.votes; changed += o.changed; cl_err += o.errs;
        }
      }
      cl_err = cons_wave_sum(cl_err);
      errs = lane == 0 ? cl_err : 0u;
      if (lane == 0) { depth[c - 1] = d; errors[c - 1] = cl_err; }
    }
  }
  votes = cons_wave_sum(votes);
  changed = cons_wave_sum(changed);
  if (lane == 0) { lds[wave][0] = multi; lds[wave][1] = changed; lds[wave][2] = votes; lds[wave][3] = errs; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const u32 t = lds[0][threadIdx.x] + lds[1][threadIdx.x] + lds[2][threadIdx.x] + lds[3][threadIdx.x];
    if (t) atomicAdd(&ctr[CONS_MULTI + threadIdx.x], (ull)t);
  }
}

// One workgroup per piece: its four waves take 256 members each and add, per 64 columns, their eight partial sums to
// the cluster's table tab[(first column * 8) + q * L + column] -- 256 contiguous bytes per atomic instruction.
static __global__ void __launch_bounds__(256)
k_cons_piece(const u8 *__restrict__ bases, const u8 *__restrict__ quals, const u64 *__restrict__ off, const u32 *__restrict__ mem_off,
             const u32 *__restrict__ mem, const u64 *__restrict__ out_off, const ConsBig *__restrict__ big,
             const ConsPiece *__restrict__ piece, u32 min_q1, u32 *tab) {
  HUMID_GUARD_LAST_VGPR();
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const ConsPiece pc = piece[blockIdx.x];
  const ConsBig bg = big[pc.big];
  const u32 c = bg.c, m0 = mem_off[c - 1], d = mem_off[c] - m0;
  const u64 L = out_off[c] - out_off[c - 1];
  const u32 lo = pc.k * CONS_PIECE + wave * (CONS_PIECE / 4u);
  if (lo >= d) return;                                          // (uniform per wave; no barrier below)
  const u32 hi = lo + CONS_PIECE / 4u < d ? lo + CONS_PIECE / 4u : d;
  u32 *t8 = tab + bg.tab * 8u;
  for (u64 j0 = 0; j0 < L; j0 += 64) {
    const u64 col = j0 + lane;
    const bool in = col < L;
    ConsAcc a;
    a.clear();
    for (u32 t0 = lo; t0 < hi; t0 += 64) {
      const u32 tn = hi - t0 < 64u ? hi - t0 : 64u;
      u64 mo = 0, ml = 0;
      if (lane < tn) { const u32 i = mem[m0 + t0 + lane]; mo = off[i]; ml = off[i + 1] - mo; }
      cons_vote_batch(a, bases, quals, mo, ml, tn, col, in, min_q1);
    }
    if (in) {
      if (a.n0) { atomicAdd(&t8[0 * L + col], a.s0); atomicAdd(&t8[4 * L + col], a.n0); }
      if (a.n1) { atomicAdd(&t8[1 * L + col], a.s1); atomicAdd(&t8[5 * L + col], a.n1); }
      if (a.n2) { atomicAdd(&t8[2 * L + col], a.s2); atomicAdd(&t8[6 * L + col], a.n2); }
      if (a.n3) { atomicAdd(&t8[3 * L + col], a.s3); atomicAdd(&t8[7 * L + col], a.n3); }
    }
  }
}

// One workgroup per large cluster: threads over its columns.
static __global__ void __launch_bounds__(256)
k_cons_final(const u8 *__restrict__ bases, const u8 *__restrict__ quals, const u64 *__restrict__ off, const u32 *__restrict__ rep,
             const u32 *__restrict__ mem_off, const u64 *__restrict__ out_off, const ConsBig *__restrict__ big,
             const u32 *__restrict__ tab, u32 cap_q, u8 *__restrict__ ob, u8 *__restrict__ oq, u32 *__restrict__ depth,
             u64 *__restrict__ errors, ull *ctr) {
  HUMID_GUARD_LAST_VGPR();
  __shared__ u64 lds[4][3];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const ConsBig bg = big[blockIdx.x];
  const u32 c = bg.c, r = rep[c];
  const u64 ro = off[r], L = off[r + 1] - ro, oo = out_off[c - 1];
  const u32 *t8 = tab + bg.tab * 8u;
  u64 votes = 0, errs = 0, changed = 0;
  for (u64 col = threadIdx.x; col < L; col += 256) {
    ConsAcc a;
    a.s0 = t8[0 * L + col]; a.s1 = t8[1 * L + col]; a.s2 = t8[2 * L + col]; a.s3 = t8[3 * L + col];
    a.n0 = t8[4 * L + col]; a.n1 = t8[5 * L + col]; a.n2 = t8[6 * L + col]; a.n3 = t8[7 * L + col];
    const ConsOut o = cons_decide(a, bases[ro + col], quals[ro + col], cap_q);
    ob[oo + col] = (u8)o.base; oq[oo + col] = (u8)o.qual;
    votes += o.votes; errs += o.errs; changed += o.changed;
  }
#pragma unroll
  for (u32 s = 32; s >= 1; s >>= 1) {
    votes += ((u64)(u32)__shfl_xor((int)(u32)(votes >> 32), (int)s) << 32) | (u32)__shfl_xor((int)(u32)votes, (int)s);
    errs += ((u64)(u32)__shfl_xor((int)(u32)(errs >> 32), (int)s) << 32) | (u32)__shfl_xor((int)(u32)errs, (int)s);
    changed += ((u64)(u32)__shfl_xor((int)(u32)(changed >> 32), (int)s) << 32) | (u32)__shfl_xor((int)(u32)changed, (int)s);
  }
  if (lane == 0) { lds[wave][0] = changed; lds[wave][1] = votes; lds[wave][2] = errs; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 ch = lds[0][0] + lds[1][0] + lds[2][0] + lds[3][0], v = lds[0][1] + lds[1][1] + lds[2][1] + lds[3][1],
              e = lds[0][2] + lds[1][2] + lds[2][2] + lds[3][2];
    depth[c - 1] = mem_off[c] - mem_off[c - 1];
    errors[c - 1] = e;
    atomicAdd(&ctr[CONS_MULTI], 1ull);
    if (ch) atomicAdd(&ctr[CONS_CHANGED], (ull)ch);
    if (v) atomicAdd(&ctr[CONS_VOTES], (ull)v);
    if (e) atomicAdd(&ctr[CONS_ERRORS], (ull)e);
  }
}

#endif  // HUMID_KERNELS_CONSENSUS_HIP_H
