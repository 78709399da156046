// passes.hip.h -- the post-run passes over device arrays: the best-scoring read per cluster, consensus reads, duplex consensus reads,
// optical duplicates.  Each body is what both C ABI forms of its pass (humid_hip.hip) run once the arguments are checked and,
// for the host form, staged.  Internal linkage; included by humid_hip.hip only (pipeline.hip.h goes into both HIP
// translation units, and humid_exchange.hip runs none of these).  Every buffer here is a PASS_ENSURE one.
#ifndef HUMID_PASSES_HIP_H
#define HUMID_PASSES_HIP_H

#include "pipeline.hip.h"
#include "kernels_best.hip.h"
#include "kernels_consensus.hip.h"
#include "kernels_dconsensus.hip.h"
#include "kernels_optical.hip.h"
static_assert(DCONS_STRAND_TOP == HUMID_STRAND_TOP && DCONS_STRAND_BOTTOM == HUMID_STRAND_BOTTOM, "kernels_dconsensus.hip.h names the strands of the header");
static_assert(OPT_WALK_DEFAULT == 64u, "humid_ctx::op_walk starts at the default");

// The refusal the three passes share, as k_best_rep / k_cons_rep report it: bit 0 of err an id above C, bit 1 a cluster
// with two kept reads; then the kept reads that claimed a cluster against C.  fn names the entry point.
static int claim_check(humid_ctx *c, const char *fn, u64 err, u64 claims, u32 C) {
  if (err & 1u) return fail(c, HUMID_E_INVALID, "%s: a cluster id above the %u clusters", fn, C);
  if (err & 2u) return fail(c, HUMID_E_INVALID, "%s: a cluster has more than one read with keep == 1", fn);
  if (claims != C) return fail(c, HUMID_E_INVALID, "%s: %llu reads with keep == 1 for %u clusters", fn, (ull)claims, C);
  return HUMID_OK;
}

// ---- best-scoring read per cluster (kernels_best.hip.h); n_reads > 0, the run's C clusters ------------------------
static int best_pass(humid_ctx *c, const u64 *d_words, const u32 *d_cluster_id, const u8 *d_keep, const u32 *d_score, u64 n_reads,
                     u32 word_nt, u32 scope, u8 *d_keep_out, u32 *d_rep_out, uint64_t *n_changed) {
  const bool wide = word_nt > 32, leaf = scope == HUMID_BEST_LEAF;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const u32 N = (u32)n_reads, C = (u32)c->C;
  PASS_ENSURE(c->bs_rep, ((size_t)C + 1) * 4);
  PASS_ENSURE(c->bs_best, ((size_t)C + 1) * 8);
  PASS_ENSURE(c->bs_ctr, BEST_CTRS * 4);
  u32 *rep = c->bs_rep.as<u32>(), *ctr = c->bs_ctr.as<u32>();
  ull *best = c->bs_best.as<ull>();
  HIPCHK(hipMemsetAsync(rep, 0xff, ((size_t)C + 1) * 4, st));
  HIPCHK(hipMemsetAsync(best, 0, ((size_t)C + 1) * 8, st));
  HIPCHK(hipMemsetAsync(ctr, 0, BEST_CTRS * 4, st));
  hipLaunchKernelGGL(k_best_rep, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_cluster_id, d_keep, N, C, rep, ctr);
  const dim3 grid(blocks_for(N)), block(256);
  if (wide && leaf)
    hipLaunchKernelGGL((k_best_vote<W2, true>), grid, block, 0, st, (const W2 *)d_words, d_cluster_id, d_score, N, C, (const u32 *)rep, (const u32 *)ctr, best);
  else if (wide)
    hipLaunchKernelGGL((k_best_vote<W2, false>), grid, block, 0, st, (const W2 *)d_words, d_cluster_id, d_score, N, C, (const u32 *)rep, (const u32 *)ctr, best);
  else if (leaf)
    hipLaunchKernelGGL((k_best_vote<u64, true>), grid, block, 0, st, d_words, d_cluster_id, d_score, N, C, (const u32 *)rep, (const u32 *)ctr, best);
  else
    hipLaunchKernelGGL((k_best_vote<u64, false>), grid, block, 0, st, d_words, d_cluster_id, d_score, N, C, (const u32 *)rep, (const u32 *)ctr, best);
  hipLaunchKernelGGL(k_best_write, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_cluster_id, N, C, (const u32 *)rep, (const ull *)best,
                     d_keep_out, d_rep_out, ctr);
  HIPCHK(hipGetLastError());
  u32 h[BEST_CTRS] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          // the pass's one host wait
  TRY(claim_check(c, "humid_select_best", h[BEST_ERR], h[BEST_CLAIMS], C));
  if (n_changed) *n_changed = h[BEST_CHANGED];
  return HUMID_OK;
}

// ---- consensus reads per cluster (kernels_consensus.hip.h); the results stay in c->cs_* ---------------------------
static int consensus_pass(humid_ctx *c, const u8 *d_bases, const u8 *d_quals, const u64 *d_off, u64 n_bytes, const u32 *d_cluster_id,
                          const u8 *d_keep, u64 n_reads, u64 n_clusters, u32 min_q, u32 cap_q, humid_consensus_summary *summary) {
  static const char *const fn = "humid_consensus";
  if (summary) memset(summary, 0, sizeof *summary);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (n_reads == 0 || n_clusters == 0) {                     // an empty result: out_off = {0}
    PASS_ENSURE(c->cs_ooff, 8);
    HIPCHK(hipMemsetAsync(c->cs_ooff.p, 0, 8, st));
    HIPCHK(hipStreamSynchronize(st));
    c->cs_sum = humid_consensus_summary{};
    c->cs_valid = true;
    return HUMID_OK;
  }
  if (n_clusters > n_reads)                                  // (some cluster then has no read at all, so no kept one)
    return fail(c, HUMID_E_INVALID, "%s: %llu clusters for %llu reads: a cluster without a read with keep == 1", fn, (ull)n_clusters,
                (ull)n_reads);
  const u32 N = (u32)n_reads, C = (u32)n_clusters, min_q1 = min_q < 1 ? 1u : min_q;
  const size_t max_big = (size_t)N / CONS_BIG + 2, max_piece = (size_t)N / CONS_PIECE + max_big + 2;
  PASS_ENSURE(c->cs_rep, ((size_t)C + 1) * 4);
  PASS_ENSURE(c->cs_cnt, ((size_t)C + 2) * 4);
  PASS_ENSURE(c->cs_moff, ((size_t)C + 1) * 4);
  PASS_ENSURE(c->cs_ctr, CONS_CTRS * 8);
  PASS_ENSURE(c->cs_ooff, ((size_t)C + 1) * 8);
  PASS_ENSURE(c->cs_big, max_big * sizeof(ConsBig));
  PASS_ENSURE(c->cs_piece, max_piece * sizeof(ConsPiece));
  u32 *rep = c->cs_rep.as<u32>(), *cnt = c->cs_cnt.as<u32>(), *moff = c->cs_moff.as<u32>();
  ull *ctr = c->cs_ctr.as<ull>();
  u64 *ooff = c->cs_ooff.as<u64>();
  ConsBig *big = c->cs_big.as<ConsBig>();
  ConsPiece *piece = c->cs_piece.as<ConsPiece>();
  HIPCHK(hipMemsetAsync(rep, 0xff, ((size_t)C + 1) * 4, st));
  HIPCHK(hipMemsetAsync(cnt, 0, ((size_t)C + 2) * 4, st));
  HIPCHK(hipMemsetAsync(ctr, 0, CONS_CTRS * 8, st));
  hipLaunchKernelGGL(k_cons_rep, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_cluster_id, d_keep, d_off, N, (u64)n_bytes, C, rep, cnt, ctr);
  TRY(exscan_in<u64>(c, ConsLenIn{rep, d_off, ctr, C}, ooff, (u64)C + 1));
  TRY(exscan_in<u32>(c, PtrIn<u32>{cnt + 1}, moff, (u64)C + 1));
  hipLaunchKernelGGL(k_cons_big_list, dim3(grid_stride_blocks(C)), dim3(256), 0, st, (const u32 *)cnt, (const u64 *)ooff, C, big, piece, ctr);
  HIPCHK(hipGetLastError());
  ull h[CONS_CTRS] = {};
  u64 total = 0;
  HIPCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&total, ooff + C, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          // the first host wait: is the input well formed, and the total that sizes the output
  TRY(claim_check(c, fn, h[CONS_ERR], C, C));                // (ids and double claims first, the claim count after the offsets)
  if (h[CONS_ERR] & 4u) return fail(c, HUMID_E_INVALID, "%s: off decreases", fn);
  if (h[CONS_ERR] & 8u) return fail(c, HUMID_E_INVALID, "%s: off[n_reads] lies beyond the %llu bytes given", fn, (ull)n_bytes);
  TRY(claim_check(c, fn, 0, h[CONS_CLAIMS], C));
  if (h[CONS_ERR] & 16u) return fail(c, HUMID_E_OVERFLOW, "%s: a cluster of more than %u reads (32-bit sums)", fn, CONS_MAX_DEPTH);
  const u32 n_big = (u32)h[CONS_NBIG], n_pieces = (u32)h[CONS_NPIECES];
  PASS_ENSURE(c->cs_ob, (size_t)total + 16);
  PASS_ENSURE(c->cs_oq, (size_t)total + 16);
  PASS_ENSURE(c->cs_depth, (size_t)C * 4);
  PASS_ENSURE(c->cs_errors, (size_t)C * 8);
  PASS_ENSURE(c->cs_cur, ((size_t)C + 1) * 4);
  PASS_ENSURE(c->cs_mem, (size_t)N * 4);
  HIPCHK(hipMemsetAsync(c->cs_cur.p, 0, ((size_t)C + 1) * 4, st));
  hipLaunchKernelGGL(k_cons_scatter, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_cluster_id, N, (const u32 *)moff, c->cs_cur.as<u32>(), c->cs_mem.as<u32>());
  hipLaunchKernelGGL(k_cons_small, dim3(blocks_for(C, 4)), dim3(256), 0, st, d_bases, d_quals, d_off, (const u32 *)rep, (const u32 *)moff,
                     (const u32 *)c->cs_mem.p, (const u64 *)ooff, C, min_q1, cap_q, c->cs_ob.as<u8>(), c->cs_oq.as<u8>(),
                     c->cs_depth.as<u32>(), c->cs_errors.as<u64>(), ctr);
  if (n_big) {
    const size_t tab_bytes = (size_t)h[CONS_TABCOLS] * 32;
    PASS_ENSURE(c->cs_tab, tab_bytes + 16);
    HIPCHK(hipMemsetAsync(c->cs_tab.p, 0, tab_bytes, st));
    hipLaunchKernelGGL(k_cons_piece, dim3(n_pieces), dim3(256), 0, st, d_bases, d_quals, d_off, (const u32 *)moff, (const u32 *)c->cs_mem.p,
                       (const u64 *)ooff, (const ConsBig *)big, (const ConsPiece *)piece, min_q1, c->cs_tab.as<u32>());
    hipLaunchKernelGGL(k_cons_final, dim3(n_big), dim3(256), 0, st, d_bases, d_quals, d_off, (const u32 *)rep, (const u32 *)moff,
                       (const u64 *)ooff, (const ConsBig *)big, (const u32 *)c->cs_tab.p, cap_q, c->cs_ob.as<u8>(), c->cs_oq.as<u8>(),
                       c->cs_depth.as<u32>(), c->cs_errors.as<u64>(), ctr);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          // the second host wait: the summary
  c->cs_sum = humid_consensus_summary{(u64)C, total, (u64)h[CONS_MULTI], (u64)h[CONS_CHANGED], (u64)h[CONS_VOTES], (u64)h[CONS_ERRORS]};
  c->cs_valid = true;
  if (summary) *summary = c->cs_sum;
  return HUMID_OK;
}

// ---- duplex consensus reads per cluster (kernels_dconsensus.hip.h); the results stay in c->cs_* and c->ds_* ---------
// consensus_pass with two layers: the same scratch, the same two host waits, the same result buffers.
static int duplex_consensus_pass(humid_ctx *c, const u8 *d_bases_s, const u8 *d_quals_s, const u64 *d_off_s, u64 n_bytes_s,
                                 const u8 *d_bases_o, const u8 *d_quals_o, const u64 *d_off_o, u64 n_bytes_o, const u32 *d_cluster_id,
                                 const u8 *d_keep, const u8 *d_strand, u64 n_reads, u64 n_clusters, u32 min_q, u32 strand_cap_q,
                                 u32 cap_q, humid_duplex_summary *summary) {
  static const char *const fn = "humid_duplex_consensus";
  if (summary) memset(summary, 0, sizeof *summary);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (n_reads == 0 || n_clusters == 0) {                     // an empty result: out_off = {0}
    PASS_ENSURE(c->cs_ooff, 8);
    HIPCHK(hipMemsetAsync(c->cs_ooff.p, 0, 8, st));
    HIPCHK(hipStreamSynchronize(st));
    c->cs_sum = humid_consensus_summary{};
    c->ds_sum = humid_duplex_summary{};
    c->cs_valid = c->cs_duplex = true;
    return HUMID_OK;
  }
  if (n_clusters > n_reads)                                  // (some cluster then has no read at all, so no kept one)
    return fail(c, HUMID_E_INVALID, "%s: %llu clusters for %llu reads: a cluster without a read with keep == 1", fn, (ull)n_clusters,
                (ull)n_reads);
  const u32 N = (u32)n_reads, C = (u32)n_clusters, min_q1 = min_q < 1 ? 1u : min_q;
  const size_t max_big = (size_t)N / CONS_BIG + 2, max_piece = (size_t)N / CONS_PIECE + max_big + 2;
  PASS_ENSURE(c->cs_rep, ((size_t)C + 1) * 4);
  PASS_ENSURE(c->cs_cnt, ((size_t)C + 2) * 4);
  PASS_ENSURE(c->ds_top, ((size_t)C + 2) * 4);
  PASS_ENSURE(c->cs_moff, ((size_t)C + 1) * 4);
  PASS_ENSURE(c->cs_ctr, DCONS_CTRS * 8);
  PASS_ENSURE(c->cs_ooff, ((size_t)C + 1) * 8);
  PASS_ENSURE(c->cs_big, max_big * sizeof(ConsBig));
  PASS_ENSURE(c->cs_piece, max_piece * sizeof(ConsPiece));
  u32 *rep = c->cs_rep.as<u32>(), *cnt = c->cs_cnt.as<u32>(), *top = c->ds_top.as<u32>(), *moff = c->cs_moff.as<u32>();
  ull *ctr = c->cs_ctr.as<ull>();
  u64 *ooff = c->cs_ooff.as<u64>();
  ConsBig *big = c->cs_big.as<ConsBig>();
  ConsPiece *piece = c->cs_piece.as<ConsPiece>();
  HIPCHK(hipMemsetAsync(rep, 0xff, ((size_t)C + 1) * 4, st));
  HIPCHK(hipMemsetAsync(cnt, 0, ((size_t)C + 2) * 4, st));
  HIPCHK(hipMemsetAsync(top, 0, ((size_t)C + 2) * 4, st));
  HIPCHK(hipMemsetAsync(ctr, 0, DCONS_CTRS * 8, st));
  hipLaunchKernelGGL(k_dcons_rep, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_cluster_id, d_keep, d_strand, d_off_s, d_off_o, N,
                     (u64)n_bytes_s, (u64)n_bytes_o, C, rep, cnt, top, ctr);
  TRY(exscan_in<u64>(c, ConsLenIn{rep, d_off_s, ctr, C}, ooff, (u64)C + 1));
  TRY(exscan_in<u32>(c, PtrIn<u32>{cnt + 1}, moff, (u64)C + 1));
  hipLaunchKernelGGL(k_cons_big_list, dim3(grid_stride_blocks(C)), dim3(256), 0, st, (const u32 *)cnt, (const u64 *)ooff, C, big, piece, ctr);
  HIPCHK(hipGetLastError());
  ull h[DCONS_CTRS] = {};
  u64 total = 0;
  HIPCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&total, ooff + C, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          // the first host wait: is the input well formed, and the total that sizes the output
  TRY(claim_check(c, fn, h[CONS_ERR], C, C));                // (ids and double claims first, the claim count after the offsets)
  if (h[CONS_ERR] & 4u) return fail(c, HUMID_E_INVALID, "%s: off decreases in one of the layers", fn);
  if (h[CONS_ERR] & 8u)
    return fail(c, HUMID_E_INVALID, "%s: off[n_reads] lies beyond the %llu / %llu bytes given", fn, (ull)n_bytes_s, (ull)n_bytes_o);
  if (h[CONS_ERR] & 32u) return fail(c, HUMID_E_INVALID, "%s: a member's strand is neither TOP nor BOTTOM", fn);
  TRY(claim_check(c, fn, 0, h[CONS_CLAIMS], C));
  if (h[CONS_ERR] & 16u) return fail(c, HUMID_E_OVERFLOW, "%s: a cluster of more than %u reads (32-bit sums)", fn, CONS_MAX_DEPTH);
  const u32 n_big = (u32)h[CONS_NBIG], n_pieces = (u32)h[CONS_NPIECES];
  PASS_ENSURE(c->cs_ob, (size_t)total + 16);
  PASS_ENSURE(c->cs_oq, (size_t)total + 16);
  PASS_ENSURE(c->cs_depth, (size_t)C * 4);
  PASS_ENSURE(c->cs_errors, (size_t)C * 8);
  PASS_ENSURE(c->ds_same, (size_t)C * 4);
  PASS_ENSURE(c->ds_other, (size_t)C * 4);
  PASS_ENSURE(c->ds_disagree, (size_t)C * 4);
  PASS_ENSURE(c->cs_cur, ((size_t)C + 1) * 8);
  PASS_ENSURE(c->cs_mem, (size_t)N * 4);
  HIPCHK(hipMemsetAsync(c->cs_cur.p, 0, ((size_t)C + 1) * 8, st));
  hipLaunchKernelGGL(k_dcons_scatter, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_cluster_id, d_strand, N, (const u32 *)moff,
                     c->cs_cur.as<u32>(), c->cs_mem.as<u32>());
  hipLaunchKernelGGL(k_dcons_small, dim3(blocks_for(C, 4)), dim3(256), 0, st, d_bases_s, d_quals_s, d_off_s, d_bases_o, d_quals_o, d_off_o,
                     d_strand, (const u32 *)rep, (const u32 *)top, (const u32 *)moff, (const u32 *)c->cs_mem.p, (const u64 *)ooff, C, min_q1,
                     strand_cap_q, cap_q, c->cs_ob.as<u8>(), c->cs_oq.as<u8>(), c->cs_depth.as<u32>(), c->ds_same.as<u32>(),
                     c->ds_other.as<u32>(), c->ds_disagree.as<u32>(), c->cs_errors.as<u64>(), ctr);
  if (n_big) {
    const size_t tab_bytes = (size_t)h[CONS_TABCOLS] * 64;
    PASS_ENSURE(c->cs_tab, tab_bytes + 16);
    HIPCHK(hipMemsetAsync(c->cs_tab.p, 0, tab_bytes, st));
    hipLaunchKernelGGL(k_dcons_piece, dim3(n_pieces), dim3(256), 0, st, d_bases_s, d_quals_s, d_off_s, d_bases_o, d_quals_o, d_off_o, d_strand,
                       (const u32 *)rep, (const u32 *)top, (const u32 *)moff, (const u32 *)c->cs_mem.p, (const u64 *)ooff,
                       (const ConsBig *)big, (const ConsPiece *)piece, min_q1, c->cs_tab.as<u32>());
    hipLaunchKernelGGL(k_dcons_final, dim3(n_big), dim3(256), 0, st, d_bases_s, d_quals_s, d_off_s, d_strand, (const u32 *)rep,
                       (const u32 *)top, (const u32 *)moff, (const u64 *)ooff, (const ConsBig *)big, (const u32 *)c->cs_tab.p, strand_cap_q,
                       cap_q, c->cs_ob.as<u8>(), c->cs_oq.as<u8>(), c->cs_depth.as<u32>(), c->ds_same.as<u32>(), c->ds_other.as<u32>(),
                       c->ds_disagree.as<u32>(), c->cs_errors.as<u64>(), ctr);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          // the second host wait: the summary
  c->cs_sum = humid_consensus_summary{(u64)C, total, (u64)h[CONS_MULTI], (u64)h[CONS_CHANGED], (u64)h[CONS_VOTES], (u64)h[CONS_ERRORS]};
  c->ds_sum = humid_duplex_summary{(u64)C, total, (u64)h[CONS_MULTI], (u64)h[CONS_CHANGED], (u64)h[CONS_VOTES], (u64)h[CONS_ERRORS],
                                   (u64)h[DCONS_DUPLEX], (u64)h[DCONS_BOTH], (u64)(h[DCONS_BOTH] - h[DCONS_DISAGREE]), (u64)h[DCONS_DISAGREE],
                                   (u64)h[DCONS_MASKED]};
  c->cs_valid = c->cs_duplex = true;
  if (summary) *summary = c->ds_sum;
  return HUMID_OK;
}

// ---- optical duplicates per cluster (kernels_optical.hip.h); n_reads > 0 ------------------------------------------
static int optical_pass(humid_ctx *c, const u32 *d_cluster_id, const u8 *d_keep, const u32 *d_tile, const u32 *d_x, const u32 *d_y,
                        u64 n_reads, u64 n_clusters, u32 distance, u8 *d_optical_out, u32 *d_origin_out, u32 *d_per_cluster_out,
                        humid_optical_summary *summary) {
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (n_clusters == 0) {                                     // no read is a member
    HIPCHK(hipMemsetAsync(d_optical_out, 0, (size_t)n_reads, st));
    if (d_origin_out) HIPCHK(hipMemsetAsync(d_origin_out, 0xff, (size_t)n_reads * 4, st));
    HIPCHK(hipStreamSynchronize(st));
    return HUMID_OK;
  }
  if (n_clusters > n_reads)                                  // (some cluster then has no read at all, so no kept one)
    return fail(c, HUMID_E_INVALID, "humid_optical_duplicates: %llu clusters for %llu reads: a cluster without a read with keep == 1",
                (ull)n_clusters, (ull)n_reads);
  const u32 N = (u32)n_reads, C = (u32)n_clusters;
  const size_t n = (size_t)N;
  PASS_ENSURE(c->op_rep, ((size_t)C + 1) * 4);
  PASS_ENSURE(c->op_bctr, BEST_CTRS * 4);
  PASS_ENSURE(c->op_ctr, OPT_CTRS * 8);
  PASS_ENSURE(c->op_k0, n * 4);
  PASS_ENSURE(c->op_v0, n * 4);
  PASS_ENSURE(c->op_v1, n * 4);
  PASS_ENSURE(c->op_ct, n * 8);
  PASS_ENSURE(c->op_xy, n * 8);
  PASS_ENSURE(c->op_vote, n * 8);
  PASS_ENSURE(c->op_parent, n * 4);
  PASS_ENSURE(c->op_root, n * 4);
  PASS_ENSURE(c->op_best, n * 8);
  PASS_ENSURE(c->op_gsize, n * 4);
  u32 *rep = c->op_rep.as<u32>(), *bctr = c->op_bctr.as<u32>(), *k0 = c->op_k0.as<u32>(), *v0 = c->op_v0.as<u32>(), *v1 = c->op_v1.as<u32>();
  u32 *parent = c->op_parent.as<u32>(), *root = c->op_root.as<u32>(), *gsize = c->op_gsize.as<u32>();
  u64 *ct = c->op_ct.as<u64>(), *xy = c->op_xy.as<u64>(), *vote = c->op_vote.as<u64>();
  ull *best = c->op_best.as<ull>(), *ctr = c->op_ctr.as<ull>();
  HIPCHK(hipMemsetAsync(rep, 0xff, ((size_t)C + 1) * 4, st));
  HIPCHK(hipMemsetAsync(bctr, 0, BEST_CTRS * 4, st));
  HIPCHK(hipMemsetAsync(ctr, 0, OPT_CTRS * 8, st));
  HIPCHK(hipMemsetAsync(best, 0xff, n * 8, st));
  HIPCHK(hipMemsetAsync(gsize, 0, n * 4, st));
  hipLaunchKernelGGL(k_best_rep, dim3(grid_stride_blocks(N)), dim3(256), 0, st, d_cluster_id, d_keep, N, C, rep, bctr);
  // the read indices by (cluster_id, tile, x): three stable sorts, least significant key first.  The sorts follow no
  // index of the input (an id above C only lands at the wrong place of an order nobody reads then).
  TRY((sort_pairs_in<u32, u32>(c, OptKeyX{d_cluster_id, d_x}, k0, IotaIn{}, v0, N, 0, 32)));
  TRY((sort_pairs_in<u32, u32>(c, OptKeyTile{d_cluster_id, d_tile, v0}, k0, PtrIn<u32>{v0}, v1, N, 0, 32)));
  TRY((sort_pairs_in<u32, u32>(c, OptKeyCid{d_cluster_id, v1}, k0, PtrIn<u32>{v1}, v0, N, 0, bits_for((u64)C + 1))));
  const dim3 grid(blocks_for(N)), block(256);
  hipLaunchKernelGGL(k_opt_gather, dim3(grid_stride_blocks(N)), block, 0, st, (const u32 *)k0, (const u32 *)v0, d_keep, d_tile, d_x, d_y, N, C,
                     (const u32 *)bctr, ct, xy, vote, parent, d_per_cluster_out);
  hipLaunchKernelGGL(k_opt_walk, grid, block, 0, st, (const u64 *)ct, (const u64 *)xy, N, C, distance, c->op_walk, (const u32 *)bctr, parent);
  hipLaunchKernelGGL(k_opt_root, grid, block, 0, st, (const u64 *)ct, (const u64 *)vote, N, C, (const u32 *)bctr, (const u32 *)parent, root,
                     best, gsize);
  hipLaunchKernelGGL(k_opt_write, dim3(grid_stride_blocks(N)), block, 0, st, (const u64 *)ct, (const u64 *)vote, (const u32 *)root,
                     (const ull *)best, (const u32 *)gsize, N, C, (const u32 *)bctr, d_optical_out, d_origin_out, d_per_cluster_out, ctr);
  HIPCHK(hipGetLastError());
  u32 hb[BEST_CTRS] = {0, 0, 0, 0};
  ull h[OPT_CTRS] = {};
  HIPCHK(hipMemcpyAsync(hb, bctr, sizeof hb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));                          // the pass's one host wait
  TRY(claim_check(c, "humid_optical_duplicates", hb[BEST_ERR], hb[BEST_CLAIMS], C));
  if (summary)
    *summary = humid_optical_summary{(u64)C, (u64)h[OPT_MEMBERS], (u64)h[OPT_MEMBERS] - C, (u64)h[OPT_OPTICAL], (u64)h[OPT_GROUPS],
                                     (u64)h[OPT_LARGEST]};
  return HUMID_OK;
}

#endif  // HUMID_PASSES_HIP_H
