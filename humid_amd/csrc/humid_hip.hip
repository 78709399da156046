// humid_hip.hip -- HUMID's neighbour-search-and-cluster hot path for MI355X (gfx950): the host
// side of libhumid_hip.so (context, stages, C ABI of include/humid_hip.h).  Kernels live in the
// headers included below.
//
// Pipeline (all device-side; integer/bit work, HBM/latency bound, no MFMA):
//   A. exact counts   kernels_count.hip.h   reads radix-partitioned by mix64(word), one LDS-resident
//                     open-address table per bucket (k_dedup_lds); fallback: one table in HBM
//                     (k_hash_insert).  Replaces Trie::add, /root/reference/src/humid.cc:95.
//                     Unique words are then sorted: Trie::walk() order.
//   B. graph          kernels_graph.hip.h   generalised pigeonhole buckets (k_combo_keys, k_pairs),
//                     CSR rows through cursors + per-row sort, union-find components.  Replaces
//                     walk x asymmetricHamming, src/humid.cc:113-130.
//                     kernels_cluster.hip.h per component: the findClusters loop + src/cluster.cc,
//                     order-exact (k_cluster_trivial / _small / _components); ids = prefix sum over
//                     creators.  Replaces src/humid.cc:167-193.
//   C. map            kernels_map.hip.h     per read (cluster_id, keep); replaces
//                     trie.find()->leaf->cluster, src/humid.cc:223-231,276-277.  Also the
//                     multi-GPU result return.
// Sorts and scans are the library's own (prims.hip.h): no third-party device code is linked in, so
// every kernel of the code object carries the last-VGPR guard (tests/test_cabi_symbols.py reads the
// code object's kernel descriptors).  No CPU fallback lives here: every entry point either runs on
// the GPU or fails.
//
// Translation units (round 3): this file = the context, the single-GPU entry points and the accessors of
// include/humid_hip.h; humid_exchange.hip = the exchange pass and the multi-GPU stage entry points; shm.cpp = the
// shared-memory gather (no HIP); pipeline.hip.h = the pipeline itself, with internal linkage, compiled into both;
// passes.hip.h = the post-run passes (best read, consensus, optical duplicates) over device arrays, into this file only.
#include "pipeline.hip.h"
#include "passes.hip.h"

static std::string g_err;
// (the error text of calls without a context: also set from humid_exchange.hip and shm.cpp)
extern "C" __attribute__((visibility("hidden"))) void humid_set_global_error(const char *text) { g_err = text ? text : ""; }

// --------------------------------------------------------------------------------
// C ABI
// --------------------------------------------------------------------------------
extern "C" {

uint32_t humid_abi_version(void) { return HUMID_ABI_VERSION; }

int humid_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *humid_last_error(const humid_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int humid_ctx_create(humid_ctx **out, int device, void *stream) {
  humid_ctx *c = nullptr;
  if (!out) return fail(nullptr, HUMID_E_INVALID, "out is null");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    return fail(nullptr, HUMID_E_HIP, "no HIP device available (%s); this library has no CPU fallback",
                hipGetErrorString(e));
  if (device < 0) { if (hipGetDevice(&device) != hipSuccess) device = 0; }
  if (device >= ndev) return fail(nullptr, HUMID_E_INVALID, "device %d out of range (%d devices)", device, ndev);
  c = new (std::nothrow) humid_ctx();
  if (!c) return fail(nullptr, HUMID_E_NOMEM, "host allocation failed");
  c->device = device;
  auto bail = [&](hipError_t err, const char *what) {
    int rc = fail(nullptr, HUMID_E_HIP, "%s: %s", what, hipGetErrorString(err));
    humid_ctx_destroy(c);
    return rc;
  };
  if ((e = hipSetDevice(device)) != hipSuccess) return bail(e, "hipSetDevice");
  if (stream) { c->stream = (hipStream_t)stream; c->own_stream = false; }
  else {
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail(e, "hipStreamCreate");
    c->own_stream = true;
  }
  if ((e = hipMalloc((void **)&c->d_ctr, CTR_N * sizeof(ull) + sizeof(PsChain))) != hipSuccess) return bail(e, "hipMalloc");
  c->ps_chain = (PsChain *)(c->d_ctr + CTR_N);                 // the scans' chain (prims.hip.h): zero once, epochs after that
  if ((e = hipMemset(c->ps_chain, 0, sizeof(PsChain))) != hipSuccess) return bail(e, "hipMemset");
  if ((e = hipMalloc((void **)&c->d_stamp, STAMP_N * sizeof(u64))) != hipSuccess) return bail(e, "hipMalloc");
  if ((e = hipMemset(c->d_stamp, 0, STAMP_N * sizeof(u64))) != hipSuccess) return bail(e, "hipMemset");
  if ((e = hipHostMalloc((void **)&c->h_ctr, (STAMP_AT + STAMP_N) * sizeof(ull), hipHostMallocDefault)) != hipSuccess) return bail(e, "hipHostMalloc");
  memset(c->h_ctr, 0, (STAMP_AT + STAMP_N) * sizeof(ull));
  if (hipHostGetDevicePointer((void **)&c->h_ctr_dev, c->h_ctr, 0) != hipSuccess) { c->h_ctr_dev = nullptr; (void)hipGetLastError(); }
  c->no_poll = getenv("HUMID_NO_POLL") != nullptr;
  c->no_chain = getenv("HUMID_NO_SCAN_CHAIN") != nullptr;
  c->gf_padded = getenv("HUMID_NO_GROUP_PAD") == nullptr;
  for (auto &ev : c->ev)
    if ((e = hipEventCreate(&ev)) != hipSuccess) return bail(e, "hipEventCreate");
  for (auto &ev : c->kev)
    if ((e = hipEventCreate(&ev)) != hipSuccess) return bail(e, "hipEventCreate");
  if (const char *m = getenv("HUMID_COUNT_MODE")) c->count_mode = (atoi(m) == 1) ? 1 : 0;
  if (const char *m = getenv("HUMID_KERNEL_TIMING")) c->kev_on = atoi(m) != 0;
  *out = c;
  return HUMID_OK;
}

void humid_ctx_destroy(humid_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
#ifdef HUMID_PHASE_CLOCKS                                    // (experiment builds only: common.hip.h)
  {
    static const char *names[PH_KERNELS] = {"k_dedup_rec", "k_p8_scatter1", "k_p8_scatter2", "k_unperm_bins8", "k_group_fine", "k_pairs_append", "k_unperm_window", "-"};
    ull h[PH_KERNELS][PH_MAX];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(humid_phase), sizeof h) == hipSuccess)
      for (int k = 0; k < PH_KERNELS; k++) {
        if (!h[k][0]) continue;
        fprintf(stderr, "[phase clocks] %-16s %6llu workgroups sampled; us per workgroup by phase:", names[k], h[k][0]);
        double tot = 0;
        for (int t = 1; t < PH_MAX; t++) { fprintf(stderr, " %.2f", (double)h[k][t] / (double)h[k][0] / 100.0); tot += (double)h[k][t]; }
        fprintf(stderr, " | sum %.2f\n", tot / (double)h[k][0] / 100.0);
      }
  }
#endif
  if (c->arena.base) (void)hipFree(c->arena.base);
  if (c->d_ctr) (void)hipFree(c->d_ctr);
  if (c->d_stamp) (void)hipFree(c->d_stamp);
  if (c->h_ctr) (void)hipHostFree(c->h_ctr);
  for (auto &ev : c->ev) if (ev) (void)hipEventDestroy(ev);
  for (auto &ev : c->kev) if (ev) (void)hipEventDestroy(ev);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;                                                  // every DBuf frees its block here, after the slab (carved blocks free nothing)
}

void *humid_host_alloc(uint64_t bytes) {
  void *p = nullptr;
  if (bytes == 0 || hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}

void humid_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

int humid_ctx_reserve(humid_ctx *c, uint64_t n_reads, uint32_t word_nt) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (c->arena.base) return HUMID_OK;                       // one slab per context
  if (n_reads == 0) return HUMID_OK;
  HIPCHK(hipSetDevice(c->device));
  // what one run over n_reads reads carves (measured: 112 B per read at 24 nt, unique/reads <= 1
  // assumed worst; wide words: +24 B) plus the host entry point's staging (14 or 22 B per read)
  const size_t per_read = (word_nt > 32 ? 200 : 180) + (word_nt > 32 ? 22 : 14);   // (168 + the padded partition level, round 2)
  size_t want = (size_t)n_reads * per_read + ((size_t)64 << 20);
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b / 2) want = free_b / 2;
  void *p = nullptr;
  if (hipMalloc(&p, want) != hipSuccess) { (void)hipGetLastError(); return HUMID_OK; }   // no slab: buffers are allocated one by one
  c->arena.base = (char *)p;
  c->arena.size = want;
  c->arena.used = 0;
  // the first launch of a process loads the library's code object (~1500 kernels with the sort /
  // scan instantiations: tens of milliseconds): pay that here, off the caller's critical path
  hipLaunchKernelGGL(k_iota, dim3(1), dim3(64), 0, c->stream, (u32 *)p, 64u);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_ctx_set_option(humid_ctx *c, const char *key, int64_t value) {
  if (!c || !key) return fail(c, HUMID_E_INVALID, "null argument");
  if (strcmp(key, "count_mode") == 0) {
    if (value != 0 && value != 1) return fail(c, HUMID_E_INVALID, "count_mode must be 0 (LDS-partitioned) or 1 (global table)");
    c->count_mode = (int)value;
    return HUMID_OK;
  }
  if (strcmp(key, "count_order") == 0) {
    if (value < -1 || value > 1) return fail(c, HUMID_E_INVALID, "count_order must be -1 (auto), 0 or 1");
    c->count_order = (int)value;
    return HUMID_OK;
  }
  if (strcmp(key, "edit_distance") == 0) {
    c->edit = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "keyrank_table_log2") == 0) {
    if (value != 0 && (value < 4 || value > 32)) return fail(c, HUMID_E_INVALID, "keyrank_table_log2 must be 0 (automatic) or 4 .. 32");
    c->kr_force_log2 = (u32)value;
    return HUMID_OK;
  }
  if (strcmp(key, "cells_table_log2") == 0) {
    if (value != 0 && (value < 4 || value > 32)) return fail(c, HUMID_E_INVALID, "cells_table_log2 must be 0 (automatic) or 4 .. 32");
    c->cd_force_log2 = (u32)value;
    return HUMID_OK;
  }
  if (strcmp(key, "whitelist_coop") == 0) {
    c->wl_coop = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "tile_partition") == 0) {
    c->use_tile_partition = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "coop_big") == 0) {
    c->coop_big = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "kernel_timing") == 0) {
    c->kev_on = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "test_fail_before_gather") == 0) {
    c->x_test_fail_after = (int)value;
    return HUMID_OK;
  }
  if (strcmp(key, "records8") == 0) {
    c->use_rec8 = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "compact_graph") == 0) {
    c->use_compact = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "group_buckets") == 0) {
    c->group_buckets = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "fused_search") == 0) {
    c->fused_search = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "pair_split") == 0) {
    c->pair_split = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "group_records") == 0) {
    c->group_records = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "overlap_waits") == 0) {
    c->overlap_waits = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "device_stamps") == 0) {
    c->device_stamps = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "static_tiles") == 0) {
    c->static_tiles = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "padded_partition") == 0) {
    c->pt_padded = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "force_comm") == 0) {
    c->force_comm = value != 0;
    return HUMID_OK;
  }
  if (strcmp(key, "bucket_walk") == 0) {
    if (value < 0 || value > (1 << 24)) return fail(c, HUMID_E_INVALID, "bucket_walk must be 0 (no limit) .. 2^24");
    c->walk_max = (u32)value;
    return HUMID_OK;
  }
  if (strcmp(key, "optical_walk") == 0) {
    if (value < 0 || value > (1 << 24)) return fail(c, HUMID_E_INVALID, "optical_walk must be 0 (no limit) .. 2^24");
    c->op_walk = (u32)value;
    return HUMID_OK;
  }
  if (strcmp(key, "plan_segments") == 0) {
    if (value < 0 || value > 32) return fail(c, HUMID_E_INVALID, "plan_segments must be 0 (auto) .. 32");
    c->force_segments = (u32)value;
    return HUMID_OK;
  }
  if (strcmp(key, "long_key_bits") == 0) {
    if (value < 1 || value > 64) return fail(c, HUMID_E_INVALID, "long_key_bits must be 1 .. 64");
    c->lg_key_bits = (u32)value;
    return HUMID_OK;
  }
  if (strcmp(key, "accum_tile") == 0) {
    if (value < 64 || value > ACC_TILE || (value & (value - 1))) return fail(c, HUMID_E_INVALID, "accum_tile must be a power of two, 64 .. %u", ACC_TILE);
    c->ac_tile = (u32)value;
    return HUMID_OK;
  }
  return fail(c, HUMID_E_INVALID, "unknown option '%s'", key);
}

int humid_dedup_run_device(humid_ctx *c, const uint64_t *d_words, const uint8_t *d_filtered,
                           uint64_t n_reads, uint32_t word_nt, uint32_t distance, uint32_t method,
                           uint32_t *d_cluster_id, uint8_t *d_keep, humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  return with_word_type(word_nt, [&](auto *w) {
    return run_device(c, (decltype(w))d_words, d_filtered, n_reads, word_nt, distance, method, d_cluster_id, d_keep, summary);
  });
}

int humid_dedup_run_grouped_device(humid_ctx *c, const uint64_t *d_words, const uint32_t *d_group,
                                   const uint8_t *d_filtered, uint64_t n_reads, uint32_t word_nt, uint32_t n_groups,
                                   uint32_t distance, uint32_t method, uint32_t *d_cluster_id, uint8_t *d_keep,
                                   humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  return with_word_type(word_nt, [&](auto *w) {
    return run_grouped_device(c, (decltype(w))d_words, d_group, d_filtered, n_reads, word_nt, n_groups, distance, method,
                              d_cluster_id, d_keep, summary);
  });
}

int humid_dedup_run_keyed_device(humid_ctx *c, const uint64_t *d_words, const uint64_t *d_key, const uint8_t *d_filtered,
                                 uint64_t n_reads, uint32_t word_nt, uint32_t distance, uint32_t method,
                                 uint32_t *d_cluster_id, uint8_t *d_keep, humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  return with_word_type(word_nt, [&](auto *w) {
    return run_keyed_device(c, (decltype(w))d_words, d_key, d_filtered, n_reads, word_nt, distance, method, d_cluster_id, d_keep,
                            summary);
  });
}

int humid_dedup_run_keyed_corrected_device(humid_ctx *c, const uint64_t *d_words, const uint64_t *d_key,
                                           const uint8_t *d_filtered, uint64_t n_reads, uint32_t word_nt, uint32_t distance,
                                           uint32_t method, uint32_t *d_cluster_id, uint8_t *d_keep, humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  return with_word_type(word_nt, [&](auto *w) {
    return run_keyed_corrected_device(c, (decltype(w))d_words, d_key, d_filtered, n_reads, word_nt, distance, method,
                                      d_cluster_id, d_keep, summary);
  });
}

int humid_dedup_run_keyed_posterior_device(humid_ctx *c, const uint64_t *d_words, const uint64_t *d_key, const uint8_t *d_qual,
                                           const uint8_t *d_filtered, uint64_t n_reads, uint32_t word_nt, uint32_t distance,
                                           uint32_t method, uint32_t min_odds, uint32_t *d_cluster_id, uint8_t *d_keep,
                                           humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  return with_word_type(word_nt, [&](auto *w) {
    return run_keyed_corrected_device(c, (decltype(w))d_words, d_key, d_filtered, n_reads, word_nt, distance, method,
                                      d_cluster_id, d_keep, summary, d_qual, min_odds, true);
  });
}

// The frame of a host entry point around its pass: four events around the two copies -- the first is the context's, the
// other three live as long as the frame -- and the copy back with ms_h2d / ms_d2h.
struct HostFrame {
  humid_ctx *c;
  hipEvent_t e[4] = {};
  explicit HostFrame(humid_ctx *ctx) : c(ctx) { e[0] = c->ev[EV_HOST_FRAME]; }
  HostFrame(const HostFrame &) = delete;
  ~HostFrame() { for (int i = 1; i < 4; i++) if (e[i]) (void)hipEventDestroy(e[i]); }
  hipError_t create() {
    hipError_t he = hipSuccess;
    for (int i = 1; i < 4 && he == hipSuccess; i++) he = hipEventCreate(&e[i]);
    return he;
  }
  hipError_t staging_begin() { return hipEventRecord(e[0], c->stream); }
  hipError_t staging_end() { return hipEventRecord(e[1], c->stream); }
  // behind a pass that succeeded: the results of n reads to the host and the two copy times into s.  The four event
  // records count for the call (the pass's reset came behind the first two); a failed copy leaves no record of the run.
  int copy_back(size_t n, uint32_t *cluster_id, uint8_t *keep, humid_summary &s) {
    hipStream_t st = c->stream;
    hipError_t he = hipEventRecord(e[2], st);
    if (he == hipSuccess && n) he = hipMemcpyAsync(cluster_id, c->out_cid.p, n * 4, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && n) he = hipMemcpyAsync(keep, c->out_keep.p, n, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipEventRecord(e[3], st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he == hipSuccess) he = hipEventElapsedTime(&s.ms_h2d, e[0], e[1]);
    if (he == hipSuccess) he = hipEventElapsedTime(&s.ms_d2h, e[2], e[3]);
    if (he != hipSuccess) { state_reset(c); return fail(c, HUMID_E_HIP, "copy back: %s", hipGetErrorString(he)); }
    c->timing_left.event_records += 4;
    return HUMID_OK;
  }
};

// host buffers in, host buffers out: words + flags, or (bases != null) the raw symbols, packed on the device.
// kind: what the run is (RUN_GROUPED: group may be null with n_groups = 1; RUN_KEYED on: key, null only without reads);
// paired: the strand-symmetric run (RUN_PLAIN only; CtxState::paired).
// Everything the kind refuses is refused here, before any copy: a refused shape moves nothing.
static int run_host(humid_ctx *c, RunKind kind, bool paired, const uint64_t *words, const uint8_t *filtered, const uint8_t *bases,
                    const uint32_t *group, uint32_t n_groups, const uint64_t *key, uint64_t n_reads, uint32_t word_nt,
                    uint32_t distance, uint32_t method, uint32_t *cluster_id, uint8_t *keep, humid_summary *summary,
                    const uint8_t *qual = nullptr, uint32_t min_odds = 0, bool posterior = false) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  state_reset(c);
  if (paired) TRY(check_paired_run_args(c, n_reads, word_nt, distance, method));
  if (kind == RUN_CORRECTED && !c->wl_n) return fail(c, HUMID_E_STATE, "no whitelist is set in this context (humid_whitelist_set)");
  if (posterior && c->sg.n_seg) return fail(c, HUMID_E_UNSUPPORTED, SEG_NO_POSTERIOR);
  if (posterior && min_odds == 0) return fail(c, HUMID_E_INVALID, "min_odds must be >= 1");
  if (posterior && n_reads && !qual) return fail(c, HUMID_E_INVALID, "null buffer");
  if (kind >= RUN_KEYED) {
    TRY(check_run_args(c, n_reads, word_nt, method, 64));
    if (n_reads && !key) return fail(c, HUMID_E_INVALID, "null buffer");
  }
  if (n_reads && (!(bases || (words && filtered)) || !cluster_id || !keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  if (n_reads > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "n_reads %llu exceeds 2^31-1", (ull)n_reads);
  if (bases) TRY(check_run_args(c, n_reads, word_nt, method, 64));
  if (kind == RUN_GROUPED) {
    TRY(check_run_args(c, n_reads, word_nt, method, 64));
    TRY(check_grouped_args(c, word_nt, n_groups));
    if (!group && n_groups > 1) return fail(c, HUMID_E_INVALID, "group is null with n_groups = %u > 1", n_groups);
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  humid_summary s;
  memset(&s, 0, sizeof s);
  HostFrame frame(c);
  HIPCHK(frame.create());
  size_t n = (size_t)n_reads;
  const size_t wbytes = word_nt > 32 ? 16 : 8;
  ENSURE(c->in_words, n * wbytes + 16);
  ENSURE(c->in_filt, n + 8);
  ENSURE(c->out_cid, n * 4 + 8);
  ENSURE(c->out_keep, n + 8);
  if (bases) ENSURE(c->in_bases, n * word_nt + 16);
  HIPCHK(frame.staging_begin());
  if (n && bases) {
    // device-side packing (makeWord, src/fastq.cc:146-161): the host only gathered the symbols
    HIPCHK(hipMemcpyAsync(c->in_bases.p, bases, n * word_nt, hipMemcpyHostToDevice, st));
    if (word_nt > 32)
      hipLaunchKernelGGL(k_pack_bases<true>, dim3(blocks_for(n)), dim3(256), 0, st, c->in_bases.as<u8>(), (u32)n, word_nt,
                         c->in_words.as<u64>(), c->in_filt.as<u8>());
    else
      hipLaunchKernelGGL(k_pack_bases<false>, dim3(blocks_for(n)), dim3(256), 0, st, c->in_bases.as<u8>(), (u32)n, word_nt,
                         c->in_words.as<u64>(), c->in_filt.as<u8>());
  } else if (n) {
    HIPCHK(hipMemcpyAsync(c->in_words.p, words, n * wbytes, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->in_filt.p, filtered, n, hipMemcpyHostToDevice, st));
  }
  if (n && kind == RUN_GROUPED && group) {
    ENSURE(c->gk_group_in, n * 4 + 8);
    HIPCHK(hipMemcpyAsync(c->gk_group_in.p, group, n * 4, hipMemcpyHostToDevice, st));
  }
  if (n && kind >= RUN_KEYED) {
    ENSURE(c->kr_key_in, n * 8 + 8);
    HIPCHK(hipMemcpyAsync(c->kr_key_in.p, key, n * 8, hipMemcpyHostToDevice, st));
  }
  if (n && posterior) {
    ENSURE(c->bc_qual_in, n * c->wl_nt + 8);
    HIPCHK(hipMemcpyAsync(c->bc_qual_in.p, qual, n * c->wl_nt, hipMemcpyHostToDevice, st));
  }
  HIPCHK(frame.staging_end());
  int rc = with_word_type(word_nt, [&](auto *w) {
    auto *d_w = (decltype(w))c->in_words.p;
    const u8 *d_f = c->in_filt.as<u8>();
    const u64 *d_k = c->kr_key_in.as<u64>();
    u32 *d_cid = c->out_cid.as<u32>();
    u8 *d_keep = c->out_keep.as<u8>();
    if (paired) return run_paired_device(c, d_w, d_f, n_reads, word_nt, distance, method, d_cid, d_keep, &s);
    switch (kind) {
      case RUN_CORRECTED: return run_keyed_corrected_device(c, d_w, d_k, d_f, n_reads, word_nt, distance, method, d_cid, d_keep, &s,
                                                            posterior ? c->bc_qual_in.as<u8>() : nullptr, min_odds, posterior);
      case RUN_KEYED: return run_keyed_device(c, d_w, d_k, d_f, n_reads, word_nt, distance, method, d_cid, d_keep, &s);
      case RUN_GROUPED: return run_grouped_device(c, d_w, group ? c->gk_group_in.as<u32>() : nullptr, d_f, n_reads, word_nt, n_groups,
                                                  distance, method, d_cid, d_keep, &s);
      default: return run_device(c, d_w, d_f, n_reads, word_nt, distance, method, d_cid, d_keep, &s);
    }
  });
  if (rc == HUMID_OK) rc = frame.copy_back(n, cluster_id, keep, s);
  if (rc == HUMID_OK && summary) *summary = s;
  return rc;
}

int humid_dedup_run(humid_ctx *c, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads,
                    uint32_t word_nt, uint32_t distance, uint32_t method, uint32_t *cluster_id,
                    uint8_t *keep, humid_summary *summary) {
  return run_host(c, RUN_PLAIN, false, words, filtered, nullptr, nullptr, 1, nullptr, n_reads, word_nt, distance, method, cluster_id, keep,
                  summary);
}

int humid_dedup_run_grouped(humid_ctx *c, const uint64_t *words, const uint32_t *group, const uint8_t *filtered,
                            uint64_t n_reads, uint32_t word_nt, uint32_t n_groups, uint32_t distance, uint32_t method,
                            uint32_t *cluster_id, uint8_t *keep, humid_summary *summary) {
  return run_host(c, RUN_GROUPED, false, words, filtered, nullptr, group, n_groups, nullptr, n_reads, word_nt, distance, method,
                  cluster_id, keep, summary);
}

int humid_dedup_run_keyed(humid_ctx *c, const uint64_t *words, const uint64_t *key, const uint8_t *filtered,
                          uint64_t n_reads, uint32_t word_nt, uint32_t distance, uint32_t method, uint32_t *cluster_id,
                          uint8_t *keep, humid_summary *summary) {
  return run_host(c, RUN_KEYED, false, words, filtered, nullptr, nullptr, 1, key, n_reads, word_nt, distance, method, cluster_id, keep,
                  summary);
}

int humid_dedup_run_keyed_corrected(humid_ctx *c, const uint64_t *words, const uint64_t *key, const uint8_t *filtered,
                                    uint64_t n_reads, uint32_t word_nt, uint32_t distance, uint32_t method,
                                    uint32_t *cluster_id, uint8_t *keep, humid_summary *summary) {
  return run_host(c, RUN_CORRECTED, false, words, filtered, nullptr, nullptr, 1, key, n_reads, word_nt, distance, method, cluster_id,
                  keep, summary);
}

int humid_dedup_run_keyed_posterior(humid_ctx *c, const uint64_t *words, const uint64_t *key, const uint8_t *qual,
                                    const uint8_t *filtered, uint64_t n_reads, uint32_t word_nt, uint32_t distance,
                                    uint32_t method, uint32_t min_odds, uint32_t *cluster_id, uint8_t *keep, humid_summary *summary) {
  return run_host(c, RUN_CORRECTED, false, words, filtered, nullptr, nullptr, 1, key, n_reads, word_nt, distance, method, cluster_id,
                  keep, summary, qual, min_odds, true);
}

int humid_dedup_run_bases(humid_ctx *c, const uint8_t *bases, uint64_t n_reads, uint32_t word_nt, uint32_t distance,
                          uint32_t method, uint32_t *cluster_id, uint8_t *keep, humid_summary *summary) {
  if (n_reads && !bases) return fail(c, HUMID_E_INVALID, "null buffer");
  return run_host(c, RUN_PLAIN, false, nullptr, nullptr, bases ? bases : (const uint8_t *)"", nullptr, 1, nullptr, n_reads, word_nt, distance,
                  method, cluster_id, keep, summary);
}

// ---- long words (kernels_long.hip.h; run_device_long in pipeline.hip.h) --------------------------------------------
int humid_dedup_run_long_device(humid_ctx *c, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                                uint32_t word_nt, uint32_t distance, uint32_t method, uint32_t *d_cluster_id, uint8_t *d_keep,
                                humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  return run_device_long(c, d_words, d_filtered, n_reads, word_nt, distance, method, d_cluster_id, d_keep, summary);
}

// host buffers: the staging of run_host with ceil(word_nt / 32) uint64 per read; a refused shape moves nothing
int humid_dedup_run_long(humid_ctx *c, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads, uint32_t word_nt,
                         uint32_t distance, uint32_t method, uint32_t *cluster_id, uint8_t *keep, humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  state_reset(c);
  TRY(check_run_args(c, n_reads, word_nt, method, HUMID_LONG_MAX_NT));
  if (c->edit) return fail(c, HUMID_E_UNSUPPORTED, "option edit_distance is not supported for long words");
  if (n_reads && (!words || !filtered || !cluster_id || !keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  humid_summary s;
  memset(&s, 0, sizeof s);
  const size_t n = (size_t)n_reads, wbytes = (size_t)((word_nt + 31) / 32) * 8;
  ENSURE(c->in_words, n * wbytes + 16);
  ENSURE(c->in_filt, n + 8);
  ENSURE(c->out_cid, n * 4 + 8);
  ENSURE(c->out_keep, n + 8);
  HostFrame frame(c);
  HIPCHK(frame.create());
  int rc = HUMID_OK;
  hipError_t he = frame.staging_begin();
  if (he == hipSuccess && n) he = hipMemcpyAsync(c->in_words.p, words, n * wbytes, hipMemcpyHostToDevice, st);
  if (he == hipSuccess && n) he = hipMemcpyAsync(c->in_filt.p, filtered, n, hipMemcpyHostToDevice, st);
  if (he == hipSuccess) he = frame.staging_end();
  if (he != hipSuccess) rc = fail(c, HUMID_E_HIP, "copy in: %s", hipGetErrorString(he));
  if (rc == HUMID_OK)
    rc = run_device_long(c, c->in_words.as<u64>(), c->in_filt.as<u8>(), n_reads, word_nt, distance, method, c->out_cid.as<u32>(),
                         c->out_keep.as<u8>(), &s);
  if (rc == HUMID_OK) rc = frame.copy_back(n, cluster_id, keep, s);
  if (rc == HUMID_OK && summary) *summary = s;
  return rc;
}

int humid_long_info(humid_ctx *c, humid_long_info_t *out) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!out) return fail(c, HUMID_E_INVALID, "null argument");
  if (!state_has_run(c) || !c->state.long_words) return fail(c, HUMID_E_STATE, "the last run was not a long-word run");
  *out = c->lg_info;
  return HUMID_OK;
}

// the packed words and flags of the last humid_dedup_run_bases (what makeWord would have returned)
int humid_get_packed_words(humid_ctx *c, uint64_t *words, uint8_t *filtered) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!state_has_run(c)) return fail(c, HUMID_E_STATE, "no completed dedup run in this context");
  if (c->state.long_words) return fail(c, HUMID_E_STATE, "the last run was a long-word run: its words are the caller's");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)c->N, wbytes = c->word_nt > 32 ? 16 : 8;
  if (n * wbytes > c->in_words.cap || n > c->in_filt.cap) return fail(c, HUMID_E_STATE, "the last run did not go through a host entry point");
  if (n && words) HIPCHK(hipMemcpyAsync(words, c->in_words.p, n * wbytes, hipMemcpyDeviceToHost, c->stream));
  if (n && filtered) HIPCHK(hipMemcpyAsync(filtered, c->in_filt.p, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

// the internal words of a grouped run's leaves (host copy, g_wpr u64 each) -> the caller's words (layout of
// gk_word_nt) and / or the groups
static void gkey_split(const humid_ctx *c, const std::vector<u64> &iw, size_t U, uint64_t *word, uint32_t *group) {
  const u32 wb = 2 * c->gk_word_nt, wpr = c->g_wpr, out_wpr = c->gk_word_nt > 32 ? 2 : 1;
  const unsigned __int128 wmask = wb >= 128 ? ~(unsigned __int128)0 : ((unsigned __int128)1 << wb) - 1;
  for (size_t i = 0; i < U; i++) {
    const unsigned __int128 v = wpr == 2 ? ((unsigned __int128)iw[2 * i] << 64) | iw[2 * i + 1] : (unsigned __int128)iw[i];
    if (word) {
      const unsigned __int128 w = v & wmask;
      if (out_wpr == 2) { word[2 * i] = (u64)(w >> 64); word[2 * i + 1] = (u64)w; }
      else word[i] = (u64)w;
    }
    if (group) group[i] = wb >= 128 ? 0u : (u32)(v >> wb);
  }
}

#define NEED_LEAVES()                                                                         \
  do {                                                                                        \
    if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");                             \
    if (!state_has_leaves(c)) return fail(c, HUMID_E_STATE, "no completed dedup run / graph stage in this context"); \
    HIPCHK(hipSetDevice(c->device));                                                          \
    TRY(expand_compact(c));                                                                   \
  } while (0)

int humid_graph_split_info(humid_ctx *c, uint64_t *pairs_direct, uint64_t *pairs_graph, uint32_t *full_graph_built) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!state_has_leaves(c)) return fail(c, HUMID_E_STATE, "no completed dedup run / graph stage in this context");
  const bool split = c->cg_valid && c->cg_split;
  if (pairs_direct) *pairs_direct = split ? c->cg_iso : 0;
  if (pairs_graph) *pairs_graph = split ? c->cg_R : c->E;
  if (full_graph_built) *full_graph_built = (!split || c->cg_full) ? 1u : 0u;
  return HUMID_OK;
}

int humid_group_records_info(humid_ctx *c, uint32_t *searched_on_records, uint32_t *orders_stored) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!state_has_leaves(c)) return fail(c, HUMID_E_STATE, "no completed dedup run / graph stage in this context");
  if (searched_on_records) *searched_on_records = c->cg_valid ? c->gr_rides : 0u;
  if (orders_stored) *orders_stored = c->cg_valid ? c->gr_orders : 0u;
  return HUMID_OK;
}

int humid_wait_overlap_info(humid_ctx *c, uint32_t *host_waits, uint32_t *overlapped) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (c->state.holds == CtxState::NOTHING) return fail(c, HUMID_E_STATE, "no completed run or stage call in this context");
  if (host_waits) *host_waits = c->wo_waits;
  if (overlapped) *overlapped = c->wo_overlapped;
  return HUMID_OK;
}

int humid_stamp_info(humid_ctx *c, uint32_t *stamps_used, uint64_t stamps[4], uint32_t *event_records) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (c->state.holds == CtxState::NOTHING) return fail(c, HUMID_E_STATE, "no completed run or stage call in this context");
  const TimingLeft &left = c->timing_left;
  if (stamps_used) *stamps_used = left.stamp_timed ? 1u : 0u;
  if (stamps) for (u32 k = 0; k < STAMP_N; k++) stamps[k] = left.stamp_live ? left.stamps[k] : 0;
  if (event_records) *event_records = left.event_records;
  return HUMID_OK;
}

int humid_get_run_roads(humid_ctx *c, humid_run_roads *out) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!out) return fail(c, HUMID_E_INVALID, "null argument");
  if (c->state.holds == CtxState::NOTHING) return fail(c, HUMID_E_STATE, "no completed run or stage call in this context");
  *out = c->roads;
  return HUMID_OK;
}

int humid_get_leaves(humid_ctx *c, uint64_t *word, uint32_t *count, uint32_t *first_read,
                     uint32_t *degree, uint32_t *cluster_id, uint8_t *is_max_leaf) {
  NEED_LEAVES();
  size_t U = (size_t)c->gU;
  if (U == 0) return HUMID_OK;
  if (first_read && !state_has_run(c))
    return fail(c, HUMID_E_STATE, "first_read is only available after a single-GPU humid_dedup_run*");
  if (word && state_groups_are(c, RUN_GROUPED) && (c->gk_leaf_nt || c->g_wpr != (c->gk_word_nt > 32 ? 2u : 1u))) {
    // grouped internal words -> the caller's words (the group goes to humid_get_leaf_groups)
    std::vector<u64> iw(U * c->g_wpr);
    HIPCHK(hipMemcpyAsync(iw.data(), c->g_word, U * 8 * c->g_wpr, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    gkey_split(c, iw, U, word, nullptr);
  } else
    D2H(word, c->g_word, U * 8 * c->g_wpr);
  D2H(count, c->g_cnt, U * 4);
  D2H(first_read, c->s_first.p, U * 4);
  D2H(degree, c->deg.p, U * 4);
  D2H(cluster_id, c->cid.p, U * 4);
  D2H(is_max_leaf, c->ismax.p, U);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_get_leaf_groups(humid_ctx *c, uint32_t *group) {
  NEED_LEAVES();
  if (!state_groups_are(c, RUN_GROUPED)) return fail(c, HUMID_E_STATE, "the last run was not a grouped run");
  size_t U = (size_t)c->gU;
  if (U == 0 || !group) return HUMID_OK;
  if (!c->gk_leaf_nt) { memset(group, 0, U * 4); return HUMID_OK; }
  std::vector<u64> iw(U * c->g_wpr);
  HIPCHK(hipMemcpyAsync(iw.data(), c->g_word, U * 8 * c->g_wpr, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  gkey_split(c, iw, U, nullptr, group);
  return HUMID_OK;
}

int humid_get_group_keys(humid_ctx *c, uint64_t *keys, uint64_t cap, uint64_t *n_out) {
  NEED_LEAVES();
  if (!state_groups_are(c, RUN_KEYED)) return fail(c, HUMID_E_STATE, "the last run was not a keyed run");
  if (!n_out) return fail(c, HUMID_E_INVALID, "null argument");
  *n_out = c->kr_n;
  const u64 take = c->kr_n < cap ? c->kr_n : cap;
  if (take && keys) {
    D2H(keys, state_keyed_graph(c) ? c->ac_keys.p : c->kr_keys.p, take * 8);
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return HUMID_OK;
}

int humid_keyed_rank_info(humid_ctx *c, uint64_t *n_keys, uint32_t *table_log2, uint32_t *n_redo) {
  NEED_LEAVES();
  if (!state_run_is(c, RUN_KEYED)) return fail(c, HUMID_E_STATE, "the last run was not a keyed run");
  if (n_keys) *n_keys = c->kr_n;
  if (table_log2) *table_log2 = c->kr_last_log2;
  if (n_redo) *n_redo = c->kr_redo;
  return HUMID_OK;
}

// ---- barcode whitelist ---------------------------------------------------------------------------------------
int humid_whitelist_set(humid_ctx *c, const uint64_t *barcodes, uint64_t n, uint32_t barcode_nt) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (n == 0) {                                              // clear
    HIPCHK(hipStreamSynchronize(st));
    c->wl_table.release();
    seg_drop(c);
    c->wl_n = 0; c->wl_nt = 0; c->wl_log2 = 0;
    wl_counts_drop(c);
    c->cd_valid = false;
    return HUMID_OK;
  }
  if (barcode_nt < 1 || barcode_nt > 32) return fail(c, HUMID_E_INVALID, "barcode_nt must be 1 .. 32");
  if (!barcodes) return fail(c, HUMID_E_INVALID, "null buffer");
  if (n > ((u64)1 << 30)) return fail(c, HUMID_E_OVERFLOW, "a whitelist of %llu barcodes exceeds 2^30", (ull)n);
  if (barcode_nt < 32) {
    const u64 lim = (u64)1 << (2 * barcode_nt);
    for (u64 i = 0; i < n; i++)
      if (barcodes[i] >= lim)
        return fail(c, HUMID_E_INVALID, "barcode %llu = 0x%llx is not a %u-nucleotide word", (ull)i, (ull)barcodes[i], barcode_nt);
  }
  u32 log2 = 1;
  while (((u64)1 << log2) < 2 * n) log2++;
  const size_t cap = (size_t)1 << log2;
  // the new table is built beside the old one, which stays in place until the new one is complete
  DBuf fresh, stage;                                         // (both free themselves on every early return)
  HIPCHK(fresh.ensure((cap + 2) * 8));
  HIPCHK(stage.ensure((size_t)n * 8));
  HIPCHK(hipMemsetAsync(fresh.p, 0xff, (cap + 1) * 8, st));
  HIPCHK(hipMemsetAsync(fresh.as<u64>() + cap + 1, 0, 8, st));
  HIPCHK(hipMemcpyAsync(stage.p, barcodes, (size_t)n * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_wl_insert, dim3(grid_stride_blocks(n)), dim3(256), 0, st, (const u64 *)stage.p, (u32)n, fresh.as<u64>(), log2);
  HIPCHK(hipGetLastError());
  u64 distinct = 0;
  HIPCHK(hipMemcpyAsync(&distinct, fresh.as<u64>() + cap + 1, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  c->wl_table = std::move(fresh);
  seg_drop(c);
  c->wl_n = distinct; c->wl_nt = barcode_nt; c->wl_log2 = log2;
  wl_counts_drop(c);                                       // (the reads per slot went with the table they index)
  c->cd_valid = false;                                       // (nor is this whitelist one a discover call installed)
  return HUMID_OK;
}

// ---- segmented whitelist (kernels_segments.hip.h) ------------------------------------------------------------------
int humid_whitelist_set_segments(humid_ctx *c, uint32_t n_seg, const uint32_t *seg_nt, const uint64_t *seg_n, const uint64_t *barcodes,
                                 uint32_t max_inexact) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (n_seg < 1 || n_seg > SEG_MAX) return fail(c, HUMID_E_INVALID, "a segmented whitelist has 1 .. %u segments", SEG_MAX);
  if (!seg_nt || !seg_n || !barcodes) return fail(c, HUMID_E_INVALID, "null buffer");
  if (max_inexact > n_seg) return fail(c, HUMID_E_INVALID, "max_inexact %u exceeds the %u segments", max_inexact, n_seg);
  SegPlan plan = {};
  plan.n_seg = n_seg;
  plan.max_inexact = max_inexact;
  u64 total = 0, entries = 0;
  for (u32 s = 0; s < n_seg; s++) {
    if (seg_nt[s] < 1 || seg_nt[s] > SEG_MAX_NT) return fail(c, HUMID_E_INVALID, "segment %u: a segment has 1 .. %u nucleotides", s, SEG_MAX_NT);
    if (seg_n[s] == 0) return fail(c, HUMID_E_INVALID, "segment %u: the list is empty", s);
    if (seg_n[s] > ((u64)1 << 30)) return fail(c, HUMID_E_OVERFLOW, "segment %u: a list of %llu barcodes exceeds 2^30", s, (ull)seg_n[s]);
    plan.key_nt += seg_nt[s];
    plan.mask[s] = (1u << (2 * seg_nt[s])) - 1u;
    plan.off[s] = (u32)entries;
    entries += (u64)plan.mask[s] + 1;
    for (u64 i = 0; i < seg_n[s]; i++)
      if (barcodes[total + i] > plan.mask[s])
        return fail(c, HUMID_E_INVALID, "segment %u: barcode %llu = 0x%llx is not a %u-nucleotide word", s, (ull)i, (ull)barcodes[total + i],
                    seg_nt[s]);
    total += seg_n[s];
  }
  if (plan.key_nt > 32) return fail(c, HUMID_E_INVALID, "the segments add up to %u nucleotides, more than 32", plan.key_nt);
  for (u32 s = 0, below = plan.key_nt; s < n_seg; s++) {           // segment 0 is the most significant
    below -= seg_nt[s];
    plan.shift[s] = 2 * below;
  }
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // the new tables are built beside the whitelist in place, which stays until they are complete
  DBuf fresh, work, stage, ndist;                            // (all free themselves on every early return)
  HIPCHK(fresh.ensure((size_t)entries * 4));
  HIPCHK(work.ensure((size_t)entries * 4));
  HIPCHK(stage.ensure((size_t)total * 8));
  HIPCHK(ndist.ensure(SEG_MAX * sizeof(ull)));
  HIPCHK(hipMemsetAsync(fresh.p, 0xff, (size_t)entries * 4, st));
  HIPCHK(hipMemsetAsync(work.p, 0, (size_t)entries * 4, st));
  HIPCHK(hipMemsetAsync(ndist.p, 0, SEG_MAX * sizeof(ull), st));
  HIPCHK(hipMemcpyAsync(stage.p, barcodes, (size_t)total * 8, hipMemcpyHostToDevice, st));
  for (u64 s = 0, at = 0; s < n_seg; at += seg_n[s], s++) {      // (a table's entries are indexed by the subkey: one pair of launches per segment)
    hipLaunchKernelGGL(k_seg_mark, dim3(grid_stride_blocks(seg_n[s])), dim3(256), 0, st, (const u64 *)stage.p + at, (u32)seg_n[s], seg_nt[s],
                       fresh.as<u32>() + plan.off[s], work.as<u32>() + plan.off[s], ndist.as<ull>() + s);
    hipLaunchKernelGGL(k_seg_finish, dim3(grid_stride_blocks((u64)plan.mask[s] + 1)), dim3(256), 0, st, fresh.as<u32>() + plan.off[s],
                       (const u32 *)work.p + plan.off[s], plan.mask[s] + 1u);
  }
  HIPCHK(hipGetLastError());
  ull distinct[SEG_MAX] = {};
  HIPCHK(hipMemcpyAsync(distinct, ndist.p, sizeof distinct, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  unsigned __int128 product = 1;
  for (u32 s = 0; s < n_seg; s++) product *= distinct[s];
  c->wl_table.release();
  c->sg_table = std::move(fresh);
  c->sg = plan;
  for (u32 s = 0; s < SEG_MAX; s++) c->sg_distinct[s] = distinct[s];
  c->sg_sum_valid = false;
  c->wl_n = product > (unsigned __int128)~0ull ? ~0ull : (u64)product;   // (all 4^32 keys of K = 32: one more than a u64 holds)
  c->wl_nt = plan.key_nt; c->wl_log2 = 0;
  wl_counts_drop(c);
  c->cd_valid = false;
  return HUMID_OK;
}

int humid_whitelist_segments_info(humid_ctx *c, uint32_t *n_seg, uint32_t seg_nt[8], uint64_t seg_n[8], uint32_t *max_inexact) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (n_seg) *n_seg = c->sg.n_seg;
  if (max_inexact) *max_inexact = c->sg.max_inexact;
  for (u32 s = 0; s < SEG_MAX; s++) {
    u32 nt = 0;
    for (u32 m = s < c->sg.n_seg ? c->sg.mask[s] : 0u; m; m >>= 2) nt++;
    if (seg_nt) seg_nt[s] = nt;
    if (seg_n) seg_n[s] = s < c->sg.n_seg ? c->sg_distinct[s] : 0;
  }
  return HUMID_OK;
}

int humid_get_barcode_segments(humid_ctx *c, uint64_t seg_counts[32], uint64_t inexact_hist[9]) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->sg.n_seg || !c->sg_sum_valid)
    return fail(c, HUMID_E_STATE, "no correction has run over a segmented whitelist of this context (humid_whitelist_set_segments)");
  HIPCHK(hipSetDevice(c->device));
  D2H(seg_counts, c->sg_sum.p, SEG_SUM_HIST * sizeof(ull));
  D2H(inexact_hist, c->sg_sum.as<ull>() + SEG_SUM_HIST, (SEG_MAX + 1) * sizeof(ull));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_whitelist_info(humid_ctx *c, uint64_t *n_distinct, uint32_t *barcode_nt, uint32_t *table_log2) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (n_distinct) *n_distinct = c->wl_n;
  if (barcode_nt) *barcode_nt = c->wl_nt;
  if (table_log2) *table_log2 = c->wl_log2;
  return HUMID_OK;
}

static int whitelist_correct_args(humid_ctx *c, const void *key, const void *filtered, uint64_t n_reads) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->wl_n) return fail(c, HUMID_E_STATE, "no whitelist is set in this context (humid_whitelist_set)");
  if (n_reads > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "n_reads %llu exceeds 2^31-1", (ull)n_reads);
  if (n_reads && (!key || !filtered)) return fail(c, HUMID_E_INVALID, "null buffer");
  return HUMID_OK;
}

int humid_whitelist_correct_device(humid_ctx *c, const uint64_t *d_key, const uint8_t *d_filtered, uint64_t n_reads,
                                   uint64_t *d_key_out, uint8_t *d_status, uint64_t counts[5]) {
  TRY(whitelist_correct_args(c, d_key, d_filtered, n_reads));
  HIPCHK(hipSetDevice(c->device));
  PASS_ENSURE(c->wc_counts, 5 * sizeof(ull));
  TRY(wl_correct_launch(c, d_key, d_filtered, (u32)n_reads, d_key_out, d_status, nullptr, c->wc_counts.as<ull>()));
  D2H(counts, c->wc_counts.p, 5 * sizeof(ull));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_whitelist_correct(humid_ctx *c, const uint64_t *key, const uint8_t *filtered, uint64_t n_reads,
                            uint64_t *key_out, uint8_t *status, uint64_t counts[5]) {
  TRY(whitelist_correct_args(c, key, filtered, n_reads));
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads;
  u64 *d_key, *d_out;
  u8 *d_filt, *d_status;
  STAGE_IN(d_key, 0, key, n * 8);
  STAGE_IN(d_filt, 1, filtered, n);
  STAGE_OUT(d_out, 0, n * 8);
  STAGE_OUT(d_status, 1, n);
  PASS_ENSURE(c->wc_counts, 5 * sizeof(ull));
  TRY(wl_correct_launch(c, d_key, d_filt, (u32)n, d_out, d_status, nullptr, c->wc_counts.as<ull>()));
  D2H(key_out, d_out, n * 8);
  D2H(status, d_status, n);
  D2H(counts, c->wc_counts.p, 5 * sizeof(ull));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

// ---- whitelist from the data (kernels_cells.hip.h) -----------------------------------------------------------------
int humid_whitelist_discover_device(humid_ctx *c, const uint64_t *d_key, const uint8_t *d_filtered, uint64_t n_reads,
                                    uint32_t barcode_nt, uint32_t mode, uint64_t param, uint32_t merge_ratio,
                                    humid_cells_summary *summary) {
  TRY(cells_discover_args(c, d_key, d_filtered, n_reads, barcode_nt, mode, param));
  return cells_discover_device(c, d_key, d_filtered, n_reads, barcode_nt, mode, param, merge_ratio, summary);
}

int humid_whitelist_discover(humid_ctx *c, const uint64_t *key, const uint8_t *filtered, uint64_t n_reads, uint32_t barcode_nt,
                             uint32_t mode, uint64_t param, uint32_t merge_ratio, humid_cells_summary *summary) {
  TRY(cells_discover_args(c, key, filtered, n_reads, barcode_nt, mode, param));
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads;
  u64 *d_key;
  u8 *d_filt;
  STAGE_IN(d_key, 0, key, n * 8);
  STAGE_IN(d_filt, 1, filtered, n);
  return cells_discover_device(c, d_key, d_filt, n_reads, barcode_nt, mode, param, merge_ratio, summary);
}

int humid_get_discovered_cells(humid_ctx *c, uint64_t *barcodes, uint32_t *reads, uint64_t cap, uint64_t *n_out) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->cd_valid) return fail(c, HUMID_E_STATE, "the whitelist of this context was not installed by humid_whitelist_discover");
  if (n_out) *n_out = c->cd_n_cells;
  const u64 take = c->cd_n_cells < cap ? c->cd_n_cells : cap;
  if (take && (barcodes || reads)) {
    HIPCHK(hipSetDevice(c->device));
    D2H(barcodes, c->cd_cells.p, (size_t)take * 8);
    D2H(reads, c->cd_cellcnt.p, (size_t)take * 4);
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return HUMID_OK;
}

int humid_get_barcode_count_hist(humid_ctx *c, uint64_t *reads, uint64_t *barcodes, uint64_t cap, uint64_t *n_out) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->cd_valid) return fail(c, HUMID_E_STATE, "the whitelist of this context was not installed by humid_whitelist_discover");
  if (!n_out) return fail(c, HUMID_E_INVALID, "null argument");
  const u64 H = c->cd_n_hist;
  *n_out = H;
  const u64 take = H < cap ? H : cap;
  if (take == 0 || (!reads && !barcodes)) return HUMID_OK;
  HIPCHK(hipSetDevice(c->device));
  // bin q starts at rank first[q] of the order by descending count; the bin below it (q - 1) is the run behind it
  std::vector<u32> first((size_t)take);
  D2H(reads, c->cd_hist_n.p, (size_t)take * 8);
  D2H(first.data(), c->cd_hist_first.p, (size_t)take * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (barcodes)
    for (u64 q = 0; q < take; q++) barcodes[q] = (q == 0 ? c->cd_G : (u64)first[(size_t)q - 1]) - (u64)first[(size_t)q];
  return HUMID_OK;
}

// ---- the barcode counter fed in chunks (kernels_cells.hip.h) ---------------------------------------------------------
#define CELLS_NEED_COUNTER()                                                                                                   \
  do {                                                                                                                         \
    if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");                                                              \
    if (c->cc_state == CC_NONE) return fail(c, HUMID_E_STATE, "no barcode counter is open in this context (humid_cells_begin)"); \
    if (c->cc_state == CC_INVALID)                                                                                             \
      return fail(c, HUMID_E_STATE, "the barcode counter is invalid after a failed add (humid_cells_begin starts a new one)");  \
  } while (0)

int humid_cells_begin(humid_ctx *c, uint32_t barcode_nt) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (barcode_nt < 1 || barcode_nt > 32) return fail(c, HUMID_E_INVALID, "barcode_nt must be 1 .. 32");
  return cells_accum_begin(c, barcode_nt);
}

static int cells_add_args(humid_ctx *c, const void *key, const void *filtered, uint64_t n_reads) {
  CELLS_NEED_COUNTER();
  if (n_reads && (!key || !filtered)) return fail(c, HUMID_E_INVALID, "null buffer");
  if (n_reads > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "n_reads %llu exceeds 2^31-1", (ull)n_reads);
  return HUMID_OK;
}

int humid_cells_add_device(humid_ctx *c, const uint64_t *d_key, const uint8_t *d_filtered, uint64_t n_reads) {
  TRY(cells_add_args(c, d_key, d_filtered, n_reads));
  HIPCHK(hipSetDevice(c->device));
  return cells_accum_add(c, d_key, d_filtered, n_reads);
}

int humid_cells_add(humid_ctx *c, const uint64_t *key, const uint8_t *filtered, uint64_t n_reads) {
  TRY(cells_add_args(c, key, filtered, n_reads));
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads;
  u64 *d_key = nullptr;
  u8 *d_filt = nullptr;
  if (n) {
    const int rc = [&]() -> int {
      STAGE_IN(d_key, 0, key, n * 8);
      STAGE_IN(d_filt, 1, filtered, n);
      return HUMID_OK;
    }();
    if (rc != HUMID_OK) {                                        // (an allocation or HIP failure during an add)
      c->cc_state = CC_INVALID;
      return rc;
    }
  }
  return cells_accum_add(c, d_key, d_filt, n_reads);
}

int humid_cells_finish(humid_ctx *c, uint32_t mode, uint64_t param, uint32_t merge_ratio, humid_cells_summary *summary) {
  CELLS_NEED_COUNTER();
  if (mode > HUMID_CELLS_MIN_READS) return fail(c, HUMID_E_INVALID, "mode %u is none of HUMID_CELLS_TOP, _EXPECTED, _MIN_READS", mode);
  if (param == 0) return fail(c, HUMID_E_INVALID, "the mode's parameter must be >= 1");
  return cells_accum_finish(c, mode, param, merge_ratio, summary);
}

int humid_cells_info(humid_ctx *c, uint32_t *barcode_nt, uint64_t *chunks, uint64_t *reads, uint64_t *usable, uint64_t *invalid_reads,
                     uint64_t *distinct, uint32_t *table_log2, uint32_t *n_grown) {
  CELLS_NEED_COUNTER();
  if (barcode_nt) *barcode_nt = c->cc_nt;
  if (chunks) *chunks = c->cc_chunks;
  if (reads) *reads = c->cc_reads;
  if (usable) *usable = c->cc_usable;
  if (invalid_reads) *invalid_reads = c->cc_invalid;
  if (distinct) *distinct = c->cc_distinct;
  if (table_log2) *table_log2 = c->cc_log2;
  if (n_grown) *n_grown = c->cc_grown;
  return HUMID_OK;
}

int humid_cells_clear(humid_ctx *c) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (c->cc_state == CC_NONE) return fail(c, HUMID_E_STATE, "no barcode counter is open in this context (humid_cells_begin)");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->cc_table.release();
  c->cc_cnt.release();
  c->cc_ctr.release();
  c->cc_pend.release();
  c->cc_state = CC_NONE;
  return HUMID_OK;
}

// ---- correction by quality and abundance (kernels_wlpost.hip.h) ------------------------------------------------
static int whitelist_posterior_args(humid_ctx *c, const void *key, const void *qual, const void *filtered, uint64_t n_reads,
                                    uint32_t min_odds) {
  TRY(whitelist_correct_args(c, key, filtered, n_reads));
  if (c->sg.n_seg) return fail(c, HUMID_E_UNSUPPORTED, SEG_NO_POSTERIOR);
  if (min_odds == 0) return fail(c, HUMID_E_INVALID, "min_odds must be >= 1");
  if (n_reads && !qual) return fail(c, HUMID_E_INVALID, "null buffer");
  return HUMID_OK;
}

// the stand-alone call's one host wait: the seven counters -> the summary
static int whitelist_posterior_finish(humid_ctx *c, humid_bc_posterior_summary *summary) {
  ull h[WLP_CTRS] = {};
  if (summary) HIPCHK(hipMemcpyAsync(h, c->wc_counts.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (summary) {
    for (int i = 0; i < 5; i++) summary->counts[i] = h[i];
    summary->multi = h[WLP_MULTI];
    summary->rescued = h[WLP_RESCUED];
  }
  return HUMID_OK;
}

int humid_whitelist_correct_posterior_device(humid_ctx *c, const uint64_t *d_key, const uint8_t *d_qual, const uint8_t *d_filtered,
                                             uint64_t n_reads, uint32_t min_odds, uint64_t *d_key_out, uint8_t *d_status,
                                             humid_bc_posterior_summary *summary) {
  TRY(whitelist_posterior_args(c, d_key, d_qual, d_filtered, n_reads, min_odds));
  HIPCHK(hipSetDevice(c->device));
  PASS_ENSURE(c->wc_counts, WLP_CTRS * sizeof(ull));
  TRY(wl_posterior_launch(c, d_key, d_filtered, d_qual, (u32)n_reads, min_odds, d_key_out, d_status, nullptr, c->wc_counts.as<ull>()));
  return whitelist_posterior_finish(c, summary);
}

int humid_whitelist_correct_posterior(humid_ctx *c, const uint64_t *key, const uint8_t *qual, const uint8_t *filtered,
                                      uint64_t n_reads, uint32_t min_odds, uint64_t *key_out, uint8_t *status,
                                      humid_bc_posterior_summary *summary) {
  TRY(whitelist_posterior_args(c, key, qual, filtered, n_reads, min_odds));
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads;
  u64 *d_key, *d_out;
  u8 *d_filt, *d_qual, *d_status;
  STAGE_IN(d_key, 0, key, n * 8);
  STAGE_IN(d_filt, 1, filtered, n);
  STAGE_IN(d_qual, 2, qual, n * c->wl_nt);
  STAGE_OUT(d_out, 0, n * 8);
  STAGE_OUT(d_status, 1, n);
  PASS_ENSURE(c->wc_counts, WLP_CTRS * sizeof(ull));
  TRY(wl_posterior_launch(c, d_key, d_filt, d_qual, (u32)n, min_odds, d_out, d_status, nullptr, c->wc_counts.as<ull>()));
  D2H(key_out, d_out, n * 8);
  D2H(status, d_status, n);
  return whitelist_posterior_finish(c, summary);
}

// ---- the posterior's prior fed in chunks -----------------------------------------------------------------------------
int humid_whitelist_prior_begin(humid_ctx *c) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->wl_n) return fail(c, HUMID_E_STATE, "no whitelist is set in this context (humid_whitelist_set)");
  if (c->sg.n_seg) return fail(c, HUMID_E_UNSUPPORTED, SEG_NO_POSTERIOR);
  return wl_prior_begin(c);
}

// what the prior calls refuse before anything moves: no whitelist, a segmented one, no (valid) prior
static int whitelist_prior_state(humid_ctx *c) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->wl_n) return fail(c, HUMID_E_STATE, "no whitelist is set in this context (humid_whitelist_set)");
  if (c->sg.n_seg) return fail(c, HUMID_E_UNSUPPORTED, SEG_NO_POSTERIOR);
  if (c->pr_state == CC_NONE)
    return fail(c, HUMID_E_STATE, "no prior is open over the whitelist of this context (humid_whitelist_prior_begin)");
  if (c->pr_state == CC_INVALID)
    return fail(c, HUMID_E_STATE, "the prior is invalid after a failed add (humid_whitelist_prior_begin starts a new one)");
  return HUMID_OK;
}

int humid_whitelist_prior_add_device(humid_ctx *c, const uint64_t *d_key, const uint8_t *d_filtered, uint64_t n_reads) {
  TRY(whitelist_prior_state(c));
  TRY(whitelist_correct_args(c, d_key, d_filtered, n_reads));
  HIPCHK(hipSetDevice(c->device));
  return wl_prior_add(c, d_key, d_filtered, (u32)n_reads);
}

int humid_whitelist_prior_add(humid_ctx *c, const uint64_t *key, const uint8_t *filtered, uint64_t n_reads) {
  TRY(whitelist_prior_state(c));
  TRY(whitelist_correct_args(c, key, filtered, n_reads));
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads;
  u64 *d_key = nullptr;
  u8 *d_filt = nullptr;
  const int rc = [&]() -> int {
    STAGE_IN(d_key, 0, key, n * 8);
    STAGE_IN(d_filt, 1, filtered, n);
    return HUMID_OK;
  }();
  if (rc != HUMID_OK) {                                          // (an allocation or HIP failure during an add)
    c->pr_state = CC_INVALID;
    return rc;
  }
  return wl_prior_add(c, d_key, d_filt, (u32)n);
}

int humid_whitelist_correct_posterior_prior_device(humid_ctx *c, const uint64_t *d_key, const uint8_t *d_qual, const uint8_t *d_filtered,
                                                   uint64_t n_reads, uint32_t min_odds, uint64_t *d_key_out, uint8_t *d_status,
                                                   humid_bc_posterior_summary *summary) {
  TRY(whitelist_prior_state(c));
  TRY(whitelist_posterior_args(c, d_key, d_qual, d_filtered, n_reads, min_odds));
  HIPCHK(hipSetDevice(c->device));
  PASS_ENSURE(c->wc_counts, WLP_CTRS * sizeof(ull));
  TRY(wl_posterior_prior_launch(c, d_key, d_filtered, d_qual, (u32)n_reads, min_odds, d_key_out, d_status, c->wc_counts.as<ull>()));
  return whitelist_posterior_finish(c, summary);
}

int humid_whitelist_correct_posterior_prior(humid_ctx *c, const uint64_t *key, const uint8_t *qual, const uint8_t *filtered,
                                            uint64_t n_reads, uint32_t min_odds, uint64_t *key_out, uint8_t *status,
                                            humid_bc_posterior_summary *summary) {
  TRY(whitelist_prior_state(c));
  TRY(whitelist_posterior_args(c, key, qual, filtered, n_reads, min_odds));
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads;
  u64 *d_key, *d_out;
  u8 *d_filt, *d_qual, *d_status;
  STAGE_IN(d_key, 0, key, n * 8);
  STAGE_IN(d_filt, 1, filtered, n);
  STAGE_IN(d_qual, 2, qual, n * c->wl_nt);
  STAGE_OUT(d_out, 0, n * 8);
  STAGE_OUT(d_status, 1, n);
  PASS_ENSURE(c->wc_counts, WLP_CTRS * sizeof(ull));
  TRY(wl_posterior_prior_launch(c, d_key, d_filt, d_qual, (u32)n, min_odds, d_out, d_status, c->wc_counts.as<ull>()));
  D2H(key_out, d_out, n * 8);
  D2H(status, d_status, n);
  return whitelist_posterior_finish(c, summary);
}

int humid_get_barcode_posterior(humid_ctx *c, uint64_t *multi, uint64_t *rescued) {
  NEED_LEAVES();
  if (!state_run_is(c, RUN_CORRECTED) || !c->bc_posterior)
    return fail(c, HUMID_E_STATE, "the last run was not a posterior corrected keyed run");
  D2H(multi, c->bc_counts.as<ull>() + WLP_MULTI, sizeof(ull));
  D2H(rescued, c->bc_counts.as<ull>() + WLP_RESCUED, sizeof(ull));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_whitelist_counts(humid_ctx *c, const uint64_t *barcodes, uint64_t n, uint32_t *counts_out) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  const bool prior = c->wp_prior && c->pr_state == CC_ON;       // the later of the two: an accumulated prior, or a one-shot posterior
  if (!c->wl_n || !(prior || c->wp_valid))
    return fail(c, HUMID_E_STATE, "no posterior correction has run over the whitelist of this context");
  if (n > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "%llu barcodes exceed 2^31-1", (ull)n);
  if (n && (!barcodes || !counts_out)) return fail(c, HUMID_E_INVALID, "null buffer");
  if (n == 0) return HUMID_OK;
  HIPCHK(hipSetDevice(c->device));
  u64 *d_bc;
  u32 *d_out;
  STAGE_IN(d_bc, 0, barcodes, (size_t)n * 8);
  STAGE_OUT(d_out, 0, (size_t)n * 4);
  hipLaunchKernelGGL(k_wlp_counts, dim3(grid_stride_blocks(n)), dim3(256), 0, c->stream, (const u64 *)d_bc, (u32)n,
                     (const u64 *)c->wl_table.p, c->wl_log2, (const u32 *)(prior ? c->pr_cnt.p : c->wp_cnt.p), d_out);
  HIPCHK(hipGetLastError());
  D2H(counts_out, d_out, (size_t)n * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_get_barcode_status(humid_ctx *c, uint8_t *status, uint64_t cap, uint64_t counts[5]) {
  NEED_LEAVES();
  if (!state_run_is(c, RUN_CORRECTED)) return fail(c, HUMID_E_STATE, "the last run was not a corrected keyed run");
  const size_t take = (size_t)(c->bc_N < cap ? c->bc_N : cap);
  D2H(status, c->bc_status.p, take);
  D2H(counts, c->bc_counts.p, 5 * sizeof(ull));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_grouped_plan_info(humid_ctx *c, uint32_t word_nt, uint32_t n_groups, uint32_t distance, uint64_t n_unique,
                            uint32_t *n_combos, uint32_t *key_bits, uint32_t *group_nt) {
  // pure host arithmetic: ctx may be NULL (no GPU needed; the automatic plan is reported)
  TRY(check_run_args(c, 0, word_nt, 0, 64));
  TRY(check_grouped_args(c, word_nt, n_groups));
  const u32 gnt = gkey_nt_for(n_groups);
  const ComboPlan plan = make_plan(word_nt, distance, n_unique, c ? c->force_segments : 0u, true, gnt);
  if (plan.ncombo == 0 || plan.ncombo > MAX_COMBOS) return fail(c, HUMID_E_INVALID, "internal: bad pigeonhole plan");
  if (n_combos) *n_combos = plan.ncombo;
  if (key_bits) *key_bits = plan.key_bits;
  if (group_nt) *group_nt = gnt;
  return HUMID_OK;
}

int humid_get_adjacency(humid_ctx *c, uint32_t *nbr_off, uint32_t *nbr_idx) {
  NEED_LEAVES();
  size_t U = (size_t)c->gU;
  if (U == 0) { if (nbr_off) nbr_off[0] = 0; return HUMID_OK; }
  D2H(nbr_off, c->nbr_off.p, (U + 1) * 4);
  D2H(nbr_idx, c->nbr_idx.p, (size_t)(2 * c->E) * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

static int export_clusters(humid_ctx *c, u32 U, u64 C, uint64_t *size, uint32_t *max_count, uint32_t *max_leaf) {
  if (C == 0) return HUMID_OK;
  ENSURE(c->scratch, (size_t)C * 16);
  u64 *d_size = c->scratch.as<u64>();
  u32 *d_mc = (u32 *)(d_size + C);
  u32 *d_ml = d_mc + C;
  hipLaunchKernelGGL(k_export_clusters, dim3(blocks_for(U)), dim3(256), 0, c->stream, c->flag.as<u32>(),
                     c->pos.as<u32>(), c->maxleaf.as<u32>(), c->cl_size.as<u64>(), c->g_cnt, U,
                     d_size, d_mc, d_ml);
  HIPCHK(hipGetLastError());
  D2H(size, d_size, (size_t)C * 8);
  D2H(max_count, d_mc, (size_t)C * 4);
  D2H(max_leaf, d_ml, (size_t)C * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_get_clusters(humid_ctx *c, uint64_t *size, uint32_t *max_count, uint32_t *max_leaf) {
  NEED_LEAVES();
  return export_clusters(c, c->gU, c->C, size, max_count, max_leaf);
}

int humid_get_histogram(humid_ctx *c, uint32_t which, uint64_t *keys, uint64_t *values, uint64_t cap,
                        uint64_t *n_out) {
  NEED_LEAVES();
  if (which > 2 || !n_out) return fail(c, HUMID_E_INVALID, "bad histogram selector");
  *n_out = 0;
  const u32 U = c->gU;
  u64 n = (which == 2) ? c->C : U;
  if (n == 0) return HUMID_OK;
  hipStream_t st = c->stream;
  // layout of scratch: vals[n] | sorted[n] | uniq[n] | counts u32[n] | head u32[n + 1] | hpos u32[n + 1] | start u32[n + 1]
  ENSURE(c->scratch, (size_t)n * 40 + 64);
  u64 *vals = c->scratch.as<u64>();
  u64 *sorted = vals + n;
  u64 *uniq = sorted + n;
  u32 *counts = (u32 *)(uniq + n);
  u32 *head = counts + n, *hpos = head + n + 1, *start = hpos + n + 1;
  u32 *runs = hpos + n;                                      // the scan's last entry = number of runs
  if (which == 0) hipLaunchKernelGGL(k_widen32, dim3(blocks_for(U)), dim3(256), 0, st, c->g_cnt, U, vals);
  else if (which == 1) hipLaunchKernelGGL(k_widen32, dim3(blocks_for(U)), dim3(256), 0, st, c->deg.as<u32>(), U, vals);
  else hipLaunchKernelGGL(k_creator_sizes, dim3(blocks_for(U)), dim3(256), 0, st, c->flag.as<u32>(),
                          c->pos.as<u32>(), c->cl_size.as<u64>(), U, vals);
  TRY(sort_keys<u64>(c, vals, sorted, n, 0, 64));
  // run-length encode: head flags, their scan, (value, first position) per run, lengths by difference
  hipLaunchKernelGGL(k_rle_heads, dim3(blocks_for(n + 1)), dim3(256), 0, st, sorted, (u32)n, head);
  TRY(exscan_u32(c, head, hpos, n + 1));
  hipLaunchKernelGGL(k_rle_runs, dim3(blocks_for(n + 1)), dim3(256), 0, st, sorted, (const u32 *)head, (const u32 *)hpos, (u32)n, uniq, start);
  hipLaunchKernelGGL(k_rle_counts, dim3(blocks_for(n)), dim3(256), 0, st, (const u32 *)start, (const u32 *)runs, counts);
  HIPCHK(hipGetLastError());
  u32 h_runs = 0;
  HIPCHK(hipMemcpyAsync(&h_runs, runs, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *n_out = h_runs;
  u64 take = h_runs < cap ? h_runs : cap;
  if (take && keys && values) {
    std::vector<u32> hc(take);
    HIPCHK(hipMemcpyAsync(keys, uniq, (size_t)take * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hc.data(), counts, (size_t)take * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (u64 i = 0; i < take; i++) values[i] = hc[i];
  }
  return HUMID_OK;
}

// Per-group statistics of the last single-GPU run, left in c->gs_* (kernels_gstats.hip.h): one exclusive scan over
// the leaves, one lower-bound search per group boundary, one difference per group.  Runs on the first call after a
// run; every later call finds the record's stats_current.  Nothing of g_word is copied to the host.
static int group_stats(humid_ctx *c) {
  if (!state_has_run(c) && !state_keyed_graph(c))
    return fail(c, HUMID_E_STATE, "group statistics need a completed single-GPU humid_dedup_run*");
  if (c->state.long_words) return fail(c, HUMID_E_STATE, "group statistics are not available after a long-word run");
  if (c->state.stats_current) return HUMID_OK;
  // (the scan below carries the reads in 32 bits: a run holds fewer, the reads of a keyed accumulator need not)
  if (c->usable > 0xffffffffull)
    return fail(c, HUMID_E_UNSUPPORTED, "group statistics over %llu accumulated reads (more than 2^32-1)", (ull)c->usable);
  hipStream_t st = c->stream;
  const u32 U = c->gU;
  const u32 G = state_groups_are(c, RUN_KEYED) ? c->kr_n : state_run_is(c, RUN_GROUPED) ? c->gk_groups : 1u;
  const size_t off_bytes = ((size_t)G + 1) * 4;
  ENSURE(c->gs_loff, off_bytes);
  ENSURE(c->gs_coff, off_bytes);
  ENSURE(c->gs_reads, (size_t)G * 8 + 8);
  ENSURE(c->gs_edges, (size_t)G * 4 + 4);
  if (U == 0 || G == 0) {                                    // no leaf: every range is empty, nothing indexes the leaf arrays
    HIPCHK(hipMemsetAsync(c->gs_loff.p, 0, off_bytes, st));
    HIPCHK(hipMemsetAsync(c->gs_coff.p, 0, off_bytes, st));
    HIPCHK(hipMemsetAsync(c->gs_reads.p, 0, (size_t)G * 8 + 8, st));
    HIPCHK(hipMemsetAsync(c->gs_edges.p, 0, (size_t)G * 4 + 4, st));
  } else {
    ENSURE(c->gs_ps, (size_t)U * 8);
    TRY(exscan_in<u64>(c, GsPairIn{c->g_cnt, c->deg.as<u32>()}, c->gs_ps.as<u64>(), U));
    const u32 gnt = state_groups_are(c, RUN_GROUPED) ? c->gk_leaf_nt : 0u, wb = 2 * c->gk_word_nt;
    const u32 nb = grid_stride_blocks((u64)G + 1);
    if (c->g_wpr == 2)
      hipLaunchKernelGGL(k_gs_offsets<W2>, dim3(nb), dim3(256), 0, st, (const W2 *)c->g_word, c->pos.as<u32>(), U, (u32)c->C, wb,
                         gnt, G, c->gs_loff.as<u32>(), c->gs_coff.as<u32>());
    else
      hipLaunchKernelGGL(k_gs_offsets<u64>, dim3(nb), dim3(256), 0, st, (const u64 *)c->g_word, c->pos.as<u32>(), U, (u32)c->C, wb,
                         gnt, G, c->gs_loff.as<u32>(), c->gs_coff.as<u32>());
    hipLaunchKernelGGL(k_gs_sums, dim3(grid_stride_blocks(G)), dim3(256), 0, st, (const u32 *)c->gs_loff.p,
                       (const u64 *)c->gs_ps.p, U, (u64)c->usable | ((u64)(2 * c->E) << 32), G, c->gs_reads.as<u64>(),
                       c->gs_edges.as<u32>());
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(st));
  c->gs_G = G;
  c->state.stats_current = true;
  return HUMID_OK;
}

int humid_get_group_stats(humid_ctx *c, uint64_t cap, uint64_t *n_out, uint64_t *reads, uint32_t *leaf_off,
                          uint32_t *cluster_off, uint32_t *edges) {
  NEED_LEAVES();
  TRY(group_stats(c));
  if (n_out) *n_out = c->gs_G;
  const size_t take = (size_t)(c->gs_G < cap ? c->gs_G : cap);
  D2H(reads, c->gs_reads.p, take * 8);
  D2H(leaf_off, c->gs_loff.p, (take + 1) * 4);
  D2H(cluster_off, c->gs_coff.p, (take + 1) * 4);
  D2H(edges, c->gs_edges.p, take * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_group_stats_device(humid_ctx *c, uint64_t *n_out, const uint64_t **d_reads, const uint32_t **d_leaf_off,
                             const uint32_t **d_cluster_off, const uint32_t **d_edges) {
  NEED_LEAVES();
  TRY(group_stats(c));
  if (n_out) *n_out = c->gs_G;
  if (d_reads) *d_reads = c->gs_reads.as<u64>();
  if (d_leaf_off) *d_leaf_off = c->gs_loff.as<u32>();
  if (d_cluster_off) *d_cluster_off = c->gs_coff.as<u32>();
  if (d_edges) *d_edges = c->gs_edges.as<u32>();
  return HUMID_OK;
}

// ---- strand-symmetric (duplex) deduplication (kernels_paired.hip.h) ------------------------------------------------
static int paired_canonical_args(humid_ctx *c, const void *words, const void *filtered, uint64_t n_reads, uint32_t word_nt,
                                 const void *words_out, const void *strand_out) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  TRY(check_paired_args(c, word_nt));
  if (n_reads > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "n_reads %llu exceeds 2^31-1", (ull)n_reads);
  if (n_reads && (!words || !filtered || !words_out || !strand_out)) return fail(c, HUMID_E_INVALID, "null buffer");
  return HUMID_OK;
}

int humid_paired_canonical_device(humid_ctx *c, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                                  uint32_t word_nt, uint64_t *d_words_out, uint8_t *d_strand_out) {
  TRY(paired_canonical_args(c, d_words, d_filtered, n_reads, word_nt, d_words_out, d_strand_out));
  if (word_nt > 32 && (((uintptr_t)d_words | (uintptr_t)d_words_out) & 15))
    return fail(c, HUMID_E_INVALID, "wide words must be 16-byte aligned on the device");
  HIPCHK(hipSetDevice(c->device));
  TRY(with_word_type(word_nt, [&](auto *w) {
    typedef typename std::remove_const<typename std::remove_pointer<decltype(w)>::type>::type WT;
    return pd_canonical_launch<WT>(c, (const WT *)d_words, d_filtered, (u32)n_reads, word_nt, (WT *)d_words_out, d_strand_out);
  }));
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_paired_canonical(humid_ctx *c, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads, uint32_t word_nt,
                           uint64_t *words_out, uint8_t *strand_out) {
  TRY(paired_canonical_args(c, words, filtered, n_reads, word_nt, words_out, strand_out));
  if (n_reads == 0) return HUMID_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads, wbytes = word_nt > 32 ? 16 : 8;
  u64 *d_words;
  u8 *d_filt, *d_strand;
  STAGE_IN(d_words, 0, words, n * wbytes);
  STAGE_IN(d_filt, 1, filtered, n);
  STAGE_OUT(d_strand, 0, n);
  TRY(with_word_type(word_nt, [&](auto *w) {
    typedef typename std::remove_const<typename std::remove_pointer<decltype(w)>::type>::type WT;
    return pd_canonical_launch<WT>(c, (const WT *)d_words, d_filt, (u32)n, word_nt, (WT *)d_words, d_strand);
  }));
  // (in place on the device: the staged copy of a filtered read's word comes back as it went in)
  D2H(words_out, d_words, n * wbytes);
  D2H(strand_out, d_strand, n);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_dedup_run_paired_device(humid_ctx *c, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads,
                                  uint32_t word_nt, uint32_t distance, uint32_t method, uint32_t *d_cluster_id,
                                  uint8_t *d_keep, humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  state_reset(c);
  TRY(check_paired_args(c, word_nt));
  return with_word_type(word_nt, [&](auto *w) {
    return run_paired_device(c, (decltype(w))d_words, d_filtered, n_reads, word_nt, distance, method, d_cluster_id, d_keep, summary);
  });
}

int humid_dedup_run_paired(humid_ctx *c, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads, uint32_t word_nt,
                           uint32_t distance, uint32_t method, uint32_t *cluster_id, uint8_t *keep, humid_summary *summary) {
  return run_host(c, RUN_PLAIN, true, words, filtered, nullptr, nullptr, 1, nullptr, n_reads, word_nt, distance, method, cluster_id, keep,
                  summary);
}

int humid_get_strands(humid_ctx *c, uint8_t *strand, uint64_t cap, uint32_t *top, uint32_t *bottom, humid_strand_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!state_has_run(c) || !c->state.paired) return fail(c, HUMID_E_STATE, "the last run was not a strand-symmetric run");
  HIPCHK(hipSetDevice(c->device));
  const size_t take = (size_t)(c->pd_N < cap ? c->pd_N : cap), C = (size_t)c->pd_sum.n_clusters;
  D2H(strand, c->pd_strand.p, take);
  D2H(top, c->pd_top.as<u32>() + 1, C * 4);
  D2H(bottom, c->pd_bottom.as<u32>() + 1, C * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (summary) *summary = c->pd_sum;
  return HUMID_OK;
}

// ---- best-scoring read per cluster (kernels_best.hip.h) --------------------------------------------------------
// what both entry points refuse before anything moves; n_reads == 0 is the caller's to return HUMID_OK on
static int select_best_args(humid_ctx *c, const void *words, const void *cid, const void *keep, const void *score,
                            uint64_t n_reads, uint32_t word_nt, uint32_t scope, const void *keep_out) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (scope > HUMID_BEST_CLUSTER) return fail(c, HUMID_E_INVALID, "scope must be 0 (leaf) or 1 (cluster)");
  if (!state_has_run(c))
    return fail(c, HUMID_E_INVALID, "humid_select_best needs a completed single-GPU humid_dedup_run* in this context");
  // words of k uint64: best_pass reads one or two per read (the word_nt == c->word_nt test below refused every length
  // beyond 64 only while no run could have one)
  if (c->state.long_words) return fail(c, HUMID_E_STATE, "humid_select_best is not available after a long-word run");
  if (word_nt > 64) return fail(c, HUMID_E_UNSUPPORTED, "word_nt %u > 64 is not supported by this entry point", word_nt);
  if (n_reads != c->N || word_nt != c->word_nt)
    return fail(c, HUMID_E_INVALID, "humid_select_best: %llu reads of %u nt, the last run had %llu of %u", (ull)n_reads, word_nt,
                (ull)c->N, c->word_nt);
  if (n_reads && (!words || !cid || !keep || !score || !keep_out)) return fail(c, HUMID_E_INVALID, "null buffer");
  return HUMID_OK;
}

int humid_select_best_device(humid_ctx *c, const uint64_t *d_words, const uint32_t *d_cluster_id, const uint8_t *d_keep,
                             const uint32_t *d_score, uint64_t n_reads, uint32_t word_nt, uint32_t scope,
                             uint8_t *d_keep_out, uint32_t *d_rep_out, uint64_t *n_changed) {
  TRY(select_best_args(c, d_words, d_cluster_id, d_keep, d_score, n_reads, word_nt, scope, d_keep_out));
  if (n_changed) *n_changed = 0;
  if (n_reads == 0) return HUMID_OK;
  if (word_nt > 32 && ((uintptr_t)d_words & 15)) return fail(c, HUMID_E_INVALID, "wide words must be 16-byte aligned on the device");
  return best_pass(c, d_words, d_cluster_id, d_keep, d_score, n_reads, word_nt, scope, d_keep_out, d_rep_out, n_changed);
}

int humid_select_best(humid_ctx *c, const uint64_t *words, const uint32_t *cluster_id, const uint8_t *keep,
                      const uint32_t *score, uint64_t n_reads, uint32_t word_nt, uint32_t scope, uint8_t *keep_out,
                      uint32_t *rep_out, uint64_t *n_changed) {
  TRY(select_best_args(c, words, cluster_id, keep, score, n_reads, word_nt, scope, keep_out));
  if (n_changed) *n_changed = 0;
  if (n_reads == 0) return HUMID_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads;
  u64 *d_words;
  u32 *d_cid, *d_score, *d_rep_out = nullptr;
  u8 *d_keep, *d_keep_out;
  STAGE_IN(d_words, 0, words, n * (word_nt > 32 ? 16 : 8));
  STAGE_IN(d_cid, 1, cluster_id, n * 4);
  STAGE_IN(d_keep, 2, keep, n);
  STAGE_IN(d_score, 3, score, n * 4);
  STAGE_OUT(d_keep_out, 0, n);
  if (rep_out) STAGE_OUT(d_rep_out, 1, n * 4);
  TRY(best_pass(c, d_words, d_cid, d_keep, d_score, n_reads, word_nt, scope, d_keep_out, d_rep_out, n_changed));
  D2H(keep_out, d_keep_out, n);
  D2H(rep_out, d_rep_out, n * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

// ---- consensus reads per cluster (kernels_consensus.hip.h) -------------------------------------------------------
static int consensus_args(humid_ctx *c, const void *bases, const void *quals, const void *off, const void *cid, const void *keep,
                          uint64_t n_reads, uint32_t min_q, uint32_t cap_q) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  c->cs_valid = c->cs_duplex = false;                        // the last results end with the next call, whatever it returns
  if (min_q > 93) return fail(c, HUMID_E_INVALID, "humid_consensus: min_q must be 0 .. 93");
  if (cap_q < 1 || cap_q > 93) return fail(c, HUMID_E_INVALID, "humid_consensus: cap_q must be 1 .. 93");
  if (n_reads && (!bases || !quals || !off || !cid || !keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  if (n_reads >= 0xffffffffull) return fail(c, HUMID_E_OVERFLOW, "humid_consensus: more than 2^32 - 2 reads");
  return HUMID_OK;
}

int humid_consensus_device(humid_ctx *c, const uint8_t *d_bases, const uint8_t *d_quals, const uint64_t *d_off, uint64_t n_bytes,
                           const uint32_t *d_cluster_id, const uint8_t *d_keep, uint64_t n_reads, uint64_t n_clusters,
                           uint32_t min_q, uint32_t cap_q, humid_consensus_summary *summary) {
  TRY(consensus_args(c, d_bases, d_quals, d_off, d_cluster_id, d_keep, n_reads, min_q, cap_q));
  return consensus_pass(c, d_bases, d_quals, d_off, n_bytes, d_cluster_id, d_keep, n_reads, n_clusters, min_q, cap_q, summary);
}

int humid_consensus(humid_ctx *c, const uint8_t *bases, const uint8_t *quals, const uint64_t *off, uint64_t n_bytes,
                    const uint32_t *cluster_id, const uint8_t *keep, uint64_t n_reads, uint64_t n_clusters, uint32_t min_q,
                    uint32_t cap_q, humid_consensus_summary *summary) {
  TRY(consensus_args(c, bases, quals, off, cluster_id, keep, n_reads, min_q, cap_q));
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads, nb = (size_t)n_bytes;
  u8 *d_bases = nullptr, *d_quals = nullptr, *d_keep = nullptr;
  u64 *d_off = nullptr;
  u32 *d_cid = nullptr;
  if (n) {                                                   // (no reads: every pointer may be null, and the pass reads none)
    STAGE_IN(d_bases, 0, bases, nb);
    STAGE_IN(d_quals, 1, quals, nb);
    STAGE_IN(d_off, 2, off, (n + 1) * 8);
    STAGE_IN(d_cid, 3, cluster_id, n * 4);
    STAGE_IN(d_keep, 4, keep, n);
  }
  return consensus_pass(c, d_bases, d_quals, d_off, n_bytes, d_cid, d_keep, n_reads, n_clusters, min_q, cap_q, summary);
}

int humid_get_consensus(humid_ctx *c, uint64_t cap_bytes, uint64_t *out_off, uint8_t *cons_bases, uint8_t *cons_quals,
                        uint32_t *depth, uint64_t *errors) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->cs_valid) return fail(c, HUMID_E_STATE, "no completed humid_consensus* call in this context");
  const humid_consensus_summary &s = c->cs_sum;
  if ((cons_bases || cons_quals) && cap_bytes < s.total_bytes)
    return fail(c, HUMID_E_INVALID, "humid_get_consensus: room for %llu bytes, the consensus has %llu", (ull)cap_bytes, (ull)s.total_bytes);
  HIPCHK(hipSetDevice(c->device));
  D2H(out_off, c->cs_ooff.p, ((size_t)s.n_clusters + 1) * 8);
  D2H(cons_bases, c->cs_ob.p, (size_t)s.total_bytes);
  D2H(cons_quals, c->cs_oq.p, (size_t)s.total_bytes);
  D2H(depth, c->cs_depth.p, (size_t)s.n_clusters * 4);
  D2H(errors, c->cs_errors.p, (size_t)s.n_clusters * 8);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_consensus_result_device(humid_ctx *c, const uint64_t **d_out_off, const uint8_t **d_bases, const uint8_t **d_quals,
                                  const uint32_t **d_depth, const uint64_t **d_errors) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->cs_valid) return fail(c, HUMID_E_STATE, "no completed humid_consensus* call in this context");
  const bool any = c->cs_sum.n_clusters != 0;
  if (d_out_off) *d_out_off = c->cs_ooff.as<u64>();
  if (d_bases) *d_bases = any ? c->cs_ob.as<u8>() : nullptr;
  if (d_quals) *d_quals = any ? c->cs_oq.as<u8>() : nullptr;
  if (d_depth) *d_depth = any ? c->cs_depth.as<u32>() : nullptr;
  if (d_errors) *d_errors = any ? c->cs_errors.as<u64>() : nullptr;
  return HUMID_OK;
}

// ---- duplex consensus reads per cluster (kernels_dconsensus.hip.h) ------------------------------------------------
static int duplex_consensus_args(humid_ctx *c, const void *bases_s, const void *quals_s, const void *off_s, const void *bases_o,
                                 const void *quals_o, const void *off_o, const void *cid, const void *keep, const void *strand,
                                 uint64_t n_reads, uint32_t min_q, uint32_t strand_cap_q, uint32_t cap_q) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  c->cs_valid = c->cs_duplex = false;                        // the last results end with the next call, whatever it returns
  if (min_q > 93) return fail(c, HUMID_E_INVALID, "humid_duplex_consensus: min_q must be 0 .. 93");
  if (strand_cap_q < 1 || strand_cap_q > 93) return fail(c, HUMID_E_INVALID, "humid_duplex_consensus: strand_cap_q must be 1 .. 93");
  if (cap_q < 1 || cap_q > 93) return fail(c, HUMID_E_INVALID, "humid_duplex_consensus: cap_q must be 1 .. 93");
  if (n_reads && (!bases_s || !quals_s || !off_s || !bases_o || !quals_o || !off_o || !cid || !keep || !strand))
    return fail(c, HUMID_E_INVALID, "null buffer");
  if (n_reads >= 0xffffffffull) return fail(c, HUMID_E_OVERFLOW, "humid_duplex_consensus: more than 2^32 - 2 reads");
  return HUMID_OK;
}

int humid_duplex_consensus_device(humid_ctx *c, const uint8_t *d_bases_s, const uint8_t *d_quals_s, const uint64_t *d_off_s,
                                  uint64_t n_bytes_s, const uint8_t *d_bases_o, const uint8_t *d_quals_o, const uint64_t *d_off_o,
                                  uint64_t n_bytes_o, const uint32_t *d_cluster_id, const uint8_t *d_keep, const uint8_t *d_strand,
                                  uint64_t n_reads, uint64_t n_clusters, uint32_t min_q, uint32_t strand_cap_q, uint32_t cap_q,
                                  humid_duplex_summary *summary) {
  TRY(duplex_consensus_args(c, d_bases_s, d_quals_s, d_off_s, d_bases_o, d_quals_o, d_off_o, d_cluster_id, d_keep, d_strand, n_reads, min_q,
                            strand_cap_q, cap_q));
  return duplex_consensus_pass(c, d_bases_s, d_quals_s, d_off_s, n_bytes_s, d_bases_o, d_quals_o, d_off_o, n_bytes_o, d_cluster_id, d_keep,
                               d_strand, n_reads, n_clusters, min_q, strand_cap_q, cap_q, summary);
}

int humid_duplex_consensus(humid_ctx *c, const uint8_t *bases_s, const uint8_t *quals_s, const uint64_t *off_s, uint64_t n_bytes_s,
                           const uint8_t *bases_o, const uint8_t *quals_o, const uint64_t *off_o, uint64_t n_bytes_o,
                           const uint32_t *cluster_id, const uint8_t *keep, const uint8_t *strand, uint64_t n_reads, uint64_t n_clusters,
                           uint32_t min_q, uint32_t strand_cap_q, uint32_t cap_q, humid_duplex_summary *summary) {
  TRY(duplex_consensus_args(c, bases_s, quals_s, off_s, bases_o, quals_o, off_o, cluster_id, keep, strand, n_reads, min_q, strand_cap_q,
                            cap_q));
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads, nbs = (size_t)n_bytes_s, nbo = (size_t)n_bytes_o;
  u8 *d_bs = nullptr, *d_qs = nullptr, *d_bo = nullptr, *d_qo = nullptr, *d_keep = nullptr, *d_strand = nullptr;
  u64 *d_os = nullptr, *d_oo = nullptr;
  u32 *d_cid = nullptr;
  if (n) {                                                   // (no reads: every pointer may be null, and the pass reads none)
    STAGE_IN(d_bs, 0, bases_s, nbs);
    STAGE_IN(d_qs, 1, quals_s, nbs);
    STAGE_IN(d_os, 2, off_s, (n + 1) * 8);
    STAGE_IN(d_cid, 3, cluster_id, n * 4);
    STAGE_IN(d_keep, 4, keep, n);
    STAGE_IN(d_bo, 5, bases_o, nbo);
    STAGE_IN(d_qo, 6, quals_o, nbo);
    STAGE_IN(d_oo, 7, off_o, (n + 1) * 8);
    STAGE_IN(d_strand, 8, strand, n);
  }
  return duplex_consensus_pass(c, d_bs, d_qs, d_os, n_bytes_s, d_bo, d_qo, d_oo, n_bytes_o, d_cid, d_keep, d_strand, n_reads, n_clusters,
                               min_q, strand_cap_q, cap_q, summary);
}

int humid_get_duplex_consensus(humid_ctx *c, uint32_t *depth_same, uint32_t *depth_other, uint32_t *disagree,
                               humid_duplex_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->cs_valid || !c->cs_duplex)
    return fail(c, HUMID_E_STATE, "the last successful consensus call in this context was no humid_duplex_consensus* call");
  const size_t C = (size_t)c->ds_sum.n_clusters;
  HIPCHK(hipSetDevice(c->device));
  D2H(depth_same, c->ds_same.p, C * 4);
  D2H(depth_other, c->ds_other.p, C * 4);
  D2H(disagree, c->ds_disagree.p, C * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (summary) *summary = c->ds_sum;
  return HUMID_OK;
}

// ---- optical duplicates per cluster (kernels_optical.hip.h) -------------------------------------------------------
// what both entry points refuse before anything moves
static int optical_args(humid_ctx *c, const void *cid, const void *keep, const void *tile, const void *x, const void *y,
                        uint64_t n_reads, const void *optical_out, humid_optical_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (summary) memset(summary, 0, sizeof *summary);
  if (n_reads && (!cid || !keep || !tile || !x || !y || !optical_out)) return fail(c, HUMID_E_INVALID, "null buffer");
  if (n_reads > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "humid_optical_duplicates: more than 2^31 - 1 reads");
  return HUMID_OK;
}

int humid_optical_duplicates_device(humid_ctx *c, const uint32_t *d_cluster_id, const uint8_t *d_keep, const uint32_t *d_tile,
                                    const uint32_t *d_x, const uint32_t *d_y, uint64_t n_reads, uint64_t n_clusters,
                                    uint32_t distance, uint8_t *d_optical_out, uint32_t *d_origin_out,
                                    uint32_t *d_per_cluster_out, humid_optical_summary *summary) {
  TRY(optical_args(c, d_cluster_id, d_keep, d_tile, d_x, d_y, n_reads, d_optical_out, summary));
  if (n_reads == 0) return HUMID_OK;
  return optical_pass(c, d_cluster_id, d_keep, d_tile, d_x, d_y, n_reads, n_clusters, distance, d_optical_out, d_origin_out,
                      d_per_cluster_out, summary);
}

int humid_optical_duplicates(humid_ctx *c, const uint32_t *cluster_id, const uint8_t *keep, const uint32_t *tile, const uint32_t *x,
                             const uint32_t *y, uint64_t n_reads, uint64_t n_clusters, uint32_t distance, uint8_t *optical_out,
                             uint32_t *origin_out, uint32_t *per_cluster_out, humid_optical_summary *summary) {
  TRY(optical_args(c, cluster_id, keep, tile, x, y, n_reads, optical_out, summary));
  if (n_reads == 0) return HUMID_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads, nc = n_clusters <= n_reads ? (size_t)n_clusters : 0;   // (more clusters than reads: refused by the pass)
  u32 *d_cid, *d_tile, *d_x, *d_y, *d_origin = nullptr, *d_pc = nullptr;
  u8 *d_keep, *d_optical;
  STAGE_IN(d_cid, 0, cluster_id, n * 4);
  STAGE_IN(d_keep, 1, keep, n);
  STAGE_IN(d_tile, 2, tile, n * 4);
  STAGE_IN(d_x, 3, x, n * 4);
  STAGE_IN(d_y, 4, y, n * 4);
  STAGE_OUT(d_optical, 0, n);
  if (origin_out) STAGE_OUT(d_origin, 1, n * 4);
  if (per_cluster_out && nc) STAGE_OUT(d_pc, 2, nc * 4);
  TRY(optical_pass(c, d_cid, d_keep, d_tile, d_x, d_y, n_reads, n_clusters, distance, d_optical, d_origin, d_pc, summary));
  D2H(optical_out, d_optical, n);
  D2H(origin_out, d_origin, n * 4);
  D2H(per_cluster_out, d_pc, nc * 4);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_cluster_graph(humid_ctx *c, const uint32_t *count, const uint32_t *nbr_off,
                        const uint32_t *nbr_idx, uint32_t n_leaves, uint32_t method,
                        uint32_t *leaf_cluster, uint64_t *cl_size, uint32_t *cl_max_count,
                        uint32_t *cl_max_leaf, uint32_t *n_clusters) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  state_reset(c);
  if (method > 1) return fail(c, HUMID_E_INVALID, "method must be 0 or 1");
  if (n_clusters) *n_clusters = 0;
  const u32 U = n_leaves;
  if (U == 0) return HUMID_OK;
  if (!count || !nbr_off) return fail(c, HUMID_E_INVALID, "null buffer");
  const u32 twoE = nbr_off[U];
  if (twoE && !nbr_idx) return fail(c, HUMID_E_INVALID, "null nbr_idx");
  for (u32 u = 0; u < U; u++)
    if (nbr_off[u] > nbr_off[u + 1]) return fail(c, HUMID_E_INVALID, "nbr_off not monotone at %u", u);
  for (u32 k = 0; k < twoE; k++)
    if (nbr_idx[k] >= U) return fail(c, HUMID_E_INVALID, "nbr_idx[%u] = %u out of range", k, nbr_idx[k]);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  c->cg_valid = false;
  ENSURE(c->s_cnt, (size_t)U * 4);
  c->g_cnt = c->s_cnt.as<u32>();
  c->gU = U;
  ENSURE(c->deg, (size_t)U * 4);
  ENSURE(c->nbr_off, (size_t)(U + 1) * 4);
  ENSURE(c->nbr_idx, (size_t)(twoE + 1) * 4);
  ENSURE(c->parent, (size_t)U * 4);
  std::vector<u32> hdeg(U);
  for (u32 u = 0; u < U; u++) hdeg[u] = nbr_off[u + 1] - nbr_off[u];
  {
    // NLeaf::neighbours is always symmetric (src/humid.cc:121-122, tests' link()); the component
    // walk relies on it.  Two linked leaves of count 0 make maxNeighbour_ (cluster.cc:39-51)
    // ping-pong forever in the reference: refuse instead of hanging the GPU.
    std::vector<u64> fwd, rev;
    fwd.reserve(twoE); rev.reserve(twoE);
    for (u32 u = 0; u < U; u++)
      for (u32 k = nbr_off[u]; k < nbr_off[u + 1]; k++) {
        const u32 v = nbr_idx[k];
        if (count[u] == 0 && count[v] == 0)
          return fail(c, HUMID_E_INVALID, "leaves %u and %u are linked and both have count 0", u, v);
        fwd.push_back(((u64)u << 32) | v);
        rev.push_back(((u64)v << 32) | u);
      }
    std::sort(fwd.begin(), fwd.end());
    std::sort(rev.begin(), rev.end());
    if (fwd != rev) return fail(c, HUMID_E_INVALID, "neighbour lists are not symmetric");
  }
  HIPCHK(hipMemcpyAsync(c->s_cnt.p, count, (size_t)U * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->deg.p, hdeg.data(), (size_t)U * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->nbr_off.p, nbr_off, (size_t)(U + 1) * 4, hipMemcpyHostToDevice, st));
  if (twoE) HIPCHK(hipMemcpyAsync(c->nbr_idx.p, nbr_idx, (size_t)twoE * 4, hipMemcpyHostToDevice, st));
  ENSURE(c->csize, (size_t)U * 4);
  ENSURE(c->small_roots, ((size_t)U / 3 + 2) * 4);
  HIPCHK(hipMemsetAsync(c->csize.p, 0, (size_t)U * 4, st));
  HIPCHK(hipMemsetAsync(&c->d_ctr[CTR_EDGES], 0, 3 * sizeof(ull), st));
  HIPCHK(hipMemsetAsync(&c->d_ctr[CTR_SMALLROOTS], 0, sizeof(ull), st));
  hipLaunchKernelGGL(k_iota, dim3(blocks_for(U)), dim3(256), 0, st, c->parent.as<u32>(), U);
  hipLaunchKernelGGL(k_union_csr, dim3(blocks_for(U)), dim3(256), 0, st, c->nbr_off.as<u32>(),
                     c->nbr_idx.as<u32>(), U, c->parent.as<u32>(),
                     method == HUMID_METHOD_MAXIMUM ? (const u32 *)nullptr : c->s_cnt.as<u32>());
  hipLaunchKernelGGL(k_comp_stats, dim3(blocks_for(U)), dim3(256), 0, st, c->deg.as<u32>(),
                     c->parent.as<u32>(), U, c->csize.as<u32>());
  hipLaunchKernelGGL(k_comp_count, dim3(512), dim3(256), 0, st, c->deg.as<u32>(), c->parent.as<u32>(),
                     c->csize.as<u32>(), U, c->d_ctr, c->small_roots.as<u32>());
  HIPCHK(hipGetLastError());
  TRY(read_counters(c));   // also drains the stream: hdeg is a host temporary
  TRY(cluster_stage(c, c->s_cnt.as<u32>(), U, c->h_ctr[CTR_NONSINGLE], c->h_ctr[CTR_MEMBERS], method));
  hipLaunchKernelGGL(k_finalize_nodes, dim3(blocks_for(U)), dim3(256), 0, st, c->cl_of.as<u32>(),
                     c->pos.as<u32>(), c->maxleaf.as<u32>(), U, c->cid.as<u32>(), c->ismax.as<u8>(),
                     (const u32 *)nullptr, (const u32 *)nullptr, (u64 *)nullptr);
  HIPCHK(hipGetLastError());
  u64 C = 0;
  TRY(n_clusters_from_scan(c, U, &C));
  D2H(leaf_cluster, c->cid.p, (size_t)U * 4);
  HIPCHK(hipStreamSynchronize(st));
  if (n_clusters) *n_clusters = (u32)C;
  TRY(export_clusters(c, U, C, cl_size, cl_max_count, cl_max_leaf));
  return state_publish(c, CtxState::HAND_GRAPH);
}

// ---- accumulated runs: a read set fed in chunks (pipeline.hip.h, kernels_accum.hip.h) -------------------------
// the record of a finish points at the accumulator's arrays: it ends with them
// (free_memory false: humid_accum_begin keeps the blocks for the next accumulator, humid_accum_clear returns them)
static void accum_release(humid_ctx *c, bool free_memory) {
  if (state_has_leaves(c) && c->gU && (c->g_word == c->ac_word[c->ac_cur].p || c->g_word == c->ac_iword.p)) state_reset(c);
  if (free_memory) {
    for (int k = 0; k < 2; k++) { c->ac_word[k].release(); c->ac_cnt[k].release(); c->ac_first[k].release(); }
    c->ac_cid.release(); c->ac_ismax.release(); c->ac_lcid.release(); c->ac_lismax.release();
    c->ac_split.release(); c->ac_tcnt.release(); c->ac_toff.release(); c->ac_flag.release();
    c->ac_head.release(); c->ac_hpos.release(); c->ac_keys.release(); c->ac_iword.release();
  }
  c->ac_on = c->ac_finished = c->ac_keyed = false;
  c->ac_nt = c->ac_cur = c->ac_key_nt = c->ac_ent_nt = 0;
  c->ac_U = c->ac_chunks = c->ac_total = c->ac_usable = c->ac_G = 0;
}

int humid_accum_begin(humid_ctx *c, uint32_t word_nt) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  TRY(check_run_args(c, 0, word_nt, 0, 64));
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  accum_release(c, false);
  c->ac_on = true;
  c->ac_nt = word_nt;
  return HUMID_OK;
}

int humid_accum_begin_keyed(humid_ctx *c, uint32_t word_nt, uint32_t key_nt) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  TRY(check_run_args(c, 0, word_nt, 0, 32));
  if (key_nt > 32) return fail(c, HUMID_E_INVALID, "key_nt must be 0 (any 64-bit key) or 1 .. 32");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  accum_release(c, false);
  c->ac_on = c->ac_keyed = true;
  c->ac_nt = word_nt;
  c->ac_key_nt = key_nt;
  // one uint64 `key << 2 * word_nt | word` while it holds both; else {key, word}, a word of 32 + key_nt nucleotides
  c->ac_ent_nt = (key_nt && key_nt + word_nt <= 32) ? key_nt + word_nt : 32 + (key_nt ? key_nt : 32);
  return HUMID_OK;
}

int humid_accum_clear(humid_ctx *c) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  accum_release(c, true);
  return HUMID_OK;
}

#define ACCUM_NEED(keyed)                                                                                        \
  do {                                                                                                           \
    if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");                                                \
    if (!c->ac_on) return fail(c, HUMID_E_STATE, "no accumulator in this context (humid_accum_begin)");          \
    if (c->ac_keyed != (keyed))                                                                                  \
      return fail(c, HUMID_E_STATE, (keyed) ? "the accumulator of this context is a plain one (humid_accum_begin_keyed)" \
                                            : "the accumulator of this context is a keyed one: use the humid_accum_*_keyed calls"); \
  } while (0)

// what add and map refuse before anything moves (key: of the keyed calls)
static int accum_chunk_args(humid_ctx *c, bool keyed, const void *words, const void *key, const void *filtered, uint64_t n_reads,
                            bool device) {
  ACCUM_NEED(keyed);
  if (n_reads > 0x7fffffffull) return fail(c, HUMID_E_OVERFLOW, "a chunk of %llu reads exceeds 2^31-1", (ull)n_reads);
  if (n_reads && (!words || !filtered || (keyed && !key))) return fail(c, HUMID_E_INVALID, "null buffer");
  if (device && c->ac_nt > 32 && ((uintptr_t)words & 15)) return fail(c, HUMID_E_INVALID, "wide words must be 16-byte aligned on the device");
  return HUMID_OK;
}

// add and map over device arrays, arguments checked (d_key: null for a plain accumulator)
static int accum_add_device(humid_ctx *c, const u64 *d_words, const u64 *d_key, const u8 *d_filt, u64 n_reads, u64 base_index) {
  state_reset(c);
  HIPCHK(hipSetDevice(c->device));
  TRY(accum_counted(c, d_words, d_key, d_filt, n_reads, [&](auto *w) {
    if (c->U) TRY(accum_merge<std::remove_cv_t<std::remove_pointer_t<decltype(w)>>>(c, base_index));
    return (int)HUMID_OK;
  }));
  HIPCHK(hipStreamSynchronize(c->stream));                     // (the caller's arrays are free again)
  c->ac_chunks++;
  c->ac_total += n_reads;
  c->ac_usable += c->usable;
  c->ac_finished = false;
  return state_publish_count(c, false);
}

static int accum_map_device(humid_ctx *c, const u64 *d_words, const u64 *d_key, const u8 *d_filt, u64 n_reads, u64 base_index,
                            u32 *d_cluster_id, u8 *d_keep, u64 *n_unknown) {
  if (!c->ac_finished) return fail(c, HUMID_E_STATE, "no humid_accum_finish since the last humid_accum_add");
  if (n_reads && (!d_cluster_id || !d_keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  state_reset(c);                                              // (the record finish published ends here: the chunk is counted in the context's buffers)
  HIPCHK(hipSetDevice(c->device));
  u64 unknown = 0;
  TRY(accum_counted(c, d_words, d_key, d_filt, n_reads, [&](auto *w) {
    return accum_map<std::remove_cv_t<std::remove_pointer_t<decltype(w)>>>(c, base_index, d_cluster_id, d_keep, &unknown);
  }));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (n_unknown) *n_unknown = unknown;
  return state_publish_count(c, false);
}

// the host forms: the chunk staged (key: null for a plain accumulator), the device form, the results copied back
static int accum_stage_chunk(humid_ctx *c, const u64 *words, const u64 *key, const u8 *filtered, size_t n) {
  const size_t wbytes = c->ac_nt > 32 ? 16 : 8;
  ENSURE(c->in_words, n * wbytes + 16);
  ENSURE(c->in_filt, n + 8);
  if (key) ENSURE(c->kr_key_in, n * 8 + 16);
  if (n) {
    HIPCHK(hipMemcpyAsync(c->in_words.p, words, n * wbytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->in_filt.p, filtered, n, hipMemcpyHostToDevice, c->stream));
    if (key) HIPCHK(hipMemcpyAsync(c->kr_key_in.p, key, n * 8, hipMemcpyHostToDevice, c->stream));
  }
  return HUMID_OK;
}

static int accum_add_host(humid_ctx *c, const u64 *words, const u64 *key, const u8 *filtered, u64 n_reads, u64 base_index) {
  HIPCHK(hipSetDevice(c->device));
  TRY(accum_stage_chunk(c, words, key, filtered, (size_t)n_reads));
  return accum_add_device(c, c->in_words.as<u64>(), key ? c->kr_key_in.as<u64>() : nullptr, c->in_filt.as<u8>(), n_reads, base_index);
}

static int accum_map_host(humid_ctx *c, const u64 *words, const u64 *key, const u8 *filtered, u64 n_reads, u64 base_index,
                          uint32_t *cluster_id, uint8_t *keep, uint64_t *n_unknown) {
  if (!c->ac_finished) return fail(c, HUMID_E_STATE, "no humid_accum_finish since the last humid_accum_add");
  if (n_reads && (!cluster_id || !keep)) return fail(c, HUMID_E_INVALID, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = (size_t)n_reads;
  TRY(accum_stage_chunk(c, words, key, filtered, n));
  ENSURE(c->out_cid, n * 4 + 8);
  ENSURE(c->out_keep, n + 8);
  TRY(accum_map_device(c, c->in_words.as<u64>(), key ? c->kr_key_in.as<u64>() : nullptr, c->in_filt.as<u8>(), n_reads, base_index,
                       c->out_cid.as<u32>(), c->out_keep.as<u8>(), n_unknown));
  D2H(cluster_id, c->out_cid.p, n * 4);
  D2H(keep, c->out_keep.p, n);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_accum_add_device(humid_ctx *c, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads, uint64_t base_index) {
  TRY(accum_chunk_args(c, false, d_words, nullptr, d_filtered, n_reads, true));
  return accum_add_device(c, d_words, nullptr, d_filtered, n_reads, base_index);
}

int humid_accum_add(humid_ctx *c, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads, uint64_t base_index) {
  TRY(accum_chunk_args(c, false, words, nullptr, filtered, n_reads, false));
  return accum_add_host(c, words, nullptr, filtered, n_reads, base_index);
}

int humid_accum_add_keyed_device(humid_ctx *c, const uint64_t *d_words, const uint64_t *d_key, const uint8_t *d_filtered,
                                 uint64_t n_reads, uint64_t base_index) {
  TRY(accum_chunk_args(c, true, d_words, d_key, d_filtered, n_reads, true));
  return accum_add_device(c, d_words, d_key, d_filtered, n_reads, base_index);
}

int humid_accum_add_keyed(humid_ctx *c, const uint64_t *words, const uint64_t *key, const uint8_t *filtered, uint64_t n_reads,
                          uint64_t base_index) {
  TRY(accum_chunk_args(c, true, words, key, filtered, n_reads, false));
  return accum_add_host(c, words, key, filtered, n_reads, base_index);
}

int humid_accum_finish(humid_ctx *c, uint32_t distance, uint32_t method, humid_summary *summary) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->ac_on) return fail(c, HUMID_E_STATE, "no accumulator in this context (humid_accum_begin)");
  TRY(check_run_args(c, c->ac_U, c->ac_nt, method, 64));
  state_reset(c);
  HIPCHK(hipSetDevice(c->device));
  humid_summary s;
  memset(&s, 0, sizeof s);
  s.total = c->ac_total;
  s.usable = c->ac_usable;
  s.unique = c->ac_U;
  c->ac_finished = false;
  c->word_nt = c->ac_nt; c->distance = distance; c->method = method;
  c->gU = 0; c->E = c->M = c->C = 0;
  c->cg_valid = false;                                         // (an empty list runs no graph stage: nothing of an earlier run's is left to expand)
  if (c->ac_keyed) {
    c->ac_G = 0;
    c->kr_n = 0;
    c->gk_word_nt = c->ac_nt; c->gk_leaf_nt = 0; c->gk_groups = 1;
    c->usable = c->ac_usable;                                  // (what the group statistics close the last group with)
    if (c->ac_U)
      TRY(with_word_type(c->ac_ent_nt, [&](auto *w) {
        return accum_finish_keyed_any<std::remove_cv_t<std::remove_pointer_t<decltype(w)>>>(c, distance, method, s);
      }));
  } else
    TRY(with_word_type(c->ac_nt, [&](auto *w) {
      return accum_finish<std::remove_cv_t<std::remove_pointer_t<decltype(w)>>>(c, distance, method, s);
    }));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->ac_finished = true;
  if (summary) *summary = s;
  return c->ac_keyed ? state_publish_keyed_graph(c) : state_publish(c, CtxState::STAGE_GRAPH);
}

int humid_accum_map_device(humid_ctx *c, const uint64_t *d_words, const uint8_t *d_filtered, uint64_t n_reads, uint64_t base_index,
                           uint32_t *d_cluster_id, uint8_t *d_keep, uint64_t *n_unknown) {
  TRY(accum_chunk_args(c, false, d_words, nullptr, d_filtered, n_reads, true));
  return accum_map_device(c, d_words, nullptr, d_filtered, n_reads, base_index, d_cluster_id, d_keep, n_unknown);
}

int humid_accum_map(humid_ctx *c, const uint64_t *words, const uint8_t *filtered, uint64_t n_reads, uint64_t base_index,
                    uint32_t *cluster_id, uint8_t *keep, uint64_t *n_unknown) {
  TRY(accum_chunk_args(c, false, words, nullptr, filtered, n_reads, false));
  return accum_map_host(c, words, nullptr, filtered, n_reads, base_index, cluster_id, keep, n_unknown);
}

int humid_accum_map_keyed_device(humid_ctx *c, const uint64_t *d_words, const uint64_t *d_key, const uint8_t *d_filtered,
                                 uint64_t n_reads, uint64_t base_index, uint32_t *d_cluster_id, uint8_t *d_keep, uint64_t *n_unknown) {
  TRY(accum_chunk_args(c, true, d_words, d_key, d_filtered, n_reads, true));
  return accum_map_device(c, d_words, d_key, d_filtered, n_reads, base_index, d_cluster_id, d_keep, n_unknown);
}

int humid_accum_map_keyed(humid_ctx *c, const uint64_t *words, const uint64_t *key, const uint8_t *filtered, uint64_t n_reads,
                          uint64_t base_index, uint32_t *cluster_id, uint8_t *keep, uint64_t *n_unknown) {
  TRY(accum_chunk_args(c, true, words, key, filtered, n_reads, false));
  return accum_map_host(c, words, key, filtered, n_reads, base_index, cluster_id, keep, n_unknown);
}

int humid_accum_get_leaves(humid_ctx *c, uint64_t *word, uint32_t *count, uint64_t *first_index, uint64_t cap, uint64_t *n_out) {
  ACCUM_NEED(false);
  HIPCHK(hipSetDevice(c->device));
  if (n_out) *n_out = c->ac_U;
  const size_t n = (size_t)std::min<u64>(cap, c->ac_U), wbytes = c->ac_nt > 32 ? 16 : 8;
  const u32 cur = c->ac_cur;
  D2H(word, c->ac_word[cur].p, n * wbytes);
  D2H(count, c->ac_cnt[cur].p, n * 4);
  D2H(first_index, c->ac_first[cur].p, n * 8);
  HIPCHK(hipStreamSynchronize(c->stream));
  return HUMID_OK;
}

int humid_accum_get_leaves_keyed(humid_ctx *c, uint64_t *key, uint64_t *word, uint32_t *count, uint64_t *first_index, uint64_t cap,
                                 uint64_t *n_out) {
  ACCUM_NEED(true);
  HIPCHK(hipSetDevice(c->device));
  if (n_out) *n_out = c->ac_U;
  const size_t n = (size_t)std::min<u64>(cap, c->ac_U), epr = c->ac_ent_nt > 32 ? 2 : 1;
  const u32 cur = c->ac_cur, wb = 2 * c->ac_nt;
  std::vector<u64> ent((key || word) ? n * epr : 0);
  D2H(ent.data(), c->ac_word[cur].p, ent.size() * 8);
  D2H(count, c->ac_cnt[cur].p, n * 4);
  D2H(first_index, c->ac_first[cur].p, n * 8);
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n && !ent.empty(); i++) {             // (a one-word entry: wb <= 62)
    if (key) key[i] = epr == 2 ? ent[2 * i] : ent[i] >> wb;
    if (word) word[i] = epr == 2 ? ent[2 * i + 1] : ent[i] & ((1ull << wb) - 1ull);
  }
  return HUMID_OK;
}

int humid_accum_keyed_info(humid_ctx *c, uint32_t *key_nt, uint32_t *entry_words, uint64_t *n_keys) {
  ACCUM_NEED(true);
  if (key_nt) *key_nt = c->ac_key_nt;
  if (entry_words) *entry_words = c->ac_ent_nt > 32 ? 2u : 1u;
  if (n_keys) *n_keys = c->ac_finished ? c->ac_G : 0;
  return HUMID_OK;
}

int humid_accum_info(humid_ctx *c, uint32_t *word_nt, uint64_t *chunks, uint64_t *total, uint64_t *usable, uint64_t *unique,
                     uint32_t *finished) {
  if (!c) return fail(nullptr, HUMID_E_INVALID, "ctx is null");
  if (!c->ac_on) return fail(c, HUMID_E_STATE, "no accumulator in this context (humid_accum_begin)");
  if (word_nt) *word_nt = c->ac_nt;
  if (chunks) *chunks = c->ac_chunks;
  if (total) *total = c->ac_total;
  if (usable) *usable = c->ac_usable;
  if (unique) *unique = c->ac_U;
  if (finished) *finished = c->ac_finished ? 1u : 0u;
  return HUMID_OK;
}

}  // extern "C"
