// The timing of a pass: who records which event, and what the summary makes of them.
// Included by pipeline.hip.h behind the context (which holds the slots' events and the two records, PassTiming and
// TimingLeft, defined in front of it) and in front of the stages.  The table of the slots: DESIGN.md, "The events of a pass".
#pragma once

// every event record of the library's passes goes through here: counted for humid_stamp_info
#define EVREC(ev, st) do { c->timing_left.event_records++; HIPCHK(hipEventRecord((ev), (st))); } while (0)

enum PairPhase : u32 { PAIRS_FILL = KEV_PAIRS_FILL, PAIRS_COUNT = KEV_PAIRS_COUNT };
// the slot of combination combo < KEV_PAIR_COMBOS in a phase of the neighbour search; end: 0 in front of it, 1 behind
static inline KernelEvent kev_pairs(PairPhase phase, u32 combo, u32 end) { return (KernelEvent)(phase + 2 * combo + end); }

// ---- the three marks: each holds its condition once ------------------------------------------------------------
// the kernel marks are on: the option, unless cg_build_full runs
static inline bool kernel_marks_on(const humid_ctx *c) { return c->kev_on && !c->timing.kernels_quiet; }
// a stage mark: recorded unless the pass is lean (outside run_device / run_device_long no pass is: always)
static int mark_stage(humid_ctx *c, hipEvent_t e) {
  if (!c->timing.lean) EVREC(e, c->stream);
  return HUMID_OK;
}
// a kernel mark: recorded with the option kernel_timing
static int mark_kernel(humid_ctx *c, hipEvent_t e) {
  if (kernel_marks_on(c)) EVREC(e, c->stream);
  return HUMID_OK;
}
// a frame mark -- pass start, the count kernel's pair, pass end: recorded unless device stamps time the pass
static int mark_frame(humid_ctx *c, hipEvent_t e) {
  if (!c->timing.stamp_timed) EVREC(e, c->stream);
  return HUMID_OK;
}
// the kernel mark of a combination of the neighbour search (those beyond KEV_PAIR_COMBOS have none)
static int mark_pairs(humid_ctx *c, PairPhase phase, u32 combo, u32 end) {
  return combo < KEV_PAIR_COMBOS ? mark_kernel(c, c->kev[kev_pairs(phase, combo, end)]) : HUMID_OK;
}

// Opens the timing of a pass and restores the between-calls state on every way out.  The stages' own events only with
// the per-kernel timing (ms_count .. ms_map are 0 without it; ms_total and the count kernel's time are always measured:
// by device stamps where the pass takes the record road, by events elsewhere).  offer_stamps, decided once, before the
// first launch: stage_count_rec takes the offer up (no other count road does) and withdraws it when its count is
// discarded; the graph stage and the pass's end are the same on every road.
struct PassTimingGuard {
  PassTiming &t;
  PassTimingGuard(humid_ctx *c, bool offer_stamps) : t(c->timing) {
    t.lean = !c->kev_on && getenv("HUMID_ALL_EVENTS") == nullptr;
    t.stamp_live = t.stamp_timed = false;
    t.stamp_ok = offer_stamps;
  }
  ~PassTimingGuard() { t.lean = t.stamp_ok = t.stamp_live = t.stamp_timed = false; }
  PassTimingGuard(const PassTimingGuard &) = delete;
};

// the context's per-pass fields in front of a count; distance / method stay as they are (the stage calls set them with
// the graph stage)
static inline void pass_begin(humid_ctx *c, u64 n_reads, u32 word_nt) {
  c->timing.unperm_tiled = false;
  c->N = n_reads; c->U = c->E = c->M = c->C = c->usable = 0;
  c->word_nt = word_nt;
  c->gU = 0;
}
static inline void pass_begin(humid_ctx *c, u64 n_reads, u32 word_nt, u32 distance, u32 method) {
  pass_begin(c, n_reads, word_nt);
  c->distance = distance; c->method = method;
}

static int gkey_check(humid_ctx *c);
// The end of a pass: waits for its last event (or has the stamps already) and turns events and stamps into the
// summary's times.  per_kernel = false (the long-word run): none of the kernel marks beyond the count kernel's pair is
// read, ms_k_map = ms_map.
static int timing_tail(humid_ctx *c, humid_summary &s, u32 n_pair_segs, bool per_kernel = true) {
  const PassTiming &t = c->timing;
  TimingLeft &left = c->timing_left;
  // (the last host wait watches a mapped flag, not the stream: the runtime may not have seen the last
  // event's signal yet -- "device not ready" from hipEventElapsedTime once in ~10^3 runs)
  const bool timed = t.stamp_timed;
  // the last host wait delivered the stamps with the counters.  (Not so in the one pass of a context whose first wait
  // finds the mapped stores invisible, no_poll: no publishing kernel ran at its end.  That pass reports no times; the
  // passes behind it record their events.)
  const bool delivered = t.stamp_live && !c->no_poll;
  if (delivered) {
    for (u32 k = 0; k < STAMP_N; k++) left.stamps[k] = c->h_ctr[STAMP_AT + k];
    left.stamp_live = true;
    left.stamp_timed = timed;
  }
  if (!timed) HIPCHK(hipEventSynchronize(c->ev[EV_PASS_END]));
  if (!t.lean) {                                             // the stages' shares: option kernel_timing
    HIPCHK(hipEventElapsedTime(&s.ms_count, c->ev[EV_PASS_START], c->ev[EV_COUNT_END]));
    HIPCHK(hipEventElapsedTime(&s.ms_neighbours, c->ev[EV_COUNT_END], c->ev[EV_GRAPH_BUILT]));
    HIPCHK(hipEventElapsedTime(&s.ms_cluster, c->ev[EV_GRAPH_BUILT], c->ev[EV_CLUSTERS_DONE]));
    HIPCHK(hipEventElapsedTime(&s.ms_map, c->ev[EV_CLUSTERS_DONE], c->ev[EV_PASS_END]));
  }
  if (timed && delivered) {                                  // ticks of 10 ns
    s.ms_total = (float)((double)(left.stamps[STAMP_END] - left.stamps[STAMP_START]) / 1e5);
    s.ms_k_insert = (float)((double)(left.stamps[STAMP_K1] - left.stamps[STAMP_K0]) / 1e5);
  } else if (!timed) HIPCHK(hipEventElapsedTime(&s.ms_total, c->ev[EV_PASS_START], c->ev[EV_PASS_END]));
  TRY(gkey_check(c));
  if (!timed) HIPCHK(hipEventElapsedTime(&s.ms_k_insert, c->kev[KEV_INSERT_BEGIN], c->kev[KEV_INSERT_END]));
  const bool kernels = per_kernel && c->kev_on;
  if (kernels && count_in_partition_order(c))                // the first map kernel alone
    HIPCHK(hipEventElapsedTime(&s.ms_k_map, c->ev[EV_CLUSTERS_DONE], c->kev[KEV_MAP_MID]));
  else s.ms_k_map = s.ms_map;                                // (with the option: the two stage events bracket exactly the k_read_map launch)
  if (!kernels) return HUMID_OK;
  if (count_in_partition_order(c) && t.unperm_tiled) HIPCHK(hipEventElapsedTime(&s.ms_k_unperm, c->kev[KEV_MAP_MID], c->kev[KEV_UNPERM_END]));
  if (count_part_timed(c)) HIPCHK(hipEventElapsedTime(&s.ms_k_part, c->kev[KEV_PART_BEGIN], c->kev[KEV_PART_END]));
  HIPCHK(hipEventElapsedTime(&s.ms_k_cluster, c->kev[KEV_CLUSTER_BEGIN], c->kev[KEV_CLUSTER_END]));
  for (u32 g = 0; g < n_pair_segs; g++) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->kev[kev_pairs(PAIRS_COUNT, g, 0)], c->kev[kev_pairs(PAIRS_COUNT, g, 1)]));
    s.ms_k_pairs += ms;
    if (c->E > 0 && !c->cg_valid) {
      HIPCHK(hipEventElapsedTime(&ms, c->kev[kev_pairs(PAIRS_FILL, g, 0)], c->kev[kev_pairs(PAIRS_FILL, g, 1)]));
      s.ms_k_pairs += ms;
    }
  }
  return HUMID_OK;
}
