"""ctypes loader of libhumid_hip.so (include/humid_hip.h).

Fails loudly: there is no CPU fallback.  torch is imported first so that this library binds to
the HIP runtime torch already loaded (same soname libamdhip64.so.7) and device pointers /
streams are shared."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libhumid_hip.so")

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)


class HumidSummary(C.Structure):
    _fields_ = [("total", C.c_uint64), ("usable", C.c_uint64), ("unique", C.c_uint64),
                ("clusters", C.c_uint64), ("edges", C.c_uint64), ("nonsingle", C.c_uint64),
                ("ms_count", C.c_float), ("ms_neighbours", C.c_float), ("ms_cluster", C.c_float),
                ("ms_map", C.c_float), ("ms_total", C.c_float), ("ms_h2d", C.c_float),
                ("ms_d2h", C.c_float), ("ms_k_insert", C.c_float), ("ms_k_pairs", C.c_float),
                ("ms_k_cluster", C.c_float), ("ms_k_map", C.c_float), ("ms_k_part", C.c_float),
                ("ms_k_unperm", C.c_float), ("count_mode_used", C.c_uint32)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        # bit 8 of count_mode_used: the word-ordered count ran on 8-byte records (kernels_part8.hip.h)
        d["records8"] = bool(d["count_mode_used"] >> 8)
        d["count_mode_used"] &= 0xff
        return d


class HumidConsensusSummary(C.Structure):
    """humid_consensus_summary of include/humid_hip.h"""
    _fields_ = [(k, C.c_uint64) for k in ("n_clusters", "total_bytes", "multi_read", "bases_changed", "votes", "errors")]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class HumidDuplexSummary(C.Structure):
    """humid_duplex_summary of include/humid_hip.h"""
    _fields_ = [(k, C.c_uint64) for k in ("n_clusters", "total_bytes", "multi_read", "bases_changed", "votes", "errors",
                                          "duplex_clusters", "both_called", "agree", "disagree", "masked")]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class HumidOpticalSummary(C.Structure):
    """humid_optical_summary of include/humid_hip.h"""
    _fields_ = [(k, C.c_uint64) for k in ("n_clusters", "members", "duplicates", "optical", "groups", "largest_group")]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class HumidStrandSummary(C.Structure):
    """humid_strand_summary of include/humid_hip.h"""
    _fields_ = [(k, C.c_uint64) for k in ("n_clusters", "duplex", "top_only", "bottom_only", "top_reads", "bottom_reads")]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# HUMID_ROAD_* of include/humid_hip.h: the event codes of humid_get_run_roads, by name
ROADS = {1: "PART_PADDED_REDO", 2: "ORDERS_REDONE", 3: "REGIONS_REGROWN", 4: "FAR_TILES", 5: "CSR_TILES", 6: "JOIN_PIECES"}
ROADS_MAX = 32


class HumidRunRoads(C.Structure):
    """humid_run_roads of include/humid_hip.h"""
    _fields_ = [("n_events", C.c_uint32), ("graph_attempts", C.c_uint32), ("events", C.c_uint8 * ROADS_MAX)]

    def asdict(self):
        n = int(self.n_events)
        return dict(events=[ROADS[int(e)] for e in self.events[:min(n, ROADS_MAX)]], n_events=n,
                    graph_attempts=int(self.graph_attempts))


class HumidLongInfo(C.Structure):
    """humid_long_info_t of include/humid_hip.h"""
    _fields_ = [("words_per_read", C.c_uint32), ("joins", C.c_uint32), ("key_bits", C.c_uint32), ("piece_joins", C.c_uint32),
                ("candidates", C.c_uint64), ("raw_edges", C.c_uint64), ("edges", C.c_uint64)]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


HOST_ALL_GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, u64p, u64p, C.c_void_p, u64p, u64p, C.c_int, C.c_void_p)


class HumidBcPosteriorSummary(C.Structure):
    """humid_bc_posterior_summary of include/humid_hip.h"""
    _fields_ = [("counts", C.c_uint64 * 5), ("multi", C.c_uint64), ("rescued", C.c_uint64)]

    def asdict(self):
        return dict(counts=[int(x) for x in self.counts], multi=int(self.multi), rescued=int(self.rescued))


class HumidCellsSummary(C.Structure):
    """humid_cells_summary of include/humid_hip.h"""
    _fields_ = [(k, C.c_uint64) for k in ("usable", "invalid_reads", "distinct", "selected", "merged", "cells",
                                          "threshold_reads", "top_reads", "reads_in_cells")]

    def asdict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class HumidComm(C.Structure):
    """humid_comm of include/humid_hip.h: what moves bytes between ranks for humid_dedup_run_exchange"""
    _fields_ = [("user", C.c_void_p), ("rank", C.c_uint32), ("world", C.c_uint32),
                ("host_all_gather", HOST_ALL_GATHER_FN), ("exchange", EXCHANGE_FN)]


class HumidExchangeInfo(C.Structure):
    _fields_ = [("unique_local", C.c_uint64), ("id_base", C.c_uint64), ("n_nodes", C.c_uint64),
                ("n_pairs", C.c_uint64), ("d_unique_count", C.c_void_p), ("d_unique_degree", C.c_void_p)]


# every symbol include/humid_hip.h declares: (restype, argtypes)
SYMBOLS = {
    "humid_abi_version": (C.c_uint32, []),
    "humid_device_count": (C.c_int, []),
    "humid_ctx_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_void_p]),
    "humid_ctx_destroy": (None, [C.c_void_p]),
    "humid_last_error": (C.c_char_p, [C.c_void_p]),
    "humid_ctx_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "humid_ctx_reserve": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32]),
    "humid_host_alloc": (C.c_void_p, [C.c_uint64]),
    "humid_host_free": (None, [C.c_void_p]),
    "humid_dedup_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                  C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.POINTER(HumidSummary)]),
    "humid_dedup_run_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_dedup_run_bases": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_get_packed_words": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "humid_dedup_run_long": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_dedup_run_long_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_long_info": (C.c_int, [C.c_void_p, C.POINTER(HumidLongInfo)]),
    "humid_dedup_run_grouped": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                          C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.POINTER(HumidSummary)]),
    "humid_dedup_run_grouped_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                 C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_get_leaf_groups": (C.c_int, [C.c_void_p, C.c_void_p]),
    "humid_grouped_plan_info": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, u32p,
                                          u32p, u32p]),
    "humid_dedup_run_keyed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_dedup_run_keyed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.POINTER(HumidSummary)]),
    "humid_get_group_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "humid_keyed_rank_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), u32p, u32p]),
    "humid_whitelist_set": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]),
    "humid_whitelist_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), u32p, u32p]),
    "humid_whitelist_correct": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "humid_whitelist_correct_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]),
    "humid_dedup_run_keyed_corrected": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.POINTER(HumidSummary)]),
    "humid_dedup_run_keyed_corrected_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                         C.POINTER(HumidSummary)]),
    "humid_get_barcode_status": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "humid_whitelist_set_segments": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "humid_whitelist_segments_info": (C.c_int, [C.c_void_p, u32p, C.c_void_p, C.c_void_p, u32p]),
    "humid_get_barcode_segments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "humid_whitelist_correct_posterior": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.POINTER(HumidBcPosteriorSummary)]),
    "humid_whitelist_correct_posterior_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                           C.c_uint32, C.c_void_p, C.c_void_p,
                                                           C.POINTER(HumidBcPosteriorSummary)]),
    "humid_dedup_run_keyed_posterior": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                  C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.POINTER(HumidSummary)]),
    "humid_dedup_run_keyed_posterior_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                         C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                         C.c_void_p, C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_get_barcode_posterior": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "humid_whitelist_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "humid_whitelist_discover": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                           C.c_uint32, C.POINTER(HumidCellsSummary)]),
    "humid_whitelist_discover_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                                  C.c_uint64, C.c_uint32, C.POINTER(HumidCellsSummary)]),
    "humid_get_discovered_cells": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "humid_get_barcode_count_hist": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "humid_cells_begin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "humid_cells_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "humid_cells_add_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "humid_cells_finish": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(HumidCellsSummary)]),
    "humid_cells_info": (C.c_int, [C.c_void_p, u32p, u64p, u64p, u64p, u64p, u64p, u32p, u32p]),
    "humid_cells_clear": (C.c_int, [C.c_void_p]),
    "humid_whitelist_prior_begin": (C.c_int, [C.c_void_p]),
    "humid_whitelist_prior_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "humid_whitelist_prior_add_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "humid_whitelist_correct_posterior_prior": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                          C.c_uint32, C.c_void_p, C.c_void_p,
                                                          C.POINTER(HumidBcPosteriorSummary)]),
    "humid_whitelist_correct_posterior_prior_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                                 C.c_uint32, C.c_void_p, C.c_void_p,
                                                                 C.POINTER(HumidBcPosteriorSummary)]),
    "humid_get_group_stats": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "humid_group_stats_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)] + [C.POINTER(C.c_void_p)] * 4),
    "humid_select_best": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                    C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "humid_select_best_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "humid_consensus": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                  C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(HumidConsensusSummary)]),
    "humid_consensus_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                         C.POINTER(HumidConsensusSummary)]),
    "humid_get_consensus": (C.c_int, [C.c_void_p, C.c_uint64] + [C.c_void_p] * 5),
    "humid_consensus_result_device": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 5),
    "humid_duplex_consensus": (C.c_int, [C.c_void_p] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] * 2 + [C.c_void_p] * 3 +
                               [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(HumidDuplexSummary)]),
    "humid_duplex_consensus_device": (C.c_int, [C.c_void_p] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] * 2 +
                                      [C.c_void_p] * 3 + [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                                          C.POINTER(HumidDuplexSummary)]),
    "humid_get_duplex_consensus": (C.c_int, [C.c_void_p] * 4 + [C.POINTER(HumidDuplexSummary)]),
    "humid_optical_duplicates": (C.c_int, [C.c_void_p] * 6 + [C.c_uint64, C.c_uint64, C.c_uint32] + [C.c_void_p] * 3 +
                                 [C.POINTER(HumidOpticalSummary)]),
    "humid_optical_duplicates_device": (C.c_int, [C.c_void_p] * 6 + [C.c_uint64, C.c_uint64, C.c_uint32] +
                                        [C.c_void_p] * 3 + [C.POINTER(HumidOpticalSummary)]),
    "humid_paired_canonical": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                         C.c_void_p]),
    "humid_paired_canonical_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                                C.c_void_p]),
    "humid_dedup_run_paired": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_dedup_run_paired_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(HumidSummary)]),
    "humid_get_strands": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                    C.POINTER(HumidStrandSummary)]),
    "humid_accum_begin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "humid_accum_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "humid_accum_add_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "humid_accum_finish": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(HumidSummary)]),
    "humid_accum_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, u64p]),
    "humid_accum_map_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                         u64p]),
    "humid_accum_get_leaves": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "humid_accum_info": (C.c_int, [C.c_void_p, u32p, u64p, u64p, u64p, u64p, u32p]),
    "humid_accum_clear": (C.c_int, [C.c_void_p]),
    "humid_accum_begin_keyed": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "humid_accum_add_keyed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "humid_accum_add_keyed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
    "humid_accum_map_keyed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                        C.c_void_p, u64p]),
    "humid_accum_map_keyed_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                               C.c_void_p, C.c_void_p, u64p]),
    "humid_accum_get_leaves_keyed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]),
    "humid_accum_keyed_info": (C.c_int, [C.c_void_p, u32p, u32p, u64p]),
    "humid_get_leaves": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6),
    "humid_get_adjacency": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "humid_get_clusters": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "humid_get_histogram": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_uint64, u64p]),
    "humid_cluster_graph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, u32p]),
    "humid_stage_histogram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                        C.c_uint32, C.c_void_p]),
    "humid_stage_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                    C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p]),
    "humid_stage_unique": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                     C.POINTER(C.c_void_p)]),
    "humid_stage_graph": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_void_p), C.POINTER(HumidSummary)]),
    "humid_stage_map": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                  C.c_void_p]),
    "humid_stage_count_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                          C.c_uint64, C.c_uint64, u64p, C.c_uint32, u64p, u64p, u64p]),
    "humid_stage_map_dense": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), u64p]),
    "humid_stage_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), u64p]),
    "humid_graph_split_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), u32p]),
    "humid_group_records_info": (C.c_int, [C.c_void_p, u32p, u32p]),
    "humid_wait_overlap_info": (C.c_int, [C.c_void_p, u32p, u32p]),
    "humid_stamp_info": (C.c_int, [C.c_void_p, u32p, C.POINTER(C.c_uint64), u32p]),
    "humid_get_run_roads": (C.c_int, [C.c_void_p, C.POINTER(HumidRunRoads)]),
    "humid_stage_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), u32p]),
    "humid_stage_route_words": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "humid_stage_route": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p, u64p, C.c_uint32, u64p,
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "humid_stage_route_check": (C.c_int, [C.c_void_p]),
    "humid_stage_exchange_ids": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_void_p)]),
    "humid_stage_plan_info": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, u32p, u32p]),
    "humid_stage_combo_route": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                          C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_void_p), u64p]),
    "humid_stage_pairs_keyed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64,
                                          C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                          C.POINTER(C.c_void_p), u64p]),
    "humid_stage_compact_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                            C.POINTER(C.c_void_p), u64p, C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p)]),
    "humid_stage_pairs_edit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), u64p]),
    "humid_stage_unique_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                           C.POINTER(C.c_void_p), u64p]),
    "humid_stage_graph_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(HumidSummary)]),
    "humid_stage_owned_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, u64p, C.c_uint32,
                                            C.POINTER(C.c_void_p), u64p]),
    "humid_stage_owner_perm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p, u64p,
                                         C.c_uint32, C.POINTER(C.c_void_p), u64p]),
    "humid_stage_owner_perm_wide": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, u64p, u64p,
                                              C.c_uint32, C.POINTER(C.c_void_p), u64p]),
    "humid_stage_scatter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                      C.c_void_p, C.c_void_p]),
    "humid_dedup_run_exchange": (C.c_int, [C.c_void_p, C.POINTER(HumidComm), C.c_void_p, C.c_void_p, C.c_uint64,
                                           C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.POINTER(HumidSummary), C.POINTER(HumidExchangeInfo)]),
    "humid_shm_open": (C.c_int, [C.POINTER(C.c_void_p), C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64]),
    "humid_shm_all_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "humid_shm_abort": (None, [C.c_void_p]),
    "humid_shm_close": (None, [C.c_void_p]),
    "humid_at_least_double": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_int)]),
}

_LIB = None


class HumidLibraryError(RuntimeError):
    pass


def load(import_torch: bool = True):
    """dlopen the HIP library and bind every C-ABI symbol.  Raises if it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if import_torch:
        try:
            import torch  # noqa: F401  (loads libamdhip64.so.7 first; see module docstring)
        except Exception:  # torch absent: the library still works with the system runtime
            pass
    if not os.path.exists(SO_PATH):
        raise HumidLibraryError(
            "%s not found: build it with `python -m humid_amd.build` (hipcc, gfx950). "
            "humid_amd has no CPU fallback." % SO_PATH)
    try:
        lib = C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)
    except OSError as e:
        raise HumidLibraryError("cannot load %s: %s" % (SO_PATH, e)) from e
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HumidLibraryError("%s does not export %s" % (SO_PATH, name)) from e
        fn.restype = res
        fn.argtypes = args
    if lib.humid_abi_version() != 5:
        raise HumidLibraryError("ABI version mismatch")
    _LIB = lib
    return lib
