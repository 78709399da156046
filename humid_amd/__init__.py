"""humid_amd -- MI355X-native neighbour-search-and-cluster hot path of HUMID.

The compute lives in libhumid_hip.so (hand-written HIP for gfx950, C ABI in
include/humid_hip.h).  This package is the Python host side: the ctypes binding, the mirror of
the reference's surface for this path, the multi-GPU orchestration and the synthetic inputs.
"""
from .api import (Accumulator, BarcodeCounter, BC_AMBIGUOUS, BC_CORRECTED, BC_EXACT, BC_FILTERED, BC_UNMATCHED,  # noqa: F401
                  BEST_CLUSTER, BEST_LEAF, CELLS_EXPECTED, CELLS_MIN_READS, CELLS_TOP, DIRECTIONAL, MAXIMUM, NO_READ, NO_TILE, STRAND_BOTTOM, STRAND_NONE, STRAND_TOP, ClusterGraph, Context, Dedup, HumidError, KeyedAccumulator, at_least_double)

__version__ = "0.1.0"
