"""Builds and loads the test harnesses under tests/csrc/ (test infrastructure): prims_harness.hip, the scan and radix
sort of humid_amd/csrc/prims.hip.h behind a C interface, and edit_harness.hip, the verifiers of the edit-distance
search (humid_amd/csrc/kernels_graph.hip.h) one thread per pair.  hipcc cross-compiles for gfx950 without a GPU; the
built libraries lie under tests/_build/ (git-ignored) and travel to the GPU box with the tree."""
import ctypes
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "humid_amd", "csrc")
SRC = os.path.join(HERE, "csrc", "prims_harness.hip")
SO = os.path.join(HERE, "_build", "libprims_harness.so")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("prims.hip.h", "common.hip.h")]
EDIT_SRC = os.path.join(HERE, "csrc", "edit_harness.hip")
EDIT_SO = os.path.join(HERE, "_build", "libedit_harness.so")
EDIT_DEPS = [EDIT_SRC] + [os.path.join(CSRC, f) for f in ("kernels_graph.hip.h", "common.hip.h")]


def _build_one(src, so, deps, force):
    if not force and os.path.exists(so) and all(os.path.getmtime(p) <= os.path.getmtime(so) for p in deps):
        return so
    os.makedirs(os.path.dirname(so), exist_ok=True)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                           "-I", CSRC, "-o", so, src], cwd=ROOT)
    return so


def build(force: bool = False) -> str:
    """both libraries; returns the path of the scan / sort harness"""
    _build_one(EDIT_SRC, EDIT_SO, EDIT_DEPS, force)
    return _build_one(SRC, SO, DEPS, force)


def load():
    import torch  # noqa: F401  (the HIP runtime torch loads comes first, as in humid_amd/_lib.py)
    lib = ctypes.CDLL(build())
    vp, u64, u32, i = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    lib.ph_exscan_u32.argtypes = [vp, vp, u64, i]
    lib.ph_exscan_u64.argtypes = [vp, vp, u64, i]
    lib.ph_sort_u32.argtypes = [vp, vp, vp, vp, u64, u32, u32, i, i]
    lib.ph_sort_u64.argtypes = [vp, vp, vp, vp, u64, u32, u32, i, i]
    lib.ph_set_epoch.argtypes = [u32]
    lib.ph_epoch.restype = u32
    return lib


def load_edit():
    """the verifier harness: eh_verify(x, y, count, word_nt, out u32[count, 3]) on host arrays"""
    import torch  # noqa: F401
    build()
    lib = ctypes.CDLL(EDIT_SO)
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.eh_verify.argtypes = [vp, vp, u32, u32, vp]
    lib.eh_verify.restype = ctypes.c_int
    return lib


if __name__ == "__main__":
    print(build(force=True))
