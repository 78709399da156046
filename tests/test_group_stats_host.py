"""CPU checks of the per-group statistics (include/humid_hip.h, humid_get_group_stats / humid_group_stats_device)
and of the groups.dat table of `humid -b K -s`: what needs no device -- the exported symbols, the refusal of a NULL
context, the usage text and the command line's refusals, which come before any output exists."""
import os
import subprocess

from humid_amd import _lib
from humid_amd.synth import synth_fastq

from cli_util import HUMID

NEW_SYMBOLS = ("humid_get_group_stats", "humid_group_stats_device")


def test_group_stats_symbols_are_exported():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name), name
    assert lib.humid_abi_version() == 5


def test_null_context_is_refused():
    lib = _lib.load()
    assert lib.humid_get_group_stats(None, 0, None, None, None, None, None) == -1
    assert lib.humid_group_stats_device(None, None, None, None, None, None) == -1
    assert b"ctx is null" in lib.humid_last_error(None)


def test_python_surface_exists():
    import humid_amd
    assert callable(humid_amd.Dedup.group_stats) and callable(humid_amd.Dedup.group_stats_device)
    assert "valid until" in humid_amd.Dedup.group_stats_device.__doc__        # the lifetime is stated


def test_usage_names_groups_dat():
    r = subprocess.run([HUMID, "-h"], capture_output=True, timeout=60)
    assert r.returncode == 0
    assert b"groups.dat" in r.stderr and b"-b" in r.stderr


def test_cli_still_refuses_barcode_statistics_on_two_gpus(tmp_path):
    """-b ... -s with -g 2: exit code 2 before any output directory exists"""
    files = synth_fastq(str(tmp_path), 4, 8, n_files=1, read_len=40)
    r = subprocess.run([HUMID, "-n", "28", "-b", "16", "-s", "-g", "2", "-d", str(tmp_path / "out"), "-l", "/dev/null"]
                       + files, capture_output=True, timeout=60)
    assert r.returncode == 2, r.stderr
    assert b"-b" in r.stderr and b"one GPU" in r.stderr
    assert not os.path.exists(tmp_path / "out")
