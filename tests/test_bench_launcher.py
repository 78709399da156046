"""bench.py as its own launcher: a bare `python bench.py --gpus N` must never
print a line for fewer ranks than it was asked for.  No GPU here: the ranks it starts fail, and what is
checked is that they WERE started with the rank environment, that the failure reaches the exit code and
that no line is printed.  Also: what a plain run leaves to --full, and the files of --dump-outputs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_bare_gpus_n_starts_n_ranks_and_propagates_their_failure():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip("a GPU is present: the launcher is exercised by the rehearsal under profiles/")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--reads", "1000", "--cpu-sample", "0", "--e2e-reads", "0"],
                       env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    err = p.stderr.decode()
    assert p.returncode != 0
    assert p.stdout.decode().strip() == ""                      # no line for a run that did not happen
    assert "needs a GPU" in err                                 # the children got as far as looking for their device
    assert "rank" in err and "exited with" in err


def test_external_launcher_with_another_world_size_is_refused():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0",
                        "--reads", "1000"],
                       env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert p.returncode != 0
    assert p.stdout.decode().strip() == ""
    assert "WORLD_SIZE 1 != --gpus 4" in p.stderr.decode()


def test_launcher_withholds_a_line_of_the_wrong_size(tmp_path, monkeypatch):
    """spawn_ranks with stand-in children: rank 0 prints n_gpus = 1 for --gpus 2 -> no line, non-zero exit"""
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    fake = tmp_path / "fake_bench.py"
    fake.write_text("import json, os\n"
                    "if os.environ['RANK'] == '0': print(json.dumps({'n_gpus': int(os.environ.get('FAKE_N', '1'))}))\n")
    monkeypatch.setattr(bench, "__file__", str(fake))
    monkeypatch.setattr(sys, "argv", ["bench.py"])

    class A:
        gpus = 2
    import pytest
    with pytest.raises(SystemExit) as ei:
        bench.spawn_ranks(A())
    assert ei.value.code not in (0, None)
    monkeypatch.setenv("FAKE_N", "2")
    with pytest.raises(SystemExit) as ei:
        bench.spawn_ranks(A())
    assert ei.value.code == 0


def _parse(monkeypatch, *args):
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(args))
    return bench.parse()


def test_plain_run_leaves_the_extra_legs_to_full(monkeypatch):
    a = _parse(monkeypatch, "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full) == (7, 2, False)
    assert (a.cpu_sample, a.e2e_reads, a.verify) == (0, 0, False)
    a = _parse(monkeypatch, "--full")
    assert (a.cpu_sample, a.e2e_reads, a.verify) == (-1, 10_000_000, True)
    a = _parse(monkeypatch, "--cpu-sample", "5000", "--no-verify", "--full")      # explicit values win
    assert (a.cpu_sample, a.verify) == (5000, False)
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_writes_float_arrays_of_a_fixed_sample(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import importlib
    import numpy as np
    bench = importlib.import_module("bench")
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    n = 5000
    cid = np.arange(n, dtype=np.uint32) * np.uint32(858_993)          # ids up to ~4.3e9: exact only in float64
    keep = (np.arange(n) % 3 == 0).astype(np.uint8)
    summary = dict(total=n, usable=n - 1, unique=7, clusters=5, edges=3, ms_total=0.5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), cid, keep, summary)
    got = {f: np.load(tmp_path / "a" / f) for f in ("read_index.npy", "cluster_id.npy", "keep.npy", "summary.npy")}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    idx = got["read_index.npy"].astype(np.int64)
    assert len(idx) == 1000 and len(np.unique(idx)) == 1000 and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(got["cluster_id.npy"].astype(np.uint32), cid[idx])
    assert np.array_equal(got["keep.npy"].astype(np.uint8), keep[idx])
    assert got["summary.npy"].tolist() == [n, n - 1, 7, 5, 3]
    for f, v in got.items():                                          # the same sample every time
        assert np.array_equal(np.load(tmp_path / "b" / f), v)
    monkeypatch.undo()
    assert bench.DUMP_SAMPLE * (8 + 8 + 4) <= 64 << 20               # the cap on what a dump writes


@pytest.mark.gpu
def test_dumped_outputs_of_a_plain_run_match_the_oracle(tmp_path):
    """a plain run at a small size: one JSON line with the headline fields, and the dumped results of its last timed
    pass equal the oracle's on the same seeded reads"""
    import numpy as np
    sys.path.insert(0, ROOT)
    from humid_amd.synth import synth_words
    from oracle import pyoracle as orc
    n = 200_000
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--reads", str(n), "--dump-outputs", str(tmp_path / "out")],
                       env=_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    line = json.loads(p.stdout.decode().strip())
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "reads/s" and line["dtype"] == "u64" and line["value"] > 0
    assert line["cpu_baseline"] is None and line["roofline"] is None and "e2e" not in line
    words, filt = synth_words(n, 1002, 24)                     # bench.py's seed for its read set
    ocid, okeep, osum, _ = orc.dedup_run(words, filt, 24, 1, 0)
    d = tmp_path / "out"
    idx = np.load(d / "read_index.npy").astype(np.int64)
    assert np.array_equal(idx, np.arange(n))
    assert np.array_equal(np.load(d / "cluster_id.npy").astype(np.uint32), ocid)
    assert np.array_equal(np.load(d / "keep.npy").astype(np.uint8), okeep)
    assert np.load(d / "summary.npy").tolist() == [osum[k] for k in ("total", "usable", "unique", "clusters", "edges")]
