"""-m gpu: `humid -b K --cells-expected N` end to end.  cells.dat and barcode_rank.dat against the truth of
tests/cells_truth.py on the barcodes of the oracle's word extraction (cli_util.expected_words, split at K); every
other output byte for byte against a second run that is given the cells of cells.dat as its -w whitelist."""
import os
import subprocess

import numpy as np
import pytest

from cli_util import HUMID, expected_words
from test_cli_keyed_gpu import split_words
from test_cli_whitelist_gpu import K, letters, whitelisted_fastq

import cells_truth as ct

pytestmark = pytest.mark.gpu


def run(args, files, out, log):
    subprocess.check_call([HUMID, "-n", "28", "-b", str(K), "-d", out, "-l", log, "-s", "-a"] + args + files, timeout=300)


@pytest.mark.parametrize("cells_flags,ratio,more", [
    (["--cells-expected", "30"], 0, []),
    (["--cells-expected", "30", "--cells-merge-ratio", "5"], 5, []),
    (["--cells-expected", "30"], 0, ["--barcode-posterior"]),
    (["--cells-min-reads", "2", "--cells-merge-ratio", "5"], 5, ["--barcode-posterior", "-x"]),
], ids=["expected", "expected_merge", "expected_posterior", "min_reads_merge_posterior_maximum"])
def test_cells_from_the_data_equal_the_whitelist_run(cells_flags, ratio, more, tmp_path):
    files, _, planted = whitelisted_fastq(tmp_path, 4000, 71)
    out1, out2 = str(tmp_path / "cells"), str(tmp_path / "listed")
    log1, log2 = str(tmp_path / "log1.txt"), str(tmp_path / "log2.txt")
    run(cells_flags + more, files, out1, log1)
    # the truth, on the barcodes the oracle extracts
    words, filt, _, _ = expected_words(files, 28)
    keys, _ = split_words(words, 28, K)
    mode, param = (ct.EXPECTED, 30) if cells_flags[0] == "--cells-expected" else (ct.MIN_READS, 2)
    cells, reads, sm, hist = ct.discover(np.asarray(keys, np.uint64), filt, K, mode, param, ratio)
    assert 10 <= sm["cells"] < sm["distinct"] and (mode == ct.EXPECTED or sm["merged"] > 0)   # (the low threshold lets error barcodes in)
    assert open(os.path.join(out1, "cells.dat")).read() == "".join("%s %d\n" % (letters(v), n) for v, n in zip(cells, reads))
    assert open(os.path.join(out1, "barcode_rank.dat")).read() == "".join("%d %d\n" % (n, b) for n, b in zip(*hist))
    assert ("  cells: %d of %d barcodes (%d selected at %d reads or more, %d merged away), %d of %d usable reads in cells"
            % (sm["cells"], sm["distinct"], sm["selected"], sm["threshold_reads"], sm["merged"], sm["reads_in_cells"], sm["usable"])) \
        in open(log1).read()
    # the second run: -w with the first column of cells.dat
    wl_path = str(tmp_path / "from_cells.txt")
    with open(wl_path, "w") as fh:
        for line in open(os.path.join(out1, "cells.dat")):
            fh.write(line.split()[0] + "\n")
    run(["-w", wl_path] + more, files, out2, log2)
    names = sorted(os.listdir(out2))
    assert sorted(os.listdir(out1)) == sorted(names + ["cells.dat", "barcode_rank.dat"])
    assert {"cells_dedup.fastq", "cells_annotated.fastq", "groups.dat", "barcodes.dat", "stats.dat"} <= set(names)
    for name in names:
        assert open(os.path.join(out1, name), "rb").read() == open(os.path.join(out2, name), "rb").read(), name
    got_groups = set(l.split()[0] for l in open(os.path.join(out1, "groups.dat")))
    assert got_groups <= set(letters(v) for v in cells) and len(got_groups) >= 10


def test_no_cell_is_an_error(tmp_path):
    files, _, _ = whitelisted_fastq(tmp_path, 500, 73)
    out = str(tmp_path / "out")
    r = subprocess.run([HUMID, "-n", "28", "-b", str(K), "-d", out, "-l", str(tmp_path / "log.txt"), "--cells-min-reads", "100000"]
                       + files, capture_output=True, timeout=300)
    assert r.returncode == 1 and b"no cell barcode was found" in r.stderr
    assert "  cells: 0 of " in open(tmp_path / "log.txt").read()
