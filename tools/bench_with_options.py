#!/usr/bin/env python3
"""bench.py with context options set: `python tools/bench_with_options.py pair_split=0 [bench.py arguments]`.

bench.py has no switch for the tuning options of humid_ctx_set_option; this sets the given KEY=VALUE pairs on every
humid_amd.Dedup that bench.py makes and then runs bench.py unchanged (profiles/r04b_pair_split.md: the pair_split = 0
row)."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import humid_amd  # noqa: E402


def main():
    options = []
    args = sys.argv[1:]
    while args and "=" in args[0] and not args[0].startswith("-"):
        key, value = args.pop(0).split("=", 1)
        options.append((key, int(value)))
    init = humid_amd.Dedup.__init__

    def init_with_options(self, *a, **k):
        init(self, *a, **k)
        for key, value in options:
            self.set_option(key, value)

    humid_amd.Dedup.__init__ = init_with_options
    sys.argv = [os.path.join(ROOT, "bench.py")] + args
    runpy.run_path(sys.argv[0], run_name="__main__")


if __name__ == "__main__":
    main()
