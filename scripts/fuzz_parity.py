#!/usr/bin/env python3
"""Randomised whole-iteration parity from a shell (the case itself: tests/fuzzlib.py; 40 cases of seed 1 run in the GPU test suite as
tests/test_gpu_fuzz.py). Prints one line per configuration and a summary; exit code 1 on any mismatch.
--wide draws layer-wise configurations instead (fuzzlib.run_wide_case: random shape, GEMM flavour and activation form).
Usage: python scripts/fuzz_parity.py [--wide] [n_configs] [seed]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import cleanrl_jl_amd as crl          # noqa: E402
import fuzzlib                         # noqa: E402
import oraclelib as O                  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--wide"]
run = fuzzlib.run_wide_case if "--wide" in sys.argv[1:] else fuzzlib.run_case
N = int(args[0]) if len(args) > 0 else 40
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 1)
fails = []
for case in range(N):
    line = run(crl, O, rng, case)
    print(json.dumps(line), flush=True)
    if not line["ok"]:
        fails.append(line)
print(json.dumps({"configs": N, "failed": len(fails)}))
sys.exit(1 if fails else 0)
