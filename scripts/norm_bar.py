#!/usr/bin/env python3
"""Measures, on the CPU, the bar tests/test_gpu_norm.py holds the statistics of crl_norm to. The device forms batch moments per tile of 256 envs and
merges the tiles in index order: a reordering of the reference's whole-batch Float64 sums. The floor of that class of reorderings is measured on the
tests' own tapes as the largest spread, over every frame of every case, between tests/norm_ref.py with whole-batch moments and with tile-wise merges
(tiles of 64 and 256, forward and reverse): of count and mean relative to |mean| + sqrt(var), of var relative to var. The bar is MARGIN = 16 x the
floor, the margin standing for the device's different order INSIDE a tile. The script also shows that the bar is sharp: batch variances formed as
E[x²] − mean² must miss it by at least 1e3 bars on the mean 1e4 / std 1e-2 dimension, or the script fails. Writes profiles/norm_bar.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import norm_ref as R  # noqa: E402

MARGIN = 16.0


def spread(a, b, D):
    """(count / mean spread, var spread) of two state vectors"""
    def mean(s): return np.r_[s[1:1 + D], s[2 * D + 2]]
    def var(s): return np.r_[s[1 + D:1 + 2 * D], s[2 * D + 3]]
    def cnt(s): return np.r_[s[0], s[2 * D + 1]]
    scale = np.abs(mean(a)) + np.sqrt(var(a))
    e_m = max(np.max(np.abs(mean(a) - mean(b)) / scale), np.max(np.abs(cnt(a) - cnt(b)) / cnt(a)))
    return float(e_m), float(np.max(np.abs(var(a) - var(b)) / var(a)))


def main():
    floor_m = floor_v = miss = 0.0
    for N, D in R.CASES:
        t = R.tape(N, D)
        base = R.run(R.Ref(N, D), *t)[0]
        for T in (64, 256):
            for rev in (False, True):
                for a, b in zip(base, R.run(R.Ref(N, D, moments=R.tiled(T, rev)), *t)[0]):
                    e_m, e_v = spread(a, b, D)
                    floor_m, floor_v = max(floor_m, e_m), max(floor_v, e_v)
        if D >= 2:
            for a, b in zip(base, R.run(R.Ref(N, D, moments=R.tiled(256, sumsq=True)), *t)[0]):
                miss = max(miss, abs(a[1 + D + 1] - b[1 + D + 1]) / a[1 + D + 1])      # var of dimension 1: mean 1e4, std 1e-2
    out = {"margin": MARGIN, "floor_mean": floor_m, "floor_var": floor_v, "bar_mean": MARGIN * floor_m, "bar_var": MARGIN * floor_v,
           "sumsq_var_error": miss, "sumsq_over_bar": miss / (MARGIN * floor_v),
           "note": "spread of tests/norm_ref.py under tile-wise merges (64 / 256, forward / reverse) on the tests' tapes; mean and count relative to "
                   "|mean| + sqrt(var), var relative to var"}
    assert floor_m > 0 and floor_v > 0, "the tapes show no reordering spread"
    assert out["sumsq_over_bar"] >= 1e3, f"E[x²] − mean² misses the bar by {out['sumsq_over_bar']:.1e} bars only: sharpen the tape"
    with open(os.path.join(ROOT, "profiles", "norm_bar.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
