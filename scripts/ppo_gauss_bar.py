#!/usr/bin/env python3
"""Measures, on the CPU, the bars of tests/test_gpu_ppo_gauss.py for the two quantities that have no discrete counterpart — the xi recovered from the
rollout buffer and the Pendulum trajectory over three episodes — as the spread of tests/ppo_gauss_ref.py run in Float32 against itself in Float64 on the
tests' own inputs, times a margin of 8 for the device's expf / tanhf / sincos / log, whose own error was NOT measured. Writes profiles/ppo_gauss_bar.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cleanrl_jl_amd as crl  # noqa: E402
import ppo_gauss_ref as G  # noqa: E402

MARGIN = 8.0


def main():
    out = {"margin": MARGIN, "note": "float32-vs-float64 spread of tests/ppo_gauss_ref.py on the tests' inputs; the device's own transcendental error is unmeasured"}
    spread = 0.0
    for ad, D, Hd, kind in G.ROLLOUT_CASES:
        p, obs, xi = G.xi_case(crl._lib, ad, D, Hd, kind)
        r32, r64 = (G.recovered_xi(p, obs, xi, D, ad, Hd, G.LO, G.HI, dt) for dt in (np.float32, np.float64))
        spread = max(spread, float(np.max(np.abs(r32 - r64))))
    out["xi_spread"] = spread; out["xi_bar"] = MARGIN * spread
    t32, t64 = G.pendulum_trajectory(np.float32), G.pendulum_trajectory(np.float64)
    for key in ("obs", "reward"):
        s = float(np.max(np.abs(t32[key].astype(np.float64) - t64[key])))
        out[f"pendulum_{key}_spread"] = s; out[f"pendulum_{key}_bar"] = MARGIN * s
    out["pendulum_done_equal"] = bool(np.array_equal(t32["done"], t64["done"]))
    with open(os.path.join(ROOT, "profiles", "ppo_gauss_bar.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
