#!/usr/bin/env python3
"""Rollout time per iteration (crl_prof_read, CRL_K_ROLLOUT) of the on-device envs against the synthetic env at the same shape, 2x256,
16384 envs x 128 steps: is the env step on the rollout's critical path?  (output kept in profiles/env_rollout_cost.txt)

    python scripts/env_rollout_cost.py [acrobot mountaincar synth6 synth2 c3]     # CRL_LIB_PATH selects another build of the library
"""
import os
import sys

import numpy as np

ROOT = os.environ.get("CRL_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # CRL_TREE: another checkout (A/B against a parent build)
sys.path.insert(0, ROOT)
import cleanrl_jl_amd as crl  # noqa: E402

L = crl._lib
CASES = {"acrobot": (getattr(L, "ENV_ACROBOT", None), 6, 3), "mountaincar": (getattr(L, "ENV_MOUNTAINCAR", None), 2, 3),
         "synth6": (L.ENV_SYNTHETIC, 6, 3), "synth2": (L.ENV_SYNTHETIC, 2, 3), "c3": (L.ENV_SYNTHETIC, 8, 4)}


def main():
    names = sys.argv[1:] or list(CASES)
    nt, k, warm, reps = 16384, 128, 3, 10
    for name in names:
        kind, D, A = CASES[name]
        cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 100)
        agent = crl.Agent(cfg, obs_dim=D, n_act=A, hidden=256, env_kind=kind)
        h = agent.handle
        h.env_reset()
        for _ in range(warm):
            h.rollout_run()
        h.sync()
        ms = []
        for _ in range(reps):
            h.prof_enable(1); h.prof_reset()
            h.rollout_run(); h.sync()
            t, n = h.prof_read()["rollout"]
            ms.append(t)
        ms = np.array(ms)
        print(f"{name:12s} obs {D} act {A} 2x256 {nt} envs x {k} steps: rollout median {np.median(ms):.3f} ms  min {ms.min():.3f}  max {ms.max():.3f}  "
              f"({os.environ.get('CRL_LIB_PATH', 'this build')})", flush=True)
        agent.close()


if __name__ == "__main__":
    main()
