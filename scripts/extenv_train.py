"""The six training curves behind tests/test_gpu_extenv.py's end-to-end check: ppo(config, env=LibraryEnv("cartpole", 256)) and ppo(config, env="cartpole"),
three seeds each, mean episode return per update -> profiles/extenv_train.json, with the seed-to-seed spread of the built-in runs.

    python scripts/extenv_train.py [--out profiles/extenv_train.json]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cleanrl_jl_amd as crl  # noqa: E402
from test_gpu_extenv import episode_return_curve  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "extenv_train.json"))
    args = ap.parse_args()
    out = {"config": "PPOConfig(num_envs=256, num_steps=128, total_timesteps=256*128*40), CartPole 4/2/64", "curves": {"external": {}, "builtin": {}}}
    with tempfile.TemporaryDirectory() as tmp:
        for seed in (1, 2, 3):
            out["curves"]["external"][str(seed)] = episode_return_curve(crl, tmp, True, seed)
            out["curves"]["builtin"][str(seed)] = episode_return_curve(crl, tmp, False, seed)
    last = {k: [float(np.mean(c[-5:])) for c in v.values()] for k, v in out["curves"].items()}
    out["last_five_mean"] = last
    out["builtin_min_over_max"] = min(last["builtin"]) / max(last["builtin"])
    out["external_over_builtin"] = float(np.mean(last["external"]) / np.mean(last["builtin"]))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("last_five_mean", "builtin_min_over_max", "external_over_builtin")}))


if __name__ == "__main__":
    main()
