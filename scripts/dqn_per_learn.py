#!/usr/bin/env python3
"""At which learning rate does a 20,000-step DQN run learn CartPole? -> profiles/dqn_per_learn.json, what tests/test_gpu_dqn_per.py's learning test
is built on (as profiles/ddpg_pendulum_train.json is for DDPG's).

Eight seeds, prioritized and uniform replay, the reference's DQNConfig at lr = 1e-4 (its default, meant for 500,000 steps) and at lr = 1e-3 (the
rate of every DQN parity test here): crl_dqn_evaluate of the initial network and after every 5,000 steps, 256 fresh CartPoles each. 20,000 steps are
2,000 updates of which 1,000 come after ε has reached 0.05; at lr = 1e-4 Adam can move a weight by at most 0.2 in them.

usage: python scripts/dqn_per_learn.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, SEEDS, EVAL_ENVS = 20_000, 8, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_per_learn.json"))
    args = ap.parse_args()
    import cleanrl_jl_amd as crl
    runs = {}
    for lr in (1e-3, 1e-4):
        for arm in ("per", "uniform"):
            rows = {}
            for seed in range(1, SEEDS + 1):
                agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=STEPS, lr=lr), seed=seed, init_seed=seed,
                                     per=crl.PEROptions() if arm == "per" else None)
                ret = [crl.dqn_evaluate(agent, num_envs=EVAL_ENVS)["report"]["return_mean"]]
                for _ in range(4):
                    agent.handle.run(STEPS // 4)
                    ret.append(crl.dqn_evaluate(agent, num_envs=EVAL_ENVS)["report"]["return_mean"])
                agent.close()
                rows[str(seed)] = ret
            runs[f"lr{lr:g}/{arm}"] = rows
            print(f"lr {lr:g} {arm:8s} initial -> 20,000 steps:", [f"{r[0]:.1f}->{r[-1]:.1f}" for r in rows.values()])
    prof = {"what": "held-out greedy return_mean (crl_dqn_evaluate, 256 envs) of the initial network and after 5,000 / 10,000 / 15,000 / 20,000 steps "
                    "of DQN at the reference's defaults but for lr; seed s sets the training seed and the initial network (scripts/dqn_per_learn.py)",
            "steps": STEPS, "eval_envs": EVAL_ENVS, "runs": runs}
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
