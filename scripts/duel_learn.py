#!/usr/bin/env python3
"""Does a 20,000-step DQN run with dueling heads learn CartPole? -> profiles/duel_learn.json, what tests/test_gpu_duel.py's learning test is built
on (as profiles/c51_learn.json is for C51's).

Eight seeds, the reference's DQNConfig at lr = 1e-3 (the rate of every DQN parity test here and of test_per_agent_learns, whose docstring says why
not the default 1e-4). Two arms: duel (the scalar dueling head) and duel_c51_per_n3_double (dueling + C51Options() + PEROptions() +
DQNTargetOptions(3, True)): crl_dqn_evaluate of the initial network and after every 5,000 steps, 256 fresh CartPoles each. Nothing is selected: a seed
that does not learn is in the file.

usage: python scripts/duel_learn.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, SEEDS, EVAL_ENVS, LR = 20_000, 8, 256, 1e-3


def arms(crl):
    return {"duel": {}, "duel_c51_per_n3_double": dict(per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True), dist=crl.C51Options())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duel_learn.json"))
    args = ap.parse_args()
    import cleanrl_jl_amd as crl
    runs = {}
    for arm, kw in arms(crl).items():
        rows = {}
        for seed in range(1, SEEDS + 1):
            agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=STEPS, lr=LR), seed=seed, init_seed=seed, dueling=True, **kw)
            ret = [crl.dqn_evaluate(agent, num_envs=EVAL_ENVS)["report"]["return_mean"]]
            for _ in range(4):
                agent.handle.run(STEPS // 4)
                ret.append(crl.dqn_evaluate(agent, num_envs=EVAL_ENVS)["report"]["return_mean"])
            agent.close()
            rows[str(seed)] = ret
        runs[arm] = rows
        print(f"{arm:24s} initial -> 20,000 steps:", [f"{r[0]:.1f}->{r[-1]:.1f}" for r in rows.values()], flush=True)
    prof = {"what": "held-out greedy return_mean (crl_dqn_evaluate, 256 envs) of the initial network and after 5,000 / 10,000 / 15,000 / 20,000 steps "
                    "of DQN with dueling heads at the reference's defaults but for lr: the scalar dueling head, and dueling + C51 + PER + 3-step + "
                    "double; seed s sets the training seed and the initial network (scripts/duel_learn.py)",
            "steps": STEPS, "eval_envs": EVAL_ENVS, "lr": LR, "runs": runs,
            "seeds_that_learned": {arm: sorted(int(s) for s, r in rows.items() if r[-1] > r[0]) for arm, rows in runs.items()}}
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
