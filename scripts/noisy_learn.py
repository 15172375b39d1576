#!/usr/bin/env python3
"""Does a 20,000-step DQN run with noisy linear layers and NO ε-greedy exploration learn CartPole? -> profiles/noisy_learn.json, what
tests/test_gpu_noisy.py's learning test is built on (as profiles/duel_learn.json is for the dueling heads').

Eight seeds, the reference's DQNConfig at lr = 1e-3 (the rate of every DQN parity test here and of test_per_agent_learns, whose docstring says why
not the default 1e-4) with epsilon_start = epsilon_end = 0: the agent explores by its noise alone. Two arms: noisy (dqn.jl's net with noisy layers)
and rainbow (noisy + dueling + C51Options() + PEROptions() + DQNTargetOptions(3, True)): crl_dqn_evaluate (the noise off) of the initial network and
after every 5,000 steps, 256 fresh CartPoles each, and the mean |sigma| per array at the same points. Nothing is selected: a seed that does not learn
is in the file.

usage: python scripts/noisy_learn.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, SEEDS, EVAL_ENVS, LR = 20_000, 8, 256, 1e-3


def arms(crl):
    return {"noisy": {}, "rainbow": dict(dueling=True, per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True), dist=crl.C51Options())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noisy_learn.json"))
    args = ap.parse_args()
    import cleanrl_jl_amd as crl
    runs, sigmas = {}, {}
    for arm, kw in arms(crl).items():
        rows, sg = {}, {}
        for seed in range(1, SEEDS + 1):
            cfg = crl.DQNConfig(total_timesteps=STEPS, lr=LR, epsilon_start=0.0, epsilon_end=0.0)
            agent = crl.DQNAgent(cfg, seed=seed, init_seed=seed, noisy=crl.NoisyOptions(), **kw)
            ret, s = [crl.dqn_evaluate(agent, num_envs=EVAL_ENVS)["report"]["return_mean"]], [crl.noisy_sigma(agent)]
            for _ in range(4):
                agent.handle.run(STEPS // 4)
                ret.append(crl.dqn_evaluate(agent, num_envs=EVAL_ENVS)["report"]["return_mean"]); s.append(crl.noisy_sigma(agent))
            agent.close()
            rows[str(seed)], sg[str(seed)] = ret, s
        runs[arm], sigmas[arm] = rows, sg
        print(f"{arm:8s} initial -> 20,000 steps:", [f"{r[0]:.1f}->{r[-1]:.1f}" for r in rows.values()], flush=True)
    prof = {"what": "held-out greedy return_mean (crl_dqn_evaluate, the noise off, 256 envs) of the initial network and after 5,000 / 10,000 / 15,000 "
                    "/ 20,000 steps of DQN with noisy linear layers and epsilon = 0 at the reference's defaults but for lr: dqn.jl's net, and noisy + "
                    "dueling + C51 + PER + 3-step + double; mean_abs_sigma: the mean |sigma| of every parameter array at the same points; seed s sets "
                    "the training seed and the initial network (scripts/noisy_learn.py)",
            "steps": STEPS, "eval_envs": EVAL_ENVS, "lr": LR, "sigma0": 0.5, "runs": runs, "mean_abs_sigma": sigmas,
            "seeds_that_learned": {arm: sorted(int(s) for s, r in rows.items() if r[-1] > r[0]) for arm, rows in runs.items()}}
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
