#!/usr/bin/env python3
"""Does prioritized replay help on CartPole? Eight seeds, uniform against PER, the held-out score at four checkpoints -> profiles/dqn_per_train.json.

Every run is the reference's default DQNConfig for `--steps` env steps; a seed sets the training env, the exploration, the draws and the initial
network alike for the two arms. At each quarter of the run crl_dqn_evaluate plays the frozen greedy policy on 256 fresh CartPoles: return_mean and
q_bias_mean (mean of max_a Q(s0, a) minus the discounted return: positive = q_net promises more than the policy collects). The JSON keeps every
figure and the mean and the population standard deviation over the seeds; nothing is selected.

usage: python scripts/dqn_per_train.py [--steps N] [--seeds 8] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50_000)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--eval_envs", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_per_train.json"))
    args = ap.parse_args()
    import cleanrl_jl_amd as crl
    checkpoints = [args.steps * i // 4 for i in (1, 2, 3, 4)]
    runs = {"uniform": [], "per": []}
    for seed in range(1, args.seeds + 1):
        for arm in runs:
            cfg = crl.DQNConfig(total_timesteps=args.steps)
            agent = crl.DQNAgent(cfg, seed=seed, init_seed=seed, per=crl.PEROptions() if arm == "per" else None)
            rec, done = {"seed": seed, "return_mean": [], "q_bias_mean": []}, 0
            for c in checkpoints:
                taken, _, _ = agent.handle.run(c - done)
                done += taken
                rep = crl.dqn_evaluate(agent, num_envs=args.eval_envs)["report"]
                rec["return_mean"].append(rep["return_mean"]); rec["q_bias_mean"].append(rep["q_bias_mean"])
            assert done == args.steps
            runs[arm].append(rec)
            agent.close()
            print(arm, rec)
    summary = {arm: {f: {"mean": [statistics.fmean(r[f][i] for r in rs) for i in range(4)],
                         "std": [statistics.pstdev(r[f][i] for r in rs) for i in range(4)]} for f in ("return_mean", "q_bias_mean")}
               for arm, rs in runs.items()}
    wins = [sum(p["return_mean"][i] > u["return_mean"][i] for p, u in zip(runs["per"], runs["uniform"])) for i in range(4)]
    prof = {"what": "DQN on CartPole at the reference defaults, uniform against prioritized replay (PEROptions defaults), held-out greedy evaluation "
                    "(crl_dqn_evaluate) at four checkpoints (scripts/dqn_per_train.py)",
            "steps": args.steps, "checkpoints": checkpoints, "eval_envs": args.eval_envs, "seeds": list(range(1, args.seeds + 1)),
            "runs": runs, "summary": summary, "seeds_where_per_scores_higher": wins}
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    for arm in runs:
        print(arm, "return_mean", [round(x, 1) for x in summary[arm]["return_mean"]["mean"]], "q_bias_mean",
              [round(x, 2) for x in summary[arm]["q_bias_mean"]["mean"]])
    return 0


if __name__ == "__main__":
    sys.exit(main())
