#!/usr/bin/env python3
"""Do dueling heads change what DQN learns on CartPole, and what it promises? Eight seeds, the held-out score at the four quarters and the Q bias ->
profiles/duel_train.json. The protocol is scripts/c51_train.py's, so its rows (uniform, c51, c51_per_n3_double in profiles/c51_train.json) are what
these stand against; the uniform arm is run again here as the check that the two files are one experiment.

Every run is the reference's default DQNConfig for `--steps` env steps; a seed sets the training env, the exploration, the draws and the initial
network alike for every arm. Arms: uniform (dqn.jl's net), duel (the scalar dueling head), duel_c51 (dueling + C51Options()) and
duel_c51_per_n3_double (with PEROptions() and DQNTargetOptions(3, True) as well). At each quarter crl_dqn_evaluate plays the frozen greedy policy on
256 fresh CartPoles: return_mean and q_bias_mean (mean of Q(s0, a) minus the discounted return: positive = the critic promises more than the policy
collects). The JSON keeps every figure and the mean and the population standard deviation over the seeds; nothing is selected.

usage: python scripts/duel_train.py [--steps N] [--seeds 8] [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duel_train.json"))
    args = ap.parse_args()
    import cleanrl_jl_amd as crl
    full = dict(per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True), dist=crl.C51Options())
    arms = {"uniform": {}, "duel": dict(dueling=True), "duel_c51": dict(dueling=True, dist=crl.C51Options()),
            "duel_c51_per_n3_double": dict(dueling=True, **full)}
    checkpoints = [args.steps * i // 4 for i in (1, 2, 3, 4)]
    runs = {arm: [] for arm in arms}
    for seed in range(1, args.seeds + 1):
        for arm, kw in arms.items():
            agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=args.steps), seed=seed, init_seed=seed, **kw)
            rec, done = {"seed": seed, "return_mean": [], "q_bias_mean": []}, 0
            for c in checkpoints:
                taken, _, _ = agent.handle.run(c - done)
                done += taken
                rep = crl.dqn_evaluate(agent, num_envs=args.eval_envs)["report"]
                rec["return_mean"].append(rep["return_mean"]); rec["q_bias_mean"].append(rep["q_bias_mean"])
            assert done == args.steps
            runs[arm].append(rec)
            agent.close()
            print(arm, rec, flush=True)
    summary = {arm: {f: {"mean": [statistics.fmean(r[f][i] for r in rs) for i in range(4)],
                         "std": [statistics.pstdev(r[f][i] for r in rs) for i in range(4)]} for f in ("return_mean", "q_bias_mean")}
               for arm, rs in runs.items()}
    higher = {arm: {f: [sum(a[f][i] > u[f][i] for a, u in zip(runs[arm], runs["uniform"])) for i in range(4)] for f in ("return_mean", "q_bias_mean")}
              for arm in arms if arm != "uniform"}
    prof = {"what": "DQN on CartPole at the reference defaults: dqn.jl's net with uniform replay, the scalar dueling head, dueling + C51, and dueling "
                    "+ C51 + PER + 3-step + double; held-out greedy evaluation (crl_dqn_evaluate) at four checkpoints (scripts/duel_train.py)",
            "steps": args.steps, "checkpoints": checkpoints, "eval_envs": args.eval_envs, "seeds": list(range(1, args.seeds + 1)),
            "runs": runs, "summary": summary, "seeds_where_the_arm_is_higher_than_uniform": higher}
    published = os.path.join(ROOT, "profiles", "c51_train.json")
    if os.path.exists(published) and args.steps == 50_000 and args.seeds == 8:
        old = json.load(open(published))
        prof["uniform_arm_equals_profiles_c51_train"] = old["runs"]["uniform"] == runs["uniform"]
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    for arm in runs:
        print(arm, "return_mean", [round(x, 1) for x in summary[arm]["return_mean"]["mean"]], "q_bias_mean",
              [round(x, 2) for x in summary[arm]["q_bias_mean"]["mean"]])
    return 0


if __name__ == "__main__":
    sys.exit(main())
