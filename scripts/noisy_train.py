#!/usr/bin/env python3
"""Do noisy linear layers change what DQN learns on CartPole, and what it promises? Eight seeds, the held-out score at the four quarters, the Q bias
and the mean |sigma| per layer -> profiles/noisy_train.json. The protocol is scripts/duel_train.py's, so its rows (profiles/duel_train.json,
profiles/c51_train.json) are what these stand against; the uniform arm is run again here as the check that the files are one experiment.

Every run is the reference's default DQNConfig for `--steps` env steps — the noisy arms with epsilon_start = epsilon_end = 0, exploration by the noise
alone —; a seed sets the training env, the draws and the initial network alike for every arm. Arms: uniform (dqn.jl's net, its ε-greedy schedule),
noisy (the same net with noisy layers, ε = 0) and rainbow (noisy + dueling + C51Options() + PEROptions() + DQNTargetOptions(3, True), ε = 0: all six
components). At each quarter crl_dqn_evaluate plays the frozen greedy policy, the noise off, on 256 fresh CartPoles: return_mean and q_bias_mean (mean
of Q(s0, a) minus the discounted return: positive = the critic promises more than the policy collects). The JSON keeps every figure and the mean and
the population standard deviation over the seeds; nothing is selected.

usage: python scripts/noisy_train.py [--steps N] [--seeds 8] [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noisy_train.json"))
    args = ap.parse_args()
    import cleanrl_jl_amd as crl
    eps0 = dict(epsilon_start=0.0, epsilon_end=0.0)
    arms = {"uniform": ({}, {}), "noisy": (eps0, dict(noisy=crl.NoisyOptions())),
            "rainbow": (eps0, dict(noisy=crl.NoisyOptions(), dueling=True, per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True), dist=crl.C51Options()))}
    checkpoints = [args.steps * i // 4 for i in (1, 2, 3, 4)]
    runs = {arm: [] for arm in arms}
    for seed in range(1, args.seeds + 1):
        for arm, (ckw, kw) in arms.items():
            agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=args.steps, **ckw), seed=seed, init_seed=seed, **kw)
            rec, done = {"seed": seed, "return_mean": [], "q_bias_mean": []}, 0
            if agent.noisy is not None:
                rec["mean_abs_sigma"] = []
            for c in checkpoints:
                taken, _, _ = agent.handle.run(c - done)
                done += taken
                rep = crl.dqn_evaluate(agent, num_envs=args.eval_envs)["report"]
                rec["return_mean"].append(rep["return_mean"]); rec["q_bias_mean"].append(rep["q_bias_mean"])
                if agent.noisy is not None:
                    rec["mean_abs_sigma"].append(crl.noisy_sigma(agent))
            assert done == args.steps
            runs[arm].append(rec)
            agent.close()
            print(arm, {k: v for k, v in rec.items() if k != "mean_abs_sigma"}, flush=True)
    summary = {arm: {f: {"mean": [statistics.fmean(r[f][i] for r in rs) for i in range(4)],
                         "std": [statistics.pstdev(r[f][i] for r in rs) for i in range(4)]} for f in ("return_mean", "q_bias_mean")}
               for arm, rs in runs.items()}
    for arm in ("noisy", "rainbow"):
        n_arr = len(runs[arm][0]["mean_abs_sigma"][0])
        summary[arm]["mean_abs_sigma"] = {"mean": [[statistics.fmean(r["mean_abs_sigma"][i][a] for r in runs[arm]) for a in range(n_arr)] for i in range(4)]}
    higher = {arm: {f: [sum(a[f][i] > u[f][i] for a, u in zip(runs[arm], runs["uniform"])) for i in range(4)] for f in ("return_mean", "q_bias_mean")}
              for arm in arms if arm != "uniform"}
    prof = {"what": "DQN on CartPole at the reference defaults: dqn.jl's net with its epsilon-greedy schedule, the same net with noisy layers and "
                    "epsilon = 0, and noisy + dueling + C51 + PER + 3-step + double with epsilon = 0 (Rainbow); held-out greedy evaluation "
                    "(crl_dqn_evaluate, the noise off) at four checkpoints; mean_abs_sigma: per parameter array, in array order (scripts/noisy_train.py)",
            "steps": args.steps, "checkpoints": checkpoints, "eval_envs": args.eval_envs, "seeds": list(range(1, args.seeds + 1)), "sigma0": 0.5,
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
