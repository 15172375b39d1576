#!/usr/bin/env python3
"""Does a 20,000-step QR-DQN run learn CartPole? -> profiles/qr_learn.json, what tests/test_gpu_qr.py's learning test is built on (as
profiles/noisy_learn.json is for the noisy layers').

Eight seeds, the reference's DQNConfig at lr = 1e-3 (the rate of every DQN parity test here and of test_per_agent_learns, whose docstring says why
not the default 1e-4). Two heads: qr (QROptions(): N = 51, kappa = 1) and everything (QR + dueling + noisy layers + PEROptions() +
DQNTargetOptions(3, True)), both on dqn.jl's ε-greedy schedule (`everything_eps0` explores by the noise alone, the NoisyNet setting), each at two target-copy periods: target_net_freq = 1000 steps (100 updates between hard
copies; arms `qr`, `everything`) and dqn.jl's default of 100 steps (10 updates; arms `qr_default`, `everything_default`). Why two: a quantile at
τ close to 1 regresses onto the top of a bootstrapped target with weight τ upwards against 1 − τ downwards, a max-like operator whose overestimation
only a lagging target damps — the QR-DQN paper copies every 10,000 frames = 2,500 updates — and ten updates between copies is next to no target
network. crl_dqn_evaluate of the initial network and after every 5,000 steps, 256 fresh CartPoles each. Nothing is selected: a seed or an arm that
does not learn is in the file. margin[arm] = half the smallest gain (last − initial) over the eight seeds, which every recorded seed therefore
clears when that gain is positive.

usage: python scripts/qr_learn.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS, SEEDS, EVAL_ENVS, LR, TARGET_NET_FREQ = 20_000, 8, 256, 1e-3, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qr_learn.json"))
    args = ap.parse_args()
    import cleanrl_jl_amd as crl
    every = dict(dist=crl.QROptions(), dueling=True, noisy=crl.NoisyOptions(), per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True))
    arms = {"qr": (dict(dist=crl.QROptions()), dict(target_net_freq=TARGET_NET_FREQ)),
            "everything": (every, dict(target_net_freq=TARGET_NET_FREQ)),
            "everything_eps0": (every, dict(epsilon_start=0.0, epsilon_end=0.0, target_net_freq=TARGET_NET_FREQ)),
            "qr_default": (dict(dist=crl.QROptions()), {}), "everything_default": (every, {})}
    runs = {}
    for arm, (kw, ckw) in arms.items():
        rows = {}
        for seed in range(1, SEEDS + 1):
            agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=STEPS, lr=LR, **ckw), seed=seed, init_seed=seed, **kw)
            ret = [crl.dqn_evaluate(agent, num_envs=EVAL_ENVS)["report"]["return_mean"]]
            for _ in range(4):
                agent.handle.run(STEPS // 4)
                ret.append(crl.dqn_evaluate(agent, num_envs=EVAL_ENVS)["report"]["return_mean"])
            agent.close()
            rows[str(seed)] = ret
        runs[arm] = rows
        print(f"{arm:18s} initial -> 20,000 steps:", [f"{r[0]:.1f}->{r[-1]:.1f}" for r in rows.values()], flush=True)
    prof = {"what": "held-out greedy return_mean (crl_dqn_evaluate, 256 envs; the noise off on the noisy arm) of the initial network and after 5,000 / "
                    "10,000 / 15,000 / 20,000 steps of QR-DQN (N = 51, kappa = 1) at the reference's defaults but for lr: the quantile critic alone, "
                    "and with dueling + noisy layers + PER + 3-step + double, on dqn.jl's epsilon schedule (everything_eps0: epsilon = 0), each with a hard target copy every 1,000 steps (qr, "
                    "everything) and every 100 steps, dqn.jl's default (qr_default, everything_default); seed s sets the training seed and the "
                    "initial network; margin = half the smallest last − initial over the eight seeds (scripts/qr_learn.py)",
            "steps": STEPS, "eval_envs": EVAL_ENVS, "lr": LR, "target_net_freq": {"qr": TARGET_NET_FREQ, "everything": TARGET_NET_FREQ,
                                                                             "everything_eps0": TARGET_NET_FREQ, "qr_default": 100, "everything_default": 100}, "runs": runs,
            "margin": {arm: 0.5 * min(r[-1] - r[0] for r in rows.values()) for arm, rows in runs.items()},
            "seeds_that_learned": {arm: sorted(int(s) for s, r in rows.items() if r[-1] > r[0]) for arm, rows in runs.items()}}
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
