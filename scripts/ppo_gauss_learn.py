#!/usr/bin/env python3
"""Does Gaussian PPO learn the on-device Pendulum within a test-sized budget? Eight seeds (env / noise key and initial weights both follow the seed) at one
shape and budget; per seed the mean episode return of the first and of the last `--tail` rollouts and a coarse curve. Rewards are unscaled and there is
no reward normalisation, so the value loss starts near 1e4 and shares ClipNorm(0.5) with the actor's gradient. Writes profiles/ppo_gauss_learn.json:
the recorded numbers, the worst seed, the seed-to-seed spread (max - min of the final returns) and `threshold` = worst - spread, the figure a
learning test may assert if `all_learned` (every seed's final return above --solved).

    python scripts/ppo_gauss_learn.py [--envs 1024 --steps 64 --updates 150 --hidden 64 --lr 1e-3 --gamma 0.9 --ent 0.0 --out profiles/ppo_gauss_learn.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import cleanrl_jl_amd as crl

ap = argparse.ArgumentParser()
for name, typ, dflt in (("envs", int, 1024), ("steps", int, 64), ("updates", int, 150), ("hidden", int, 64), ("tail", int, 10), ("lr", float, 1e-3),
                        ("gamma", float, 0.9), ("ent", float, 0.0), ("solved", float, -400.0), ("out", str, os.path.join(ROOT, "profiles", "ppo_gauss_learn.json"))):
    ap.add_argument("--" + name, type=typ, default=dflt)
a = ap.parse_args()


def config():
    """The one place the learning shape is written down: tests read it back from the json."""
    return dict(num_envs=a.envs, num_steps=a.steps, total_timesteps=a.envs * a.steps * a.updates, lr=a.lr, gamma=a.gamma, ent_coeff=a.ent,
                clip_value_loss=False)


def run(seed):
    agent = crl.Agent(crl.PPOConfig(**config()), action="gaussian", env_kind=crl._lib.ENV_PENDULUM, obs_dim=3, n_act=1, hidden=a.hidden, seed=0x5EED + seed,
                      init_seed=seed)
    h = agent.handle
    h.env_reset()
    t0 = time.perf_counter()
    rets = []
    for _ in range(a.updates):
        h.iterate(1, want_stats=False)
        ep = h.episode_stats()
        rets.append(ep["return_sum"] / ep["episodes"] if ep["episodes"] else float("nan"))
    sec = time.perf_counter() - t0
    agent.close()
    rets = np.array(rets)
    return dict(seed=seed, first=float(np.nanmean(rets[:a.tail])), final=float(np.nanmean(rets[-a.tail:])), seconds=sec,
                curve=[float(np.nanmean(rets[i:i + a.tail])) for i in range(0, a.updates, a.tail)])


runs = [run(s) for s in range(8)]
final = np.array([r["final"] for r in runs])
spread = float(final.max() - final.min())
out = dict(metric=f"mean episode return (200-step Pendulum episodes, unscaled reward) of the first / last {a.tail} rollouts of {a.updates} updates",
           config=config(), hidden=a.hidden, updates=a.updates, tail=a.tail, solved_above=a.solved, runs=runs, worst_final=float(final.min()),
           best_final=float(final.max()), spread=spread, threshold=float(final.min() - spread), all_learned=bool((final > a.solved).all()))
print(json.dumps({k: v for k, v in out.items() if k != "runs"}), [round(r["first"]) for r in runs], [round(r["final"]) for r in runs], flush=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
