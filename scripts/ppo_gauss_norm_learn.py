#!/usr/bin/env python3
"""Does running observation / reward normalisation (crl.NormalizedEnv) make Gaussian PPO learn the Pendulum? Eight seeds through the device-resident
path (train_external's loop on LibraryEnv("pendulum")), wrapped and unwrapped, at the shape and budget of profiles/ppo_gauss_learn.json. Reports RAW
episode returns — the wrapped arm's come from the normaliser's own books — as the mean of the first and of the last `--tail` rollouts per seed and a
coarse curve, whichever way it goes. Writes profiles/ppo_gauss_norm_learn.json.

    python scripts/ppo_gauss_norm_learn.py [--envs 1024 --steps 64 --updates 150 --hidden 64 --lr 1e-3 --gamma 0.9 --seeds 8]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import cleanrl_jl_amd as crl

ap = argparse.ArgumentParser()
for name, typ, dflt in (("envs", int, 1024), ("steps", int, 64), ("updates", int, 150), ("hidden", int, 64), ("tail", int, 10), ("lr", float, 1e-3),
                        ("gamma", float, 0.9), ("ent", float, 0.0), ("seeds", int, 8), ("first_seed", int, 0),
                        ("out", str, os.path.join(ROOT, "profiles", "ppo_gauss_norm_learn.json"))):
    ap.add_argument("--" + name, type=typ, default=dflt)
a = ap.parse_args()
L = crl._lib


def config():
    return dict(num_envs=a.envs, num_steps=a.steps, total_timesteps=a.envs * a.steps * a.updates, lr=a.lr, gamma=a.gamma, ent_coeff=a.ent,
                clip_value_loss=False)


def run(seed, wrapped):
    cfg = crl.PPOConfig(**config())
    agent = crl.Agent(cfg, action="gaussian", env_kind=L.ENV_EXTERNAL, obs_dim=3, n_act=1, hidden=a.hidden, seed=0x5EED + seed, init_seed=seed)
    env = crl.LibraryEnv("pendulum", a.envs, seed=0x5EED + seed)
    if wrapped:
        env = crl.NormalizedEnv(env, gamma=a.gamma)
    h, action = agent.handle, L.DeviceBuffer(4 * a.envs)
    stats = env.episode_stats if wrapped else h.episode_stats
    t0 = time.perf_counter()
    rets = []
    obs, done = env.reset()
    for _ in range(a.updates):                                   # train_external's loop, the rollout's raw returns kept
        for s in range(a.steps):
            h.act_device_gaussian(s, obs, done, action, peer_stream=env.stream)
            reward, obs, done = env.step(action)
            h.record_device_gaussian(s, reward, obs, done, peer_stream=env.stream)
        ep = stats()
        h.update(want_stats=False)
        rets.append(ep["return_sum"] / ep["episodes"] if ep["episodes"] else float("nan"))
    sec = time.perf_counter() - t0
    env.close(); agent.close()
    rets = np.array(rets)
    return dict(seed=seed, first=float(np.nanmean(rets[:a.tail])), final=float(np.nanmean(rets[-a.tail:])), seconds=sec,
                curve=[float(np.nanmean(rets[i:i + a.tail])) for i in range(0, a.updates, a.tail)])


out = dict(metric=f"mean RAW episode return (200-step Pendulum episodes) of the first / last {a.tail} rollouts of {a.updates} updates, device-resident path",
           config=config(), hidden=a.hidden, updates=a.updates, tail=a.tail, arms={})
for name, wrapped in (("unwrapped", False), ("wrapped", True)):
    runs = [run(s, wrapped) for s in range(a.first_seed, a.first_seed + a.seeds)]
    final = np.array([r["final"] for r in runs])
    out["arms"][name] = dict(runs=runs, worst_final=float(final.min()), best_final=float(final.max()), mean_final=float(final.mean()))
    print(name, [round(r["first"]) for r in runs], [round(r["final"]) for r in runs], f"{sum(r['seconds'] for r in runs):.0f} s", flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:                                  # written after every arm: a run cut short keeps what it measured
        json.dump(out, f, indent=1)
        f.write("\n")
