#!/usr/bin/env python3
"""Gaussian PPO beside the softmax handle of the nearest shape, same box and same run: ms per iteration (rollout + GAE + 16 optimiser steps) of
Pendulum (obs 3, act_dim 1) and MountainCar (obs 2, 3 actions) at 16384 envs x 128 steps, 2x256 and 2x64; the rollout's share (CRL_K_ROLLOUT) and
the loss launch's own time (CRL_K_LOSS: wide_loss_gauss_kernel against wide_loss_kernel) from a profiled pass of their own. A Gaussian handle rolls
out per step (three launches a step); the softmax handle at 2x256 takes a one-launch rollout by default, so it is also timed with
wide_rollout_persist = 0, the per-step route, which is the like-for-like row. Writes profiles/ppo_gauss_bench.json with the box's shader clock.

    python scripts/bench_ppo_gauss.py [iterations]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import cleanrl_jl_amd as crl

L = crl._lib
NT, K, WARM = 16384, 128, 2
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
CASES = {"gaussian_pendulum": (dict(action="gaussian", env_kind=L.ENV_PENDULUM, obs_dim=3, n_act=1), {}, "per-step (wide_step_kernel, Gaussian head)"),
         "softmax_mountaincar": (dict(env_kind=L.ENV_MOUNTAINCAR, obs_dim=2, n_act=3), {}, "default: one launch at 2x256, per-step at 2x64"),
         "softmax_mountaincar_per_step": (dict(env_kind=L.ENV_MOUNTAINCAR, obs_dim=2, n_act=3), {"wide_rollout_persist": 0}, "per-step (wide_step_kernel)")}


def measure(hidden, shape, options):
    cfg = crl.PPOConfig(num_envs=NT, num_steps=K, total_timesteps=NT * K * 1000)
    agent = crl.Agent(cfg, hidden=hidden, options=options, **shape)
    h = agent.handle
    h.env_reset()
    h.iterate(WARM, want_stats=False); h.sync()
    it = []
    for _ in range(REPS):
        t0 = time.perf_counter(); h.iterate(1, want_stats=False); h.sync(); it.append(1e3 * (time.perf_counter() - t0))
    h.prof_enable(1); h.prof_reset()
    h.iterate(2, want_stats=False); h.sync()
    prof = h.prof_read(); h.prof_enable(0)
    agent.close()
    loss_ms, loss_n = prof["loss"]
    return dict(iteration_ms=dict(median=float(np.median(it)), min=min(it), max=max(it)), steps_per_s=NT * K / (np.median(it) * 1e-3),
                rollout_ms=prof["rollout"][0] / max(prof["rollout"][1], 1), loss_launch_us=1e3 * loss_ms / max(loss_n, 1), loss_launches=loss_n,
                samples_per_loss_launch=NT * K // cfg.num_minibatches)


clock = L.clock_probe(0)
out = {"metric": f"ms per PPO iteration, {NT} envs x {K} steps, 4 minibatches x 4 epochs; rollout_ms and loss_launch_us from a profiled pass (events on "
                 "the stream around the launches), not part of iteration_ms", "shapes": {}}
for hidden in (256, 64):
    rows = {name: measure(hidden, shape, opts) | {"rollout_route": route} for name, (shape, opts, route) in CASES.items()}
    g, d, ds = (rows[n] for n in CASES)
    rows["ratio"] = dict(iteration_gaussian_over_softmax=g["iteration_ms"]["median"] / d["iteration_ms"]["median"],
                         iteration_gaussian_over_softmax_per_step=g["iteration_ms"]["median"] / ds["iteration_ms"]["median"],
                         loss_launch_gaussian_over_softmax=g["loss_launch_us"] / d["loss_launch_us"])
    out["shapes"][f"2x{hidden}"] = rows
    print(f"2x{hidden}", json.dumps(rows), flush=True)
out["shader_clock_mhz"] = {"median": clock[0], "min": clock[1], "max": clock[2]}
with open(os.path.join(ROOT, "profiles", "ppo_gauss_bench.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
