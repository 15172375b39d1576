#!/usr/bin/env python3
"""Gaussian PPO beside the softmax handle of the nearest shape, same box and same run: ms per iteration (rollout + GAE + 16 optimiser steps) of
Pendulum (obs 3, act_dim 1) and MountainCar (obs 2, 3 actions) at 16384 envs x 128 steps, 2x256 and 2x64; the rollout's share (CRL_K_ROLLOUT) and
the loss launch's own time (CRL_K_LOSS: wide_loss_gauss_kernel against wide_loss_kernel) from a profiled pass of their own. Both handles
take a one-launch rollout at 2x256 by default and roll out per step (three launches a step) at 2x64, so the softmax handle is also timed with
wide_rollout_persist = 0, the per-step route, which is the like-for-like row. Writes profiles/ppo_gauss_bench.json with the box's shader clock.

    python scripts/bench_ppo_gauss.py [iterations]

The rollout alone, 2x256 — the Gaussian handle's one-launch route (wide_rs_rollout_gauss_kernel) against the same handle per step and against the softmax
handle's one-launch rollout, arms alternating inside one process for `rounds` rounds; then, for every name=library given, the same arms in alternating
child processes (CRL_LIB_PATH), this build against that one: the other tail split of the Gaussian kernel, or the parent commit's softmax rollout.
Writes profiles/ppo_gauss_rollout_bench.json.

    python scripts/bench_ppo_gauss.py rollout [rounds] [name=path/to/libcleanrl_hip.so ...]"""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import cleanrl_jl_amd as crl

L = crl._lib
NT, K, WARM = 16384, 128, 2
REPS = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 7
CASES = {"gaussian_pendulum": (dict(action="gaussian", env_kind=L.ENV_PENDULUM, obs_dim=3, n_act=1), {}, "default: one launch at 2x256, per-step at 2x64"),
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


ARMS = {"gaussian_pendulum": (dict(action="gaussian", env_kind=L.ENV_PENDULUM, obs_dim=3, n_act=1), {}),
        "gaussian_pendulum_per_step": (dict(action="gaussian", env_kind=L.ENV_PENDULUM, obs_dim=3, n_act=1), {"wide_rollout_persist": 0}),
        "softmax_mountaincar": (dict(env_kind=L.ENV_MOUNTAINCAR, obs_dim=2, n_act=3), {}),
        "gaussian_synthetic_act4": (dict(action="gaussian", env_kind=L.ENV_SYNTHETIC, obs_dim=16, n_act=4), {})}


def rollout_rounds(names, rounds):
    """per arm and round: CRL_K_ROLLOUT of two iterations (events on the stream) and the host-clock time of one unprofiled iteration"""
    cfg = crl.PPOConfig(num_envs=NT, num_steps=K, total_timesteps=NT * K * 1000)
    agents = {n: crl.Agent(cfg, hidden=256, options=ARMS[n][1], **ARMS[n][0]) for n in names}
    rows = {n: dict(rollout_route=a.handle.rollout_route(), rollout_ms=[], iteration_ms=[]) for n, a in agents.items()}
    for a in agents.values():
        a.handle.env_reset(); a.handle.iterate(WARM, want_stats=False); a.handle.sync()
    for _ in range(rounds):
        for n, a in agents.items():
            h = a.handle
            t0 = time.perf_counter(); h.iterate(1, want_stats=False); h.sync(); rows[n]["iteration_ms"].append(1e3 * (time.perf_counter() - t0))
            h.prof_enable(1); h.prof_reset(); h.iterate(2, want_stats=False); h.sync()
            ms, cnt = h.prof_read()["rollout"]; h.prof_enable(0)
            rows[n]["rollout_ms"].append(ms / max(cnt, 1))
    for a in agents.values():
        a.close()
    return rows


def spread(v):
    return dict(median=float(np.median(v)), min=min(v), max=max(v))


if sys.argv[1:2] == ["rollout-child"]:      # one child process of the mode below: one round of the named arms, one JSON line
    print(json.dumps(rollout_rounds(sys.argv[2:], 1)))
    sys.exit(0)
if sys.argv[1:2] == ["rollout"]:
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 6
    libs = dict(a.split("=", 1) for a in sys.argv[2:] if "=" in a)
    alt = None
    if libs:     # first, while this process has not touched the GPU yet
        child_arms = ["gaussian_pendulum", "gaussian_synthetic_act4", "softmax_mountaincar"]
        libs = {"this_build": os.environ.get("CRL_LIB_PATH", "")} | libs
        got = {name: {n: [] for n in child_arms} for name in libs}
        for _ in range(rounds):
            for name, path in libs.items():
                env = dict(os.environ); env.pop("CRL_LIB_PATH", None)
                if path: env["CRL_LIB_PATH"] = os.path.abspath(path)
                r = json.loads(subprocess.run([sys.executable, __file__, "rollout-child"] + child_arms, env=env, check=True, timeout=300,
                                              capture_output=True, text=True).stdout.strip().splitlines()[-1])
                for n in child_arms: got[name][n] += r[n]["rollout_ms"]
        alt = {name: {n: spread(v) | {"us_per_step": 1e3 * float(np.median(v)) / K} for n, v in arms.items()} for name, arms in got.items()}
    clock = L.clock_probe(0)
    rows = rollout_rounds(list(ARMS), rounds)
    out = {"metric": f"ms per rollout (CRL_K_ROLLOUT: the env loop and the batched critic forward behind it) and per whole PPO iteration, {NT} envs x {K} "
                     f"steps, 2x256; {rounds} rounds, arms alternating in one process; us_per_step = rollout median / {K}",
           "arms": {n: dict(rollout_route=r["rollout_route"], rollout_ms=spread(r["rollout_ms"]), us_per_step=1e3 * float(np.median(r["rollout_ms"])) / K,
                            iteration_ms=spread(r["iteration_ms"])) for n, r in rows.items()}}
    if alt: out["alternating_processes"] = alt
    out["shader_clock_mhz"] = {"median": clock[0], "min": clock[1], "max": clock[2]}
    print(json.dumps(out), flush=True)
    with open(os.path.join(ROOT, "profiles", "ppo_gauss_rollout_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(0)

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
