#!/usr/bin/env python3
"""What a held-out evaluation costs next to a training rollout of the same shape, on one box, in one process:

    crl_ppo_evaluate, greedy, 4096 envs x 1 episode        (csrc/eval.hip: one launch, actor only, nothing stored per step)
    crl_rollout_run on a 4096-env x 128-step handle        (the training rollout kernels: actor + critic + buffer stores) — the yardstick

for CartPole 2x64 (fused path) and Acrobot 2x256 (layer-wise path). Median of five timed calls after one warm-up, wall clock around the call
plus crl_sync; env-steps/s and microseconds per sequential step (evaluation: the longest episode of the call; rollout: num_steps), with the
shader clock crl_clock_probe reports, to profiles/eval_cost.txt.

The evaluation figure is the whole call as a user pays for it, host work included: the scratch reset, the launch, the device-to-host copies of the two
4096-entry arrays, the Float64 report, and the Python shell's allocation of the result arrays. crl_rollout_run is a launch and a
sync. The output file says so.

    python scripts/eval_cost.py [--out profiles/eval_cost.txt]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cleanrl_jl_amd as crl  # noqa: E402
from cleanrl_jl_amd.ppo import env_shape  # noqa: E402

NT, K, RUNS = 4096, 128, 5


def timed(fn, sync):
    fn(); sync()                                   # warm-up (first-use allocations, code load)
    out = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        res = fn(); sync()
        out.append((time.perf_counter() - t0, res))
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "eval_cost.txt")
    L = crl._lib
    med, lo, hi = L.clock_probe(0, 5.0)
    lines = [f"shader clock under load (crl_clock_probe): median {med:.0f} MHz, min {lo:.0f}, max {hi:.0f}",
             f"{NT} envs; evaluation: greedy, 1 episode per env; rollout: {K} steps; median of {RUNS} calls after one warm-up",
             "wall clock around each call. The crl_ppo_evaluate figures include its host work (result arrays allocated, scratch reset, two device-to-host copies,",
             "the Float64 report); 'us per step' is that wall time over the longest episode of the call. crl_rollout_run is one launch and a sync.", ""]
    for env, hidden in (("cartpole", 64), ("acrobot", 256)):
        cfg = crl.PPOConfig(num_envs=NT, num_steps=K, total_timesteps=NT * K * 10)
        agent = crl.Agent(cfg, **env_shape(env, hidden=hidden))
        h = agent.handle
        h.env_reset()
        ev = timed(lambda: h.evaluate(NT, 1, L.EVAL_GREEDY, seed=1), h.sync)
        ro = timed(lambda: h.rollout_run(), h.sync)
        t_ev = statistics.median(t for t, _ in ev); rep = ev[0][1]["report"]; longest = int(ev[0][1]["lengths"].max())
        t_ro = statistics.median(t for t, _ in ro)
        ev_rate, ro_rate = rep["env_steps"] / t_ev, NT * K / t_ro
        lines += [f"{env} 2x{hidden}",
                  f"  crl_ppo_evaluate  {t_ev * 1e3:9.3f} ms  {rep['env_steps']:9d} env-steps  {ev_rate / 1e6:8.2f} M env-steps/s  "
                  f"{t_ev * 1e6 / longest:7.2f} us per step ({longest} sequential steps; mean length {rep['length_mean']:.1f}, mean return {rep['return_mean']:.1f})",
                  f"  crl_rollout_run   {t_ro * 1e3:9.3f} ms  {NT * K:9d} env-steps  {ro_rate / 1e6:8.2f} M env-steps/s  {t_ro * 1e6 / K:7.2f} us per step ({K} sequential steps)",
                  f"  evaluation / rollout, per env-step: {ro_rate / ev_rate:.2f}x the time", ""]
        agent.close()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
