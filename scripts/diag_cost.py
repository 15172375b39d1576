#!/usr/bin/env python3
"""What one crl_ppo_diagnose costs next to a training iteration of the same shape, on one box:

    65536 envs x 128 steps, obs 4 / act 2 / 2x64 (CartPole, the headline shape of bench.py)
    16384 envs x 128 steps, obs 8 / act 4 / 2x256 (synthetic env, bench.py --workload c3)

Diagnosis: per-sample outputs NULL, HIP events around the launch (read-only option diag_last_ns), one warm-up call, median of five, on a handle that
has just run two training iterations. The comparison point is bench.py's own result line of the same box and run: ms_per_step is its iteration time,
kernel_ms_per_step["update"] the update kernels' HIP-event time per iteration, of which an update epoch is 1 / update_epochs. Written with the shader
clock crl_clock_probe reports to profiles/diag_cost.txt.

    python bench.py --gpus 1 --steps 10 --warmup 3 --no-extras --no-cpu-baseline > headline.json
    python bench.py --gpus 1 --steps 10 --warmup 3 --no-extras --no-cpu-baseline --workload c3 > c3.json
    python scripts/diag_cost.py --bench headline.json c3.json [--out profiles/diag_cost.txt]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cleanrl_jl_amd as crl  # noqa: E402

SHAPES = [("65536 x 128, 4 / 2 / 2x64, CartPole", dict(num_envs=65536), dict()),
          ("16384 x 128, 8 / 4 / 2x256, synthetic", dict(num_envs=16384), dict(obs_dim=8, n_act=4, hidden=256, env_kind=crl._lib.ENV_SYNTHETIC))]
RUNS = 5


def bench_line(path):
    for line in reversed(open(path).read().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise SystemExit(f"{path}: no JSON result line")


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "diag_cost.txt")
    if "--bench" not in sys.argv:
        raise SystemExit(__doc__)
    i = sys.argv.index("--bench")
    benches = [bench_line(p) for p in sys.argv[i + 1:i + 3]]
    med, lo, hi = crl._lib.clock_probe(0)
    lines = [f"crl_ppo_diagnose next to bench.py's iteration of the same box and run; shader clock under load {med:.0f} MHz (min {lo:.0f}, max {hi:.0f})",
             f"diagnosis: HIP events around the launch, per-sample outputs NULL, median of {RUNS} after one warm-up", ""]
    for (label, ckw, shape), b in zip(SHAPES, benches):
        cfg = crl.PPOConfig(num_steps=128, total_timesteps=10 ** 12, **ckw)
        agent = crl.Agent(cfg, **shape)
        h = agent.handle
        h.env_reset()
        h.iterate(2, want_stats=False); h.sync()
        h.diagnose()
        ds = []
        for _ in range(RUNS):
            rep = h.diagnose(); ds.append(h.get_option("diag_last_ns") * 1e-6)
        d = statistics.median(ds)
        it, upd = b["ms_per_step"], b["kernel_ms_per_step"]["update"]
        epoch = upd / cfg.update_epochs
        verdict = "less than one update epoch" if d < epoch else "MORE than one update epoch: the expectation is not met"
        lines += [f"{label}",
                  f"  bench.py iteration   {it:9.3f} ms, of which update kernels {upd:.3f} ms = {epoch:.3f} ms per update epoch",
                  f"  crl_ppo_diagnose     {d:9.3f} ms per launch: {verdict} ({d / it * 100:.1f} % of an iteration; {cfg.num_envs * 128 / d / 1e6:.2f} G samples/s)",
                  f"  report: approx_kl {rep['approx_kl']:.3e} clipfrac {rep['clipfrac']:.4f} entropy {rep['entropy']:.4f} explained_variance {rep['explained_variance']:.4f}", ""]
        agent.close()
    text = "\n".join(lines)
    print(text)
    with open(out_path, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
