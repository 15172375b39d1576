#!/usr/bin/env python3
"""What the quantile-regression (QR-DQN) critic costs per DQN cycle on the GPU, next to the categorical one, and whether the plain handle kept its
speed -> profiles/qr_bench.json.

Arms, at the reference defaults (ring 10 000, batch 120, an update every 10 steps): plain (crl_dqn_create), c51 (C51Options(): N = 51), qr
(QROptions(): N = 51, kappa = 1), duel_qr (dueling + QR) and everything (noisy + dueling + QR + PER + 3-step + double). Each arm runs in a fresh
process of its own (`--child-arm NAME`): a warm-up, then `--repeats` windows of `--steps` env steps, a host clock around crl_dqn_run, which ends in a
stream synchronise; us per cycle = window time / (steps / train_freq). All processes of one invocation run on one box, one after the other: compare
within a file only.

The TD launch and the collect launch on their own come from `rocprofv3 --kernel-trace --stats`, in a run of its own (`--trace-run` plays the c51, qr
and everything arms); `--kernel-stats FILE` folds that run's kernel statistics (CSV) into the JSON (scripts/bench_dqn_per.py's reader).

The plain handle against the parent commit: `--parent LIB` as scripts/bench_c51.py — scripts/bench_dqn_target.py's child, bare ctypes calls the
parent's library has too, one fresh child per library and round, alternating.

usage: python scripts/bench_qr.py [--steps N] [--repeats R] [--rounds K] [--parent LIB] [--kernel-stats CSV] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_qr.py --trace-run"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_c51 as BC           # noqa: E402
import bench_dqn_per as BP       # noqa: E402
import bench_dqn_target as BT    # noqa: E402

ARMS = ("plain", "c51", "qr", "duel_qr", "everything")


def _agent(crl, cfg, arm):
    kw = {"plain": {}, "c51": dict(dist=crl.C51Options()), "qr": dict(dist=crl.QROptions()), "duel_qr": dict(dist=crl.QROptions(), dueling=True),
          "everything": dict(dist=crl.QROptions(), dueling=True, noisy=crl.NoisyOptions(), per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True))}[arm]
    return crl.DQNAgent(cfg, seed=1, **kw)


def child_arm(arm, steps, repeats):
    import cleanrl_jl_amd as crl
    cfg = crl.DQNConfig(total_timesteps=steps * (repeats + 2))
    agent = _agent(crl, cfg, arm)
    clock0 = crl._lib.clock_probe(0)
    agent.handle.run(steps)                                       # warm-up: code objects, the ring past min_buff_size, every kernel of the cycle
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        taken, _, _ = agent.handle.run(steps)
        times.append(time.perf_counter() - t0)
        assert taken == steps
    out = BT._window_stats(times, steps / cfg.train_freq)
    out["shader_clock_mhz_median"] = {"before": clock0[0], "after": crl._lib.clock_probe(0)[0]}
    print("RESULT " + json.dumps(out))


def trace_run(steps):
    import cleanrl_jl_amd as crl
    cfg = crl.DQNConfig(total_timesteps=2 * steps)
    for arm in ("c51", "qr", "everything"):
        _agent(crl, cfg, arm).handle.run(2 * steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--parent", default=None, help="the parent commit's libcleanrl_hip.so")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qr_bench.json"))
    ap.add_argument("--child-arm", default=None)
    ap.add_argument("--trace-run", action="store_true")
    args = ap.parse_args()
    if args.child_arm:
        return child_arm(args.child_arm, args.steps, args.repeats)
    if args.trace_run:
        return trace_run(args.steps)
    size = ["--steps", str(args.steps), "--repeats", str(args.repeats)]
    arms = {arm: BC._child(os.path.abspath(__file__), ["--child-arm", arm] + size) for arm in ARMS}
    base = arms["plain"]["us_per_cycle_median"]
    for k, v in arms.items():
        v["over_plain_percent"] = 100.0 * (v["us_per_cycle_median"] - base) / base
        print(f"{k:12s} {v['us_per_cycle_median']:.2f} us/cycle ({v['over_plain_percent']:+.1f} %)", flush=True)
    prof = {"what": "us per DQN cycle (ten launches; eleven with noisy layers) at the reference defaults: the scalar critic, C51 at N = 51, QR-DQN at "
                    "N = 51 and kappa = 1, dueling + QR, and noisy + dueling + QR + PER + 3-step + double, one fresh process per arm, one after the "
                    "other on one box; the kernels on their own from a rocprofv3 run of its own; the plain handle of this tree against the parent "
                    "commit's library, alternating child processes (scripts/bench_qr.py). One box, one run: compare within this file only.",
            "steps_per_window": args.steps, "windows": args.repeats, "arms": arms}
    if args.kernel_stats:
        prof["kernels"] = BP.kernel_stats(args.kernel_stats)
    if args.parent:
        from cleanrl_jl_amd import _lib as L
        libs = {"parent": os.path.abspath(args.parent), "tree": os.path.abspath(L.LIB_PATH)}
        rounds = {k: [] for k in libs}
        for _ in range(args.rounds):
            for k, path in libs.items():
                rounds[k].append(BC._child(os.path.abspath(BT.__file__), ["--child-plain", path] + size)["us_per_cycle_median"])
        lo, hi, med = min(rounds["parent"]), max(rounds["parent"]), statistics.median(rounds["tree"])
        prof["plain_handle_vs_parent"] = {"rounds": args.rounds, "us_per_cycle_per_round": rounds, "parent_median": statistics.median(rounds["parent"]),
                                          "parent_min": lo, "parent_max": hi, "tree_median": med, "tree_min": min(rounds["tree"]),
                                          "tree_max": max(rounds["tree"]), "tree_median_inside_parent_spread": lo <= med <= hi}
        print("plain handle, us/cycle per round:", {k: [round(x, 2) for x in v] for k, v in rounds.items()},
              "tree median inside the parent's spread:", lo <= med <= hi)
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
