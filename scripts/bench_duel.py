#!/usr/bin/env python3
"""What dueling heads cost per DQN cycle on the GPU, and whether the plain handle kept its speed -> profiles/duel_bench.json. scripts/bench_c51.py's
protocol with more arms.

Arms, at the reference defaults (ring 10 000, batch 120, an update every 10 steps): plain (crl_dqn_create), duel (the scalar dueling head), c51
(C51Options(): N = 51), duel_c51 and duel_c51_per_n3_double (with PEROptions() and DQNTargetOptions(3, True)). They run alternately in one process: a
warm-up, then `--repeats` windows of `--steps` env steps each, a host clock around crl_dqn_run, which ends in a stream synchronise. us per cycle =
window time / (steps / train_freq); the median and the spread over the windows are kept, with the shader clock under load (crl_clock_probe) before and
after.

The kernels on their own (the collect launch and the TD launch among them, per launch) come from `rocprofv3 --kernel-trace --stats`, in a run of its
own (`--trace-run` plays the duel and the duel_c51_per_n3_double arms); `--kernel-stats FILE` folds that run's kernel statistics (CSV) into the JSON.

The plain handle against the parent commit: `--parent LIB` as scripts/bench_c51.py — bare ctypes calls that the parent's library has too, one fresh
child per library and round, alternating, on one box in one run.

usage: python scripts/bench_duel.py [--steps N] [--repeats R] [--rounds K] [--parent LIB] [--kernel-stats CSV] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_duel.py --trace-run"""
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


def _agents(total, only=None):
    import cleanrl_jl_amd as crl
    cfg = crl.DQNConfig(total_timesteps=total)
    full = dict(per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True), dist=crl.C51Options())
    kinds = {"plain": {}, "duel": dict(dueling=True), "c51": dict(dist=crl.C51Options()), "duel_c51": dict(dueling=True, dist=crl.C51Options()),
             "duel_c51_per_n3_double": dict(dueling=True, **full)}
    return crl, cfg, {k: crl.DQNAgent(cfg, seed=1, **kw) for k, kw in kinds.items() if only is None or k in only}


def child_arms(steps, repeats):
    crl, cfg, agents = _agents(steps * (repeats + 2))
    clock0 = crl._lib.clock_probe(0)
    for a in agents.values():
        a.handle.run(steps)                                   # warm-up: code objects, the ring past min_buff_size, every kernel of the cycle
    times = {k: [] for k in agents}
    for _ in range(repeats):
        for kind, a in agents.items():                        # alternating, same process, same box
            t0 = time.perf_counter()
            taken, _, _ = a.handle.run(steps)
            times[kind].append(time.perf_counter() - t0)
            assert taken == steps
    clock1 = crl._lib.clock_probe(0)
    out = {k: BT._window_stats(v, steps / cfg.train_freq) for k, v in times.items()}
    out["shader_clock_mhz"] = {"before": dict(zip(("median", "min", "max"), clock0)), "after": dict(zip(("median", "min", "max"), clock1))}
    print("RESULT " + json.dumps(out))


def trace_run(steps):
    _, _, agents = _agents(2 * steps, only=("duel", "duel_c51_per_n3_double"))
    for a in agents.values():
        a.handle.run(2 * steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--parent", default=None, help="the parent commit's libcleanrl_hip.so")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "duel_bench.json"))
    ap.add_argument("--child-arms", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    args = ap.parse_args()
    if args.child_arms:
        return child_arms(args.steps, args.repeats)
    if args.trace_run:
        return trace_run(args.steps)
    size = ["--steps", str(args.steps), "--repeats", str(args.repeats)]
    arms = BC._child(os.path.abspath(__file__), ["--child-arms"] + size)
    base = arms["plain"]["us_per_cycle_median"]
    for k, v in arms.items():
        if k != "shader_clock_mhz":
            v["over_plain_percent"] = 100.0 * (v["us_per_cycle_median"] - base) / base
            print(f"{k:24s} {v['us_per_cycle_median']:.2f} us/cycle ({v['over_plain_percent']:+.1f} %)")
    prof = {"what": "us per ten-launch DQN cycle at the reference defaults: dqn.jl's net, the scalar dueling head, C51 at N = 51, dueling + C51, and "
                    "dueling + C51 + PER + 3-step + double, alternating windows in one process; the kernels on their own from a rocprofv3 run of "
                    "its own; the plain handle of this tree against the parent commit's library, alternating child processes (scripts/bench_duel.py)",
            "steps_per_window": args.steps, "windows": args.repeats, "arms": arms}
    if os.path.exists(args.out):                               # a second call (the kernel statistics come from a run of their own) keeps what is there
        old = json.load(open(args.out))
        prof.update({k: old[k] for k in ("kernels", "plain_handle_vs_parent") if k in old})
    if args.kernel_stats:
        prof["kernels"] = BP.kernel_stats(args.kernel_stats)
    if args.parent:
        from cleanrl_jl_amd import _lib as L
        libs = {"parent": os.path.abspath(args.parent), "tree": os.path.abspath(L.LIB_PATH)}
        rounds = {k: [] for k in libs}
        for _ in range(args.rounds):
            for k, path in libs.items():
                rounds[k].append(BC._child(os.path.abspath(BT.__file__), ["--child-plain", path] + size)["us_per_cycle_median"])
        lo, hi = min(rounds["parent"]), max(rounds["parent"])
        med = statistics.median(rounds["tree"])
        prof["plain_handle_vs_parent"] = {"rounds": args.rounds, "us_per_cycle_per_round": rounds,
                                          "parent_median": statistics.median(rounds["parent"]), "parent_min": lo, "parent_max": hi, "tree_median": med,
                                          "tree_min": min(rounds["tree"]), "tree_max": max(rounds["tree"]), "tree_median_inside_parent_spread": lo <= med <= hi,
                                          "tree_median_minus_parent_median": med - statistics.median(rounds["parent"])}
        print("plain handle, us/cycle per round:", {k: [round(x, 2) for x in v] for k, v in rounds.items()},
              "tree median inside the parent's spread:", lo <= med <= hi)
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
