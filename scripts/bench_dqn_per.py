#!/usr/bin/env python3
"""What prioritized replay costs per DQN cycle on the GPU, and which LDS split of the draw it is measured with -> profiles/dqn_per_bench.json.

At the reference defaults (ring 10 000, so a tree of C = 16 384 leaves and 14 levels; batch 120; an update every 10 steps) a uniform handle
(crl_dqn_create: the parent's code path, which prioritized replay does not change) and a PER handle (crl_dqn_per_create) run alternately in one
process: a warm-up, then `--repeats` windows of `--steps` env steps each, a host clock around crl_dqn_run, which ends in a stream synchronise.
us per cycle = window time / (steps / train_freq); the median and the spread over the windows are kept. One fresh child process per library:
the default build and, with --variants, builds of csrc/dqn_per.hpp at other CRL_DQN_PER_LDS_LEVELS (scripts/build_variant.sh; the library is
chosen by CRL_LIB_PATH at import).

The two PER kernels apart: `--trace-run` runs the PER handle alone for `--steps` steps and is meant to be the program of
`rocprofv3 --kernel-trace --stats`, in a run of its own; `--kernel-stats FILE` folds that run's kernel statistics (CSV) into the JSON.

usage: python scripts/bench_dqn_per.py [--steps N] [--repeats R] [--variants L0=path/lib.so,L8=...] [--kernel-stats FILE] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_dqn_per.py --trace-run"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _agents(total):
    import cleanrl_jl_amd as crl
    cfg = crl.DQNConfig(total_timesteps=total)
    return crl, cfg, {"uniform": crl.DQNAgent(cfg, seed=1), "per": crl.DQNAgent(cfg, seed=1, per=crl.PEROptions())}


def child(steps, repeats):
    crl, cfg, agents = _agents(steps * (repeats + 2))
    for a in agents.values():
        a.handle.run(steps)                                   # warm-up: code objects, the ring past min_buff_size, every kernel of the cycle
    times = {k: [] for k in agents}
    for _ in range(repeats):
        for kind, a in agents.items():                        # alternating, same process, same box
            t0 = time.perf_counter()
            taken, _, _ = a.handle.run(steps)
            times[kind].append(time.perf_counter() - t0)
            assert taken == steps
    cycles = steps / cfg.train_freq
    out = {k: {"us_per_cycle_median": 1e6 * statistics.median(v) / cycles, "us_per_cycle_min": 1e6 * min(v) / cycles,
               "us_per_cycle_max": 1e6 * max(v) / cycles} for k, v in times.items()}
    out["per_status"] = {k: float(v) for k, v in agents["per"].handle.per_status().items()}
    print("RESULT " + json.dumps(out))


def trace_run(steps):
    crl, cfg, agents = _agents(2 * steps)
    agents["per"].handle.run(2 * steps)


def kernel_stats(path):
    """rocprofv3's kernel statistics (Name, Calls, TotalDurationNs, AverageNs, ...) -> {kernel: {calls, average_us}} for the dqn kernels"""
    out = {}
    for row in csv.DictReader(open(path)):
        name = row["Name"].split("(")[0].split("::")[-1]
        if name.startswith("dqn_"):
            out[name] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "total_ms": float(row["TotalDurationNs"]) / 1e6}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--variants", default="", help="label=library,... : other builds to measure next to the default one")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_per_bench.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.steps, args.repeats)
    if args.trace_run:
        return trace_run(args.steps)
    libs = [("default", None)] + [tuple(v.split("=", 1)) for v in args.variants.split(",") if v]
    results = {}
    for label, lib in libs:
        env = dict(os.environ)
        if lib:
            env["CRL_LIB_PATH"] = os.path.abspath(lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--repeats", str(args.repeats)], env=env,
                           capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            return 1
        r = json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])
        r["overhead_us_per_cycle"] = r["per"]["us_per_cycle_median"] - r["uniform"]["us_per_cycle_median"]
        r["overhead_percent"] = 100.0 * r["overhead_us_per_cycle"] / r["uniform"]["us_per_cycle_median"]
        results[label] = r
        print(f"{label:8s} uniform {r['uniform']['us_per_cycle_median']:.2f} us/cycle, PER {r['per']['us_per_cycle_median']:.2f} us/cycle "
              f"({r['overhead_percent']:+.1f} %)")
    prof = {"what": "us per ten-launch DQN cycle at the reference defaults, uniform against prioritized replay, alternating windows in one process "
                    "per library (scripts/bench_dqn_per.py); labels Ln = csrc/dqn_per.hpp built with CRL_DQN_PER_LDS_LEVELS = n",
            "steps_per_window": args.steps, "windows": args.repeats, "libraries": results}
    if args.kernel_stats:
        prof["kernels"] = kernel_stats(args.kernel_stats)
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
