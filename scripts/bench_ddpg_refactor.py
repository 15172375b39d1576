#!/usr/bin/env python3
"""Did csrc/ddpg.hip and csrc/sac.hpp keep their speed when their passes, steps and host calls were stated once ("One function per
job")? This tree's library against the parent commit's, never against itself -> profiles/ddpg_refactor_bench.json.

Two measurements, each in fresh child processes that alternate tree, parent, tree, parent … for `--rounds` rounds on one box in one run; a child loads
its library through CRL_LIB_PATH:
  cycle     scripts/bench_sac.py's method at the reference defaults (batch 120, one update per env step after warmup_steps = 2500): us per six-launch
            cycle of DDPG, TD3 at policy_delay 1 and 2, SAC with autotune on and off; wall clock around crl_ddpg_run, the median of three windows
  evaluate  crl_ddpg_evaluate at scripts/ddpg_eval_cost.py's shape, 256 envs x 1 episode of 200 steps on a DDPG handle, wall clock around the call,
            the median of `--eval-repeats` calls after one warm-up
The criterion is the project's: the tree's median over its rounds lies inside the parent's own min–max over its rounds
(tree_median_inside_parent_spread); a median below the parent's minimum is marked tree_median_below_parent_min, and none_above_parent_max says that no
figure lies above the parent's spread. The shader clock under load (crl_clock_probe) is kept for every child.

usage: python scripts/bench_ddpg_refactor.py --parent LIB [--updates N] [--eval-repeats R] [--rounds K] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
ARMS = ("ddpg", "td3_policy_delay_1", "td3_policy_delay_2", "sac", "sac_autotune_off")
QUIET = 2500 + 2000                                          # the warm-up and 2000 cycles before the first timed window


def _us_per_cycle(agent, updates):
    h = agent.handle
    h.run(QUIET)
    windows = []
    for _ in range(3):
        s0 = h.status(); t0 = time.perf_counter()
        h.run(updates // 3)
        dt = time.perf_counter() - t0
        windows.append(1e6 * dt / (h.status()["global_step"] - s0["global_step"]))
    agent.close()
    return statistics.median(windows)


def child_cycle(updates):
    import cleanrl_jl_amd as crl
    total = QUIET + updates
    clock = crl._lib.clock_probe(0)
    make = {"ddpg": lambda: crl.DDPGAgent(crl.DDPGConfig(total_timesteps=total), seed=1),
            "td3_policy_delay_1": lambda: crl.TD3Agent(crl.TD3Config(total_timesteps=total, policy_delay=1), seed=1),
            "td3_policy_delay_2": lambda: crl.TD3Agent(crl.TD3Config(total_timesteps=total, policy_delay=2), seed=1),
            "sac": lambda: crl.SACAgent(crl.SACConfig(total_timesteps=total), seed=1),
            "sac_autotune_off": lambda: crl.SACAgent(crl.SACConfig(total_timesteps=total, autotune=False, alpha=0.2), seed=1)}
    out = {a: _us_per_cycle(make[a](), updates) for a in ARMS}
    out["shader_clock_mhz"] = {"median": clock[0], "min": clock[1], "max": clock[2]}
    print("RESULT " + json.dumps(out))


def child_eval(repeats):
    import cleanrl_jl_amd as crl
    agent = crl.DDPGAgent(crl.DDPGConfig(total_timesteps=1000), seed=1)
    h = agent.handle
    h.evaluate(256, 1, 0xE7A1)                                   # warm-up: the code object, the scratch
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        h.evaluate(256, 1, 0xE7A1)
        times.append(time.perf_counter() - t0)
    agent.close()
    print("RESULT " + json.dumps({"us_median": 1e6 * statistics.median(times), "us_min": 1e6 * min(times), "us_max": 1e6 * max(times)}))


def _child(args, lib):
    env = dict(os.environ)
    env.pop("CRL_LIB_PATH", None)
    if lib:
        env["CRL_LIB_PATH"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=300, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(1)
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def _verdict(rounds):
    """rounds: {"tree": [x per round], "parent": [...]} -> the project's criterion"""
    lo, hi, med = min(rounds["parent"]), max(rounds["parent"]), statistics.median(rounds["tree"])
    return {"per_round": rounds, "parent_median": statistics.median(rounds["parent"]), "parent_min": lo, "parent_max": hi, "tree_median": med,
            "tree_min": min(rounds["tree"]), "tree_max": max(rounds["tree"]), "tree_median_inside_parent_spread": lo <= med <= hi,
            "tree_median_below_parent_min": med < lo,      # outside the spread on the fast side: not a loss
            "tree_median_minus_parent_median": med - statistics.median(rounds["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's libcleanrl_hip.so")
    ap.add_argument("--updates", type=int, default=15_000, help="timed cycles per arm and child, in three windows")
    ap.add_argument("--eval-repeats", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ddpg_refactor_bench.json"))
    ap.add_argument("--child-cycle", action="store_true")
    ap.add_argument("--child-eval", action="store_true")
    args = ap.parse_args()
    if args.child_cycle:
        return child_cycle(args.updates)
    if args.child_eval:
        return child_eval(args.eval_repeats)
    if not args.parent:
        ap.error("--parent LIB is required: the comparison is against the parent commit's library")
    libs = {"tree": None, "parent": os.path.abspath(args.parent)}
    cycle = {a: {k: [] for k in libs} for a in ARMS}
    evaluate = {k: [] for k in libs}
    clocks = []
    for r in range(args.rounds):
        for k, lib in libs.items():
            res = _child(["--child-cycle", "--updates", str(args.updates)], lib)
            clocks.append({"round": r, "library": k, **res["shader_clock_mhz"]})
            for a in ARMS:
                cycle[a][k].append(res[a])
            evaluate[k].append(_child(["--child-eval", "--eval-repeats", str(args.eval_repeats)], lib)["us_median"])
            print(f"round {r} {k:6s} cycle us " + " ".join(f"{a}={cycle[a][k][-1]:.2f}" for a in ARMS) + f" | evaluate us {evaluate[k][-1]:.0f}", flush=True)
    prof = {"what": "this tree's library against the parent commit's, alternating fresh child processes on one box in one run: us per six-launch cycle "
                    "at the reference defaults (batch 120) for DDPG, TD3 at policy_delay 1 and 2 and SAC with autotune on and off, and us per "
                    "crl_ddpg_evaluate call at 256 envs x 1 episode of 200 steps (scripts/bench_ddpg_refactor.py)",
            "rounds": args.rounds, "updates_per_arm": args.updates, "windows": 3, "evaluate_calls": args.eval_repeats,
            "us_per_cycle": {a: _verdict(v) for a, v in cycle.items()}, "us_per_evaluate": {"ddpg_256x1": _verdict(evaluate)}, "shader_clock_mhz": clocks}
    figures = list(prof["us_per_cycle"].items()) + list(prof["us_per_evaluate"].items())
    prof["none_above_parent_max"] = all(v["tree_median_inside_parent_spread"] or v["tree_median_below_parent_min"] for _, v in figures)
    for k, v in figures:
        print(f"{k:20s} tree {v['tree_median']:.2f} parent {v['parent_min']:.2f}..{v['parent_max']:.2f} inside: {v['tree_median_inside_parent_spread']} "
              f"below: {v['tree_median_below_parent_min']}")
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
