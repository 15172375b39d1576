#!/usr/bin/env python3
"""Did csrc/dqn.hip keep its speed when its loops were stated once? This tree's library against the parent commit's, never against
itself -> profiles/dqn_refactor_bench.json.

Two measurements, each in fresh child processes that alternate tree, parent, tree, parent … for `--rounds` rounds on one box in one run; a child loads
its library through CRL_LIB_PATH (all five handle kinds exist in the parent):
  cycle     scripts/bench_duel.py --child-arms: us per ten-launch cycle of the plain, duel, c51, duel_c51 and duel_c51_per_n3_double arms
  evaluate  crl_dqn_evaluate at 256 envs x 1 episode on the three heads, wall clock around the call, the median of `--eval-repeats` calls after one
            warm-up: the balancer net of tests/value_eval_ref.py on the plain head (every episode runs to the step limit), a fresh net on the others
The criterion is the project's: the tree's median over its rounds lies inside the parent's own min–max over its rounds
(tree_median_inside_parent_spread); a median below the parent's minimum is marked tree_median_below_parent_min, and none_above_parent_max says that no
arm or head lies above the parent's spread. The shader clock under load (crl_clock_probe) is kept before and after.

usage: python scripts/bench_dqn_refactor.py --parent LIB [--steps N] [--repeats R] [--rounds K] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
ARMS = ("plain", "duel", "c51", "duel_c51", "duel_c51_per_n3_double")


def child_eval(repeats):
    import cleanrl_jl_amd as crl
    import value_eval_ref as V
    cfg = crl.DQNConfig(total_timesteps=1000)
    agents = {"plain": crl.DQNAgent(cfg, seed=1, params=V.dqn_balancer()), "c51": crl.DQNAgent(cfg, seed=1, dist=crl.C51Options()),
              "duel": crl.DQNAgent(cfg, seed=1, dueling=True)}
    out = {}
    for kind, a in agents.items():
        a.handle.evaluate(256, 1, seed=3)                       # warm-up: the code object, the scratch
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            rep = a.handle.evaluate(256, 1, seed=3)["report"]
            times.append(time.perf_counter() - t0)
        out[kind] = {"us_median": 1e6 * statistics.median(times), "us_min": 1e6 * min(times), "us_max": 1e6 * max(times), "env_steps": rep["env_steps"]}
    print("RESULT " + json.dumps(out))


def _child(args, lib):
    env = dict(os.environ)
    env.pop("CRL_LIB_PATH", None)
    if lib:
        env["CRL_LIB_PATH"] = lib
    p = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=600, env=env)
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
    ap.add_argument("--steps", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--eval-repeats", type=int, default=9)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_refactor_bench.json"))
    ap.add_argument("--child-eval", action="store_true")
    args = ap.parse_args()
    if args.child_eval:
        return child_eval(args.eval_repeats)
    if not args.parent:
        ap.error("--parent LIB is required: the comparison is against the parent commit's library")
    libs = {"tree": None, "parent": os.path.abspath(args.parent)}
    cycle_args = [os.path.join(ROOT, "scripts", "bench_duel.py"), "--child-arms", "--steps", str(args.steps), "--repeats", str(args.repeats)]
    eval_args = [os.path.abspath(__file__), "--child-eval", "--eval-repeats", str(args.eval_repeats)]
    cycle = {a: {k: [] for k in libs} for a in ARMS}
    evaluate = {h: {k: [] for k in libs} for h in ("plain", "c51", "duel")}
    clocks = []
    for r in range(args.rounds):
        for k, lib in libs.items():
            res = _child(cycle_args, lib)
            clocks.append({"round": r, "library": k, **res["shader_clock_mhz"]})
            for a in ARMS:
                cycle[a][k].append(res[a]["us_per_cycle_median"])
            res = _child(eval_args, lib)
            for h in evaluate:
                evaluate[h][k].append(res[h]["us_median"])
            print(f"round {r} {k:6s} cycle us " + " ".join(f"{a}={cycle[a][k][-1]:.2f}" for a in ARMS) +
                  " | evaluate us " + " ".join(f"{h}={evaluate[h][k][-1]:.0f}" for h in evaluate), flush=True)
    prof = {"what": "this tree's library against the parent commit's, alternating fresh child processes on one box in one run: us per ten-launch DQN "
                    "cycle of five handle kinds (scripts/bench_duel.py --child-arms, the median of its windows per round) and us per "
                    "crl_dqn_evaluate call at 256 envs x 1 episode on the three heads (scripts/bench_dqn_refactor.py)",
            "rounds": args.rounds, "steps_per_window": args.steps, "windows": args.repeats, "evaluate_calls": args.eval_repeats,
            "us_per_cycle": {a: _verdict(v) for a, v in cycle.items()}, "us_per_evaluate": {h: _verdict(v) for h, v in evaluate.items()},
            "shader_clock_mhz": clocks}
    prof["none_above_parent_max"] = all(v["tree_median_inside_parent_spread"] or v["tree_median_below_parent_min"] for d in (prof["us_per_cycle"], prof["us_per_evaluate"]) for v in d.values())
    for name, d in (("cycle", prof["us_per_cycle"]), ("evaluate", prof["us_per_evaluate"])):
        for k, v in d.items():
            print(f"{name:8s} {k:24s} tree {v['tree_median']:.2f} parent {v['parent_min']:.2f}..{v['parent_max']:.2f} inside: {v['tree_median_inside_parent_spread']}")
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
