#!/usr/bin/env python3
"""What noisy linear layers cost per DQN cycle on the GPU, and whether the plain handle kept its speed -> profiles/noisy_bench.json. Everything in
ONE call of this script, so on one box in one run.

Arms, at the reference defaults (ring 10 000, batch 120, an update every 10 steps): plain (crl_dqn_create), noisy (crl_dqn_noisy_create on dqn.jl's
net), full (dueling + C51Options() + PEROptions() + DQNTargetOptions(3, True): Rainbow's twin without noise) and rainbow (the same with noisy layers:
all six components). The twins' cycle is ten launches; a noisy arm's is eleven: its first nine are the twin's kernels, the tenth is
dqn_noisy_adam_kernel (Adam over mu and sigma where the twin steps its parameters) and the eleventh dqn_noisy_materialise_kernel (both images of the
next generation). So `over_twin_us`, the difference of the two cycle times, is what those two launches cost over the twin's Adam launch. No kernel is
timed on its own here.

One round = one fresh child process in which the four arms run alternately: a warm-up, then `--repeats` windows of `--steps` env steps each, a host
clock around crl_dqn_run, which ends in a stream synchronise; us per cycle = window time / (steps / train_freq); the shader clock under load
(crl_clock_probe) before and after. `--rounds` such children; an arm's figure is the median of its rounds' medians.

`--alt LIB` (with `--alt-name`) runs the same child on a second build of the library after each round, alternating: how the one-block tail
(make EXTRA=-DCRL_NOISY_SPLIT_TAIL=0, scripts/build_variant.sh: both images formed in the Adam launch's one block, a ten-launch cycle) was measured
against the default's eleventh launch.

`--parent LIB`: the plain handle of this tree against the parent commit's library — bare ctypes calls that the parent's library has too
(scripts/bench_dqn_target.py --child-plain), one fresh child per library and round, alternating, `--parent-rounds` each.

usage: python scripts/bench_noisy.py [--steps N] [--repeats R] [--rounds K] [--alt LIB --alt-name NAME] [--parent LIB --parent-rounds K] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bench_dqn_target as BT    # noqa: E402

ARMS = ("plain", "noisy", "full", "rainbow")
TWIN = {"noisy": "plain", "rainbow": "full"}


def _agents(total):
    import cleanrl_jl_amd as crl
    cfg = crl.DQNConfig(total_timesteps=total)
    full = dict(dueling=True, per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True), dist=crl.C51Options())
    kinds = {"plain": {}, "noisy": dict(noisy=crl.NoisyOptions()), "full": full, "rainbow": dict(noisy=crl.NoisyOptions(), **full)}
    return crl, cfg, {k: crl.DQNAgent(cfg, seed=1, **kinds[k]) for k in ARMS}


def child_arms(steps, repeats):
    """the library is the package's: CRL_LIB_PATH in the environment selects another build"""
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


def _child(script, args, lib=None):
    env = dict(os.environ)
    if lib is not None:
        env["CRL_LIB_PATH"] = os.path.abspath(lib)
    p = subprocess.run([sys.executable, script] + args, capture_output=True, text=True, timeout=600, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(1)
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def _fold(rounds):
    """the rounds of one library → per arm the median of the rounds' medians, the extremes over every window, and the rounds' medians"""
    out = {}
    for k in ARMS:
        meds = [r[k]["us_per_cycle_median"] for r in rounds]
        out[k] = {"us_per_cycle_median": statistics.median(meds), "us_per_cycle_min": min(r[k]["us_per_cycle_min"] for r in rounds),
                  "us_per_cycle_max": max(r[k]["us_per_cycle_max"] for r in rounds), "us_per_cycle_median_per_round": meds}
    for k, twin in TWIN.items():
        out[k]["over_twin_us"] = out[k]["us_per_cycle_median"] - out[twin]["us_per_cycle_median"]
        out[k]["over_twin_percent"] = 100.0 * out[k]["over_twin_us"] / out[twin]["us_per_cycle_median"]
    clocks = [r["shader_clock_mhz"][w][f] for r in rounds for w in ("before", "after") for f in ("min", "max")]
    out["shader_clock_mhz"] = {"min": min(clocks), "max": max(clocks)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--alt", default=None, help="a second build of this tree's library, measured alternately with it")
    ap.add_argument("--alt-name", default="alt")
    ap.add_argument("--parent", default=None, help="the parent commit's libcleanrl_hip.so")
    ap.add_argument("--parent-rounds", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noisy_bench.json"))
    ap.add_argument("--child-arms", action="store_true")
    args = ap.parse_args()
    if args.child_arms:
        return child_arms(args.steps, args.repeats)
    me, size = os.path.abspath(__file__), ["--steps", str(args.steps), "--repeats", str(args.repeats)]
    tree, alt = [], []
    for _ in range(args.rounds):
        tree.append(_child(me, ["--child-arms"] + size))
        if args.alt:
            alt.append(_child(me, ["--child-arms"] + size, lib=args.alt))
    arms = _fold(tree)
    for k in ARMS:
        v = arms[k]
        print(f"{k:8s} {v['us_per_cycle_median']:.2f} us/cycle" +
              (f" ({v['over_twin_us']:+.2f} us, {v['over_twin_percent']:+.1f} % over {TWIN[k]})" if k in TWIN else ""))
    prof = {"what": "us per DQN cycle at the reference defaults: dqn.jl's net (plain), the same with noisy layers (noisy), dueling + C51 + PER + 3-step "
                    "+ double (full), and the same with noisy layers (rainbow); a twin's cycle is ten launches, a noisy arm's eleven — nine of the "
                    "twin's kernels, the Adam launch over mu and sigma, the launch that forms both images —, and over_twin_us is the difference of the "
                    "cycle times; no kernel is timed on its own. Rounds of fresh child processes, the arms alternating inside each; alt: the same "
                    "children on a second build, alternating with the tree's; plain_handle_vs_parent: the plain handle of this tree against the parent "
                    "commit's library, alternating child processes. One call of scripts/bench_noisy.py: one box, one run",
            "steps_per_window": args.steps, "windows": args.repeats, "rounds": args.rounds, "arms": arms}
    if args.alt:
        prof["alt"] = {"name": args.alt_name, "arms": _fold(alt)}
        for k in TWIN:
            d = arms[k]["us_per_cycle_median"] - prof["alt"]["arms"][k]["us_per_cycle_median"]
            prof["alt"][f"tree_minus_alt_us_{k}"] = d
            print(f"{k:8s} tree {arms[k]['us_per_cycle_median']:.2f} against {args.alt_name} {prof['alt']['arms'][k]['us_per_cycle_median']:.2f} us/cycle ({d:+.2f})")
    if args.parent:
        from cleanrl_jl_amd import _lib as L
        libs = {"parent": os.path.abspath(args.parent), "tree": os.path.abspath(L.LIB_PATH)}
        rounds = {k: [] for k in libs}
        for _ in range(args.parent_rounds):
            for k, path in libs.items():
                rounds[k].append(_child(os.path.abspath(BT.__file__), ["--child-plain", path] + size)["us_per_cycle_median"])
        lo, hi = min(rounds["parent"]), max(rounds["parent"])
        med = statistics.median(rounds["tree"])
        prof["plain_handle_vs_parent"] = {"rounds": args.parent_rounds, "us_per_cycle_per_round": rounds,
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
