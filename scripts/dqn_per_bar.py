#!/usr/bin/env python3
"""Measures what the prioritized-replay parity bars are worth, on the CPU, and writes profiles/dqn_per_bar.json — scripts/td3_bar.py for
tests/dqn_per_bar.py's table.

For every case: the jitter floor (tests/dqn_per_ref.py against a twin whose every pow result is moved by -16..+16 ulp, three seeds, the maximum),
whether every twin drew the reference's own idx and Float32 leaves after every update (the tie condition), the reference's own statistics of the case
and the distance of every applicable one-line mutant. Then loss_bar = 32 x the largest loss floor over the table, param_bar = 2^-21, and the conditions
the table has to meet are checked: the tie condition holds in every case, every applicable mutant moves at least one of the three observables past 10x
its bar in every case it applies to, and every mutant applies somewhere — except a mutant named in UNOBSERVABLE below, with the reason. The script fails
otherwise — then the case (its seed), not the bar, changes. Everything is seeded: a second run writes the same bytes.

usage: python scripts/dqn_per_bar.py [--jobs N] [--out FILE]"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dqn_per_bar as B   # noqa: E402

# M8 needs a draw whose target rounding puts at or past the left sum of a node with an empty right subtree. The leaves are 24-bit values, so the sums
# of a ring are exact unless its priorities span more than 2^13, and target < node then holds exactly at every visited node; what is left is the
# rounding of target - l, one chance in about 2^52 per level. No run of a few hundred updates meets it ("zero_saves" counts them: 0 in every case).
# The zero test is pinned directly instead: tests/test_dqn_per_cpu.py descends with a constructed target, and the probe cases of
# tests/test_gpu_dqn_per.py with n < C assert that no slot >= n comes back.
UNOBSERVABLE = {"M8": "no draw of any case needs the zero test (zero_saves = 0): about 2^-52 per level; pinned by a constructed target on the CPU"}


def _measure(name):
    return name, B.measure(B.CASE[name])


def build(jobs):
    with multiprocessing.Pool(jobs) as pool:
        cases = dict(pool.map(_measure, [c["name"] for c in B.CASES], chunksize=1))
    loss_floor = max(cases[n]["floor"][o] for n in cases for o in B.LOSSES)
    loss_bar = B.LOSS_FACTOR * loss_floor
    for c in B.CASES:
        rec = cases[c["name"]]
        cfg = B.case_cfg(c)
        rec.update(batch_size=cfg.batch_size, buffer_size=cfg.buffer_size, seed=c["seed"], per=B.case_per(c), edge=c["edge"])
        rec["mutant_ratio"] = {m: B.mutant_ratio(dist, loss_bar) for m, dist in rec["mutants"].items()}
    mutants = {}
    for m, (what, _, _) in B.MUTANTS.items():
        ratios = {n: cases[n]["mutant_ratio"][m] for n in cases if m in cases[n]["mutant_ratio"]}
        if not ratios:
            mutants[m] = {"what": what, "cases": 0, "unobservable": UNOBSERVABLE.get(m)}
            continue
        worst = min(ratios, key=ratios.get)
        mutants[m] = {"what": what, "cases": len(ratios), "worst_ratio": ratios[worst], "worst_case": worst, "best_ratio": max(ratios.values())}
    return {
        "what": "distances are max |x - dqn_per_ref| / max |dqn_per_ref| per array; floor: x = dqn_per_ref with pow jittered; mutants: x = a one-line "
                "wrong dqn_per_ref; mutant_ratio: the largest distance / bar over the three observables (scripts/dqn_per_bar.py)",
        "jitter_ulp": B.JITTER_ULP, "jitter_ulp_source": "OpenCL full-profile bound for pow; the ROCm tree states none for the device pow, and none was measured",
        "jitter_seeds": list(B.JITTER_SEEDS), "loss_factor": B.LOSS_FACTOR, "mutant_factor": B.MUTANT_FACTOR,
        "loss_floor": loss_floor, "loss_bar": loss_bar, "param_bar": B.PARAM_BAR, "cases": cases, "mutants": mutants,
    }


def check(prof):
    """the conditions; → list of what fails"""
    bad = []
    for n, rec in prof["cases"].items():
        if not rec["ties_ok"]:
            bad.append(f"{n}: a jittered twin drew other idx or left other Float32 leaves: change the case's seed")
        bad += [f"{n}: the jitter floor of {o} is {rec['floor'][o]}, not 0.0" for o in B.PARAMS if rec["floor"][o] != 0.0]
        bad += [f"{n}: {m} moves no observable past {prof['mutant_factor']} bars (ratio {r:.3g})" for m, r in rec["mutant_ratio"].items()
                if not r >= prof["mutant_factor"]]
    for m, rec in prof["mutants"].items():
        if rec["cases"] == 0 and not rec.get("unobservable"):
            bad.append(f"{m} applies to no case of the table")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=B.BAR_JSON)
    args = ap.parse_args()
    prof = build(args.jobs)
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"loss floor {prof['loss_floor']:.3e} -> loss_bar {prof['loss_bar']:.3e}; param_bar {prof['param_bar']:.3e}")
    for m, rec in prof["mutants"].items():
        if rec["cases"]:
            print(f"{m:3s} worst ratio {rec['worst_ratio']:.3e} ({rec['worst_case']}, {rec['cases']} cases)  {rec['what']}")
        else:
            print(f"{m:3s} applies to no case: {rec['unobservable']}  {rec['what']}")
    bad = check(prof)
    for b in bad:
        print("FAILS:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
