#!/usr/bin/env python3
"""Measures what the DDPG parity bars are worth, on the CPU, and writes profiles/ddpg_bar.json.

For every case of tests/ddpg_bar.py's table:
  floor    the distance between tests/ddpg_ref.py and a twin of itself whose every exp / log / cos result is moved by a seeded random integer in
           -2..+2 ulp (three seeds, the maximum): how far two correct implementations of the same loop may be apart. The amplitude is the error
           bound of the least accurate of the three device functions in Float64 (cos, 2 ulp); exp and log get the same.
  mutants  the distance between ddpg_ref and one-line wrong versions of it, each mirroring one line of csrc/ddpg.hip.
Then loss_bar = 32 x the largest loss floor, param_bar = 2^-21, and the two conditions the table has to meet are checked: every parameter floor
is exactly 0.0, and every applicable mutant moves at least one of the six observables past 10x its bar in every case. The script fails if either
does not hold — then the case, not the bar, changes. Everything is seeded: a second run writes the same bytes.

usage: python scripts/ddpg_bar.py [--jobs N] [--out profiles/ddpg_bar.json]"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ddpg_bar as B   # noqa: E402


def _measure(name):
    return name, B.measure(B.CASE[name])


def build(jobs):
    with multiprocessing.Pool(jobs) as pool:
        cases = dict(pool.map(_measure, [c["name"] for c in B.CASES], chunksize=1))
    loss_floor = max(cases[n]["floor"][o] for n in cases for o in B.LOSSES)
    loss_bar = B.LOSS_FACTOR * loss_floor
    for c in B.CASES:
        rec = cases[c["name"]]
        d = B.case_cfg(c)
        rec.update(D=c["D"], A=c["A"], batch_size=d["batch_size"], updates=c["T"] - B.threshold(d), edge=c["edge"])
        if c["name"] in B.MULTI_ROUND:
            rec["candidates_max"] = max(B.case_candidates(c))
        rec["mutant_ratio"] = {m: B.mutant_ratio(dist, loss_bar) for m, dist in rec["mutants"].items()}
    mutants = {}
    for m, (what, _, _) in B.MUTANTS.items():
        ratios = {n: cases[n]["mutant_ratio"][m] for n in cases if m in cases[n]["mutant_ratio"]}
        worst = min(ratios, key=ratios.get)
        mutants[m] = {"what": what, "cases": len(ratios), "worst_ratio": ratios[worst], "worst_case": worst}
    return {
        "what": "distances are max |x - ddpg_ref| / max |ddpg_ref| per array; floor: x = ddpg_ref with exp / log / cos jittered; mutants: x = a one-line "
                "wrong ddpg_ref; mutant_ratio: the largest distance / bar over the six observables (scripts/ddpg_bar.py)",
        "jitter_ulp": B.JITTER_ULP, "jitter_seeds": list(B.JITTER_SEEDS), "loss_factor": B.LOSS_FACTOR, "mutant_factor": B.MUTANT_FACTOR,
        "loss_floor": loss_floor, "loss_bar": loss_bar, "param_bar": B.PARAM_BAR, "cases": cases, "mutants": mutants,
    }


def check(prof):
    """the two conditions; → list of what fails"""
    bad = []
    for n, rec in prof["cases"].items():
        bad += [f"{n}: the jitter floor of {o} is {rec['floor'][o]}, not 0.0" for o in B.PARAMS if rec["floor"][o] != 0.0]
        bad += [f"{n}: {m} moves no observable past {prof['mutant_factor']} bars (ratio {r:.3g})" for m, r in rec["mutant_ratio"].items()
                if not r >= prof["mutant_factor"]]
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
        print(f"{m:4s} worst ratio {rec['worst_ratio']:.3e} ({rec['worst_case']}, {rec['cases']} cases)  {rec['what']}")
    bad = check(prof)
    for b in bad:
        print("FAILS:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
