#!/usr/bin/env python3
"""Measures what the dueling-DQN parity bars are worth, on the CPU, and writes profiles/duel_bar.json — scripts/c51_bar.py for tests/duel_bar.py's
table.

For every case: the jitter floor (tests/duel_ref.py against a twin whose every exp, log and pow result is moved by -2..+2 ulp, three seeds, the
maximum; the device's own error in the three has not been measured), whether every twin stayed on the reference's own trajectory (greedy actions, a*,
idx, Float32 PER leaves: the tie condition), and the distance of every one-line mutant on the cases where a run is cheap. Then loss_bar = 32 x the
largest loss floor over the table, proj_bar = 32 x the largest floor of the projected targets, param_bar = 2^-21, and the conditions are checked: the
tie condition holds in every case, every parameter floor lies under param_bar, the scalar cases with uniform replay have a floor of exactly 0, and every
mutant moves some observable past 10 bars on the case that sees it best. The script fails otherwise — then the case (its seed), not the bar, changes.
Everything is seeded: a second run writes the same bytes.

usage: python scripts/duel_bar.py [--jobs N] [--out FILE]"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import duel_bar as B   # noqa: E402


def _measure(name):
    return name, B.measure(B.CASE[name])


def build(jobs):
    with multiprocessing.Pool(jobs) as pool:
        cases = dict(pool.map(_measure, [c["name"] for c in B.CASES], chunksize=1))
    loss_floor = max(cases[n]["floor"]["loss"] for n in cases)
    proj_floor = max(cases[n]["floor"]["proj"] for n in cases)
    bars = {"loss": B.LOSS_FACTOR * loss_floor, "q": B.PARAM_BAR, "target": B.PARAM_BAR, "proj": B.LOSS_FACTOR * proj_floor}
    for c in B.CASES:
        rec = cases[c["name"]]
        cfg = B.case_cfg(c)
        rec.update(batch_size=cfg.batch_size, buffer_size=cfg.buffer_size, seed=c["seed"], per=B.case_per(c), tgt=B.case_tgt(c), c51=B.case_c51(c),
                   edge=c["edge"])
        rec["mutant_ratio"] = {m: B.mutant_ratio(dist, bars) for m, dist in rec["mutants"].items()}
    mutants = {}
    for m, (what, _) in B.MUTANTS.items():
        ratios = {n: cases[n]["mutant_ratio"][m] for n in cases if m in cases[n]["mutant_ratio"]}
        best = max(ratios, key=ratios.get)
        mutants[m] = {"what": what, "cases": len(ratios), "best_ratio": ratios[best], "best_case": best, "worst_ratio": min(ratios.values())}
    return {
        "what": "distances: loss max |x - ref| / max |ref| over the logged losses; q, target max |x - ref| / max |ref| per array; proj max |x - ref| "
                "of the last update's projected targets (0 on a scalar head). floor: x = duel_ref with exp, log and pow jittered; mutants: x = a "
                "one-line wrong duel_ref; mutant_ratio: the largest distance / bar over the observables (scripts/duel_bar.py)",
        "jitter_ulp": B.JITTER_ULP, "jitter_ulp_source": "ddpg_bar.JITTER_ULP, the amplitude this suite assumes for exp, log and pow; the device's own "
                                                         "error has not been measured",
        "jitter_seeds": list(B.JITTER_SEEDS), "loss_factor": B.LOSS_FACTOR, "mutant_factor": B.MUTANT_FACTOR,
        "loss_floor": loss_floor, "loss_bar": bars["loss"], "proj_floor": proj_floor, "proj_bar": bars["proj"], "param_bar": B.PARAM_BAR,
        "cases": cases, "mutants": mutants,
    }


def check(prof):
    """the conditions; → list of what fails"""
    bad = []
    for n, rec in prof["cases"].items():
        if not rec["ties_ok"]:
            bad.append(f"{n}: a jittered twin left the reference's trajectory (greedy action, a*, idx or Float32 leaf): change the case's seed")
        bad += [f"{n}: the jitter floor of {o} is {rec['floor'][o]:.3g}, above param_bar" for o in B.PARAMS if not rec["floor"][o] <= prof["param_bar"]]
        if n in B.SCALAR_UNIFORM and any(rec["floor"][o] != 0.0 for o in B.OBSERVABLES):
            bad.append(f"{n}: a scalar head with uniform replay runs no transcendental, yet its floor is not 0")
    for m, rec in prof["mutants"].items():
        if not rec["best_ratio"] >= prof["mutant_factor"]:
            bad.append(f"{m}: moves no observable past {prof['mutant_factor']} bars on any case (best ratio {rec['best_ratio']:.3g})")
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
    print(f"loss floor {prof['loss_floor']:.3e} -> loss_bar {prof['loss_bar']:.3e}; proj floor {prof['proj_floor']:.3e} -> proj_bar "
          f"{prof['proj_bar']:.3e}; param_bar {prof['param_bar']:.3e}")
    for m, rec in prof["mutants"].items():
        print(f"{m:3s} best ratio {rec['best_ratio']:.3e} ({rec['best_case']}), worst {rec['worst_ratio']:.3e} over {rec['cases']} cases  {rec['what']}")
    bad = check(prof)
    for b in bad:
        print("FAILS:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
