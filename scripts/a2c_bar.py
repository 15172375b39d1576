#!/usr/bin/env python3
"""Measures what the A2C parity bars are worth, on the CPU, and writes profiles/a2c_bar.json.

For every case of tests/a2c_bar.py's table, on the batches the C oracle (oracle/a2c_oracle.c) plays:
  floor           the distance between tests/a2c_ref.py and a twin of itself whose every exp / log result is moved by a seeded random integer in
                  -2..+2 ulp (three seeds, the maximum): how far two correct implementations of the same update may be apart
  oracle_to_twin  the distance between the C oracle and a2c_ref
  mutants         the distance between a2c_ref and one-line wrong versions of it, each mirroring one line of csrc/a2c.hip
Then loss_bar = 32 x the largest loss floor, param_bar = 2^-21 (gradients and parameters), and the conditions the table has to meet are checked: the
oracle is within the bars of the twin in every case, and every applicable mutant moves at least one of the four observables past 10x its bar in
every case. A mutant that only the gradients show (crl_a2c_read_grads; Adam's step is blind to a gradient's scale) is marked only_read_grads. The
script fails if a condition does not hold: then the case, not the bar, changes. Everything is seeded: a second run writes the same bytes. What a
GPU run recorded under "device" (tests/test_gpu_a2c_edges.py) is kept.

usage: python scripts/a2c_bar.py [--jobs N] [--out profiles/a2c_bar.json]"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import a2c_bar as B   # noqa: E402


def _measure(name):
    rec = B.measure(B.CASE[name])
    rec["n"] = [u["n"] for u in B.oracle_run(name)[1]]
    return name, rec


def build(jobs):
    with multiprocessing.Pool(jobs) as pool:
        cases = dict(pool.map(_measure, [c["name"] for c in B.CASES], chunksize=1))
    loss_floor = max(cases[n]["floor"][o] for n in cases for o in B.LOSSES)
    loss_bar = B.LOSS_FACTOR * loss_floor
    for c in B.CASES:
        rec = cases[c["name"]]
        rec.update(edge=c["edge"], max_steps=c["max_steps"], min_replay_size=c["min_replay_size"], gamma=c["gamma"], head=c["head"])
        rec["mutant_ratio"] = {m: B.mutant_ratio(d, loss_bar) for m, d in rec["mutants"].items()}
        rec["mutant_ratio_without_grads"] = {m: B.mutant_ratio(d, loss_bar, without=("grads",)) for m, d in rec["mutants"].items()}
    mutants = {}
    for m, (what, _, _) in B.MUTANTS.items():
        ratios = {n: cases[n]["mutant_ratio"][m] for n in cases if m in cases[n]["mutant_ratio"]}
        blind = {n: cases[n]["mutant_ratio_without_grads"][m] for n in ratios}
        worst = min(ratios, key=ratios.get)
        mutants[m] = {"what": what, "cases": len(ratios), "worst_ratio": ratios[worst], "worst_case": worst,
                      "only_read_grads": sorted(n for n in blind if blind[n] < B.MUTANT_FACTOR), "synthetic_open_end": m in B.SYNTHETIC}
    return {
        "what": "distances: per update and array max |x - ref| / max |ref| (grads, params after the step), the maximum over the updates; losses "
                "relative to the case's largest. floor: ref = a2c_ref, x = a2c_ref with exp / log jittered; oracle_to_twin: ref = the C oracle, x = "
                "a2c_ref; mutants: x = a one-line wrong a2c_ref; mutant_ratio: the largest distance / bar over the four observables; "
                "only_read_grads: the cases where the mutant stays under 10 bars on losses and parameters (scripts/a2c_bar.py). device: ref = the C "
                "oracle, x = the library on an MI355X (tests/test_gpu_a2c_edges.py)",
        "jitter_ulp": {k: B.JITTER_ULP[k] for k in ("exp", "log")}, "jitter_seeds": list(B.JITTER_SEEDS), "loss_factor": B.LOSS_FACTOR,
        "mutant_factor": B.MUTANT_FACTOR, "loss_floor": loss_floor, "loss_bar": loss_bar, "param_bar": B.PARAM_BAR, "cases": cases, "mutants": mutants,
    }


def check(prof):
    """the conditions; → list of what fails"""
    bad = []
    for n, rec in prof["cases"].items():
        bad += [f"{n}: the oracle is {v} from the twin on {o}" for o, v in rec["oracle_to_twin"].items()
                if not v <= B.bar_of(o, prof["loss_bar"], prof["param_bar"])]
        bad += [f"{n}: {m} moves no observable past {prof['mutant_factor']} bars (ratio {r:.3g})" for m, r in rec["mutant_ratio"].items()
                if not r >= prof["mutant_factor"]]
        if not B.n_matches(B.CASE[n], B.oracle_run(n)[1]):
            bad.append(f"{n}: the batch sizes {rec['n']} are not the table's")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=B.BAR_JSON)
    args = ap.parse_args()
    prof = build(args.jobs)
    try:
        device = json.load(open(args.out)).get("device")
    except (OSError, ValueError):
        device = None
    if device:
        prof["device"] = device
    with open(args.out, "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"loss floor {prof['loss_floor']:.3e} -> loss_bar {prof['loss_bar']:.3e}; param_bar {prof['param_bar']:.3e}")
    for m, rec in prof["mutants"].items():
        print(f"{m:3s} worst ratio {rec['worst_ratio']:.3e} ({rec['worst_case']}, {rec['cases']} cases), only grads in {len(rec['only_read_grads'])}  {rec['what']}")
    bad = check(prof)
    for b in bad:
        print("FAILS:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
