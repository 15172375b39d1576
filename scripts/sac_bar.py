#!/usr/bin/env python3
"""Measures what the SAC parity bars are worth, on the CPU, and writes profiles/sac_bar.json — scripts/td3_bar.py for tests/sac_bar.py's tables.

For every case: the jitter floor (tests/sac_ref.py against a twin whose every exp / log / cos result is moved by -2..+2 ulp, three seeds, the
maximum) over the nine observables, the reference's own counters of the case (samples of both passes, |y| = 1 exactly, 0 < 1 - y² < 1e-6, log_std
within 1e-3 of either end) and the distance of every applicable one-line mutant. Then loss_bar = 32 x the largest loss floor over the table and
param_bar = 2^-21. The conditions: no parameter floor (log_alpha included) above param_bar — a floor above it is reported, never absorbed —, every
mutant moves an observable past 10 bars on at least one case it applies to, and the cases built around an edge met it on the reference's counters.
The script fails otherwise. The edge table's profile also holds a "rejected" block: the floors of tests/sac_bar.py's REJECTED settings, which are
above param_bar and therefore not cases. Everything is seeded: a second run writes the same bytes.

usage: python scripts/sac_bar.py [--table cases|edges] [--jobs N] [--out FILE]"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sac_bar as B   # noqa: E402


def _measure(job):
    table, name = job
    return name, B.measure(next(c for c in B.TABLES[table][0] if c["name"] == name))


def build(jobs, table="cases"):
    table_cases = B.TABLES[table][0]
    with multiprocessing.Pool(jobs) as pool:
        cases = dict(pool.map(_measure, [(table, c["name"]) for c in table_cases], chunksize=1))
    loss_floors = {n: max(cases[n]["floor"][o] for o in B.LOSSES) for n in cases}
    loss_floor = max(loss_floors.values())
    loss_bar = B.LOSS_FACTOR * loss_floor
    for c in table_cases:
        rec = cases[c["name"]]
        d = B.case_cfg(c)
        rec.update(D=c["D"], A=c["A"], batch_size=d["batch_size"], updates=c["T"] - B.threshold(d), edge=c["edge"], loss_floor=loss_floors[c["name"]])
        rec["mutant_ratio"] = {m: B.mutant_ratio(dist, loss_bar) for m, dist in rec["mutants"].items()}
    mutants = {}
    for m, (what, _, _) in B.MUTANTS.items():
        ratios = {n: cases[n]["mutant_ratio"][m] for n in cases if m in cases[n]["mutant_ratio"]}
        if ratios:
            best = max(ratios, key=ratios.get)
            mutants[m] = {"what": what, "cases": len(ratios), "best_ratio": ratios[best], "best_case": best, "worst_ratio": min(ratios.values())}
    extra = {}
    if table == "edges":
        # settings that were measured and are not cases: a parameter floor above param_bar is recorded here, and the bar stays
        for c in B.REJECTED:
            rec = B.measure_floor(c)
            rec.update(edge=c["edge"], updates=c["T"] - B.threshold(B.case_cfg(c)),
                       above_param_bar=sorted(o for o, v in rec["floor"].items() if o not in B.LOSSES and v > B.PARAM_BAR))
            extra.setdefault("rejected", {})[c["name"]] = rec
    return {
        **extra,
        "what": "distances are max |x - sac_ref| / max |sac_ref| per array (log_alpha: |x - ref| / max(1, |ref|)); floor: x = sac_ref with exp / log / "
                "cos jittered; mutants: x = a one-line wrong sac_ref; mutant_ratio: the largest distance / bar over the nine observables",
        "jitter_ulp": B.JITTER_ULP, "jitter_seeds": list(B.JITTER_SEEDS), "loss_factor": B.LOSS_FACTOR, "mutant_factor": B.MUTANT_FACTOR,
        "loss_floor": loss_floor, "loss_bar": loss_bar, "param_bar": B.PARAM_BAR, "cases": cases, "mutants": mutants,
    }


def check(prof, table="cases"):
    """the conditions; → list of what fails"""
    bad = []
    for n, rec in prof["cases"].items():
        bad += [f"{n}: the jitter floor of {o} is {rec['floor'][o]}, above param_bar" for o in B.PARAMS + ("log_alpha",)
                if rec["floor"][o] > prof["param_bar"]]
        if not B.edge_met(n, rec["stats"]):
            bad.append(f"{n}: the edge is not met: {rec['stats']}")
    bad += [f"{m}: no case moves an observable past {prof['mutant_factor']} bars (best {r['best_ratio']:.3g})" for m, r in prof["mutants"].items()
            if not r["best_ratio"] >= prof["mutant_factor"]]
    if table == "cases":
        bad += [f"{m}: applies to no case" for m in B.MUTANTS if m not in prof["mutants"]]
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--table", choices=sorted(B.TABLES), default="cases")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    prof = build(args.jobs, args.table)
    with open(args.out or B.TABLES[args.table][1], "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"loss floor {prof['loss_floor']:.3e} -> loss_bar {prof['loss_bar']:.3e}; param_bar {prof['param_bar']:.3e}")
    for n, rec in prof["cases"].items():
        print(f"{n:20s} loss floor {rec['loss_floor']:.3e}  param floors {max(rec['floor'][o] for o in B.PARAMS):.3e}  log_alpha {rec['floor']['log_alpha']:.3e}  {rec['stats']}")
    for m, rec in prof["mutants"].items():
        print(f"{m:4s} best ratio {rec['best_ratio']:.3e} ({rec['best_case']}), worst {rec['worst_ratio']:.3e}, {rec['cases']} cases  {rec['what']}")
    for n, rec in prof.get("rejected", {}).items():
        print(f"rejected {n:16s} param floors {max(rec['floor'][o] for o in B.PARAMS):.3e}  above param_bar: {rec['above_param_bar']}  {rec['stats']}")
    bad = check(prof, args.table)
    for b in bad:
        print("FAILS:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
