#!/usr/bin/env python3
"""Measures what the TD3 parity bars are worth, on the CPU, and writes profiles/td3_bar.json — scripts/ddpg_bar.py for tests/td3_bar.py's table.

For every case: the jitter floor (tests/td3_ref.py against a twin whose every exp / log / cos result is moved by -2..+2 ulp, three seeds, the
maximum), the reference's own statistics of the case (actor steps, smoothing draws and how many the noise clip cut, target actions and how many the
action bounds cut) and the distance of every applicable one-line mutant. Then loss_bar = 32 x the largest loss floor over this table, param_bar =
2^-21, and the conditions the table has to meet are checked: every parameter floor is exactly 0.0, every applicable mutant moves at least one of
the eight observables past 10x its bar in every case, and the cases built around an edge met it. The script fails otherwise — then the case, not
the bar, changes. Everything is seeded: a second run writes the same bytes.

--table edges does the same for the second table (EDGE_CASES, with the mutants T10 and T11 next to T1 to T9) and writes profiles/td3_edges_bar.json:
a loss bar of its own, the same param_bar, and that table's conditions (kmax_a16's clip and clamp bind, bounds_a6's clamp binds on a part, the three
ring cases draw more than one round of candidates).

usage: python scripts/td3_bar.py [--table cases|edges] [--jobs N] [--out FILE]"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import td3_bar as B   # noqa: E402


def _measure(job):
    table, name = job
    table_cases, mutants, _ = B.TABLES[table]
    return name, B.measure(next(c for c in table_cases if c["name"] == name), mutants)


def build(jobs, table="cases"):
    table_cases, table_mutants, _ = B.TABLES[table]
    with multiprocessing.Pool(jobs) as pool:
        cases = dict(pool.map(_measure, [(table, c["name"]) for c in table_cases], chunksize=1))
    loss_floor = max(cases[n]["floor"][o] for n in cases for o in B.LOSSES)
    loss_bar = B.LOSS_FACTOR * loss_floor
    for c in table_cases:
        rec = cases[c["name"]]
        d = B.case_cfg(c)
        rec.update(D=c["D"], A=c["A"], batch_size=d["batch_size"], updates=c["T"] - B.threshold(d), policy_delay=d["policy_delay"], edge=c["edge"])
        rec["mutant_ratio"] = {m: B.mutant_ratio(dist, loss_bar) for m, dist in rec["mutants"].items()}
    mutants = {}
    for m, (what, _, _) in table_mutants.items():
        ratios = {n: cases[n]["mutant_ratio"][m] for n in cases if m in cases[n]["mutant_ratio"]}
        worst = min(ratios, key=ratios.get)
        mutants[m] = {"what": what, "cases": len(ratios), "worst_ratio": ratios[worst], "worst_case": worst}
    return {
        "what": "distances are max |x - td3_ref| / max |td3_ref| per array; floor: x = td3_ref with exp / log / cos jittered; mutants: x = a one-line "
                "wrong td3_ref; mutant_ratio: the largest distance / bar over the eight observables (scripts/td3_bar.py)",
        "jitter_ulp": B.JITTER_ULP, "jitter_seeds": list(B.JITTER_SEEDS), "loss_factor": B.LOSS_FACTOR, "mutant_factor": B.MUTANT_FACTOR,
        "loss_floor": loss_floor, "loss_bar": loss_bar, "param_bar": B.PARAM_BAR, "cases": cases, "mutants": mutants,
    }


def check_edges(prof):
    """the edges the second table is built around, on the reference's own statistics; → list of what fails"""
    bad = []
    st = prof["cases"]["kmax_a16"]["stats"]
    if not 0.1 * st["n_noise"] <= st["n_noise_clipped"] <= 0.9 * st["n_noise"]:
        bad.append(f"kmax_a16: {st['n_noise_clipped']} of {st['n_noise']} draws clipped, not between 10 % and 90 %")
    if not st["n_target_clamped"] > 0:
        bad.append("kmax_a16: the clamp of the target action never binds")
    st = prof["cases"]["bounds_a6"]["stats"]
    if not 0 < st["n_target_clamped"] < st["n_target_actions"]:
        bad.append(f"bounds_a6: the clamp binds on {st['n_target_clamped']} of {st['n_target_actions']} target actions")
    for n in B.EDGE_MULTI_ROUND:
        most = max(B.case_candidates(B.EDGE_CASE[n]))
        if not most > 1024:
            bad.append(f"{n}: no draw needs more than {most} candidates, one round of 1024 is enough")
    return bad


def check(prof, table="cases"):
    """the conditions; → list of what fails"""
    bad = []
    for n, rec in prof["cases"].items():
        bad += [f"{n}: the jitter floor of {o} is {rec['floor'][o]}, not 0.0" for o in B.PARAMS if rec["floor"][o] != 0.0]
        bad += [f"{n}: {m} moves no observable past {prof['mutant_factor']} bars (ratio {r:.3g})" for m, r in rec["mutant_ratio"].items()
                if not r >= prof["mutant_factor"]]
    if table == "edges":
        return bad + check_edges(prof)
    st = prof["cases"]["noise1_clip05"]["stats"]
    if not 0.1 * st["n_noise"] <= st["n_noise_clipped"] <= 0.9 * st["n_noise"]:
        bad.append(f"noise1_clip05: {st['n_noise_clipped']} of {st['n_noise']} draws clipped, not between 10 % and 90 %")
    st = prof["cases"]["bounds"]["stats"]
    if not 0 < st["n_target_clamped"] < st["n_target_actions"]:
        bad.append(f"bounds: the clamp binds on {st['n_target_clamped']} of {st['n_target_actions']} target actions")
    if prof["cases"]["delay_never"]["stats"]["n_actor_steps"] != 0:
        bad.append("delay_never: the actor stepped")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--table", choices=sorted(B.TABLES), default="cases", help="cases: tests/td3_bar.py's CASES; edges: its EDGE_CASES, T10 and T11")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    prof = build(args.jobs, args.table)
    with open(args.out or B.TABLES[args.table][2], "w") as f:
        json.dump(prof, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"loss floor {prof['loss_floor']:.3e} -> loss_bar {prof['loss_bar']:.3e}; param_bar {prof['param_bar']:.3e}")
    for m, rec in prof["mutants"].items():
        print(f"{m:4s} worst ratio {rec['worst_ratio']:.3e} ({rec['worst_case']}, {rec['cases']} cases)  {rec['what']}")
    bad = check(prof, args.table)
    for b in bad:
        print("FAILS:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
