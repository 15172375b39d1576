#!/usr/bin/env python3
"""Measures what the noisy-layer parity bars are worth, on the CPU, and writes profiles/noisy_bar.json — scripts/duel_bar.py for tests/noisy_bar.py's
table.

For every case that runs a transcendental (pow under PER, exp / log on the categorical head): the jitter floor — tests/noisy_ref.py against a twin
whose every exp, log and pow result is moved by -2..+2 ulp, three seeds, the maximum; the device's own error in the three has not been measured — and
whether every twin replayed the base run's episodes. The uniform scalar cases run none, so their floor is 0 by construction and is not measured (the GPU
test asks them for bit-equality). Then loss_bar = 32 x the largest loss floor, proj_bar = 32 x the largest floor of the projected targets, param_bar =
2^-21 for mu, sigma and both images, and the conditions are checked: every twin stayed on the base run's episodes and every parameter and image floor
lies under param_bar. The script fails otherwise — then the case (its seed), not the bar, changes. Everything is seeded.

usage: python scripts/noisy_bar.py [--jobs N] [--out FILE]"""
import argparse
import json
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import noisy_bar as B   # noqa: E402

PARAMS = ("q", "target", "image_q", "image_t")


def _measure(name):
    return name, B.measure(B.CASE[name])


def build(jobs):
    names = [c["name"] for c in B.CASES if c["name"] not in B.EXACT]
    with multiprocessing.Pool(jobs) as pool:
        cases = dict(pool.map(_measure, names, chunksize=1))
    loss_floor = max(cases[n]["floor"]["loss"] for n in cases)
    proj_floor = max(cases[n]["floor"]["proj"] for n in cases)
    for n in cases:
        c = B.CASE[n]
        cfg = B.case_cfg(c)
        cases[n].update(batch_size=cfg.batch_size, buffer_size=cfg.buffer_size, seed=c["seed"], per=B.case_per(c), tgt=B.case_tgt(c), c51=B.case_c51(c),
                        dueling=c["dueling"], edge=c["edge"])
    return {
        "what": "distances: loss max |x - ref| / max |ref| over the logged losses; q, target (mu then sigma) and image_q, image_t max |x - ref| / max "
                "|ref| per array; proj max |x - ref| of the last update's projected targets (0 on a scalar head). floor: x = noisy_ref with exp, log "
                "and pow jittered (scripts/noisy_bar.py)",
        "jitter_ulp": B.JITTER_ULP, "jitter_ulp_source": "ddpg_bar.JITTER_ULP, the amplitude this suite assumes for exp, log and pow; the device's own "
                                                         "error has not been measured",
        "jitter_seeds": list(B.JITTER_SEEDS), "loss_factor": B.LOSS_FACTOR, "mutant_factor": B.MUTANT_FACTOR,
        "loss_floor": loss_floor, "loss_bar": B.LOSS_FACTOR * loss_floor, "proj_floor": proj_floor, "proj_bar": B.LOSS_FACTOR * proj_floor,
        "param_bar": B.PARAM_BAR, "exact_cases": list(B.EXACT), "cases": cases,
    }


def check(prof):
    bad = []
    for n, rec in prof["cases"].items():
        if not rec["same_episodes"]:
            bad.append(f"{n}: a jittered twin left the base run's episodes: change the case's seed")
        bad += [f"{n}: the jitter floor of {o} is {rec['floor'][o]:.3g}, above param_bar" for o in PARAMS if not rec["floor"][o] <= prof["param_bar"]]
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
    bad = check(prof)
    for b in bad:
        print("FAILS:", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
