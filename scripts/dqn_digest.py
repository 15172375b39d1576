#!/usr/bin/env python3
"""SHA-256 of everything a DQN handle lets the host read, after short runs of every handle kind: for comparing two builds of the library bit for
bit where the oracle tests cannot (the PER, C51 and dueling cases meet pow / exp / log, so their tests hold a jitter bar, not equality).
scripts/optim_digest.py's protocol on csrc/dqn.hip.

    python scripts/dqn_digest.py [--json FILE]                                                       # this build
    CRL_LIB_PATH=cleanrl.jl_amd/variants/<name>/libcleanrl_hip.so python scripts/dqn_digest.py       # another one (scripts/build_variant.sh, make OUT=…)

Cases: every case of tests/dqn_per_bar.py, dqn_target_bar.py, c51_bar.py and duel_bar.py, and the two configurations of
tests/test_gpu_dqn.py::test_run_matches_oracle_bit_for_bit. Each handle runs to the end of its case in chunks of 1, 7 and the rest; the digest then
covers both parameter sets, status(), the episode and loss records of every chunk, per_read / target_read / c51_read where the handle has them,
q_values / c51_probs / dueling_streams on eight fixed observations, and one evaluate(envs_per_block + 1 envs, 2 episodes, 50 trace steps) with all
its arrays and its report.

Equal lines = equal bits. Run it twice on one build first: a case whose digest does not reproduce there says nothing about two builds.

    python scripts/dqn_digest.py --compare profiles/dqn_refactor_digest.json tree_1=a.json tree_2=b.json parent_1=c.json parent_2=d.json

merges lists that --json wrote into one record and compares them line for line (exit status 1 unless all are equal)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cleanrl_jl_amd as crl
import oraclelib as O
import dqn_per_bar as PB
import dqn_target_bar as TB
import c51_bar as CB
import duel_bar as DB

L = crl._lib
# eight fixed observations inside and at the edge of CartPole's box: (4, 8), one per column
OBS = np.asfortranarray(np.random.default_rng(5).uniform(-1.0, 1.0, (4, 8)) * np.array([[2.4], [3.0], [0.21], [3.0]]))


def _cfg(ocfg):
    return L.CrlDQNConfig(*[getattr(ocfg, f) for f, _ in O.DQNConfigC._fields_])


def _handle(ocfg, params, per=None, tgt=None, c51=None, dueling=False):
    h = L.DQNHandle(_cfg(ocfg), 0,
                    per=None if per is None else L.CrlDQNPEROptions(per["alpha"], per["beta_start"], per["beta_end"], per["beta_duration"], per["eps"]),
                    target=None if tgt is None else L.CrlDQNTargetOptions(int(tgt["n_step"]), int(tgt["double_q"])),
                    c51=None if c51 is None else L.CrlDQNC51Options(int(c51["n_atoms"]), 0, float(c51["v_min"]), float(c51["v_max"])), dueling=dueling)
    h.write_params(params)
    return h


def _oracle_cfg(**kw):
    T = 4000 if not kw else 1500
    return O.dqn_config(total_timesteps=T, lr=1e-3, seed=21, **kw)


def cases():
    """(name, () -> handle, total_timesteps)"""
    out = []
    for kw in (dict(), dict(batch_size=32, min_buff_size=40, train_freq=3, target_net_freq=9, buffer_size=150, epsilon_duration=300.0, log_frequency=30)):
        ocfg = _oracle_cfg(**kw)
        out.append(("oracle/" + ("small_ring" if kw else "default"), lambda ocfg=ocfg: _handle(ocfg, O.dqn_params(1)), ocfg.total_timesteps))
    for c in PB.CASES:
        out.append(("per/" + c["name"], lambda c=c: _handle(PB.case_cfg(c), PB.case_params(c), per=PB.case_per(c)), PB.case_cfg(c).total_timesteps))
    for c in TB.CASES:
        out.append(("target/" + c["name"], lambda c=c: _handle(TB.case_cfg(c), TB.case_params(c), per=TB.case_per(c), tgt=c["tgt"]),
                    TB.case_cfg(c).total_timesteps))
    for c in CB.CASES:
        out.append(("c51/" + c["name"], lambda c=c: _handle(CB.case_cfg(c), CB.case_params(c), per=CB.case_per(c), tgt=CB.case_tgt(c), c51=CB.case_c51(c)),
                    CB.case_cfg(c).total_timesteps))
    for c in DB.CASES:
        out.append(("duel/" + c["name"], lambda c=c: _handle(DB.case_cfg(c), DB.case_params(c), per=DB.case_per(c), tgt=DB.case_tgt(c), c51=DB.case_c51(c),
                                                             dueling=True), DB.case_cfg(c).total_timesteps))
    return out


def digest_of(h, total):
    sha = hashlib.sha256()

    def add(*arrays):
        for a in arrays:
            sha.update(np.ascontiguousarray(a).tobytes())

    def add_dict(d):
        for k in sorted(d):
            add(np.asarray(d[k]))

    taken_all = 0
    for chunk in (1, 7, total):                                   # the last chunk ends at total_timesteps
        taken, eps, losses = h.run(chunk)
        taken_all += taken
        add(np.array([taken], np.int64), np.array(eps, np.float64).reshape(-1, 4), np.array(losses, np.float64).reshape(-1, 2))
    st = h.status()
    assert taken_all == total == st["global_step"], (taken_all, total, st["global_step"])
    add(*h.read_params())
    add_dict(st)
    if h.per is not None:
        add_dict(h.per_read())
        add_dict(h.per_status())
    if h.target is not None or h.c51 is not None or h.dueling:    # a categorical or a dueling handle always carries target options
        add_dict(h.target_read())
    if h.c51 is not None:
        add_dict(h.c51_read())
        add(h.c51_probs(OBS))
    add(h.q_values(OBS))
    if h.dueling:
        add_dict(h.dueling_streams(OBS))
    ev = h.evaluate(L.dqn_eval_envs_per_block() + 1, 2, seed=11, trace_steps=50)
    add_dict(ev.pop("report"))
    add_dict(ev)
    return sha.hexdigest(), f"{st['n_updates']} updates"


def compare(out, runs):
    """`--compare OUT tree_1=a.json tree_2=b.json parent_1=c.json parent_2=d.json`: the lists that `--json` wrote, merged into one record (the shape of
    profiles/dqn_refactor_digest.json). A case that two runs of one library (names that differ only behind the last `_`) do not reproduce says nothing
    about two builds: it is listed and left out of all_equal. Exit status 1 unless every remaining case is equal in every list and none was left out."""
    loaded = {name: json.load(open(path)) for name, path in (r.split("=", 1) for r in runs)}
    lists = {k: v["digests"] for k, v in loaded.items()}
    names = list(next(iter(lists.values())))
    same_cases = all(list(v) == names for v in lists.values())
    by_lib = {}
    for k in lists:
        by_lib.setdefault(k.rsplit("_", 1)[0], []).append(k)
    unstable = {lib: [n for n in names if len({lists[k].get(n) for k in ks}) != 1] for lib, ks in by_lib.items()}
    left_out = sorted({n for v in unstable.values() for n in v})
    differing = [n for n in names if n not in left_out and len({v.get(n) for v in lists.values()}) != 1]
    rec = {"what": "scripts/dqn_digest.py, one fresh process per list; SHA-256 per case over everything the handle lets the host read (the script's docstring)",
           "cases": len(names), "libraries": {k: v["library"] for k, v in loaded.items()}, "seconds": {k: round(v["seconds"], 2) for k, v in loaded.items()},
           "digests": lists, "not_reproduced": unstable, "differing": differing, "all_equal": same_cases and not differing and not left_out}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{len(names)} cases x {len(lists)} lists; not reproduced by one library: {left_out}; differing between lists: {differing}; "
          f"all equal: {rec['all_equal']}")
    return 0 if rec["all_equal"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write {case: digest} and the run time to this file")
    ap.add_argument("--compare", nargs="+", metavar=("OUT", "NAME=FILE"), default=None, help="merge and compare lists written by --json (no GPU needed)")
    ap.add_argument("names", nargs="*", help="case names (default: all)")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1:]))
    print("library:", os.environ.get("CRL_LIB_PATH", "this build"), flush=True)
    t0 = time.perf_counter()
    digests = {}
    for name, make, total in cases():
        if args.names and name not in args.names:
            continue
        h = make()
        digests[name], note = digest_of(h, total)
        h.close()
        print(f"{name:36s} {digests[name]}  ({note})", flush=True)
    seconds = time.perf_counter() - t0
    print(f"{len(digests)} cases in {seconds:.1f} s", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"library": os.environ.get("CRL_LIB_PATH", "this build"), "seconds": seconds, "digests": digests}, f, indent=1)
            f.write("\n")
