#!/usr/bin/env python3
"""SHA-256 of everything a DDPG, TD3 or SAC handle lets the host read, after short runs of every handle kind: for comparing two builds of the
library bit for bit where the GPU tests cannot (the family's tests hold jitter bars against Float64 references, not equality).
scripts/dqn_digest.py's protocol on csrc/ddpg.hip and csrc/sac.hpp.

    python scripts/ddpg_digest.py [--json FILE]                                                      # this build
    CRL_LIB_PATH=cleanrl.jl_amd/variants/<name>/libcleanrl_hip.so python scripts/ddpg_digest.py      # another one (scripts/build_variant.sh, make OUT=…)

Cases: every case of tests/ddpg_bar.py's CASES and of tests/td3_bar.py's and tests/sac_bar.py's CASES and EDGE_CASES, on a host-driven handle fed
through act / observe as the tests' feed helpers do (read at the last quiet step, the first update, the middle and the end), and one Pendulum
handle per kind and setting (DDPG with noise_in_update 0 and 1, TD3 with policy_delay 1 and 2, SAC with autotune on and off), run in chunks of 1, 7
and the rest with a short warm-up. The digest covers read_params, status (and sac_status), the loss, episode and alpha records of every chunk,
buffer(), actor and q_values / q_values_both on eight fixed observations and, on the Pendulum handles, one evaluate(CRL_EVAL_WAVES + 1 envs,
2 episodes, 50 trace steps) with all its arrays and its report.

Equal lines = equal bits. Run it twice on one build first: a case whose digest does not reproduce there says nothing about two builds.

    python scripts/ddpg_digest.py --compare profiles/ddpg_refactor_digest.json tree_1=a.json tree_2=b.json parent_1=c.json parent_2=d.json

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

EVAL_WAVES = 4                                               # csrc/ddpg.hip's default CRL_EVAL_WAVES: the evaluation spans two blocks
PENDULUM_STEPS = 400
PENDULUM = dict(warmup_steps=50, min_buff_size=60, batch_size=32, seed=5, log_frequency=7)   # 340 updates


def _cfg(L, d, external):
    return L.CrlDDPGConfig(d["total_timesteps"], d["buffer_size"], d["min_buff_size"], d["batch_size"], d["warmup_steps"], d["log_frequency"], d["lr"],
                           d["tau"], d["gamma"], d["exploration_noise"], d["obs_dim"], d["act_dim"],
                           L.DDPG_ENV_EXTERNAL if external else L.DDPG_ENV_PENDULUM, d["max_steps"], d["act_low"], d["act_high"],
                           d["noise_in_update"], 0, d["seed"])


def _handle(L, kind, d, external, nets):
    """kind: "ddpg", "td3" or "sac"; d: the config dict with the kind's option fields in it"""
    c = _cfg(L, d, external)
    if kind == "td3":
        h = L.TD3Handle(c, L.CrlTD3Options(d["policy_delay"], 0, d["policy_noise"], d["noise_clip"]), 0)
    elif kind == "sac":
        h = L.SACHandle(c, L.CrlSACOptions(d["autotune"], 0, d["alpha"], d["target_entropy"]), 0)
    else:
        h = L.DDPGHandle(c, 0)
    h.write_params(*nets)
    return h


def cases(L):
    """(name, kind, () -> handle, the case or None for a Pendulum handle, config dict)"""
    import ddpg_bar as DB
    import sac_bar as SB
    import td3_bar as TB
    out = []
    for kind, mod, tables in (("ddpg", DB, (("cases", DB.CASES),)), ("td3", TB, (("cases", TB.CASES), ("edges", TB.EDGE_CASES))),
                              ("sac", SB, (("cases", SB.CASES), ("edges", SB.EDGE_CASES)))):
        for table, cs in tables:
            for c in cs:
                d = mod.case_cfg(c)
                out.append((f"{kind}/{table}/{c['name']}", kind, lambda kind=kind, mod=mod, c=c, d=d: _handle(L, kind, d, True, mod.case_params(c)), c, d))
    pend = dict(name="pendulum", D=3, A=1, T=PENDULUM_STEPS, terminal="some", kw={}, mu_gain=1.0, s_gain=1.0, mu_shift=0.0)
    for kind, mod, settings in (("ddpg", DB, (dict(noise_in_update=0), dict(noise_in_update=1))), ("td3", TB, (dict(policy_delay=1), dict(policy_delay=2))),
                                ("sac", SB, (dict(autotune=1), dict(autotune=0, alpha=0.2)))):
        for kw in settings:
            d = mod.case_cfg(dict(pend, kw=dict(PENDULUM, **kw)))
            tag = "_".join(f"{k}{v}" for k, v in kw.items() if k != "alpha")
            out.append((f"{kind}/pendulum/{tag}", kind, lambda kind=kind, mod=mod, d=d: _handle(L, kind, d, False, mod.case_params(pend)), None, d))
    return out


def digest_of(h, kind, case, d):
    import ddpg_bar as DB
    sha = hashlib.sha256()

    def add(*arrays):
        for a in arrays:
            sha.update(np.ascontiguousarray(a).tobytes())

    def add_dict(x):
        for k in sorted(x):
            add(np.asarray(x[k]))

    def add_records(losses):
        add(np.array(losses, np.float64).reshape(-1, 3))
        if kind == "sac":
            add(np.array(h.alpha_records(), np.float64).reshape(-1, 4))

    D, A, T = d["obs_dim"], d["act_dim"], d["total_timesteps"]
    if case is not None:                                         # the tests' feed: observe up to each checkpoint, act on the segment's first observation
        trs, thr, i = DB.case_transitions(case), DB.threshold(d), 0
        for end in sorted({1, thr, thr + 1, (thr + T) // 2, T}):
            add(h.act(trs[i][0]))
            for tr in trs[i:end]:
                h.observe(*tr)
            i = end
            add_dict(h.status())
            add_records(h.read_losses())
    else:
        taken_all = 0
        for chunk in (1, 7, T):                                  # the last chunk ends at total_timesteps
            taken, eps, losses = h.run(chunk)
            taken_all += taken
            add(np.array([taken], np.int64), np.array(eps, np.float64).reshape(-1, 3))
            add_records(losses)
        assert taken_all == T, (taken_all, T)
    st = h.status()
    assert st["global_step"] == T and st["n_updates"] == T - DB.threshold(d), st
    add(*h.read_params())
    add_dict(st)
    if kind == "sac":
        add_dict(h.sac_status())
    add_dict(h.buffer())
    rng = np.random.default_rng([5, D, A])                       # eight fixed observations and actions, one per column
    obs, act = np.asfortranarray(rng.standard_normal((D, 8))), np.asfortranarray(rng.uniform(-2.0, 2.0, (A, 8)))
    add(h.actor(obs), h.q_values(obs, act))
    if kind != "ddpg":
        add(*h.q_values_both(obs, act))
    if case is None:
        ev = h.evaluate(EVAL_WAVES + 1, 2, seed=11, trace_steps=50)
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
    rec = {"what": "scripts/ddpg_digest.py, one fresh process per list; SHA-256 per case over everything the handle lets the host read (the script's docstring)",
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
    import cleanrl_jl_amd as crl
    print("library:", os.environ.get("CRL_LIB_PATH", "this build"), flush=True)
    t0 = time.perf_counter()
    digests = {}
    for name, kind, make, case, d in cases(crl._lib):
        if args.names and name not in args.names:
            continue
        h = make()
        digests[name], note = digest_of(h, kind, case, d)
        h.close()
        print(f"{name:36s} {digests[name]}  ({note})", flush=True)
    seconds = time.perf_counter() - t0
    print(f"{len(digests)} cases in {seconds:.1f} s", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"library": os.environ.get("CRL_LIB_PATH", "this build"), "seconds": seconds, "digests": digests}, f, indent=1)
            f.write("\n")
