#!/usr/bin/env python3
"""What double Q-learning and n-step returns cost per DQN cycle on the GPU, and whether the plain handle kept its speed
-> profiles/dqn_target_bench.json.

Arms, at the reference defaults (ring 10 000, batch 120, an update every 10 steps): uniform (crl_dqn_create), double, n3, n3_double (crl_dqn_create_with,
uniform replay) and per_n3_double (with PEROptions()). They run alternately in one process: a warm-up, then `--repeats` windows of `--steps` env steps
each, a host clock around crl_dqn_run, which ends in a stream synchronise. us per cycle = window time / (steps / train_freq); the median and the
spread over the windows are kept, with the shader clock under load (crl_clock_probe) before and after.

The plain handle against the parent commit: `--parent LIB` names a build of the parent's csrc (scripts/build_variant.sh's layout:
cleanrl.jl_amd/variants/<name>/libcleanrl_hip.so). The parent's library lacks this feature's symbols, so the package cannot load it; both libraries
are therefore driven through the same bare ctypes calls (crl_dqn_create, crl_dqn_init_params, crl_dqn_run), one fresh child process per library
and round, alternating as scripts/ab.sh does, on one box in one run. Each child reports the median of its windows; the JSON keeps every child's
figure, and says whether the in-tree median lies inside the parent's own min..max over its rounds.

usage: python scripts/bench_dqn_target.py [--steps N] [--repeats R] [--rounds K] [--parent LIB] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window_stats(times, cycles):
    return {"us_per_cycle_median": 1e6 * statistics.median(times) / cycles, "us_per_cycle_min": 1e6 * min(times) / cycles,
            "us_per_cycle_max": 1e6 * max(times) / cycles}


def child_arms(steps, repeats):
    import cleanrl_jl_amd as crl
    cfg = crl.DQNConfig(total_timesteps=steps * (repeats + 2))
    clock0 = crl._lib.clock_probe(0)
    T = crl.DQNTargetOptions
    agents = {"uniform": crl.DQNAgent(cfg, seed=1), "double": crl.DQNAgent(cfg, seed=1, target=T(1, True)),
              "n3": crl.DQNAgent(cfg, seed=1, target=T(3, False)), "n3_double": crl.DQNAgent(cfg, seed=1, target=T(3, True)),
              "per_n3_double": crl.DQNAgent(cfg, seed=1, per=crl.PEROptions(), target=T(3, True))}
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
    out = {k: _window_stats(v, steps / cfg.train_freq) for k, v in times.items()}
    out["shader_clock_mhz"] = {"before": dict(zip(("median", "min", "max"), clock0)), "after": dict(zip(("median", "min", "max"), clock1))}
    print("RESULT " + json.dumps(out))


def child_plain(lib_path, steps, repeats):
    """the plain handle through bare ctypes calls that the parent's library has too"""
    import importlib
    from cleanrl_jl_amd import _lib as L
    D = importlib.import_module("cleanrl_jl_amd.dqn")         # the package attribute `dqn` is the function
    lib = C.CDLL(lib_path)
    c = D.DQNConfig(total_timesteps=steps * (repeats + 2))
    cfg = L.CrlDQNConfig(int(c.log_frequencey), int(c.total_timesteps), int(c.buffer_size), int(c.min_buff_size), float(c.lr), int(c.train_freq),
                         int(c.target_net_freq), int(c.batch_size), float(c.gamma), float(c.epsilon_start), float(c.epsilon_end),
                         float(c.epsilon_duration), 200, 0, 1)
    vp = C.c_void_p
    lib.crl_dqn_create.argtypes = [C.POINTER(L.CrlDQNConfig), C.c_int32, C.POINTER(vp)]
    lib.crl_dqn_init_params.argtypes = [vp, C.c_uint64]
    lib.crl_dqn_run.argtypes = [vp, C.c_int64, C.POINTER(L.CrlDQNEpisode), C.c_int32, C.POINTER(C.c_int32), C.POINTER(L.CrlDQNLossRecord), C.c_int32,
                                C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.crl_dqn_destroy.argtypes = [vp]
    h = vp()
    assert lib.crl_dqn_create(C.byref(cfg), 0, C.byref(h)) == 0
    assert lib.crl_dqn_init_params(h, 0) == 0
    eps, ls = (L.CrlDQNEpisode * 8192)(), (L.CrlDQNLossRecord * 4096)()
    ne, nl, taken = C.c_int32(), C.c_int32(), C.c_int64()

    def run():
        assert lib.crl_dqn_run(h, steps, eps, 8192, C.byref(ne), ls, 4096, C.byref(nl), C.byref(taken)) == 0 and taken.value == steps
    run()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        times.append(time.perf_counter() - t0)
    lib.crl_dqn_destroy(h)
    print("RESULT " + json.dumps(_window_stats(times, steps / c.train_freq)))


def _child(args, timeout=600):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(1)
    return json.loads(next(l for l in p.stdout.splitlines() if l.startswith("RESULT "))[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent", default=None, help="the parent commit's libcleanrl_hip.so")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dqn_target_bench.json"))
    ap.add_argument("--child-arms", action="store_true")
    ap.add_argument("--child-plain", default=None)
    args = ap.parse_args()
    if args.child_arms:
        return child_arms(args.steps, args.repeats)
    if args.child_plain:
        return child_plain(args.child_plain, args.steps, args.repeats)
    size = ["--steps", str(args.steps), "--repeats", str(args.repeats)]
    arms = _child(["--child-arms"] + size)
    base = arms["uniform"]["us_per_cycle_median"]
    for k, v in arms.items():
        if k != "shader_clock_mhz":
            v["over_uniform_percent"] = 100.0 * (v["us_per_cycle_median"] - base) / base
            print(f"{k:14s} {v['us_per_cycle_median']:.2f} us/cycle ({v['over_uniform_percent']:+.1f} %)")
    prof = {"what": "us per ten-launch DQN cycle at the reference defaults for the TD-target options, alternating windows in one process, and the plain "
                    "handle of this tree against the parent commit's library, alternating child processes (scripts/bench_dqn_target.py)",
            "steps_per_window": args.steps, "windows": args.repeats, "arms": arms}
    if args.parent:
        from cleanrl_jl_amd import _lib as L
        libs = {"parent": os.path.abspath(args.parent), "tree": os.path.abspath(L.LIB_PATH)}
        rounds = {k: [] for k in libs}
        for _ in range(args.rounds):
            for k, path in libs.items():
                rounds[k].append(_child(["--child-plain", path] + size)["us_per_cycle_median"])
        lo, hi = min(rounds["parent"]), max(rounds["parent"])
        med = statistics.median(rounds["tree"])
        prof["plain_handle_vs_parent"] = {"rounds": args.rounds, "us_per_cycle_per_round": rounds,
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
