#!/usr/bin/env python3
"""What a held-out DQN / A2C evaluation costs, on one box (→ profiles/value_eval_cost.json):

    (a) crl_dqn_evaluate and crl_a2c_evaluate at 256 x 1 and at 4096 x 1 episodes (csrc/dqn.hip dqn_eval_kernel around csrc/dqn_loops.hpp dqn_eval_episodes, csrc/a2c.hip a2c_eval_kernel: one
        launch, the network on the chip), for two policies, because the policy decides how many steps the launch runs: a fresh glorot / orthogonal
        net, whose episodes are short, and the hand-made balancer of tests/value_eval_ref.py, whose episodes all run into the step limit
        (201 steps for DQN's max_steps = 200, 501 for A2C's 500); A2C also sampled
    (b) DQN only — A2C had no public forward before, so there is no earlier route to compare with: the same 256-env evaluation without that call, a
        host loop of one crl_dqn_q_values(n = 256) call per step around the Float64 CartPole of the tests (the oracle's a2c_cartpole_step, env by
        env through ctypes), all a user could do before. Its time is split into the crl_dqn_q_values calls (one launch plus two copies each) and the
        rest (the host env)
    (c) the training cycle of the same handle: DQN train_freq = 10 env steps plus one 120-sample update (wall clock around crl_dqn_run after the
        ring has filled), A2C one crl_a2c_run_until_update call that ends in an update (> 512 env steps plus the update)
    (d) envs per block: the same calls on experiment builds of the library (scripts/build_variant.sh ew<n> "-DCRL_DQN_EVAL_WAVES=n
        -DCRL_A2C_EVAL_WAVES=n" "dqn a2c"), each in a fresh process through CRL_LIB_PATH, the builds alternating twice

Wall clock around each call (every one of them synchronises before it returns), median of RUNS calls after one warm-up call; (a) includes the call's
host work (result arrays, the device-to-host copies, the Float64 report). (a) and (b) must agree bit for bit on returns, lengths, discounted returns
and q0, or the script fails: a faster number for another result is no number.

    python scripts/value_eval_cost.py [--out profiles/value_eval_cost.json] [--variants 1=path/to/lib.so,2=...,8=...]
    python scripts/value_eval_cost.py --probe        (what (d) runs in each child process: the (a) timings of the loaded library, one JSON line)"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cleanrl_jl_amd as crl  # noqa: E402
import value_eval_ref as V  # noqa: E402

RUNS, SEED = 7, 0xE7A1
SIZES = (256, 4096)


def timed(fn, runs=RUNS):
    fn()                                            # warm-up: first-use allocations, code load
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        res = fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out), res


def entry(t, envs):
    rep = t[3]["report"]
    e = {"envs": envs, "episodes_per_env": 1, "length_mean": rep["length_mean"], "env_steps": rep["env_steps"], "return_mean": rep["return_mean"],
         "median_ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3, "env_steps_per_s": rep["env_steps"] / t[0]}
    return e


def agents():
    """(DQN agent, A2C agent) at the reference defaults, fresh parameters"""
    return crl.DQNAgent(crl.DQNConfig(), seed=1), crl.A2CAgent(crl.A2CConfig(), seed=1)


def eval_timings(dqn, a2c):
    """(a): every policy x size of both algorithms"""
    L = crl._lib
    out = {"dqn": {}, "a2c": {}}
    fresh_q, fresh_a = dqn.handle.read_params()[0], a2c.handle.read_params()
    for name, params in (("fresh_net", fresh_q), ("balancer", V.dqn_balancer())):
        dqn.handle.write_params(params)
        out["dqn"][name] = [entry(timed(lambda: dqn.handle.evaluate(n, 1, SEED)), n) for n in SIZES]
    for name, params, mode in (("fresh_net", fresh_a, L.EVAL_GREEDY), ("fresh_net_sampled", fresh_a, L.EVAL_SAMPLE), ("balancer", V.a2c_balancer(), L.EVAL_GREEDY)):
        a2c.handle.write_params(params)
        out["a2c"][name] = [entry(timed(lambda: a2c.handle.evaluate(n, 1, mode, SEED)), n) for n in SIZES]
    dqn.handle.write_params(fresh_q); a2c.handle.write_params(fresh_a)
    return out


def host_loop(h, n, max_steps, gamma):
    """(b): n envs x 1 episode with the forward on the device and everything else here — the reset draw, the oracle's CartPole and the sums as the
    header defines them. → (returns, lengths, disc_returns, q0, seconds spent inside crl_dqn_q_values)"""
    s = np.stack([V.reset(SEED, e) for e in range(n)])                      # (n, 4), episode 0 of env e: gstep = e
    t = np.zeros(n, np.int32); alive = np.ones(n, bool)
    ret, disc_ret, q0, length, disc = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.float64(1.0)
    in_q = 0.0
    while alive.any():
        t0 = time.perf_counter()
        q = h.q_values(s.T)                                                  # one launch + two copies for all n envs, finished ones included
        in_q += time.perf_counter() - t0
        action = (q[1] > q[0]).astype(np.int32)
        if length.max() == 0:
            q0 = q[action, np.arange(n)]
        for e in np.flatnonzero(alive):
            row = np.ascontiguousarray(s[e])
            t[e], done = V.step(row, int(t[e]), int(action[e]), max_steps)
            s[e] = row
            rew = np.float64(0.0 if done else 1.0)
            ret[e] = ret[e] + rew; disc_ret[e] = disc_ret[e] + disc * rew; length[e] += 1
            alive[e] = not done
        disc = disc * gamma                                                   # every env is on the same step of its one episode
    return ret, length, disc_ret, q0, in_q


def training_cycles(dqn, a2c):
    """(c) → (seconds per DQN cycle of train_freq steps + one update, seconds per A2C collect-and-update call)"""
    h = dqn.handle
    h.run(1000)                                                              # past min_buff_size = 200: every 10th step trains
    per = []
    for _ in range(3):
        t0 = time.perf_counter(); taken = h.run(2000)[0]; per.append((time.perf_counter() - t0) / (taken / dqn.config.train_freq))
    a = a2c.handle
    a.run_until_update()
    calls = []
    for _ in range(5):
        t0 = time.perf_counter(); _, ts, _ = a.run_until_update(); dt = time.perf_counter() - t0
        if ts["trained"]:
            calls.append(dt)
    return statistics.median(per), statistics.median(calls)


def probe():
    dqn, a2c = agents()
    out = eval_timings(dqn, a2c)
    out["envs_per_block"] = {"dqn": crl._lib.dqn_eval_envs_per_block(), "a2c": crl._lib.a2c_eval_envs_per_block()}
    dqn.close(); a2c.close()
    print(json.dumps(out))


def main():
    if "--probe" in sys.argv:
        return probe()
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "value_eval_cost.json")
    variants = dict(kv.split("=", 1) for kv in sys.argv[sys.argv.index("--variants") + 1].split(",")) if "--variants" in sys.argv else {}
    clock = crl._lib.clock_probe(0)
    dqn, a2c = agents()
    fresh_q = dqn.handle.read_params()[0]
    # (b) against (a), on both policies, before any training moves the parameters
    b = {}
    for name, params in (("fresh_net", fresh_q), ("balancer", V.dqn_balancer())):
        dqn.handle.write_params(params)
        tb = timed(lambda: host_loop(dqn.handle, 256, 200, np.float64(dqn.config.gamma)), runs=3)
        dev = dqn.handle.evaluate(256, 1, SEED)
        ret, length, disc_ret, q0, in_q = tb[3]
        same = bool(np.array_equal(dev["returns"][0], ret) and np.array_equal(dev["lengths"][0], length) and
                    np.array_equal(dev["disc_returns"][0], disc_ret) and np.array_equal(dev["q0"][0], q0))
        assert same, "the host loop and crl_dqn_evaluate disagree"
        b[name] = {"envs": 256, "sequential_steps": int(length.max()), "median_ms": tb[0] * 1e3, "min_ms": tb[1] * 1e3, "max_ms": tb[2] * 1e3,
                   "ms_inside_crl_dqn_q_values": in_q * 1e3, "bit_identical_to_crl_dqn_evaluate": same}
    dqn.handle.write_params(fresh_q)
    a = eval_timings(dqn, a2c)                                               # fresh parameters: the reference's starting point
    cyc = training_cycles(dqn, a2c)
    for algo, cycle in zip(("dqn", "a2c"), cyc):                             # (c): the same calls in training cycles of the same handle
        for entries in a[algo].values():
            for e in entries:
                e["training_cycles"] = e["median_ms"] * 1e-3 / cycle
    for name in b:
        b[name]["over_crl_dqn_evaluate_at_256_envs"] = b[name]["median_ms"] / a["dqn"][name][0]["median_ms"]
        b[name]["q_values_calls_over_crl_dqn_evaluate"] = b[name]["ms_inside_crl_dqn_q_values"] / a["dqn"][name][0]["median_ms"]
    dqn.close(); a2c.close()
    ablation = []
    for _ in range(2 if variants else 0):                                     # alternating twice, a fresh process per build
        for n, path in [("default", None)] + sorted(variants.items()):
            env = dict(os.environ)
            if path:
                env["CRL_LIB_PATH"] = os.path.abspath(path)
            r = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--probe"], env=env, check=True, capture_output=True,
                                          text=True, timeout=300).stdout.strip().splitlines()[-1])
            ablation.append({"build": n, "envs_per_block": r["envs_per_block"],
                             **{f"{algo}_{name}_ms_{e['envs']}": round(e["median_ms"], 4) for algo in ("dqn", "a2c") for name in r[algo] for e in r[algo][name]},
                             "dqn_balancer_return_mean_4096": r["dqn"]["balancer"][1]["return_mean"],
                             "a2c_fresh_net_return_mean_4096": r["a2c"]["fresh_net"][1]["return_mean"]})
    out = {"what": "wall clock per call, median of %d after one warm-up call (scripts/value_eval_cost.py); every call synchronises before it returns; "
                   "1 episode per env; DQN max_steps 200, A2C 500" % RUNS,
           "a_crl_dqn_evaluate": a["dqn"], "a_crl_a2c_evaluate": a["a2c"],
           "b_host_loop_of_crl_dqn_q_values": b,
           "c_training_cycle_us": {"dqn_10_steps_and_one_update": cyc[0] * 1e6, "a2c_collect_and_update_call": cyc[1] * 1e6},
           "d_envs_per_block": ablation,
           "shader_clock_mhz": {"median": clock[0], "min": clock[1], "max": clock[2]}}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
