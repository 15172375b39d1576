#!/usr/bin/env python3
"""What a held-out DDPG evaluation costs, on one box, in one process (→ profiles/ddpg_eval_cost.json):

    (a) crl_ddpg_evaluate at 256 x 1 and at 4096 x 1 episodes of 200 steps  (csrc/ddpg.hip, ddpg_eval_kernel: one launch, the actor on the chip)
    (b) the same 256-env evaluation without that call: a host loop of 200 crl_ddpg_actor(n = 256) calls around a numpy Pendulum (vectorised over
        the envs, the same Float64 operations in the same order), plus one crl_ddpg_q_values — all a user could do before
    (c) the training cycle (one env step + one 120-sample update, six dependent launches) by scripts/bench_ddpg.py's method: the timed region
        starts after the warm-up, wall clock around crl_ddpg_run

Wall clock around each call (every one of them synchronises before it returns), median of RUNS calls after one warm-up call; (a) includes the
call's host work (result arrays, three device-to-host copies, the Float64 report). (a) and (b) must agree bit for bit on returns, discounted
returns and q0, or the script fails: a faster number for another result is no number.

    python scripts/ddpg_eval_cost.py [--out profiles/ddpg_eval_cost.json]"""
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cleanrl_jl_amd as crl  # noqa: E402

RUNS, STEPS, SEED, S_EVAL = 7, 200, 0xE7A1, 0x16
PI = 3.141592653589793
SIN_C = [(-1.0 if i % 2 == 0 else 1.0) / float(math.factorial(2 * i + 3)) for i in range(14)]
COS_C = [(-1.0 if i % 2 == 0 else 1.0) / float(math.factorial(2 * i + 2)) for i in range(14)]


def horner(c, x2):
    p = np.full_like(x2, c[13])
    for i in range(12, -1, -1):
        p = p * x2 + c[i]
    return p


def host_loop(h, n, gamma):
    """(b): n envs x 1 episode with the forwards on the device and everything else here — the reset draw, the Pendulum and the sums as the header
    defines them, vectorised over the envs"""
    th, thd = reset_states(n)
    ret = np.zeros(n); disc_ret = np.zeros(n); disc = np.float64(1.0); q0 = None
    for t in range(STEPS):
        x2 = th * th
        obs = np.stack([1.0 + x2 * horner(COS_C, x2), th + (th * x2) * horner(SIN_C, x2), thd])
        a = h.actor(obs)[0]
        if t == 0:
            q0 = h.q_values(obs, a[None, :])
        u = np.clip(a, -2.0, 2.0)
        cost = th * th + 0.1 * (thd * thd) + 0.001 * (u * u)
        thd = np.clip(thd + (15.0 * obs[1] + 3.0 * u) * 0.05, -8.0, 8.0)
        th = th + thd * 0.05
        th = np.where(th >= PI, th - 2.0 * PI, np.where(th < -PI, th + 2.0 * PI, th))
        ret = ret + -cost; disc_ret = disc_ret + disc * -cost; disc = disc * gamma
    return ret, disc_ret, q0


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words"""
    M = 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0; p1 = np.uint64(0xCD9E8D57) * c2
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & np.uint64(M), p1 >> np.uint64(32), p1 & np.uint64(M)
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0 = (k0 + 0x9E3779B9) & M; k1 = (k1 + 0xBB67AE85) & M
    return c0, c1


def reset_states(n):
    """the evaluation reset of env e, episode 0: components 0 and 1 of the Philox draw at (key = SEED, gstep = e, stream 0x16)"""
    g = np.arange(n, dtype=np.uint64)
    u = []
    for comp in (0, 1):
        x, y = philox(np.full_like(g, comp), g, np.zeros_like(g), np.full_like(g, S_EVAL), SEED & 0xFFFFFFFF, SEED >> 32)
        u.append((((x << np.uint64(32)) | y) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)
    return -PI + (2.0 * PI) * u[0], -1.0 + 2.0 * u[1]


def timed(fn):
    fn()                                            # warm-up: first-use allocations, code load
    out = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        res = fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out), res


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ddpg_eval_cost.json")
    clock = crl._lib.clock_probe(0)
    # a trained-for-a-while agent at the reference defaults: (c) is measured on the way
    n_upd = 6000
    cfg = crl.DDPGConfig(total_timesteps=2500 + 2000 + n_upd)
    agent = crl.DDPGAgent(cfg, seed=1)
    h = agent.handle
    h.run(2500 + 2000)
    cycles = []
    for _ in range(3):
        s0 = h.status(); t0 = time.perf_counter()
        h.run(n_upd // 3)
        dt = time.perf_counter() - t0
        cycles.append(dt / (h.status()["global_step"] - s0["global_step"]))
    cycle = statistics.median(cycles)

    a256 = timed(lambda: h.evaluate(256, 1, SEED))
    a4096 = timed(lambda: h.evaluate(4096, 1, SEED))
    b256 = timed(lambda: host_loop(h, 256, np.float64(cfg.gamma)))
    dev, (ret, disc_ret, q0) = a256[3], b256[3]
    same = bool(np.array_equal(dev["returns"][0], ret) and np.array_equal(dev["disc_returns"][0], disc_ret) and np.array_equal(dev["q0"][0], q0))
    agent.close()

    def entry(t, envs):
        return {"envs": envs, "episodes_per_env": 1, "steps_per_episode": STEPS, "median_ms": t[0] * 1e3, "min_ms": t[1] * 1e3, "max_ms": t[2] * 1e3,
                "us_per_sequential_step": t[0] * 1e6 / STEPS, "env_steps_per_s": envs * STEPS / t[0], "training_cycles": t[0] / cycle}
    out = {"what": "wall clock per call, median of %d after one warm-up call (scripts/ddpg_eval_cost.py); every call synchronises before it returns" % RUNS,
           "a_crl_ddpg_evaluate": [entry(a256, 256), entry(a4096, 4096)],
           "b_host_loop_of_crl_ddpg_actor": entry(b256, 256),
           "c_training_cycle_us": cycle * 1e6,
           "b_over_a_at_256_envs": b256[0] / a256[0],
           "a_and_b_bit_identical": same,
           "report_256": dev["report"],
           "shader_clock_mhz": {"median": clock[0], "min": clock[1], "max": clock[2]}}
    print(json.dumps(out))
    assert same, "the host loop and crl_ddpg_evaluate disagree"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
