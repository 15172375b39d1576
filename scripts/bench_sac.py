#!/usr/bin/env python3
"""SAC side measurement, next to DDPG's and TD3's from the same box and the same run: env-steps/s of the whole loop on the library's Pendulum at the
reference defaults (batch 120, one update per env step after warmup_steps = 2500) and the µs per cycle that is. A cycle is six launches for all
three; SAC's actor pass runs on every cycle (TD3 is measured at policy_delay 1, the like-for-like setting, and at its default 2), on two waves per
sample with one more exp and log per component. Writes profiles/sac_bench.json with the box's shader clock.

    python scripts/bench_sac.py [update_steps]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import cleanrl_jl_amd as crl

N_UPD = int(sys.argv[1]) if len(sys.argv) > 1 else 30_000
clock = crl._lib.clock_probe(0)
TOTAL = 2500 + 2000 + N_UPD


def whole_loop(agent):
    h = agent.handle
    h.run(2500 + 2000)
    runs = []
    for _ in range(3):
        s0 = h.status(); t0 = time.perf_counter()
        h.run(N_UPD // 3)
        dt = time.perf_counter() - t0; s1 = h.status()
        runs.append(dict(steps=s1["global_step"] - s0["global_step"], updates=s1["n_updates"] - s0["n_updates"], seconds=dt,
                         steps_per_s=(s1["global_step"] - s0["global_step"]) / dt))
    agent.close()
    runs.sort(key=lambda r: r["steps_per_s"])
    return {"median_steps_per_s": runs[1]["steps_per_s"], "us_per_cycle": 1e6 / runs[1]["steps_per_s"], "runs": runs}


out = {"metric": "env-steps/s of the whole loop (library Pendulum, ddpg.jl defaults: batch 120, ring 1e5, one update per env step after warmup_steps = "
                 "2500); one cycle = one env step = six launches for DDPG, TD3 and SAC",
       "launches_per_cycle": {"ddpg": 6, "td3": 6, "sac": 6},
       "ddpg": whole_loop(crl.DDPGAgent(crl.DDPGConfig(total_timesteps=TOTAL), seed=1)),
       "td3_policy_delay_1": whole_loop(crl.TD3Agent(crl.TD3Config(total_timesteps=TOTAL, policy_delay=1), seed=1)),
       "td3_policy_delay_2": whole_loop(crl.TD3Agent(crl.TD3Config(total_timesteps=TOTAL, policy_delay=2), seed=1)),
       "sac": whole_loop(crl.SACAgent(crl.SACConfig(total_timesteps=TOTAL), seed=1)),
       "sac_autotune_off": whole_loop(crl.SACAgent(crl.SACConfig(total_timesteps=TOTAL, autotune=False, alpha=0.2), seed=1)),
       "shader_clock_mhz": {"median": clock[0], "min": clock[1], "max": clock[2]}}
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "sac_bench.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
