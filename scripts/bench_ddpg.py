#!/usr/bin/env python3
"""DDPG side measurement: env-steps/s of the whole ddpg.jl loop on the library's Pendulum at the reference defaults (one 120-sample update per env
step once global_step > warmup_steps = 2500: six dependent launches per step), and env-steps/s of the warm-up-only phase (rand(act_space), env step,
Buffer.add! — every step inside one launch). Writes profiles/ddpg_bench.json with the box's shader clock.

    python scripts/bench_ddpg.py [update_steps] [warmup_steps]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import cleanrl_jl_amd as crl

N_UPD = int(sys.argv[1]) if len(sys.argv) > 1 else 30_000
N_WARM = int(sys.argv[2]) if len(sys.argv) > 2 else 500_000
clock = crl._lib.clock_probe(0)

# whole loop at the reference defaults: the timed region starts once the warm-up is over
cfg = crl.DDPGConfig(total_timesteps=2500 + 2000 + N_UPD)
agent = crl.DDPGAgent(cfg, seed=1)
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

# warm-up only: no update is ever due
cfg = crl.DDPGConfig(total_timesteps=N_WARM + 10_000, warmup_steps=N_WARM + 10_000)
agent = crl.DDPGAgent(cfg, seed=1)
h = agent.handle
h.run(10_000)
t0 = time.perf_counter(); taken = h.run(N_WARM)[0]; dt_w = time.perf_counter() - t0
assert h.status()["n_updates"] == 0
agent.close()

runs.sort(key=lambda r: r["steps_per_s"])
out = {"metric": "DDPG env-steps/s (library Pendulum, ddpg.jl defaults: batch 120, ring 1e5, one update per env step after warmup_steps = 2500)",
       "whole_loop": {"median_steps_per_s": runs[1]["steps_per_s"], "us_per_step": 1e6 / runs[1]["steps_per_s"], "runs": runs},
       "warmup_only": {"steps": taken, "seconds": dt_w, "steps_per_s": taken / dt_w},
       "shader_clock_mhz": {"median": clock[0], "min": clock[1], "max": clock[2]}}
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "ddpg_bench.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
