#!/usr/bin/env python3
"""Does the on-device DDPG learn the library's Pendulum? Eight seeds, reference hyper-parameters except a shorter warm-up and a larger step size
(stated in the output). Per seed: the mean return of the warm-up episodes (rand(act_space): the random policy's level on this env), the mean
return of every block of ten episodes, and of the last ten. Writes profiles/ddpg_pendulum_train.json.

    python scripts/ddpg_train.py [total_timesteps] [lr]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import cleanrl_jl_amd as crl

T = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
LR = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-3
WARM = 2000
seeds = list(range(1, 9))
out = {"what": "DDPG on the library Pendulum (episode = 200 steps, return = sum of -(th^2 + 0.1 thd^2 + 0.001 u^2))",
       "config": dict(total_timesteps=T, warmup_steps=WARM, lr=LR, batch_size=120, tau=0.005, gamma=0.99, exploration_noise=0.1, noise_in_update=1),
       "seeds": {}}
t0 = time.perf_counter()
for s in seeds:
    agent = crl.DDPGAgent(crl.DDPGConfig(total_timesteps=T, warmup_steps=WARM, lr=LR), seed=s, init_seed=s)
    eps = []
    while True:
        taken, e, _ = agent.handle.run(4000)
        eps += e
        if taken == 0:
            break
    agent.close()
    ret = np.array([r for r, _, _ in eps]); n_warm = WARM // 200
    blocks = [float(ret[i:i + 10].mean()) for i in range(0, len(ret) - 9, 10)]
    out["seeds"][str(s)] = dict(episodes=len(ret), warmup_mean_return=float(ret[:n_warm].mean()), block10_mean_returns=blocks,
                                last10_mean_return=float(ret[-10:].mean()))
out["seconds"] = time.perf_counter() - t0
out["random_level"] = float(np.mean([v["warmup_mean_return"] for v in out["seeds"].values()]))
out["worst_last10"] = float(min(v["last10_mean_return"] for v in out["seeds"].values()))
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "ddpg_pendulum_train.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
