#!/usr/bin/env python3
"""Does the on-device SAC learn the library's Pendulum, and what does it do to the critic's bias? Eight seeds at the step budget and the
hyper-parameters of scripts/td3_train.py (warm-up 2000, lr 1e-3), SAC at its defaults (autotune, alpha 1, target_entropy -1), and TD3 and DDPG
again at the same seeds in the same process. Per algorithm and seed: the mean return of the warm-up episodes, of every block of ten episodes and of
the last ten (what tests/test_gpu_sac.py builds its threshold from; SAC's training episodes are its SAMPLED policy's), and crl_ddpg_evaluate's
return_mean / q_bias_mean (256 held-out envs, the deterministic actor, critic 1) every 4000 steps; for SAC also the final alpha. Writes
profiles/sac_pendulum_train.json.

    python scripts/sac_train.py [total_timesteps] [lr]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import cleanrl_jl_amd as crl

T = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
LR = float(sys.argv[2]) if len(sys.argv) > 2 else 1e-3
WARM, CHUNK = 2000, 4000
seeds = list(range(1, 9))
common = dict(total_timesteps=T, warmup_steps=WARM, lr=LR, batch_size=120, tau=0.005, gamma=0.99, exploration_noise=0.1)


def train(make):
    per_seed, t0 = {}, time.perf_counter()
    for s in seeds:
        agent = make(s)
        eps, evals = [], {}
        while True:
            taken, e, _ = agent.handle.run(CHUNK)
            eps += e
            if taken == 0:
                break
            rep = crl.ddpg_evaluate(agent, num_envs=256)["report"]
            evals[str(agent.handle.status()["global_step"])] = dict(return_mean=rep["return_mean"], q_bias_mean=rep["q_bias_mean"], q0_mean=rep["q0_mean"])
        extra = dict(final_alpha=agent.handle.sac_status()["alpha"]) if isinstance(agent, crl.SACAgent) else {}
        agent.close()
        ret = np.array([r for r, _, _ in eps]); n_warm = WARM // 200
        per_seed[str(s)] = dict(episodes=len(ret), warmup_mean_return=float(ret[:n_warm].mean()),
                                block10_mean_returns=[float(ret[i:i + 10].mean()) for i in range(0, len(ret) - 9, 10)],
                                last10_mean_return=float(ret[-10:].mean()), eval=evals, **extra)
    out = dict(seeds=per_seed, seconds=time.perf_counter() - t0)
    out["random_level"] = float(np.mean([v["warmup_mean_return"] for v in per_seed.values()]))
    out["worst_last10"] = float(min(v["last10_mean_return"] for v in per_seed.values()))
    out["eval_mean_over_seeds"] = {g: {k: float(np.mean([v["eval"][g][k] for v in per_seed.values()])) for k in ("return_mean", "q_bias_mean")}
                                   for g in per_seed["1"]["eval"]}
    return out


sac = train(lambda s: crl.SACAgent(crl.SACConfig(total_timesteps=T, warmup_steps=WARM, lr=LR), seed=s, init_seed=s))
sac["config"] = dict(common, autotune=True, alpha=1.0, target_entropy=-1.0)
td3 = train(lambda s: crl.TD3Agent(crl.TD3Config(total_timesteps=T, warmup_steps=WARM, lr=LR), seed=s, init_seed=s))
td3["config"] = dict(common, policy_delay=2, policy_noise=0.2, noise_clip=0.5)
ddpg = train(lambda s: crl.DDPGAgent(crl.DDPGConfig(total_timesteps=T, warmup_steps=WARM, lr=LR), seed=s, init_seed=s))
ddpg["config"] = dict(common, noise_in_update=1)
out = {"what": "SAC, TD3 and DDPG on the library Pendulum (episode = 200 steps, return = sum of -(th^2 + 0.1 thd^2 + 0.001 u^2)), the same eight seeds; eval: "
               "crl_ddpg_evaluate on 256 held-out envs after every 4000 steps, q_bias_mean = mean(q0 - discounted return)",
       "sac": sac, "td3": td3, "ddpg": ddpg}
print(json.dumps({k: {"random_level": v["random_level"], "worst_last10": v["worst_last10"], "eval_mean_over_seeds": v["eval_mean_over_seeds"],
                      "seconds": v["seconds"]} for k, v in (("sac", sac), ("td3", td3), ("ddpg", ddpg))}))
with open(os.path.join(ROOT, "profiles", "sac_pendulum_train.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
