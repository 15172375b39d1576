"""SAC (Haarnoja et al. 2018: squashed-Gaussian actor, twin critics, entropy bonus, tuned temperature) on the library's DDPG handle — the reference
lists SAC as a to-do; the file follows td3.py and ddpg.py, the host-side mirror of src/algorithms/ddpg.jl, and shares their loop, env protocol and
logger records. All arithmetic runs in libcleanrl_hip.so (csrc/ddpg.hip + csrc/sac.hpp, the crl_sac_* block of include/cleanrl_hip.h)."""
import dataclasses
from typing import Optional

import numpy as np

from . import _lib as L
from .ddpg import DDPGAgent, DDPGConfig, _loop
from .td3 import make_td3_nn


@dataclasses.dataclass
class SACConfig(DDPGConfig):
    """DDPGConfig's fields (ddpg.jl:1-15; exploration_noise is not read) plus SAC's three: the temperature starts at alpha and, with autotune, follows
    Adam(lr) on log_alpha towards the entropy target_entropy (None: -act_dim)."""
    autotune: bool = True
    alpha: float = 1.0
    target_entropy: Optional[float] = None


def make_sac_nn(obs_dim, act_dim, seed=0):
    """(actor, critic1, critic2): the critics are make_td3_nn(seed)'s; the actor — Dense(obs,64) → Dense(64,64) → Dense(64,2·act), rows 0..act-1 of
    the head the mean, the rest the raw log-std — is Flux's default init (glorot_uniform weights, zero biases) from the numpy stream [seed, 0x5AC]."""
    rng = np.random.default_rng([seed, 0x5AC])
    parts = []
    for rows, cols in ((64, obs_dim), (64, 64), (2 * act_dim, 64)):
        lim = np.sqrt(6.0 / (rows + cols))
        parts += [rng.uniform(-lim, lim, rows * cols).astype(np.float32), np.zeros(rows, np.float32)]
    return (np.concatenate(parts),) + make_td3_nn(obs_dim, act_dim, seed)[1:]


class SACAgent(DDPGAgent):
    """actor, two critics and their targets, log_alpha, four Adam states and the ReplayBuffer(buffer_size) of one sac(config) run, on one GPU. A
    DDPGAgent to ddpg_evaluate (the deterministic action scale·tanh(μ) + bias) and get_q (critic 1)."""

    def __init__(self, config: SACConfig, *, obs_dim=3, act_dim=1, act_low=-2.0, act_high=2.0, external=False, device=0, params=None, seed=0x5EED,
                 init_seed=0, max_steps=200):
        self.config = config
        self.crl_cfg = L.CrlDDPGConfig(int(config.total_timesteps), int(config.buffer_size), int(config.min_buff_size), int(config.batch_size),
                                       int(config.warmup_steps), int(config.log_frequencey), float(config.lr), float(config.tau), float(config.gamma),
                                       float(config.exploration_noise), int(obs_dim), int(act_dim),
                                       L.DDPG_ENV_EXTERNAL if external else L.DDPG_ENV_PENDULUM, int(max_steps), float(act_low), float(act_high),
                                       0, 0, seed)
        target_entropy = -float(act_dim) if config.target_entropy is None else float(config.target_entropy)
        self.crl_opt = L.CrlSACOptions(int(bool(config.autotune)), 0, float(config.alpha), target_entropy)
        self.handle = L.SACHandle(self.crl_cfg, self.crl_opt, device)
        self.handle.write_params(*(make_sac_nn(obs_dim, act_dim, init_seed) if params is None else params))


def _alpha_fields(handle, losses):
    recs = handle.alpha_records()
    assert [r[0] for r in recs] == [l[0] for l in losses]
    return [dict(alpha=a, alpha_loss=al, entropy=e) for _, a, al, e in recs]


def sac(config: SACConfig = None, env="pendulum", *, device=0, seed=0x5EED, params=None, chunk=4096, eval_every=0, eval_envs=256, eval_episodes=1,
        eval_env=None, **logger_kw):
    """ddpg()'s loop with a SACAgent: env="pendulum" (the library's Pendulum, one library call per `chunk` env steps) or a host env object (obs_dim,
    act_dim, act_low, act_high, reset() -> obs, step(action) -> (reward, next_obs, terminal)); the same "Episode Statistics"; "Training Statistics"
    carry alpha, alpha_loss and entropy (= -mean logπ of the actor pass) beside actor_loss and critic_loss (the sum of the two critics' losses);
    with eval_every=N > 0 the same "Evaluation Statistics", of the deterministic action (eval_q_bias is critic 1's). params: (actor, critic1,
    critic2). Returns the agent."""
    return _loop("sac", SACAgent, config or SACConfig(), env, device=device, seed=seed, params=params, chunk=chunk, eval_every=eval_every,
                 eval_envs=eval_envs, eval_episodes=eval_episodes, eval_env=eval_env, train_extra=_alpha_fields, **logger_kw)
