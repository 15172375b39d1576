"""Host-side mirror of the reference's DDPG file (src/algorithms/ddpg.jl) over the C ABI: same names (`DDPGConfig`, `make_ddpg_nn`,
`polyak_update`, `get_q`, `ddpg`) and logger records. All arithmetic of the loop runs in libcleanrl_hip.so (csrc/ddpg.hip); the env is the
library's Pendulum or any host object (the reference's own env is a MuJoCo one behind PyCall, ddpg.jl:50)."""
import dataclasses
import logging
import time

import numpy as np

from . import _lib as L
from . import logger as Logger


@dataclasses.dataclass
class DDPGConfig:
    """ddpg.jl:1-15 (field names — including `log_frequencey` — and defaults of the reference)."""
    run_name: str = dataclasses.field(default_factory=lambda: time.strftime("%y-%m-%d|%H:%M:%S"))
    total_timesteps: int = 5_000_000
    buffer_size: int = 100_000
    min_buff_size: int = 200
    batch_size: int = 120
    warmup_steps: int = 2500
    log_frequencey: int = 1000
    lr: float = 0.0001
    tau: float = 0.005
    gamma: float = 0.99
    exploration_noise: float = 0.1


def make_ddpg_nn(obs_dim, act_dim, seed=0):
    """ddpg.jl:19-37: (actor, critic) as flat float32 vectors in Flux.params order — Dense(obs,64) → Dense(64,64) → Dense(64,act) and
    Dense(obs+act,64) → Dense(64,64) → Dense(64,1); Flux's default init (glorot_uniform weights, zero biases) with a numpy stream."""
    rng = np.random.default_rng(seed)
    nets = []
    for n_in, n_out in ((obs_dim, act_dim), (obs_dim + act_dim, 1)):
        parts = []
        for rows, cols in ((64, n_in), (64, 64), (n_out, 64)):
            lim = np.sqrt(6.0 / (rows + cols))
            parts += [rng.uniform(-lim, lim, rows * cols).astype(np.float32), np.zeros(rows, np.float32)]
        nets.append(np.concatenate(parts))
    return nets[0], nets[1]


def polyak_update(target, source, tau):
    """ddpg.jl:39-43 on flat float32 vectors, in place (host-side helper; the loop does the same per element on the device)."""
    target[:] = (tau * source.astype(np.float64) + (1.0 - tau) * target.astype(np.float64)).astype(np.float32)
    return target


def get_q(agent, obs, act):
    """ddpg.jl:45: critic(vcat(obs, act)) of the agent's critic, (obs_dim, n), (act_dim, n) → (n,)."""
    return agent.handle.q_values(obs, act)


class DDPGAgent:
    """actor, critic, their targets, both Adam states and the ReplayBuffer(buffer_size) of one ddpg(config) run, on one GPU."""

    def __init__(self, config: DDPGConfig, *, obs_dim=3, act_dim=1, act_low=-2.0, act_high=2.0, external=False, device=0, params=None, seed=0x5EED,
                 init_seed=0, max_steps=200, noise_in_update=True):
        self.config = config
        self.crl_cfg = L.CrlDDPGConfig(int(config.total_timesteps), int(config.buffer_size), int(config.min_buff_size), int(config.batch_size),
                                       int(config.warmup_steps), int(config.log_frequencey), float(config.lr), float(config.tau), float(config.gamma),
                                       float(config.exploration_noise), int(obs_dim), int(act_dim),
                                       L.DDPG_ENV_EXTERNAL if external else L.DDPG_ENV_PENDULUM, int(max_steps), float(act_low), float(act_high),
                                       int(bool(noise_in_update)), 0, seed)
        self.handle = L.DDPGHandle(self.crl_cfg, device)
        actor, critic = make_ddpg_nn(obs_dim, act_dim, init_seed) if params is None else params
        self.handle.write_params(actor, critic)

    def close(self):
        self.handle.close()


def _emit(lg, records):
    for _, msg, kv in sorted(records, key=lambda x: x[0]):
        lg.info(msg, extra={"crl": kv})


def ddpg(config: DDPGConfig = None, env="pendulum", *, device=0, seed=0x5EED, params=None, chunk=4096, noise_in_update=True, **logger_kw):
    """ddpg.jl:47-136. env="pendulum": the library's Pendulum, one library call per `chunk` env steps. Otherwise `env` is a host object with
    obs_dim, act_dim, act_low, act_high, reset() -> obs and step(action) -> (reward, next_obs, terminal): the library picks the action and learns,
    this loop steps the env and keeps the episode statistics of ddpg.jl:92-101. The "CleanRL" logger receives "Episode Statistics"
    (episode_return, episode_length, steps_per_sec, global_step; ddpg.jl:97) and "Training Statistics" (actor_loss, critic_loss; :132)."""
    config = config or DDPGConfig()
    Logger.make_logger(f"ddpg|{config.run_name}", **({"to_terminal": False} | logger_kw))        # ddpg.jl:48
    lg = logging.getLogger("CleanRL")
    start = time.time()
    if isinstance(env, str):
        if env != "pendulum":
            raise ValueError(f"ddpg: the only built-in env is 'pendulum', got {env!r}")
        agent = DDPGAgent(config, device=device, seed=seed, params=params, noise_in_update=noise_in_update)
        while True:
            taken, episodes, losses = agent.handle.run(chunk)
            records = [(g, "Episode Statistics", dict(episode_return=r, episode_length=n, steps_per_sec=int(g / max(time.time() - start, 1e-9)),
                                                      global_step=g)) for r, n, g in episodes]
            records += [(g, "Training Statistics", dict(actor_loss=a, critic_loss=c)) for g, a, c in losses]
            _emit(lg, records)
            if taken == 0 or agent.handle.status()["global_step"] >= config.total_timesteps:
                break
        return agent
    agent = DDPGAgent(config, obs_dim=env.obs_dim, act_dim=env.act_dim, act_low=env.act_low, act_high=env.act_high, external=True, device=device,
                      seed=seed, params=params, noise_in_update=noise_in_update)
    h = agent.handle
    episode_return, episode_length = 0.0, 0
    obs = np.asarray(env.reset(), np.float64)                                                    # ddpg.jl:74
    for global_step in range(1, config.total_timesteps + 1):
        action = h.act(obs)                                                                      # :79
        reward, next_obs, terminal = env.step(action)                                            # :80
        next_obs = np.asarray(next_obs, np.float64)
        h.observe(obs, action, reward, next_obs, terminal)                                       # :83-90, 105-129
        episode_return += float(reward); episode_length += 1                                     # :93-94
        obs = next_obs
        if terminal:                                                                             # :95-101
            _emit(lg, [(global_step, "Episode Statistics", dict(episode_return=episode_return, episode_length=episode_length,
                                                                steps_per_sec=int(global_step / max(time.time() - start, 1e-9)),
                                                                global_step=global_step))])
            episode_return, episode_length = 0.0, 0
            obs = np.asarray(env.reset(), np.float64)
        if global_step % config.log_frequencey == 0:                                             # :131-133
            _emit(lg, [(g, "Training Statistics", dict(actor_loss=a, critic_loss=c)) for g, a, c in h.read_losses()])
    return agent
