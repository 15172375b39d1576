"""TD3 (Fujimoto et al. 2018: twin critics, delayed actor, target policy smoothing) on the library's DDPG handle — the reference has no TD3; the
file follows ddpg.py, the host-side mirror of src/algorithms/ddpg.jl, and shares its loop, its env protocol and its logger records. All arithmetic
runs in libcleanrl_hip.so (csrc/ddpg.hip, the crl_td3_* block of include/cleanrl_hip.h)."""
import dataclasses

from . import _lib as L
from .ddpg import DDPGAgent, DDPGConfig, _loop, make_ddpg_nn


@dataclasses.dataclass
class TD3Config(DDPGConfig):
    """DDPGConfig's fields (ddpg.jl:1-15) plus TD3's three: the actor and the targets move on every policy_delay-th step, and the target action
    gets clamp(policy_noise·randn, ±noise_clip) per sample."""
    policy_delay: int = 2
    policy_noise: float = 0.2
    noise_clip: float = 0.5


def make_td3_nn(obs_dim, act_dim, seed=0):
    """(actor, critic1, critic2): make_ddpg_nn(seed), and the critic of make_ddpg_nn(seed + 1) as the second critic."""
    actor, critic1 = make_ddpg_nn(obs_dim, act_dim, seed)
    return actor, critic1, make_ddpg_nn(obs_dim, act_dim, seed + 1)[1]


class TD3Agent(DDPGAgent):
    """actor, two critics, their three targets, three Adam states and the ReplayBuffer(buffer_size) of one td3(config) run, on one GPU. A DDPGAgent
    to ddpg_evaluate and get_q (critic 1)."""

    def __init__(self, config: TD3Config, *, obs_dim=3, act_dim=1, act_low=-2.0, act_high=2.0, external=False, device=0, params=None, seed=0x5EED,
                 init_seed=0, max_steps=200):
        self.config = config
        self.crl_cfg = L.CrlDDPGConfig(int(config.total_timesteps), int(config.buffer_size), int(config.min_buff_size), int(config.batch_size),
                                       int(config.warmup_steps), int(config.log_frequencey), float(config.lr), float(config.tau), float(config.gamma),
                                       float(config.exploration_noise), int(obs_dim), int(act_dim),
                                       L.DDPG_ENV_EXTERNAL if external else L.DDPG_ENV_PENDULUM, int(max_steps), float(act_low), float(act_high),
                                       0, 0, seed)
        self.crl_opt = L.CrlTD3Options(int(config.policy_delay), 0, float(config.policy_noise), float(config.noise_clip))
        self.handle = L.TD3Handle(self.crl_cfg, self.crl_opt, device)
        self.handle.write_params(*(make_td3_nn(obs_dim, act_dim, init_seed) if params is None else params))


def td3(config: TD3Config = None, env="pendulum", *, device=0, seed=0x5EED, params=None, chunk=4096, eval_every=0, eval_envs=256, eval_episodes=1,
        eval_env=None, **logger_kw):
    """ddpg()'s loop with a TD3Agent: env="pendulum" (the library's Pendulum, one library call per `chunk` env steps) or a host env object (obs_dim,
    act_dim, act_low, act_high, reset() -> obs, step(action) -> (reward, next_obs, terminal)); the same "Episode Statistics" and "Training
    Statistics" records (critic_loss is the sum of the two critics' losses; actor_loss is the latest actor step's) and, with eval_every=N > 0, the
    same "Evaluation Statistics" (eval_q_bias is critic 1's). params: (actor, critic1, critic2). Returns the agent."""
    return _loop("td3", TD3Agent, config or TD3Config(), env, device=device, seed=seed, params=params, chunk=chunk, eval_every=eval_every,
                 eval_envs=eval_envs, eval_episodes=eval_episodes, eval_env=eval_env, **logger_kw)
