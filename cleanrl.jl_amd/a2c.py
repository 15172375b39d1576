"""Host-side mirror of the reference's A2C file (src/algorithms/a2c.jl) over the C ABI: same names (`A2CConfig`, `a2c`,
`discounted_future_rewards`), same argument meaning and the same two logger records. All arithmetic runs in
libcleanrl_hip.so (csrc/a2c.hip); this module only orchestrates and logs."""
import dataclasses
import time

import numpy as np

from . import _lib as L
from . import logger as Logger
from . import networks
from .ddpg import _check_eval_args
from .ppo import EVAL_SEED    # the key of the evaluation envs is its own: a held-out score does not replay the training env's initial states


@dataclasses.dataclass
class A2CConfig:
    """a2c.jl:1-10 (field names and defaults of the reference)."""
    run_name: str = dataclasses.field(default_factory=lambda: time.strftime("%y-%m-%d|%H:%M:%S"))
    lr: float = 0.0001
    total_timesteps: int = 1_000_000
    min_replay_size: int = 512
    gamma: float = 0.99


def discounted_future_rewards(rewards, terminals, final_value, gamma, *, device=0):
    """a2c.jl:13-24. All-Float64 like the reference's method signature; `terminals` is a Bool vector."""
    rewards = np.asarray(rewards)
    if rewards.dtype != np.float64:
        raise TypeError("discounted_future_rewards: rewards must be Float64 (a2c.jl:13 Vector{T}, final_value::T, γ::T)")
    terminals = np.asarray(terminals)
    if terminals.shape != rewards.shape:
        raise ValueError("discounted_future_rewards: rewards and terminals differ in length")
    return L.a2c_discounted_future_rewards_host(rewards, terminals.astype(np.uint8), float(final_value), float(gamma), device)


class A2CAgent:
    """Actor, critic, Optimiser(ClipNorm(0.5), Adam(lr)) state, ReplayBuffer(2*min_replay_size) and the CartPoleEnv of one
    a2c(config) run (a2c.jl:32-52), resident on one GPU."""

    def __init__(self, config: A2CConfig, *, device=0, params=None, seed=0x5EED, init_seed=0, max_steps=500):
        self.config = config
        self.crl_cfg = L.CrlA2CConfig(float(config.lr), int(config.total_timesteps), int(config.min_replay_size), int(max_steps),
                                      float(config.gamma), seed)
        self.handle = L.A2CHandle(self.crl_cfg, device)
        if params is None:
            params = networks.make_actor_critic(2, 4, [64, 64], seed=init_seed)   # a2c.jl:37 make_actor_critic(env)
        self.handle.write_params(params)

    def close(self):
        self.handle.close()


def a2c_evaluate(agent, *, num_envs=256, episodes_per_env=1, greedy=True, seed=EVAL_SEED, trace_steps=0):
    """How good is the current actor, and does the critic over-estimate? crl_a2c_evaluate: the agent's actor, frozen, plays `episodes_per_env` whole
    episodes on each of `num_envs` fresh CartPoles in one launch on the GPU — greedy=True takes the larger logit, greedy=False samples from the
    softmax as the training loop does (no reference counterpart: a2c.jl only logs the sampled policy's returns on the training env, when an episode
    happens to end). Training state is not touched. Returns {"report": {episodes, env_steps, return_mean, return_std, return_min, return_max,
    length_mean, disc_return_mean, v0_mean, v_bias_mean}, "returns", "lengths", "disc_returns", "v0"} — the arrays are (episodes_per_env, num_envs);
    v0 = critic(s0) and v_bias_mean = mean(v0 − discounted return): positive = the critic promises more than the policy collects — plus
    "trace_action" (trace_steps, num_envs), the actions of each env's first trace_steps steps (−1 once it has finished), when trace_steps > 0.
    Arguments are validated here, before the library is touched."""
    if not isinstance(agent, A2CAgent):
        raise TypeError("a2c_evaluate: agent must be a cleanrl_jl_amd A2CAgent")
    if not isinstance(greedy, (bool, np.bool_)):
        raise ValueError(f"a2c_evaluate: greedy must be True or False, got {greedy!r}")
    _check_eval_args("a2c_evaluate", num_envs, episodes_per_env, seed, trace_steps, int(agent.crl_cfg.max_steps), last_step=True)
    return agent.handle.evaluate(num_envs, episodes_per_env, L.EVAL_GREEDY if greedy else L.EVAL_SAMPLE, seed, trace_steps)


def a2c(config: A2CConfig = None, *, device=0, seed=0x5EED, params=None, eval_every=0, eval_envs=256, eval_episodes=1, **logger_kw):
    """a2c.jl:29-113. Returns the agent after total_timesteps env steps. The "CleanRL" logger receives the reference's
    "Training Statistics" (actor_loss, critic_loss; a2c.jl:100) and "Episode Statistics" (a2c.jl:106) records.
    `eval_every=N > 0` adds an "Evaluation Statistics" record (eval_return_mean, eval_return_std, eval_v_bias, global_step) after the records of
    every env step that is a multiple of N: the greedy a2c_evaluate of the parameters that step left, on eval_envs fresh CartPoles x eval_episodes
    episodes. The library calls are cut at multiples of N (crl_a2c_run_until_update takes a step budget; chunking changes no bit of the run). 0
    (default) keeps the record stream what it was."""
    import logging
    if isinstance(eval_every, bool) or not isinstance(eval_every, (int, np.integer)) or eval_every < 0:
        raise ValueError(f"a2c: eval_every must be an integer >= 0, got {eval_every!r}")
    if eval_every:
        _check_eval_args("a2c", eval_envs, eval_episodes, EVAL_SEED, 0, 1)
    config = config or A2CConfig()
    Logger.make_logger(f"a2c|{config.run_name}", **({"to_terminal": False} | logger_kw))      # a2c.jl:30
    lg = logging.getLogger("CleanRL")

    def log(msg, **kv):
        lg.info(msg, extra={"crl": kv})
    agent = A2CAgent(config, device=device, seed=seed, params=params)
    start = time.time()
    global_step = 0
    while True:
        taken, ts, episodes = agent.handle.run_until_update(eval_every - global_step % eval_every) if eval_every else agent.handle.run_until_update()
        # the episode whose end triggered the update is the call's LAST record, and the reference logs the update first (a2c.jl:100, then :106)
        for i, (ret, length, gstep) in enumerate(episodes):                   # a2c.jl:105-106
            if ts["trained"] and i == len(episodes) - 1:
                log("Training Statistics", actor_loss=ts["actor_loss"], critic_loss=ts["critic_loss"])   # a2c.jl:100
            log("Episode Statistics", episode_return=ret, episode_length=length, global_step=gstep,
                steps_per_sec=int(gstep / max(time.time() - start, 1e-9)))
        if ts["trained"] and not episodes:
            log("Training Statistics", actor_loss=ts["actor_loss"], critic_loss=ts["critic_loss"])
        global_step = agent.handle.env()[1]
        if eval_every and taken > 0 and global_step % eval_every == 0:
            rep = agent.handle.evaluate(eval_envs, eval_episodes, L.EVAL_GREEDY, EVAL_SEED, 0)["report"]
            log("Evaluation Statistics", eval_return_mean=rep["return_mean"], eval_return_std=rep["return_std"], eval_v_bias=rep["v_bias_mean"],
                global_step=global_step)
        if taken == 0 or global_step >= config.total_timesteps:
            break
    return agent
