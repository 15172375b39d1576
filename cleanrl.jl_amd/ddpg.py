"""Host-side mirror of the reference's DDPG file (src/algorithms/ddpg.jl) over the C ABI: same names (`DDPGConfig`, `make_ddpg_nn`,
`polyak_update`, `get_q`, `ddpg`) and logger records. All arithmetic of the loop runs in libcleanrl_hip.so (csrc/ddpg.hip); the env is the
library's Pendulum or any host object (the reference's own env is a MuJoCo one behind PyCall, ddpg.jl:50)."""
import dataclasses
import logging
import time

import numpy as np

from . import _lib as L
from . import logger as Logger
from .ppo import EVAL_SEED    # the key of the evaluation envs is its own: a held-out score does not replay the training env's initial states


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


def eval_report(returns, disc_returns, q0, env_steps):
    """The fields of crl_ddpg_eval_report from per-episode arrays, the library's formulas: Float64, sums in array order, population standard
    deviation, q_bias_mean = Σ(q0 − disc_return) / episodes."""
    ret, disc, q = (np.asarray(x, np.float64).reshape(-1) for x in (returns, disc_returns, q0))
    n = np.float64(ret.size)
    rsum = dsum = qsum = bsum = var = np.float64(0.0)
    for r, d, v in zip(ret, disc, q):
        rsum = rsum + r; dsum = dsum + d; qsum = qsum + v; bsum = bsum + (v - d)
    mean = rsum / n
    for r in ret:
        var = var + (r - mean) * (r - mean)
    return dict(episodes=int(ret.size), env_steps=int(env_steps), return_mean=float(mean), return_std=float(np.sqrt(var / n)),
                return_min=float(ret.min()), return_max=float(ret.max()), disc_return_mean=float(dsum / n), q0_mean=float(qsum / n),
                q_bias_mean=float(bsum / n))


def _check_eval_args(who, num_envs, episodes_per_env, seed, trace_steps, max_steps, last_step=False):
    """The argument checks of the *_evaluate calls, before the library is touched. last_step: an episode may take max_steps + 1 steps (the CartPole
    of dqn / a2c ends at t > max_steps), so that is what bounds the trace."""
    for name, v, lo, hi in (("num_envs", num_envs, 1, 65536), ("episodes_per_env", episodes_per_env, 1, 1024), ("trace_steps", trace_steps, 0, None)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{who}: {name} must be an integer, got {type(v).__name__}")
        if v < lo or (hi is not None and v > hi):
            raise ValueError(f"{who}: {name} must be in {lo}..{hi}, got {v}" if hi else f"{who}: {name} must be >= {lo}, got {v}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{who}: seed must be an integer in [0, 2^64), got {seed!r}")
    if num_envs * episodes_per_env > 1 << 20:
        raise ValueError(f"{who}: num_envs * episodes_per_env must be <= 1048576, got {num_envs * episodes_per_env}")
    per_episode, label = (max_steps + 1, "(max_steps + 1)") if last_step else (max_steps, "max_steps")
    if trace_steps > episodes_per_env * per_episode:
        raise ValueError(f"{who}: trace_steps must be <= episodes_per_env * {label} = {episodes_per_env * per_episode}, got {trace_steps}")
    if trace_steps * num_envs > 1 << 24:
        raise ValueError(f"{who}: trace_steps * num_envs must be <= 16777216, got {trace_steps * num_envs}")


def _evaluate_on_host_env(agent, env, episodes):
    """ddpg_evaluate's host route: the env is an object in this process, the actions are crl_ddpg_actor's, the sums the library's (Float64, step order)."""
    h, gamma = agent.handle, np.float64(agent.config.gamma)
    ret, disc_ret, q0, steps = np.zeros((episodes, 1)), np.zeros((episodes, 1)), np.zeros((episodes, 1)), 0
    for j in range(episodes):
        obs = np.asarray(env.reset(), np.float64)
        r_sum, d_sum, disc, first, terminal = np.float64(0.0), np.float64(0.0), np.float64(1.0), True, False
        while not terminal:
            action = h.actor(obs)[:, 0]
            if first:
                q0[j, 0] = h.q_values(obs, action)[0]; first = False
            reward, obs, terminal = env.step(action)
            obs = np.asarray(obs, np.float64); reward = np.float64(reward)
            r_sum = r_sum + reward; d_sum = d_sum + disc * reward; disc = disc * gamma; steps += 1
        ret[j, 0] = r_sum; disc_ret[j, 0] = d_sum
    return {"report": eval_report(ret, disc_ret, q0, steps), "returns": ret, "disc_returns": disc_ret, "q0": q0}


def ddpg_evaluate(agent, *, num_envs=256, episodes_per_env=1, seed=EVAL_SEED, trace_steps=0, env=None):
    """How good is the current actor, and does the critic over-estimate? crl_ddpg_evaluate: the agent's actor, frozen and WITHOUT the exploration
    noise, plays `episodes_per_env` whole episodes on each of `num_envs` fresh Pendulums in one launch on the GPU (no reference counterpart: ddpg.jl
    only logs the returns of its noisy behaviour policy). Training state is not touched. Returns {"report": {episodes, env_steps, return_mean,
    return_std, return_min, return_max, disc_return_mean, q0_mean, q_bias_mean}, "returns", "disc_returns", "q0"} — the arrays are
    (episodes_per_env, num_envs) float64; q0 = Q(s0, actor(s0)) and q_bias_mean = mean(q0 − discounted return): positive = the critic promises more
    than the policy collects — plus "trace_action" (trace_steps, num_envs), the actions of each env's first trace_steps steps, when trace_steps > 0.
    `env=<host env object>` (the protocol of ddpg(config, env)) serves an agent whose env lives in this process: a host loop over the handle's
    noise-free actor, episode after episode until `terminal`, through the same report; num_envs is then 1 (leave it alone), and seed / trace_steps
    belong to the on-device envs and are refused. Arguments are validated here, before the library is touched. A TD3Agent (td3.py) is served alike:
    its q0 is critic 1's."""
    if not isinstance(agent, DDPGAgent):
        raise TypeError("ddpg_evaluate: agent must be a cleanrl_jl_amd DDPGAgent (PPO agents: evaluate)")
    if env is not None:
        if isinstance(env, str):
            raise ValueError("ddpg_evaluate: env must be a host env object (the built-in Pendulum needs none)")
        if num_envs not in (1, 256) or isinstance(num_envs, bool):
            raise ValueError(f"ddpg_evaluate: a host env is one env — num_envs must be left alone (or 1), got {num_envs!r}")
        if seed != EVAL_SEED or trace_steps != 0:
            raise ValueError("ddpg_evaluate: seed and trace_steps belong to the on-device envs; a host env is seeded and traced by its owner")
        _check_eval_args("ddpg_evaluate", 1, episodes_per_env, EVAL_SEED, 0, 1)
        return _evaluate_on_host_env(agent, env, int(episodes_per_env))
    _check_eval_args("ddpg_evaluate", num_envs, episodes_per_env, seed, trace_steps, int(agent.crl_cfg.max_steps))
    return agent.handle.evaluate(num_envs, episodes_per_env, seed, trace_steps)   # an external handle: the library's message points to crl_ddpg_actor


def _eval_record(global_step, report):
    return (global_step, "Evaluation Statistics", dict(eval_return_mean=report["return_mean"], eval_return_std=report["return_std"],
                                                       eval_q_bias=report["q_bias_mean"], global_step=global_step))


def ddpg(config: DDPGConfig = None, env="pendulum", *, device=0, seed=0x5EED, params=None, chunk=4096, noise_in_update=True, eval_every=0,
         eval_envs=256, eval_episodes=1, eval_env=None, **logger_kw):
    """ddpg.jl:47-136. env="pendulum": the library's Pendulum, one library call per `chunk` env steps. Otherwise `env` is a host object with
    obs_dim, act_dim, act_low, act_high, reset() -> obs and step(action) -> (reward, next_obs, terminal): the library picks the action and learns,
    this loop steps the env and keeps the episode statistics of ddpg.jl:92-101. The "CleanRL" logger receives "Episode Statistics"
    (episode_return, episode_length, steps_per_sec, global_step; ddpg.jl:97) and "Training Statistics" (actor_loss, critic_loss; :132).
    `eval_every=N > 0` adds an "Evaluation Statistics" record (eval_return_mean, eval_return_std, eval_q_bias, global_step) after the records of
    every step that is a multiple of N: ddpg_evaluate of the parameters that step left, on eval_envs fresh Pendulums x eval_episodes episodes (the
    library calls are cut at multiples of N; chunking changes no bit of the run) or, with a host env, eval_episodes episodes on `eval_env`, a SECOND
    env object — the training env is in the middle of an episode. 0 (default) keeps the record stream what it was."""
    return _loop("ddpg", lambda config, **kw: DDPGAgent(config, noise_in_update=noise_in_update, **kw), config or DDPGConfig(), env, device=device,
                 seed=seed, params=params, chunk=chunk, eval_every=eval_every, eval_envs=eval_envs, eval_episodes=eval_episodes, eval_env=eval_env,
                 **logger_kw)


def _training_records(handle, losses, train_extra):
    """the "Training Statistics" records of the loss records a run() / read_losses() call just returned"""
    extras = train_extra(handle, losses) if train_extra is not None else [{}] * len(losses)
    return [(g, "Training Statistics", dict(actor_loss=a, critic_loss=c, **extra)) for (g, a, c), extra in zip(losses, extras)]


def _loop(who, make_agent, config, env, *, device, seed, params, chunk, eval_every, eval_envs, eval_episodes, eval_env, train_extra=None, **logger_kw):
    """The loop of ddpg() for any agent on a crl_ddpg handle (td3() and sac() run it too): make_agent(config, device=, seed=, params=[, obs_dim=,
    act_dim=, act_low=, act_high=, external=True]) builds it; `who` names the caller in messages and in the logger's run name. train_extra(handle,
    losses) -> one dict per loss record just read: further fields of that step's "Training Statistics" record (sac(): alpha, alpha_loss, entropy);
    None leaves the record what ddpg.jl:132 logs."""
    if isinstance(eval_every, bool) or not isinstance(eval_every, (int, np.integer)) or eval_every < 0:
        raise ValueError(f"{who}: eval_every must be an integer >= 0, got {eval_every!r}")
    host_env = not isinstance(env, str)
    if eval_every:
        if host_env and (eval_env is None or isinstance(eval_env, str) or eval_env is env):
            raise ValueError(f"{who}: eval_every with a host env needs eval_env, a second env object (evaluating on the training env would break its episode)")
        _check_eval_args(who, 1 if host_env else eval_envs, eval_episodes, EVAL_SEED, 0, 1)
    Logger.make_logger(f"{who}|{config.run_name}", **({"to_terminal": False} | logger_kw))        # ddpg.jl:48
    lg = logging.getLogger("CleanRL")
    start = time.time()
    if not host_env:
        if env != "pendulum":
            raise ValueError(f"{who}: the only built-in env is 'pendulum', got {env!r}")
        agent = make_agent(config, device=device, seed=seed, params=params)
        global_step = 0
        while True:
            budget = min(chunk, eval_every - global_step % eval_every) if eval_every else chunk
            taken, episodes, losses = agent.handle.run(budget)
            records = [(g, "Episode Statistics", dict(episode_return=r, episode_length=n, steps_per_sec=int(g / max(time.time() - start, 1e-9)),
                                                      global_step=g)) for r, n, g in episodes]
            records += _training_records(agent.handle, losses, train_extra)
            _emit(lg, records)
            global_step = agent.handle.status()["global_step"]
            if eval_every and taken > 0 and global_step % eval_every == 0:
                _emit(lg, [_eval_record(global_step, agent.handle.evaluate(eval_envs, eval_episodes, EVAL_SEED, 0)["report"])])
            if taken == 0 or global_step >= config.total_timesteps:
                break
        return agent
    agent = make_agent(config, obs_dim=env.obs_dim, act_dim=env.act_dim, act_low=env.act_low, act_high=env.act_high, external=True, device=device,
                       seed=seed, params=params)
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
            _emit(lg, _training_records(h, h.read_losses(), train_extra))
        if eval_every and global_step % eval_every == 0:
            _emit(lg, [_eval_record(global_step, _evaluate_on_host_env(agent, eval_env, int(eval_episodes))["report"])])
    return agent
