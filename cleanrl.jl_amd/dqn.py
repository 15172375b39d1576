"""Host-side mirror of the reference's DQN file (src/algorithms/dqn.jl) over the C ABI: same names (`DQNConfig`, `make_nn`,
`linear_schedule`, `dqn`) and logger records. All arithmetic of the loop runs in libcleanrl_hip.so (csrc/dqn.hip)."""
import dataclasses
import logging
import time

import numpy as np

from . import _lib as L
from . import logger as Logger
from .ddpg import _check_eval_args, _emit
from .ppo import EVAL_SEED    # the key of the evaluation envs is its own: a held-out score does not replay the training env's initial states


@dataclasses.dataclass
class DQNConfig:
    """dqn.jl:1-19 (field names — including `log_frequencey` — and defaults of the reference)."""
    run_name: str = dataclasses.field(default_factory=lambda: time.strftime("%y-%m-%d|%H:%M:%S"))
    log_frequencey: int = 1000
    total_timesteps: int = 500_000
    buffer_size: int = 10_000
    min_buff_size: int = 200
    lr: float = 0.0001
    train_freq: int = 10
    target_net_freq: int = 100
    batch_size: int = 120
    gamma: float = 0.99
    epsilon_start: float = 1.0
    epsilon_end: float = 0.05
    epsilon_duration: float = 10_000


@dataclasses.dataclass
class PEROptions:
    """Prioritized experience replay (Schaul et al. 2016, proportional; crl_dqn_per_options) — not in dqn.jl, so not in DQNConfig. beta_duration =
    None means config.total_timesteps."""
    alpha: float = 0.6
    beta_start: float = 0.4
    beta_end: float = 1.0
    beta_duration: float = None
    eps: float = 1e-6


def per_beta(per, global_step):
    """beta(g) as include/cleanrl_hip.h pins it (host-side helper for the logger; the update evaluates the same expression on the device)."""
    slope = (per.beta_end - per.beta_start) / per.beta_duration
    v = slope * float(global_step) + per.beta_start
    if slope < 0.0:
        return per.beta_end if v < per.beta_end else v
    return per.beta_end if v > per.beta_end else v


def _check_per(per, config):
    """→ a PEROptions with beta_duration filled in, validated before the library is touched"""
    if not isinstance(per, PEROptions):
        raise TypeError(f"per must be a PEROptions or None, got {type(per).__name__}")
    per = dataclasses.replace(per, beta_duration=float(config.total_timesteps if per.beta_duration is None else per.beta_duration))
    for name, lo, hi in (("alpha", 0.0, 1.0), ("beta_start", 0.0, 1.0), ("beta_end", 0.0, 1.0), ("eps", 1e-6, 1.0)):
        v = getattr(per, name)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (lo <= v <= hi):
            raise ValueError(f"PEROptions.{name} must be in {lo}..{hi}, got {v!r}")
    if not (per.beta_duration > 0.0) or not np.isfinite(per.beta_duration):
        raise ValueError(f"PEROptions.beta_duration must be > 0, got {per.beta_duration!r}")
    return per


@dataclasses.dataclass
class DQNTargetOptions:
    """How the TD target is formed (crl_dqn_target_options) — not in dqn.jl, so not in DQNConfig: uncorrected n-step returns (n_step in 1..16) and
    double Q-learning (the bootstrap action is q_net's, its value target_net's). The defaults are dqn.jl's 1-step max over target_net."""
    n_step: int = 1
    double_q: bool = False


def _check_target(target):
    """→ the DQNTargetOptions, validated before the library is touched"""
    if not isinstance(target, DQNTargetOptions):
        raise TypeError(f"target must be a DQNTargetOptions or None, got {type(target).__name__}")
    n = target.n_step
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not (1 <= n <= 16):
        raise ValueError(f"DQNTargetOptions.n_step must be an integer in 1..16, got {n!r}")
    if not isinstance(target.double_q, (bool, np.bool_)):
        raise ValueError(f"DQNTargetOptions.double_q must be True or False, got {target.double_q!r}")
    return target


@dataclasses.dataclass
class C51Options:
    """The categorical value distribution of Bellemare et al. 2017 (crl_dqn_c51_options) — not in dqn.jl, so not in DQNConfig: n_atoms atoms (2..64)
    evenly spaced on [v_min, v_max]. CartPole at max_steps = 200 and gamma = 0.99 returns at most 86.6, so the default support covers it."""
    n_atoms: int = 51
    v_min: float = 0.0
    v_max: float = 100.0


def _check_c51(dist):
    """→ the C51Options, validated before the library is touched"""
    if not isinstance(dist, C51Options):
        raise TypeError(f"dist must be a C51Options or None, got {type(dist).__name__}")
    n = dist.n_atoms
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not (2 <= n <= 64):
        raise ValueError(f"C51Options.n_atoms must be an integer in 2..64, got {n!r}")
    for name in ("v_min", "v_max"):
        v = getattr(dist, name)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError(f"C51Options.{name} must be a finite number, got {v!r}")
    if not (dist.v_min < dist.v_max):
        raise ValueError(f"C51Options.v_min must be < v_max, got {dist.v_min!r} >= {dist.v_max!r}")
    return dist


@dataclasses.dataclass
class NoisyOptions:
    """Noisy linear layers (NoisyNets, Fortunato et al. 2018; crl_dqn_noisy_options) — not in dqn.jl, so not in DQNConfig: every dense layer learns
    mu and sigma per parameter and acts on mu + sigma·eps with factorised Gaussian eps, redrawn after every update; sigma starts at sigma0 / sqrt(in).
    The ε-greedy schedule is honoured as configured: the NoisyNet setting is DQNConfig(epsilon_start=0.0, epsilon_end=0.0), exploration by the noise
    alone."""
    sigma0: float = 0.5


def _check_noisy(noisy):
    """→ the NoisyOptions, validated before the library is touched"""
    if not isinstance(noisy, NoisyOptions):
        raise TypeError(f"noisy must be a NoisyOptions or None, got {type(noisy).__name__}")
    v = noisy.sigma0
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (0.0 <= v <= 10.0):
        raise ValueError(f"NoisyOptions.sigma0 must be in 0..10, got {v!r}")
    return noisy


NOISY_PLAIN_LAYERS = ((4, 120), (120, 84))                # (in, out) of the trunk; the head follows: (84, 2) or (84, 2N)


def noisy_layers(dueling=False, n_atoms=None):
    """(in, out) of a net's dense layers in parameter-array order: the rows of the noise table and of noisy_sigma"""
    if dueling:
        R = 1 if n_atoms is None else int(n_atoms)
        return ((4, 120), (120, 84), (84, R), (120, 84), (84, 2 * R))
    return NOISY_PLAIN_LAYERS + ((84, 2 if n_atoms is None else 2 * int(n_atoms)),)


def make_nn_noisy(seed=0, sigma0=0.5, dueling=False, n_atoms=None):
    """A noisy net's 2P numbers, mu (P, the twin's layout) then sigma (P): Fortunato's factorised rule, mu ~ U(−1/√in, +1/√in) for weights and biases
    and sigma = sigma0/√in, with a numpy stream — weights are an input."""
    rng = np.random.default_rng(seed)
    layers = noisy_layers(dueling, n_atoms)
    P = sum(o * (i + 1) for i, o in layers)
    out = np.zeros(2 * P, np.float32)
    at = 0
    for i, o in layers:
        n, lim = o * (i + 1), 1.0 / np.sqrt(float(i))
        out[at:at + n] = rng.uniform(-lim, lim, n).astype(np.float32)
        out[P + at:P + at + n] = np.float32(float(sigma0) * lim)
        at += n
    return out


def linear_schedule(start_e, end_e, duration, t):
    """dqn.jl:28-31 (host-side helper; the loop evaluates the same expression on the device)."""
    slope = (end_e - start_e) / duration
    return max(slope * t + start_e, end_e)


def make_nn(seed=0):
    """dqn.jl:22-26 for CartPole: Chain(Dense(4,120,relu), Dense(120,84,relu), Dense(84,2)) as ONE flat float32 vector in
    Flux.params order; Flux's default init (glorot_uniform weights, zero biases) with a numpy stream — weights are an input."""
    rng = np.random.default_rng(seed)
    out = np.zeros(L.DQN_PARAM_COUNT, np.float32)
    off = np.cumsum([0, 480, 120, 10080, 84, 168, 2])
    for i, (rows, cols) in zip((0, 2, 4), ((120, 4), (84, 120), (2, 84))):
        lim = np.sqrt(6.0 / (rows + cols))
        out[off[i]:off[i + 1]] = rng.uniform(-lim, lim, rows * cols).astype(np.float32)
    return out


def make_nn_c51(seed=0, n_atoms=51):
    """make_nn with the categorical head Dense(84, 2·n_atoms) (row a·n_atoms + i = atom i of action a): the same rule, and for the same seed the same
    trunk draws, on 10764 + 85·2·n_atoms numbers."""
    rng = np.random.default_rng(seed)
    rows3 = 2 * int(n_atoms)
    out = np.zeros(L.dqn_c51_param_count(n_atoms), np.float32)
    off = np.cumsum([0, 480, 120, 10080, 84, 84 * rows3, rows3])
    for i, (rows, cols) in zip((0, 2, 4), ((120, 4), (84, 120), (rows3, 84))):
        lim = np.sqrt(6.0 / (rows + cols))
        out[off[i]:off[i + 1]] = rng.uniform(-lim, lim, rows * cols).astype(np.float32)
    return out


def make_nn_dueling(seed=0, n_atoms=None):
    """make_nn for the dueling net (Wang et al. 2016): ten arrays W1 b1 W2v b2v W3v b3v W2a b2a W3a b3a with R = 1 (n_atoms None: scalar head) or
    R = n_atoms rows per stream output, 20928 + 255·R numbers; the same rule, the arrays drawing in that order, so W1 and W2v get make_nn's W1 and
    W2 draws for the same seed."""
    rng = np.random.default_rng(seed)
    R = 1 if n_atoms is None else int(n_atoms)
    out = np.zeros(L.dqn_dueling_param_count(R), np.float32)
    o = 0
    for rows, cols in ((120, 4), (84, 120), (R, 84), (84, 120), (2 * R, 84)):
        lim = np.sqrt(6.0 / (rows + cols))
        out[o:o + rows * cols] = rng.uniform(-lim, lim, rows * cols).astype(np.float32)
        o += rows * cols + rows
    return out


class DQNAgent:
    """q_net, target_net, Adam state, ReplayBuffer(buffer_size) and the CartPoleEnv of one dqn(config) run, on one GPU."""

    def __init__(self, config: DQNConfig, *, device=0, params=None, seed=0x5EED, init_seed=0, max_steps=200, per=None, target=None, dist=None, dueling=False,
                 noisy=None):
        if not isinstance(dueling, (bool, np.bool_)):
            raise ValueError(f"dueling must be True or False, got {dueling!r}")
        self.config = config
        self.noisy = None if noisy is None else _check_noisy(noisy)
        self.dueling = bool(dueling)
        self.dist = None if dist is None else _check_c51(dist)
        self.per = None if per is None else _check_per(per, config)
        self.target = None if target is None else _check_target(target)
        self.crl_cfg = L.CrlDQNConfig(int(config.log_frequencey), int(config.total_timesteps), int(config.buffer_size),
                                      int(config.min_buff_size), float(config.lr), int(config.train_freq), int(config.target_net_freq),
                                      int(config.batch_size), float(config.gamma), float(config.epsilon_start), float(config.epsilon_end),
                                      float(config.epsilon_duration), int(max_steps), 0, seed)
        p = self.per
        self.handle = L.DQNHandle(self.crl_cfg, device, per=None if p is None else L.CrlDQNPEROptions(float(p.alpha), float(p.beta_start),
                                                                                                      float(p.beta_end), float(p.beta_duration),
                                                                                                      float(p.eps)),
                                  target=None if self.target is None else L.CrlDQNTargetOptions(int(self.target.n_step), int(self.target.double_q)),
                                  c51=None if self.dist is None else L.CrlDQNC51Options(int(self.dist.n_atoms), 0, float(self.dist.v_min),
                                                                                        float(self.dist.v_max)),
                                  dueling=self.dueling, noisy=None if self.noisy is None else L.CrlDQNNoisyOptions(float(self.noisy.sigma0)))
        if params is None and self.noisy is not None:
            params = make_nn_noisy(init_seed, self.noisy.sigma0, self.dueling, None if self.dist is None else self.dist.n_atoms)
        elif params is None and self.dueling:
            params = make_nn_dueling(init_seed, None if self.dist is None else self.dist.n_atoms)
        elif params is None:
            params = make_nn(init_seed) if self.dist is None else make_nn_c51(init_seed, self.dist.n_atoms)
        self.handle.write_params(params)

    def close(self):
        self.handle.close()


def dqn_evaluate(agent, *, num_envs=256, episodes_per_env=1, seed=EVAL_SEED, trace_steps=0):
    """How good is the greedy policy, and does q_net over-estimate? crl_dqn_evaluate: the agent's q_net (not the target), frozen and WITHOUT the
    ε-greedy exploration, plays `episodes_per_env` whole episodes on each of `num_envs` fresh CartPoles in one launch on the GPU (no reference
    counterpart: dqn.jl only logs the returns of its ε >= 0.05 behaviour policy on the training env). Training state is not touched. Returns
    {"report": {episodes, env_steps, return_mean, return_std, return_min, return_max, length_mean, disc_return_mean, q0_mean, q_bias_mean},
    "returns", "lengths", "disc_returns", "q0"} — the arrays are (episodes_per_env, num_envs); q0 = max_a Q(s0, a) and q_bias_mean = mean(q0 −
    discounted return): positive = q_net promises more than the greedy policy collects — plus "trace_action" (trace_steps, num_envs), the actions
    of each env's first trace_steps steps (−1 once it has finished), when trace_steps > 0. Arguments are validated here, before the library is
    touched."""
    if not isinstance(agent, DQNAgent):
        raise TypeError("dqn_evaluate: agent must be a cleanrl_jl_amd DQNAgent")
    _check_eval_args("dqn_evaluate", num_envs, episodes_per_env, seed, trace_steps, int(agent.crl_cfg.max_steps), last_step=True)
    return agent.handle.evaluate(num_envs, episodes_per_env, seed, trace_steps)


def noisy_sigma(agent):
    """The mean |sigma| of each parameter array of the agent's q_net, read from the handle, in array order (W1 b1 W2 b2 W3 b3, or the dueling net's
    ten): how much noise the layers have kept. NoisyNets anneal their own exploration, so this is the curve to watch where ε would be."""
    if not isinstance(agent, DQNAgent) or agent.noisy is None:
        raise TypeError("noisy_sigma: agent must be a DQNAgent made with noisy=NoisyOptions(...)")
    q, _ = agent.handle.read_params()
    sigma = q[q.size // 2:]
    out, at = [], 0
    for i, o in noisy_layers(agent.dueling, None if agent.dist is None else agent.dist.n_atoms):
        out.append(float(np.abs(sigma[at:at + o * i]).mean())); at += o * i
        out.append(float(np.abs(sigma[at:at + o]).mean())); at += o
    return out


def _eval_record(global_step, report):
    return (global_step, "Evaluation Statistics", dict(eval_return_mean=report["return_mean"], eval_return_std=report["return_std"],
                                                       eval_q_bias=report["q_bias_mean"], global_step=global_step))


def dqn(config: DQNConfig = None, per: PEROptions = None, target: DQNTargetOptions = None, dist: C51Options = None, dueling=False, noisy: NoisyOptions = None, *, device=0, seed=0x5EED, params=None, chunk=10_000, eval_every=0, eval_envs=256,
        eval_episodes=1, **logger_kw):
    """dqn.jl:34-120. One library call per `chunk` env steps; the "CleanRL" logger receives "Episode Statistics"
    (episode_return, episode_length, global_step, ϵ, steps_per_sec; dqn.jl:88) and "Training Statistics" (loss; dqn.jl:116).
    `eval_every=N > 0` adds an "Evaluation Statistics" record (eval_return_mean, eval_return_std, eval_q_bias, global_step) after the records of
    every env step that is a multiple of N: dqn_evaluate of the parameters that step left, on eval_envs fresh CartPoles x eval_episodes episodes.
    The library calls are cut at multiples of N (crl_dqn_run takes a step budget; chunking changes no bit of the run). 0 (default) keeps the record
    stream what it was. `per` (a PEROptions) replays with proportional priorities instead of uniformly (crl_dqn_per_create); "Training Statistics" then
    carries beta, the importance exponent of that update, next to the loss (the importance-weighted one). None (default) is dqn.jl. `target` (a
    DQNTargetOptions) forms the TD target from n-step returns and / or with double Q-learning (crl_dqn_create_with), with either replay; the log records
    are unchanged, and None (default) is dqn.jl's 1-step max. `dist` (a C51Options) makes the critic categorical (crl_dqn_c51_create), with either
    replay and any target options: "Training Statistics".loss is then the cross-entropy against the projected target distribution, and the evaluation
    record's eval_q_bias is that of the expected value. None (default) is the scalar critic, bit for bit what it was. `dueling=True` splits layers 2 and 3 into a value and an
    advantage stream (crl_dqn_dueling_create), with either head, either replay and any target options; the records are unchanged, and False (default)
    is the one-headed net, bit for bit what it was. `noisy` (a NoisyOptions) makes every dense layer a noisy one (crl_dqn_noisy_create), with every
    option above; the records are unchanged (ϵ is logged as configured: set epsilon_start = epsilon_end = 0 to explore by the noise alone), evaluation
    runs with the noise off, and None (default) is the log stream it was."""
    if isinstance(eval_every, bool) or not isinstance(eval_every, (int, np.integer)) or eval_every < 0:
        raise ValueError(f"dqn: eval_every must be an integer >= 0, got {eval_every!r}")
    if eval_every:
        _check_eval_args("dqn", eval_envs, eval_episodes, EVAL_SEED, 0, 1)
    config = config or DQNConfig()
    Logger.make_logger(f"dqn|{config.run_name}", **({"to_terminal": False} | logger_kw))         # dqn.jl:35
    lg = logging.getLogger("CleanRL")
    agent = DQNAgent(config, device=device, seed=seed, params=params, per=per, target=target, dist=dist, dueling=dueling, noisy=noisy)
    start = time.time()
    global_step = 0
    while True:
        taken, episodes, losses = agent.handle.run(min(chunk, eval_every - global_step % eval_every) if eval_every else chunk)
        records = [(g, "Episode Statistics", dict(episode_return=r, episode_length=n, global_step=g, **{"ϵ": e},
                                                  steps_per_sec=int(g / max(time.time() - start, 1e-9)))) for r, n, g, e in episodes]
        records += [(g, "Training Statistics", dict(loss=v) if agent.per is None else dict(loss=v, beta=per_beta(agent.per, g))) for g, v in losses]
        _emit(lg, records)
        global_step = agent.handle.status()["global_step"]
        if eval_every and taken > 0 and global_step % eval_every == 0:
            _emit(lg, [_eval_record(global_step, agent.handle.evaluate(eval_envs, eval_episodes, EVAL_SEED, 0)["report"])])
        if taken == 0 or global_step >= config.total_timesteps:
            break
    return agent
