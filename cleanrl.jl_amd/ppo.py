"""Host-side mirror of sash-a/CleanRL.jl `src/algorithms/ppo.jl` over the C ABI (include/cleanrl_hip.h).

The reference host language is Julia, which this image lacks; the Julia shell a maintainer would use is in
INTEGRATION.md / julia/CleanRLHip.jl. This Python mirror keeps the same names, argument meaning and error behaviour
(`PPOConfig`, `ppo`, `get_action`, `logprob_actions`, `gae`, the two logger records) so the parity tests read like
tests of the reference. All arithmetic happens in libcleanrl_hip.so on the GPU; nothing here computes on the CPU.
"""
import dataclasses
import logging
import time

import numpy as np

from . import _lib as L
from . import networks

log = logging.getLogger("CleanRL")


@dataclasses.dataclass
class PPOConfig:
    """ppo.jl:1-19 — same field names and defaults (Float32 fields are rounded to float32 at the boundary)."""
    total_timesteps: int = 500_000
    num_steps: int = 32
    num_envs: int = 4
    num_minibatches: int = 4
    update_epochs: int = 4
    lr: float = 2.5e-4
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_coef: float = 0.2
    ent_coeff: float = 0.01
    v_coef: float = 0.5
    normalize_advantages: bool = True
    clip_value_loss: bool = True
    anneal_lr: bool = True


def _crl_config(config: PPOConfig, *, obs_dim=4, n_act=2, hidden=64, gae_mode=L.GAE_COMPAT, env_kind=L.ENV_CARTPOLE,
                stale_obs=True, env_id_offset=0, shuffle_mode=L.SHUFFLE_BLOCKED_FY, seed=0x5EED, num_envs=None):
    return L.CrlConfig(config.total_timesteps, config.num_steps, config.num_envs if num_envs is None else num_envs,
                       config.num_minibatches, config.update_epochs, config.lr, config.gamma, config.gae_lambda,
                       config.clip_coef, config.ent_coeff, config.v_coef, int(config.normalize_advantages),
                       int(config.clip_value_loss), int(config.anneal_lr), obs_dim, n_act, hidden, gae_mode, env_kind,
                       int(stale_obs), env_id_offset, shuffle_mode, seed)


# The on-device envs by name: env_kind, obs_dim, n_act — what ppo.jl:85-86 reads off `single_obs_space` / `single_act_space` of the env of ppo.jl:82
ENVS = {
    "cartpole": (L.ENV_CARTPOLE, 4, 2),        # CartPoleEnv(T=Float32, max_steps=500)
    "mountaincar": (L.ENV_MOUNTAINCAR, 2, 3),  # MountainCarEnv(T=Float32, max_steps=200)
    "acrobot": (L.ENV_ACROBOT, 6, 3),          # AcrobotEnv(T=Float32, max_steps=200)
}


def env_shape(env, **shape):
    """ppo.jl:82,85-86: the shape keywords of an Agent for the named env (`env=None`: the keywords as given — an explicit env_kind keeps working).
    obs_dim / n_act / env_kind given next to `env` must agree with it."""
    if env is None:
        return shape
    key = str(env).lower().replace("env", "").replace("_", "").replace("-", "")
    if key not in ENVS:
        raise ValueError(f"unknown env {env!r}: one of {sorted(ENVS)} (or pass env_kind / obs_dim / n_act yourself)")
    kind, obs_dim, n_act = ENVS[key]
    for name, want in (("env_kind", kind), ("obs_dim", obs_dim), ("n_act", n_act)):
        if shape.get(name, want) != want:
            raise ValueError(f"env={env!r} has {name}={want}, got {name}={shape[name]}")
    return shape | dict(env_kind=kind, obs_dim=obs_dim, n_act=n_act)


class Policy:
    """What `actor` / `critic` (Flux Chains in the reference, networks.jl:36-49) are here: a view of one network of an
    Agent whose weights live in HBM."""

    def __init__(self, agent, which):
        self.agent, self.which = agent, which

    def __call__(self, obs):
        obs = np.asfortranarray(obs, np.float32)
        if obs.ndim == 1:
            obs = obs[:, None]
        if self.which == "critic":
            _, _, v = self.agent.handle.policy_act(obs, np.zeros(obs.shape[1]))
            return v[None, :]
        raise TypeError("call get_action / logprob_actions for the actor (logits stay on the GPU)")


class Agent:
    """Actor + critic + optimiser state + rollout buffer + vectorised env of one PPO run, all resident on one GPU."""

    def __init__(self, config: PPOConfig, *, device=0, params=None, seed=0x5EED, init_seed=0, options=None, **shape):
        self.config = config
        self.crl_cfg = _crl_config(config, seed=seed, **shape)
        self.handle = L.Handle(self.crl_cfg, device)
        for key, value in (options or {}).items():      # crl_ppo_set_option: kernel-flavour switches of this handle
            self.handle.set_option(key, value)
        if params is None:
            params = networks.make_actor_critic(self.crl_cfg.n_act, self.crl_cfg.obs_dim, [self.crl_cfg.hidden] * 2, seed=init_seed)
        self.set_params(params)
        self.actor, self.critic = Policy(self, "actor"), Policy(self, "critic")

    def set_params(self, flat):
        self.handle.write(L.F_PARAMS, np.ascontiguousarray(flat, np.float32))

    def get_params(self):
        return self.handle.read(L.F_PARAMS)

    def close(self):
        self.handle.close()


def get_action(obs, actor: Policy, u=None, rng=None):
    """ppo.jl:21-32. Returns (action, logprob_action); actions are 1-based like the reference's `Base.OneTo(2)`.
    `u` are the uniform Float64 draws StatsBase.sample would take from the global RNG (one per column)."""
    obs = np.asfortranarray(obs, np.float32)
    if obs.ndim == 1:
        obs = obs[:, None]
    n = obs.shape[1]
    if u is None:
        u = (rng or np.random.default_rng()).random(n)
    a, lp, _ = actor.agent.handle.policy_act(obs, u, with_value=False)
    return a.astype(np.int64) + 1, lp


def logprob_actions(obs, actor: Policy, actions):
    """ppo.jl:34-45. `actions` 1-based Int32 like the reference; entropy is the (n_act, batch) matrix (Q3)."""
    actions = np.asarray(actions)
    if actions.dtype != np.int32:
        raise TypeError("logprob_actions: actions must be Int32 (ppo.jl:34 AbstractVector{Int32})")
    return actor.agent.handle.logprob_actions(obs, actions - 1)


def gae(values, rewards, terminals, gamma, lam, *, mode=L.GAE_COMPAT, device=0, seg=0, tile=0, nt_loads=2):
    """ppo.jl:48-73 for one env: values [0,k], rewards [1,k], terminals [0,k] → advantages.
    In compat mode the last slot is 0.0 (the reference leaves it uninitialised, ppo.jl:62,66)."""
    values = np.asarray(values, np.float32); rewards = np.asarray(rewards, np.float32)
    terminals = np.asarray(terminals).astype(np.uint8)
    k = rewards.shape[0]
    if values.shape[0] != k + 1 or terminals.shape[0] != k + 1:
        raise ValueError("gae: values and terminals need length(rewards)+1 entries")
    if k == 0:
        return np.zeros(0, np.float32)
    adv, _ = L.gae_host(values[None, :k], rewards[None, :], terminals[None, :k], values[k:], terminals[k:], gamma, lam, mode, device, seg, tile, nt_loads)
    return adv[0]


def _linear_eta(config, update, num_updates):
    # ppo.jl:118-121 (update is 1-based); Float64 like the reference
    if not config.anneal_lr:
        return float(np.float32(config.lr))
    frac = 1.0 - (update - 1.0) / num_updates
    return frac * float(np.float32(config.lr))


EVAL_SEED = 0xE7A1    # default key of the evaluation envs: its own, so that a held-out score does not replay the training envs' initial states


def _check_eval_args(num_envs, episodes_per_env, seed, trace_steps):
    for name, v, lo in (("num_envs", num_envs, 1), ("episodes_per_env", episodes_per_env, 1), ("trace_steps", trace_steps, 0)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"evaluate: {name} must be an integer, got {type(v).__name__}")
        if v < lo:
            raise ValueError(f"evaluate: {name} must be >= {lo}, got {v}")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"evaluate: seed must be an integer in [0, 2^64), got {seed!r}")
    if num_envs > 1 << 20 or episodes_per_env > 4096 or num_envs * episodes_per_env > 1 << 24 or trace_steps * num_envs > 1 << 26:
        raise ValueError("evaluate: size past the cap (num_envs <= 1048576, episodes_per_env <= 4096, num_envs * episodes_per_env <= 16777216, "
                         "trace_steps * num_envs <= 67108864)")


def evaluate(agent, *, num_envs=256, episodes_per_env=1, greedy=True, seed=EVAL_SEED, trace_steps=0):
    """How good is the current policy? crl_ppo_evaluate: the agent's actor, frozen, plays `episodes_per_env` whole episodes on each of `num_envs`
    fresh envs of its kind, in one launch on the GPU (no reference counterpart: ppo.jl only logs the returns of its sampled training rollouts).
    greedy=True takes the largest logit (lowest index on a tie), False samples like get_action (ppo.jl:21-32). Training state is not touched.
    Returns {"report": {episodes, env_steps, return_mean, return_std, return_min, return_max, length_mean}, "returns", "lengths"} — the arrays
    are (episodes_per_env, num_envs) — plus "trace" (trace_steps, num_envs), the actions of the first trace_steps steps, when trace_steps > 0.
    Arguments are validated here, before the library is touched."""
    _check_eval_args(num_envs, episodes_per_env, seed, trace_steps)
    if not isinstance(greedy, (bool, np.bool_)):
        raise TypeError(f"evaluate: greedy must be a bool, got {type(greedy).__name__}")
    if not isinstance(agent, Agent):
        raise TypeError("evaluate: agent must be a cleanrl_jl_amd Agent (PPO); A2C / DQN handles have no evaluation entry")
    return agent.handle.evaluate(num_envs, episodes_per_env, L.EVAL_GREEDY if greedy else L.EVAL_SAMPLE, seed, trace_steps)


def diagnose(agent, per_sample=False):
    """Is the update healthy? crl_ppo_diagnose: one read-only launch over the rollout buffer the agent currently holds, with its current parameters
    (after an update: the last rollout against the post-update policy; no reference counterpart). Returns the fields of crl_ppo_diag as a dict —
    approx_kl, old_approx_kl, clipfrac, entropy (per sample: n_act x the reference's entropy_loss), explained_variance (stored values) and
    explained_variance_new (current critic), ratio_min / ratio_max, n, n_clipped and the raw Float64 sums; per_sample=True adds "new_logprob" and
    "new_value" as (num_envs, num_steps) arrays. Training state is not touched."""
    if not isinstance(per_sample, (bool, np.bool_)):
        raise TypeError(f"diagnose: per_sample must be a bool, got {type(per_sample).__name__}")
    if not isinstance(agent, Agent):
        raise TypeError("diagnose: agent must be a cleanrl_jl_amd Agent (PPO); A2C / DQN handles have no diagnostics entry")
    return agent.handle.diagnose(bool(per_sample))


def train(agent: Agent, num_updates=None, log_every=1, episode_records=0, eval_every=0, eval_envs=256, eval_episodes=1, diag_every=0):
    """`train!`-style driver = the `for update in 1:num_updates` loop of ppo.jl:117-253, fully on device.
    Emits the reference's two records: "Episode Statistics" and "Training Statistics". By default the episode record is one
    aggregate per rollout (with 65536 envs the reference's one-record-per-episode is ~10^5 log lines per update);
    `episode_records=N` turns on the device ring (crl_episode_ring_enable) and logs up to N episodes per rollout one by one,
    in the reference's order (step, then env; global_step as in ppo.jl:124,148).
    `eval_every=N > 0` adds an "Evaluation Statistics" record (eval_return_mean, eval_return_std, eval_length_mean, global_step) after every N-th
    update: a greedy crl_ppo_evaluate of the parameters that update left, on eval_envs fresh envs x eval_episodes episodes. 0 (default) keeps the
    record stream what it was. `diag_every=N > 0` adds a "Policy Diagnostics" record (approx_kl, old_approx_kl, clipfrac, entropy, explained_variance,
    global_step) after every N-th update: crl_ppo_diagnose of that update's rollout against the parameters it left; placed like the evaluation record
    (in front of it when both fall on one update). 0 (default) keeps the record stream what it was."""
    if diag_every:
        if isinstance(diag_every, bool) or not isinstance(diag_every, (int, np.integer)) or diag_every < 0:
            raise ValueError(f"train: diag_every must be an integer >= 0, got {diag_every!r}")
    if eval_every:
        if isinstance(eval_every, bool) or not isinstance(eval_every, (int, np.integer)) or eval_every < 0:
            raise ValueError(f"train: eval_every must be an integer >= 0, got {eval_every!r}")
        _check_eval_args(eval_envs, eval_episodes, EVAL_SEED, 0)
    cfg = agent.config
    batch_size = cfg.num_steps * cfg.num_envs
    if num_updates is None:
        num_updates = max(1, cfg.total_timesteps // batch_size)  # ppo.jl:91
    h = agent.handle
    if episode_records:
        h.episode_ring_enable(int(episode_records))
    if h.iteration == 0:
        h.env_reset()
    start_time = time.time()
    last_log_step = 0

    def emit(rep):
        """The records of one update, in the reference's order: its episodes (ppo.jl:147-165), then its 16 minibatches (ppo.jl:246-248)."""
        nonlocal last_log_step
        base = rep["iteration"] * batch_size
        global_step = base + batch_size
        ep = rep["episodes"]
        if episode_records:
            for step, env, ret, length in rep["records"]:
                gs = base + (step + 1) * cfg.num_envs                              # ppo.jl:124 global_step += num_envs
                inc = 0 if last_log_step == 0 else gs - last_log_step
                log.info("Episode Statistics", extra={"crl": dict(
                    episode_return=ret, episode_length=length, global_step=gs,
                    steps_per_sec=int(gs / max(time.time() - start_time, 1e-9)), log_step_increment=inc)})
                last_log_step = gs
        elif ep["episodes"] > 0:
            inc = 0 if last_log_step == 0 else global_step - last_log_step
            log.info("Episode Statistics", extra={"crl": dict(
                episode_return=ep["return_sum"] / ep["episodes"], episode_length=ep["length_sum"] / ep["episodes"],
                global_step=global_step, steps_per_sec=int(global_step / max(time.time() - start_time, 1e-9)), log_step_increment=inc)})
            last_log_step = global_step
        if log_every:
            for s in rep["stats"]:
                inc = 0 if last_log_step == 0 else global_step - last_log_step
                log.info("Training Statistics", extra={"crl": dict(
                    loss=s["loss"], pg_loss=s["pg_loss"], v_loss=s["v_loss"], entropy_loss=s["entropy_loss"],
                    log_step_increment=inc)})
                last_log_step = global_step

    # Pipelined read-back (crl_ppo_iterate_async): update k's records are picked up after update k + 1 has been enqueued, so the GPU never idles while the host
    # logs; the record stream is the same, one update late, and crl_ppo_drain hands over the last one.
    def emit_eval(update):
        # the evaluation reads the parameters update `update` (1-based) left: it runs behind that update on the stream, before the next one is enqueued
        ev = h.evaluate(eval_envs, eval_episodes, L.EVAL_GREEDY, EVAL_SEED, 0, want_arrays=False)["report"]
        log.info("Evaluation Statistics", extra={"crl": dict(
            eval_return_mean=ev["return_mean"], eval_return_std=ev["return_std"], eval_length_mean=ev["length_mean"],
            global_step=update * batch_size)})

    def emit_diag(update):
        # the buffer still holds update `update`'s rollout and the parameters are the ones it left: the next update has not been enqueued
        d = h.diagnose()
        log.info("Policy Diagnostics", extra={"crl": dict(
            approx_kl=d["approx_kl"], old_approx_kl=d["old_approx_kl"], clipfrac=d["clipfrac"], entropy=d["entropy"],
            explained_variance=d["explained_variance"], global_step=update * batch_size)})

    for update in range(1, num_updates + 1):
        rep = h.iterate_async(want_stats=bool(log_every))
        if rep is not None:
            emit(rep)
        evaluating = bool(eval_every) and update % eval_every == 0
        diagnosing = bool(diag_every) and update % diag_every == 0
        if evaluating or diagnosing:
            # keep the record order of the stream: update's own records first (they are one call late otherwise), then its diagnostics and evaluation
            rep = h.drain(want_stats=bool(log_every))
            if rep is not None:
                emit(rep)
            if diagnosing:
                emit_diag(update)
            if evaluating:
                emit_eval(update)
    rep = h.drain(want_stats=bool(log_every))
    if rep is not None:
        emit(rep)
    return agent


# ---------------------------------------------------------------------------------------------------------------- device-resident external envs
# The device-env protocol. `ppo(config, env=obj)` / `train_external(agent, obj)` drive any object with
#   num_envs, obs_dim, n_act          ints (ppo.jl:85-86 reads them off the env's spaces)
#   reset() -> (obs, done)            ppo.jl:112-115: obs (obs_dim, num_envs) Float32, done [num_envs] UInt8
#   step(action) -> (reward, next_obs, next_done)
#                                     ppo.jl:130-144: `action` is the pointer-like the agent wrote its 0-based Int32 actions [num_envs] to; reward
#                                     [num_envs] Float32; terminated envs are already reset, next_obs is what the policy sees next
#   stream (optional)                 the hipStream_t (int) the env enqueues its work on; passed as peer_stream, so neither side waits on the host
#   action (optional)                 pointer-like [num_envs] Int32 the env wants the actions written into (a torch env hands over its own tensor and
#                                     gets it back in step); without it the loop allocates a DeviceBuffer
# where every pointer-like is an int device address or an object with data_ptr() (a torch tensor, a DeviceBuffer) into buffers the ENV owns, on the
# agent's device. Nothing in the loop touches host memory; the one host wait per update is crl_ppo_update's (4 / 2 / 64 path only).
_PROTOCOL = ("num_envs", "obs_dim", "n_act", "reset", "step")


def check_device_env(env):
    """TypeError naming the first protocol attribute `env` lacks (nothing on the device is touched)."""
    for name in _PROTOCOL:
        if not hasattr(env, name):
            raise TypeError(f"env={type(env).__name__} is neither an env name nor a device env: it has no `{name}` "
                            f"(the device-env protocol needs {', '.join(_PROTOCOL)} and optionally stream, action)")
    for name in ("reset", "step"):
        if not callable(getattr(env, name)):
            raise TypeError(f"device env: `{name}` must be callable")
    return env


class LibraryEnv:
    """One of the library's on-device envs ("cartpole", "mountaincar", "acrobot") behind the device-env protocol: a second handle's built-in env stepped
    with crl_env_reset + crl_env_step_device into device buffers this object owns (hipMalloc through ctypes; torch is not needed). The reference
    implementation of the protocol — and the env of its tests. stale_obs / env_id_offset as for an Agent: with the Agent's defaults the env is the one a
    built-in-env Agent of the same seed trains on."""

    def __init__(self, name, num_envs, seed=0x5EED, device=0, stale_obs=True, env_id_offset=0):
        shape = env_shape(name)
        self.name, self.num_envs, self.obs_dim, self.n_act = name, int(num_envs), shape["obs_dim"], shape["n_act"]
        cfg = _crl_config(PPOConfig(num_envs=self.num_envs, num_steps=1, num_minibatches=1, total_timesteps=self.num_envs), seed=seed,
                          stale_obs=stale_obs, env_id_offset=env_id_offset, hidden=64, **shape)
        self.handle = L.Handle(cfg, device)          # only its env is used: its parameters stay unset
        self.stream = self.handle.stream
        n, d = self.num_envs, self.obs_dim
        self.obs, self.reward, self.done = L.DeviceBuffer(4 * n * d, device), L.DeviceBuffer(4 * n, device), L.DeviceBuffer(n, device)
        self.gstep = 0

    def reset(self):
        """ppo.jl:112-115. (Set-up, not the stepping path: the initial observation is read from CRL_F_CUR_OBS through the host once.)"""
        h = self.handle
        h.env_reset()
        self.obs.write(h.read(L.F_CUR_OBS)); self.done.write(h.read(L.F_NEXT_DONE))
        self.gstep = 0
        return self.obs, self.done

    def step(self, action):
        self.handle.env_step_device(action, self.gstep, self.obs, self.reward, self.done)   # on the env handle's own stream
        self.gstep += 1
        return self.reward, self.obs, self.done

    def close(self):
        self.handle.close()
        for b in (self.obs, self.reward, self.done):
            b.close()


def train_external(agent: Agent, env, num_updates=None, log_every=1, episode_records=0, eval_every=0, diag_every=0):
    """The `for update in 1:num_updates` loop of ppo.jl:117-253 with the env OUTSIDE the library but on the same GPU (the device-env protocol above):
    reset once; per step crl_rollout_act_device -> env.step -> crl_rollout_record_device; per update crl_ppo_update. Emits the records of `train`:
    "Episode Statistics" (one aggregate per rollout, or one per episode with episode_records=N), "Training Statistics", and "Policy Diagnostics" every
    diag_every-th update. eval_every is refused: crl_ppo_evaluate has no external env to run."""
    if eval_every:
        raise ValueError("train_external: eval_every is not available — crl_ppo_evaluate runs the library's own envs and has none for an external env")
    if diag_every:
        if isinstance(diag_every, bool) or not isinstance(diag_every, (int, np.integer)) or diag_every < 0:
            raise ValueError(f"train_external: diag_every must be an integer >= 0, got {diag_every!r}")
    check_device_env(env)
    cfg = agent.config
    if (env.num_envs, env.obs_dim, env.n_act) != (cfg.num_envs, agent.crl_cfg.obs_dim, agent.crl_cfg.n_act):
        raise ValueError(f"train_external: the env has (num_envs, obs_dim, n_act) = {(env.num_envs, env.obs_dim, env.n_act)}, the agent "
                         f"{(cfg.num_envs, agent.crl_cfg.obs_dim, agent.crl_cfg.n_act)}")
    batch_size = cfg.num_steps * cfg.num_envs
    if num_updates is None:
        num_updates = max(1, cfg.total_timesteps // batch_size)  # ppo.jl:91
    h = agent.handle
    if episode_records:
        h.episode_ring_enable(int(episode_records))
    peer = getattr(env, "stream", None) or None
    action = getattr(env, "action", None)
    if action is None:
        action = L.DeviceBuffer(4 * cfg.num_envs, agent.handle.device)
    start_time = time.time()
    last_log_step = 0
    obs, done = env.reset()                                                        # ppo.jl:112-115
    for update in range(1, num_updates + 1):
        base = (update - 1) * batch_size
        for step in range(cfg.num_steps):                                          # ppo.jl:123-166
            h.act_device(step, obs, done, action, peer_stream=peer)
            reward, obs, done = env.step(action)
            h.record_device(step, reward, obs, done, peer_stream=peer)
        # the episode records of this rollout are read before the next rollout's first step clears them; the reads are this loop's host waits
        ep = h.episode_stats()
        records = h.episode_records()[0] if episode_records else []
        stats = h.update(want_stats=bool(log_every))                               # ppo.jl:168-253
        global_step = base + batch_size
        if episode_records:
            for step, _env, ret, length in records:
                gs = base + (step + 1) * cfg.num_envs
                inc = 0 if last_log_step == 0 else gs - last_log_step
                log.info("Episode Statistics", extra={"crl": dict(
                    episode_return=ret, episode_length=length, global_step=gs,
                    steps_per_sec=int(gs / max(time.time() - start_time, 1e-9)), log_step_increment=inc)})
                last_log_step = gs
        elif ep["episodes"] > 0:
            inc = 0 if last_log_step == 0 else global_step - last_log_step
            log.info("Episode Statistics", extra={"crl": dict(
                episode_return=ep["return_sum"] / ep["episodes"], episode_length=ep["length_sum"] / ep["episodes"],
                global_step=global_step, steps_per_sec=int(global_step / max(time.time() - start_time, 1e-9)), log_step_increment=inc)})
            last_log_step = global_step
        for s in stats or []:
            inc = 0 if last_log_step == 0 else global_step - last_log_step
            log.info("Training Statistics", extra={"crl": dict(
                loss=s["loss"], pg_loss=s["pg_loss"], v_loss=s["v_loss"], entropy_loss=s["entropy_loss"], log_step_increment=inc)})
            last_log_step = global_step
        if diag_every and update % diag_every == 0:
            d = h.diagnose()
            log.info("Policy Diagnostics", extra={"crl": dict(
                approx_kl=d["approx_kl"], old_approx_kl=d["old_approx_kl"], clipfrac=d["clipfrac"], entropy=d["entropy"],
                explained_variance=d["explained_variance"], global_step=update * batch_size)})
    return agent


def ppo(config: PPOConfig = None, *, device=0, seed=0x5EED, init_seed=0, params=None, episode_records=4096, run_name="ppo-2-test",
        logger_kw=None, env=None, eval_every=0, eval_envs=256, eval_episodes=1, diag_every=0, **shape):
    """ppo.jl:75 — `ppo(config::PPOConfig=PPOConfig())`: CartPole, 2x64 actor/critic, whole loop on one MI355X. `env="cartpole" | "mountaincar" |
    "acrobot"` is the one-line change of ppo.jl:82: obs_dim / n_act follow from it (ppo.jl:85-86). Like the Julia shell
    (julia/CleanRLHip.jl) it logs ONE "Episode Statistics" record per finished episode in the reference's order (ppo.jl:147-165), up
    to `episode_records` per rollout (the device ring's capacity; 0 = one aggregate record per update), and the 16 "Training
    Statistics" records of every update (ppo.jl:246-248). `logger_kw` goes to Logger.make_logger (logger.jl:7); `shape` keywords
    (obs_dim, n_act, hidden, env_kind, gae_mode, stale_obs, shuffle_mode) to the Agent — the reference derives them from the env
    (ppo.jl:85-87). `eval_every=N > 0`: an "Evaluation Statistics" record after every N-th update (see train / evaluate);
    `diag_every=N > 0`: a "Policy Diagnostics" record after every N-th update (see train / diagnose). Both are validated before a device is touched.
    `env=<object>` (not a string): a device-resident external env following the device-env protocol above — the agent is built with
    env_kind=ENV_EXTERNAL and the object's obs_dim / n_act, and the loop is train_external; an object that lacks a protocol attribute is a TypeError."""
    if isinstance(diag_every, bool) or not isinstance(diag_every, (int, np.integer)) or diag_every < 0:
        raise ValueError(f"ppo: diag_every must be an integer >= 0, got {diag_every!r}")
    external = env is not None and not isinstance(env, str)
    if external:     # a device env (see the protocol above): its shape comes from the object, the loop is train_external
        check_device_env(env)
        if eval_every:
            raise ValueError("ppo: eval_every is not available with a device env (crl_ppo_evaluate has no external env)")
        for name in ("env_kind", "obs_dim", "n_act"):
            if name in shape:
                raise ValueError(f"ppo: {name} follows from the device env, do not pass it")
    from . import logger as _logger
    config = config or PPOConfig()
    if external:
        if env.num_envs != config.num_envs:
            raise ValueError(f"ppo: the env has num_envs={env.num_envs}, the config {config.num_envs}")
        _logger.make_logger(run_name, **({"to_terminal": False} | (logger_kw or {})))
        agent = Agent(config, device=device, seed=seed, init_seed=init_seed, params=params,
                      **(shape | dict(env_kind=L.ENV_EXTERNAL, obs_dim=int(env.obs_dim), n_act=int(env.n_act))))
        try:
            train_external(agent, env, episode_records=episode_records, diag_every=diag_every)
            return agent.get_params()
        finally:
            agent.close()
    shape = env_shape(env, **shape)      # ppo.jl:82,85-86 (an unknown env is a ValueError before anything is created)
    _logger.make_logger(run_name, **({"to_terminal": False} | (logger_kw or {})))
    agent = Agent(config, device=device, seed=seed, init_seed=init_seed, params=params, **shape)
    try:
        train(agent, episode_records=episode_records, eval_every=eval_every, eval_envs=eval_envs, eval_episodes=eval_episodes, diag_every=diag_every)
        return agent.get_params()
    finally:
        agent.close()
