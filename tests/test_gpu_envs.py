"""On-device MountainCar / Acrobot (csrc/env.hpp) against the numpy restatement of their contracts (tests/envs_ref.py), through every layer:
crl_env_step on grids of states, resets against the Philox words, every rollout route against every other and against a replay through
crl_env_step, whole iterations against a host-driven twin, return_max with negative returns, and learning on Acrobot against a control whose
envs are stepped by the restatement on the host.

Tolerances are measured, not guessed: the single-step bar is 4 x the largest error of the SAME restatement evaluated in numpy Float32 against
Float64 on the same inputs, per variable (the margin covers a different but equally rounded polynomial and FMA order); the numbers go to
profiles/env_step_error.json when CRL_WRITE_PROFILES=1."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import envs_ref as R
import oraclelib as O
from test_gpu_parity import crl  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED
WRITE = os.environ.get("CRL_WRITE_PROFILES") == "1"


def _agent(crl, name, hidden, nt, k, params=None, kind=None, **kw):   # noqa: F811
    e = R.ENVS[name]
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=kw.pop("total_timesteps", nt * k * 10))
    return crl.Agent(cfg, params=params, obs_dim=e["obs_dim"], n_act=e["n_act"], hidden=hidden, env_kind=e["kind"] if kind is None else kind,
                     seed=SEED, **kw)


def _write_state(h, F, name, s, t):
    e = R.ENVS[name]
    full = np.zeros((e["obs_dim"], s.shape[1]), np.float32)
    full[:e["n_state"]] = s
    h.write(F.F_ENV_STATE, full); h.write(F.F_ENV_T, t.astype(np.int32))


def _philox_uniforms(gids, gstep, stream):
    out = np.zeros((len(gids), 4), np.uint32)
    w = (C.c_uint32 * 4)()
    for i, g in enumerate(gids):
        O.lib().orc_philox(int(g), gstep & 0xFFFFFFFF, gstep >> 32, stream, SEED & 0xFFFFFFFF, SEED >> 32, w)
        out[i] = w[:]
    return R.uniforms24(out)                                           # (4, n)


def _circ(a, b):
    d = np.abs(a - b)
    return np.minimum(d, np.abs(d - 2 * np.pi))


def _state_err(name, got, want):
    """per-variable largest |error|; Acrobot's angles by circular distance (a result within rounding of +-pi wraps to either end)"""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    if name == "acrobot":
        return np.array([_circ(got[0], want[0]).max(), _circ(got[1], want[1]).max(), np.abs(got[2] - want[2]).max(), np.abs(got[3] - want[3]).max()])
    return np.abs(got - want).max(axis=1)


# ------------------------------------------------------------------------------------------------------------- single steps
@pytest.mark.parametrize("hidden", [64, 256])
@pytest.mark.parametrize("name", ["mountaincar", "acrobot"])
def test_single_steps_match_the_restatement(crl, name, hidden):   # noqa: F811
    e = R.ENVS[name]; F = crl._lib
    s, t = R.state_grid(name)
    n = s.shape[1]
    agent = _agent(crl, name, hidden, n, 8, stale_obs=True)
    h = agent.handle
    rec = {"env": name, "hidden": hidden, "cases": 0, "near_threshold": 0, "state": {}, "obs": {}}
    worst = {k: np.zeros(e["n_state"] if k[1] == "s" else e["obs_dim"]) for k in (("f32", "s"), ("hip", "s"), ("f32", "o"), ("hip", "o"))}
    near_total = 0
    for a in range(e["n_act"]):
        act = np.full(n, a, np.int32)
        s64, t64, r64, d64, m64 = e["step"](s.astype(np.float64), t, act, np.float64)
        s32, _, _, d32, m32 = e["step"](s, t, act, np.float32)
        o64 = e["obs"](s64, np.float64); o32 = e["obs"](s32, np.float32)
        _write_state(h, F, name, s, t)
        # a forced terminal resets the env: read the pre-reset observation (stale_obs) and recover the stepped state from non-terminal envs only
        obs, rew, done = h.env_step(act, gstep=7)
        tg = h.read(F.F_ENV_T); sg = h.read(F.F_ENV_STATE)[:e["n_state"]]
        # float tolerance of the goal margin: 4 x the Float32 restatement's own margin error
        mtol = 4 * np.abs(m32.astype(np.float64) - m64).max()
        near = (np.abs(m64) <= mtol) & (t64 < R.MAX_STEPS)
        near_total += int(near.sum())
        ok = ~near
        print(f"{name} hidden {hidden} a={a}: done mismatches {int(np.sum(done.astype(bool) != d64))}, near-threshold states {int(near.sum())} (margin tol {mtol:.3g})")
        assert np.array_equal(done.astype(bool)[ok], d64[ok]) and np.array_equal(rew[ok], r64[ok].astype(np.float32))
        assert np.array_equal(tg[ok], np.where(d64, 0, t64)[ok])
        assert np.array_equal(h.read(F.F_NEXT_DONE)[ok], d64[ok].astype(np.uint8))
        live = ok & ~d64 & ~done.astype(bool)
        for key, got, want in ((("f32", "s"), s32[:, live], s64[:, live]), (("hip", "s"), sg[:, live], s64[:, live])):
            worst[key] = np.maximum(worst[key], _state_err(name, got, want))
        for key, got, want in ((("f32", "o"), o32[:, ok], o64[:, ok]), (("hip", "o"), obs[:, ok], o64[:, ok])):
            worst[key] = np.maximum(worst[key], np.abs(got.astype(np.float64) - want).max(axis=1))
        rec["cases"] += n
    rec["near_threshold"] = near_total
    assert near_total <= 1e-3 * rec["cases"], "the near-threshold exception may cover at most 0.1 % of the cases"
    for part, k in (("state", "s"), ("obs", "o")):
        f32, hip = worst[("f32", k)], worst[("hip", k)]
        bar = 4 * f32
        rec[part] = {"float32_numpy_error": f32.tolist(), "hip_error": hip.tolist(), "bar": bar.tolist()}
        print(f"{name} hidden {hidden} {part}: float32-numpy error {f32}, HIP error {hip}, bar {bar}")
    if WRITE:
        path = os.path.join(ROOT, "profiles", "env_step_error.json")
        allrec = json.load(open(path)) if os.path.exists(path) else {}
        allrec[f"{name}/{hidden}"] = rec
        json.dump(allrec, open(path, "w"), indent=1, sort_keys=True)
    for part in ("state", "obs"):
        assert np.all(np.array(rec[part]["hip_error"]) <= np.array(rec[part]["bar"])), (part, rec[part])
    agent.close()


# ------------------------------------------------------------------------------------------------------------- resets
@pytest.mark.parametrize("hidden", [64, 256])
@pytest.mark.parametrize("name", ["mountaincar", "acrobot"])
def test_resets_are_the_map_of_the_philox_words(crl, name, hidden):   # noqa: F811
    """Construction: stream 2 at gstep 0 (as cartpole's). After a forced terminal (t = max_steps - 1): stream 1 at the caller's gstep. Bit-equal:
    0.2f * u rounds once and the subtraction once, the same two Float32 operations on both sides (contraction is off in the kernel)."""
    e = R.ENVS[name]; F = crl._lib
    nt, off = 96, 1000
    for stale in (True, False):
        agent = _agent(crl, name, hidden, nt, 8, stale_obs=stale, env_id_offset=off)
        h = agent.handle
        h.env_reset()
        gids = off + np.arange(nt)
        want0 = e["reset"](_philox_uniforms(gids, 0, 2))
        s0 = h.read(F.F_ENV_STATE)
        assert np.array_equal(s0[:e["n_state"]], want0) and not s0[e["n_state"]:].any() and not h.read(F.F_ENV_T).any()
        assert np.array_equal(h.read(F.F_CUR_OBS), e["obs"](want0, np.float32)) or name == "acrobot"
        if name == "acrobot":   # cos / sin of the fresh state: the kernel's polynomial against numpy's Float32, 4 ulp of 1
            assert np.abs(h.read(F.F_CUR_OBS).astype(np.float64) - e["obs"](want0.astype(np.float64))).max() < 4 * 2.0 ** -23
        h.write(F.F_ENV_T, np.full(nt, R.MAX_STEPS - 1, np.int32))
        gstep = (5 << 32) + 12345                                       # both halves of the 64-bit step key the stream
        pre64, _, _, d64, _ = e["step"](want0.astype(np.float64), np.full(nt, R.MAX_STEPS - 1), np.ones(nt, int), np.float64)
        obs, rew, done = h.env_step(np.ones(nt, np.int32), gstep=gstep)
        want1 = e["reset"](_philox_uniforms(gids, gstep, 1))
        assert done.all() and not rew.any() and not h.read(F.F_ENV_T).any()
        assert np.array_equal(h.read(F.F_ENV_STATE)[:e["n_state"]], want1)
        fresh64 = e["obs"](want1.astype(np.float64)); stale64 = e["obs"](pre64)
        assert np.abs(obs.astype(np.float64) - (stale64 if stale else fresh64)).max() < 1e-5   # which state the policy sees (Q7); values pinned above
        assert np.array_equal(h.read(F.F_CUR_OBS), obs)
        agent.close()


def test_env_step_errors_and_cartpole(crl):   # noqa: F811
    F = crl._lib
    cfg = crl.PPOConfig(num_envs=64, num_steps=8, total_timesteps=64 * 8 * 10)
    for kind in (F.ENV_SYNTHETIC, F.ENV_EXTERNAL):
        a = crl.Agent(cfg, obs_dim=6, n_act=3, hidden=64, env_kind=kind)
        with pytest.raises(crl.CrlError, match="stateful on-device env"):
            a.handle.env_step(np.zeros(64, np.int32))
        a.close()
    for kind, D, A in ((F.ENV_ACROBOT, 4, 2), (F.ENV_MOUNTAINCAR, 6, 3)):
        with pytest.raises(crl.CrlError, match="needs obs_dim"):
            crl.Agent(cfg, obs_dim=D, n_act=A, hidden=64, env_kind=kind)
    a = _agent(crl, "acrobot", 64, 64, 8)
    with pytest.raises(crl.CrlError, match="outside"):
        a.handle.env_step(np.full(64, 3, np.int32))
    a.close()
    # CartPole on the 4 / 2 / 64 path: crl_env_step reproduces what the oracle's step gives from the same state
    a = crl.Agent(cfg, seed=SEED); h = a.handle
    h.env_reset()
    s0 = h.read(F.F_ENV_STATE).copy(); act = (np.arange(64) & 1).astype(np.int32)
    obs, rew, done = h.env_step(act, gstep=3)
    st = np.ascontiguousarray(s0.T.copy()); tt = np.zeros(64, np.int32); dd = np.zeros(64, np.int32)
    for i in range(64):
        row = st[i].copy(); t1 = C.c_int32(0); d1 = C.c_int32(0)
        O.lib().orc_cartpole_step(row.ctypes.data_as(C.POINTER(C.c_float)), C.byref(t1), int(act[i]), 500, C.byref(d1))
        st[i] = row; tt[i] = t1.value; dd[i] = d1.value
    assert not dd.any() and np.array_equal(obs, st.T) and np.array_equal(rew, np.ones(64, np.float32)) and np.array_equal(h.read(F.F_ENV_T), tt)
    a.close()


# ------------------------------------------------------------------------------------------------------------- routes
ROUTES = {256: [("rs", {}), ("pc", {"wide_rs": 25}), ("persist1", {"wide_rollout_persist": 1}), ("per-step", {"wide_rollout_persist": 0})],
          64: [("per-step", {})]}
FIELDS = ("F_OBS", "F_REWARD", "F_TERMINAL")


def _rollout(crl, name, hidden, nt, k, params, opts, iters=2):   # noqa: F811
    F = crl._lib
    agent = _agent(crl, name, hidden, nt, k, params=params, options=opts)
    h = agent.handle
    h.env_reset()
    out = []
    for it in range(iters):
        start = {"state": h.read(F.F_ENV_STATE).copy(), "t": h.read(F.F_ENV_T).copy(), "cur": h.read(F.F_CUR_OBS).copy()}
        h.rollout_run()
        # crl_rollout_run does not advance the handle's iteration: iteration 0's streams every time — start the second pass from where the first ended
        out.append({"start": start, **{f: h.read(getattr(F, f)).copy() for f in FIELDS + ("F_ACTION", "F_ENV_STATE", "F_ENV_T", "F_CUR_OBS", "F_NEXT_DONE")},
                    "stats": h.episode_stats()})
    return agent, out


@pytest.mark.parametrize("hidden", [64, 256])
@pytest.mark.parametrize("name", ["mountaincar", "acrobot"])
@pytest.mark.parametrize("nt", [128, 70])
def test_every_rollout_route_agrees_and_replays(crl, name, hidden, nt):   # noqa: F811
    """num_envs = 128 admits every one-launch kernel at hidden 256; 70 (not a multiple of 64) declines to wide_rollout_persist_kernel / per-step launches."""
    e = R.ENVS[name]; F = crl._lib
    k = 48
    ocfg = O.make_config(num_envs=nt, num_steps=k, obs_dim=e["obs_dim"], n_act=e["n_act"], hidden=hidden, env_kind=1)
    rng = np.random.default_rng(3)
    params = O.orthogonal_params(ocfg, 3) + (0.05 * rng.standard_normal(O.lib().orc_param_count(ocfg))).astype(np.float32)
    off = O.param_offsets(ocfg); params[off[4]:off[5]] *= 30             # spread the logits: every action occurs
    runs = []
    for label, opts in ROUTES[hidden]:
        agent, out = _rollout(crl, name, hidden, nt, k, params, opts, iters=1)
        runs.append((label, agent, out[0]))
    ref_label, ref_agent, ref = runs[0]
    assert len(set(ref["F_ACTION"].ravel().tolist())) == e["n_act"]
    for label, agent, got in runs[1:]:
        diff = ref["F_ACTION"] != got["F_ACTION"]                        # (nt, k)
        first = np.where(diff.any(axis=1), diff.argmax(axis=1), k)        # per env: first step whose action differs (k: none)
        for env in np.flatnonzero(first < k):                            # the margin rule: such a draw sits within 1e-6 of a CDF knot
            stp = int(first[env])
            u = O.lib().orc_u53(SEED, int(env), stp, 0)
            _, _, _, margin = O.get_action(ocfg, params, np.asfortranarray(ref["F_OBS"][:, env, stp:stp + 1]), np.array([u]))
            assert margin[0] <= 1e-6, (label, env, stp, margin)
        assert (first < k).mean() <= 0.02
        steps = np.arange(k)[None, :]
        same = steps <= first[:, None]                                    # up to and including the diverging step the inputs agree
        assert np.array_equal(ref["F_OBS"][:, same], got["F_OBS"][:, same]), label
        after = steps < first[:, None]                                    # its outputs agree while the actions did
        assert np.array_equal(ref["F_REWARD"][after], got["F_REWARD"][after]) and np.array_equal(ref["F_TERMINAL"][same], got["F_TERMINAL"][same]), label
        whole = first == k
        for f in ("F_ENV_STATE", "F_CUR_OBS"):
            assert np.array_equal(ref[f][:, whole], got[f][:, whole]), (label, f)
        for f in ("F_ENV_T", "F_NEXT_DONE"):
            assert np.array_equal(ref[f][whole], got[f][whole]), (label, f)
    # replay of every route's own recorded actions through crl_env_step (gstep = iteration * k + step, iteration 0) reproduces its buffer bit for bit
    for label, agent, got in runs:
        h = agent.handle
        h.write(F.F_ENV_STATE, got["start"]["state"]); h.write(F.F_ENV_T, got["start"]["t"]); h.write(F.F_CUR_OBS, got["start"]["cur"])
        cur = got["start"]["cur"]; nd = np.zeros(nt, np.uint8)
        for stp in range(k):
            assert np.array_equal(got["F_OBS"][:, :, stp], cur) and np.array_equal(got["F_TERMINAL"][:, stp], nd), (label, stp)
            cur, rew, nd = h.env_step(got["F_ACTION"][:, stp], gstep=stp)
            assert np.array_equal(got["F_REWARD"][:, stp], rew), (label, stp)
        assert np.array_equal(h.read(F.F_ENV_STATE), got["F_ENV_STATE"]) and np.array_equal(h.read(F.F_ENV_T), got["F_ENV_T"]), label
        assert np.array_equal(cur, got["F_CUR_OBS"]) and np.array_equal(nd, got["F_NEXT_DONE"]), label
        agent.close()


# ------------------------------------------------------------------------------------------------------------- return_max
@pytest.mark.parametrize("name,hidden", [("acrobot", 256), ("acrobot", 64), ("mountaincar", 256)])
def test_return_max_is_the_true_maximum_of_negative_returns(crl, name, hidden):   # noqa: F811
    F = crl._lib
    nt, k = 128, 64
    agent = _agent(crl, name, hidden, nt, k); h = agent.handle
    h.env_reset()
    h.episode_ring_enable(4096)
    h.rollout_run()                                                     # no episode can finish in 64 steps from t = 0 (no goal from rest, limit 200)
    es = h.episode_stats()
    if es["episodes"] == 0:
        assert es["return_max"] == 0.0
    t = h.read(F.F_ENV_T); t[:] = R.MAX_STEPS - 1 - (np.arange(nt) % 50); h.write(F.F_ENV_T, t)
    h.rollout_run()
    es = h.episode_stats(); recs, n_eps = h.episode_records()
    rets = np.array([r[2] for r in recs], np.float64)
    assert es["episodes"] >= nt and len(rets) == es["episodes"] == n_eps
    assert es["return_max"] < 0 and es["return_max"] == rets.max() and abs(es["return_sum"] - rets.sum()) < 1e-6 * abs(rets.sum())
    # the async report carries the same number
    h.iterate_async(want_stats=False); rep = h.drain(want_stats=False)
    r2 = np.array([r[2] for r in rep["records"]], np.float64)
    assert rep["episodes"]["return_max"] == (r2.max() if len(r2) else 0.0)
    agent.close()


def test_return_max_on_cartpole_is_unchanged(crl):   # noqa: F811
    cfg = crl.PPOConfig(num_envs=64, num_steps=128, total_timesteps=64 * 128 * 10)
    a = crl.Agent(cfg, seed=SEED); h = a.handle
    h.env_reset(); h.episode_ring_enable(4096); h.rollout_run()
    es = h.episode_stats(); recs, _ = h.episode_records()
    rets = [r[2] for r in recs]
    assert es["episodes"] > 0 and es["return_max"] == max(rets) > 0
    a.close()


# ------------------------------------------------------------------------------------------------------------- whole iterations
def _host_iteration(crl, dev_h, twin, cfg, it, num_updates, stepper):   # noqa: F811
    """One ppo.jl:117-253 body on an ENV_EXTERNAL twin: `stepper(actions, gstep) -> (next_obs, reward, done)` steps the envs, crl_policy_act samples
    with the device's uniforms, crl_rollout_store fills the buffer, then the same update calls crl_ppo_iterate makes on the layer-wise path."""
    F = crl._lib
    nt, k = cfg.num_envs, cfg.num_steps
    cur, nd = stepper.cur, stepper.nd
    flips = 0
    dev_actions = dev_h.read(F.F_ACTION) if dev_h is not None else None
    for stp in range(k):
        gstep = it * k + stp
        u = np.array([O.lib().orc_u53(SEED, e, gstep, 0) for e in range(nt)])
        a, lp, v = twin.policy_act(cur, u)
        if dev_h is not None:                                            # knot flips between two kernels' logits: follow the device's action
            da = dev_actions[:, stp]
            if not np.array_equal(a, da):
                flips += int(np.sum(a != da))
                a = da.astype(np.int32)
                lp, _ = twin.logprob_actions(cur, a)
        nxt, rew, done = stepper(a, gstep)
        twin.rollout_store(stp, cur, a, lp, rew, nd, v)
        cur, nd = nxt, done.astype(np.uint8)
    stepper.cur, stepper.nd = cur, nd
    twin.write(F.F_CUR_OBS, cur); twin.write(F.F_NEXT_DONE, nd)
    twin.compute_gae()
    frac = 1.0 - it / num_updates
    eta = frac * float(np.float32(cfg.lr))
    for ep in range(cfg.update_epochs):
        twin.shuffle(it * cfg.update_epochs + ep)
        twin.adv_stats()
        for mb in range(cfg.num_minibatches):
            twin.update_minibatch(mb, eta, apply_update=True, want_stats=False)
    return flips


class _DeviceStepper:
    """steps a second on-device handle's envs through crl_env_step"""
    def __init__(self, h, F):
        self.h = h; h.env_reset()
        self.cur = h.read(F.F_CUR_OBS).copy(); self.nd = np.zeros(self.cur.shape[1], np.uint8)

    def __call__(self, a, gstep):
        return self.h.env_step(a, gstep=gstep)


def test_three_acrobot_iterations_match_the_host_driven_twin(crl):   # noqa: F811
    """1024 envs x 128 steps, 2x256. Bar: test_gpu_wide.py::test_wide_full_iteration_matches_oracle's max |Δparams| < 1e-5. Actions at CDF knots (the
    rollout kernel's logits against crl_policy_act's) follow the device: at most a handful, counted and printed."""
    F = crl._lib
    nt, k, iters = 1024, 128, 3
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * iters)
    shape = dict(obs_dim=6, n_act=3, hidden=256, seed=SEED)
    dev = crl.Agent(cfg, env_kind=F.ENV_ACROBOT, init_seed=4, **shape)
    envs = crl.Agent(cfg, env_kind=F.ENV_ACROBOT, init_seed=4, **shape)      # only its envs are used
    twin = crl.Agent(cfg, env_kind=F.ENV_EXTERNAL, init_seed=4, **shape)
    assert np.array_equal(dev.get_params(), twin.get_params())
    stepper = _DeviceStepper(envs.handle, F)
    dev.handle.env_reset()
    flips = 0
    for it in range(iters):
        dev.handle.iterate(1, want_stats=False)
        flips += _host_iteration(crl, dev.handle, twin.handle, cfg, it, iters, stepper)
        assert np.array_equal(dev.handle.read(F.F_OBS), twin.handle.read(F.F_OBS)) and np.array_equal(dev.handle.read(F.F_REWARD), twin.handle.read(F.F_REWARD))
        assert np.array_equal(dev.handle.read(F.F_TERMINAL), twin.handle.read(F.F_TERMINAL))
        d = np.max(np.abs(dev.get_params() - twin.get_params()))
        print(f"iteration {it}: max |Δparams| {d:.3g}, knot flips so far {flips}")
        assert d < 1e-5, (it, d)
    assert flips <= 1e-4 * nt * k * iters
    for a in (dev, envs, twin):
        a.close()


# ------------------------------------------------------------------------------------------------------------- learning
UPDATES = 60                        # x 256 envs x 128 steps = 1,966,080 = total_timesteps; a run takes a few seconds on the device
FLOOR = -199.0                      # the lowest possible return: 199 steps of -1 and the time limit's 0 — where an untrained policy sits


class _HostStepper:
    """tests/envs_ref.py (Float32) steps the control's envs on the host; resets from numpy's own generator (the control is not the code under test)"""
    def __init__(self, nt, seed):
        self.rng = np.random.default_rng(seed); self.nt = nt
        self.s = R.acrobot_reset(self.rng.random((4, nt)).astype(np.float32)); self.t = np.zeros(nt, np.int64)
        self.cur = np.asfortranarray(R.acrobot_obs(self.s, np.float32)); self.nd = np.zeros(nt, np.uint8)
        self.ret = np.zeros(nt); self.finished = []

    def __call__(self, a, gstep):
        self.s, self.t, rew, done, _ = R.acrobot_step(self.s, self.t, a, np.float32)
        obs = R.acrobot_obs(self.s, np.float32)                          # stale_obs: the terminal observation is what the policy sees
        self.ret += rew
        for e in np.flatnonzero(done):
            self.finished.append(self.ret[e]); self.ret[e] = 0
        if done.any():
            fresh = R.acrobot_reset(self.rng.random((4, self.nt)).astype(np.float32))
            self.s = np.where(done[None, :], fresh, self.s); self.t = np.where(done, 0, self.t)
        return np.asfortranarray(obs), rew.astype(np.float32), done


def _control_curve(crl, hidden):   # noqa: F811
    F = crl._lib
    nt, k = 32, 128                 # fewer envs, the same number of updates
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * UPDATES)
    twin = crl.Agent(cfg, obs_dim=6, n_act=3, hidden=hidden, env_kind=F.ENV_EXTERNAL, seed=SEED, init_seed=11)
    stepper = _HostStepper(nt, 5)
    curve = []
    for it in range(UPDATES):
        stepper.finished = []
        _host_iteration(crl, None, twin.handle, cfg, it, UPDATES, stepper)
        curve.append(float(np.mean(stepper.finished)) if stepper.finished else None)
    twin.close()
    return curve


@pytest.mark.parametrize("hidden", [64, 256])
def test_ppo_learns_acrobot_on_the_device_env(crl, hidden, tmp_path):   # noqa: F811
    """ppo(env="acrobot"), three seeds, 256 envs x 128 steps, total_timesteps = 60 updates. Metric: the mean episode return of the last update that
    finished an episode. Control: the same configuration through CRL_ENV_EXTERNAL with tests/envs_ref.py stepping 32 envs on the host for the same 60
    updates. Requirement: every device run ends above the midpoint between -199 (the floor) and the control's final mean."""
    control = _control_curve(crl, hidden)
    c_final = [c for c in control if c is not None][-1]
    bar = 0.5 * (FLOOR + c_final)
    curves = {}
    for seed in (1, 2, 3):
        cfg = crl.PPOConfig(num_envs=256, num_steps=128, total_timesteps=256 * 128 * UPDATES)
        crl.ppo(cfg, env="acrobot", hidden=hidden, seed=seed, init_seed=seed, episode_records=0, run_name=f"acro-{hidden}-{seed}",
                logger_kw=dict(to_tensorboard=False, to_json=True, log_dir=str(tmp_path)))
        recs = [json.loads(line) for line in open(tmp_path / f"acro-{hidden}-{seed}.json")]
        curves[seed] = [r["episode_return"] for r in recs if r["msg"] == "Episode Statistics"]
        print(f"hidden {hidden} seed {seed}: first {curves[seed][0]:.1f} last {curves[seed][-1]:.1f}; control last {c_final:.1f}; bar {bar:.1f}")
    if WRITE:
        path = os.path.join(ROOT, "profiles", "env_acrobot_train.json")
        allrec = json.load(open(path)) if os.path.exists(path) else {}
        allrec[f"2x{hidden}"] = {"updates": UPDATES, "control_32_envs_host_stepped": control, "device_256_envs": {str(s): c for s, c in curves.items()},
                                 "floor": FLOOR, "bar": bar}
        json.dump(allrec, open(path, "w"), indent=1, sort_keys=True)
    assert c_final > FLOOR + 20, f"the control itself did not learn ({c_final})"
    for seed, c in curves.items():
        assert c[-1] > bar, (hidden, seed, c[-1], bar)
