"""Gaussian PPO handles (crl_ppo_create_gaussian) on the GPU against the Float64 restatement tests/ppo_gauss_ref.py.

Bars. Gradients (relative L2 per array, _grad_close), losses (loss_close) and log-probabilities (rel_err_s) take the bars tests/test_gpu_wide.py applies
to the discrete path: RTOL = 1e-5 with its floors. The recovered xi and the Pendulum trajectory have no discrete counterpart: their bars come from
profiles/ppo_gauss_bar.json (scripts/ppo_gauss_bar.py: the restatement in Float32 against itself in Float64 on these inputs, times 8; the device's own
expf / tanhf / sincos error is unmeasured)."""
import itertools
import json
import os

import numpy as np
import pytest

import ppo_gauss_ref as G
from test_gpu_parity import RTOL, _grad_close, crl, loss_close, rel_err  # noqa: F401  (crl is the module fixture)
from test_gpu_wide import rel_err_s

pytestmark = pytest.mark.gpu

LO, HI = G.LO, G.HI     # sigma = 1 at s = 0: see tests/ppo_gauss_ref.py for why not the defaults
BAR = json.load(open(os.path.join(os.path.dirname(__file__), "..", "profiles", "ppo_gauss_bar.json")))
GRID = list(itertools.product([1, 3, 8], [3, 17, 64], [64, 256]))     # act_dim (head 2, 6 -> 8, 16 = AMAX) x obs_dim x hidden


def make(crl, nt, k, D, ad, Hd, params=None, env_kind=None, lo=LO, hi=HI, **kw):
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 10, **{a: b for a, b in kw.items() if a in ("num_minibatches", "clip_value_loss")})
    shape = {a: b for a, b in kw.items() if a in ("seed", "options", "stale_obs")}
    return crl.Agent(cfg, params=params, action="gaussian", gaussian=crl.GaussianOptions(lo, hi, 0.0), obs_dim=D, n_act=ad, hidden=Hd,
                     env_kind=crl._lib.ENV_SYNTHETIC if env_kind is None else env_kind, **shape)


def spread_params(crl, D, ad, Hd, seed, lo=LO, hi=HI):
    return G.spread_params(crl._lib, D, ad, Hd, seed, lo, hi)


@pytest.mark.parametrize("ad,D,Hd", GRID)
@pytest.mark.parametrize("n", [1, 257])
def test_probes_match_restatement(crl, ad, D, Hd, n):
    rng = np.random.default_rng(n + D + ad)
    p = spread_params(crl, D, ad, Hd, 3)
    agent = make(crl, 8, 16, D, ad, Hd, params=p)
    obs = np.asfortranarray(rng.standard_normal((D, n)).astype(np.float32))
    xi = rng.standard_normal((ad, n)).astype(np.float32)
    actor, critic = G.unpack(p, D, ad, Hd)
    z = G.mlp(actor, obs.astype(np.float64))[0]; v = G.mlp(critic, obs.astype(np.float64))[0][0]
    a_o, lp_o = G.act(z, xi.astype(np.float64), ad, LO, HI)
    a_g, lp_g, v_g = agent.handle.policy_act_gaussian(obs, xi)
    assert rel_err_s(a_g, a_o) < RTOL and rel_err_s(lp_g, lp_o) < RTOL and rel_err(v_g, v) < RTOL
    acts = (a_o + 0.5 * rng.standard_normal((ad, n))).astype(np.float32)
    lp_o2, H_o, _, _ = G.logprob_entropy(z, acts.astype(np.float64), ad, LO, HI)
    lp_g2, H_g = agent.handle.logprob_actions_gaussian(obs, acts)
    assert H_g.shape == (n,) and rel_err_s(lp_g2, lp_o2) < RTOL and rel_err_s(H_g, H_o) < RTOL
    agent.close()


# the grid at sigma = 1 under both value losses, plus the library's default bounds (-5, 2) at the grid's corners
UPDATES = [(*g, M, cv, LO, HI) for g in GRID for M in (96, 320) for cv in (False, True)] + [(1, 3, 64, 96, True, -5.0, 2.0), (8, 64, 256, 320, True, -5.0, 2.0)]


@pytest.mark.parametrize("ad,D,Hd,M,clipv,lo,hi", UPDATES)
def test_update_gradient_and_stats_match_restatement(crl, ad, D, Hd, M, clipv, lo, hi):
    """crl_ppo_update_minibatch(apply_update = 0) on written buffers: M = 96 is a tile tail, 320 a tail of the loss kernel's 256-position block.
    Bars: RTOL on everything at bounds (-2, 2). logpi and its cotangents see mu through (a - mu) / sigma, so a Float32 rounding of the forward's mu
    reaches them divided by sigma: in the default-bounds cases the actor's six arrays, pg_loss and loss take RTOL / (the minibatch's smallest sigma),
    computed on the restatement; the critic's arrays, v_loss and the entropy keep RTOL."""
    nt, k, nmb = M // 8, 16, 2
    rng = np.random.default_rng(M + D + ad)
    p = spread_params(crl, D, ad, Hd, 5, lo, hi)
    agent = make(crl, nt, k, D, ad, Hd, params=p, lo=lo, hi=hi, num_minibatches=nmb, clip_value_loss=clipv)
    h, F = agent.handle, crl._lib
    B = nt * k
    obs = rng.standard_normal((D, B)).astype(np.float32)
    actor, critic = G.unpack(p, D, ad, Hd)
    z = G.mlp(actor, obs.astype(np.float64))[0]
    act, lp = G.act(z, rng.standard_normal((ad, B)), ad, lo, hi)
    act = act.astype(np.float32)
    lp = G.logprob_entropy(z, act.astype(np.float64), ad, lo, hi)[0]
    old_lp = (lp - np.tile([0.0, 0.5, -0.5, 0.1], B // 4)).astype(np.float32)      # ratios inside the clip, above it and below it
    # old values on both sides of the value clip around the current critic; returns near them
    old_v = (G.mlp(critic, obs.astype(np.float64))[0][0] + np.tile([0.05, 0.5, -0.5, -0.1], B // 4)).astype(np.float32)
    adv = (2 * rng.standard_normal(B)).astype(np.float32); ret = (3 * rng.standard_normal(B)).astype(np.float32)
    perm = rng.permutation(B).astype(np.int32)
    for f, arr in ((F.F_OBS, obs), (F.FIELD_ACTION_F, act), (F.F_LOGPROB, old_lp), (F.F_VALUE, old_v), (F.F_ADVANTAGE, adv), (F.F_RETURN, ret), (F.F_PERM, perm)):
        h.write(f, arr)
    h.adv_stats()
    hp = dict(clip=0.2, ent_coeff=0.01, v_coef=0.5, clip_vloss=clipv)
    saturated, off = False, G.offsets(D, ad, Hd)
    for mb in range(nmb):
        idx = perm[mb * M:(mb + 1) * M]
        t_o, g_o, dg = G.minibatch_loss(p, D, ad, Hd, lo, hi, obs[:, idx], act[:, idx], old_lp[idx], old_v[idx], adv[idx], ret[idx], hp)
        r = dg["ratio"]
        assert (r > 1.2).any() and (r < 0.8).any() and ((r > 0.8) & (r < 1.2)).any() and (dg["Ahat"] > 0).any() and (dg["Ahat"] < 0).any()
        saturated |= bool((np.abs(dg["s"]) > 4).any())
        amp = max(1.0, float(np.exp(-G.log_std(dg["s"], lo, hi).min()))) if lo < LO else 1.0
        gs = h.update_minibatch(mb, 2.5e-4, apply_update=False)
        for key in ("loss", "pg_loss", "v_loss", "entropy_loss"):
            assert loss_close(key, gs[key], t_o[key], RTOL * (amp if key in ("loss", "pg_loss") else 1.0)), (key, gs[key], t_o[key])
        g_g = h.read(F.F_GRADS)
        _grad_close(np.concatenate([g_g[:off[6]], g_o[off[6]:]]), g_o, off, RTOL * amp)      # the actor's arrays
        _grad_close(np.concatenate([g_o[:off[6]], g_g[off[6]:]]), g_o, off, RTOL)            # the critic's
    assert saturated, "at least one s beyond ±4"
    agent.close()


@pytest.mark.parametrize("nt", [64, 96])
@pytest.mark.parametrize("ad,D,Hd,kind", G.ROLLOUT_CASES)
def test_rollout_logprob_and_noise_stream(crl, nt, ad, D, Hd, kind):
    """The one route a Gaussian handle takes, the per-step one: wide_rollout_route picks it whatever wide_rollout_persist says, so there is no second
    route to compare with."""
    F, k, seed = crl._lib, 5, 0x5EED
    p = spread_params(crl, D, ad, Hd, 7)
    agent = make(crl, nt, k, D, ad, Hd, params=p, env_kind=F.ENV_PENDULUM if kind == "pendulum" else None, seed=seed)
    h = agent.handle
    h.env_reset(); h.rollout_run()
    obs, act, lp, val = [h.read(f) for f in (F.F_OBS, F.FIELD_ACTION_F, F.F_LOGPROB, F.F_VALUE)]
    agent.close()
    assert act.shape == (ad, nt, k)
    actor, critic = G.unpack(p, D, ad, Hd)
    X = obs.reshape(D, -1, order="F").astype(np.float64)
    z = G.mlp(actor, X)[0]
    lp_o, _, xi_rec, _ = G.logprob_entropy(z, act.reshape(ad, -1, order="F").astype(np.float64), ad, LO, HI)
    assert rel_err_s(lp.reshape(-1, order="F"), lp_o) < RTOL and rel_err(val.reshape(-1, order="F"), G.mlp(critic, X)[0][0]) < RTOL
    xi_pin = np.concatenate([G.rollout_xi(seed, np.arange(nt), g, ad) for g in range(k)], axis=1)
    err = np.max(np.abs(xi_rec - xi_pin))
    print(f"recovered xi: max |err| = {err:.3e}, bar {BAR['xi_bar']:.3e} (profiles/ppo_gauss_bar.json)")
    assert err < BAR["xi_bar"]


def test_pendulum_matches_restatement(crl):
    """crl_env_step_gaussian for three episodes: torques beyond ±2, thetadot driven to ±8, theta crossing ±pi (asserted on the restatement)."""
    F = crl._lib
    ref = G.pendulum_trajectory()
    assert (np.abs(G.pendulum_actions()) > 2).any() and (np.abs(ref["thd"]) == 8).any() and (np.abs(np.diff(ref["th"], axis=0)) > 6).any()
    agent = make(crl, G.PEND_ENVS, 4, 3, 1, 64, env_kind=F.ENV_PENDULUM, seed=G.PEND_SEED, stale_obs=False)
    h = agent.handle
    h.env_reset()
    obs, rew, done = zip(*[h.env_step_gaussian(a, g) for g, a in enumerate(G.pendulum_actions())])
    e_obs, e_rew = np.max(np.abs(np.array(obs) - ref["obs"])), np.max(np.abs(np.array(rew) - ref["reward"]))
    print(f"pendulum: obs err {e_obs:.3e} (bar {BAR['pendulum_obs_bar']:.3e}), reward err {e_rew:.3e} (bar {BAR['pendulum_reward_bar']:.3e})")
    assert np.array_equal(np.array(done).astype(bool), ref["done"]) and ref["done"].sum() == 3 * G.PEND_ENVS
    assert e_obs < BAR["pendulum_obs_bar"] and e_rew < BAR["pendulum_reward_bar"]
    agent.close()


def test_discrete_handles_unchanged_and_errors_name_the_reason(crl):
    F = crl._lib

    def discrete_run():
        cfg = crl.PPOConfig(num_envs=64, num_steps=8, total_timesteps=64 * 8 * 10)
        a = crl.Agent(cfg, obs_dim=8, n_act=4, hidden=256, env_kind=F.ENV_SYNTHETIC)
        a.handle.env_reset(); st = a.handle.iterate(1)
        out = (a.handle.read(F.F_ACTION), a.get_params(), st[-1]["loss"])
        a.close()
        return out
    alone = discrete_run()
    g = make(crl, 64, 8, 8, 3, 256)
    g.handle.env_reset(); g.handle.iterate(1)
    beside = discrete_run()
    assert np.array_equal(alone[0], beside[0]) and np.array_equal(alone[1], beside[1]) and alone[2] == beside[2]
    h = g.handle
    for call in (lambda: h.evaluate(4), lambda: h.diagnose(), lambda: h.act_device(0, 1, 1, 1), lambda: h.record_device(0, 1, 1, 1),
                 lambda: h.env_step_device(1, 0, None, 1, 1)):
        with pytest.raises(crl.CrlError, match="not built for Gaussian handles"):
            call()
    with pytest.raises(crl.CrlError, match="CRL_F_ACTION_F"):
        h.read(F.F_ACTION)
    g.close()
    d = crl.Agent(crl.PPOConfig(num_envs=8, num_steps=8), obs_dim=8, n_act=4, hidden=64, env_kind=F.ENV_SYNTHETIC)
    with pytest.raises(crl.CrlError, match="Gaussian handle"):
        d.handle.read(F.FIELD_ACTION_F)
    d.close()


def test_ppo_continuous_trains_on_the_pendulum(crl):
    """the public entry end to end: two updates on the on-device Pendulum move every parameter array and leave finite numbers"""
    cfg = crl.PPOConfig(num_envs=64, num_steps=8, total_timesteps=64 * 8 * 2)
    p0 = crl._lib.make_actor_critic_gaussian_host(3, 1, 64, crl.GaussianOptions(), seed=0)
    p1 = crl.ppo_continuous(cfg, env="pendulum", hidden=64, episode_records=0)
    off = G.offsets(3, 1, 64)
    assert np.all(np.isfinite(p1)) and all(np.any(p1[off[i]:off[i + 1]] != p0[off[i]:off[i + 1]]) for i in range(12))


class HostEnv:
    """A tiny numpy env with float actions: the act_dim protocol of ppo_continuous / train_host_gaussian."""
    num_envs, obs_dim, act_dim = 16, 5, 2

    def __init__(self):
        self.rng, self.t = np.random.default_rng(3), 0

    def reset(self):
        return self.rng.standard_normal((5, 16)).astype(np.float32), np.zeros(16, np.uint8)

    def step(self, action):
        self.t += 1
        return -np.abs(action).sum(0).astype(np.float32), self.rng.standard_normal((5, 16)).astype(np.float32), np.full(16, self.t % 7 == 0, np.uint8)


def test_host_env_update_equals_iterate_on_the_same_buffer(crl):
    """crl_rollout_store_gaussian + crl_ppo_update (ppo(env=obj) -> ppo_continuous -> train_host_gaussian) against a second handle whose buffer is
    written field by field with what the first one stored: the same GAE, shuffle and 16 optimiser steps, so the same parameters bit for bit."""
    F = crl._lib
    cfg = crl.PPOConfig(num_envs=16, num_steps=8, total_timesteps=16 * 8)
    p1 = crl.ppo(cfg, env=HostEnv(), hidden=64)
    a = crl.Agent(cfg, action="gaussian", env_kind=F.ENV_EXTERNAL, obs_dim=5, n_act=2, hidden=64)
    env, rng, h = HostEnv(), np.random.default_rng(0), a.handle
    obs, done = env.reset()
    stored = []
    for step in range(8):
        act, lp, val = h.policy_act_gaussian(obs, rng.standard_normal((2, 16)).astype(np.float32))
        rew, nobs, ndone = env.step(act)
        stored.append((obs, act, lp, rew, done, val)); obs, done = nobs, ndone
    for f, i, dt in ((F.F_OBS, 0, np.float32), (F.FIELD_ACTION_F, 1, np.float32), (F.F_LOGPROB, 2, np.float32), (F.F_REWARD, 3, np.float32),
                     (F.F_TERMINAL, 4, np.uint8), (F.F_VALUE, 5, np.float32)):
        h.write(f, np.stack([np.asarray(s[i], dt) for s in stored], axis=-1))
    h.write(F.F_CUR_OBS, obs); h.write(F.F_NEXT_DONE, done)
    h.update(want_stats=False)
    assert np.array_equal(a.get_params(), p1) and np.any(p1 != F.make_actor_critic_gaussian_host(5, 2, 64, crl.GaussianOptions(), seed=0))
    a.close()
