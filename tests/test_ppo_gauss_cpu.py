"""CPU checks of the Gaussian PPO yardstick (tests/ppo_gauss_ref.py) and of crl_make_actor_critic_gaussian; no GPU.

The analytic minibatch gradient of the restatement against central finite differences in Float64, step h = 1e-5. The bound, as in tests/test_sac_cpu.py:
fd = (f(w + h) − f(w − h)) / 2h differs from f'(w) by the truncation h²·|f'''|/6 plus the rounding (e₊ + e₋)/2h of the two evaluations. The loss is a mean
over M = 24 samples of terms of size <= 10 built from ~1500 multiply-adds per sample (obs 5, hidden 16): every operation rounding in the worst direction
gives e <= 1500 · 1.1e-16 · 10 = 1.7e-12, so the rounding term is <= 1.7e-7. Each derivative of logπ with respect to a head input brings a factor of at
most 1/σ, and the case keeps log_std >= −2 (σ >= 0.135, 1/σ³ <= 400): with ratios below e, advantages of size 3 and weights of size 0.4, |f'''| <= 1e4,
a truncation <= 1.7e-7. TOL = 4e-7 is their sum rounded up. The step moves logπ by at most h · 16 · … < 1e-3, so the test asserts that no ratio lies
within 1e-3 of a clip edge and no pg1 − pg2 within 1e-3 of zero except where both branches coincide exactly (inside the clip): no kink is crossed."""
import numpy as np
import pytest

import ppo_gauss_ref as G

H_STEP, TOL = 1e-5, 4e-7
D, AD, HID, M = 5, 3, 16, 24
LO, HI = -2.0, 2.0
HP = dict(clip=0.2, ent_coeff=0.01, v_coef=0.5, clip_vloss=False)


def _case(seed, clip_vloss):
    rng = np.random.default_rng(seed)
    off = G.offsets(D, AD, HID)
    p = 0.4 * rng.standard_normal(off[-1])
    # s rows of the head bias: one saturated at each end (|s| > 4), one in the middle
    p[off[5] + AD:off[6]] = [6.0, -6.0, 0.3]
    obs = rng.standard_normal((D, M))
    actor, _ = G.unpack(p, D, AD, HID)
    z, _, _ = G.mlp(actor, obs)
    a, lp = G.act(z, rng.standard_normal((AD, M)), AD, LO, HI)
    # old logprobs offset so that the ratio falls on both sides of the clip and inside it
    old_lp = lp - np.tile([0.0, 0.5, -0.5, 0.1], M // 4)
    adv = 3.0 * rng.standard_normal(M); ret = rng.standard_normal(M); old_v = rng.standard_normal(M)
    return p, obs, a, old_lp, old_v, adv, ret, dict(HP, clip_vloss=clip_vloss)


@pytest.mark.parametrize("clip_vloss", [False, True])
def test_analytic_gradient_matches_finite_differences(clip_vloss):
    p, obs, a, old_lp, old_v, adv, ret, hp = _case(3, clip_vloss)
    f = lambda w: G.minibatch_loss(w, D, AD, HID, LO, HI, obs, a, old_lp, old_v, adv, ret, hp, want_grad=False)[0]["loss"]
    terms, g, dg = G.minibatch_loss(p, D, AD, HID, LO, HI, obs, a, old_lp, old_v, adv, ret, hp)
    r = dg["ratio"]
    assert (r > 1.2 + 1e-3).any() and (r < 0.8 - 1e-3).any() and ((r > 0.8 + 1e-3) & (r < 1.2 - 1e-3)).any(), "cases on each side of the clip"
    assert np.all(np.minimum(np.abs(r - 0.8), np.abs(r - 1.2)) > 1e-3)
    assert (dg["Ahat"] > 0).any() and (dg["Ahat"] < 0).any()
    assert (dg["s"] > 4).any() and (dg["s"] < -4).any(), "tanh(s) saturated at each end"
    rng = np.random.default_rng(0)
    off = G.offsets(D, AD, HID)
    idx = np.concatenate([rng.integers(off[i], off[i + 1], 6) for i in range(12)] + [np.arange(off[5], off[6])])
    for i in idx:
        e = np.zeros_like(p); e[i] = H_STEP
        fd = (f(p + e) - f(p - e)) / (2 * H_STEP)
        assert abs(fd - g[i]) <= TOL, (i, fd, g[i])
    assert np.abs(g[off[5]:off[6]]).max() > 1e-4 and np.abs(g[off[0]:off[1]]).max() > 1e-4


@pytest.mark.parametrize("init,lo,hi", [(0.0, -5.0, 2.0), (-1.5, -3.0, 0.5), (1.9, -5.0, 2.0)])
def test_make_actor_critic_gaussian_gives_the_initial_log_std(init, lo, hi):
    import cleanrl_jl_amd as crl
    L = crl._lib
    D_, ad, Hd = 3, 2, 64
    p = L.make_actor_critic_gaussian_host(D_, ad, Hd, crl.GaussianOptions(lo, hi, init), seed=7)
    base = L.make_actor_critic_host(D_, 2 * ad, Hd, seed=7)
    off = G.offsets(D_, ad, Hd)
    s0 = p[off[5] + ad:off[6]].astype(np.float64)
    assert np.allclose(G.log_std(s0, lo, hi), init, atol=2e-6 * (hi - lo))     # float32 rounding of s0 through the slope 0.5 (hi − lo)(1 − tanh²) <= 0.5 (hi − lo)
    other = np.ones(p.size, bool); other[off[5] + ad:off[6]] = False
    assert np.array_equal(p[other], base[other]) and np.all(p[off[5]:off[5] + ad] == 0)
    for bad in (crl.GaussianOptions(2.0, 2.0, 0.0), crl.GaussianOptions(-5.0, 2.0, 2.0), crl.GaussianOptions(-5.0, 2.0, -5.0)):
        with pytest.raises(crl.CrlError, match="log_std"):
            L.make_actor_critic_gaussian_host(D_, ad, Hd, bad)


def test_ppo_continuous_rejects_unknown_envs_before_a_device_is_touched():
    import cleanrl_jl_amd as crl
    with pytest.raises(ValueError, match="continuous env"):
        crl.ppo_continuous(crl.PPOConfig(), env="cartpole")
    with pytest.raises(ValueError, match="follows from the env"):
        crl.ppo_continuous(crl.PPOConfig(), env="pendulum", n_act=2)
    with pytest.raises(TypeError, match="host env"):
        crl.ppo_continuous(crl.PPOConfig(), env=object())
