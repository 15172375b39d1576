"""The staged host calls of every handle family across a regrow of their device scratch (csrc/stage.hpp). For one handle per family the same call is
made three times: small, large enough that the scratch must be freed and allocated again, then the small one again on the first call's inputs.

* the first and the third result are bit-identical: a regrow in between leaves nothing of the larger call behind;
* the large call agrees with the float64 reference the entry point's own test uses, under that test's bar (named at each case; no bar is set here);
* n = 0 returns without touching its outputs;
* a call with an optional output left out returns its other outputs bit for bit as the call with all of them.

A crl_ppo handle's stage starts at 1 MiB, so its large call is n = 70,000 at obs_dim 4 (2.5 MB); every other scratch starts empty: n = 1, then 257."""
import ctypes as C

import numpy as np
import pytest

import ddpg_ref as DR
import noisy_ref as NZ
import oraclelib as O
import ppo_gauss_ref as PG
import qr_ref as Q
import value_eval_gpu as VG
import value_eval_ref as V
from test_gpu_ddpg import _cfg as ddpg_cfg, _params as ddpg_params
from test_gpu_parity import RTOL, crl, rel_err  # noqa: F401  (crl is the module fixture)
from test_gpu_ppo_gauss import HI, LO, make as make_gauss, spread_params as gauss_params
from test_gpu_qr import _cfg as qr_cfg, _handle as qr_handle, _params as qr_params
from test_gpu_wide import make_wide, ocfg, rel_err_s, spread_params

pytestmark = pytest.mark.gpu
PPO_SMALL, PPO_LARGE = 3, 70_000
SMALL, LARGE = 1, 257
SENTINEL = 123456789


def three_calls(call, small, large):
    """call(*inputs) → tuple of arrays. → the large call's result, after checking that the small call gives the same bits before and after it"""
    first = call(*small)
    big = call(*large)
    third = call(*small)
    assert all(np.array_equal(a, b) for a, b in zip(first, third)), "the small call's bits moved across a regrow"
    return big


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------- PPO, softmax head, layer-wise path
def test_ppo_softmax_calls_across_a_regrow(crl):
    """bars of tests/test_gpu_wide.py::test_wide_policy_act_and_logprob_match_oracle, reference oraclelib"""
    D, A, Hd = 4, 3, 64
    cfg = ocfg(8, 16, D, A, Hd)
    params = spread_params(cfg, 3)
    agent = make_wide(crl, 8, 16, D, A, Hd, params=params)
    h = agent.handle

    def inputs(n, seed):
        rng = np.random.default_rng(seed)
        return np.asfortranarray(rng.standard_normal((D, n)).astype(np.float32)), rng.random(n), rng.integers(0, A, n).astype(np.int32)
    (obs_s, u_s, act_s), (obs, u, acts) = inputs(PPO_SMALL, 1), inputs(PPO_LARGE, 2)
    a_g, lp_g, v_g = three_calls(h.policy_act, (obs_s, u_s), (obs, u))
    a_o, lp_o, v_o, margin = O.get_action(cfg, params, obs, u)
    safe = margin > 1e-6
    same = a_g == a_o
    print(f"policy_act n={PPO_LARGE}: safe {safe.mean():.4f}, logprob {rel_err_s(lp_g[same], lp_o[same]):.3e}, value {rel_err(v_g, v_o):.3e}")
    assert np.array_equal(a_g[safe], a_o[safe]), "action indices must be bit-exact away from CDF knots"
    assert safe.mean() > 0.98 and len(set(a_o.tolist())) == A
    assert rel_err_s(lp_g[same], lp_o[same]) < RTOL and rel_err(v_g, v_o) < RTOL
    lp_g2, ent_g = three_calls(h.logprob_actions, (obs_s, act_s), (obs, acts))
    lp_o2, ent_o = O.logprob_actions(cfg, params, obs, acts)
    print(f"logprob_actions n={PPO_LARGE}: logprob {rel_err_s(lp_g2, lp_o2):.3e}, entropy {rel_err(ent_g, ent_o):.3e}")
    assert ent_g.shape == (A, PPO_LARGE) and rel_err_s(lp_g2, lp_o2) < RTOL and rel_err(ent_g, ent_o) < RTOL
    # value left out: the same actions and log-probabilities
    a_n, lp_n, _ = h.policy_act(obs_s, u_s, with_value=False)
    a_w, lp_w, _ = h.policy_act(obs_s, u_s)
    assert same_bits(a_n, a_w) and same_bits(lp_n, lp_w)
    # n = 0: nothing is written
    L = crl._lib
    lib = L.load()
    ai = np.full(4, SENTINEL, np.int32); f1 = np.full(4, SENTINEL, np.float32); f2 = np.full(4 * A, SENTINEL, np.float32)
    assert lib.crl_policy_act(h._h, L._ptr(obs_s, C.c_float), L._ptr(u_s, C.c_double), 0, L._ptr(ai, C.c_int32), L._ptr(f1, C.c_float), L._ptr(f2, C.c_float)) == 0
    assert lib.crl_logprob_actions(h._h, L._ptr(obs_s, C.c_float), L._ptr(act_s, C.c_int32), 0, L._ptr(f1, C.c_float), L._ptr(f2, C.c_float)) == 0
    assert (ai == SENTINEL).all() and (f1 == np.float32(SENTINEL)).all() and (f2 == np.float32(SENTINEL)).all()
    agent.close()


# ---------------------------------------------------------------------------------------------------- PPO, Gaussian head
def test_ppo_gaussian_calls_across_a_regrow(crl):
    """bars of tests/test_gpu_ppo_gauss.py::test_probes_match_restatement, reference tests/ppo_gauss_ref.py"""
    D, ad, Hd = 4, 3, 64
    p = gauss_params(crl, D, ad, Hd, 3)
    agent = make_gauss(crl, 8, 16, D, ad, Hd, params=p)
    h = agent.handle
    actor, critic = PG.unpack(p, D, ad, Hd)

    def inputs(n, seed):
        rng = np.random.default_rng(seed)
        return np.asfortranarray(rng.standard_normal((D, n)).astype(np.float32)), rng.standard_normal((ad, n)).astype(np.float32)
    (obs_s, xi_s), (obs, xi) = inputs(PPO_SMALL, 1), inputs(PPO_LARGE, 2)
    a_g, lp_g, v_g = three_calls(h.policy_act_gaussian, (obs_s, xi_s), (obs, xi))
    z = PG.mlp(actor, obs.astype(np.float64))[0]; v = PG.mlp(critic, obs.astype(np.float64))[0][0]
    a_o, lp_o = PG.act(z, xi.astype(np.float64), ad, LO, HI)
    print(f"policy_act_gaussian n={PPO_LARGE}: action {rel_err_s(a_g, a_o):.3e}, logprob {rel_err_s(lp_g, lp_o):.3e}, value {rel_err(v_g, v):.3e}")
    assert rel_err_s(a_g, a_o) < RTOL and rel_err_s(lp_g, lp_o) < RTOL and rel_err(v_g, v) < RTOL
    rng = np.random.default_rng(5)
    acts = (a_o + 0.5 * rng.standard_normal((ad, PPO_LARGE))).astype(np.float32)
    acts_s = rng.standard_normal((ad, PPO_SMALL)).astype(np.float32)
    lp_g2, H_g = three_calls(h.logprob_actions_gaussian, (obs_s, acts_s), (obs, acts))
    lp_o2, H_o, _, _ = PG.logprob_entropy(z, acts.astype(np.float64), ad, LO, HI)
    print(f"logprob_actions_gaussian n={PPO_LARGE}: logprob {rel_err_s(lp_g2, lp_o2):.3e}, entropy {rel_err_s(H_g, H_o):.3e}")
    assert H_g.shape == (PPO_LARGE,) and rel_err_s(lp_g2, lp_o2) < RTOL and rel_err_s(H_g, H_o) < RTOL
    L = crl._lib
    lib = L.load()
    f0 = np.full(4 * ad, SENTINEL, np.float32); f1 = np.full(4, SENTINEL, np.float32); f2 = np.full(4, SENTINEL, np.float32)
    assert lib.crl_policy_act_gaussian(h._h, L._ptr(obs_s, C.c_float), L._ptr(xi_s, C.c_float), 0, L._ptr(f0, C.c_float), L._ptr(f1, C.c_float), L._ptr(f2, C.c_float)) == 0
    assert lib.crl_logprob_actions_gaussian(h._h, L._ptr(obs_s, C.c_float), L._ptr(acts_s, C.c_float), 0, L._ptr(f1, C.c_float), L._ptr(f2, C.c_float)) == 0
    assert all((f == np.float32(SENTINEL)).all() for f in (f0, f1, f2))
    agent.close()


# ---------------------------------------------------------------------------------------------------- DQN, dueling + QR
def test_dqn_dueling_qr_calls_across_a_regrow(crl):
    """bit for bit against tests/qr_ref.py on the device's parameters, as tests/test_gpu_qr.py and tests/test_gpu_duel.py hold this head (nothing in it
    is transcendental)"""
    N = 8
    cfg, lay = qr_cfg({}), NZ.layers(True, N)
    params = qr_params(lay, False)
    h = qr_handle(crl, cfg, N, dueling=True, params=params)
    ref = Q.make(cfg, None, None, dict(n_quantiles=N, kappa=1.0), True, params)
    xs, X = np.random.default_rng(1).uniform(-2.4, 2.4, (4, SMALL)), np.random.default_rng(2).uniform(-2.4, 2.4, (4, LARGE))
    (q,) = three_calls(lambda x: (h.q_values(x),), (xs,), (X,))
    (th,) = three_calls(lambda x: (h.qr_quantiles(x),), (xs,), (X,))
    val, adv = three_calls(lambda x: tuple(h.dueling_streams(x)[k] for k in ("value", "adv")), (xs,), (X,))
    rs = ref.streams(X)
    assert q.shape == (2, LARGE) and th.shape == (N, 2, LARGE) and val.shape == (N, LARGE) and adv.shape == (N, 2, LARGE)
    assert np.array_equal(q, ref.q_values(X)) and np.array_equal(th, ref.quantiles(X))
    assert np.array_equal(val, rs["value"]) and np.array_equal(adv, rs["adv"])
    # one stream left out: the other one's bits are those of the call with both
    L = crl._lib
    lib = h._L
    xp = np.asfortranarray(X)
    only_v = np.zeros((N, LARGE), np.float64, order="F"); only_a = np.zeros((N, 2, LARGE), np.float64, order="F")
    assert lib.crl_dqn_dueling_streams(h._h, L._ptr(xp, C.c_double), LARGE, L._ptr(only_v, C.c_double), None) == 0
    assert lib.crl_dqn_dueling_streams(h._h, L._ptr(xp, C.c_double), LARGE, None, L._ptr(only_a, C.c_double)) == 0
    assert same_bits(only_v, val) and same_bits(only_a, adv)
    # n = 0
    d0 = np.full(4 * N, float(SENTINEL)); d1 = np.full(4 * N, float(SENTINEL))
    assert lib.crl_dqn_q_values(h._h, L._ptr(xp, C.c_double), 0, L._ptr(d0, C.c_double)) == 0
    assert lib.crl_dqn_qr_quantiles(h._h, L._ptr(xp, C.c_double), 0, L._ptr(d0, C.c_double)) == 0
    assert lib.crl_dqn_dueling_streams(h._h, L._ptr(xp, C.c_double), 0, L._ptr(d0, C.c_double), L._ptr(d1, C.c_double)) == 0
    assert (d0 == SENTINEL).all() and (d1 == SENTINEL).all()
    h.close()


# ---------------------------------------------------------------------------------------------------- DDPG
def test_ddpg_calls_across_a_regrow(crl):
    """bar of tests/test_gpu_ddpg.py::test_forwards_match_the_reference (1e-10 absolute), reference tests/ddpg_ref.py"""
    D, A = 17, 6
    _, c = ddpg_cfg(crl, D, A, True)
    h = crl._lib.DDPGHandle(c, 0)
    actor, critic = ddpg_params(crl, D, A, 3)
    h.write_params(actor, critic)

    def inputs(n, seed):
        rng = np.random.default_rng(seed)
        return rng.standard_normal((D, n)), rng.uniform(-2, 2, (A, n))
    (obs_s, act_s), (obs, act) = inputs(SMALL, 1), inputs(LARGE, 2)
    (out,) = three_calls(lambda o: (h.actor(o),), (obs_s,), (obs,))
    (q,) = three_calls(lambda o, a: (h.q_values(o, a),), (obs_s, act_s), (obs, act))
    d_actor = np.abs(out - DR.actor_forward(actor, D, A, obs)[2] * 2.0).max()
    d_q = np.abs(q - DR.q_values(critic, D, A, obs, act)).max()
    print(f"ddpg n={LARGE}: actor {d_actor:.3e}, q {d_q:.3e}")
    assert d_actor <= 1e-10 and d_q <= 1e-10
    L = crl._lib
    d0 = np.full(4 * A, float(SENTINEL))
    op, ap = np.asfortranarray(obs), np.asfortranarray(act)
    assert h._L.crl_ddpg_actor(h._h, L._ptr(op, C.c_double), 0, L._ptr(d0, C.c_double)) == 0
    assert h._L.crl_ddpg_q_values(h._h, L._ptr(op, C.c_double), L._ptr(ap, C.c_double), 0, L._ptr(d0, C.c_double)) == 0
    assert (d0 == SENTINEL).all()
    h.close()


# ---------------------------------------------------------------------------------------------------- A2C
def test_a2c_forward_across_a_regrow(crl):
    """bar of tests/test_gpu_a2c_eval.py::test_forward_matches_oracle (value_eval_gpu.forward_bar: 1e-9 relative), reference tests/value_eval_ref.py"""
    params = V.a2c_perturbed(4)
    h = VG.handle(crl, V.A2C, params)
    xs, X = np.random.default_rng(1).standard_normal((SMALL, 4)), np.random.default_rng(2).standard_normal((LARGE, 4))
    for net in (0, 1):
        three_calls(lambda o: (h.forward(net, o.T),), (xs,), (X,))
    VG.forward_bar(h, params, X)      # both nets at n = 257 against the oracle's forward
    L = crl._lib
    d0 = np.full(8, float(SENTINEL))
    xp = np.asfortranarray(X.T)
    for net in (0, 1):
        assert h._L.crl_a2c_forward(h._h, net, L._ptr(xp, C.c_double), 0, L._ptr(d0, C.c_double)) == 0
    assert (d0 == SENTINEL).all()
    h.close()
