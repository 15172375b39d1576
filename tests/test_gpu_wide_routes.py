"""Parity of every route of the layer-wise ("wide") path against the CPU oracle, not only the default one. The shapes the library takes
(obs 1..64, act 2..16, hidden 64 / 128 / 256) are split between kernels by a handful of predicates in wide.hip — those of the rollout
and of the update pass each written once, in wide_rollout_route and wide_update_route; each case below is sized to reach one of them.
(The predicates are in wide.hip; the wide_wgrad_* kernels they select live in wide_wgrad.hpp, the tile-resident ones in wide_fused.hpp / wide_rs.hpp.)
Same bars as test_gpu_wide.py / test_gpu_parity.py: actions, permutations, env fields bit-equal; float32 results within RTOL = 1e-5
(rel_err / rel_err_s), losses by loss_close, gradients by _grad_close; whole iterations as test_wide_full_iteration_matches_oracle.

| case                                   | kernels it reaches                                                  | predicate (wide.hip)                                        |
|----------------------------------------|---------------------------------------------------------------------|-------------------------------------------------------------|
| wide_gemm = 1, hidden 256               | wide_pack_x3_kernel, wide_dense_x3_kernel<EPI_TANH, 1, 8> with the  | wide_x3 && !wide_x2 (ensure_pack, wide_forward); M <= 32768 |
|                                        | fused head (tile_tanh_head, ldz = A8), wide_wgrad_x3_kernel,        | (dense_x3_launch); wide_backward: H == 256 && wide_x3       |
|                                        | wide_dense_x3_kernel<EPI_DTANH, 1, 8>                               |                                                             |
| wide_gemm = 0, hidden 256               | wide_dense_kernel<4, 2, 1, 1> for both 256x256 layers, wide_wgrad_  | !wide_x3: dense_launch(256), H >= 128 wgrad                 |
|                                        | kernel<2>                                                           |                                                             |
| wide_tanh_rational = 1                  | no fused kernel; tanh_fast in every layer (rollout kernels too)     | wide_fused_ok false (both routes); fast_act = 0 (wide_forward)|
| 2x256, 9..16 actions (12/16, 33/9,     | update: wide_fused_fwd_kernel<dp, true> (h1 stored), layer-wise     | wide_update_route: wide_fused_ok (A <= AMAX = 16) but A >    |
|  64/16)                                 | wide_backward with its own K = 16 δ2 launch and wide_wgrad_x2_kernel| PC_AMAX = FB_AMAX = 8 (FWD_FUSED, BWD_LAYERS); d2_sweep = NO |
|                                        | over the stored h1; rollout: wide_rollout_persist_kernel (D <= 16)  | <= 8 false; wide_rollout_route: A > PC_AMAX, D <= 16: PERSIST|
| obs 17..64 at hidden 256 / 128          | generic layer 1 with K up to 64 behind the x2 layer 2; the non-prep | ensure_pack: D <= 16 false; wide_forward_pair per-net       |
|                                        | branch of ensure_pack (wide_pack_kernel, wide_pack_x2_kernel)       | fallback only past M 32768 (else the pair kernels)          |
| (5, 6, 256)                            | D % 4 != 0 with 4 < A <= 8: the fused producer / consumer kernels,  | wide_rs needs D % 4 == 0                                    |
|                                        | not the register-stationary ones                                    |                                                             |
| M % 128 != 0 (96, odd, < 32)           | the layer-wise update kernels behind a fused-shape network          | wide_update_route: wide_fused_ok && M % FX_MB == 0          |
| ragged M in (32768, 131072], wide_fuse 0| wide_dense_kernel<4, 2, 1, 2>, wide_dense_x2_kernel<EPI, 2>,        | dense_launch / dense_x2_launch / dense_x3_launch: M > 32768 |
|                                        | wide_dense_x3_kernel<EPI, 2, 8>                                     |                                                             |
| ragged M > 131072, wide_fuse 0          | wide_dense_x2_kernel<EPI, 4>                                        | dense_x2_launch: M > 131072                                 |
| rollout at 33,000 envs, obs 33          | per-network wide_forward with the M > 32768 tiles                   | wide_forward_pair: M <= 32768 false                         |
| wide_rollout_persist 2 / 1 / 0          | wide_rs_rollout_kernel / wide_rollout_pc_kernel (nt % 64 == 0),     | wide_rollout_route: wide_rollout_persist, nt % RP_MB, A <= 8 |
|                                        | wide_rollout_persist_kernel, wide_forward_pair + wide_step_kernel   |                                                             |
"""
import numpy as np
import pytest

import oraclelib as O
from test_gpu_parity import RTOL, _grad_close, crl, loss_close, rel_err  # noqa: F401  (crl is the module fixture)
from test_gpu_wide import force_wide, inject, make_wide, ocfg, rel_err_s, spread_params  # noqa: F401  (force_wide: CRL_FORCE_WIDE=1)

pytestmark = pytest.mark.gpu

LOSS_KEYS = ("loss", "pg_loss", "v_loss", "entropy_loss")
GEMM = [{"wide_gemm": 2}, {"wide_gemm": 1}, {"wide_gemm": 0}]
RATIONAL = {"wide_tanh_rational": 1}


def _ids(o):
    return ",".join(f"{a}={b}" for a, b in o.items()) or "default"


def _flavours(shapes, rational_on=None):
    """(shape, options) pairs: all three GEMM flavours at hidden 256 (at 64 / 128 the option selects nothing), wide_tanh_rational = 1
    on `rational_on` (every shape when None)."""
    out = []
    for s in shapes:
        for g in (GEMM if s[2] == 256 else GEMM[:1]):
            out.append(s + (g,))
        if rational_on is None or s in rational_on:
            out.append(s + (RATIONAL,))
    return out


def _forward64(params, off, D, H, NO, x, net=0):
    """float64 restatement of one network (Flux layout, column-major weights) on observations x (D, n)."""
    o = [int(v) for v in off[6 * net:6 * net + 7]]
    W1 = params[o[0]:o[1]].astype(np.float64).reshape((H, D), order="F"); b1 = params[o[1]:o[2]].astype(np.float64)
    W2 = params[o[2]:o[3]].astype(np.float64).reshape((H, H), order="F"); b2 = params[o[3]:o[4]].astype(np.float64)
    W3 = params[o[4]:o[5]].astype(np.float64).reshape((NO, H), order="F"); b3 = params[o[5]:o[6]].astype(np.float64)
    h = np.tanh(W1 @ x + b1[:, None])
    h = np.tanh(W2 @ h + b2[:, None])
    return W3 @ h + b3[:, None]


def _c3_spread_params(cfg, seed):
    """spread_params with the actor head rescaled so that the largest |logit| over 300 standard-normal observations is 33, what the
    x30 spread gives C3's shape (obs 8 / act 4 / 2x256). rel_err_s's floor is calibrated there; the same x30 at obs 33..64 or 16 actions
    spreads the logits to ±40..60, where float32 rounding of the logits alone (in the oracle as much as on the GPU) reaches 1e-5 of a
    log-probability near 0."""
    params = spread_params(cfg, seed)
    off = O.param_offsets(cfg)
    x = np.random.default_rng(0).standard_normal((cfg.obs_dim, 300))
    z = _forward64(params, off, cfg.obs_dim, cfg.hidden, cfg.n_act, x)
    params[off[4]:off[6]] *= np.float32(33.0 / np.abs(z).max())
    return params


# --------------------------------------------------------------------------------------------------------- host calls
ACT_SHAPES = [(8, 4, 256), (12, 16, 256), (33, 9, 256), (64, 16, 256), (64, 16, 128)]


@pytest.mark.parametrize("D,A,Hd,opts", _flavours(ACT_SHAPES, rational_on=[(8, 4, 256)]), ids=lambda v: _ids(v) if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("n", [1, 33, 300])
def test_policy_act_and_logprob_every_flavour(crl, D, A, Hd, opts, n):
    rng = np.random.default_rng(n + D + A)
    cfg = ocfg(8, 16, D, A, Hd)
    params = _c3_spread_params(cfg, 3)
    agent = make_wide(crl, 8, 16, D, A, Hd, params=params, options=opts)
    obs = np.asfortranarray(rng.standard_normal((D, n)).astype(np.float32))
    u = rng.random(n)
    a_o, lp_o, v_o, margin = O.get_action(cfg, params, obs, u)
    a_g, lp_g, v_g = agent.handle.policy_act(obs, u)
    safe = margin > 1e-6
    assert np.array_equal(a_g[safe], a_o[safe]), "action indices must be bit-exact away from CDF knots"
    assert safe.mean() > 0.98 and len(set(a_o.tolist())) >= min(A, 2 if n > 1 else 1)
    same = a_g == a_o
    assert rel_err_s(lp_g[same], lp_o[same]) < RTOL and rel_err(v_g, v_o) < RTOL
    acts = rng.integers(0, A, n).astype(np.int32)
    lp_o2, ent_o = O.logprob_actions(cfg, params, obs, acts)
    lp_g2, ent_g = crl.logprob_actions(obs, agent.actor, acts + 1)
    assert ent_g.shape == (A, n) and rel_err_s(lp_g2, lp_o2) < RTOL and rel_err(ent_g, ent_o) < RTOL
    agent.close()


# --------------------------------------------------------------------------------------------------------- rollout + GAE
def _rollout_cases():
    out = []
    P = lambda p: {"wide_rollout_persist": p}   # noqa: E731
    for s in [(8, 4, 256), (12, 16, 256), (33, 9, 256), (64, 16, 128)]:
        D, A, Hd = s
        opts = [{}]
        if Hd == 256:
            opts += [{"wide_gemm": 1}, {"wide_gemm": 0}]
            if D <= 16:                       # the persistent rollout kernels take obs <= 16 only; past 8 actions 2 and 1 are the same kernel
                opts += ([P(1)] if A <= 8 else []) + [P(0)]
        opts.append(RATIONAL)
        out += [s + (o,) for o in opts]
    return out


def _rollout_and_gae(crl, h, st):
    F = crl._lib
    h.rollout_run(); st.rollout()
    assert np.array_equal(h.read(F.F_ACTION), st.action), f"{np.sum(h.read(F.F_ACTION) != st.action)} actions differ"
    assert np.array_equal(h.read(F.F_OBS), st.obs) and np.array_equal(h.read(F.F_REWARD), st.reward)
    assert np.array_equal(h.read(F.F_TERMINAL), st.terminal) and np.array_equal(h.read(F.F_NEXT_DONE), st.next_done)
    assert np.array_equal(h.read(F.F_CUR_OBS), st.cur_obs)
    assert rel_err_s(h.read(F.F_LOGPROB), st.logprob) < RTOL and rel_err(h.read(F.F_VALUE), st.value) < RTOL
    es = h.episode_stats(); n_ep, ret_sum, len_sum = st.episode_stats
    assert es["episodes"] == n_ep and es["length_sum"] == len_sum and abs(es["return_sum"] - ret_sum) < 1e-4 * max(1, abs(ret_sum))
    h.compute_gae(); st.compute_gae()
    assert rel_err(h.read(F.F_ADVANTAGE), st.adv) < RTOL and rel_err(h.read(F.F_RETURN), st.ret) < RTOL


@pytest.mark.parametrize("D,A,Hd,opts", _rollout_cases(), ids=lambda v: _ids(v) if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("nt", [70, 128])
def test_rollout_every_flavour(crl, D, A, Hd, opts, nt):
    """num_envs = 128 takes the one-launch rollout kernels of the fp16x2 flavour (a multiple of 64 envs), 70 does not."""
    k = 8
    cfg = ocfg(nt, k, D, A, Hd)
    params = spread_params(cfg, 5)
    agent = make_wide(crl, nt, k, D, A, Hd, params=params, options=opts)
    st = O.State(cfg); st.params[:] = params; st.env_init()
    agent.handle.env_reset()
    _rollout_and_gae(crl, agent.handle, st)
    agent.close(); st.close()


@pytest.mark.parametrize("opts", [{}, {"wide_gemm": 1}], ids=_ids)
def test_rollout_past_32768_envs_per_network_launches(crl, opts):
    """obs 33 keeps every persistent rollout kernel away, and num_envs > 32768 sends wide_forward_pair to one wide_forward per network:
    layer 1 on wide_dense_kernel<4, 2, 1, 2>, layer 2 on the 64-sample tiles (wide_dense_x2_kernel<EPI, 2> / wide_dense_x3_kernel<EPI, 2, 8>).
    Integer fields and episode statistics bit-equal to the oracle. Over 66,000 samples the oracle's own float32 values are 8e-6 (rel_err)
    from a float64 evaluation, as large as the bar, so log-probabilities and values are held to RTOL against the float64 restatement instead
    (the same observations, actions and parameters), and the advantages to RTOL against the oracle's Float64 GAE of the GPU's own values."""
    D, A, Hd, nt, k = 33, 9, 256, 33000, 2
    cfg = ocfg(nt, k, D, A, Hd)
    params = spread_params(cfg, 6)
    off = O.param_offsets(cfg)
    params[off[4]:off[5]] /= 10                     # logits within ±6, as in the whole-iteration tests
    agent = make_wide(crl, nt, k, D, A, Hd, params=params, options=opts)
    st = O.State(cfg); st.params[:] = params; st.env_init()
    h = agent.handle; F = crl._lib
    h.env_reset()
    h.rollout_run(); st.rollout()
    assert np.array_equal(h.read(F.F_ACTION), st.action), f"{np.sum(h.read(F.F_ACTION) != st.action)} actions differ"
    assert np.array_equal(h.read(F.F_OBS), st.obs) and np.array_equal(h.read(F.F_REWARD), st.reward)
    assert np.array_equal(h.read(F.F_TERMINAL), st.terminal) and np.array_equal(h.read(F.F_NEXT_DONE), st.next_done)
    assert np.array_equal(h.read(F.F_CUR_OBS), st.cur_obs)
    es = h.episode_stats(); n_ep, ret_sum, len_sum = st.episode_stats
    assert es["episodes"] == n_ep and es["length_sum"] == len_sum and abs(es["return_sum"] - ret_sum) < 1e-4 * max(1, abs(ret_sum))
    x = st.obs.reshape(D, -1, order="F").astype(np.float64)
    z = _forward64(params, off, D, Hd, A, x)
    a = st.action.reshape(-1, order="F")
    zm = z.max(0)
    lp64 = z[a, np.arange(z.shape[1])] - (zm + np.log(np.exp(z - zm).sum(0)))
    v64 = _forward64(params, off, D, Hd, 1, x, net=1)[0]
    assert rel_err_s(h.read(F.F_LOGPROB).reshape(-1, order="F"), lp64) < RTOL
    assert rel_err(h.read(F.F_VALUE).reshape(-1, order="F"), v64) < RTOL
    h.compute_gae()
    nv = _forward64(params, off, D, Hd, 1, st.cur_obs.reshape(D, -1, order="F").astype(np.float64), net=1)[0].astype(np.float32)
    adv_o, ret_o = O.gae_batch(h.read(F.F_VALUE), st.reward, st.terminal, nv, st.next_done, cfg.gamma, cfg.gae_lambda, cfg.gae_mode)
    assert rel_err(h.read(F.F_ADVANTAGE), adv_o) < RTOL and rel_err(h.read(F.F_RETURN), ret_o) < RTOL
    agent.close(); st.close()


# --------------------------------------------------------------------------------------------------------- update gradient
UPD_SHAPES = [(8, 4, 256), (12, 16, 256), (33, 9, 256), (64, 16, 256), (64, 16, 128), (5, 6, 256)]
# minibatch sizes M = nt * k / 4: a multiple of 128 (the fused kernels where the shape allows), a multiple of 32 only, odd, below 32
UPD_SIZES = [(8, 64, 10.0, True), (12, 32, 0.05, True), (7, 52, 3.0, False), (3, 12, 10.0, True)]


@pytest.mark.parametrize("D,A,Hd,opts", _flavours(UPD_SHAPES), ids=lambda v: _ids(v) if isinstance(v, dict) else str(v))
@pytest.mark.parametrize("nt,k,ret_scale,clipv", UPD_SIZES)
def test_update_gradient_every_flavour(crl, D, A, Hd, opts, nt, k, ret_scale, clipv):
    """ret_scale = 0.05 drives u = mean(v - R²) > 0 (Q4): the unclipped-wins count must be live and equal."""
    rng = np.random.default_rng(nt + k + D + A)
    cfg = ocfg(nt, k, D, A, Hd, clip_value_loss=clipv)
    params = O.orthogonal_params(cfg, 5) + (0.05 * rng.standard_normal(O.lib().orc_param_count(cfg))).astype(np.float32)
    off = O.param_offsets(cfg)
    if ret_scale < 1:
        params[off[11]] = 0.3
    agent = make_wide(crl, nt, k, D, A, Hd, params=params, clip_value_loss=clipv, options=opts)
    st = O.State(cfg); st.params[:] = params
    inject(crl, agent, st, rng, D, A, ret_scale)
    h = agent.handle
    h.adv_stats()
    M = nt * k // 4
    for mb in (0, 3):
        gs = h.update_minibatch(mb, 2.5e-4, apply_update=False)
        g_gpu = h.read(crl._lib.F_GRADS)
        g_orc, so = O.loss_grad(cfg, params, st.obs.reshape(D, -1, order="F"), st.action, st.logprob, st.value, st.adv, st.ret,
                                st.perm[mb * M:(mb + 1) * M])
        if ret_scale < 1 and clipv:
            assert so["n_unclipped_wins"] > 0 and gs["n_unclipped_wins"] == so["n_unclipped_wins"]
        for key in LOSS_KEYS:
            assert loss_close(key, gs[key], so[key], RTOL), (mb, key, gs[key], so[key])
        _grad_close(g_gpu, g_orc, off)
    agent.close(); st.close()


@pytest.mark.parametrize("nt,k", [(1601, 100), (1501, 400)], ids=["M=40025", "M=150100"])
@pytest.mark.parametrize("D,A", [(8, 4), (33, 9)])
def test_large_ragged_minibatch_tiles_every_flavour(crl, D, A, nt, k):
    """Ragged minibatches past the M thresholds of the layer-wise launches, with wide_fuse = 0: M = 40,025 takes the 64-sample tiles
    (wide_dense_kernel<4, 2, 1, 2>, wide_dense_x2_kernel<EPI, 2>, wide_dense_x3_kernel<EPI, 2, 8>), M = 150,100 the 128-sample
    wide_dense_x2_kernel<EPI, 4>; both end in a partial tile. One minibatch, one oracle call; the three GEMM flavours on the same buffers."""
    Hd = 256
    rng = np.random.default_rng(nt + D)
    cfg = ocfg(nt, k, D, A, Hd)
    params = O.orthogonal_params(cfg, 5) + (0.05 * rng.standard_normal(O.lib().orc_param_count(cfg))).astype(np.float32)
    off = O.param_offsets(cfg)
    agent = make_wide(crl, nt, k, D, A, Hd, params=params, options={"wide_fuse": 0})
    st = O.State(cfg); st.params[:] = params
    inject(crl, agent, st, rng, D, A, 3.0)
    h = agent.handle
    h.adv_stats()
    M = nt * k // 4
    assert M % 32 and M > (131072 if k == 400 else 32768)
    mb = 3
    g_orc, so = O.loss_grad(cfg, params, st.obs.reshape(D, -1, order="F"), st.action, st.logprob, st.value, st.adv, st.ret,
                            st.perm[mb * M:(mb + 1) * M])
    for gemm in (2, 1, 0):
        h.set_option("wide_gemm", gemm)
        gs = h.update_minibatch(mb, 2.5e-4, apply_update=False)
        for key in LOSS_KEYS:
            assert loss_close(key, gs[key], so[key], RTOL), (gemm, key, gs[key], so[key])
        _grad_close(h.read(crl._lib.F_GRADS), g_orc, off)
    agent.close(); st.close()


# --------------------------------------------------------------------------------------------------------- whole iterations
@pytest.mark.parametrize("opts", [{}, {"wide_gemm": 1}, RATIONAL], ids=_ids)
@pytest.mark.parametrize("D,A", [(12, 16), (33, 9), (8, 4)])
def test_whole_iterations_every_flavour(crl, D, A, opts):
    """crl_ppo_iterate (rollout, GAE, serial Fisher–Yates, 4 epochs x 4 minibatches, ClipNorm + Adam) twice against orc_iterate, at the bars
    of test_gpu_wide.py::test_wide_full_iteration_matches_oracle: permutation and actions bit-equal, advantages and every loss record at
    1e-5 relative, parameters at 1e-5 absolute."""
    Hd, nt, k = 256, 16, 32
    cfg = ocfg(nt, k, D, A, Hd)
    params = spread_params(cfg, 7)
    off = O.param_offsets(cfg)
    params[off[4]:off[5]] /= 10
    agent = make_wide(crl, nt, k, D, A, Hd, params=params, shuffle_mode=0, options=opts)
    st = O.State(cfg); st.params[:] = params; st.env_init()
    h = agent.handle; F = crl._lib
    h.env_reset()
    for it in range(2):
        gs = h.iterate(1)
        os_ = st.iterate(10, gen_perm=True)
        assert np.array_equal(h.read(F.F_PERM), st.perm)
        acts = h.read(F.F_ACTION)
        assert np.array_equal(acts, st.action), f"iteration {it}: {np.sum(acts != st.action)} actions differ"
        assert rel_err(h.read(F.F_ADVANTAGE), st.adv) < RTOL
        assert len(gs) == len(os_) == 16
        for a, b in zip(gs, os_):
            for key in LOSS_KEYS:
                assert loss_close(key, a[key], b[key], RTOL), (it, key, a[key], b[key])
        assert np.max(np.abs(h.read(F.F_PARAMS) - st.params)) < 1e-5
    agent.close(); st.close()
