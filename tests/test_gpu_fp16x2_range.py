"""Range edges of the 64-wide fp16x2 products of the headline 4/2/64 path (csrc/mlp_x2.hpp) against the CPU oracle AND a float64 autograd
restatement (oraclelib.torch_loss): update_x2_kernel (update_tile = 32), update_t16_kernel with its repair launch (update_tile = 16), the rollout's
critic in the one-, two-, three- and six-wave kernels, and gemm = 1 (bf16x3 everywhere) as the control where range should not matter.

The fp16x2 products carry their accuracy in a scaling scheme, not in float32 operands: weights × 2^8 (a |w| >= 255 sends the role to bf16x3, and so
does a network whose largest hidden-layer weight is below 2^-11, where the fp16 lo pieces go subnormal), cotangents × a power of two per sample,
and the weight-gradient product × ONE carried scale G per launch and role, checked per tile. These tests drive each of those to its edges:
  (a) the weight window at both ends: hidden layers scaled by 1e-2 … 1e-5, one weight at ±254.9 (stays fp16x2), at ±255 (falls back);
  (b) cotangents spanning nine orders of magnitude in one launch, and a minibatch laid out so that, in ONE launch, some tiles fit G and others
      fall below X2_DW_SMALL or overflow X2_DW_OVER;
  (c) G across launches: the return-error scale jumps by 2^±24, G is mispredicted once and re-centred; both clamp ends of G.
Bars: every gradient array within RTOL = 1e-5 relative L2 of the float64 restatement, losses within RTOL of it; and the same against the
float32 oracle wherever that oracle is itself within RTOL / 2 of float64 — on the extreme data of (b) and (c) the oracle's own float32 rounding
can be the larger error (as for the 33,000-env rollout in test_gpu_wide_routes.py), and there float64 is the reference."""
import numpy as np
import pytest
import torch

import oraclelib as O
from test_gpu_parity import IT_LOSS, IT_PARAM, RTOL, loss_close, make_agent, rel_err

pytestmark = pytest.mark.gpu

NT, K = 8, 128
M = NT * K // 4                  # minibatch: 256 samples = 8 tiles of 32 (16 of 16)
LOSSES = ("loss", "pg_loss", "v_loss", "entropy_loss")
FLAVOURS = {"x2_32": {"gemm": 2, "update_tile": 32}, "x2_16": {"gemm": 2, "update_tile": 16}, "bf16x3": {"gemm": 1}}
X2 = ("x2_32", "x2_16")
# parameter arrays (param_offsets): 0-5 actor W1 b1 W2 b2 W3 b3, 6-11 the critic's
A_W2, C_W2, C_W3, C_B3 = 2, 8, 10, 11


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _base_params(cfgo, seed=5):
    rng = np.random.default_rng(seed)
    return O.orthogonal_params(cfgo, seed) + (0.05 * rng.standard_normal(O.lib().orc_param_count(cfgo))).astype(np.float32)


def _batch(rng, cfgo, params, ret_scale=10.0):
    """A synthetic rollout buffer in sample order (index i = env + num_envs·step, the order of the flat GPU fields), for any obs_dim / n_act. The
    returns sit below every value prediction: the critic's cotangent has one sign, so that dW3 = Σ h2·dv and db3 = Σ dv are not cancelling sums —
    with the near-constant h2 of a network of tiny hidden weights their float32 rounding (on any summation order) would otherwise be larger than
    the bar."""
    B, D, A = cfgo.num_envs * cfgo.num_steps, cfgo.obs_dim, cfgo.n_act
    b = dict(obs=rng.standard_normal((D, B)).astype(np.float32), action=rng.integers(0, A, B).astype(np.int32),
             logprob=(np.log(1.0 / A) + 0.3 * rng.standard_normal(B)).astype(np.float32), value=rng.standard_normal(B).astype(np.float32),
             adv=(2 * rng.standard_normal(B)).astype(np.float32), ret=(-5.0 - ret_scale * np.abs(rng.standard_normal(B))).astype(np.float32),
             perm=rng.permutation(B).astype(np.int32))
    return b


def _load(crl, h, st, b):
    F = crl._lib
    st.obs[:] = b["obs"].reshape(st.obs.shape, order="F")
    for name, f in (("action", F.F_ACTION), ("logprob", F.F_LOGPROB), ("value", F.F_VALUE), ("adv", F.F_ADVANTAGE), ("ret", F.F_RETURN)):
        arr = getattr(st, name)
        arr[:] = b[name].reshape(arr.shape, order="F")
        h.write(f, arr)
    st.perm[:] = b["perm"]
    h.write(F.F_OBS, st.obs); h.write(F.F_PERM, st.perm)
    h.adv_stats()


def _critic_value(cfgo, params, obs):
    return O.get_action(cfgo, params, obs, np.zeros(obs.shape[1]))[2]


def _float64(cfgo, params, b, idx):
    p64 = torch.tensor(params.astype(np.float64), requires_grad=True)
    off = O.param_offsets(cfgo)
    loss, pg, vl, ent = O.torch_loss(p64, cfgo, off, b["obs"][:, idx], b["action"][idx], b["logprob"][idx], b["value"][idx], b["adv"][idx], b["ret"][idx])
    loss.backward()
    return p64.grad.numpy(), {"loss": loss.item(), "pg_loss": pg.item(), "v_loss": vl.item(), "entropy_loss": ent.item()}


def _l2(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _reference(cfgo, params, b, mb):
    """Both references of minibatch `mb`: (oracle gradient, oracle stats, float64 gradient, float64 losses). They depend on the inputs alone:
    a test that runs several kernel flavours on one minibatch computes them once and hands them to _check_minibatch."""
    M = cfgo.num_envs * cfgo.num_steps // cfgo.num_minibatches
    idx = b["perm"][mb * M:(mb + 1) * M]
    g_o, so = O.loss_grad(cfgo, params, b["obs"], b["action"], b["logprob"], b["value"], b["adv"], b["ret"], idx)
    return (g_o, so) + _float64(cfgo, params, b, idx)


def _minibatch_errors(cfgo, ref, g):
    """The figures _check_minibatch asserts on, for one launch's gradient `g`: the float64 and oracle losses, per gradient array the relative L2
    error against float64 ("e64"), the oracle's own ("o64") and the error against the oracle ("eo")."""
    g_o, so, g64, l64 = ref
    off = O.param_offsets(cfgo)
    sl = [slice(off[i], off[i + 1]) for i in range(12)]
    return {"l64": l64, "lo": {key: so[key] for key in LOSSES}, "e64": [_l2(g[s], g64[s]) for s in sl],
            "o64": [_l2(g_o[s], g64[s]) for s in sl], "eo": [_l2(g[s], g_o[s]) for s in sl]}


def _check_minibatch(crl, h, cfgo, params, b, mb, tag, apply_update=False, rec=None, ref=None):
    """One update launch on minibatch `mb` against the float64 restatement (always) and the float32 oracle (where it is close to float64).
    `rec`, a list, receives the launch's figures (_minibatch_errors) before anything is asserted; `ref` is _reference(cfgo, params, b, mb)
    where the caller already has it."""
    gs = h.update_minibatch(mb, 0.0, apply_update=apply_update)
    g = h.read(crl._lib.F_GRADS)
    assert np.isfinite(g).all(), f"{tag}: non-finite gradient"
    e = _minibatch_errors(cfgo, _reference(cfgo, params, b, mb) if ref is None else ref, g)
    if rec is not None:
        rec.append(dict(e, gs={key: gs[key] for key in LOSSES}, tag=tag))
    l64, so = e["l64"], e["lo"]
    for key in LOSSES:
        assert loss_close(key, gs[key], l64[key], RTOL), (tag, key, gs[key], l64[key])
        if loss_close(key, so[key], l64[key], RTOL / 2):
            assert loss_close(key, gs[key], so[key], RTOL), (tag, key, gs[key], so[key])
    for i in range(12):
        assert e["e64"][i] < RTOL, f"{tag}: gradient array {i}: rel L2 error {e['e64'][i]:.3e} against float64"
        if e["o64"][i] < RTOL / 2:
            assert e["eo"][i] < RTOL, f"{tag}: gradient array {i}: rel L2 error {e['eo'][i]:.3e} against the oracle"
    return gs, g


# ---------------------------------------------------------------------------------------------------------
# (a) the weight window at both ends
WEIGHT_CASES = ([f"{who}*{f:g}" for f in (1e-2, 1e-3, 1e-4, 1e-5) for who in ("actor", "critic", "both")]
                + ["w=+254.9", "w=-254.9", "w=+255", "w=-255"])


def _weights(cfgo, case):
    off = O.param_offsets(cfgo)
    p = _base_params(cfgo)
    if case.startswith("w="):
        w = np.float32(case[2:])
        p[off[A_W2] + 11] = w          # one weight of each network's W2
        p[off[C_W2] + 7] = w
    else:
        who, f = case.split("*")
        f = np.float32(f)
        for arr, name in ((A_W2, "actor"), (C_W2, "critic")):
            if who in (name, "both"):
                p[off[arr]:off[arr + 1]] *= f
    return p


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("case", WEIGHT_CASES)
def test_hidden_weights_at_the_edges_of_the_fp16_window(crl, case, flavour):
    """Minibatch gradient and losses, one whole iteration and (for the two rollout flavours) the rollout in every small-shard kernel, for hidden
    layers scaled down to 1e-5 and single weights just inside and just outside |w| < 255. 254.9 must stay on fp16x2 (gemm_fallback_seen stays 0
    on a fresh handle), ±255 must fall back (it goes to 1), and so must a network whose largest hidden weight is below 2^-11. The few
    comparisons listed in GRADIENT_MISSES / VALUE_MISSES miss the bar for a reason outside the fp16 window; they run, as strict xfails, in
    test_known_misses_of_the_exp2_activation_next_to_a_large_weight."""
    cfgo = O.make_config(num_envs=NT, num_steps=K)
    params = _weights(cfgo, case)
    opts = FLAVOURS[flavour]
    # one whole iteration (rollout, GAE, 4 epochs x 4 minibatches, ClipNorm + Adam) from a fresh handle
    agent = make_agent(crl, nt=NT, k=K, params=params, shuffle_mode=0, options=opts)
    h = agent.handle
    st = O.State(cfgo); st.params[:] = params; st.env_init()
    h.env_reset()
    gs = h.iterate(1)
    os_ = st.iterate(10, gen_perm=True)
    edge = case.startswith("w=")
    assert np.array_equal(h.read(crl._lib.F_ACTION), st.action)
    for a, b in zip(gs, os_):
        for key in LOSSES:
            assert loss_close(key, a[key], b[key], RTOL if edge else IT_LOSS), (key, a[key], b[key])
    if edge:   # next to a weight of 255 (see GRADIENT_MISSES below): the north-star bar, as smoke()
        assert np.allclose(h.read(crl._lib.F_PARAMS), st.params, rtol=1e-4, atol=1e-6)
    else:
        assert np.max(np.abs(h.read(crl._lib.F_PARAMS) - st.params)) < IT_PARAM
    agent.close(); st.close()

    agent = make_agent(crl, nt=NT, k=K, params=params, options=opts)
    h = agent.handle
    assert h.get_option("gemm_fallback_seen") == 0
    st = O.State(cfgo); st.params[:] = params
    b = _batch(np.random.default_rng(11), cfgo, params)
    _load(crl, h, st, b)
    for mb in (0, 2):
        if (case, flavour) in GRADIENT_MISSES:   # compared in test_known_misses_of_the_exp2_activation_next_to_a_large_weight
            assert np.isfinite(h.update_minibatch(mb, 0.0, apply_update=False)["loss"]) and np.isfinite(h.read(crl._lib.F_GRADS)).all()
        else:
            _check_minibatch(crl, h, cfgo, params, b, mb, f"{case} mb {mb}")
    if flavour != "x2_16":        # the rollout kernels do not depend on update_tile
        for split in (0, 1, 2, 3):
            h.set_option("rollout_split", split)
            st2 = O.State(cfgo); st2.params[:] = params; st2.env_init()
            h.env_reset(); h.rollout_run(); st2.rollout()
            assert np.array_equal(h.read(crl._lib.F_ACTION), st2.action), (case, split)
            if (case, flavour, split) not in VALUE_MISSES:   # (the same)
                assert rel_err(h.read(crl._lib.F_VALUE), st2.value) < RTOL, (case, split)
            st2.close()
    # the fallback flag: raised exactly when a network's W2 has a |w| >= 255 or its largest |w| is below 2^-11 (X2_W_SMALL, mlp_x2.hpp);
    # gemm = 1 never stages fp16x2 pieces and never raises it
    off = O.param_offsets(cfgo)
    w2max = [np.abs(params[off[i]:off[i + 1]]).max() for i in (A_W2, C_W2)]
    falls_back = any(m >= 255.0 or m < 2.0 ** -11 for m in w2max)
    assert h.get_option("gemm_fallback_seen") == (1 if flavour in X2 and falls_back else 0), (case, w2max)
    agent.close(); st.close()


# Known misses of the 1e-5 bar, all next to a weight of ±254.9 / +255 on a kernel that keeps the exp2 activation (the fp16x2 kernels inside the
# window, gemm = 1 everywhere; the bf16x3 fallbacks past the window use the reference's rational tanh_fast and meet the bar). That activation has
# an ABSOLUTE error of a few 1e-8 near 0, where tanh_fast is accurate relative to |h|; a weight of 255 multiplies the error of a small h1 into
# the next pre-activation (≈1e-5) and from there into the value and the W1 / b1 gradients. The fp16 window plays no part: the same mechanism
# should be reachable with any large weight. It is a defect of the activation, kept visible here as strict xfails until it is fixed.
GRADIENT_MISSES = {("w=+254.9", "x2_32"), ("w=+254.9", "bf16x3"), ("w=+255", "bf16x3")}   # critic W1: 1.2e-5 against float64
VALUE_MISSES = {(c, "x2_32", sp) for c in ("w=+254.9", "w=-254.9") for sp in (0, 1, 3)}     # rollout critic on fp16x2: 4e-5


@pytest.mark.xfail(strict=True, reason="the exp2 activation's absolute error near 0, multiplied by a weight of 255: up to 1.2e-5 on the "
                   "critic's W1 gradient and 4e-5 on rollout values (the rational tanh_fast of the reference and of the bf16x3 fallbacks meets the bar)")
@pytest.mark.parametrize("what", sorted(GRADIENT_MISSES) + sorted({(c, "rollout") for c, _, _ in VALUE_MISSES}))
def test_known_misses_of_the_exp2_activation_next_to_a_large_weight(crl, what):
    """The comparisons test_hidden_weights_at_the_edges_of_the_fp16_window leaves out, each against the bar it misses: the minibatch gradient
    against float64 (and the oracle), or the rollout critic's values of the one-, three- and six-wave kernels against the oracle."""
    case, flavour = what
    cfgo = O.make_config(num_envs=NT, num_steps=K)
    params = _weights(cfgo, case)
    agent = make_agent(crl, nt=NT, k=K, params=params, options=FLAVOURS["x2_32" if flavour == "rollout" else flavour])
    h = agent.handle
    st = O.State(cfgo); st.params[:] = params
    try:
        if flavour == "rollout":
            for split in (0, 1, 3):
                h.set_option("rollout_split", split)
                st2 = O.State(cfgo); st2.params[:] = params; st2.env_init()
                h.env_reset(); h.rollout_run(); st2.rollout()
                err = rel_err(h.read(crl._lib.F_VALUE), st2.value)
                st2.close()
                assert err < RTOL, (case, split, err)
        else:
            b = _batch(np.random.default_rng(11), cfgo, params)
            _load(crl, h, st, b)
            for mb in (0, 2):
                _check_minibatch(crl, h, cfgo, params, b, mb, f"{case} mb {mb}")
    finally:
        agent.close(); st.close()


# ---------------------------------------------------------------------------------------------------------
# (b) cotangents of very different size inside one launch
def _set_return_errors(cfgo, params, b, err):
    """R = v + err, with v the critic's own prediction (clip_value_loss = False: the critic's cotangent is v − R = −err per sample)."""
    b["ret"] = (_critic_value(cfgo, params, b["obs"]).astype(np.float64) + err).astype(np.float32)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_cotangents_spanning_nine_orders_of_magnitude(crl, flavour):
    """The layer-wise path's test (test_gpu_wide.py) on the headline kernels: advantages and return errors from 1e-6 to 1e3, two envs' worth of
    samples with advantage 0 and return error 0 (up to the critic's float32 rounding) among them."""
    cfgo = O.make_config(num_envs=NT, num_steps=K, clip_value_loss=False)
    params = _base_params(cfgo)
    rng = np.random.default_rng(77)
    agent = make_agent(crl, nt=NT, k=K, params=params, clip_value_loss=False, options=FLAVOURS[flavour])
    h = agent.handle
    st = O.State(cfgo); st.params[:] = params
    b = _batch(rng, cfgo, params)
    mag = 10.0 ** rng.uniform(-6, 3, NT * K)
    mag[(np.arange(NT * K) % NT) < 2] = 0.0       # envs 0 and 1
    b["adv"] = (b["adv"] * mag).astype(np.float32)
    _set_return_errors(cfgo, params, b, 3.0 * np.abs(rng.standard_normal(NT * K)) * mag)
    _load(crl, h, st, b)
    for mb in (0, 2, 2):
        _check_minibatch(crl, h, cfgo, params, b, mb, f"mb {mb}")
    agent.close(); st.close()


# tile kinds of the structured minibatch, by 32-sample tile of the launch (positions 32t … 32t + 31 of the minibatch: update.hip walks a minibatch
# in tiles of consecutive positions, and the 16-sample kernel in halves of them). Critic: return-error scale of the tile, relative to the launch
# before it; "0" = the critic's own prediction as return. Actor: "clip" = every sample on the clipped side of the PPO objective (zero cotangent).
CRITIC_TILES = (1.0, 2.0 ** 17, 0.0, 1.0, 2.0 ** -24, 2.0 ** 17, 1.0, 0.0)
ACTOR_TILES = ("live", "clip", "live", "clip", "clip", "live", "clip", "live")


def _structured(rng, cfgo, params, b, mb):
    idx = b["perm"][mb * M:(mb + 1) * M]
    err = 3.0 * rng.standard_normal(NT * K)
    adv = b["adv"].astype(np.float64)
    # advantages of the clipped tiles: |A| >= 1 on a minibatch whose mean is ≈ 0, so that the sign of the normalised advantage is the sign of A
    for t in range(M // 32):
        s = idx[32 * t:32 * t + 32]
        err[s] *= CRITIC_TILES[t]
        if ACTOR_TILES[t] == "clip":
            adv[s] = np.sign(adv[s] + 1e-30) * (1.0 + np.abs(adv[s]))
    adv[idx] -= adv[idx].mean()
    b["adv"] = adv.astype(np.float32)
    nlp = O.logprob_actions(cfgo, params, b["obs"], b["action"])[0].astype(np.float64)
    lp = b["logprob"].astype(np.float64)
    for t in range(M // 32):
        if ACTOR_TILES[t] == "clip":
            s = idx[32 * t:32 * t + 32]
            # ratio = e (> 1 + clip) where the advantage is positive, 1/e (< 1 − clip) where it is negative: the clipped branch wins, d/dθ = 0
            lp[s] = nlp[s] - np.sign(b["adv"][s])
    b["logprob"] = lp.astype(np.float32)
    _set_return_errors(cfgo, params, b, err)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_tiles_that_fit_underflow_and_overflow_the_carried_scale_in_one_launch(crl, flavour):
    """Minibatch 0 (plain data) sets the carried weight-gradient scale G; minibatch 1 then has, in ONE launch, critic tiles at the scale G was set
    for (fit), tiles 2^17 larger (|δ2|·G past X2_DW_OVER), tiles 2^-24 smaller and tiles of zero return error (below X2_DW_SMALL), and actor
    tiles whose every sample sits on the clipped side of the objective with ent_coeff = 0 (an exactly zero cotangent: below X2_DW_SMALL).
    The fp16x2 kernels must take bf16x3 (32-sample tiles) or the repair launch (16-sample tiles) for exactly those tiles and still meet the bar;
    G of the critic must then re-centre on the larger data."""
    cfgo = O.make_config(num_envs=NT, num_steps=K, clip_value_loss=False, ent_coeff=0.0)
    params = _base_params(cfgo)
    rng = np.random.default_rng(19)
    agent = make_agent(crl, nt=NT, k=K, params=params, clip_value_loss=False, ent_coeff=0.0, options=FLAVOURS[flavour])
    h = agent.handle
    st = O.State(cfgo); st.params[:] = params
    b = _batch(rng, cfgo, params)
    _structured(rng, cfgo, params, b, 1)
    _load(crl, h, st, b)
    _check_minibatch(crl, h, cfgo, params, b, 0, "plain minibatch")
    _check_minibatch(crl, h, cfgo, params, b, 0, "plain minibatch, G settled")
    g_before = h.get_option("dw_scale_log2_critic")
    _check_minibatch(crl, h, cfgo, params, b, 1, "fit / over / small tiles")
    if flavour in X2:
        # the tiles 2^17 above the settled scale moved the launch's largest |δ2| out of G's band: re-centred by a multiple of 8 downwards
        g_after = h.get_option("dw_scale_log2_critic")
        assert g_after < g_before and (g_before - g_after) % 8 == 0, (g_before, g_after)
        assert h.get_option("gemm_fallback_seen") == 0       # range misses of G are not weight-window fallbacks
    _check_minibatch(crl, h, cfgo, params, b, 1, "fit / over / small tiles, G re-centred")
    agent.close(); st.close()


# ---------------------------------------------------------------------------------------------------------
# (c) G across launches
def _scaled_critic_head(cfgo, base, b0, s):
    """Critic head W3, b3 and the returns × 2^s: the value, its error and the head cotangent scale by 2^s, δ2 (and dW2, db2, dW1, db1, the value
    loss) by 2^2s — exactly, so every launch has a float64 reference and only the magnitudes move."""
    off = O.param_offsets(cfgo)
    p = base.copy()
    f = np.float32(2.0 ** s)
    p[off[C_W3]:off[C_B3 + 1]] *= f
    b = dict(b0)
    b["ret"] = (b0["ret"] * f).astype(np.float32)
    return p, b


def _largest_d2_log2(cfgo, params, b, mb):
    """log2 of the critic's largest |δ2| on minibatch `mb` (float64 forward; clip_value_loss = False: dv = v_coef·(v − R) / M)."""
    off = O.param_offsets(cfgo)
    q = params.astype(np.float64)
    W1, b1 = q[off[6]:off[7]].reshape(4, 64).T, q[off[7]:off[8]]
    W2, b2 = q[off[8]:off[9]].reshape(64, 64).T, q[off[9]:off[10]]
    W3, b3 = q[off[10]:off[11]].reshape(64, 1).T, q[off[11]:off[12]]
    idx = b["perm"][mb * M:(mb + 1) * M]
    h2 = np.tanh(W2 @ np.tanh(W1 @ b["obs"][:, idx].astype(np.float64) + b1[:, None]) + b2[:, None])
    dv = cfgo.v_coef * ((W3 @ h2)[0] + b3[0] - b["ret"][idx]) / M
    return float(np.log2(np.max(np.abs(W3.T * dv[None, :] * (1.0 - h2 * h2)))))


def _g_steps(L):
    """(head exponent s, what the launch is) for a base whose largest |δ2| is 2^L: δ2 moves by 2^2s. s_lo puts the largest |δ2| below 2^-94 (G goes
    to its clamp 2^100); s_hi then brings it to ≈ 2^2, about the largest δ2 whose products with G = 2^100 and the 2^14 activation scale still sum
    over a launch to a finite float32 (the tiles that overflow fp16 take the fallback with the same G). Every "repeat" runs the launch before it
    again at the G that launch left unchanged: its bits must not change."""
    s_lo, s_hi = int(np.floor((-94 - L) / 2)), int(np.floor((2 - L) / 2))
    return ((0, "start"), (0, "settled"), (0, "repeat"), (12, "jump up"), (12, "re-centred"), (12, "repeat"), (0, "drop"), (0, "re-centred"),
            (0, "repeat"), (-12, "drop"), (-12, "re-centred"), (-12, "repeat"), (0, "jump up"), (s_lo, "below 2^-92"), (s_lo, "at the upper clamp"),
            (s_lo, "repeat"), (s_hi, "after the upper clamp"), (s_hi, "re-centred"), (s_hi, "repeat"), (0, "back"))


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_carried_scale_follows_the_data_across_launches(crl, flavour):
    """A sequence of optimiser steps (η = 0: ClipNorm + Adam run, the parameters stay) on one handle while the critic's cotangents jump by 2^±24 and
    to the upper end of G's clamp [2^-100, 2^100]. Every launch — the first after a jump (G mispredicted: its tiles take the fallback) and the one
    after it (G re-centred) — against float64; G is read back after each launch and must have moved (or stayed) as mlp_x2.hpp says. The same
    minibatch twice at the same G (each "repeat" step) gives the same bits — checked at six points of the sequence, including the clamp."""
    cfgo = O.make_config(num_envs=NT, num_steps=K, clip_value_loss=False)
    base = _base_params(cfgo)
    agent = make_agent(crl, nt=NT, k=K, params=base, clip_value_loss=False, options=FLAVOURS[flavour])
    h = agent.handle
    st = O.State(cfgo); st.params[:] = base
    b0 = _batch(np.random.default_rng(23), cfgo, base)
    steps = _g_steps(_largest_d2_log2(cfgo, base, b0, 1))
    x2 = flavour in X2
    G, same_bits = [], 0
    prev, last = None, None
    for s, what in steps:
        p, b = _scaled_critic_head(cfgo, base, b0, s)
        if prev is None or s != prev[0]:
            agent.set_params(p); st.params[:] = p
            _load(crl, h, st, b)
        g_in = (h.get_option("dw_scale_log2_actor"), h.get_option("dw_scale_log2_critic"))
        gs, g = _check_minibatch(crl, h, cfgo, p, b, 1, f"head 2^{s} ({what})", apply_update=True)
        assert np.array_equal(h.read(crl._lib.F_PARAMS), p)
        G.append(h.get_option("dw_scale_log2_critic") if x2 else 0)
        if what == "repeat":
            assert (s, g_in) == prev, f"head 2^{s}: the launch before this repeat moved G"
            assert np.array_equal(g, last[1]) and gs["loss"] == last[0]["loss"], f"head 2^{s} ({what}): same minibatch, same G, different bits"
            same_bits += 1
        prev, last = (s, g_in), (gs, g)
    assert same_bits == 6
    if x2:
        assert all(v % 8 == 0 or abs(v) == 100 for v in G), G
        assert G[3] < G[2] and G[4] == G[3] == G[5], G           # data x 2^24: re-centred after the first launch, then sticky
        assert G[6] > G[5] and G[7] == G[6] == G[8], G           # and back
        assert G[9] > G[8] and G[10] == G[9] == G[11], G
        assert G[12] < G[11], G
        assert G[13] == G[14] == G[15] == 100, G                 # largest |δ2| below 2^-92: the upper clamp
        assert G[16] < 100 and G[17] == G[16] == G[18], G
        assert h.get_option("gemm_fallback_seen") == 0
    agent.close(); st.close()


def test_carried_scale_reaches_its_lower_clamp(crl):
    """The other end of G's clamp: a launch whose largest |δ2| is 2^108 or more sends G to 2^-100 (reached in two steps, the first one to 2^86: from the
    initial G the fallback tiles' products with the 2^14 activation scale would not stay finite), and the launches there stay within the bar."""
    cfgo = O.make_config(num_envs=NT, num_steps=K, clip_value_loss=False)
    base = _base_params(cfgo)
    agent = make_agent(crl, nt=NT, k=K, params=base, clip_value_loss=False, options=FLAVOURS["x2_32"])
    h = agent.handle
    st = O.State(cfgo)
    b0 = _batch(np.random.default_rng(29), cfgo, base)
    # return error 1/2: the float32 sum of the value-loss terms (× 2^2s) over the launch stays finite
    _set_return_errors(cfgo, base, b0, np.full(NT * K, 0.5))
    L = _largest_d2_log2(cfgo, base, b0, 1)
    for target, what in ((86, "mispredicted"), (86, "settled"), (108, "mispredicted"), (108, "at the lower clamp")):
        s = int(np.ceil((target - L) / 2))
        p, b = _scaled_critic_head(cfgo, base, b0, s)
        agent.set_params(p); st.params[:] = p
        _load(crl, h, st, b)
        _check_minibatch(crl, h, cfgo, p, b, 1, f"largest δ2 2^{target} ({what})")
    assert h.get_option("dw_scale_log2_critic") == -100
    assert -100 <= h.get_option("dw_scale_log2_actor") <= 100
    agent.close(); st.close()
