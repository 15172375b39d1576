"""The case table of the 256-wide range tests: test_wide_range_cpu.py (the float32 oracle alone against float64: the precondition) and
test_gpu_wide_range.py (the HIP kernels against both) build their parameters, minibatches and observations here, so that both see the same bits.

A case is a name of CASES; build(case, D, A) gives its oracle config, its parameter vector and its synthetic rollout buffer (num_envs = 8,
num_steps = 128, four minibatches of M = 256 = two 128-sample tiles = eight 32-sample slabs; hidden 256), forward_inputs(case, D, A, n) the
parameters and n observations for the forward consumers. Results are cached and must be left unchanged by their users."""
import functools

import numpy as np

import oraclelib as O
from test_gpu_fp16x2_range import _batch, _reference, _set_return_errors

NT, K, HID = 8, 128, 256
M = NT * K // 4
SHAPES = ((8, 4), (3, 2), (33, 9))      # C3's; obs_dim % 4 != 0 (the wide_fused.hpp kernels); obs_dim > 16 (no fused W1 fragments)
# parameter arrays (param_offsets): 0-5 actor W1 b1 W2 b2 W3 b3, 6-11 the critic's
A_W1, A_B1, A_W2, A_W3, C_W1, C_B1, C_W2, C_W3 = 0, 1, 2, 4, 6, 7, 8, 10

# option sets of the update launch. fp16x2: every kernel family that stages fp16x2 pieces; controls: no fp16 window at all
X2_FLAVOURS = {"default": {}, "rs=11": {"wide_rs": 11}, "rs=0": {"wide_rs": 0}, "fuse=0": {"wide_fuse": 0},
               "d2_split=0": {"wide_fuse": 3, "wide_d2_split": 0}, "wgrad_full=0": {"wide_fuse": 3, "wide_wgrad_full": 0}}
CONTROLS = {"bf16x3": {"wide_gemm": 1}, "f32": {"wide_gemm": 0}}
RATIONAL = {"rational": {"wide_tanh_rational": 1}}     # the fp16x2 products with the reference's tanh_fast: separates activation from window
FLAVOURS = {**X2_FLAVOURS, **CONTROLS, **RATIONAL}

W2_MAGNITUDE = ["W2*1e-2", "W2*1e-4", "W2*1e-6", "W2*1e-8", "W2max=2^-2", "W2max<2^-2", "criticW2=0"]
W2_LADDER = ["w2=2^8", "w2=2^12", "w2=2^16", "w2=2^20", "w2=2^24"]
W2_RANGE = W2_LADDER + ["w2=300"]
W1_CASES = ["W1*1e-3", "W1*1e-6", "w1=100", "w1=1e4"]
W3_CASES = ["w3*1e6"]
OBS_CASES = ["obs*1e-6", "obs*1e-3", "obs*1e6", "obs/feature", "obs/sample"]
SLAB_LADDER = [f"slab=2^{e}" for e in (0, 8, 16, 24, 32, 40)]     # (small, big) = (1, 2^e): the ratios of (2^-e/2, 2^e/2), see _slab
# the same slabs with BOTH ends moved, (small, big) = (2^-e, 2^e): the small samples' h1 ≈ W1·x is then 2^-e itself (b1 = 0), which is the exp2
# activation's weak spot and not the slab scale's — see _slab. The activation is the same under every product flavour: one of each family runs
TINY_LADDER = [f"tiny=2^{e}" for e in (4, 8, 12, 16, 20)]
TINY_FLAVOURS = ("default", "fuse=0", "bf16x3", "f32", "rational")
COT_CASES = ["cotangents"]
LARGE_WEIGHT = W2_RANGE + ["w1=100", "w1=1e4", "w3*1e6"]          # where the activation control runs
PARAM_CASES = W2_MAGNITUDE + W2_RANGE + W1_CASES + W3_CASES
# forward consumers: every parameter and observation case on which the float32 oracle's own per-sample error leaves a kernel room under the bar
# (test_wide_range_cpu.py asserts it below RTOL; the largest that stays in is 6e-6). The head-weight case does not: a value of 1e6·w·h2[k] + 255
# small terms carries the float32 rounding of h2[k] a million times over, and the oracle's values are 1.4e-5 from float64 on obs 33 (over the
# bar) and 9.4e-6 on obs 8 — under it by 6 %, where an equally good kernel passes or fails by its summation order. It is left out on both.
FORWARD_CASES = W2_MAGNITUDE + W2_RANGE + W1_CASES + OBS_CASES
CASES = PARAM_CASES + OBS_CASES + SLAB_LADDER + TINY_LADDER + COT_CASES
LADDER_COL = 162
BIG_POS = 5                        # position of the big sample inside every 32-sample slab of a minibatch


def shapes_of(case):
    """The shapes a case runs on: all three, but ladder 2 and ±300 on the base network alone, and the head-weight case not on two actions — on
    the other shapes the float32 oracle itself misses RTOL / 2 there (test_wide_range_cpu.py would fail: conditioning, not a kernel)."""
    if case in W2_RANGE or case in TINY_LADDER:
        return SHAPES[:1]
    if case in W3_CASES:
        return (SHAPES[0], SHAPES[2])
    return SHAPES


def config(case, D, A, nt=NT, k=K):
    kw = {}
    if case in SLAB_LADDER or case in TINY_LADDER:
        kw = dict(ent_coeff=0.0)
    elif case in COT_CASES:
        kw = dict(clip_value_loss=False)
    return O.make_config(num_envs=nt, num_steps=k, obs_dim=D, n_act=A, hidden=HID, env_kind=1, **kw), kw


def _pow2(txt):
    return np.float32(2.0 ** int(txt.split("^")[1]))


def params_of(case, cfgo, seed=5):
    rng = np.random.default_rng(seed)
    p = O.orthogonal_params(cfgo, seed) + (0.05 * rng.standard_normal(O.lib().orc_param_count(cfgo))).astype(np.float32)
    off = O.param_offsets(cfgo)
    sl = lambda i: slice(off[i], off[i + 1])
    if case.startswith("W2*"):
        f = np.float32(case[3:])
        p[sl(A_W2)] *= f; p[sl(C_W2)] *= f
    elif case.startswith("W2max"):
        top = _pow2(case)
        if case[5] == "<":
            top = np.nextafter(top, np.float32(0))
        for i in (A_W2, C_W2):
            w = p[sl(i)].astype(np.float64)
            j = int(np.argmax(np.abs(w)))
            w *= 0.999 * float(top) / np.abs(w[j])
            w[j] = np.sign(w[j]) * float(top)        # the largest |w| is `top` to the bit
            p[sl(i)] = w.astype(np.float32)
            assert np.abs(p[sl(i)]).max() == top
    elif case == "criticW2=0":
        p[sl(C_W2)] = 0.0
    elif case.startswith("w2="):
        # 300: the weights test_wide_fp16x2_weight_scale_follows_the_weights sets. The ladder: row 7 / 11 of column LADDER_COL, the input unit whose
        # |h1| stays above 3e-3 on minibatches 0 and 2 in both networks — from 2^12 on every sample saturates the unit the weight feeds; a sample
        # that leaves it unsaturated under a weight that large dominates dW1 and is ill-conditioned in float32 (the oracle alone misses there)
        w, col = (np.float32(300.0), 0) if case == "w2=300" else (_pow2(case), LADDER_COL)
        p[off[C_W2] + 7 + HID * col] = w; p[off[A_W2] + 11 + HID * col] = -w
    elif case.startswith("W1*"):
        f = np.float32(case[3:])
        p[sl(A_W1)] *= f; p[sl(C_W1)] *= f
    elif case.startswith("w1="):
        w = np.float32(case[3:])
        p[off[C_W1] + 7] = w; p[off[A_W1] + 11] = -w
    elif case == "w3*1e6":
        p[off[C_W3] + 7] *= np.float32(1e6); p[off[A_W3] + 11] *= np.float32(1e6)
    elif case in SLAB_LADDER or case in TINY_LADDER:
        p[sl(A_B1)] = 0.0; p[sl(C_B1)] = 0.0         # h1 of the small samples depends on x alone
    return p


def scale_obs(case, rng, obs, top=3):
    """The observation cases' magnitudes on unit-scale observations (D, n); per-feature magnitudes 10^U(top − 7, top)."""
    D, n = obs.shape
    if case.startswith("obs*"):
        return (obs * np.float32(case[4:])).astype(np.float32)
    if case == "obs/feature":
        return (obs * (10.0 ** rng.uniform(top - 7, top, (D, 1)))).astype(np.float32)
    if case == "obs/sample":
        # seven orders of magnitude between samples, topping out at 10 and not at 1e3: a whole SAMPLE of magnitude 1e3 has pre-activations of a
        # few hundred with float32 rounding of 1e-4 under them, and it dominates dW1 = Σ δ1·xᵀ — the oracle alone is then 2e-5 from float64
        return (obs * (10.0 ** rng.uniform(-6, 1, (1, n)))).astype(np.float32)
    return obs


def saturated(rng, cfgo, params, obs):
    """obs*1e6 promises that EVERY first-layer unit of every sample saturates (|W1·x + b1| >= 8.13, where tanh_fast returns ±1 and its derivative an
    exact zero); of 2 x 256 units x n samples a few land below that by chance, and there the pre-activation — a cancelling sum of terms 1e6 large —
    is ill-conditioned in float32. Samples with a unit below 64 are drawn again until none is left."""
    off = O.param_offsets(cfgo)
    d, h = cfgo.obs_dim, cfgo.hidden
    q = params.astype(np.float64)
    W1 = np.concatenate([q[off[i]:off[i + 1]].reshape(d, h).T for i in (A_W1, C_W1)])
    b1 = np.concatenate([q[off[i]:off[i + 1]] for i in (A_B1, C_B1)])
    obs = obs.copy()
    for _ in range(100):
        bad = np.abs(W1 @ obs.astype(np.float64) + b1[:, None]).min(axis=0) < 64.0
        if not bad.any():
            return obs
        obs[:, bad] = (rng.standard_normal((d, int(bad.sum()))) * 1e6).astype(np.float32)
    raise AssertionError("no saturating observations found")


@functools.lru_cache(maxsize=None)
def build(case, D, A):
    """(cfgo, config keywords, params, batch): the batch in sample order, as _batch of test_gpu_fp16x2_range.py."""
    cfgo, kw = config(case, D, A)
    params = params_of(case, cfgo)
    rng = np.random.default_rng(11)
    b = _batch(rng, cfgo, params)
    B = NT * K
    if case in OBS_CASES:
        b["obs"] = scale_obs(case, rng, b["obs"])
        if case == "obs*1e6":
            b["obs"] = saturated(rng, cfgo, params, b["obs"])
    elif case in COT_CASES:
        # the nine-orders case of test_gpu_wide.py / test_gpu_fp16x2_range.py: advantages and return errors from 1e-6 to 1e3, two envs at zero
        mag = 10.0 ** rng.uniform(-6, 3, B)
        mag[(np.arange(B) % NT) < 2] = 0.0
        b["adv"] = (b["adv"] * mag).astype(np.float32)
        _set_return_errors(cfgo, params, b, 3.0 * np.abs(rng.standard_normal(B)) * mag)
    elif case in SLAB_LADDER:
        _slab(rng, cfgo, params, b, 1.0, 2.0 ** int(case.split("^")[1]))
    elif case in TINY_LADDER:
        _slab(rng, cfgo, params, b, 2.0 ** -int(case.split("^")[1]), 2.0 ** int(case.split("^")[1]))
    return cfgo, kw, params, b


@functools.lru_cache(maxsize=None)
def reference(case, D, A, mb):
    """(oracle gradient, oracle stats, float64 gradient, float64 losses) of minibatch `mb`: computed once, shared by every flavour."""
    cfgo, _, params, b = build(case, D, A)
    return _reference(cfgo, params, b, mb)


def big_mask(b):
    """True for the samples that sit at position BIG_POS of a 32-sample slab of their minibatch."""
    big = np.zeros(NT * K, bool)
    big[b["perm"][BIG_POS::32]] = True               # M is a multiple of 32: positions through perm, every minibatch alike
    return big


def _slab(rng, cfgo, params, b, small, big_mag):
    """After _structured of test_gpu_fp16x2_range.py: in minibatch order every 32nd sample has observations of magnitude `big_mag` and
    no cotangent at all; the 31 samples around it have magnitude `small` and carry the whole gradient. The actor's side: the clipped side of the
    objective with ent_coeff = 0. The critic's side: return = the critic's own value, and — so that the zero is exact in float32 and in float64
    alike — the clipped side of the VALUE loss too (clip_value_loss = True, old value = the critic's value + 1: v_clipped is a constant, and
    (v_clipped − R)² = 0.64 is above u = mean(v − R²) < 0). With return = value alone (clip_value_loss = False) the big samples keep a cotangent
    of the critic's float32 rounding, ≈ 1e-7·|v|, which the ratio big / small = 2^2e multiplies: the float32 oracle itself then misses the bar
    from 2^8 on (1e-4 on the critic's W1, measured) and the case would say nothing about a kernel. The small samples' old value is the
    critic's value: their value loss is unclipped, (v − R)² with R = v + error.
    Two ladders use it. SLAB_LADDER holds small at 1 and raises big alone, to the ratios 1, 2^8 … 2^40: what a scale shared by a slab loses
    depends on the ratio alone, and with h1 of ordinary size nothing else is in play. TINY_LADDER moves both ends, (2^-e, 2^e), the same ratios:
    there h1 ≈ W1·x·2^-e of the small samples is tiny, and the exp2 activation's ABSOLUTE error of ≈ 3e-8 near 0 (mlp_x3.hpp) is 1e-5 of an h1
    of 2^-8 and 3e-2 of one of 2^-20 — every flavour with that activation, the bf16x3 and f32 MFMA ones included, misses dW2 from e = 8 on by the
    same amount, while the oracle (tanh_fast, accurate relative to |x|) stays at 1e-6 and wide_tanh_rational = 1 is the control."""
    B = NT * K
    big = big_mask(b)
    b["obs"] = (b["obs"] * np.where(big, big_mag, small)[None, :]).astype(np.float32)
    adv = b["adv"].astype(np.float64)
    # |A| >= 1 on minibatches whose mean is ≈ 0: the sign of the normalised advantage is the sign of A
    adv[big] = np.sign(adv[big] + 1e-30) * (1.0 + np.abs(adv[big]))
    for mb in range(4):
        idx = b["perm"][mb * M:(mb + 1) * M]
        adv[idx] -= adv[idx].mean()
    b["adv"] = adv.astype(np.float32)
    assert np.abs(b["adv"][big]).min() > 0.5
    nlp = O.logprob_actions(cfgo, params, b["obs"], b["action"])[0].astype(np.float64)
    lp = b["logprob"].astype(np.float64)
    # ratio = e (> 1 + clip) where the advantage is positive, 1/e (< 1 − clip) where it is negative: the clipped branch wins, d/dθ = 0
    lp[big] = nlp[big] - np.sign(b["adv"][big])
    b["logprob"] = lp.astype(np.float32)
    _set_return_errors(cfgo, params, b, np.where(big, 0.0, 3.0 * rng.standard_normal(B)))
    v = O.get_action(cfgo, params, b["obs"], np.zeros(B))[2]
    assert np.array_equal(b["ret"][big], v[big])
    b["value"] = np.where(big, v + np.float32(1.0), v).astype(np.float32)


@functools.lru_cache(maxsize=None)
def forward_inputs(case, D, A, n, nt=NT, k=16):
    """(cfgo, params, obs (D, n), u (n,)) for the forward consumers: the case's parameters with the actor head x 10 (logits spread: every
    action occurs and the log-probabilities depend on h2), and unit-normal observations under the case's magnitudes."""
    cfgo, _ = config(case, D, A, nt, k)
    params = params_of(case, cfgo)
    off = O.param_offsets(cfgo)
    params[off[A_W3]:off[A_W3 + 1]] *= 10
    rng = np.random.default_rng(1000 + n)
    # per-feature magnitudes top out at 1e2 here, not 1e3: the forward bars are per sample, and with 33 features up to 1e3 the float32 oracle's
    # own values are 9.8e-6 from float64 (the kernels: 1.2e-5, bf16x3 control included)
    obs = scale_obs(case, rng, rng.standard_normal((D, n)).astype(np.float32), top=2)
    if case == "obs*1e6":
        obs = saturated(rng, cfgo, params, obs)
    return cfgo, params, np.asfortranarray(obs), rng.random(n)


def forward64(cfgo, params, obs):
    """float64 numpy forward with the reference's rational tanh_fast (as oraclelib.torch_loss): log-probabilities (A, n) and values (n,)."""
    off = O.param_offsets(cfgo)
    q = params.astype(np.float64)
    h, d, A = cfgo.hidden, cfgo.obs_dim, cfgo.n_act

    def tanh_fast(x):
        x2 = x * x
        n = 1.0 + x2 * (0.1346604 + x2 * (0.0035974074 + x2 * (2.2332108e-5 + x2 * 1.587199e-8)))
        dd = 1.0 + x2 * (0.4679937 + x2 * (0.026262015 + x2 * (0.0003453992 + x2 * 8.7767893e-7)))
        return np.where(x2 < 66.0, x * (n / dd), np.sign(x))

    def net(base, n_out):
        W1 = q[off[base]:off[base + 1]].reshape(d, h).T
        W2 = q[off[base + 2]:off[base + 3]].reshape(h, h).T
        W3 = q[off[base + 4]:off[base + 5]].reshape(h, n_out).T
        h1 = tanh_fast(W1 @ obs.astype(np.float64) + q[off[base + 1]:off[base + 2], None])
        h2 = tanh_fast(W2 @ h1 + q[off[base + 3]:off[base + 4], None])
        return W3 @ h2 + q[off[base + 5]:off[base + 6], None]

    z = net(0, A)
    z = z - z.max(axis=0, keepdims=True)
    lp = z - np.log(np.exp(z).sum(axis=0, keepdims=True))
    return lp, net(6, 1)[0]


def sample64(lp, u):
    """The sampler on float64 probabilities: the first action whose cumulative probability reaches u."""
    c = np.cumsum(np.exp(lp), axis=0)
    return np.minimum((c < u[None, :]).sum(axis=0), lp.shape[0] - 1).astype(np.int32)
