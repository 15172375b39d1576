"""Float64 numpy restatement of the Gaussian PPO handle (the crl_ppo_create_gaussian block of include/cleanrl_hip.h): the yardstick of
tests/test_ppo_gauss_cpu.py and tests/test_gpu_ppo_gauss.py. Written from the header — not from the kernels.

Conventions. Parameters are one flat float32 vector in Flux.params(actor, critic) order (W1 b1 W2 b2 W3 b3 per network, each W (out, in) column-major);
the actor head has 2 act_dim rows, z = (mu, s). Activations are true tanh. Every function takes `dt` (np.float64 by default): run with np.float32 it
gives the spread the GPU tests' bars are measured from (scripts/ppo_gauss_bar.py)."""
import numpy as np

from ddpg_ref import philox_env, _u53

STREAM0, S_RESET, S_RESET0 = 0x20, 1, 2
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


def offsets(D, ad, H):
    sizes = [H * D, H, H * H, H, 2 * ad * H, 2 * ad, H * D, H, H * H, H, H, 1]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def unpack(params, D, ad, H, dt=np.float64):
    off, p = offsets(D, ad, H), np.asarray(params, dt)
    shapes = [(H, D), (H,), (H, H), (H,), (2 * ad, H), (2 * ad,), (H, D), (H,), (H, H), (H,), (1, H), (1,)]
    arr = [p[off[i]:off[i + 1]].reshape(s, order="F") for i, s in enumerate(shapes)]
    return arr[:6], arr[6:]


def mlp(net, X):
    """Forward of one network over columns of X: (head output, h1, h2)."""
    W1, b1, W2, b2, W3, b3 = net
    h1 = np.tanh(W1 @ X + b1[:, None]); h2 = np.tanh(W2 @ h1 + b2[:, None])
    return W3 @ h2 + b3[:, None], h1, h2


def mlp_backward(net, X, h1, h2, dout):
    """Gradients of sum(dout * out) w.r.t. the six arrays, flattened column-major in parameter order."""
    W1, b1, W2, b2, W3, b3 = net
    d2 = (W3.T @ dout) * (1.0 - h2 * h2); d1 = (W2.T @ d2) * (1.0 - h1 * h1)
    return [(d1 @ X.T), d1.sum(1), (d2 @ h1.T), d2.sum(1), (dout @ h2.T), dout.sum(1)]


def log_std(s, lo, hi):
    return lo + 0.5 * (hi - lo) * (np.tanh(s) + 1.0)


def logprob_entropy(z, a, ad, lo, hi):
    """z (2 ad, n), a (ad, n) -> (logpi[n], H[n], xi (ad, n), log_std (ad, n))."""
    ls = log_std(z[ad:2 * ad], lo, hi)
    xi = (a - z[:ad]) / np.exp(ls)
    return (-0.5 * xi * xi - ls - HALF_LOG_2PI).sum(0), (ls + 0.5 + HALF_LOG_2PI).sum(0), xi, ls


def act(z, xi, ad, lo, hi):
    ls = log_std(z[ad:2 * ad], lo, hi)
    return z[:ad] + np.exp(ls) * xi, (-0.5 * xi * xi - ls - HALF_LOG_2PI).sum(0)


def rollout_xi(seed, gids, gstep, ad):
    """The pinned stream: xi_i = Box–Muller over all four words of block (seed, env id, gstep, 0x20 + i), rounded to float32."""
    out = np.zeros((ad, len(gids)))
    for i in range(ad):
        x, y, z, w = philox_env(seed, gids, gstep, STREAM0 + i)
        out[i] = np.sqrt(-2.0 * np.log(1.0 - _u53(x, y))) * np.cos(6.283185307179586 * _u53(z, w))
    return out.astype(np.float32)


def minibatch_loss(params, D, ad, H, lo, hi, obs, a, old_lp, old_v, adv, ret, hp, dt=np.float64, want_grad=True):
    """Loss, statistics and gradient of one minibatch (columns already gathered). hp: clip, ent_coeff, v_coef, clip_vloss.
    Returns (loss terms dict, flat gradient or None, per-sample diagnostics dict)."""
    actor, critic = unpack(params, D, ad, H, dt)
    X = np.asarray(obs, dt); a = np.asarray(a, dt)
    M = X.shape[1]
    z, h1a, h2a = mlp(actor, X); vv, h1c, h2c = mlp(critic, X); v = vv[0]
    lp, Hs, xi, ls = logprob_entropy(z, a, ad, dt(lo), dt(hi))
    adv = np.asarray(adv, np.float32)
    mean_f, std_f = np.float32(adv.astype(np.float64).mean()), np.float32(adv.astype(np.float64).std(ddof=1))
    Ahat = (adv - mean_f).astype(dt) / (dt(std_f) + dt(1e-8))
    clip = dt(hp["clip"])
    ratio = np.exp(lp - np.asarray(old_lp, dt)); rc = np.clip(ratio, 1 - clip, 1 + clip)
    pg1, pg2 = -Ahat * ratio, -Ahat * rc
    first = pg1 > pg2
    inside = (ratio >= 1 - clip) & (ratio <= 1 + clip)
    pg = np.where(first, pg1, pg2)
    dlp = np.where(first | inside, pg1, 0.0) / M            # d loss / d logpi
    R, ov = np.asarray(ret, dt), np.asarray(old_v, dt)
    if hp["clip_vloss"]:
        u = (v - R * R).mean()
        dvv = v - ov; vc = ov + np.clip(dvv, -clip, clip); q = (vc - R) ** 2
        qw = ~(u > q)
        term = np.where(qw, q, u)
        inner = np.where(qw & (dvv >= -clip) & (dvv <= clip), 2.0 * (vc - R), 0.0)
        dv = hp["v_coef"] * 0.5 / M * ((~qw).sum() / M + inner)
    else:
        u = (v - R * R).mean(); term = (v - R) ** 2; dv = hp["v_coef"] * 0.5 / M * 2.0 * (v - R)
    terms = dict(pg_loss=pg.mean(), entropy_loss=Hs.mean(), v_loss=0.5 * term.mean(), u_value=u)
    terms["loss"] = terms["pg_loss"] - hp["ent_coeff"] * terms["entropy_loss"] + hp["v_coef"] * terms["v_loss"]
    diag = dict(ratio=ratio, Ahat=Ahat, s=z[ad:2 * ad], first=first, inside=inside)
    if not want_grad:
        return terms, None, diag
    th = np.tanh(z[ad:2 * ad])
    dz = np.zeros_like(z)
    dz[:ad] = dlp * xi / np.exp(ls)
    dz[ad:2 * ad] = (dlp * (xi * xi - 1.0) - hp["ent_coeff"] / M) * 0.5 * (hi - lo) * (1.0 - th * th)
    ga = mlp_backward(actor, X, h1a, h2a, dz); gc = mlp_backward(critic, X, h1c, h2c, dv[None, :])
    return terms, np.concatenate([np.asarray(g).reshape(-1, order="F") for g in ga + gc]), diag


# ---------------------------------------------------------------- Pendulum
def pendulum_reset(seed, gids, gstep, stream, dt=np.float64):
    x, y, _, _ = philox_env(seed, gids, gstep, stream)
    ux = (x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24); uy = (y >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (dt(2 * np.pi) * ux.astype(dt) - dt(np.pi)), (dt(2.0) * uy.astype(dt) - dt(1.0))


def pendulum_step(th, thd, a, dt=np.float64):
    """One step of every env: (theta, thetadot, reward). The caller counts steps (done after 200) and resets."""
    th, thd = np.asarray(th, dt), np.asarray(thd, dt)
    u = np.clip(np.asarray(a, dt), dt(-2), dt(2))
    cost = th * th + dt(0.1) * (thd * thd) + dt(0.001) * (u * u)
    nthd = np.clip(thd + (dt(15) * np.sin(th) + dt(3) * u) * dt(0.05), dt(-8), dt(8))
    nth = th + nthd * dt(0.05)
    pi = dt(np.pi)
    nth = np.where(nth >= pi, nth - dt(2) * pi, np.where(nth < -pi, nth + dt(2) * pi, nth))
    return nth.astype(dt), nthd.astype(dt), -cost


def pendulum_obs(th, thd):
    return np.stack([np.cos(th), np.sin(th), thd])


# ---------------------------------------------------------------- inputs shared by tests/test_gpu_ppo_gauss.py and scripts/ppo_gauss_bar.py
PEND_ENVS, PEND_STEPS, PEND_SEED = 6, 600, 0x5EED
# log-std bounds of the GPU tests' handles: s near 0 gives sigma = 1. logpi and its cotangents depend on mu through (a - mu)/sigma, so every Float32 rounding
# of the forward's mu reaches them divided by sigma: with the library's defaults (-5, 2: sigma = 0.22 at s = 0) the shared layer-wise forward's ~1e-6
# absolute error on z alone puts the actor gradient 4e-6 .. 8e-6 from Float64 (measured, every wide_gemm / wide_tanh_rational flavour alike, the critic
# arrays at 3e-7 beside them) — the conditioning of the inputs, not of a kernel. The tests keep the discrete path's bars and choose sigma = 1.
LO, HI = -2.0, 2.0


def spread_params(lib, D, ad, Hd, seed, lo=LO, hi=HI):
    """The library's initial networks plus noise; the bias of s row 0 at 4.5, so that s_0 lies beyond +4 (tanh saturated, sigma at its upper bound)."""
    from cleanrl_jl_amd import GaussianOptions
    rng = np.random.default_rng(seed)
    p = lib.make_actor_critic_gaussian_host(D, ad, Hd, GaussianOptions(lo, hi, 0.0), seed=seed)
    p = p + (0.05 * rng.standard_normal(p.size)).astype(np.float32)
    p[offsets(D, ad, Hd)[5] + ad] = 4.5
    return p.astype(np.float32)


def pendulum_actions():
    """(steps, envs) torques for 3 episodes: beyond ±2 (clipped), a constant push that drives thetadot to ±8, and free swinging across ±pi."""
    rng = np.random.default_rng(11)
    a = (3.0 * rng.standard_normal((PEND_STEPS, PEND_ENVS))).astype(np.float32)
    a[:, 0] = 2.5; a[:, 1] = -2.5; a[:, 2] = 0.0
    return a


def pendulum_trajectory(dt=np.float64):
    """The stale_obs = 0 trajectory of PEND_ENVS envs under pendulum_actions(): (obs (steps, 3, envs), reward, done, theta, thetadot)."""
    gids, acts = np.arange(PEND_ENVS), pendulum_actions()
    th, thd = pendulum_reset(PEND_SEED, gids, 0, S_RESET0, dt)
    t = np.zeros(PEND_ENVS, int)
    out = dict(obs=[], reward=[], done=[], th=[], thd=[])
    for g in range(PEND_STEPS):
        th, thd, rew = pendulum_step(th, thd, acts[g], dt)
        t += 1
        done = t >= 200
        if done.any():
            rth, rthd = pendulum_reset(PEND_SEED, gids, g, S_RESET, dt)
            th, thd, t = np.where(done, rth, th), np.where(done, rthd, thd), np.where(done, 0, t)
        for k, v in (("obs", pendulum_obs(th, thd)), ("reward", rew), ("done", done), ("th", th), ("thd", thd)):
            out[k].append(np.array(v))
    return {k: np.array(v) for k, v in out.items()}


ROLLOUT_CASES = [(3, 8, 256, "synthetic"), (1, 3, 64, "pendulum"), (8, 17, 128, "synthetic")]     # act_dim, obs_dim, hidden, env of the rollout test


def xi_case(lib, ad, D, Hd, kind, nt=96, k=5, seed=0x5EED):
    """Parameters, observations and normals of the rollout test: spread_params (seed 7), observations of its env's range (U(-1, 1)^D, or (cos, sin,
    thetadot) with |thetadot| <= 8; the device's own observations are not restated) and the pinned stream's xi for its envs and steps."""
    rng = np.random.default_rng(ad)
    obs = rng.uniform(-1, 1, (D, nt * k))
    if kind == "pendulum":
        th = rng.uniform(-np.pi, np.pi, nt * k); obs = np.stack([np.cos(th), np.sin(th), rng.uniform(-8, 8, nt * k)])
    xi = np.concatenate([rollout_xi(seed, np.arange(nt), g, ad) for g in range(k)], axis=1)
    return spread_params(lib, D, ad, Hd, 7), obs.astype(np.float32), xi


def recovered_xi(p, obs, xi, D, ad, Hd, lo, hi, dt):
    """What the rollout test recovers when forward and a = mu + sigma xi run in `dt`: the float32 action under the Float64 forward of the observation."""
    z = mlp(unpack(p, D, ad, Hd, dt)[0], obs.astype(dt))[0]
    a = (z[:ad] + np.exp(log_std(z[ad:], dt(lo), dt(hi))) * xi.astype(dt)).astype(np.float32).astype(np.float64)
    z64 = mlp(unpack(p, D, ad, Hd)[0], obs.astype(np.float64))[0]
    return (a - z64[:ad]) / np.exp(log_std(z64[ad:], lo, hi))
