"""Shared by test_optim_cpu.py (oracle only) and test_gpu_optim.py (HIP library): the routes, step schedules, synthetic rollout buffers
and input preconditions that pin every implementation of Optimiser(ClipNorm(0.5), Adam(η)) to orc_clipnorm_adam bit for bit.

A case is a route (shape + options that select one optimiser kernel) and a schedule (per optimiser step: how large the critic's and
the actor's gradients are made, and η). The buffer of a step is a pure function of (route, seed, step, current parameters), so the CPU
replay and the GPU run write the same inputs; the GPU's gradients differ from the oracle's by ~1e-5, which is why every norm is kept
outside [0.45, 0.55]."""
import numpy as np

import oraclelib as O

THRESH = 0.5
BAND = (0.45, 0.55)
F32_MIN_NORMAL = np.float32(1.1754944e-38)


class Route:
    def __init__(self, name, D, A, H, clipv, options=None, wide=False, comm=False, fused=False, seed=1, ent_coeff=0.01, clip_coef=0.2):
        self.name, self.D, self.A, self.H, self.clipv = name, D, A, H, clipv
        self.options, self.wide, self.comm, self.fused, self.seed = dict(options or {}), wide, comm, fused, seed
        self.ent_coeff, self.clip_coef = ent_coeff, clip_coef
        # the reference's own default batch (ppo.jl:1-19): 4 envs x 32 steps, 4 minibatches of 32 samples — accepted by every path
        self.nt, self.k, self.nmb = 4, 32, 4
        self.M = self.nt * self.k // self.nmb

    def ocfg(self):
        return O.make_config(num_envs=self.nt, num_steps=self.k, num_minibatches=self.nmb, clip_value_loss=self.clipv, obs_dim=self.D,
                             n_act=self.A, hidden=self.H, env_kind=1 if self.wide else 0, ent_coeff=self.ent_coeff, clip_coef=self.clip_coef)

    @property
    def P(self):
        D, A, H = self.D, self.A, self.H
        return 2 * (H * D + H + H * H + H) + A * H + A + H + 1


# seeds: chosen on the CPU with orc_loss_grad standing in for the kernels; test_optim_cpu.py replays every schedule and asserts the conditions
# (seed 1 met them on every route; a seed that stops doing so fails there with a message that says so)
ROUTES = {r.name: r for r in (
    Route("block", 4, 2, 64, True, seed=1),                                                 # 1: clipnorm_adam_kernel, 12 blocks
    Route("fused,gemm=2", 4, 2, 64, False, {"gemm": 2}, fused=True, seed=1),                # 2: reduce_optim_kernel
    Route("fused,gemm=1", 4, 2, 64, False, {"gemm": 1}, fused=True, seed=1),
    Route("block,layerwise", 5, 3, 64, True, wide=True, seed=1),                            # 3: clipnorm_adam_kernel behind wide_update
    Route("slices,128", 4, 2, 128, True, wide=True, seed=1),                                # 4: clipnorm_partial + adam_slice
    Route("slices,256,wide_gemm=2", 17, 5, 256, True, {"wide_gemm": 2}, wide=True, seed=1),  # 5
    Route("slices,256,wide_gemm=0", 17, 5, 256, True, {"wide_gemm": 0}, wide=True, seed=1),
    Route("block,stats", 4, 2, 64, False, {"comm_force": 1, "fuse_optim": 0}, comm=True, seed=1),   # 6: the same kernel, 13 blocks
    Route("two-launch", 4, 2, 64, False, {"fuse_optim": 0}, seed=1),                        # cross-route partner of "fused,gemm=2"
)}

# (critic, actor, eta): "big" drives every array of that network over 0.55, "small" under 0.45 (see step_buffer)
SCHEDULE = [("big", "big", 2.5e-4), ("small", "big", 1e-3), ("small", "small", 2.5e-4), ("big", "small", 0.0),
            ("big", "big", 3e-3), ("small", "small", 1e-4), ("big", "small", 2.5e-4), ("small", "big", 5e-4)]
EDGE_STEPS = [("big", "small", 2.5e-4), ("small", "big", 1e-3), ("big", "big", 2.5e-4)]
EDGES = ("late", "early", "eps", "dead")
EDGE_ROUTES = ("block", "fused,gemm=2", "slices,256,wide_gemm=2")
LATE_N = 20000


def base_params(route):
    """Flux.orthogonal-shaped start with the actor's head at gain 0.5 instead of 0.01: the actor's hidden layers then see a cotangent of the
    head's size, so the same levers move all six actor arrays across the threshold."""
    cfg = route.ocfg()
    p = O.orthogonal_params(cfg, 100 + route.seed)
    off = O.param_offsets(cfg)
    p[off[4]:off[5]] *= 50
    return p


def critic_values(route, params, obs):
    """critic(obs) under `params` (oracle forward pass): what `small` critic steps use as stored values and as returns."""
    n = route.nt * route.k
    _, _, v, _ = O.get_action(route.ocfg(), params, obs.reshape(route.D, n, order="F"), np.full(n, 0.5))
    return v.reshape((route.nt, route.k), order="F")


def policy_logprobs(route, params, obs, action):
    """log π(action | obs) under `params` (oracle forward pass)."""
    lp, _ = O.logprob_actions(route.ocfg(), params, obs.reshape(route.D, -1, order="F"), action.ravel(order="F"))
    return lp.reshape((route.nt, route.k), order="F")


def step_buffer(route, step, spec, params, zero_obs=None):
    """The rollout buffer of one step: dict of CRL_F_* name → array. Levers (all inputs):
    critic: stored values = critic(obs) under the current parameters (so the value clip never cuts the gradient); `big`: returns = those
    + 10·(1 + N(0,1)) → every critic array's norm ≫ 0.5 (the common offset drives the biases); `small`: returns = those + 1e-3·N(0,1) → ≪ 0.5.
    actor: advantages are negative for action 0 and positive for the others, so the samples pull one way; `big`: stored log-probabilities
    3.5 below the policy's → ratio ≈ e^3.5 on the samples whose unclipped term wins (Â < 0); `small`: 3 above → ratio ≈ e^-3: the unclipped
    term wins where Â > 0 and carries the factor e^-3, the clipped one has no gradient.
    zero_obs: that observation feature is identically zero (the ε-dominated edge)."""
    critic, actor, _ = spec
    nt, k, D, A = route.nt, route.k, route.D, route.A
    rng = np.random.default_rng([route.seed, step])
    buf = {}
    buf["obs"] = rng.standard_normal((D, nt, k)).astype(np.float32)
    if zero_obs is not None:
        buf["obs"][zero_obs] = 0.0
    buf["action"] = rng.integers(0, A, (nt, k)).astype(np.int32)
    off = -3.5 if actor == "big" else 3.0
    lp = policy_logprobs(route, params, buf["obs"], buf["action"]).astype(np.float64)
    buf["logprob"] = (lp + off + 0.1 * rng.standard_normal((nt, k))).astype(np.float32)
    buf["advantage"] = (np.where(buf["action"] == 0, -1.0, 1.0) * (0.5 + np.abs(2 * rng.standard_normal((nt, k))))).astype(np.float32)
    noise_r = rng.standard_normal((nt, k))
    v = critic_values(route, params, buf["obs"]).astype(np.float64)
    buf["value"] = v.astype(np.float32)
    buf["ret"] = (v + (10.0 * (1.0 + noise_r) if critic == "big" else 1e-3 * noise_r)).astype(np.float32)
    buf["perm"] = rng.permutation(nt * k).astype(np.int32)
    return buf


def oracle_grad(route, params, buf, mb):
    """orc_loss_grad of minibatch `mb` of the buffer: the CPU stand-in for the update kernels."""
    M = route.M
    g, _ = O.loss_grad(route.ocfg(), params, buf["obs"].reshape(route.D, -1, order="F"), buf["action"], buf["logprob"], buf["value"],
                       buf["advantage"], buf["ret"], buf["perm"][mb * M:(mb + 1) * M])
    return g


# ---- preconditions on the gradient the optimiser consumed -------------------------------------------------------------------------
def array_norms(route, g):
    """Per array: (Float64 √Σg², the Float32 norm the kernels clip by, clipped?)."""
    off = O.param_offsets(route.ocfg())
    out = []
    for a in range(12):
        x = g[off[a]:off[a + 1]].astype(np.float64)
        r = float(np.sqrt(np.sum(x * x)))
        out.append((r, np.float32(r), bool(float(np.float32(r)) > THRESH)))
    return out


def midpoint_distance(r):
    """Relative distance of the Float64 norm r from the nearest midpoint of two adjacent Float32 values: the routes add Σg² in different
    orders (n terms: within n·2⁻⁵² relative), so their Float32 norms can differ only if r lies that close to such a midpoint."""
    f = np.float32(r)
    up, dn = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    m1, m2 = (float(f) + float(up)) / 2, (float(f) + float(dn)) / 2
    return min(abs(r - m1), abs(r - m2)) / r


def check_step_inputs(route, g, step, where):
    """Preconditions ON THE INPUT (not tolerances): every non-zero norm outside [0.45, 0.55]; every clipped array's norm further from a Float32
    rounding midpoint than (array length)·2⁻⁵². Returns the clip flags of the 12 arrays."""
    off = O.param_offsets(route.ocfg())
    flags = []
    for a, (r, f, clipped) in enumerate(array_norms(route, g)):
        assert not (BAND[0] <= r <= BAND[1]), f"{where} input precondition: step {step} array {a} has norm {r:.6f} inside [0.45, 0.55] — pick another seed"
        if clipped:
            n = int(off[a + 1] - off[a])
            d = midpoint_distance(r)
            assert d > n * 2.0 ** -52, (f"{where} input precondition: step {step} array {a} norm {r!r} lies {d:.3e} (relative) from a Float32 rounding "
                                        f"midpoint, inside the {n}·2^-52 summation-order window — pick another seed")
        flags.append(clipped)
    return flags


def check_schedule(flags, where):
    """The three crossing conditions over a whole sequence; flags[s][a] = array a clipped in step s."""
    F = np.asarray(flags, bool)
    assert any(row.any() and not row.all() for row in F), f"{where}: no step has both a clipped and an unclipped array"
    for a in range(12):
        assert F[:, a].any() and not F[:, a].all(), f"{where}: array {a} is {'always' if F[:, a].all() else 'never'} clipped over the sequence"
    down = (F[:-1] & ~F[1:]).any(); up = (~F[:-1] & F[1:]).any()
    assert down and up, f"{where}: no array goes clipped → unclipped ({down}) and none the other way ({up}) between consecutive steps"


# ---- optimiser state of the edges --------------------------------------------------------------------------------------------------
DEAD_OBS = 1   # the observation feature that is identically zero in the ε-dominated edge


def dead_input_entries(route):
    """Flat indices of column DEAD_OBS of both networks' W1 (H x D, column-major): with that feature identically zero their gradient is exactly
    zero at every step, whatever the parameters — the entries of a dead input."""
    off = O.param_offsets(route.ocfg())
    H = route.H
    return np.concatenate([np.arange(off[b] + DEAD_OBS * H, off[b] + (DEAD_OBS + 1) * H) for b in (0, 6)]).astype(np.int64)


def edge_state(route, edge):
    """(params, m, v, betap, info) at the start of a state edge."""
    P = route.P
    rng = np.random.default_rng([route.seed, 7, EDGES.index(edge)])
    params = base_params(route)
    m = np.zeros(P, np.float32); v = np.zeros(P, np.float32)
    betap = np.array([0.9, 0.999] * 12)
    info = {}
    if edge == "late":     # n = 20000 steps in: 0.9ⁿ underflows to 0 in Float64, 1 − 0.999ⁿ ≈ 1; state at realistic sizes
        betap = np.array([0.9 ** LATE_N, 0.999 ** LATE_N] * 12)
        assert betap[0] == 0.0 and 0.0 < betap[1] < 1e-8
        m = (1e-3 * rng.standard_normal(P)).astype(np.float32)
        v = (1e-6 * rng.standard_normal(P) ** 2 + 1e-9).astype(np.float32)
    elif edge == "eps":    # a dead input's entries: v subnormal or 0, |m| 1e-12 … 1e-6; everything else at realistic sizes
        idx = dead_input_entries(route)
        betap = np.array([0.9 ** 50, 0.999 ** 50] * 12)
        m = (1e-3 * rng.standard_normal(P)).astype(np.float32)
        v = (1e-6 * rng.standard_normal(P) ** 2 + 1e-9).astype(np.float32)
        sub = np.array([1e-40, 1e-41, 1e-42, 1e-43, 1e-44, 1e-45, 0.0]).astype(np.float32)
        assert all(0 < s < F32_MIN_NORMAL for s in sub[:-1])
        v[idx] = sub[np.arange(idx.size) % sub.size]
        m[idx] = (rng.choice([-1.0, 1.0], idx.size) * 10.0 ** rng.uniform(-12, -6, idx.size)).astype(np.float32)
        info["idx"] = idx; info["subnormal"] = idx[v[idx] != 0]; info["zero_obs"] = DEAD_OBS
    elif edge == "dead":
        params = np.zeros(P, np.float32)
    return params, m, v, betap, info


def first_mismatch(route, name, got, want, flags):
    """None, or the message the issue asks for: array, first differing flat index, clipped?, the two values (compared as bits)."""
    gb, wb = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(gb != wb)
    if bad.size == 0:
        return None
    i = int(bad[0])
    off = O.param_offsets(route.ocfg())
    a = int(np.searchsorted(off, i, side="right") - 1)
    return (f"{name}: {bad.size} entries differ; first at flat index {i} = array {a} (entries {off[a]}…{off[a + 1] - 1}, offset {i - off[a]} in it, "
            f"slice {(i - off[a]) // 4096}, 64-float chunk {i // 64}), array {'CLIPPED' if flags[a] else 'not clipped'}: "
            f"got {got[i]!r} (0x{gb[i]:08x}), oracle {want[i]!r} (0x{wb[i]:08x})")
