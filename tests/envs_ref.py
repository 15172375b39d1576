"""numpy restatement of the MountainCar and Acrobot contracts (RLEnvs 0.6.12 / Gym MountainCar-v0 / Acrobot-v1 as recalled: parity unpinned).

Written from the contract text, not from the HIP code, and importing nothing of the package. Every function is vectorised over envs and takes
the dtype to evaluate in: np.float64 is the reference the GPU tests compare against, np.float32 is the same restatement at the kernels'
precision — its distance from the Float64 evaluation is what the tolerances of tests/test_gpu_envs.py are measured from.

Common rules: actions are 0-based, the command is a - 1; t counts steps since reset; done = goal || t >= MAX_STEPS; reward = done ? 0 : -1.
"""
import numpy as np

MAX_STEPS = 200

# ---------------------------------------------------------------------------------------------------- MountainCar
MC_MIN_X, MC_MAX_X, MC_MAX_V, MC_GOAL_X, MC_GOAL_V = -1.2, 0.6, 0.07, 0.5, 0.0


def mountaincar_step(state, t, action, dtype=np.float64):
    """state (2, n) = (x, v). Returns (state', t', reward, done, goal_margin) — goal_margin: Float distance of x from the goal line."""
    f = dtype
    x, v = np.asarray(state[0], f).copy(), np.asarray(state[1], f).copy()
    cmd = (np.asarray(action) - 1).astype(f)
    v = v + (cmd * f(0.001) + np.cos(f(3) * x) * f(-0.0025))
    v = np.clip(v, f(-MC_MAX_V), f(MC_MAX_V))
    x = x + v
    x = np.clip(x, f(MC_MIN_X), f(MC_MAX_X))
    v = np.where((x == f(MC_MIN_X)) & (v < 0), f(0), v)
    t2 = np.asarray(t) + 1
    goal = (x >= f(MC_GOAL_X)) & (v >= f(MC_GOAL_V))
    done = goal | (t2 >= MAX_STEPS)
    reward = np.where(done, f(0), f(-1))
    return np.stack([x, v]).astype(f), t2, reward, done, (x - f(MC_GOAL_X)).astype(f)


def mountaincar_obs(state, dtype=np.float64):
    return np.asarray(state, dtype)[:2].copy()


def mountaincar_reset(u, dtype=np.float32):
    """u (4, n): the 24-bit uniforms of the env's Philox words (x, y, z, w); only the first is used."""
    f = dtype
    u = np.asarray(u, f)
    return np.stack([f(0.2) * u[0] - f(0.6), np.zeros_like(u[0])]).astype(f)


# ---------------------------------------------------------------------------------------------------- Acrobot
AC_DT, AC_G = 0.2, 9.8
AC_MAX_W1, AC_MAX_W2 = 4 * np.pi, 9 * np.pi


def _acrobot_dsdt(y, tau, f):
    m1 = m2 = l1 = I1 = I2 = f(1)
    lc1 = lc2 = f(0.5)
    g = f(AC_G)
    th1, th2, w1, w2 = y
    hpi = f(np.pi / 2)
    d1 = m1 * lc1 * lc1 + m2 * (l1 * l1 + lc2 * lc2 + f(2) * l1 * lc2 * np.cos(th2)) + I1 + I2
    d2 = m2 * (lc2 * lc2 + l1 * lc2 * np.cos(th2)) + I2
    phi2 = m2 * lc2 * g * np.cos(th1 + th2 - hpi)
    phi1 = -m2 * l1 * lc2 * w2 * w2 * np.sin(th2) - f(2) * m2 * l1 * lc2 * w2 * w1 * np.sin(th2) + (m1 * lc1 + m2 * l1) * g * np.cos(th1 - hpi) + phi2
    dw2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 * w1 * np.sin(th2) - phi2) / (m2 * lc2 * lc2 + I2 - d2 * d2 / d1)
    dw1 = -(d2 * dw2 + phi1) / d1
    return np.stack([w1, w2, dw1, dw2]).astype(f)


def wrap_pi(x, dtype=np.float64):
    """into [-pi, pi)"""
    f = dtype
    x = np.asarray(x, f)
    pi, two_pi = f(np.pi), f(2 * np.pi)
    x = x - two_pi * np.floor((x + pi) / two_pi)
    x = np.where(x >= pi, x - two_pi, x)
    x = np.where(x < -pi, x + two_pi, x)
    return x.astype(f)


def acrobot_step(state, t, action, dtype=np.float64):
    """state (4, n) = (th1, th2, w1, w2). Returns (state', t', reward, done, goal_margin) — goal_margin = -cos th1 - cos(th1 + th2) - 1."""
    f = dtype
    s = np.asarray(state, f).copy()
    tau = (np.asarray(action) - 1).astype(f)
    dt = f(AC_DT)
    k1 = _acrobot_dsdt(s, tau, f)
    k2 = _acrobot_dsdt(s + dt / f(2) * k1, tau, f)
    k3 = _acrobot_dsdt(s + dt / f(2) * k2, tau, f)
    k4 = _acrobot_dsdt(s + dt * k3, tau, f)
    y = s + dt / f(6) * (k1 + f(2) * k2 + f(2) * k3 + k4)
    th1, th2 = wrap_pi(y[0], f), wrap_pi(y[1], f)
    w1 = np.clip(y[2], f(-AC_MAX_W1), f(AC_MAX_W1))
    w2 = np.clip(y[3], f(-AC_MAX_W2), f(AC_MAX_W2))
    t2 = np.asarray(t) + 1
    margin = -np.cos(th1) - np.cos(th1 + th2) - f(1)
    goal = margin > 0
    done = goal | (t2 >= MAX_STEPS)
    reward = np.where(done, f(0), f(-1))
    return np.stack([th1, th2, w1, w2]).astype(f), t2, reward, done, margin.astype(f)


def acrobot_obs(state, dtype=np.float64):
    s = np.asarray(state, dtype)
    return np.stack([np.cos(s[0]), np.sin(s[0]), np.cos(s[1]), np.sin(s[1]), s[2], s[3]]).astype(dtype)


def acrobot_reset(u, dtype=np.float32):
    f = dtype
    u = np.asarray(u, f)
    return (f(0.2) * u[:4] - f(0.1)).astype(f)


def acrobot_energy(state):
    """Total mechanical energy (Float64) of the two-link pendulum of the "book" model; conserved under tau = 0."""
    th1, th2, w1, w2 = np.asarray(state, np.float64)
    m1 = m2 = l1 = I1 = I2 = 1.0
    lc1 = lc2 = 0.5
    d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * np.cos(th2)) + I1 + I2
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * np.cos(th2)) + I2
    d22 = m2 * lc2 ** 2 + I2
    kinetic = 0.5 * d1 * w1 ** 2 + d2 * w1 * w2 + 0.5 * d22 * w2 ** 2
    potential = -(m1 * lc1 + m2 * l1) * AC_G * np.cos(th1) - m2 * lc2 * AC_G * np.cos(th1 + th2)
    return kinetic + potential


ENVS = {
    "mountaincar": dict(kind=3, obs_dim=2, n_act=3, n_state=2, step=mountaincar_step, obs=mountaincar_obs, reset=mountaincar_reset),
    "acrobot": dict(kind=4, obs_dim=6, n_act=3, n_state=4, step=acrobot_step, obs=acrobot_obs, reset=acrobot_reset),
}


def uniforms24(words):
    """Philox words (…, 4) uint32 -> the 24-bit uniforms (4, …) as exact float32."""
    w = np.asarray(words, np.uint32)
    return np.moveaxis((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24), -1, 0)


# ---------------------------------------------------------------------------------------------------- the single-step test grid
def state_grid(name, n=4096, seed=0):
    """At least n states covering the env's state box (angles in [-pi, pi), velocities to their limits; MountainCar x at both walls and around the
    goal line), each with t drawn from {0, …, MAX_STEPS - 2} ∪ {MAX_STEPS - 1} (the last forces the time limit)."""
    rng = np.random.default_rng(seed)
    if name == "mountaincar":
        x = rng.uniform(MC_MIN_X, MC_MAX_X, n); v = rng.uniform(-MC_MAX_V, MC_MAX_V, n)
        x[:64] = MC_MIN_X; x[64:128] = MC_MAX_X                      # both walls
        x[128:512] = rng.uniform(0.40, 0.56, 384)                    # around the goal line x = 0.5
        v[:32] = -MC_MAX_V; v[64:96] = MC_MAX_V
        x[512:640] = rng.uniform(MC_MIN_X, MC_MIN_X + 0.07, 128); v[512:640] = -np.abs(v[512:640])   # runs into the left wall
        s = np.stack([x, v])
    else:
        th = rng.uniform(-np.pi, np.pi, (2, n))
        w1 = rng.uniform(-AC_MAX_W1, AC_MAX_W1, n); w2 = rng.uniform(-AC_MAX_W2, AC_MAX_W2, n)
        th[:, :32] = -np.pi; th[0, 32:64] = np.nextafter(np.float32(np.pi), np.float32(0))   # the wrap edges
        w1[64:96] = AC_MAX_W1; w1[96:128] = -AC_MAX_W1; w2[128:160] = AC_MAX_W2; w2[160:192] = -AC_MAX_W2   # the velocity limits
        th[0, 192:704] = rng.uniform(2.0, np.pi, 512) * rng.choice([-1, 1], 512)             # upper half: around the goal boundary
        w1[192:704] = rng.uniform(-2, 2, 512); w2[192:704] = rng.uniform(-2, 2, 512)
        s = np.stack([th[0], th[1], w1, w2])
    t = rng.integers(0, MAX_STEPS - 1, n)
    t[::16] = MAX_STEPS - 1
    return s.astype(np.float32), t.astype(np.int32)
