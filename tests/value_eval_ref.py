"""Float64 restatement of crl_dqn_evaluate / crl_a2c_evaluate as include/cleanrl_hip.h defines them: the yardstick of tests/test_value_eval_cpu.py,
tests/test_gpu_dqn_eval.py and tests/test_gpu_a2c_eval.py. Written from the header's definition — not from the kernels — on top of what the tests
already have: the C oracle's CartPole step and forwards (a2c_cartpole_step, dqn_forward, a2c_forward, loaded through oraclelib) and the Philox
restatement of tests/ddpg_ref.py.

Env e of n, episode j of E: s[i] = 0.1·u53(Philox(seed, i, j·n + e, 0x20)) − 0.05, t = 0. Per step obs = s; DQN: action = q[1] > q[0]; A2C greedy:
z[1] > z[0]; A2C sample: p0 = e0 / (e0 + e1) <= u53(Philox(seed, e, r, 0x21)), r = the env's step count across its episodes. v0 on an episode's first
step: q[action] (DQN) or the critic's value (A2C). done = CartPole step; rew = 0 on the terminating step, else 1; ret += rew; disc_ret += disc·rew;
disc = disc·gamma; length += 1. Arrays are (E, n); the trace is (E·(max_steps + 1), n), −1 after the env's quota."""
import ctypes as C

import numpy as np

import ddpg_ref as R
import oraclelib as O

S_RESET, S_DRAW = 0x20, 0x21
GREEDY, SAMPLE = 0, 1
DQN, A2C = "dqn", "a2c"
A2C_ACTOR = 4 * 64 + 64 + 64 * 64 + 64 + 2 * 64 + 2        # floats of the actor in the flat A2C parameter vector; the critic follows
A2C_P = A2C_ACTOR + 4 * 64 + 64 + 64 * 64 + 64 + 64 + 1
SAMPLE_SEEDS = (0xA2C1, 0xA2C2)      # the sample-mode seeds of tests/test_gpu_a2c_eval.py; tests/test_value_eval_cpu.py shows that the reference
SAMPLE_CASE = dict(n=5, E=2, max_steps=40, gamma=0.97)      # has no decision within that test's tolerance for them
_ready = False
_cfg = None


def _lib():
    """the oracle library with this file's own ctypes signatures for the three functions it calls"""
    global _ready, _cfg
    L = O.lib()
    if not _ready:
        dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.a2c_cartpole_step.restype = None; L.a2c_cartpole_step.argtypes = [dp, ip, C.c_int32, C.c_int32, ip]
        L.dqn_forward.restype = None; L.dqn_forward.argtypes = [fp, dp, dp]
        L.a2c_forward.restype = None; L.a2c_forward.argtypes = [C.POINTER(O.A2CConfigC), fp, C.c_int, dp, dp]
        _cfg = O.a2c_config()
        _ready = True
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def reset(seed, gstep):
    """env_reset64 at the evaluation stream: four draws in [−0.05, 0.05)"""
    return 0.1 * R.uniform(seed, np.arange(4), gstep, S_RESET) - 0.05


def draw(seed, e, r):
    return float(R.uniform(seed, np.array([e]), r, S_DRAW)[0])


def step(s, t, action, max_steps):
    """the oracle's CartPoleEnv{Float64} step, in place on s → (t', done)"""
    tt, done = C.c_int32(t), C.c_int32(0)
    _lib().a2c_cartpole_step(_dp(s), C.byref(tt), int(action), int(max_steps), C.byref(done))
    return tt.value, bool(done.value)


def q_values(params, obs):
    q = np.zeros(2)
    _lib().dqn_forward(params.ctypes.data_as(C.POINTER(C.c_float)), _dp(obs), _dp(q))
    return q


def a2c_forward(params, net, obs):
    out = np.zeros(1 if net else 2)
    L = _lib()
    L.a2c_forward(C.byref(_cfg), params.ctypes.data_as(C.POINTER(C.c_float)), int(net), _dp(obs), _dp(out))
    return out


def softmax_p0(z):
    """a2c_collect_kernel's expressions"""
    z0, z1 = np.float64(z[0]), np.float64(z[1])
    m = z1 if z1 > z0 else z0
    e0, e1 = np.exp(z0 - m), np.exp(z1 - m)
    return e0 / (e0 + e1)


def evaluate(kind, params, n, E, seed, max_steps, gamma, mode=GREEDY, actions=None):
    """→ dict(returns, disc_returns, v0 (E, n) float64; lengths (E, n) int32; trace_action (E·(max_steps + 1), n) int32, −1 after the quota; obs
    (rows, n, 4): the observation each action answers; first (E, n): the trace row of each episode's first step; p0 / draws (rows, n): the sampler's
    probability and draw (SAMPLE only, NaN elsewhere)). The action of a step is the reference's own (actions=None) or actions[r, e]: a device trace
    replayed through the reference's env; p0, draws and v0 are the reference's for the replayed observations either way (DQN's v0 is q[the action
    used])."""
    params = np.ascontiguousarray(params, np.float32)
    gamma = np.float64(gamma)
    rows = E * (max_steps + 1)
    out = dict(returns=np.zeros((E, n)), disc_returns=np.zeros((E, n)), v0=np.zeros((E, n)), lengths=np.zeros((E, n), np.int32),
               trace_action=np.full((rows, n), -1, np.int32), obs=np.zeros((rows, n, 4)), first=np.zeros((E, n), np.int64),
               p0=np.full((rows, n), np.nan), draws=np.full((rows, n), np.nan))
    for e in range(n):
        r = 0
        for j in range(E):
            s = np.ascontiguousarray(reset(seed, j * n + e))
            t, length, ret, disc_ret, disc = 0, 0, np.float64(0.0), np.float64(0.0), np.float64(1.0)
            out["first"][j, e] = r
            while True:
                obs = s.copy()
                z = q_values(params, obs) if kind == DQN else a2c_forward(params, 0, obs)
                if mode == GREEDY:
                    a = 1 if z[1] > z[0] else 0
                else:
                    assert kind == A2C, "DQN has no sampling policy"
                    p0, u = softmax_p0(z), draw(seed, e, r)
                    out["p0"][r, e] = p0; out["draws"][r, e] = u
                    a = 1 if p0 <= u else 0
                if actions is not None:
                    a = int(actions[r, e])
                    assert a in (0, 1), f"row {r} of env {e} lies inside its quota and must hold an action, got {a}"
                if length == 0:
                    out["v0"][j, e] = z[a] if kind == DQN else a2c_forward(params, 1, obs)[0]
                out["trace_action"][r, e] = a; out["obs"][r, e] = obs
                r += 1
                t, done = step(s, t, a, max_steps)
                rew = np.float64(0.0 if done else 1.0)
                ret = ret + rew
                disc_ret = disc_ret + disc * rew
                disc = disc * gamma
                length += 1
                if done:
                    break
            out["returns"][j, e] = ret; out["disc_returns"][j, e] = disc_ret; out["lengths"][j, e] = length
        if actions is not None:
            assert (np.asarray(actions)[r:, e] == -1).all(), f"env {e}: rows after its quota must hold -1"
    return out


def report(returns, lengths, disc_returns, v0, prefix="v"):
    """crl_value_eval_report from the per-episode arrays: sequential Float64 sums in array order (env fastest), population standard deviation.
    prefix="q" names the last two fields q0_mean / q_bias_mean, as the Python mirror does for DQN."""
    ret, disc, v = (np.asarray(x, np.float64).reshape(-1) for x in (returns, disc_returns, v0))
    ln = np.asarray(lengths).reshape(-1)
    n = np.float64(ret.size)
    rsum = dsum = vsum = bsum = lsum = np.float64(0.0)
    for i in range(ret.size):
        rsum = rsum + ret[i]; dsum = dsum + disc[i]; vsum = vsum + v[i]; bsum = bsum + (v[i] - disc[i]); lsum = lsum + np.float64(ln[i])
    mean = rsum / n
    var = np.float64(0.0)
    for i in range(ret.size):
        d = ret[i] - mean
        var = var + d * d
    return {"episodes": int(ret.size), "env_steps": int(ln.astype(np.int64).sum()), "return_mean": float(mean), "return_std": float(np.sqrt(var / n)),
            "return_min": float(ret.min()), "return_max": float(ret.max()), "length_mean": float(lsum / n), "disc_return_mean": float(dsum / n),
            f"{prefix}0_mean": float(vsum / n), f"{prefix}_bias_mean": float(bsum / n)}


# ---------------------------------------------------------------------------------------------------- hand-made nets
# Flux.params order, (out, in) column-major: W[i, k] sits at i + out·k.
BALANCE = (0.1, 0.2, 1.0, 0.5)      # c = 0.1·x + 0.2·ẋ + θ + 0.5·θ̇


def dqn_balancer():
    """A Q-net whose argmax is a fixed function of the state, led by the pole's angle: c = θ + θ̇/2 + x/10 + ẋ/5; h1 = (relu(c), relu(−c)), passed
    on by layer 2, q = (h2[1], h2[0]) — action 1 (push right) exactly when c > 0. The angle alone lets the pole fall after 25–60 steps; with the
    damping terms the bang-bang rule keeps pole and cart in range, so every episode runs into the step limit, at max_steps 200 and 500 alike
    (pinned by tests/test_value_eval_cpu.py)."""
    p = np.zeros(O.DQN_P, np.float32)
    W1, W2, W3 = (p[O.DQN_OFF[i]:O.DQN_OFF[i + 1]] for i in (0, 2, 4))
    for k, c in enumerate(BALANCE):
        W1[0 + 120 * k] = c; W1[1 + 120 * k] = -c
    W2[0 + 84 * 0] = 1.0; W2[1 + 84 * 1] = 1.0
    W3[1 + 2 * 0] = 1.0; W3[0 + 2 * 1] = 1.0
    return p


def dqn_constant():
    """A Q-net that always prefers action 1 (b3 = (0, 1), every weight zero): the pole falls over after a few steps."""
    p = np.zeros(O.DQN_P, np.float32)
    p[O.DQN_OFF[5] + 1] = 1.0
    return p


def _a2c_parts(p):
    o = np.cumsum([0, 256, 64, 4096, 64, 128, 2, 256, 64, 4096, 64, 64, 1])
    return [p[o[i]:o[i + 1]] for i in range(12)]


def _a2c_critic(parts):
    """V = 0.5 + tanh_fast(tanh_fast(θ/4)): small pre-activations, so tanh_fast stays on its polynomial branch (x² < 0.017) and the value has no exp
    in it — the device's and the oracle's agree bit for bit."""
    parts[6][0 + 64 * 2] = 0.25; parts[8][0] = 1.0; parts[10][0] = 1.0; parts[11][0] = 0.5


def a2c_balancer():
    """An actor whose argmax is the same function c of the state: unit 0 carries tanh_fast(c/16) through both hidden layers, z = (−h, h). |c/16|
    stays below 0.13, tanh_fast's polynomial branch: no exp anywhere, logits bit-equal on the device and in the oracle."""
    p = np.zeros(A2C_P, np.float32)
    parts = _a2c_parts(p)
    for k, c in enumerate(BALANCE):
        parts[0][0 + 64 * k] = c / 16
    parts[2][0] = 1.0
    parts[4][0 + 2 * 0] = -1.0; parts[4][1 + 2 * 0] = 1.0
    _a2c_critic(parts)
    return p


def a2c_constant():
    """An actor that always prefers action 1 (b3 = (0, 1), every weight zero)."""
    p = np.zeros(A2C_P, np.float32)
    parts = _a2c_parts(p)
    parts[5][1] = 1.0
    _a2c_critic(parts)
    return p


# ---------------------------------------------------------------------------------------------------- random nets
def dqn_perturbed(seed):
    """perturbed glorot Q-net with non-zero biases, as tests/test_gpu_dqn.py makes"""
    return O.dqn_params(seed) + (0.05 * np.random.default_rng(seed).standard_normal(O.DQN_P)).astype(np.float32)


def a2c_perturbed(seed):
    """tests/test_gpu_a2c.py's parameters (orthogonal, a head that is not 50/50), perturbed so that every bias is non-zero"""
    pc = O.make_config()
    p = O.orthogonal_params(pc, seed)
    off = O.param_offsets(pc)
    p[off[4]:off[5]] *= 20
    return p + (0.05 * np.random.default_rng(seed).standard_normal(p.size)).astype(np.float32)
