"""Float64 numpy restatement of crl_ddpg_evaluate as include/cleanrl_hip.h defines it, on top of tests/ddpg_ref.py (the Pendulum is restated there bit
for bit, the forwards to within 1e-10): the yardstick of tests/test_ddpg_eval_cpu.py and tests/test_gpu_ddpg_eval.py. Written from the header's
definition — not from the kernel.

Env e of n, episode j of E: (θ, θ̇) = the Pendulum reset draw at (key = seed, gstep = j·n + e, stream 0x16); per step obs = (cos θ, sin θ, θ̇),
a = the noise-free actor output, the Pendulum step gives r; ret += r; disc_ret += disc·r; disc = disc·gamma (Float64, step order, multiply then add);
q0 = Q(obs, a) on the first step; every episode has max_steps steps. Arrays are (E, n); the trace is (E·max_steps, n), row j·max_steps + t."""
import numpy as np

import ddpg_ref as R

S_EVAL = 0x16


def evaluate(actor, critic, n, E, seed, max_steps, gamma, actions=None):
    """→ dict(returns, disc_returns, q0 (E, n); trace_action, and obs (E·max_steps, n, 3) — the observation each action answers —, theta / theta_dot
    (E·max_steps, n) before each step, wrapped / clamped: how often θ wrapped and θ̇ hit ±8). The action of a step is the reference's own
    actor_mean (actions=None) or actions[j·max_steps + t, e]: a device trace replayed through the reference's Pendulum. q0 is the reference critic's
    value for (obs, the action used) and is None when critic is None."""
    gamma = np.float64(gamma)
    rows = E * max_steps
    out = dict(returns=np.zeros((E, n)), disc_returns=np.zeros((E, n)), q0=None if critic is None else np.zeros((E, n)),
               trace_action=np.zeros((rows, n)), obs=np.zeros((rows, n, 3)), theta=np.zeros((rows, n)), theta_dot=np.zeros((rows, n)),
               wrapped=0, clamped=0)
    for e in range(n):
        for j in range(E):
            th, thd = R.pendulum_reset(seed, j * n + e, S_EVAL)
            t, ret, disc_ret, disc = 0, np.float64(0.0), np.float64(0.0), np.float64(1.0)
            while True:
                row = j * max_steps + t
                obs = R.pendulum_obs(th, thd)
                a = np.float64(R.actor_mean(actor, 3, 1, obs)[0, 0] if actions is None else actions[row, e])
                if t == 0 and critic is not None:
                    out["q0"][j, e] = R.q_values(critic, 3, 1, obs, np.array([a]))[0]
                out["trace_action"][row, e] = a; out["obs"][row, e] = obs; out["theta"][row, e] = th; out["theta_dot"][row, e] = thd
                nth, nthd, t, r, term = R.pendulum_step(th, thd, t, a, max_steps)
                out["wrapped"] += int(abs(nth - (th + nthd * 0.05)) > 1.0)
                out["clamped"] += int(abs(nthd) == 8.0)
                th, thd = nth, nthd
                ret = ret + r
                disc_ret = disc_ret + disc * r
                disc = disc * gamma
                if term:
                    break
            assert t == max_steps
            out["returns"][j, e] = ret; out["disc_returns"][j, e] = disc_ret
    return out


def report(returns, disc_returns, q0, max_steps):
    """crl_ddpg_eval_report from the per-episode arrays: sequential Float64 sums in array order (env fastest), population standard deviation"""
    ret, disc, q = (np.asarray(x, np.float64).reshape(-1) for x in (returns, disc_returns, q0))
    n = np.float64(ret.size)
    rsum = dsum = qsum = bsum = np.float64(0.0)
    for i in range(ret.size):
        rsum = rsum + ret[i]; dsum = dsum + disc[i]; qsum = qsum + q[i]; bsum = bsum + (q[i] - disc[i])
    mean = rsum / n
    var = np.float64(0.0)
    for i in range(ret.size):
        d = ret[i] - mean
        var = var + d * d
    return dict(episodes=int(ret.size), env_steps=int(ret.size) * int(max_steps), return_mean=float(mean), return_std=float(np.sqrt(var / n)),
                return_min=float(ret.min()), return_max=float(ret.max()), disc_return_mean=float(dsum / n), q0_mean=float(qsum / n),
                q_bias_mean=float(bsum / n))


def hard_actor(scale=1e3, pump=1e6):
    """An actor that saturates and pumps energy into the Pendulum: glorot weights and biases times `scale`, and one path of weight `pump` from θ̇
    through unit 0 of both hidden layers to the head, so that the head's pre-activation is ≈ ±pump — far inside tanh_fast64's sign branch
    (x² > 900), the action exactly 2·sign(θ̇). A torque that always follows the velocity speeds the Pendulum up until θ̇ sits on its ±8 clamp and θ
    wraps again and again."""
    rng = np.random.default_rng(12)
    parts = []
    for rows, cols in ((64, 3), (64, 64), (1, 64)):
        lim = np.sqrt(6.0 / (rows + cols))
        parts += [(scale * rng.uniform(-lim, lim, rows * cols)).astype(np.float32), (scale * rng.uniform(-0.1, 0.1, rows)).astype(np.float32)]
    W1, b1, W2, b2, W3, b3 = parts
    W1[0 + 64 * 2] = pump; W2[0 + 64 * 0] = pump; W3[0] = pump            # (out, in) column-major: W1[0, 2], W2[0, 0], W3[0, 0]
    return np.concatenate(parts)


HARD = dict(n=2, E=1, seed=1, max_steps=200, gamma=0.99)     # pinned by tests/test_ddpg_eval_cpu.py: this rollout wraps θ and clamps θ̇
