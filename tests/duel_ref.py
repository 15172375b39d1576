"""Float64 numpy restatement of the dueling heads as include/cleanrl_hip.h pins them (the "Dueling heads" block), scalar (R = 1) and categorical
(R = n_atoms): the yardstick of tests/test_duel_cpu.py and tests/test_gpu_duel.py. Written from the header — not from the kernels.

It builds on tests/dqn_per_ref.py, tests/dqn_target_ref.py and tests/c51_ref.py by import and edits none of them: env, ring, samplers, tree, n-step
walk, the target, softmax, projection and cross-entropy are theirs. Restated here: the ten-array layout, the two-stream forward with the combine, and
its backward pass. DuelScalar runs dqn_target_ref.DQNTarget's `update` and DuelC51 runs c51_ref.C51's with the network functions those look up
(`forward`, `loss_grads`) replaced for the duration of the call; the loop is c51_ref.C51.run, whose greedy action goes through `q_values`.

The lines a mutant replaces are small module-level functions (tests/duel_bar.py)."""
import contextlib

import numpy as np

import c51_ref as Z
import ddpg_ref as R
import dqn_per_ref as P
import dqn_target_ref as T

FIXED = 20928                                  # the R-independent part: W1 b1 W2v b2v W2a b2a


def sizes(Rr):
    """W1 b1 W2v b2v W3v b3v W2a b2a W3a b3a"""
    return [480, 120, 10080, 84, 84 * Rr, Rr, 10080, 84, 84 * 2 * Rr, 2 * Rr]


def shapes(Rr):
    return ((120, 4), (120,), (84, 120), (84,), (Rr, 84), (Rr,), (84, 120), (84,), (2 * Rr, 84), (2 * Rr,))


def param_count(Rr):
    return FIXED + 255 * Rr


def split(p, Rr):
    """flat float32 → the ten arrays as float64, each (out, in) column-major"""
    out, o = [], 0
    for n, shape in zip(sizes(Rr), shapes(Rr)):
        out.append(np.asarray(p[o:o + n], np.float32).astype(np.float64).reshape(shape, order="F")); o += n
    return out


# ---------------------------------------------------------------------------------------------------- hooks the mutants replace
def centre(A):
    """A (2, R, k) → A − mean over the two ACTIONS, mean_i = (A_0i + A_1i) · 0.5"""
    return A - ((A[0] + A[1]) * 0.5)[None]


def value_input(h2v, h2a):
    return h2v


def d_value(g):
    return g


def d_adv_other(half):
    return -half


def d1_streams(W2v, W2a):
    """the matrices that carry d2v and d2a back to h1, in that order"""
    return W2v, W2a


# ---------------------------------------------------------------------------------------------------- forward, backward
def forward(p, Rr, X):
    """X (4, k) → (h1 (120, k), h2v (84, k), h2a (84, k), V (R, k), A (2, R, k), out (2, R, k))"""
    W1, b1, W2v, b2v, W3v, b3v, W2a, b2a, W3a, b3a = split(p, Rr)
    h1 = P.relu(R.dense(W1, b1, X))
    h2v = P.relu(R.dense(W2v, b2v, h1)); h2a = P.relu(R.dense(W2a, b2a, h1))
    V = R.dense(W3v, b3v, value_input(h2v, h2a))
    A = R.dense(W3a, b3a, h2a).reshape(2, Rr, -1)
    return h1, h2v, h2a, V, A, V[None] + centre(A)


def backward(p, Rr, X, a, g, fwd):
    """g (R, k): the cotangent on out[a_b, :, b] → the flat float64 gradient before the float32 projection"""
    k = a.size
    h1, h2v, h2a = fwd[:3]
    W1, b1, W2v, b2v, W3v, b3v, W2a, b2a, W3a, b3a = split(p, Rr)
    dV = d_value(g)
    half = g * 0.5
    dA = np.where(np.arange(2)[:, None, None] == a[None, None, :], half[None], d_adv_other(half)[None]).reshape(2 * Rr, k)
    t2v = np.zeros((84, k))
    for i in range(Rr):
        t2v += W3v[i, :][:, None] * dV[i][None, :]
    d2v = np.where(h2v > 0.0, t2v, 0.0)
    t2a = np.zeros((84, k))
    for row in range(2 * Rr):
        t2a += W3a[row, :][:, None] * dA[row][None, :]
    d2a = np.where(h2a > 0.0, t2a, 0.0)
    Bv, Ba = d1_streams(W2v, W2a)
    t1 = np.zeros((120, k))
    for j in range(84):
        t1 += Bv[j, :][:, None] * d2v[j:j + 1, :]
    for j in range(84):
        t1 += Ba[j, :][:, None] * d2a[j:j + 1, :]
    d1 = np.where(h1 > 0.0, t1, 0.0)
    gs = [np.zeros(s) for s in shapes(Rr)]
    for b in range(k):                                   # every sum over the samples in sample order
        gs[0] += d1[:, b][:, None] * X[:, b][None, :]; gs[1] += d1[:, b]
        gs[2] += d2v[:, b][:, None] * h1[:, b][None, :]; gs[3] += d2v[:, b]
        gs[4] += dV[:, b][:, None] * h2v[:, b][None, :]; gs[5] += dV[:, b]
        gs[6] += d2a[:, b][:, None] * h1[:, b][None, :]; gs[7] += d2a[:, b]
        gs[8] += dA[:, b][:, None] * h2a[:, b][None, :]; gs[9] += dA[:, b]
    return R._flat(gs)


def _mean_in_order(v, k):
    s = np.float64(0.0)
    for b in range(k):
        s = s + v[b]
    return s / np.float64(k)


def scalar_forward(p, X):
    """what dqn_per_ref.forward returns, from the dueling net: (h1, (h2v, h2a), q (2, k))"""
    f = forward(p, 1, X)
    return f[0], (f[1], f[2]), f[5][:, 0, :]


def scalar_loss_grads(qp, state, a, td, w):
    """dqn_target_ref.loss_grads on the dueling net: the importance-weighted mse against td → (loss, flat gradient, δ)"""
    k = td.size
    f = forward(qp, 1, state)
    diff = td - f[5][a, 0, np.arange(k)]
    loss = _mean_in_order(w * (diff * diff), k)
    return loss, backward(qp, 1, state, a, P.cotangent(w, diff, k)[None, :], f), diff


def c51_forward(p, N, X):
    """what c51_ref.forward returns, from the dueling net: (h1, (h2v, h2a), logits (2, N, k))"""
    f = forward(p, N, X)
    return f[0], (f[1], f[2]), f[5]


def c51_loss_grads(qp, N, state, a, m, w):
    """c51_ref.loss_grads on the dueling net: the cross-entropy against m → (loss, flat gradient, loss_j)"""
    k = a.size
    f = forward(qp, N, state)
    p, logp = Z.softmax(f[5][Z.taken(a), :, np.arange(k)].T)
    loss_j = -Z.sum_atoms(m * logp)
    return _mean_in_order(w * loss_j, k), backward(qp, N, state, a, Z.cotangent(w, p, m, k), f), loss_j


# ---------------------------------------------------------------------------------------------------- the loop
@contextlib.contextmanager
def replaced(mod, **attrs):
    saved = {n: getattr(mod, n) for n in attrs}
    try:
        for n, v in attrs.items():
            setattr(mod, n, v)
        yield
    finally:
        for n, v in saved.items():
            setattr(mod, n, v)


class Adam(R.Adam):
    """ddpg_ref.Adam with one β-power pair for each of the ten arrays"""

    def __init__(self, n, sizes_, lr):
        super().__init__(n, sizes_[:6], lr)
        self.arr = np.repeat(np.arange(len(sizes_)), sizes_); self.bp = np.tile(np.array([R.B1, R.B2]), (len(sizes_), 1))


class DuelScalar(T.DQNTarget):
    """cfg, per (None = uniform), tgt as dqn_target_ref.DQNTarget; params: the flat float32 net of param_count(1) = 21183 numbers"""
    R = 1

    def __init__(self, cfg, per, tgt, params):
        super().__init__(cfg, per, tgt, params)
        assert self.q.size == param_count(1)
        self.opt = Adam(param_count(1), sizes(1), cfg.lr)
        self.greedy, self.seen = [], []                   # as c51_ref.C51: what the tie condition compares

    def q_values(self, obs):
        return scalar_forward(self.q, np.asarray(obs, np.float64).reshape(4, -1, order="F"))[2]

    def streams(self, obs):
        f = forward(self.q, self.R, np.asarray(obs, np.float64).reshape(4, -1, order="F"))
        return dict(value=f[3], adv=np.moveaxis(f[4], 0, 1))          # (R, n), (R, 2, n)

    def update(self):
        with replaced(P, forward=scalar_forward), replaced(T, loss_grads=scalar_loss_grads):
            super().update()
        self.seen.append((self.global_step, self.idx.copy(), self.astar.copy(), self.leaves.copy()))

    run = Z.C51.run


class DuelC51(Z.C51):
    """cfg, per, tgt, c51 as c51_ref.C51; params: the flat float32 net of param_count(n_atoms) numbers"""

    def __init__(self, cfg, per, tgt, c51, params):
        with replaced(Z, param_count=param_count, sizes=lambda N: sizes(N)[:6]):   # its six-array Adam is replaced below
            super().__init__(cfg, per, tgt, c51, params)
        self.R = self.N
        self.opt = Adam(param_count(self.N), sizes(self.N), cfg.lr)

    def logits(self, obs):
        return forward(self.q, self.N, np.asarray(obs, np.float64).reshape(4, -1, order="F"))[5]

    def q_values(self, obs):
        return Z.q_of(self.logits(obs), self.z)

    def probs(self, obs):
        l3 = self.logits(obs)
        return np.stack([Z.softmax(l3[a])[0] for a in range(2)], axis=1)          # (N, 2, n)

    streams = DuelScalar.streams

    def update(self):
        with replaced(Z, forward=c51_forward, loss_grads=c51_loss_grads):
            super().update()


def make(cfg, per, tgt, c51, params):
    return DuelScalar(cfg, per, tgt, params) if c51 is None else DuelC51(cfg, per, tgt, c51, params)
