"""Float64 numpy restatement of the DQN loop with the quantile-regression critic as include/cleanrl_hip.h pins it (the "Quantile-regression DQN"
block): the yardstick of tests/test_qr_cpu.py and tests/test_gpu_qr.py. Written from the header — not from the kernels.

It builds on tests/c51_ref.py, tests/duel_ref.py and tests/noisy_ref.py by import and edits none of them. The head has the categorical head's shape,
so c51_ref.C51 gives the ring, both samplers, the n-step walk, Adam, `run` and the frame of `update`; for the duration of an update the functions that
frame looks up in c51_ref are replaced (duel_ref.replaced) by this file's: the value is the ascending mean of the quantile rows, "p'" is the a* row of
target_net(x) itself, the "projection" is the target T_j, and loss_grads is the pair loss with its cotangent. The dueling net swaps forward and
backward the same way; noisy_ref._Noisy is mixed in front as noisy_ref.make does. Every sum the header pins is an explicit ascending loop."""
import numpy as np

import c51_ref as Z
import ddpg_ref as R
import duel_ref as D
import noisy_ref as NZ


def taus(N):
    return (np.arange(N).astype(np.float64) + 0.5) / np.float64(N)


def value(th3):
    """quantile rows (2, N, k) → Q (2, k): (Σ_i θ_i, ascending from 0.0) / N"""
    return np.stack([Z.sum_atoms(th3[a]) for a in range(2)]) / np.float64(th3.shape[1])


def targets(theta_next, R_, disc, term):
    """θ' rows (N, k) → T (N, k)"""
    return R_ + ((disc * theta_next) * (1.0 - np.asarray(term).astype(np.float64)))


def pair(theta, T, kappa):
    """theta, T (N, k) → (loss_s (k,), G (N, k)); row i of the sums walks j ascending"""
    N = theta.shape[0]
    kappa = np.float64(kappa)
    tau = taus(N)[:, None]
    sh, G = np.zeros(theta.shape), np.zeros(theta.shape)
    for j in range(N):
        u = T[j][None, :] - theta
        au = np.abs(u)
        h = np.where(au <= kappa, (0.5 * u) * u, kappa * (au - 0.5 * kappa))
        c = np.where(au <= kappa, u, np.where(u < 0.0, -kappa, kappa))
        wt = np.abs(tau - np.where(u < 0.0, 1.0, 0.0))
        sh = sh + (wt * h) / kappa
        G = G + wt * c
    return Z.sum_atoms(sh / np.float64(N)), G


def dtheta(G, kappa):
    """the cotangent of loss_s on θ: (−(G_i / κ)) / N"""
    return (-(G / np.float64(kappa))) / np.float64(G.shape[0])


def plain_backward(qp, N, state, a, dl, fwd):
    """dl (N, k) on the taken action's rows → the flat float64 gradient of the six arrays: c51_ref.loss_grads' pullback, restated for a given dl"""
    k = a.size
    h1, h2 = fwd[0], fwd[1]
    W1, b1, W2, b2, W3, b3 = Z.split(qp, N)
    t2 = np.zeros((84, k))
    for i in range(N):
        t2 += W3[a * N + i, :].T * dl[i][None, :]
    d2 = np.where(h2 > 0.0, t2, 0.0)
    t1 = np.zeros((120, k))
    for j in range(84):
        t1 += W2[j, :][:, None] * d2[j:j + 1, :]
    d1 = np.where(h1 > 0.0, t1, 0.0)
    gs = [np.zeros(s) for s in ((120, 4), (120,), (84, 120), (84,), (2 * N, 84), (2 * N,))]
    for b in range(k):                                   # sample order; the other action's rows get an exact 0.0
        gs[0] += d1[:, b][:, None] * state[:, b][None, :]; gs[1] += d1[:, b]
        gs[2] += d2[:, b][:, None] * h1[:, b][None, :]; gs[3] += d2[:, b]
        r = slice(a[b] * N, (a[b] + 1) * N)
        gs[4][r, :] += dl[:, b][:, None] * h2[:, b][None, :]; gs[5][r] += dl[:, b]
    return R._flat(gs)


class QR(Z.C51):
    """cfg, per, tgt as c51_ref.C51; qr: dict(n_quantiles, kappa); params: the flat float32 net of c51_ref.param_count(n_quantiles) numbers.
    After an update `proj` holds the targets T (N, k) and `sample_loss` the loss_s."""
    net_forward = staticmethod(lambda p, N, X, f=Z.forward: f(p, N, X) + (None,))   # → (h1, h2, rows (2, N, k), what backward needs); c51_ref's own
                                                                                    # forward, bound now: `update` replaces the module's name
    net_backward = staticmethod(plain_backward)

    def __init__(self, cfg, per, tgt, qr, params):
        super().__init__(cfg, per, tgt, dict(n_atoms=int(qr["n_quantiles"]), v_min=0.0, v_max=1.0), params)   # the support is never read
        self.kappa = np.float64(qr["kappa"])

    def quantiles(self, obs):
        th = self.net_forward(self.q, self.N, np.asarray(obs, np.float64).reshape(4, -1, order="F"))[2]
        return np.moveaxis(th, 0, 1)                                                # (N, 2, n)

    def q_values(self, obs):
        return value(np.moveaxis(self.quantiles(obs), 1, 0))

    def _loss_grads(self, qp, N, state, a, T, w):
        k = a.size
        f = self.net_forward(qp, N, state)
        loss_s, G = pair(f[2][a, :, np.arange(k)].T, T, self.kappa)
        dl = ((np.asarray(w)[None, :] * (-(G / self.kappa))) / np.float64(N)) / np.float64(k)
        return D._mean_in_order(w * loss_s, k), self.net_backward(qp, N, state, a, dl, f if f[3] is None else f[3]), loss_s

    def update(self):
        with D.replaced(Z, forward=lambda p, N, X: self.net_forward(p, N, X)[:3], q_of=lambda l3, z: value(l3), softmax=lambda l: (l, None),
                        project=lambda th, R_, disc, term, c51: targets(th, R_, disc, term), loss_grads=self._loss_grads):
            super().update()


class DuelQR(QR):
    """QR on the dueling net of duel_ref: rows combine as the categorical logits do, R = N"""
    net_forward = staticmethod(lambda p, N, X: (lambda f: (f[0], (f[1], f[2]), f[5], f))(D.forward(p, N, X)))
    net_backward = staticmethod(D.backward)

    def __init__(self, cfg, per, tgt, qr, params):
        with D.replaced(Z, param_count=D.param_count, sizes=lambda N: D.sizes(N)[:6]):   # its six-array Adam is replaced below
            super().__init__(cfg, per, tgt, qr, params)
        self.R = self.N
        self.opt = D.Adam(D.param_count(self.N), D.sizes(self.N), cfg.lr)

    streams = D.DuelScalar.streams


def make(cfg, per, tgt, qr, dueling, params, noisy=False, tape=None):
    """the restatement of a crl_dqn_qr_create handle; noisy: params are 2P float32 (mu, sigma) and tape the device's {(gen, net): xi table} or None"""
    base = DuelQR if dueling else QR
    tgt = {"n_step": 1, "double_q": 0} if tgt is None else tgt
    if not noisy:
        return base(cfg, per, tgt, qr, params)
    lay = NZ.layers(dueling, qr["n_quantiles"])

    class Noisy(NZ._Noisy, base):
        pass
    agent = Noisy(cfg, per, tgt, qr, np.asarray(params, np.float32)[:NZ.param_count(lay)])
    agent._noisy_init(lay, params, tape)
    return agent
