"""Float64 numpy restatement of ONE training update of src/algorithms/a2c.jl as the library runs it (csrc/a2c.hip: a2c_forward_kernel, a2c_loss_kernel,
a2c_backward_kernel, a2c_wgrad_kernel, then ClipNorm + Adam): the yardstick of tests/test_a2c_bar_cpu.py and tests/test_gpu_a2c_edges.py. It is
written from a2c.jl:13-24,77-98 and from NNlib's tanh_fast, not from the C oracle: forward, discounted_future_rewards, both losses and the explicit
backward are numpy here; only Optimiser(ClipNorm(0.5), Adam(lr)) is the one every optimiser test of the suite is pinned to (tests/optimlib.py's
yardstick, oraclelib.clipnorm_adam), because the optimiser is checked bit for bit elsewhere and what this twin is for is everything in front of it.

Sums run in the order the kernels and the oracle use (products in input order, bias last; samples in sample order), so that two correct
implementations differ only where exp and log do. Those two are reached through the module's `np`: tests/a2c_bar.py replaces it for one run by
a numpy whose exp / log results are moved in their last bits, and replaces single functions of this module by one-line wrong versions."""
import numpy as np

import oraclelib as O

H, D, A = 64, 4, 2
SIZES = (H * D, H, H * H, H, A * H, A, H * D, H, H * H, H, H, 1)          # the PPO layout at 4 / 2 / 64: the actor's six arrays, then the critic's
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
P = int(OFF[-1])
CHUNK = 128


def tanh_fast64(x):
    """NNlib tanh_fast(x::Float64): (exp(2x) - 1) / (exp(2x) + 1), a polynomial in x² where x² < 0.017, sign(x) where x² > 900"""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x + x)
        y = (e - 1.0) / (e + 1.0)
    x2 = x * x
    p = np.full_like(x, -0.008697141630499953)
    for c in (0.02186660872609521, -0.05396823125794372, 0.13333333325511604, -0.33333333333324583, 1.0):
        p = p * x2 + c
    return np.where(x2 > 900.0, np.sign(x), np.where(x2 < 0.017, x * p, y))


def layers(params, net):
    """→ [(W (out, in) Float64, b (out,) Float64)] x 3 of the actor (net 0) or the critic (net 1); W is stored column-major"""
    base, n_out = (6, 1) if net else (0, A)
    out = []
    for i, (rows, cols) in enumerate(((H, D), (H, H), (n_out, H))):
        W = np.asarray(params[OFF[base + 2 * i]:OFF[base + 2 * i + 1]], np.float64).reshape((rows, cols), order="F")
        out.append((W, np.asarray(params[OFF[base + 2 * i + 1]:OFF[base + 2 * i + 2]], np.float64)))
    return out


def _dense(W, b, x):
    """W·x + b for x (in, n): products added in input order, the bias last"""
    acc = np.zeros((W.shape[0], x.shape[1]))
    for k in range(W.shape[1]):
        acc = acc + W[:, k, None] * x[None, k, :]
    return acc + b[:, None]


def forward(params, net, x):
    """x (4, n) → (out (n_out, n), h1 (64, n), h2 (64, n))"""
    (W1, b1), (W2, b2), (W3, b3) = layers(params, net)
    h1 = tanh_fast64(_dense(W1, b1, x))
    h2 = tanh_fast64(_dense(W2, b2, h1))
    return _dense(W3, b3, h2), h1, h2


def discounted_future_rewards(rewards, terminals, final_value, gamma):
    """a2c.jl:13-24"""
    n = len(rewards)
    G = np.zeros(n)
    nxt = 0.0 if terminals[n - 1] else rewards[n - 1] + gamma * final_value
    G[n - 1] = nxt
    for j in range(n - 2, -1, -1):
        nxt = 0.0 if terminals[j] else rewards[j] + gamma * nxt
        G[j] = nxt
    return G


def _sum_seq(x):
    """the last axis summed front to back"""
    return np.add.accumulate(np.asarray(x, np.float64), axis=-1)[..., -1]


def _sum_samples(f, n, shape):
    """Σ_b f(b0, b1)[..., b] front to back, f evaluated on chunks of samples"""
    acc = np.zeros(shape)
    for b0 in range(0, n, CHUNK):
        acc = _sum_seq(np.concatenate([acc[..., None], f(b0, min(n, b0 + CHUNK))], axis=-1))
    return acc


def final_value(params, final_state, reset_state=None):
    """critic(state(env))[1] on the terminal, not yet reset state (a2c.jl:78); reset_state is what a wrong implementation would read"""
    return float(forward(params, 1, np.asarray(final_state, np.float64)[:, None])[0][0, 0])


def critic_loss(params, states, G):
    """a2c.jl:82-86 → (loss, advantage, dL/dv, h1, h2)"""
    v, h1, h2 = forward(params, 1, states)
    adv = G - v[0]
    n = len(G)
    return _sum_seq(adv * adv) / n, adv, (-2.0 * adv / n)[None, :], h1, h2


def softmax_cotangent(p, actions, k):
    """d(Σ_b k_b · log p[a_b, b]) / dz: k · (onehot(a) − p)"""
    onehot = (np.arange(A)[:, None] == actions[None, :]).astype(np.float64)
    return k[None, :] * (onehot - p)


def actor_loss(params, states, actions, adv):
    """a2c.jl:91-96 with the advantage a captured constant → (loss, dL/dz, h1, h2)"""
    z, h1, h2 = forward(params, 0, states)
    m = np.maximum(z[0], z[1])
    e = np.exp(z - m[None, :])
    p = e / (e[0] + e[1])[None, :]
    n = len(adv)
    lp = np.log(p[actions, np.arange(n)])
    return -(_sum_seq(lp * adv) / n), softmax_cotangent(p, actions, -adv / n), h1, h2


def dtanh(h, layer):
    """tanh' from the stored activation of hidden layer 1 or 2"""
    return 1.0 - h * h


def backward(params, net, states, dout, h1, h2):
    """the six parameter gradients of one network, Float64, flat in the layout's order"""
    (W1, b1), (W2, b2), (W3, b3) = layers(params, net)
    n, n_out = states.shape[1], W3.shape[0]
    s = np.zeros((H, n))
    for q in range(n_out):
        s = s + W3[q, :, None] * dout[None, q, :]
    d2 = s * dtanh(h2, 2)
    s = np.zeros((H, n))
    for i in range(H):
        s = s + W2[i, :, None] * d2[None, i, :]
    d1 = s * dtanh(h1, 1)

    def outer(d, x):
        return _sum_samples(lambda b0, b1: d[:, None, b0:b1] * x[None, :, b0:b1], n, (d.shape[0], x.shape[0]))

    def bias(d):
        return _sum_samples(lambda b0, b1: d[:, b0:b1], n, (d.shape[0],))

    return np.concatenate([outer(d1, states).ravel(order="F"), bias(d1), outer(d2, h1).ravel(order="F"), bias(d2),
                           outer(dout, h2).ravel(order="F"), bias(dout)])


class A2C:
    """parameters and optimiser state; update() is a2c.jl:77-98 on one batch"""

    def __init__(self, params, lr, gamma):
        self.params = np.array(params, np.float32)
        assert self.params.size == P
        self.m = np.zeros(P, np.float32); self.v = np.zeros(P, np.float32)
        self.betap = np.array([0.9, 0.999] * 12)
        self.lr, self.gamma = float(lr), float(gamma)

    def update(self, states, actions, rewards, terminals, final_state, reset_state=None):
        """states (4, n) Float64, actions 0-based, final_state: the env after the batch's last step, before its reset (reset_state, the env after the
        reset, is what a wrong implementation would read) → {"critic_loss", "actor_loss", "grads" Float32, "params" Float32 after the step}"""
        states = np.asarray(states, np.float64); actions = np.asarray(actions, np.int64)
        fv = final_value(self.params, final_state, reset_state)
        G = discounted_future_rewards(np.asarray(rewards, np.float64), np.asarray(terminals), fv, self.gamma)
        cl, adv, dv, h1, h2 = critic_loss(self.params, states, G)
        gc = backward(self.params, 1, states, dv, h1, h2)
        al, dz, h1, h2 = actor_loss(self.params, states, actions, adv)
        ga = backward(self.params, 0, states, dz, h1, h2)
        grads = np.concatenate([ga, gc]).astype(np.float32)
        # both gradients are of the parameters before the step (the advantage is captured before the critic's), and the arrays are independent
        O.clipnorm_adam(O.make_config(obs_dim=D, n_act=A, hidden=H), self.params, grads.copy(), self.m, self.v, self.betap, self.lr)
        return dict(critic_loss=float(cl), actor_loss=float(al), grads=grads, params=self.params.copy())
