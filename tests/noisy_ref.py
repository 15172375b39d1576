"""Numpy restatement of the noisy linear layers of include/cleanrl_hip.h ("Noisy linear layers" block; csrc/dqn_noisy.hpp, dqn_noisy_adam_step of
csrc/dqn_loops.hpp). It wraps the existing restatements — dqn_target_ref (scalar head), c51_ref, duel_ref, all imported and untouched — around the
effective image: their forward, loss and gradient functions run on w = mu + sigma·eps exactly as they run on a plain net, and this file adds what is
new: the noise table, eps, the image, the split of the gradient, the 2P-entry Adam, the target copy of mu and sigma, and the generation schedule.

xi comes from this file's own Box–Muller (ddpg_ref's Philox) or from an injected tape {(gen, net): float32 table}, e.g. the device's own, fetched per
generation through crl_dqn_noisy_noise. Every expression a one-line mutant replaces (tests/noisy_bar.py) is a module-level function here."""
import numpy as np

import c51_ref as Z
import ddpg_ref as R
import dqn_target_ref as T
import duel_ref as D

S_NOISY = (0x22, 0x23)                         # Philox stream words: q_net, target_net
F32 = np.float32


# ---------------------------------------------------------------------------------------------------- the table
def layers(dueling=False, n_atoms=None):
    """(in, out) of the dense layers in parameter-array order"""
    if dueling:
        Rr = 1 if not n_atoms else int(n_atoms)
        return ((4, 120), (120, 84), (84, Rr), (120, 84), (84, 2 * Rr))
    return ((4, 120), (120, 84), (84, 2 * int(n_atoms) if n_atoms else 2))


def n_xi(lay):
    return sum(i + o for i, o in lay)


def param_count(lay):
    return sum(o * (i + 1) for i, o in lay)


def array_sizes(lay):
    return [n for i, o in lay for n in (o * i, o)]


# ---------------------------------------------------------------------------------------------------- the noise
def _log(x):
    return np.log(x)


def _cos(x):
    return np.cos(x)


def normal(seed, comps, gen, stream):
    """ddpg_ref.normal with this module's log / cos, so that a test can nudge them"""
    x, y, z, w = R.philox_env(seed, comps, gen, stream)
    u1, u2 = R._u53(x, y), R._u53(z, w)
    return np.sqrt(-2.0 * _log(1.0 - u1)) * _cos(6.283185307179586 * u2)


def squash(z):
    """f(x) = sgn(x)·sqrt|x| in Float64"""
    return np.where(z < 0.0, -np.sqrt(np.abs(z)), np.sqrt(np.abs(z)))


def stream_of(net):
    return S_NOISY[net]


def xi_table(seed, lay, gen, net):
    """the whole table of one net and generation → float32 [n_xi]; component = position in the table"""
    return squash(normal(int(seed), np.arange(n_xi(lay)), int(gen), stream_of(net))).astype(F32)


def weight_eps(xo, xi):
    """eps of a layer's weights (out, in) = xi_out[i] * xi_in[j], a Float32 multiply"""
    return xo[:, None] * xi[None, :]


def bias_eps(xo, xi):
    return xo


def eps_of(lay, table):
    """float32 [P]: per layer the weights' eps flattened with the output index fastest, then the biases'"""
    table = np.asarray(table, F32)
    out, at = [], 0
    for i, o in lay:
        xi, xo = table[at:at + i], table[at + i:at + i + o]
        out += [np.asarray(weight_eps(xo, xi), F32).reshape(-1, order="F"), np.asarray(bias_eps(xo, xi), F32)]
        at += i + o
    return np.concatenate(out)


def image(mu, sigma, eps):
    """w = mu + sigma * eps: a Float32 multiply, then a Float32 add"""
    return (np.asarray(mu, F32) + (np.asarray(sigma, F32) * np.asarray(eps, F32)).astype(F32)).astype(F32)


def sigma_grad(g32, eps):
    """the gradient of sigma: (float)g * eps in Float32"""
    return (np.asarray(g32, F32) * np.asarray(eps, F32)).astype(F32)


def split_grad(g64, eps):
    """the effective-weight gradient (float64, before the Float32 projection) → the 2P-entry gradient Adam reads: g_mu = (float)g, g_sigma = g_mu * eps"""
    g32 = np.asarray(g64, np.float64).astype(F32)
    return np.concatenate([g32, sigma_grad(g32, eps)])


# ---------------------------------------------------------------------------------------------------- the schedule
def online_gen(n_updates):
    """the generation of the online image after n_updates completed updates"""
    return n_updates


def target_gen(n_updates, copied, previous):
    """the generation of the target image after n_updates completed updates: redrawn every update, whether or not a copy happened"""
    return n_updates


def greedy_image(agent):
    """what evaluation and crl_dqn_q_values read: the mu half, the noise off"""
    return agent.pq[:agent.P]


# ---------------------------------------------------------------------------------------------------- the loop
class _SplitOpt:
    """stands where the twin's restatement keeps its Adam: takes the effective-weight gradient, steps mu and sigma, leaves the image to the owner"""

    def __init__(self, owner):
        self.owner = owner

    def step(self, q, g64):
        o = self.owner
        o.pq = o.adam.step(o.pq, split_grad(g64, o.eps_q).astype(np.float64))
        return q


class _Noisy:
    """mixed in front of the twin's restatement (make below). params: 2P float32, mu then sigma; tape: None or {(gen, net): xi table}"""

    def _noisy_init(self, lay, params, tape):
        self.lay, self.tape = lay, tape
        self.P = param_count(lay)
        assert np.asarray(params).size == 2 * self.P
        self.pq = np.array(params, F32); self.pt = self.pq.copy()
        self.adam = D.Adam(2 * self.P, array_sizes(lay) * 2, self.c.lr)
        self.opt = _SplitOpt(self)
        self.gen_q = online_gen(0); self.gen_t = target_gen(0, True, None)
        self.gens = [(0, self.gen_q, self.gen_t)]          # (n_updates, online generation, target generation): the schedule as it ran
        self.rebuild()

    def xi(self, gen, net):
        if self.tape is not None:
            return np.asarray(self.tape[(int(gen), int(net))], F32)
        return xi_table(self.c.seed, self.lay, gen, net)

    def rebuild(self):
        """both images from mu, sigma and the two generations (crl_dqn_write_params does this at the current ones)"""
        P = self.P
        self.eps_q = eps_of(self.lay, self.xi(self.gen_q, 0)); self.eps_t = eps_of(self.lay, self.xi(self.gen_t, 1))
        self.q = image(self.pq[:P], self.pq[P:], self.eps_q); self.t = image(self.pt[:P], self.pt[P:], self.eps_t)

    def write_params(self, params):
        self.pq = np.array(params, F32); self.pt = self.pq.copy()
        self.rebuild()

    def update(self):
        super().update()                                   # forwards, target, loss, gradient on the images; _SplitOpt steps mu and sigma
        copied = self.global_step % self.c.target_net_freq == 0
        if copied:
            self.pt = self.pq.copy()
        self.gen_q = online_gen(self.n_updates); self.gen_t = target_gen(self.n_updates, copied, self.gen_t)
        self.gens.append((self.n_updates, self.gen_q, self.gen_t))
        self.rebuild()

    def greedy_q_values(self, obs):
        """crl_dqn_q_values: the twin's Q on the mu half"""
        keep = self.q
        try:
            self.q = np.asarray(greedy_image(self), F32)
            return self.q_values(obs)
        finally:
            self.q = keep


def make(cfg, per, tgt, c51, dueling, params, tape=None):
    """cfg, per, tgt, c51 as duel_ref.make; dueling: bool; params: 2P float32 → the restatement of a crl_dqn_noisy_create handle"""
    lay = layers(dueling, None if c51 is None else c51["n_atoms"])
    base = (D.DuelScalar if c51 is None else D.DuelC51) if dueling else (T.DQNTarget if c51 is None else Z.C51)
    tgt = {"n_step": 1, "double_q": 0} if tgt is None else tgt
    mu = np.asarray(params, F32)[:param_count(lay)]

    class Noisy(_Noisy, base):
        pass
    agent = Noisy(cfg, per, tgt, mu) if c51 is None else Noisy(cfg, per, tgt, c51, mu)
    if not hasattr(agent, "q_values"):                     # the scalar one-headed restatement has none of its own
        import value_eval_ref as V
        Noisy.q_values = lambda self, obs: V.q_values(np.ascontiguousarray(self.q, F32), np.ascontiguousarray(obs, np.float64))
    agent._noisy_init(lay, params, tape)
    return agent
