"""Float64 numpy restatement of the DQN loop with the categorical (C51) critic as include/cleanrl_hip.h pins it (the "Categorical DQN" block): the
yardstick of tests/test_c51_cpu.py and tests/test_gpu_c51.py. Written from the header — not from the kernels.

It builds on tests/dqn_target_ref.py and tests/dqn_per_ref.py by import: the env, the ring, both samplers, the tree, the n-step walk, Adam and the
trunk's dense layers are theirs. Restated here: the head of 2N rows, softmax, expectation, the projection (in the header's GATHER form: every target
atom looks at every source atom, sources ascending), the cross-entropy, its backward pass, and `update` / `run`, because the greedy action and the
target are formed inside them. Every sum whose order the header pins is an explicit ascending loop (np.sum is pairwise).

The pieces are small module-level functions, so that tests/c51_bar.py can replace one line at a time (mutants) or move every exp and log result by a
few ulp (the jittered twin): `_exp` and `_log` are the two transcendentals of the feature."""
import numpy as np

import ddpg_ref as R
import dqn_per_ref as P
import dqn_target_ref as T
import value_eval_ref as V

TRUNK = 10764                                  # W1 b1 W2 b2


def _exp(x):
    return np.exp(x)


def _log(x):
    return np.log(x)


# ---------------------------------------------------------------------------------------------------- the network
def sizes(N):
    return [480, 120, 10080, 84, 84 * 2 * N, 2 * N]


def param_count(N):
    return TRUNK + 85 * 2 * N


def split(p, N):
    """flat float32 → [W1 (120, 4), b1, W2 (84, 120), b2, W3 (2N, 84), b3] as float64"""
    out, o = [], 0
    for n, shape in zip(sizes(N), ((120, 4), (120,), (84, 120), (84,), (2 * N, 84), (2 * N,))):
        out.append(np.asarray(p[o:o + n], np.float32).astype(np.float64).reshape(shape, order="F")); o += n
    return out


def forward(p, N, X):
    """X (4, k) → (h1 (120, k), h2 (84, k), logits (2, N, k)): row a·N + i of the head is atom i of action a"""
    W1, b1, W2, b2, W3, b3 = split(p, N)
    h1 = P.relu(R.dense(W1, b1, X)); h2 = P.relu(R.dense(W2, b2, h1))
    return h1, h2, R.dense(W3, b3, h2).reshape(2, N, -1)


def atoms(c51):
    N = c51["n_atoms"]
    delta = (np.float64(c51["v_max"]) - np.float64(c51["v_min"])) / np.float64(N - 1)
    return np.float64(c51["v_min"]) + np.arange(N).astype(np.float64) * delta, delta


def sum_atoms(M):
    """Σ over axis 0, ascending, from 0.0"""
    acc = np.zeros(M.shape[1:], np.float64)
    for i in range(M.shape[0]):
        acc = acc + M[i]
    return acc


def softmax(l):
    """l (N, k) → (p, logp)"""
    mx = l.max(axis=0)
    d = l - mx
    e = _exp(d)
    S = sum_atoms(e)
    return e / S, d - _log(S)


def expect(p, z):
    return sum_atoms(z[:, None] * p)


def q_of(l3, z):
    """logits (2, N, k) → Q (2, k)"""
    return np.stack([expect(softmax(l3[a])[0], z) for a in range(2)])


# ---------------------------------------------------------------------------------------------------- the target: hooks the mutants replace
def astar_source(double_q, Qs, Qt):
    return Qs if double_q else Qt


def pprime_source(ls, lt):
    """the logits p' is the softmax of: target_net(x)"""
    return lt


def shifted(R_, disc, z_s, term):
    return R_ + ((disc * z_s) * (1.0 - term))


def clamp(Tz, v_min, v_max):
    return np.where(Tz < v_min, v_min, np.where(Tz > v_max, v_max, Tz))


def split_weights(pp, b, lo, up):
    """→ (what lo receives, what up receives) when lo != up"""
    return pp * (up - b), pp * (b - lo)


def taken(a):
    return a


def cotangent(w, p, m, k):
    return w * (p - m) / np.float64(k)


def project(pp, R_, disc, term, c51):
    """pp (N, k) p' rows, R_, disc (k,), term uint8 (k,) → m (N, k), gather form"""
    N, v_min, v_max = c51["n_atoms"], np.float64(c51["v_min"]), np.float64(c51["v_max"])
    z, delta = atoms(c51)
    term = np.asarray(term).astype(np.float64)
    top = np.float64(N - 1)
    lo, up, wl, wu = [], [], [], []
    for s in range(N):
        Tz = clamp(shifted(R_, disc, z[s], term), v_min, v_max)
        b = (Tz - v_min) / delta
        b = np.where(b > top, top, b)
        l_, u_ = np.floor(b), np.ceil(b)
        a_, c_ = split_weights(pp[s], b, l_, u_)
        lo.append(l_); up.append(u_); wl.append(np.where(l_ == u_, pp[s], a_)); wu.append(np.where(l_ == u_, 0.0, c_))
    me = np.arange(N).astype(np.float64)[:, None]
    m = np.zeros((N, pp.shape[1]))
    for s in range(N):                                   # every target atom i looks at source s: lo first, else up, else nothing (an exact 0.0)
        m = m + np.where(lo[s][None, :] == me, wl[s][None, :], np.where(up[s][None, :] == me, wu[s][None, :], 0.0))
    return m


# ---------------------------------------------------------------------------------------------------- cross-entropy, backward
def sample_losses(qp, N, state, a, m):
    """→ (h1, h2, p, loss_j) for the taken actions' rows"""
    k = a.size
    h1, h2, l3 = forward(qp, N, state)
    p, logp = softmax(l3[taken(a), :, np.arange(k)].T)
    return h1, h2, p, -sum_atoms(m * logp)


def loss_grads(qp, N, state, a, m, w):
    """→ (loss, the flat float64 gradient before the float32 projection, loss_j)"""
    k = a.size
    h1, h2, p, loss_j = sample_losses(qp, N, state, a, m)
    wl = w * loss_j
    loss = np.float64(0.0)
    for b in range(k):
        loss = loss + wl[b]
    loss = loss / np.float64(k)
    dl = cotangent(w, p, m, k)                           # (N, k) on the taken action's logits
    W1, b1, W2, b2, W3, b3 = split(qp, N)
    t2 = np.zeros((84, k))
    for i in range(N):
        t2 += W3[a * N + i, :].T * dl[i][None, :]
    d2 = np.where(h2 > 0.0, t2, 0.0)
    t1 = np.zeros((120, k))
    for j in range(84):
        t1 += W2[j, :][:, None] * d2[j:j + 1, :]
    d1 = np.where(h1 > 0.0, t1, 0.0)
    gW1, gb1, gW2, gb2 = np.zeros((120, 4)), np.zeros(120), np.zeros((84, 120)), np.zeros(84)
    gW3, gb3 = np.zeros((2 * N, 84)), np.zeros(2 * N)
    for b in range(k):                                   # every sum over the samples in sample order; the other action's rows get an exact 0.0
        gW1 += d1[:, b][:, None] * state[:, b][None, :]; gb1 += d1[:, b]
        gW2 += d2[:, b][:, None] * h1[:, b][None, :]; gb2 += d2[:, b]
        r = slice(a[b] * N, (a[b] + 1) * N)
        gW3[r, :] += dl[:, b][:, None] * h2[:, b][None, :]; gb3[r] += dl[:, b]
    return loss, R._flat([gW1, gb1, gW2, gb2, gW3, gb3]), loss_j


# ---------------------------------------------------------------------------------------------------- the loop
class C51(T.DQNTarget):
    """cfg: an oraclelib.DQNConfigC; per: None or the PER dict; tgt: dict(n_step, double_q); c51: dict(n_atoms, v_min, v_max); params: the flat float32
    net of param_count(n_atoms) numbers"""

    def __init__(self, cfg, per, tgt, c51, params):
        super().__init__(cfg, per, tgt, params)
        self.c51 = dict(c51); self.N = int(c51["n_atoms"])
        assert self.q.size == param_count(self.N)
        self.opt = R.Adam(param_count(self.N), sizes(self.N), cfg.lr)
        self.z = atoms(self.c51)[0]
        k = cfg.batch_size
        self.proj = np.zeros((self.N, k)); self.sample_loss = np.zeros(k)
        self.greedy = []                                  # (global_step, action) of every greedy step
        self.seen = []                                    # (g, idx, astar, leaves after the update) of every update: what the tie condition compares

    def q_values(self, obs):
        return q_of(forward(self.q, self.N, np.asarray(obs, np.float64).reshape(4, -1, order="F"))[2], self.z)

    def probs(self, obs):
        l3 = forward(self.q, self.N, np.asarray(obs, np.float64).reshape(4, -1, order="F"))[2]
        return np.stack([softmax(l3[a])[0] for a in range(2)], axis=1)          # (N, 2, n)

    def update(self):
        c, g, k = self.c, self.global_step, self.c.batch_size
        fresh = min(g - self.synced_step, c.buffer_size)                   # Add: the slots behind ptr get max_leaf
        slots = (self.ptr - 1 - np.arange(fresh)) % c.buffer_size
        self._set_leaves(slots, P.new_slot_leaf(self.max_leaf))
        self.synced_step = g
        self.beta = P.beta_schedule(self.per, g)
        if self.sampler is None:
            idx = P.sample(self.tree, self.C, c.seed, g, k)
            w = P.weights(self.tree, self.C, self.size, idx, self.beta)
        else:
            idx, w = self.sampler(self, g, self.size)
        idx = np.asarray(idx, np.int32)
        last, m_steps, nret, ndisc = T.walk_batch(self.reward, self.terminal, c.buffer_size, self.ptr, idx, self.n_step, c.gamma)
        x = self.next_state[:, last]
        lt, ls = forward(self.t, self.N, x)[2], forward(self.q, self.N, x)[2]
        Qt, Qs = q_of(lt, self.z), q_of(ls, self.z)
        astar = T.first_max(astar_source(self.double_q, Qs, Qt))
        pp = softmax(pprime_source(ls, lt)[astar, :, np.arange(k)].T)[0]
        proj = project(pp, nret, ndisc, self.terminal[last], self.c51)
        a = self.action[idx]
        self.last_loss, grad, loss_j = loss_grads(self.q, self.N, self.state[:, idx], a, proj, w)
        self.last_loss = float(self.last_loss)
        self.q = self.opt.step(self.q, grad)
        self.n_updates += 1
        if g % c.target_net_freq == 0:
            self.t = self.q.copy()
        self.idx, self.w, self.abs_td = idx, w, loss_j
        self.last, self.m, self.nret, self.ndisc, self.astar = last, m_steps, nret, ndisc, astar.astype(np.int32)
        self.td = T.target(nret, ndisc, Qt[astar, np.arange(k)], self.terminal[last])
        self.proj, self.sample_loss = proj, loss_j
        new = P.leaf_of(loss_j, self.per)                                  # duplicates carry identical values
        self._set_leaves(idx, new)
        self.max_leaf = P.raise_max(self.max_leaf, new)
        self.seen.append((g, idx.copy(), self.astar.copy(), self.leaves.copy()))

    def run(self, max_env_steps):
        """dqn_per_ref.DQNPER.run with the greedy action taken from the expected values → (taken, episodes, losses)"""
        c = self.c
        taken_, eps, losses = 0, [], []
        while taken_ < max_env_steps and self.global_step < c.total_timesteps:
            self.global_step += 1; taken_ += 1
            g = self.global_step
            obs = self.env.copy()
            slope = (c.epsilon_end - c.epsilon_start) / c.epsilon_duration
            v = slope * float(g) + c.epsilon_start
            eps_t = v if v > c.epsilon_end else c.epsilon_end
            if float(R.uniform(c.seed, np.array([0]), g, 0)[0]) < eps_t:
                action = int(R.philox_env(c.seed, np.array([0]), g, 4)[0][0] >> np.uint64(31))
            else:
                q = self.q_values(obs)[:, 0]
                action = 1 if q[1] > q[0] else 0
                self.greedy.append((g, action))
            self.env_t, done = V.step(self.env, self.env_t, action, c.max_steps)
            rew = 0.0 if done else 1.0
            p = self.ptr
            self.state[:, p] = obs; self.next_state[:, p] = self.env; self.action[p] = action; self.reward[p] = rew; self.terminal[p] = 1 if done else 0
            self.ptr = 0 if p + 1 >= c.buffer_size else p + 1
            self.size = min(c.buffer_size, self.size + 1)
            self.episode_return += rew; self.episode_length += 1
            if done:
                eps.append((self.episode_return, self.episode_length, g, eps_t))
                self.episode_length = 0; self.episode_return = 0.0
                self.env = P.reset(c.seed, g, 1); self.env_t = 0
            if g > c.min_buff_size and g % c.train_freq == 0:
                self.update()
                if g % c.log_frequency == 0:
                    losses.append((g, self.last_loss))
        return taken_, eps, losses
