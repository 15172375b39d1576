"""Float64 numpy restatement of the dqn.jl loop with prioritized replay as include/cleanrl_hip.h pins it (the crl_dqn_per_* block): the yardstick of
tests/test_dqn_per_cpu.py and tests/test_gpu_dqn_per.py. Written from the header and from oracle/dqn_oracle.c — not from the kernels.

What comes from elsewhere: the CartPoleEnv{Float64} step and the acting forward are the C oracle's (a2c_cartpole_step, dqn_forward, through
tests/value_eval_ref.py), Philox and Adam are tests/ddpg_ref.py's. The update is restated here in the device's order: a Dense layer adds its products in
input order and the bias last, a sum over the batch runs in sample order, a gradient is rounded to Float32 before Adam. No BLAS call anywhere.

The sampler, the weights and the schedule are small module-level functions, so that tests/dqn_per_bar.py can replace one line at a time (mutants) or
move every pow by a few ulp (the jittered twin): `_pow` is the one transcendental of the feature."""
import numpy as np

import ddpg_ref as R
import oraclelib as O
import value_eval_ref as V

S_PER = 0xDA                                   # the prioritized draw's Philox stream (the uniform draw is 0xD9)
SIZES = [480, 120, 10080, 84, 168, 2]          # W1 b1 W2 b2 W3 b3
OFF = O.DQN_OFF
LEAF_MIN, LEAF_MAX = 2.0 ** -100, 2.0 ** 100
LEAF_T = np.float32                            # leaves are Float32, stored widened
COUNTS = {"zero_saves": 0}                     # draws that only the zero test kept out of an empty subtree (rounding put target at or past the left sum)


def _pow(x, y):
    return np.power(x, y)


# ---------------------------------------------------------------------------------------------------- the tree
def tree_leaves(cap):
    C = 1
    while C < cap:
        C *= 2
    return C


def build_tree(leaves, C=None):
    """the whole tree from the leaves (slots past len(leaves) hold 0.0): every inner node is left + right, one add"""
    leaves = np.asarray(leaves, np.float64)
    C = tree_leaves(leaves.size) if C is None else C
    tree = np.zeros(2 * C)
    tree[C:C + leaves.size] = leaves
    P = C // 2
    while P >= 1:
        tree[P:2 * P] = tree[2 * P:4 * P:2] + tree[2 * P + 1:4 * P:2]
        P //= 2
    return tree


def repair(tree, C, slots):
    """the ancestors of the touched slots, level by level (the incremental form; build_tree gives the same bits)"""
    nodes = np.unique(C + np.asarray(slots, np.int64))
    while nodes.size and nodes[0] > 1:
        nodes = np.unique(nodes >> 1)
        tree[nodes] = tree[2 * nodes] + tree[2 * nodes + 1]


# ---------------------------------------------------------------------------------------------------- the sampler
def draw_targets(seed, g, k, total):
    seg = total / np.float64(k)
    u = R.uniform(seed, np.arange(k), g, S_PER)
    return (np.arange(k).astype(np.float64) + u) * seg


def go_left(target, l, r):
    return target < l or r == 0.0


def descend(tree, C, target):
    i = 1
    while i < C:
        l, r = tree[2 * i], tree[2 * i + 1]
        if r == 0.0 and not target < l:
            COUNTS["zero_saves"] += 1
        if go_left(target, l, r):
            i = 2 * i
        else:
            target = target - l
            i = 2 * i + 1
    return i - C


def sample(tree, C, seed, g, k):
    return np.array([descend(tree, C, t) for t in draw_targets(seed, g, k, tree[1])], np.int32)


# ---------------------------------------------------------------------------------------------------- weights, schedule, leaves
def beta_schedule(per, g):
    slope = (per["beta_end"] - per["beta_start"]) / per["beta_duration"]
    v = slope * float(g) + per["beta_start"]
    if slope < 0.0:
        return per["beta_end"] if v < per["beta_end"] else v
    return per["beta_end"] if v > per["beta_end"] else v


def normalise(w):
    return w / w.max()


def weights(tree, C, n, idx, beta):
    return normalise(_pow(np.float64(n) * tree[C + idx] / tree[1], -np.float64(beta)))


def priority(abs_td, eps):
    return abs_td + eps


def leaf_of(abs_td, per):
    p = _pow(priority(np.asarray(abs_td, np.float64), per["eps"]), np.float64(per["alpha"]))
    p = np.where(p >= LEAF_MIN, np.where(p > LEAF_MAX, LEAF_MAX, p), LEAF_MIN)
    return p.astype(LEAF_T).astype(np.float64)


def new_slot_leaf(max_leaf):
    return max_leaf


def raise_max(max_leaf, new_leaves):
    return max(max_leaf, float(new_leaves.max()))


def cotangent(w, diff, k):
    return -2.0 * w * diff / np.float64(k)


# ---------------------------------------------------------------------------------------------------- the Q-network
def split(p):
    """flat float32 → [W1 (120, 4), b1, W2 (84, 120), b2, W3 (2, 84), b3] as float64"""
    out = []
    for i, shape in enumerate(((120, 4), (120,), (84, 120), (84,), (2, 84), (2,))):
        out.append(np.asarray(p[OFF[i]:OFF[i + 1]], np.float32).astype(np.float64).reshape(shape, order="F"))
    return out


def relu(x):
    return np.where(x > 0.0, x, 0.0)


def forward(p, X):
    """X (4, k) → (h1 (120, k), h2 (84, k), q (2, k))"""
    W1, b1, W2, b2, W3, b3 = split(p)
    h1 = relu(R.dense(W1, b1, X)); h2 = relu(R.dense(W2, b2, h1))
    return h1, h2, R.dense(W3, b3, h2)


def loss_grads(qp, tp, batch, gamma, w):
    """The TD target from the target net, the importance-weighted mse and its gradient (float64, flat, before the float32 projection), and δ.
    batch: state / next_state (4, k), action int (k,), reward (k,), terminal uint8 (k,)"""
    k = batch["reward"].size
    a = batch["action"]
    tq = forward(tp, batch["next_state"])[2]
    next_q = np.where(tq[1] > tq[0], tq[1], tq[0])
    td = batch["reward"] + gamma * next_q * (1.0 - batch["terminal"].astype(np.float64))
    h1, h2, q = forward(qp, batch["state"])
    diff = td - q[a, np.arange(k)]
    sq = w * (diff * diff)
    loss = np.float64(0.0)
    for b in range(k):
        loss = loss + sq[b]
    loss = loss / np.float64(k)
    dz = cotangent(w, diff, k)
    W1, b1, W2, b2, W3, b3 = split(qp)
    d2 = np.where(h2 > 0.0, W3[a, :].T * dz[None, :], 0.0)
    t1 = np.zeros((120, k))
    for j in range(84):
        t1 += W2[j, :][:, None] * d2[j:j + 1, :]
    d1 = np.where(h1 > 0.0, t1, 0.0)
    gW1, gb1, gW2, gb2 = np.zeros((120, 4)), np.zeros(120), np.zeros((84, 120)), np.zeros(84)
    gW3, gb3 = np.zeros((2, 84)), np.zeros(2)
    X = batch["state"]
    for b in range(k):                                   # every sum over the samples in sample order
        gW1 += d1[:, b][:, None] * X[:, b][None, :]; gb1 += d1[:, b]
        gW2 += d2[:, b][:, None] * h1[:, b][None, :]; gb2 += d2[:, b]
        gW3[a[b], :] += dz[b] * h2[:, b]; gb3[a[b]] += dz[b]
    return loss, R._flat([gW1, gb1, gW2, gb2, gW3, gb3]), diff


# ---------------------------------------------------------------------------------------------------- the loop
def reset(seed, gstep, stream):
    return np.ascontiguousarray(0.1 * R.uniform(seed, np.arange(4), gstep, stream) - 0.05)


def uniform_sampler(agent, g, n):
    """dqn.jl's own draw (the oracle's), unit weights: what the anchor test of tests/test_dqn_per_cpu.py runs"""
    return O.dqn_sample_indices(agent.c.seed, g, n, agent.c.batch_size), np.ones(agent.c.batch_size)


class DQNPER:
    """cfg: an oraclelib.DQNConfigC; per: dict(alpha, beta_start, beta_end, beta_duration, eps); params: the flat float32 q-net. sampler=None is
    prioritized replay; a callable (agent, g, n) → (idx, w) replaces draw and weights (the tree is kept up either way)."""

    def __init__(self, cfg, per, params, sampler=None):
        self.c, self.per, self.sampler = cfg, dict(per), sampler
        self.q = np.array(params, np.float32); self.t = self.q.copy()
        self.opt = R.Adam(O.DQN_P, SIZES, cfg.lr)
        cap = cfg.buffer_size
        self.state = np.zeros((4, cap)); self.next_state = np.zeros((4, cap)); self.action = np.zeros(cap, np.int64)
        self.reward = np.zeros(cap); self.terminal = np.zeros(cap, np.uint8)
        self.ptr = self.size = 0
        self.C = tree_leaves(cap)
        self.leaves = np.zeros(cap); self.tree = np.zeros(2 * self.C)
        self.max_leaf = 1.0; self.synced_step = 0; self.beta = self.per["beta_start"]
        self.env = reset(cfg.seed, 0, 2); self.env_t = 0
        self.global_step = self.n_updates = 0; self.last_loss = 0.0
        self.episode_return = 0.0; self.episode_length = 0
        self.idx = np.zeros(cfg.batch_size, np.int32); self.w = np.zeros(cfg.batch_size); self.abs_td = np.zeros(cfg.batch_size)
        self.n_spread = 0                                 # updates that drew from leaves that were not all equal
        self.seen = []                                    # (g, idx, leaves after the update) of every update: what the tie condition compares

    def _set_leaves(self, slots, values):
        self.leaves[slots] = values
        self.tree[self.C + np.asarray(slots)] = values
        repair(self.tree, self.C, slots)

    def update(self):
        c, g, k = self.c, self.global_step, self.c.batch_size
        fresh = min(g - self.synced_step, c.buffer_size)                   # Add: the slots behind ptr get max_leaf
        slots = (self.ptr - 1 - np.arange(fresh)) % c.buffer_size
        self._set_leaves(slots, new_slot_leaf(self.max_leaf))
        self.synced_step = g
        self.beta = beta_schedule(self.per, g)
        self.n_spread += int(self.leaves[:self.size].min() != self.leaves[:self.size].max())
        if self.sampler is None:
            idx = sample(self.tree, self.C, c.seed, g, k)
            w = weights(self.tree, self.C, self.size, idx, self.beta)
        else:
            idx, w = self.sampler(self, g, self.size)
        batch = dict(state=self.state[:, idx], next_state=self.next_state[:, idx], action=self.action[idx], reward=self.reward[idx],
                     terminal=self.terminal[idx])
        self.last_loss, grad, diff = loss_grads(self.q, self.t, batch, c.gamma, w)
        self.last_loss = float(self.last_loss)
        self.q = self.opt.step(self.q, grad)
        self.n_updates += 1
        if g % c.target_net_freq == 0:
            self.t = self.q.copy()
        self.idx, self.w, self.abs_td = np.asarray(idx, np.int32), w, np.abs(diff)
        new = leaf_of(self.abs_td, self.per)                               # duplicates carry identical values
        self._set_leaves(idx, new)
        self.max_leaf = raise_max(self.max_leaf, new)
        self.seen.append((g, self.idx.copy(), self.leaves.copy()))

    def run(self, max_env_steps):
        """→ (taken, episodes, losses) as oraclelib.DQNState.run"""
        c = self.c
        taken, eps, losses = 0, [], []
        while taken < max_env_steps and self.global_step < c.total_timesteps:
            self.global_step += 1; taken += 1
            g = self.global_step
            obs = self.env.copy()
            slope = (c.epsilon_end - c.epsilon_start) / c.epsilon_duration
            v = slope * float(g) + c.epsilon_start
            eps_t = v if v > c.epsilon_end else c.epsilon_end
            if float(R.uniform(c.seed, np.array([0]), g, 0)[0]) < eps_t:
                action = int(R.philox_env(c.seed, np.array([0]), g, 4)[0][0] >> np.uint64(31))
            else:
                q = V.q_values(self.q, obs)
                action = 1 if q[1] > q[0] else 0
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
                self.env = reset(c.seed, g, 1); self.env_t = 0
            if g > c.min_buff_size and g % c.train_freq == 0:
                self.update()
                if g % c.log_frequency == 0:
                    losses.append((g, self.last_loss))
        return taken, eps, losses

    def status(self):
        return dict(state=self.env.copy(), global_step=self.global_step, rb_size=self.size, n_updates=self.n_updates, last_loss=self.last_loss)

    def per_status(self):
        return dict(beta=self.beta, total=float(self.tree[1]), max_leaf=np.float32(self.max_leaf), tree_leaves=self.C)
