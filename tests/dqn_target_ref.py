"""Float64 numpy restatement of the DQN loop with n-step returns and double Q-learning as include/cleanrl_hip.h pins them (the "DQN target options"
block): the yardstick of tests/test_dqn_target_cpu.py and tests/test_gpu_dqn_target.py. Written from the header — not from the kernels.

It builds on tests/dqn_per_ref.py by import: the env, the ring, the acting forward, both samplers, the tree, Adam and the loop are DQNPER's; only
`update` is restated here, because the TD target is formed inside it. The backward pass is dqn_per_ref.loss_grads' with the target passed in.

The walk, the a* choice and the target are small module-level functions, so that tests/dqn_target_bar.py can replace one line at a time (mutants).
COUNTS holds four events per run (reset it before one): walks a terminal stopped before n_step, walks the head stopped, walks that crossed slot
cap−1 → 0, and samples whose double-Q a* is not target_net's argmax."""
import numpy as np

import ddpg_ref as R
import dqn_per_ref as P

EVENTS = ("terminal_stops", "head_stops", "wraps", "disagree")
COUNTS = {e: 0 for e in EVENTS}


def reset_counts():
    for e in EVENTS:
        COUNTS[e] = 0


# ---------------------------------------------------------------------------------------------------- the walk
def window_terminal(t):
    return t != 0


def head_stop(nx, ptr):
    return nx == ptr


def walk(reward, terminal, cap, ptr, s, n_step, gamma):
    """→ (last, m, R, disc) of the header's walk from slot s; Python floats are Float64, one operation per operator"""
    R_, disc, c, m = 0.0, 1.0, int(s), 0
    gamma = float(gamma)
    while True:
        R_ = R_ + disc * float(reward[c])
        disc = disc * gamma
        m += 1
        last = c
        if window_terminal(terminal[last]):
            COUNTS["terminal_stops"] += int(m < n_step)
            break
        if m == n_step:
            break
        nx = 0 if last + 1 == cap else last + 1
        if head_stop(nx, ptr):
            COUNTS["head_stops"] += 1
            break
        COUNTS["wraps"] += int(nx == 0)
        c = nx
    return last, m, R_, disc


def walk_batch(reward, terminal, cap, ptr, idx, n_step, gamma):
    out = [walk(reward, terminal, cap, ptr, s, n_step, gamma) for s in idx]
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.float64),
            np.array([o[3] for o in out], np.float64))


# ---------------------------------------------------------------------------------------------------- the target
def boot_slot(s, last):
    return last


def first_max(q):
    """(2, k) → the first maximum per column"""
    return np.where(q[1] > q[0], 1, 0)


def astar_source(double_q, sq, tq):
    return sq if double_q else tq


def next_q_source(sq, tq):
    return tq


def td_disc(disc, gamma):
    return disc


def target(R_, disc, next_q, term):
    return R_ + disc * next_q * (1.0 - term.astype(np.float64))


# ---------------------------------------------------------------------------------------------------- mse, backward (dqn_per_ref.loss_grads with td given)
def loss_grads(qp, state, a, td, w):
    k = td.size
    h1, h2, q = P.forward(qp, state)
    diff = td - q[a, np.arange(k)]
    sq = w * (diff * diff)
    loss = np.float64(0.0)
    for b in range(k):
        loss = loss + sq[b]
    loss = loss / np.float64(k)
    dz = P.cotangent(w, diff, k)
    W1, b1, W2, b2, W3, b3 = P.split(qp)
    d2 = np.where(h2 > 0.0, W3[a, :].T * dz[None, :], 0.0)
    t1 = np.zeros((120, k))
    for j in range(84):
        t1 += W2[j, :][:, None] * d2[j:j + 1, :]
    d1 = np.where(h1 > 0.0, t1, 0.0)
    gW1, gb1, gW2, gb2 = np.zeros((120, 4)), np.zeros(120), np.zeros((84, 120)), np.zeros(84)
    gW3, gb3 = np.zeros((2, 84)), np.zeros(2)
    for b in range(k):                                   # every sum over the samples in sample order
        gW1 += d1[:, b][:, None] * state[:, b][None, :]; gb1 += d1[:, b]
        gW2 += d2[:, b][:, None] * h1[:, b][None, :]; gb2 += d2[:, b]
        gW3[a[b], :] += dz[b] * h2[:, b]; gb3[a[b]] += dz[b]
    return loss, R._flat([gW1, gb1, gW2, gb2, gW3, gb3]), diff


# ---------------------------------------------------------------------------------------------------- the loop
PER_OFF = dict(alpha=0.6, beta_start=0.4, beta_end=1.0, beta_duration=1.0, eps=1e-6)     # the unused tree of a uniform run needs some options


class DQNTarget(P.DQNPER):
    """cfg: an oraclelib.DQNConfigC; per: None (uniform replay: the oracle's draw, unit weights) or the PER dict; tgt: dict(n_step, double_q)"""

    def __init__(self, cfg, per, tgt, params):
        super().__init__(cfg, PER_OFF if per is None else per, params, sampler=P.uniform_sampler if per is None else None)
        self.uniform = per is None
        self.n_step, self.double_q = int(tgt["n_step"]), bool(tgt["double_q"])
        k = cfg.batch_size
        self.last = np.zeros(k, np.int32); self.m = np.zeros(k, np.int32); self.astar = np.zeros(k, np.int32)
        self.nret = np.zeros(k); self.ndisc = np.zeros(k); self.td = np.zeros(k)

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
        last, m, nret, ndisc = walk_batch(self.reward, self.terminal, c.buffer_size, self.ptr, idx, self.n_step, c.gamma)
        x = self.next_state[:, boot_slot(idx, last)]
        tq, sq = P.forward(self.t, x)[2], P.forward(self.q, x)[2]
        astar = first_max(astar_source(self.double_q, sq, tq))
        if self.double_q:
            COUNTS["disagree"] += int((astar != first_max(tq)).sum())
        next_q = next_q_source(sq, tq)[astar, np.arange(k)]
        td = target(nret, td_disc(ndisc, c.gamma), next_q, self.terminal[last])
        self.last_loss, grad, diff = loss_grads(self.q, self.state[:, idx], self.action[idx], td, w)
        self.last_loss = float(self.last_loss)
        self.q = self.opt.step(self.q, grad)
        self.n_updates += 1
        if g % c.target_net_freq == 0:
            self.t = self.q.copy()
        self.idx, self.w, self.abs_td = idx, w, np.abs(diff)
        self.last, self.m, self.nret, self.ndisc, self.astar, self.td = last, m, nret, ndisc, astar.astype(np.int32), td
        new = P.leaf_of(self.abs_td, self.per)                             # duplicates carry identical values
        self._set_leaves(idx, new)
        self.max_leaf = P.raise_max(self.max_leaf, new)

    def target_read(self):
        return dict(last=self.last, m=self.m, nret=self.nret, ndisc=self.ndisc, astar=self.astar, td=self.td)
