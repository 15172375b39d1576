"""Float64 numpy restatement of src/algorithms/ddpg.jl as the library runs it (the crl_ddpg_* block of include/cleanrl_hip.h): the yardstick of
tests/test_ddpg_cpu.py and tests/test_gpu_ddpg.py. Written from ddpg.jl, replay_buffer.jl and the interface's description — not from the kernels.

Conventions. Weights are float32, every activation / loss / cotangent is float64. A network is one flat float32 vector in Flux.params order
(W1 b1 W2 b2 W3 b3, each W (out, in) column-major). A Dense layer adds its products in input order and the bias last; a sum over the batch runs in
sample order; a gradient is rounded to float32 before Adam. Counters: philox(component, global_step lo, hi, stream; key = seed). Streams: 0x10
behaviour noise, 0x11 warm-up uniform, 0x12 target-actor noise, 0x13 actor-loss noise, 0x14 / 0x15 Pendulum reset (loop / first), 0xD9 sampling."""
import math

import numpy as np

H = 64
S_BEHAVE, S_WARMUP, S_TARGET, S_ACTOR, S_RESET, S_RESET0, S_SAMPLE = 0x10, 0x11, 0x12, 0x13, 0x14, 0x15, 0xD9
B1, B2, EPS = 0.9, 0.999, 1e-8
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- Philox4x32-10, u53, Box–Muller
def philox(c0, c1, c2, c3, k0, k1):
    """Vectorised over c0 (any integer array); the other words are scalars. Returns four uint64 arrays holding 32-bit words."""
    c0 = np.asarray(c0, np.uint64) & np.uint64(M32)
    c1 = np.full_like(c0, c1 & M32); c2 = np.full_like(c0, c2 & M32); c3 = np.full_like(c0, c3 & M32)
    k0 &= M32; k1 &= M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0; p1 = np.uint64(0xCD9E8D57) * c2
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(M32)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(M32)
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0 = (k0 + 0x9E3779B9) & M32; k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox_env(seed, comp, gstep, stream):
    return philox(comp, gstep & M32, gstep >> 32, stream, seed & M32, seed >> 32)


def _u53(hi, lo):
    return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def uniform(seed, comps, gstep, stream):
    x, y, _, _ = philox_env(seed, comps, gstep, stream)
    return _u53(x, y)


def normal(seed, comps, gstep, stream):
    """Box–Muller from the two u53 halves of one Philox block."""
    x, y, z, w = philox_env(seed, comps, gstep, stream)
    u1, u2 = _u53(x, y), _u53(z, w)
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(6.283185307179586 * u2)


# ---------------------------------------------------------------- activations, Pendulum
def tanh_fast64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x + x)
        y = (e - 1.0) / (e + 1.0)
    x2 = x * x
    p = np.full_like(x, -0.008697141630499953)
    for c in (0.02186660872609521, -0.05396823125794372, 0.13333333325511604, -0.33333333333324583, 1.0):
        p = p * x2 + c
    return np.where(x2 > 900.0, np.sign(x), np.where(x2 < 0.017, x * p, y))


_SIN_C = [(-1.0 if i % 2 == 0 else 1.0) / float(math.factorial(2 * i + 3)) for i in range(14)]
_COS_C = [(-1.0 if i % 2 == 0 else 1.0) / float(math.factorial(2 * i + 2)) for i in range(14)]


def pend_sin(x):
    x = np.float64(x); x2 = x * x
    p = np.float64(_SIN_C[13])
    for i in range(12, -1, -1):
        p = p * x2 + _SIN_C[i]
    return x + (x * x2) * p


def pend_cos(x):
    x = np.float64(x); x2 = x * x
    p = np.float64(_COS_C[13])
    for i in range(12, -1, -1):
        p = p * x2 + _COS_C[i]
    return 1.0 + x2 * p


PI = 3.141592653589793


def pendulum_obs(th, thd):
    return np.array([pend_cos(th), pend_sin(th), thd], np.float64)


def pendulum_step(th, thd, t, a0, max_steps=200):
    """→ (θ', θ̇', t', reward, terminal): g = 10, m = l = 1, dt = 0.05; the cost is the old state's."""
    th, thd, a0 = np.float64(th), np.float64(thd), np.float64(a0)
    u = np.float64(-2.0) if a0 < -2.0 else (np.float64(2.0) if a0 > 2.0 else a0)
    cost = th * th + 0.1 * (thd * thd) + 0.001 * (u * u)
    nthd = thd + (15.0 * pend_sin(th) + 3.0 * u) * 0.05
    nthd = np.float64(-8.0) if nthd < -8.0 else (np.float64(8.0) if nthd > 8.0 else nthd)
    nth = th + nthd * 0.05
    if nth >= PI:
        nth = nth - 2.0 * PI
    elif nth < -PI:
        nth = nth + 2.0 * PI
    return nth, nthd, t + 1, -cost, (t + 1) >= max_steps


def pendulum_reset(seed, gstep, stream):
    u = uniform(seed, np.arange(2), gstep, stream)
    return np.float64(-PI + (2.0 * PI) * u[0]), np.float64(-1.0 + 2.0 * u[1])


class Pendulum:
    """Host env object for the external mode (obs_dim / act_dim / act_low / act_high / reset / step), built on the functions above."""
    obs_dim, act_dim, act_low, act_high = 3, 1, -2.0, 2.0

    def __init__(self, seed=0, max_steps=200):
        self.seed, self.max_steps, self.n_resets = seed, max_steps, 0

    def reset(self):
        self.th, self.thd = pendulum_reset(self.seed, self.n_resets, S_RESET)
        self.t = 0; self.n_resets += 1
        return pendulum_obs(self.th, self.thd)

    def step(self, action):
        self.th, self.thd, self.t, r, term = pendulum_step(self.th, self.thd, self.t, np.asarray(action, np.float64)[0], self.max_steps)
        return float(r), pendulum_obs(self.th, self.thd), bool(term)


# ---------------------------------------------------------------- networks
def net_sizes(n_in, n_out):
    return [H * n_in, H, H * H, H, n_out * H, n_out]


def param_count(obs_dim, act_dim):
    return sum(net_sizes(obs_dim, act_dim)), sum(net_sizes(obs_dim + act_dim, 1))


def split(p, n_in, n_out):
    """flat float32 → [W1 (64, in), b1, W2 (64, 64), b2, W3 (out, 64), b3] as float64 views of the float32 values"""
    out, o = [], 0
    for n, shape in zip(net_sizes(n_in, n_out), ((H, n_in), (H,), (H, H), (H,), (n_out, H), (n_out,))):
        out.append(np.asarray(p[o:o + n], np.float32).astype(np.float64).reshape(shape, order="F")); o += n
    return out


def dense(W, b, X):
    """W (out, in), X (in, k) → (out, k): products added in input order, bias last"""
    acc = np.zeros((W.shape[0], X.shape[1]), np.float64)
    for j in range(W.shape[1]):
        acc += W[:, j:j + 1] * X[j:j + 1, :]
    return acc + b[:, None]


def actor_forward(p, obs_dim, act_dim, X):
    """→ (h1, h2, y3) with y3 = tanh_fast of the head; the Chain's output is y3·2 + noise (ddpg.jl:28)"""
    W1, b1, W2, b2, W3, b3 = split(p, obs_dim, act_dim)
    h1 = tanh_fast64(dense(W1, b1, X)); h2 = tanh_fast64(dense(W2, b2, h1)); y3 = tanh_fast64(dense(W3, b3, h2))
    return h1, h2, y3


def actor_mean(p, obs_dim, act_dim, X):
    return actor_forward(p, obs_dim, act_dim, np.asarray(X, np.float64).reshape(obs_dim, -1, order="F"))[2] * 2.0


def critic_forward(p, n_in, X):
    W1, b1, W2, b2, W3, b3 = split(p, n_in, 1)
    h1 = np.maximum(dense(W1, b1, X), 0.0); h2 = np.maximum(dense(W2, b2, h1), 0.0)
    return h1, h2, dense(W3, b3, h2)[0]


def q_values(p, obs_dim, act_dim, X, A):
    X = np.asarray(X, np.float64).reshape(obs_dim, -1, order="F"); A = np.asarray(A, np.float64).reshape(act_dim, -1, order="F")
    return critic_forward(p, obs_dim + act_dim, np.vstack([X, A]))[2]


def _sum_samples(M):
    """Σ over the last axis in sample order"""
    acc = np.zeros(M.shape[:-1], np.float64)
    for b in range(M.shape[-1]):
        acc = acc + M[..., b]
    return acc


def _flat(gs):
    return np.concatenate([np.asarray(g, np.float64).reshape(-1, order="F") for g in gs])


def td_target(actor_t, critic_t, obs_dim, act_dim, batch, gamma, noise_t):
    _, _, y3 = actor_forward(actor_t, obs_dim, act_dim, batch["next_state"])
    next_act = y3 * 2.0 + noise_t[:, None]                                               # ddpg.jl:108
    next_q = critic_forward(critic_t, obs_dim + act_dim, np.vstack([batch["next_state"], next_act]))[2]   # :109
    return batch["reward"] + gamma * next_q * (1.0 - batch["terminal"].astype(np.float64))              # :110


def critic_loss_grad(critic, obs_dim, act_dim, batch, td):
    """Flux.mse(td_target, q) and its hand-written gradient (float64, flat, before the float32 projection)   ddpg.jl:114-117"""
    k = td.size
    X = np.vstack([batch["state"], batch["action"]])
    W1, b1, W2, b2, W3, b3 = split(critic, obs_dim + act_dim, 1)
    h1, h2, q = critic_forward(critic, obs_dim + act_dim, X)
    diff = td - q
    loss = _sum_samples(diff * diff) / k
    dq = -2.0 * diff / k
    d2 = np.where(h2 > 0.0, W3[0][:, None] * dq[None, :], 0.0)
    t1 = np.zeros((H, k))
    for j in range(H):
        t1 += W2[j, :][:, None] * d2[j:j + 1, :]
    d1 = np.where(h1 > 0.0, t1, 0.0)
    gs = [_sum_samples(d1[:, None, :] * X[None, :, :]), _sum_samples(d1), _sum_samples(d2[:, None, :] * h1[None, :, :]), _sum_samples(d2),
          _sum_samples(dq[None, None, :] * h2[None, :, :]), _sum_samples(dq[None, :])]
    return loss, _flat(gs)


def actor_loss_grad(actor, critic, obs_dim, act_dim, batch, noise_a):
    """−mean(get_q(critic, state, actor(state))) and its gradient with respect to the actor only   ddpg.jl:122-124"""
    X = batch["state"]; k = X.shape[1]
    W1, b1, W2, b2, W3, b3 = split(actor, obs_dim, act_dim)
    C1, c1, C2, c2, C3, c3 = split(critic, obs_dim + act_dim, 1)
    h1, h2, y3 = actor_forward(actor, obs_dim, act_dim, X)
    act = y3 * 2.0 + noise_a[:, None]
    g1, g2, q = critic_forward(critic, obs_dim + act_dim, np.vstack([X, act]))
    loss = -(_sum_samples(q) / k)
    dq = np.full(k, -1.0 / k)
    e2 = np.where(g2 > 0.0, C3[0][:, None] * dq[None, :], 0.0)
    t1 = np.zeros((H, k))
    for j in range(H):
        t1 += C2[j, :][:, None] * e2[j:j + 1, :]
    e1 = np.where(g1 > 0.0, t1, 0.0)
    ga = np.zeros((act_dim, k))
    for i in range(H):
        ga += C1[i, obs_dim:][:, None] * e1[i:i + 1, :]
    d3 = (ga * 2.0) * (1.0 - y3 * y3)
    s2 = np.zeros((H, k))
    for c in range(act_dim):
        s2 += W3[c, :][:, None] * d3[c:c + 1, :]
    d2 = s2 * (1.0 - h2 * h2)
    t1 = np.zeros((H, k))
    for j in range(H):
        t1 += W2[j, :][:, None] * d2[j:j + 1, :]
    d1 = t1 * (1.0 - h1 * h1)
    gs = [_sum_samples(d1[:, None, :] * X[None, :, :]), _sum_samples(d1), _sum_samples(d2[:, None, :] * h1[None, :, :]), _sum_samples(d2),
          _sum_samples(d3[:, None, :] * h2[None, :, :]), _sum_samples(d3)]
    return loss, _flat(gs)


# ---------------------------------------------------------------- Adam, polyak, ring, sampling
class Adam:
    """Flux Adam(lr): float32 m, v and parameters, float64 scalars; one β-power pair per array (advanced after the step)"""

    def __init__(self, n, sizes, lr):
        self.m = np.zeros(n, np.float32); self.v = np.zeros(n, np.float32); self.lr = lr
        self.arr = np.repeat(np.arange(6), sizes); self.bp = np.tile(np.array([B1, B2]), (6, 1))

    def step(self, p, g64):
        g = g64.astype(np.float32).astype(np.float64)
        self.m = (B1 * self.m.astype(np.float64) + (1 - B1) * g).astype(np.float32)
        self.v = (B2 * self.v.astype(np.float64) + (1 - B2) * g * g).astype(np.float32)
        bp0, bp1 = self.bp[self.arr, 0], self.bp[self.arr, 1]
        delta = self.m.astype(np.float64) / (1 - bp0) / (np.sqrt(self.v.astype(np.float64) / (1 - bp1)) + EPS) * self.lr
        self.bp = self.bp * np.array([B1, B2])
        return p - delta.astype(np.float32)


def polyak(t, s, tau):
    return (tau * s.astype(np.float64) + (1.0 - tau) * t.astype(np.float64)).astype(np.float32)


def sample_indices(seed, gstep, n, k):
    """Buffer.sample: candidates in counter order, ((x·n) >> 32), one already taken is skipped (0-based slots)"""
    out, seen, base = [], set(), 0
    while len(out) < k:
        x = philox(np.arange(base, base + 1024), gstep & M32, gstep >> 32, S_SAMPLE, seed & M32, seed >> 32)[0]
        for j in ((x * np.uint64(n)) >> np.uint64(32)).tolist():
            if j not in seen:
                seen.add(j); out.append(j)
                if len(out) == k:
                    break
        base += 1024
    return np.array(out, np.int32)


class Ring:
    """replay_buffer.jl:9-37 with a 0-based ptr"""

    def __init__(self, obs_dim, act_dim, cap):
        self.cap, self.ptr, self.size = cap, 0, 0
        self.state = np.zeros((obs_dim, cap)); self.next_state = np.zeros((obs_dim, cap)); self.action = np.zeros((act_dim, cap))
        self.reward = np.zeros(cap); self.terminal = np.zeros(cap, np.uint8)

    def add(self, s, a, r, ns, term):
        p = self.ptr
        self.state[:, p] = s; self.action[:, p] = a; self.reward[p] = r; self.next_state[:, p] = ns; self.terminal[p] = 1 if term else 0
        self.ptr = 0 if p + 1 >= self.cap else p + 1
        self.size = min(self.cap, self.size + 1)

    def gather(self, idx):
        return dict(state=self.state[:, idx], action=self.action[:, idx], reward=self.reward[idx], next_state=self.next_state[:, idx],
                    terminal=self.terminal[idx])


# ---------------------------------------------------------------- the loop
class DDPG:
    """cfg: dict with total_timesteps, buffer_size, min_buff_size, batch_size, warmup_steps, log_frequency, lr, tau, gamma, exploration_noise, obs_dim,
    act_dim, max_steps, act_low, act_high, noise_in_update, seed"""

    def __init__(self, cfg, actor, critic):
        self.c = dict(cfg); D, A = cfg["obs_dim"], cfg["act_dim"]
        self.actor = np.array(actor, np.float32); self.critic = np.array(critic, np.float32)
        self.actor_t = self.actor.copy(); self.critic_t = self.critic.copy()                   # ddpg.jl:53-54
        self.opt_a = Adam(self.actor.size, net_sizes(D, A), cfg["lr"]); self.opt_c = Adam(self.critic.size, net_sizes(D + A, 1), cfg["lr"])
        self.rb = Ring(D, A, cfg["buffer_size"])
        self.global_step = 0; self.n_updates = 0; self.losses = []; self.episodes = []
        self.actor_loss = self.critic_loss = 0.0
        self.episode_return = 0.0; self.episode_length = 0

    def act(self, obs):
        """ddpg.jl:79 for step global_step + 1"""
        c = self.c; g = self.global_step + 1; comps = np.arange(c["act_dim"])
        if g <= c["warmup_steps"]:
            return c["act_low"] + (c["act_high"] - c["act_low"]) * uniform(c["seed"], comps, g, S_WARMUP)
        y = actor_mean(self.actor, c["obs_dim"], c["act_dim"], obs)[:, 0]
        return y + normal(c["seed"], comps, g, S_BEHAVE) * c["exploration_noise"]

    def observe(self, obs, action, reward, next_obs, terminal):
        c = self.c
        self.global_step += 1
        self.rb.add(obs, action, reward, next_obs, terminal)                                   # :83-90
        if self.global_step > c["min_buff_size"] and self.global_step > c["warmup_steps"]:    # :105
            self.update()

    def update(self):
        c = self.c; D, A, g = c["obs_dim"], c["act_dim"], self.global_step; comps = np.arange(A)
        batch = self.rb.gather(sample_indices(c["seed"], g, self.rb.size, c["batch_size"]))    # :106
        on = 1.0 if c["noise_in_update"] else 0.0
        noise_t = normal(c["seed"], comps, g, S_TARGET) * c["exploration_noise"] * on
        noise_a = normal(c["seed"], comps, g, S_ACTOR) * c["exploration_noise"] * on
        td = td_target(self.actor_t, self.critic_t, D, A, batch, c["gamma"], noise_t)
        self.critic_loss, gc = critic_loss_grad(self.critic, D, A, batch, td)
        self.critic = self.opt_c.step(self.critic, gc)                                         # :118
        self.actor_loss, ga = actor_loss_grad(self.actor, self.critic, D, A, batch, noise_a)
        self.actor = self.opt_a.step(self.actor, ga)                                           # :125
        self.actor_t = polyak(self.actor_t, self.actor, c["tau"])                              # :128-129
        self.critic_t = polyak(self.critic_t, self.critic, c["tau"])
        self.n_updates += 1
        if g % c["log_frequency"] == 0:                                                        # :131-133
            self.losses.append((g, float(self.actor_loss), float(self.critic_loss)))

    def run_transitions(self, transitions):
        """the transition-fed loop: (obs, action, reward, next_obs, terminal) tuples"""
        for tr in transitions:
            self.observe(*tr)

    def run_pendulum(self, n_steps):
        """the Pendulum-driven loop (ddpg.jl:74-135); the first call resets the env with stream 0x15"""
        c = self.c
        if not hasattr(self, "th"):
            self.th, self.thd = pendulum_reset(c["seed"], 0, S_RESET0); self.t = 0
        taken = 0
        while taken < n_steps and self.global_step < c["total_timesteps"]:
            obs = pendulum_obs(self.th, self.thd)
            a = self.act(obs)
            self.th, self.thd, self.t, r, term = pendulum_step(self.th, self.thd, self.t, a[0], c["max_steps"])
            g = self.global_step + 1
            self.episode_return += r; self.episode_length += 1
            nxt = pendulum_obs(self.th, self.thd)
            if term:
                self.episodes.append((float(self.episode_return), self.episode_length, g))
                self.episode_return = 0.0; self.episode_length = 0
                self.th, self.thd = pendulum_reset(c["seed"], g, S_RESET); self.t = 0
            self.observe(obs, a, r, nxt, term)
            taken += 1
        return taken
