"""Float64 numpy restatement of SAC as the library runs it (the crl_sac_* block of include/cleanrl_hip.h): the yardstick of tests/test_sac_cpu.py and
tests/test_gpu_sac.py. Written from the header's description — not from the kernels — on top of tests/ddpg_ref.py: dense layers, tanh_fast, the
critic's forward and gradient, Adam, polyak, the ring, the sampler and observe() are that module's, reached through it, and every exp / log is
ddpg_ref's numpy (R.np), so an instrument that patches ddpg_ref (the jitter of ddpg_bar) reaches SAC too.

Every step of the update that SAC adds is a module-level function of its own, so that tests/sac_bar.py can replace exactly one of them."""
import numpy as np

import ddpg_ref as R

S_NEXT, S_PI = 0x18, 0x19                   # the ε of the next action (critic pass) and of the actor pass
LOG_STD_MIN, LOG_STD_HALF_SPAN = -5.0, 3.5  # log_std = −5 + 3.5·(tanh_fast(s) + 1) ∈ [−5, 2]
HALF_LOG_2PI = 0.9189385332046727
SQUASH_EPS = 1e-6


def param_count(obs_dim, act_dim):
    return sum(R.net_sizes(obs_dim, 2 * act_dim)), sum(R.net_sizes(obs_dim + act_dim, 1))


def scale_bias(act_low, act_high):
    return (act_high - act_low) / 2.0, (act_high + act_low) / 2.0


def draws(seed, gstep, k, act_dim, stream):
    """ε(b, c): (act_dim, k) normals on `stream` at gstep, component word 16·b + c — one draw per sample and component"""
    comps = 16 * np.arange(k)[None, :] + np.arange(act_dim)[:, None]
    return R.normal(seed, comps, gstep, stream)


def actor_stream():
    return S_PI


def next_obs(batch):
    return batch["next_state"]


def actor_head(p, obs_dim, act_dim, X):
    """→ (h1, h2, z): the two tanh_fast layers and the LINEAR head, (2·act_dim, k)"""
    W1, b1, W2, b2, W3, b3 = R.split(p, obs_dim, 2 * act_dim)
    h1 = R.tanh_fast64(R.dense(W1, b1, X)); h2 = R.tanh_fast64(R.dense(W2, b2, h1))
    return h1, h2, R.dense(W3, b3, h2)


def head_rows(z, act_dim):
    """(μ, s): head rows 0..A−1 and A..2A−1"""
    return z[:act_dim], z[act_dim:]


def squash_term(y, scale):
    return R.np.log(scale * (1.0 - y * y) + SQUASH_EPS)


def log_prob(eps, log_std, y, scale):
    """Σ_c [((−0.5·ε² − log_std) − 0.5·log 2π) − log(scale·(1 − y²) + 1e-6)], c ascending from 0.0"""
    terms = ((-0.5 * (eps * eps) - log_std) - HALF_LOG_2PI) - squash_term(y, scale)
    acc = np.zeros(terms.shape[1], np.float64)
    for c in range(terms.shape[0]):
        acc = acc + terms[c]
    return acc


def sample(actor, obs_dim, act_dim, X, eps, scale, bias):
    h1, h2, z = actor_head(actor, obs_dim, act_dim, X)
    mu, s = head_rows(z, act_dim)
    t = R.tanh_fast64(s)
    log_std = LOG_STD_MIN + LOG_STD_HALF_SPAN * (t + 1.0)
    sigma = R.np.exp(log_std)
    y = R.tanh_fast64(mu + sigma * eps)
    return dict(h1=h1, h2=h2, mu=mu, t=t, log_std=log_std, sigma=sigma, y=y, a=scale * y + bias, logp=log_prob(eps, log_std, y, scale))


def mean_action(actor, obs_dim, act_dim, X, scale, bias):
    """the deterministic action scale·tanh_fast(μ) + bias, (act_dim, n)"""
    z = actor_head(actor, obs_dim, act_dim, np.asarray(X, np.float64).reshape(obs_dim, -1, order="F"))[2]
    return scale * R.tanh_fast64(z[:act_dim]) + bias


def min_q(q1, q2):
    return np.where(q2 < q1, q2, q1)


def entropy_term(alpha, logp):
    return alpha * logp


def td_target(reward, gamma, terminal, q1, q2, alpha, logp):
    return reward + (gamma * (1.0 - terminal.astype(np.float64))) * (min_q(q1, q2) - entropy_term(alpha, logp))


def grad_critic(q1, q2):
    """per sample: does the actor gradient run through critic 2?"""
    return q2 < q1


def direct_term(ak):
    """∂(α·logπ/k)/∂log_std read off the −log_std term of logπ: −α/k"""
    return ak


def critic_action_grad(critic, obs_dim, act_dim, g1, g2, k):
    """∂(−Q/k)/∂a through one critic: ddpg_ref.actor_loss_grad's pullback (cotangent −1/k, δ2, δ1, then Σ_i W1[i, D + c]·δ1[i], i ascending)"""
    C1, _, C2, _, C3, _ = R.split(critic, obs_dim + act_dim, 1)
    dq = np.full(k, -1.0 / k)
    e2 = np.where(g2 > 0.0, C3[0][:, None] * dq[None, :], 0.0)
    t1 = np.zeros((R.H, k))
    for j in range(R.H):
        t1 += C2[j, :][:, None] * e2[j:j + 1, :]
    e1 = np.where(g1 > 0.0, t1, 0.0)
    ga = np.zeros((act_dim, k))
    for i in range(R.H):
        ga += C1[i, obs_dim:][:, None] * e1[i:i + 1, :]
    return ga


def actor_pass(actor, critic1, critic2, obs_dim, act_dim, batch, eps, alpha, scale, bias):
    """→ (logπ (k), qmin (k), the gradient of mean(α·logπ − qmin) with respect to the actor: Float64, flat, before the Float32 projection, stats)"""
    X = batch["state"]; k = X.shape[1]
    W1, b1, W2, b2, W3, b3 = R.split(actor, obs_dim, 2 * act_dim)
    s = sample(actor, obs_dim, act_dim, X, eps, scale, bias)
    Xc = np.vstack([X, s["a"]])
    g11, g12, q1 = R.critic_forward(critic1, obs_dim + act_dim, Xc)
    g21, g22, q2 = R.critic_forward(critic2, obs_dim + act_dim, Xc)
    ga = np.where(grad_critic(q1, q2)[None, :], critic_action_grad(critic2, obs_dim, act_dim, g21, g22, k),
                  critic_action_grad(critic1, obs_dim, act_dim, g11, g12, k))
    y, h1, h2 = s["y"], s["h1"], s["h2"]
    ak = alpha / k
    omy = 1.0 - y * y
    den = scale * omy + SQUASH_EPS
    dy = ga * scale + ak * ((2.0 * scale * y) / den)
    du = dy * omy
    dls = du * (s["sigma"] * eps) - direct_term(ak)
    ds = (dls * LOG_STD_HALF_SPAN) * (1.0 - s["t"] * s["t"])
    d3 = np.vstack([du, ds])
    s2 = np.zeros((R.H, k))
    for r in range(2 * act_dim):
        s2 += W3[r, :][:, None] * d3[r:r + 1, :]
    d2 = s2 * (1.0 - h2 * h2)
    t1 = np.zeros((R.H, k))
    for j in range(R.H):
        t1 += W2[j, :][:, None] * d2[j:j + 1, :]
    d1 = t1 * (1.0 - h1 * h1)
    gs = [R._sum_samples(d1[:, None, :] * X[None, :, :]), R._sum_samples(d1), R._sum_samples(d2[:, None, :] * h1[None, :, :]), R._sum_samples(d2),
          R._sum_samples(d3[:, None, :] * h2[None, :, :]), R._sum_samples(d3)]
    return s["logp"], min_q(q1, q2), R._flat(gs), s, q1 - q2


def actor_loss(alpha, logp, qmin):
    return R._sum_samples(alpha * logp - qmin) / logp.size


def alpha_loss(alpha, logp, target_entropy):
    """−α·mean(logπ + target_entropy); its derivative with respect to log_alpha is the same expression"""
    return -(alpha * (R._sum_samples(logp + target_entropy) / logp.size))


def alpha_of(log_alpha):
    return R.np.exp(np.float64(log_alpha))


def alpha_due(autotune):
    return bool(autotune)


def reported_alpha(alpha_before, log_alpha_after):
    """the α that actor_loss, alpha_loss and the alpha record carry: the one the update's passes used"""
    return alpha_before


def polyak_sources(agent):
    """what the critic targets are mixed with: the critics after this update's step"""
    return agent.critic, agent.critic2


class SAC(R.DDPG):
    """cfg: ddpg_ref.DDPG's dict (noise_in_update = 0; exploration_noise is not read) plus autotune, alpha, target_entropy"""

    def __init__(self, cfg, actor, critic1, critic2):
        super().__init__(cfg, actor, critic1)
        assert not cfg["noise_in_update"] and cfg["alpha"] > 0 and cfg["autotune"] in (0, 1)
        D, A = cfg["obs_dim"], cfg["act_dim"]
        assert self.actor.size == param_count(D, A)[0]
        self.opt_a = R.Adam(self.actor.size, R.net_sizes(D, 2 * A), cfg["lr"])
        self.critic2 = np.array(critic2, np.float32); self.critic2_t = self.critic2.copy()
        self.opt_c2 = R.Adam(self.critic2.size, R.net_sizes(D + A, 1), cfg["lr"])
        self.log_alpha = np.array([np.log(cfg["alpha"])], np.float32)
        self.opt_alpha = R.Adam(1, [1, 0, 0, 0, 0, 0], cfg["lr"])
        self.scale, self.bias = scale_bias(cfg["act_low"], cfg["act_high"])
        self.alpha, self.alpha_loss, self.entropy = float(cfg["alpha"]), 0.0, 0.0
        self.alpha_records = []
        del self.actor_t                                                                      # there is no target actor
        # what the squash met, over both passes of every update, for the tests that need an edge to have been met
        self.n_samples = self.n_y_one = self.n_y_near = self.n_ls_low = self.n_ls_high = 0
        self.min_q_gap = np.inf

    def _count(self, s):
        omy = 1.0 - s["y"] * s["y"]
        self.n_samples += omy.size; self.n_y_one += int((omy == 0.0).sum()); self.n_y_near += int(((omy < SQUASH_EPS) & (omy > 0.0)).sum())
        self.n_ls_low += int((s["log_std"] < LOG_STD_MIN + 1e-3).sum()); self.n_ls_high += int((s["log_std"] > 2.0 - 1e-3).sum())

    def act(self, obs):
        """the action of step global_step + 1: rand(act_space) during the warm-up, then a sample with ε on stream 0x10, component c"""
        c = self.c; g = self.global_step + 1; comps = np.arange(c["act_dim"])
        if g <= c["warmup_steps"]:
            return c["act_low"] + (c["act_high"] - c["act_low"]) * R.uniform(c["seed"], comps, g, R.S_WARMUP)
        eps = R.normal(c["seed"], comps, g, R.S_BEHAVE)[:, None]
        X = np.asarray(obs, np.float64).reshape(c["obs_dim"], 1)
        return sample(self.actor, c["obs_dim"], c["act_dim"], X, eps, self.scale, self.bias)["a"][:, 0]

    def update(self):
        c = self.c; D, A, g, k = c["obs_dim"], c["act_dim"], self.global_step, c["batch_size"]
        batch = self.rb.gather(R.sample_indices(c["seed"], g, self.rb.size, k))
        alpha = alpha_of(self.log_alpha[0])
        # next action, TD target
        nxt = sample(self.actor, D, A, next_obs(batch), draws(c["seed"], g, k, A, S_NEXT), self.scale, self.bias)
        self._count(nxt)
        Xn = np.vstack([batch["next_state"], nxt["a"]])
        q1 = R.critic_forward(self.critic_t, D + A, Xn)[2]; q2 = R.critic_forward(self.critic2_t, D + A, Xn)[2]
        td = td_target(batch["reward"], c["gamma"], batch["terminal"], q1, q2, alpha, nxt["logp"])
        # both critics
        loss1, g1 = R.critic_loss_grad(self.critic, D, A, batch, td)
        loss2, g2 = R.critic_loss_grad(self.critic2, D, A, batch, td)
        self._pre = (self.critic, self.critic2)
        self.critic = self.opt_c.step(self.critic, g1)
        self.critic2 = self.opt_c2.step(self.critic2, g2)
        self.critic_loss = loss1 + loss2
        # the actor, through the updated critics
        logp, qmin, ga, smp, gap = actor_pass(self.actor, self.critic, self.critic2, D, A, batch, draws(c["seed"], g, k, A, actor_stream()), alpha,
                                              self.scale, self.bias)
        self._count(smp)
        self.min_q_gap = min(self.min_q_gap, float(np.abs(gap).min()))
        self.actor = self.opt_a.step(self.actor, ga)
        # the temperature
        if alpha_due(c["autotune"]):
            self.log_alpha = self.opt_alpha.step(self.log_alpha, np.array([alpha_loss(alpha, logp, c["target_entropy"])]))
        rep = reported_alpha(alpha, self.log_alpha[0])
        self.alpha = float(rep)
        self.actor_loss = actor_loss(rep, logp, qmin)
        self.alpha_loss = alpha_loss(rep, logp, c["target_entropy"])
        self.entropy = -(R._sum_samples(logp) / k)
        # the targets, every update
        s1, s2 = polyak_sources(self)
        self.critic_t = R.polyak(self.critic_t, s1, c["tau"]); self.critic2_t = R.polyak(self.critic2_t, s2, c["tau"])
        self.n_updates += 1
        if g % c["log_frequency"] == 0:
            self.losses.append((g, float(self.actor_loss), float(self.critic_loss)))
            self.alpha_records.append((g, self.alpha, float(self.alpha_loss), float(self.entropy)))

    def params(self):
        return (self.actor, self.critic, self.critic2, self.critic_t, self.critic2_t)
