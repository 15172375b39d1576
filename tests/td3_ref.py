"""Float64 numpy restatement of TD3 as the library runs it (the crl_td3_* block of include/cleanrl_hip.h): the yardstick of tests/test_td3_cpu.py and
tests/test_gpu_td3.py. Written from the header's description — not from the kernels — on top of tests/ddpg_ref.py: forwards, gradients, Adam,
polyak, the ring, the sampler, act() and observe() are that module's, reached through it (so an instrument that patches ddpg_ref reaches TD3 too).

Every step of the update that TD3 adds is a module-level function of its own, so that tests/td3_bar.py can replace exactly one of them."""
import numpy as np

import ddpg_ref as R

S_SMOOTH = 0x17


def clamp(x, lo, hi):
    """x < lo ? lo : (x > hi ? hi : x)"""
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def smoothing_draws(seed, gstep, k, act_dim):
    """z(b, c): (act_dim, k) normals on stream 0x17 at gstep, component word 16·b + c — one draw per sample and component"""
    comps = 16 * np.arange(k)[None, :] + np.arange(act_dim)[:, None]
    return R.normal(seed, comps, gstep, S_SMOOTH)


def smoothing_noise(z, policy_noise, noise_clip):
    return clamp(policy_noise * z, -noise_clip, noise_clip)


def target_action(y3, noise, act_low, act_high):
    return clamp(y3 * 2.0 + noise, act_low, act_high)


def next_q(q1, q2):
    return np.where(q2 < q1, q2, q1)


def actor_due(gstep, policy_delay):
    return gstep % policy_delay == 0


def targets_due(gstep, policy_delay):
    return gstep % policy_delay == 0


def critic2_cotangent_td(td, critic1, critic2, obs_dim, act_dim, batch):
    """the TD target critic 2's loss sees: the shared one"""
    return td


def critic2_step(agent, grad):
    """critic 2's Adam step, with its own moments and β powers"""
    return agent.opt_c2.step(agent.critic2, grad)


def actor_loss_critic(agent):
    """the critic the actor loss runs through: the updated critic 1"""
    return agent.critic


def polyak_targets(agent, tau):
    """the three target updates of a due step: polyak_update! of the actor's and of both critics' targets, every element"""
    agent.actor_t = R.polyak(agent.actor_t, agent.actor, tau)
    agent.critic_t = R.polyak(agent.critic_t, agent.critic, tau)
    agent.critic2_t = R.polyak(agent.critic2_t, agent.critic2, tau)


class TD3(R.DDPG):
    """cfg: ddpg_ref.DDPG's dict (noise_in_update = 0) plus policy_delay, policy_noise, noise_clip"""

    def __init__(self, cfg, actor, critic1, critic2):
        super().__init__(cfg, actor, critic1)
        assert not cfg["noise_in_update"] and cfg["policy_delay"] >= 1 and cfg["policy_noise"] >= 0 and cfg["noise_clip"] >= 0
        D, A = cfg["obs_dim"], cfg["act_dim"]
        self.critic2 = np.array(critic2, np.float32); self.critic2_t = self.critic2.copy()
        self.opt_c2 = R.Adam(self.critic2.size, R.net_sizes(D + A, 1), cfg["lr"])
        self.n_actor_steps = 0
        # what the target smoothing did, for the tests that need an edge to have been met: draws, draws the noise clip cut, target actions,
        # target actions the action bounds cut
        self.n_noise = self.n_noise_clipped = self.n_target_actions = self.n_target_clamped = 0

    def update(self):
        c = self.c; D, A, g, k = c["obs_dim"], c["act_dim"], self.global_step, c["batch_size"]
        batch = self.rb.gather(R.sample_indices(c["seed"], g, self.rb.size, k))
        # target action, TD target
        z = smoothing_draws(c["seed"], g, k, A)
        raw = c["policy_noise"] * z
        noise = smoothing_noise(z, c["policy_noise"], c["noise_clip"])
        y3 = R.actor_forward(self.actor_t, D, A, batch["next_state"])[2]
        a2 = target_action(y3, noise, c["act_low"], c["act_high"])
        self.n_noise += raw.size; self.n_noise_clipped += int((np.abs(raw) > c["noise_clip"]).sum())
        free = y3 * 2.0 + noise
        self.n_target_actions += free.size; self.n_target_clamped += int(((free < c["act_low"]) | (free > c["act_high"])).sum())
        Xn = np.vstack([batch["next_state"], a2])
        q1 = R.critic_forward(self.critic_t, D + A, Xn)[2]; q2 = R.critic_forward(self.critic2_t, D + A, Xn)[2]
        td = batch["reward"] + c["gamma"] * next_q(q1, q2) * (1.0 - batch["terminal"].astype(np.float64))
        # both critics, every update
        loss1, g1 = R.critic_loss_grad(self.critic, D, A, batch, td)
        loss2, g2 = R.critic_loss_grad(self.critic2, D, A, batch, critic2_cotangent_td(td, self.critic, self.critic2, D, A, batch))
        self.critic = self.opt_c.step(self.critic, g1)
        self.critic2 = critic2_step(self, g2)
        self.critic_loss = loss1 + loss2
        # the delayed actor and targets
        if actor_due(g, c["policy_delay"]):
            self.actor_loss, ga = R.actor_loss_grad(self.actor, actor_loss_critic(self), D, A, batch, np.zeros(A))
            self.actor = self.opt_a.step(self.actor, ga)
            self.n_actor_steps += 1
        if targets_due(g, c["policy_delay"]):
            polyak_targets(self, c["tau"])
        self.n_updates += 1
        if g % c["log_frequency"] == 0:
            self.losses.append((g, float(self.actor_loss), float(self.critic_loss)))

    def params(self):
        return (self.actor, self.critic, self.critic2, self.actor_t, self.critic_t, self.critic2_t)
