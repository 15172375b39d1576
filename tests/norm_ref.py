"""Float64 numpy restatement of the "Running normalisation" block of include/cleanrl_hip.h (crl_norm), written from the header, and the fixed-seed
tapes tests/test_gpu_norm.py and scripts/norm_bar.py share. Batch moments are whole-batch np.mean / np.var unless another `moments` is passed."""
import numpy as np

CASES = [(1, 1), (255, 3), (256, 64), (257, 17), (600, 64)]   # one env; one ragged tile; a full tile; the first env of a second; a ragged third, D ∤ 256
STEPS, ALL_DONE = 6, 3


def whole(x):
    return [(x.shape[-1], x.mean(-1), x.var(-1))]


def tiled(T, reverse=False, sumsq=False):
    """moments tile by tile (merged in the order returned); sumsq: E[x²] − mean², the variant that must NOT pass"""
    def f(x):
        parts = [x[..., i:i + T] for i in range(0, x.shape[-1], T)]
        var = (lambda p: (p * p).mean(-1) - p.mean(-1) ** 2) if sumsq else (lambda p: p.var(-1))
        return [(p.shape[-1], p.mean(-1), var(p)) for p in (parts[::-1] if reverse else parts)]
    return f


def merge(count, mean, var, n_b, mean_b, var_b):
    delta, tot = mean_b - mean, count + n_b
    m2 = var * count + var_b * n_b + delta * delta * count * n_b / tot
    return tot, mean + delta * n_b / tot, m2 / tot


class Ref:
    def __init__(self, N, D, norm_obs=True, norm_reward=True, gamma=0.99, eps=1e-8, clip_obs=10.0, clip_reward=10.0, moments=whole):
        self.o = (1e-4, np.zeros(D), np.ones(D)); self.r = (1e-4, 0.0, 1.0)
        self.acc, self.ep_ret, self.ep_len = np.zeros(N), np.zeros(N), np.zeros(N)
        self.agg = dict(episodes=0.0, return_sum=0.0, length_sum=0.0, return_max=0.0)
        self.norm_obs, self.norm_reward, self.gamma, self.eps, self.clip = norm_obs, norm_reward, gamma, eps, (clip_obs, clip_reward)
        self.moments = moments

    def _merge(self, stat, x):
        for part in self.moments(x):
            stat = merge(*stat, *part)
        return stat

    def _obs(self, obs, update):
        if not self.norm_obs:
            return obs.copy()
        if update:
            self.o = self._merge(self.o, obs.astype(np.float64))
        y = (obs.astype(np.float64) - self.o[1][:, None]) / np.sqrt(self.o[2][:, None] + self.eps)
        return np.clip(y, -self.clip[0], self.clip[0]).astype(np.float32)

    def reset(self, obs, update=True):
        self.acc[:] = 0; self.ep_ret[:] = 0; self.ep_len[:] = 0
        return self._obs(obs, update)

    def step(self, obs, reward, done, update=True):
        out, r = self._obs(obs, update), reward.astype(np.float64)
        rout = reward.copy()
        if self.norm_reward:
            self.acc = self.acc * self.gamma + r
            if update:
                self.r = self._merge(self.r, self.acc)
            rout = np.clip(r / np.sqrt(self.r[2] + self.eps), -self.clip[1], self.clip[1]).astype(np.float32)
        self.ep_ret += r; self.ep_len += 1
        for e in np.flatnonzero(done):                           # envs in index order
            a = self.agg
            a["return_max"] = self.ep_ret[e] if a["episodes"] == 0 else max(a["return_max"], self.ep_ret[e])
            a["episodes"] += 1; a["return_sum"] += self.ep_ret[e]; a["length_sum"] += self.ep_len[e]
        self.ep_ret[done != 0] = 0; self.ep_len[done != 0] = 0; self.acc[done != 0] = 0
        return out, rout

    def state(self):
        return np.concatenate([[self.o[0]], self.o[1], self.o[2], self.r])


def tape(N, D, seed=7):
    """obs (STEPS + 1, D, N) Float32 (frame 0 is the reset), reward (STEPS, N), done (STEPS, N). Dimensions cycle through N(0, 1); mean 1e4 with std 1e-2;
    a constant; N(0, 1) with ±50σ outliers in the last two frames. Rewards in −16 … 0 with two of magnitude 1e3; done with p = 0.2, all envs at ALL_DONE."""
    rng = np.random.default_rng(seed + 1000 * N + D)
    obs = rng.standard_normal((STEPS + 1, D, N))
    obs[:, 1::4] = 1e4 + 1e-2 * obs[:, 1::4]
    obs[:, 2::4] = 3.5
    for f in (STEPS - 1, STEPS):
        obs[f, 3::4, :2] = 50.0; obs[f, 3::4, -2:] = -50.0
    reward = -16.0 * rng.random((STEPS, N))
    reward[2, 0] = -1e3; reward[4, N - 1] = 1e3
    done = (rng.random((STEPS, N)) < 0.2).astype(np.uint8)
    done[ALL_DONE] = 1
    return obs.astype(np.float32), reward.astype(np.float32), done


def run(ref, obs, reward, done):
    """the tape through `ref`: the state after the reset and after every step, and the outputs"""
    outs, states = [(ref.reset(obs[0]), None)], [ref.state()]
    for s in range(STEPS):
        outs.append(ref.step(obs[s + 1], reward[s], done[s])); states.append(ref.state())
    return states, outs
