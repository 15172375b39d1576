"""crl_norm (csrc/norm.hip) against the Float64 restatement tests/norm_ref.py on its fixed-seed tapes. The statistics are held to
profiles/norm_bar.json (scripts/norm_bar.py: 16 x the measured spread of tile-wise merges), the outputs to one Float32 ulp of the reference's Float32
values, the raw episode aggregate to 1e-12; a second object on the same tape, frozen statistics and the copy-through options bit for bit."""
import json
import os

import numpy as np
import pytest

import hipmem
import norm_ref as R
import ppo_gauss_ref as G
from test_gpu_eval import limit
from test_gpu_parity import crl  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "norm_bar.json")) as _f:
    BAR = json.load(_f)


class Dev:
    """one Normalizer with device buffers of its own; reset / step return host copies of what the device wrote"""

    def __init__(self, crl, N, D, **kw):   # noqa: F811
        self.n, self.N, self.D = crl._lib.Normalizer(crl._lib.NormOptions(N, D, **kw)), N, D
        self.oi, self.oo, self.ri, self.ro, self.dn = (hipmem.Buf(b) for b in (4 * N * D, 4 * N * D, 4 * N, 4 * N, N))

    def reset(self, obs, update=True):
        self.n.reset_device(self.oi.put(np.asfortranarray(obs)), self.oo, update)
        return self.oo.get(np.float32, (self.D, self.N))

    def step(self, obs, reward, done, update=True):
        self.n.step_device(self.oi.put(np.asfortranarray(obs)), self.ri.put(reward), self.dn.put(done), self.oo, self.ro, update)
        return self.oo.get(np.float32, (self.D, self.N)), self.ro.get(np.float32)


def within_ulp(got, want):
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))))


def stat_err(got, want, D):
    def parts(s): return np.r_[s[0], s[2 * D + 1]], np.r_[s[1:1 + D], s[2 * D + 2]], np.r_[s[1 + D:1 + 2 * D], s[2 * D + 3]]
    (cg, mg, vg), (cw, mw, vw) = parts(got), parts(want)
    return max(np.max(np.abs(cg - cw) / cw), np.max(np.abs(mg - mw) / (np.abs(mw) + np.sqrt(vw)))), np.max(np.abs(vg - vw) / vw)


@pytest.mark.parametrize("N,D", R.CASES)
def test_statistics_outputs_and_books_follow_the_restatement(crl, N, D):   # noqa: F811
    obs, reward, done = R.tape(N, D)
    ref, a, b = R.Ref(N, D), Dev(crl, N, D), Dev(crl, N, D)
    lo = hi = rclip = False
    with limit(120):
        for s in range(-1, R.STEPS):
            if s < 0:
                want, got, twin = (ref.reset(obs[0]),), (a.reset(obs[0]),), (b.reset(obs[0]),)
            else:
                want, got, twin = (x.step(obs[s + 1], reward[s], done[s]) for x in (ref, a, b))
                rclip |= bool(np.any(np.abs(want[1]) == 10.0))
            lo |= bool(np.any(want[0] == -10.0)); hi |= bool(np.any(want[0] == 10.0))
            st = a.n.state()
            e = stat_err(st, ref.state(), D)
            print(f"frame {s + 1}: mean {e[0]:.2e} (bar {BAR['bar_mean']:.2e}) var {e[1]:.2e} (bar {BAR['bar_var']:.2e})")
            assert e[0] <= BAR["bar_mean"] and e[1] <= BAR["bar_var"]
            assert all(within_ulp(g, w) for g, w in zip(got, want))
            assert all(g.tobytes() == t.tobytes() for g, t in zip(got, twin)) and st.tobytes() == b.n.state().tobytes()
            ag, aw = a.n.episode_stats(clear=False), ref.agg
            assert ag["episodes"] == aw["episodes"] and ag["length_sum"] == aw["length_sum"]
            assert all(abs(ag[k] - aw[k]) <= 1e-12 * abs(aw[k]) for k in ("return_sum", "return_max"))
    # the tape did what it is for: some and all envs done, the reward clip, and (where a dimension carries outliers) both observation clips
    assert done[R.ALL_DONE].all() and (N == 1 or any(0 < d.sum() < N for d in done)) and rclip and (D < 4 or (lo and hi))
    assert a.n.episode_stats()["episodes"] == done.sum() and a.n.episode_stats()["episodes"] == 0


def test_frozen_statistics_shared_state_and_copy_through(crl):   # noqa: F811
    N, D = 257, 17
    obs, reward, done = R.tape(N, D)
    ref, a = R.Ref(N, D), Dev(crl, N, D)
    with limit(120):
        ref.reset(obs[0]); a.reset(obs[0])
        for s in range(2):
            ref.step(obs[s + 1], reward[s], done[s]); a.step(obs[s + 1], reward[s], done[s])
        st = a.n.state()
        b = Dev(crl, N, D); b.n.load_state(st)
        for s in range(2, 4):                                    # frozen: the state keeps its bits, the outputs follow the frozen reference
            want, got, twin = (x.step(obs[s + 1], reward[s], done[s], update=False) for x in (ref, a, b))
            assert a.n.state().tobytes() == st.tobytes() and all(within_ulp(g, w) for g, w in zip(got, want))
            assert got[0].tobytes() == twin[0].tobytes() and got[1].tobytes() == twin[1].tobytes()   # a fresh object with the written state
        for kw in (dict(norm_obs=False), dict(norm_reward=False)):
            c, cref = Dev(crl, N, D, **kw), R.Ref(N, D, **kw)
            o, r = c.step(obs[1], reward[0], done[0]); ow, rw = cref.step(obs[1], reward[0], done[0])
            assert (o.tobytes() == obs[1].tobytes()) == ("norm_obs" in kw) and (r.tobytes() == reward[0].tobytes()) == ("norm_reward" in kw)
            assert within_ulp(o, ow) and within_ulp(r, rw) and c.n.episode_stats()["episodes"] == done[0].sum()


def test_ppo_trains_through_a_normalized_env(crl):   # noqa: F811
    cfg = crl.PPOConfig(num_envs=64, num_steps=8, total_timesteps=64 * 8 * 2)
    env = crl.NormalizedEnv(crl.LibraryEnv("pendulum", 64))
    with limit(120):
        p1 = crl.ppo_continuous(cfg, env=env, hidden=64, episode_records=0)
        st = env.state()
        crl.ppo(cfg, env=crl.NormalizedEnv(crl.LibraryEnv("cartpole", 64), norm_reward=False), hidden=64, episode_records=0)
    p0, off = crl._lib.make_actor_critic_gaussian_host(3, 1, 64, crl.GaussianOptions(), seed=0), G.offsets(3, 1, 64)
    assert np.all(np.isfinite(p1)) and all(np.any(p1[off[i]:off[i + 1]] != p0[off[i]:off[i + 1]]) for i in range(12))
    assert st[0] == pytest.approx(1e-4 + 64 * (1 + 16), rel=1e-12) and st[2 * 3 + 1] == pytest.approx(1e-4 + 64 * 16, rel=1e-12)
    env.close()
