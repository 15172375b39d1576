"""Device-resident external envs on a Gaussian handle (csrc/extenv.hip, ext_act_kernel<H, ExtHeadGauss>) against the Float64 restatement
tests/ppo_gauss_ref.py on the pinned xi stream. Bars: those of tests/test_gpu_ppo_gauss.py — RTOL with its floors on actions, logprob and value,
profiles/ppo_gauss_bar.json's xi_bar on the recovered xi. Copies and bookkeeping are compared bit for bit."""
import sys

import numpy as np
import pytest

import hipmem
import ppo_gauss_ref as G
from test_gpu_eval import limit
from test_gpu_extenv import _same_bits
from test_gpu_ppo_gauss import BAR, RTOL, HostEnv, crl, rel_err, rel_err_s  # noqa: F401  (crl is the module fixture)

pytestmark = pytest.mark.gpu
SEED, OFFSET, K, STEP, GUARD = 0x5EED, 1000, 4, 2, 16


def _agent(crl, nt, D, ad, Hd, k=K, env_kind=None, **kw):   # noqa: F811
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, num_minibatches=1, total_timesteps=nt * k * 10)
    return crl.Agent(cfg, action="gaussian", gaussian=crl.GaussianOptions(G.LO, G.HI, 0.0), obs_dim=D, n_act=ad, hidden=Hd,
                     env_kind=crl._lib.ENV_EXTERNAL if env_kind is None else env_kind, **({"seed": SEED} | kw))


# head 2 / 6 / 16 = AMAX; a partial tile; W1 streamed from the parameters (64 / 8 / 256); one env; two pairs per thread (hidden 64, act_dim 8); iteration > 0
ACT_CASES = [(1, 3, 64, 96, 0), (3, 8, 256, 64, 2), (8, 17, 128, 33, 0), (8, 64, 256, 37, 1), (4, 16, 256, 1, 0), (8, 3, 64, 40, 0)]


@pytest.mark.parametrize("ad,D,Hd,nt,iteration", ACT_CASES)
def test_act_device_gaussian_matches_restatement(crl, ad, D, Hd, nt, iteration):   # noqa: F811
    F = crl._lib; p = G.spread_params(F, D, ad, Hd, 7)
    agent = _agent(crl, nt, D, ad, Hd, params=p, env_id_offset=OFFSET)
    h, rng = agent.handle, np.random.default_rng(nt + D)
    obs = np.asfortranarray(rng.standard_normal((D, nt)).astype(np.float32)); done = (rng.random(nt) < 0.3).astype(np.uint8)
    o_d, d_d, r_d = hipmem.upload(obs), hipmem.upload(done), hipmem.upload(rng.random(nt).astype(np.float32))
    act_d = hipmem.Buf(4 * (ad * nt + GUARD))
    with limit(120):
        for _ in range(iteration):                               # the iteration counter moves by crl_ppo_update only
            for s in range(K):
                h.act_device_gaussian(s, o_d, d_d, act_d); h.record_device_gaussian(s, r_d, o_d, d_d)
            h.update(want_stats=False)
        agent.set_params(p)
        act_d.put(np.full(ad * nt + GUARD, -77.0, np.float32)); h.act_device_gaussian(STEP, o_d, d_d, act_d); h.sync()
    got = act_d.get(np.float32); a_g = got[:ad * nt].reshape(ad, nt, order="F")
    assert h.iteration == iteration and (got[ad * nt:] == -77.0).all(), "a word behind action_d was overwritten"
    slot = {f: h.read(getattr(F, f))[..., STEP] for f in ("F_OBS", "F_TERMINAL", "FIELD_ACTION_F", "F_LOGPROB", "F_VALUE")}
    agent.close()
    assert _same_bits(np.asfortranarray(slot["F_OBS"]), obs) and np.array_equal(slot["F_TERMINAL"], done) and _same_bits(np.asfortranarray(slot["FIELD_ACTION_F"]), a_g)
    (actor, critic), X = G.unpack(p, D, ad, Hd), obs.astype(np.float64)
    z = G.mlp(actor, X)[0]
    xi = G.rollout_xi(SEED, OFFSET + np.arange(nt), iteration * K + STEP, ad)
    a_o, lp_o = G.act(z, xi.astype(np.float64), ad, G.LO, G.HI)
    e_a, e_lp, e_v = rel_err_s(a_g, a_o), rel_err_s(slot["F_LOGPROB"], lp_o), rel_err(slot["F_VALUE"], G.mlp(critic, X)[0][0])
    e_xi = np.max(np.abs(G.logprob_entropy(z, a_g.astype(np.float64), ad, G.LO, G.HI)[2] - xi))
    print(f"action {e_a:.2e} logprob {e_lp:.2e} value {e_v:.2e} (bar {RTOL:.0e}); recovered xi {e_xi:.2e} (bar {BAR['xi_bar']:.2e})")
    assert e_a < RTOL and e_lp < RTOL and e_v < RTOL and e_xi < BAR["xi_bar"]


@pytest.mark.parametrize("Hd", [64, 256])
def test_update_reads_the_buffer_the_device_calls_left(crl, Hd):   # noqa: F811
    F, nt, k = crl._lib, 64, 8
    env = crl.LibraryEnv("pendulum", nt, seed=SEED)
    a, b = _agent(crl, nt, 3, 1, Hd, k=k), _agent(crl, nt, 3, 1, Hd, k=k)
    p0 = a.get_params(); b.set_params(p0)
    ha, hb, act_d = a.handle, b.handle, hipmem.Buf(4 * nt)
    with limit(120):
        obs, done = env.reset()
        for s in range(k):
            ha.act_device_gaussian(s, obs, done, act_d, peer_stream=env.stream)
            reward, obs, done = env.step(act_d)
            ha.record_device_gaussian(s, reward, obs, done, peer_stream=env.stream)
        fld = [ha.read(f) for f in (F.F_OBS, F.FIELD_ACTION_F, F.F_LOGPROB, F.F_REWARD, F.F_TERMINAL, F.F_VALUE)]
        for s in range(k):
            hb.rollout_store_gaussian(s, *[np.asfortranarray(x[..., s]) for x in fld])
        hb.write(F.F_CUR_OBS, ha.read(F.F_CUR_OBS)); hb.write(F.F_NEXT_DONE, ha.read(F.F_NEXT_DONE))
        sa, sb = ha.update(), hb.update()
    assert np.any(fld[3] != 0) and _same_bits(a.get_params(), b.get_params()) and np.any(a.get_params() != p0)
    assert len(sa) == len(sb) == 4 and all(np.float64(x[key]).tobytes() == np.float64(y[key]).tobytes() for x, y in zip(sa, sb) for key in x)
    a.close(); b.close(); env.close()


def test_env_step_device_gaussian_equals_env_step_gaussian_and_record_keeps_the_books(crl):   # noqa: F811
    F, nt, acts = crl._lib, G.PEND_ENVS, G.pendulum_actions()
    h1, h2 = [_agent(crl, nt, 3, 1, 64, env_kind=F.ENV_PENDULUM, seed=G.PEND_SEED, stale_obs=False).handle for _ in range(2)]
    rec = _agent(crl, nt, 3, 1, 64, k=G.PEND_STEPS, env_id_offset=OFFSET).handle; rec.episode_ring_enable(4096)
    obs_d, rew_d, done_d, act_d = hipmem.Buf(12 * nt), hipmem.Buf(4 * nt), hipmem.Buf(nt), hipmem.Buf(4 * nt)
    ep_ret, ep_len, want = np.zeros(nt, np.float32), np.zeros(nt, np.int32), []
    with limit(240):
        h1.env_reset(); h2.env_reset()
        rec.act_device_gaussian(0, hipmem.upload(h2.read(F.F_CUR_OBS)), hipmem.upload(h2.read(F.F_NEXT_DONE)), act_d)   # step 0 clears the statistics
        for g, a in enumerate(acts):
            o1, r1, d1 = h1.env_step_gaussian(a, g)
            h2.env_step_device_gaussian(hipmem.upload(a), g, obs_d, rew_d, done_d); h2.sync()
            assert _same_bits(o1, obs_d.get(np.float32, (3, nt))) and _same_bits(r1, rew_d.get(np.float32)) and np.array_equal(d1, done_d.get(np.uint8)), g
            rec.record_device_gaussian(g, rew_d, obs_d, done_d)
            ep_ret = ep_ret + r1; ep_len += 1                    # Float32 running sum in step order
            for e in np.flatnonzero(d1):
                want.append((g, OFFSET + int(e), float(ep_ret[e]), int(ep_len[e]))); ep_ret[e] = 0; ep_len[e] = 0
        st, (recs, total) = rec.episode_stats(), rec.episode_records()
    assert len(want) == 3 * nt == total == st["episodes"] and recs == sorted(want)
    assert st["return_sum"] == sum(w[2] for w in want) and st["length_sum"] == 200.0 * len(want) and st["return_max"] == max(w[2] for w in want)
    h1.close(); h2.close(); rec.close()


def test_errors_name_the_reason_and_leave_the_handle_usable(crl):   # noqa: F811
    F = crl._lib; d = crl.Agent(crl.PPOConfig(num_envs=8, num_steps=K), obs_dim=8, n_act=4, hidden=64, env_kind=F.ENV_EXTERNAL)
    b, dn, ac = hipmem.upload(np.zeros(64, np.float32)), hipmem.upload(np.zeros(8, np.uint8)), hipmem.Buf(4 * 2 * 8)
    for call in (lambda: d.handle.act_device_gaussian(0, b, b, b), lambda: d.handle.record_device_gaussian(0, b, b, b),
                 lambda: d.handle.env_step_device_gaussian(b, 0, None, b, b)):
        with pytest.raises(F.CrlError, match="needs a Gaussian handle"):
            call()
    d.handle.act_device(0, b, dn, ac); d.handle.sync(); d.close()
    g = _agent(crl, 8, 8, 2, 64)
    h, lib, p = g.handle, F.load(), b.data_ptr()
    for step in (-1, K):
        with pytest.raises(F.CrlError, match="crl_rollout_act_device_gaussian: step out of range"):
            h.act_device_gaussian(step, b, b, b)
        with pytest.raises(F.CrlError, match="crl_rollout_record_device_gaussian: step out of range"):
            h.record_device_gaussian(step, b, b, b)
    for call, name in ((lambda: lib.crl_rollout_act_device_gaussian(h._h, 0, p, None, p, None), "done_d"),
                       (lambda: lib.crl_rollout_record_device_gaussian(h._h, 0, p, None, p, None), "next_obs_d"),
                       (lambda: lib.crl_env_step_device_gaussian(h._h, p, 0, None, p, p, None), "CRL_ENV_PENDULUM")):
        assert call() != 0 and name in lib.crl_last_error().decode()
    h.act_device_gaussian(0, b, dn, ac); h.sync()
    assert np.all(np.isfinite(h.read(F.FIELD_ACTION_F)[..., 0]))
    g.close()


def test_ppo_continuous_on_a_device_resident_pendulum(crl, monkeypatch):   # noqa: F811
    cfg = crl.PPOConfig(num_envs=64, num_steps=8, total_timesteps=64 * 8 * 2)
    with limit(120):
        p1 = crl.ppo_continuous(cfg, env=crl.LibraryEnv("pendulum", 64), hidden=64, episode_records=0)
    p0, off = crl._lib.make_actor_critic_gaussian_host(3, 1, 64, crl.GaussianOptions(), seed=0), G.offsets(3, 1, 64)
    assert np.all(np.isfinite(p1)) and all(np.any(p1[off[i]:off[i + 1]] != p0[off[i]:off[i + 1]]) for i in range(12))
    with pytest.raises(ValueError, match="crl_ppo_diagnose is not built for Gaussian handles"):
        crl.train_external(_agent(crl, 64, 3, 1, 64), crl.LibraryEnv("pendulum", 64), diag_every=1)
    called = []                                                  # a host env (no on_device) still goes to train_host_gaussian
    monkeypatch.setattr(sys.modules[crl.Agent.__module__], "train_host_gaussian", lambda agent, e: called.append(e))
    crl.ppo_continuous(crl.PPOConfig(num_envs=16, num_steps=8, total_timesteps=16 * 8), env=HostEnv(), hidden=64)
    assert len(called) == 1 and isinstance(called[0], HostEnv)
