"""Device-resident external envs on the GPU (csrc/extenv.hip, include/cleanrl_hip.h "Device-resident external envs"): crl_rollout_act_device against the
CPU oracle and crl_policy_act, crl_ppo_diagnose on an external rollout, crl_rollout_record_device against a numpy restatement, crl_env_step_device against
crl_env_step, crl_ppo_update against the update half of crl_ppo_iterate, peer-stream ordering without host waits, and ppo(config, env=LibraryEnv(...)).

Bars. logprob / value: the project bar 1e-5 |x| + 1e-6 (tests/test_gpu_parity.py). Actions: equal to the oracle sampler's on the same Philox uniform
wherever the oracle's CDF-knot margin exceeds 1e-6; the exceptions may cover at most 1 % of a case's samples (the share is printed). Everything that is a
copy or integer bookkeeping is compared bit for bit.

Device buffers come from tests/hipmem.py (ctypes on libamdhip64); nothing here needs torch. Every GPU step runs under the `limit` watchdog."""
import json
import math

import numpy as np
import pytest

import hipmem
import oraclelib as O
from test_gpu_eval import limit
from test_gpu_parity import crl  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
SEED = 0x5EED
OFFSET = 1000
K = 4
RTOL, ATOL = 1e-5, 1e-6


def _ocfg(D, A, H, nt, k=K):
    return O.make_config(num_envs=nt, num_steps=k, obs_dim=D, n_act=A, hidden=H, env_kind=0 if (D, A) == (4, 2) else 1, stale_obs=0, seed=SEED)


def _params(crl, D, A, H, seed=3, head=100.0):   # noqa: F811
    """crl_make_actor_critic with the actor head scaled from gain 0.01 to gain 1 (as test_gpu_eval._params): logit gaps are O(1), near-ties rare"""
    p = crl._lib.make_actor_critic_host(D, A, H, seed)
    off = O.param_offsets(_ocfg(D, A, H, 8))
    p[off[4]:off[6]] *= np.float32(head)
    return p


def _agent(crl, D, A, H, nt, k=K, params=None, env_kind=None, nmb=1, **kw):   # noqa: F811
    F = crl._lib
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, num_minibatches=nmb, total_timesteps=nt * k * 10)
    return crl.Agent(cfg, params=params, obs_dim=D, n_act=A, hidden=H, env_kind=F.ENV_EXTERNAL if env_kind is None else env_kind,
                     **({"seed": SEED, "env_id_offset": OFFSET} | kw))


def _within_bar(got, want):
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    return np.abs(got - want) <= RTOL * np.abs(want) + ATOL


def _same_bits(a, b):
    """equal shape, dtype and bytes (NaN-safe; the arrays are column-major, which a uint8 view does not take)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes(order="A") == b.tobytes(order="A")


def _inputs(D, nt, k, seed):
    rng = np.random.default_rng(seed)
    obs = np.asfortranarray((rng.random((D, nt, k)) * 4 - 2).astype(np.float32))
    done = np.asfortranarray((rng.random((nt, k)) < 0.3).astype(np.uint8))
    return obs, done


BUFFER_FIELDS = ("F_OBS", "F_ACTION", "F_LOGPROB", "F_REWARD", "F_TERMINAL", "F_VALUE")
SENTINEL = {"F_OBS": -77.0, "F_ACTION": -7, "F_LOGPROB": -77.0, "F_REWARD": -77.0, "F_TERMINAL": 0xAB, "F_VALUE": -77.0}
GUARD = 16    # int32 words behind action_d


def _act_rollout(h, F, obs, done, nt, D, k=K, first_step=0):
    """k crl_rollout_act_device steps from uploaded inputs; returns the actions action_d received, (nt, k), and the guard words behind it"""
    actions = np.zeros((nt, k), np.int32, order="F")
    act_d = hipmem.Buf(4 * (nt + GUARD)).put(np.full(nt + GUARD, 0x5A5A5A5A, np.int32))
    for s in range(first_step, k):
        o_d, d_d = hipmem.upload(obs[:, :, s]), hipmem.upload(done[:, s])
        with limit(60):
            h.act_device(s, o_d, d_d, act_d)
            h.sync()
        got = act_d.get(np.int32)
        actions[:, s] = got[:nt]
        assert (got[nt:] == 0x5A5A5A5A).all(), f"step {s}: a guard word behind action_d was overwritten"
    return actions


# --------------------------------------------------------------------------------------------------------------- 1. act parity
ACT_CASES = [(4, 2, 64, 37, 0), (4, 2, 64, 37, 2), (4, 2, 64, 1, 0), (6, 3, 128, 70, 0), (8, 4, 256, 64, 0), (64, 16, 256, 33, 0), (3, 2, 64, 96, 0)]


@pytest.mark.parametrize("D,A,H,nt,iteration", ACT_CASES, ids=["fused-37", "fused-37-it2", "fused-1", "6-3-128-70", "8-4-256-64", "64-16-256-33", "3-2-64-96"])
def test_act_device_matches_oracle_and_policy_act(crl, D, A, H, nt, iteration):   # noqa: F811
    F = crl._lib
    params = _params(crl, D, A, H)
    ocfg = _ocfg(D, A, H, nt)
    agent = _agent(crl, D, A, H, nt, params=params)
    h = agent.handle
    obs, done = _inputs(D, nt, K, 100 * D + nt)
    if iteration:
        # the iteration counter moves by crl_ppo_update only: fill the buffer with a rollout (random rewards), update twice, put the parameters back
        with limit(120):
            _act_rollout(h, F, obs, done, nt, D)
            rng = np.random.default_rng(5)
            for s in range(K):
                h.record_device(s, hipmem.upload(rng.random(nt).astype(np.float32)), hipmem.upload(obs[:, :, s]), hipmem.upload(done[:, s]))
            for _ in range(iteration):
                h.update(want_stats=False)
            h.sync()
            agent.set_params(params)
        assert h.iteration == iteration
    for f in BUFFER_FIELDS:
        h.write(getattr(F, f), np.full(h._shape(getattr(F, f)), SENTINEL[f], F._FIELD_DTYPES[getattr(F, f)]))
    before = {f: h.read(getattr(F, f)) for f in BUFFER_FIELDS}
    actions = np.zeros((nt, K), np.int32, order="F")
    act_d = hipmem.Buf(4 * (nt + GUARD)).put(np.full(nt + GUARD, 0x5A5A5A5A, np.int32))
    for s in range(K):
        o_d, d_d = hipmem.upload(obs[:, :, s]), hipmem.upload(done[:, s])
        with limit(60):
            h.act_device(s, o_d, d_d, act_d)
            h.sync()
        got = act_d.get(np.int32)
        actions[:, s] = got[:nt]
        assert (got[nt:] == 0x5A5A5A5A).all(), f"step {s}: a guard word behind action_d was overwritten"
        now = {f: h.read(getattr(F, f)) for f in BUFFER_FIELDS}
        for f in BUFFER_FIELDS:                                   # nothing outside slot s changed
            other = [t for t in range(K) if t != s]
            assert np.array_equal(now[f][..., other], before[f][..., other]), f"step {s}: {f} changed outside its slot"
        assert np.array_equal(now["F_REWARD"], before["F_REWARD"]), "act_device does not write rewards"
        before = now
    buf = before
    assert np.array_equal(buf["F_OBS"].view(np.uint32), obs.view(np.uint32)), "CRL_F_OBS holds the observations passed in, bit for bit"
    assert np.array_equal(buf["F_TERMINAL"], done) and np.array_equal(buf["F_ACTION"], actions)
    assert ((actions >= 0) & (actions < A)).all()
    soft = 0
    for s in range(K):
        u = np.array([O.lib().orc_u53(SEED, OFFSET + e, iteration * K + s, 0) for e in range(nt)])
        x = np.asfortranarray(obs[:, :, s])
        a_o, lp_o, v_o, margin = O.get_action(ocfg, params, x, u)
        knot = margin <= 1e-6
        soft += int(knot.sum())
        assert np.array_equal(actions[~knot, s], a_o[~knot]), f"step {s}: action differs from the oracle sampler away from a CDF knot"
        same = actions[:, s] == a_o
        assert _within_bar(buf["F_LOGPROB"][same, s], lp_o[same]).all(), f"step {s}: logprob against the oracle"
        assert _within_bar(buf["F_VALUE"][:, s], v_o).all(), f"step {s}: value against the oracle"
        with limit(60):
            a_p, lp_p, v_p = h.policy_act(x, u)
        assert np.array_equal(actions[~knot, s], a_p[~knot]), f"step {s}: action differs from crl_policy_act away from a CDF knot"
        same = actions[:, s] == a_p
        assert _within_bar(buf["F_LOGPROB"][same, s], lp_p[same]).all() and _within_bar(buf["F_VALUE"][:, s], v_p).all(), f"step {s}: against crl_policy_act"
    share = soft / (nt * K)
    print(f"act parity {D}/{A}/{H} nt={nt}: {soft} of {nt * K} samples at a CDF knot ({share:.2%})")
    assert share <= 0.01
    agent.close()


def test_act_device_errors(crl):   # noqa: F811
    F = crl._lib
    import sys
    h = F.Handle(sys.modules[crl.Agent.__module__]._crl_config(crl.PPOConfig(num_envs=32, num_steps=K, num_minibatches=1), env_kind=F.ENV_EXTERNAL), 0)
    b = hipmem.Buf(4 * 32 * 4)
    with pytest.raises(F.CrlError, match="parameters not set"):
        h.act_device(0, b, b, b)
    h.init_params(0)
    for step in (-1, K):
        with pytest.raises(F.CrlError, match="step out of range"):
            h.act_device(step, b, b, b)
        with pytest.raises(F.CrlError, match="step out of range"):
            h.record_device(step, b, b, b)
    assert h.stream != 0
    h.close()


# --------------------------------------------------------------------------------------------------------------- 2. diagnose agrees
@pytest.mark.parametrize("D,A,H,nt", [(4, 2, 64, 37), (8, 4, 256, 64), (64, 16, 256, 33)], ids=["fused-37", "8-4-256-64", "64-16-256-33"])
def test_diagnose_agrees_with_an_external_rollout(crl, D, A, H, nt):   # noqa: F811
    """The values are compared bit for bit as well: crl_ppo_diagnose and crl_rollout_act_device run the critic through the same forward block
    (csrc/fwd_rs_x3.hpp) on the same observations and parameters, so a difference means the two kernels no longer share it. 64 / 16 / 256 streams W1 from the
    parameters instead of LDS. The logprobs keep their bar: the two kernels write the log-softmax differently."""
    F = crl._lib
    agent = _agent(crl, D, A, H, nt, params=_params(crl, D, A, H))
    h = agent.handle
    obs, done = _inputs(D, nt, K, 7)
    rng = np.random.default_rng(8)
    with limit(120):
        _act_rollout(h, F, obs, done, nt, D)
        for s in range(K):
            h.record_device(s, hipmem.upload(rng.random(nt).astype(np.float32)), hipmem.upload(obs[:, :, s]), hipmem.upload(done[:, s]))
        h.compute_gae()
        d = h.diagnose(per_sample=True)
    lp, v = h.read(F.F_LOGPROB), h.read(F.F_VALUE)
    assert _within_bar(d["new_logprob"], lp).all() and _within_bar(d["new_value"], v).all()
    assert np.array_equal(d["new_value"].view(np.uint32), v.view(np.uint32)), "new_value and CRL_F_VALUE differ in bits"
    assert d["clipfrac"] == 0.0
    # |logratio| of a sample is at most the logprob bar r = 1e-5 max|logprob| + 1e-6; kl_b = (e^x - 1) - x = x^2 / 2 + O(x^3) <= x^2 for |x| <= 1, so the mean
    # over the samples, approx_kl, is below r^2
    r = RTOL * float(np.abs(lp).max()) + ATOL
    assert abs(d["approx_kl"]) < r * r, (d["approx_kl"], r * r)
    agent.close()


# --------------------------------------------------------------------------------------------------------------- 3. record
@pytest.mark.parametrize("ring_cap", [4096, 5], ids=["ring-all", "ring-small"])
def test_record_device_bookkeeping(crl, ring_cap):   # noqa: F811
    """Device order of the statistics: lanes of a wave by butterfly, waves by atomic arrival — not (step, env). The Float64 sums of Float32 returns are
    exact for these magnitudes (checked below against math.fsum), so every order gives the bits of the (step, env) restatement."""
    F = crl._lib
    D, A, H, nt, k = 6, 3, 128, 70, 16
    agent = _agent(crl, D, A, H, nt, k=k, params=_params(crl, D, A, H))
    h = agent.handle
    h.episode_ring_enable(ring_cap)
    rng = np.random.default_rng(11)
    reward = np.asfortranarray((rng.random((nt, k)) * 3 - 1).astype(np.float32))          # signed, sums not exactly representable
    nobs = np.asfortranarray(rng.standard_normal((D, nt, k)).astype(np.float32))
    ndone = np.asfortranarray((rng.random((nt, k)) < 0.3).astype(np.uint8))
    ndone[:, 0] = 0; ndone[3, :] = 0                                                      # known boundaries: nobody ends at step 0, env 3 never ends
    zero_obs, zero_done, act_d = hipmem.Buf(4 * D * nt).put(np.zeros(D * nt, np.float32)), hipmem.Buf(nt).put(np.zeros(nt, np.uint8)), hipmem.Buf(4 * nt)
    with limit(120):
        h.act_device(0, zero_obs, zero_done, act_d)                                       # step 0 of a rollout clears the statistics and the ring
        for s in range(k):
            h.record_device(s, hipmem.upload(reward[:, s]), hipmem.upload(nobs[:, :, s]), hipmem.upload(ndone[:, s]))
        h.sync()
        st = h.episode_stats()
        recs, total = h.episode_records()
    assert np.array_equal(h.read(F.F_REWARD).view(np.uint32), reward.view(np.uint32))
    assert np.array_equal(h.read(F.F_CUR_OBS).view(np.uint32), nobs[:, :, k - 1].view(np.uint32)) and np.array_equal(h.read(F.F_NEXT_DONE), ndone[:, k - 1])
    ep_ret = np.zeros(nt, np.float32); ep_len = np.zeros(nt, np.int32)
    want, rsum, lsum = [], 0.0, 0.0
    for s in range(k):
        ep_ret = ep_ret + reward[:, s]; ep_len += 1                                        # Float32 running sum in step order
        for e in np.flatnonzero(ndone[:, s]):
            want.append((s, OFFSET + int(e), float(ep_ret[e]), int(ep_len[e])))
            rsum += float(ep_ret[e]); lsum += float(ep_len[e])                             # Float64, (step, env) order
            ep_ret[e] = 0; ep_len[e] = 0
    assert len(want) > ring_cap or ring_cap == 4096
    assert rsum == math.fsum(w[2] for w in want), "the restatement's sum is exact, hence order-free"
    assert st["episodes"] == len(want) and st["length_sum"] == lsum and st["return_sum"] == rsum
    assert st["return_max"] == max(w[2] for w in want)
    assert total == len(want)
    if ring_cap >= len(want):
        assert recs == sorted(want)
    else:
        assert len(recs) == ring_cap and len(set(recs)) == ring_cap and set(recs) <= set(want)
    agent.close()


# --------------------------------------------------------------------------------------------------------------- 4. env_step_device
@pytest.mark.parametrize("name,kind,D,A", [("cartpole", 0, 4, 2), ("mountaincar", 3, 2, 3), ("acrobot", 4, 6, 3)])
def test_env_step_device_equals_env_step(crl, name, kind, D, A):   # noqa: F811
    F = crl._lib
    nt, steps = 37, 8
    a1 = _agent(crl, D, A, 64, nt, env_kind=kind); a2 = _agent(crl, D, A, 64, nt, env_kind=kind, params=a1.get_params())
    h1, h2 = a1.handle, a2.handle
    rng = np.random.default_rng(4)
    obs_d, rew_d, done_d = hipmem.Buf(4 * D * nt), hipmem.Buf(4 * nt), hipmem.Buf(nt)
    with limit(120):
        h1.env_reset(); h2.env_reset()
        for g in range(steps):
            act = rng.integers(0, A, nt).astype(np.int32)
            o1, r1, d1 = h1.env_step(act, gstep=g)
            h2.env_step_device(hipmem.upload(act), g, obs_d, rew_d, done_d)
            h2.sync()
            o2, r2, d2 = obs_d.get(np.float32, (D, nt)), rew_d.get(np.float32), done_d.get(np.uint8)
            assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)) and np.array_equal(r1.view(np.uint32), r2.view(np.uint32)) and np.array_equal(d1, d2), g
        for f in (F.F_ENV_STATE, F.F_ENV_T, F.F_CUR_OBS, F.F_NEXT_DONE):
            assert _same_bits(h1.read(f), h2.read(f)), f
        bad = np.zeros(nt, np.int32); bad[5] = A
        h2.env_step_device(hipmem.upload(bad), steps, None, rew_d, done_d)                 # enqueues; nothing is read back here
        with pytest.raises(F.CrlError, match="crl_env_step_device: an action was outside"):
            h2.sync()
        h2.sync()                                                                          # reported once
    a1.close(); a2.close()


# --------------------------------------------------------------------------------------------------------------- 5. update = the update half of iterate
COPIED = ("F_OBS", "F_ACTION", "F_LOGPROB", "F_REWARD", "F_TERMINAL", "F_VALUE", "F_ADVANTAGE", "F_RETURN", "F_CUR_OBS", "F_NEXT_DONE")
COMPARED = ("F_PARAMS", "F_ADAM_M", "F_ADAM_V", "F_BETAP", "F_PERM", "F_ADVANTAGE", "F_RETURN")
UPDATE_CASES = [(0, 4, 2, 64, 64, 32, {"gemm": 2}), (0, 4, 2, 64, 64, 32, {"gemm": 1}), (4, 6, 3, 128, 64, 32, {}), (1, 8, 4, 256, 64, 8, {})]


@pytest.mark.parametrize("kind,D,A,H,nt,k,opts", UPDATE_CASES, ids=["cartpole-x2", "cartpole-x3", "acrobot-128", "synthetic-256"])
def test_update_equals_the_update_half_of_iterate(crl, kind, D, A, H, nt, k, opts):   # noqa: F811
    F = crl._lib
    params = crl._lib.make_actor_critic_host(D, A, H, 1)
    a = _agent(crl, D, A, H, nt, k=k, nmb=4, params=params, env_kind=kind, env_id_offset=0, options=opts | {"gae_fuse": 0})
    b = _agent(crl, D, A, H, nt, k=k, nmb=4, params=params, env_kind=F.ENV_EXTERNAL, env_id_offset=0, options=opts)
    ha, hb = a.handle, b.handle
    for it in range(2):                                                                    # the second pass: anneal_lr and the epoch keys have moved
        with limit(120):
            sa = ha.iterate(1)
            for f in COPIED:
                hb.write(getattr(F, f), ha.read(getattr(F, f)))
            sb = hb.update()
        assert ha.iteration == hb.iteration == it + 1
        for f in COMPARED:
            x, y = ha.read(getattr(F, f)), hb.read(getattr(F, f))
            assert _same_bits(x, y), f"iteration {it}: {f} differs"
        assert len(sa) == len(sb) == 16
        for x, y in zip(sa, sb):
            assert all(np.float64(x[key]).tobytes() == np.float64(y[key]).tobytes() for key in x), (it, x, y)
    a.close(); b.close()


# --------------------------------------------------------------------------------------------------------------- 6. streams
def _stream_run(crl, synced, counter):   # noqa: F811
    F = crl._lib
    nt, k = 64, 32
    env = crl.LibraryEnv("cartpole", nt, seed=SEED)
    agent = _agent(crl, 4, 2, 64, nt, k=k, params=_params(crl, 4, 2, 64), env_id_offset=0)
    h = agent.handle
    assert env.stream and h.stream and env.stream != h.stream
    act_d = hipmem.Buf(4 * nt)
    obs, done = env.reset()
    h.sync(); env.handle.sync()
    counter[0] = 0
    for s in range(k):
        h.act_device(s, obs, done, act_d, peer_stream=env.stream)
        if synced:
            h.sync(); env.handle.sync()
        reward, obs, done = env.step(act_d)
        if synced:
            h.sync(); env.handle.sync()
        h.record_device(s, reward, obs, done, peer_stream=env.stream)
        if synced:
            h.sync(); env.handle.sync()
    calls = counter[0]
    h.sync(); env.handle.sync()
    out = {f: h.read(getattr(F, f)) for f in BUFFER_FIELDS + ("F_CUR_OBS", "F_NEXT_DONE")}
    out["stats"] = h.episode_stats()
    agent.close(); env.close()
    return out, calls


def test_peer_streams_order_the_loop_without_host_waits(crl, monkeypatch):   # noqa: F811
    counter = [0]
    real = crl._lib.Handle.sync

    def counting(self):
        counter[0] += 1
        return real(self)
    monkeypatch.setattr(crl._lib.Handle, "sync", counting)
    with limit(120):
        free, calls = _stream_run(crl, False, counter)
        assert calls == 0, "act_device / env_step_device / record_device wrappers do not synchronise"
        ref, calls = _stream_run(crl, True, counter)
        assert calls == 32 * 6
    for f in ref:
        if f == "stats":
            assert free[f] == ref[f]
        else:
            assert _same_bits(free[f], ref[f]), f
    assert ref["stats"]["episodes"] > 0


# --------------------------------------------------------------------------------------------------------------- 7. end to end
def episode_return_curve(crl, tmp, external, seed, nt=256, k=128, updates=40):   # noqa: F811
    """mean episode return per update of ppo(config, env=...) — the "Episode Statistics" aggregates of its JSON-lines log"""
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * updates)
    name = f"extenv-{'ext' if external else 'lib'}-{seed}"
    env = crl.LibraryEnv("cartpole", nt, seed=seed) if external else "cartpole"
    try:
        crl.ppo(cfg, env=env, seed=seed, init_seed=seed, episode_records=0, run_name=name, logger_kw=dict(to_tensorboard=False, to_json=True, log_dir=str(tmp)))
    finally:
        if external:
            env.close()
    recs = [json.loads(line) for line in open(f"{tmp}/{name}.json")]
    return [r["episode_return"] for r in recs if r["msg"] == "Episode Statistics"]


def test_external_cartpole_trains_like_the_builtin_env(crl, tmp_path):   # noqa: F811
    """ppo(config, env=LibraryEnv("cartpole", 256)) against ppo(config, env="cartpole"): two samples of one training distribution (the act kernel's bf16x3
    forward and the on-device rollout's fp16x2 forward pick different actions at CDF knots, so trajectories diverge). Mean episode return over the last
    five updates, averaged over three seeds: external >= 0.8 x built-in, and external >= 3 x its own first update. The 0.8 is the issue's guess at the
    seed-to-seed spread; scripts/extenv_train.py writes the six curves and the measured built-in spread to profiles/extenv_train.json."""
    last, first = {True: [], False: []}, []
    for seed in (1, 2, 3):
        for external in (True, False):
            with limit(300):
                c = episode_return_curve(crl, tmp_path, external, seed)
            assert len(c) >= 30
            last[external].append(float(np.mean(c[-5:])))
            if external:
                first.append(c[0])
    ext, lib = float(np.mean(last[True])), float(np.mean(last[False]))
    print(f"last-five mean return: external {last[True]} -> {ext:.1f}, built-in {last[False]} -> {lib:.1f}; external first update {first}")
    assert ext >= 0.8 * lib
    assert ext >= 3 * float(np.mean(first))
