"""crl_a2c_evaluate and crl_a2c_forward (csrc/a2c.hip, a2c_eval_kernel / a2c_forward_kernel) against their definition in include/cleanrl_hip.h: the
device's trace is replayed through the oracle's CartPole and every output is held bit for bit — actions against the argmax of h.forward(0, obs),
sums against the replay, v0 against h.forward(1, obs0), the report against the formulas on the returned arrays (tests/value_eval_gpu.py).
tanh_fast has an exp in it, so h.forward is held to the oracle's a2c_forward at tests/test_gpu_a2c.py's bar for Float64 quantities (1e-9 relative),
not bit for bit; the hand-made nets of tests/value_eval_ref.py stay on tanh_fast's polynomial branch, and there the reference's own rollout must
give the identical outputs. Sampled actions are held to p0 <= draw with the reference's p0 and the Philox restatement's draw."""
import json
import os

import numpy as np
import pytest

import oraclelib as O
import value_eval_gpu as G
import value_eval_ref as V

pytestmark = pytest.mark.gpu
ENVS_PER_BLOCK = 4      # a2c_eval_kernel's A2C_EVAL_WAVES: n = 5 below is "envs per block + 1"; 67 and 257 leave the last block partial
K = V.A2C


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


# ---------------------------------------------------------------------------------------------------- the public forward
def test_forward_matches_oracle(crl):
    rng = np.random.default_rng(0)
    params = V.a2c_perturbed(4)
    h = G.handle(crl, K, params)
    obs = rng.standard_normal((33, 4))
    G.forward_bar(h, params, obs)
    z, v = h.forward(0, obs.T), h.forward(1, obs.T)
    assert z.shape == (2, 33) and v.shape == (33,)
    assert np.array_equal(h.forward(0, obs[7]), z[:, 7:8]) and np.array_equal(h.forward(1, obs[7]), v[7:8]), "one observation, the same bits"
    assert h.forward(0, np.zeros((4, 0))).shape == (2, 0)
    # on tanh_fast's polynomial branch there is no exp: bit for bit
    p = V.a2c_balancer()
    hb = G.handle(crl, K, p)
    small = 0.05 * rng.standard_normal((17, 4))
    assert np.array_equal(hb.forward(0, small.T), np.stack([V.a2c_forward(p, 0, np.ascontiguousarray(o)) for o in small], 1))
    assert np.array_equal(hb.forward(1, small.T), np.array([V.a2c_forward(p, 1, np.ascontiguousarray(o))[0] for o in small]))
    h.close(); hb.close()


# ---------------------------------------------------------------------------------------------------- 1. trajectory, 2. unequal lengths
@pytest.mark.parametrize("max_steps,n,E", [(1, 1, 1), (5, ENVS_PER_BLOCK + 1, 3), (5, 67, 2), (5, 257, 3), (200, 3, 2)])
def test_trajectory_follows_the_definition(crl, max_steps, n, E):
    assert G.envs_per_block(crl, K) == ENVS_PER_BLOCK and 67 % ENVS_PER_BLOCK and 257 % ENVS_PER_BLOCK and 3 <= ENVS_PER_BLOCK
    params, seed, gamma = V.a2c_perturbed(4), 0xE7A1 + n, 0.97
    h = G.handle(crl, K, params, max_steps=max_steps, gamma=gamma)
    out, rp, _ = G.check_against_the_definition(crl, h, K, params, n, E, seed, max_steps, gamma)
    assert len({tuple(o) for o in rp["obs"][rp["first"].reshape(-1), np.tile(np.arange(n), E)]}) == n * E, "every episode starts somewhere else"
    G.check_without_trace_and_with_null_arrays(crl, h, K, out, n, E, seed)
    if max_steps == 200:
        # unequal episode lengths inside one block: a wave that leaves early must not disturb its neighbours
        assert n <= ENVS_PER_BLOCK and len(set(out["lengths"].sum(0))) >= 2 and any(len(set(row)) >= 2 for row in out["lengths"])
        assert (out["lengths"] < 201).all(), "this net drops the pole long before the step limit"
        G.check_envs_do_not_disturb_each_other(crl, h, K, out, n, E, seed)
    else:
        assert (out["lengths"] == max_steps + 1).all(), "no CartPole falls within 6 steps of its reset"
    h.close()


# ---------------------------------------------------------------------------------------------------- 3. both endings
@pytest.mark.parametrize("net,max_steps,ending", [(V.a2c_balancer, 60, "limit"), (V.a2c_constant, 200, "angle")])
def test_both_endings(crl, net, max_steps, ending):
    params, n, E, seed, gamma = net(), 6, 2, 3, 0.99
    h = G.handle(crl, K, params, max_steps=max_steps, gamma=gamma)
    out, rp, _ = G.check_against_the_definition(crl, h, K, params, n, E, seed, max_steps, gamma)
    ref = V.evaluate(K, params, n, E, seed, max_steps, gamma)         # no exp on these nets: the reference's own rollout, bit for bit
    assert np.array_equal(ref["trace_action"], out["trace_action"]) and np.array_equal(ref["v0"], out["v0"])
    assert all(np.array_equal(ref[k], out[k]) for k in G.ARRAYS)
    if ending == "limit":
        assert (out["lengths"] == max_steps + 1).all() and (out["returns"] == max_steps).all() and (out["trace_action"] >= 0).all()
    else:
        assert (out["lengths"] < 20).all() and (out["trace_action"][out["trace_action"] >= 0] == 1).all()
        assert (out["trace_action"] == -1).sum() == out["trace_action"].size - out["lengths"].sum()
    assert (out["v0"] != 0.5).all() and np.abs(out["v0"] - 0.5).max() < 0.02
    h.close()


# ---------------------------------------------------------------------------------------------------- 4. sample mode
def test_sample_mode(crl):
    """seeds and case of tests/test_value_eval_cpu.py::test_sample_seeds_leave_no_decision_out: the reference alone leaves no decision out"""
    params, c = V.a2c_perturbed(4), V.SAMPLE_CASE
    h = G.handle(crl, K, params, max_steps=c["max_steps"], gamma=c["gamma"])
    outs = []
    for seed in V.SAMPLE_SEEDS:
        out, rp, left_out = G.check_against_the_definition(crl, h, K, params, c["n"], c["E"], seed, c["max_steps"], c["gamma"], mode=V.SAMPLE)
        assert left_out == 0, "the reference leaves none out for these seeds, and the device's p0 is within 1e-12 of it"
        ref = V.evaluate(K, params, c["n"], c["E"], seed, c["max_steps"], c["gamma"], mode=V.SAMPLE)
        assert np.array_equal(ref["trace_action"], out["trace_action"])
        G.check_without_trace_and_with_null_arrays(crl, h, K, out, c["n"], c["E"], seed, mode=V.SAMPLE)
        outs.append(out)
    assert not np.array_equal(outs[0]["trace_action"], outs[1]["trace_action"]), "two seeds, two traces"
    rows = c["E"] * (c["max_steps"] + 1)
    again = h.evaluate(c["n"], c["E"], V.SAMPLE, V.SAMPLE_SEEDS[0], rows)
    assert G.same(again, outs[0], K, with_trace=True), "the same seed, the same trace"
    greedy = h.evaluate(c["n"], c["E"], V.GREEDY, V.SAMPLE_SEEDS[0], rows)
    assert not np.array_equal(greedy["trace_action"], outs[0]["trace_action"])
    # a larger draw of decisions under the 1-in-10,000 cap
    big, _, left_out = G.check_against_the_definition(crl, h, K, params, 64, 2, 0xB16, c["max_steps"], c["gamma"], mode=V.SAMPLE)
    assert big["lengths"].sum() > 1000 and left_out * 10_000 <= big["lengths"].sum()
    h.close()


# ---------------------------------------------------------------------------------------------------- 5. read-only
def _state(h):
    return h.read_params(), h.env(), h.buffer()


def _same_state(a, b):
    (pa, (sa, ga, na), ba), (pb, (sb, gb, nb), bb) = a, b
    return np.array_equal(pa, pb) and np.array_equal(sa, sb) and (ga, na) == (gb, nb) and all(np.array_equal(x, y) for x, y in zip(ba, bb))


def test_evaluation_reads_and_never_writes(crl):
    """tests/test_gpu_a2c.py's training run across three updates with an evaluation before every call: against the oracle at that file's bars, and
    bit for bit against a second device handle that never evaluates."""
    params = O.orthogonal_params(O.make_config(), 5)
    cfg = crl.A2CConfig(total_timesteps=6000, lr=1e-3)
    agent, twin = crl.A2CAgent(cfg, params=params, seed=3), crl.A2CAgent(cfg, params=params, seed=3)
    st = O.A2CState(O.a2c_config(total_timesteps=6000, lr=1e-3, seed=3), params)
    h, n_updates, evals = agent.handle, 0, []
    while n_updates < 3:
        before = _state(h)
        mode = V.SAMPLE if n_updates % 2 else V.GREEDY
        evals.append(h.evaluate(ENVS_PER_BLOCK + 1, 2, mode, 77, 9))
        assert G.same(h.evaluate(ENVS_PER_BLOCK + 1, 2, mode, 77, 9), evals[-1], K, with_trace=True)
        assert _same_state(before, _state(h))
        budget = 300 if n_updates == 0 else 1 << 40                  # a call that stops mid-episode, too
        tg, ts_g, eps_g = h.run_until_update(budget)
        tt, ts_t, eps_t = twin.handle.run_until_update(budget)
        to, ts_o, eps_o = st.run_until_update(budget)
        assert (tg, ts_g, eps_g) == (tt, ts_t, eps_t) and _same_state(_state(h), _state(twin.handle)), "bit for bit the handle that never evaluated"
        assert tg == to and eps_g == eps_o and ts_g["trained"] == ts_o["trained"] and ts_g["n"] == ts_o["n"]
        if ts_g["trained"]:
            n_updates += 1
            for k in ("actor_loss", "critic_loss"):
                assert abs(ts_g[k] - ts_o[k]) <= 1e-9 * max(1.0, abs(ts_o[k])), (k, ts_g[k], ts_o[k])
            assert np.max(np.abs(h.read_params() - st.get_params())) < 1e-6
    assert not np.array_equal(evals[0]["v0"], h.evaluate(ENVS_PER_BLOCK + 1, 2, V.GREEDY, 77)["v0"]), "the evaluated parameters are the current ones"
    agent.close(); twin.close(); st.close()


# ---------------------------------------------------------------------------------------------------- 6. errors
def test_errors_name_the_field(crl):
    L = crl._lib
    h = G.handle(crl, K, V.a2c_constant(), max_steps=200)
    for args, field in (((0, 1), "num_envs"), ((65537, 1), "num_envs"), ((-1, 1), "num_envs"), ((1, 0), "episodes_per_env"), ((1, 1025), "episodes_per_env"),
                        ((65536, 17), r"num_envs \* episodes_per_env"), ((1, 1, 2), "mode must be"), ((1, 1, -1), "mode must be"),
                        ((1, 1, 0, 0, 202), "trace_steps"), ((2, 2, 1, 0, 403), "trace_steps"), ((65536, 2, 0, 0, 257), r"trace_steps \* num_envs")):
        with pytest.raises(crl.CrlError, match="crl_a2c_evaluate: " + field):
            h.evaluate(*args)
    rep = L.CrlValueEvalReport(); buf = np.zeros(8, np.int32)
    ptr = buf.ctypes.data_as(L.C.POINTER(L.C.c_int32))
    for cfg, report, trace, msg in ((None, rep, None, "null cfg or report"), (L.CrlEvalConfig(2, 1, 0, 0, 1), None, None, "null cfg or report"),
                                    (L.CrlEvalConfig(2, 1, 1, -1, 1), rep, None, "trace_steps"),
                                    (L.CrlEvalConfig(2, 1, 0, 3, 1), rep, None, "trace_action must be given exactly when trace_steps > 0"),
                                    (L.CrlEvalConfig(2, 1, 1, 0, 1), rep, ptr, "trace_action must be given exactly when trace_steps > 0")):
        rc, err = G.raw_evaluate(crl, h, K, cfg, report, trace=trace)
        assert rc != 0 and "crl_a2c_evaluate: " in err and msg in err, (msg, err)
    assert h.evaluate(2, 1, V.SAMPLE, 1, 201)["trace_action"].shape == (201, 2)          # the largest trace of one episode is accepted
    fresh = G.handle(crl, K, None)
    with pytest.raises(crl.CrlError, match="crl_a2c_evaluate: parameters not set"):
        fresh.evaluate(2)
    with pytest.raises(crl.CrlError, match="crl_a2c_forward: parameters not set"):
        fresh.forward(0, np.zeros((4, 1)))
    # crl_a2c_forward
    lib = L.load()
    dp = L.C.POINTER(L.C.c_double)
    x = np.zeros(4); o = np.zeros(2)
    with pytest.raises(crl.CrlError, match="crl_a2c_forward: net must be 0"):
        h.forward(2, x)
    for args, msg in (((-1, x.ctypes.data_as(dp), 1, o.ctypes.data_as(dp)), "net must be 0"), ((0, x.ctypes.data_as(dp), -1, o.ctypes.data_as(dp)), "n must be >= 0"),
                      ((0, None, 1, o.ctypes.data_as(dp)), "null obs or out"), ((1, x.ctypes.data_as(dp), 1, None), "null obs or out")):
        assert lib.crl_a2c_forward(h._h, *args) != 0
        assert "crl_a2c_forward: " + msg in lib.crl_last_error().decode(), msg
    assert lib.crl_a2c_forward(h._h, 0, None, 0, None) == 0                              # nothing to do is no error
    # the Python-side validation raises before the library is touched: this agent has no handle to touch
    agent = object.__new__(crl.A2CAgent); agent.handle = None; agent.crl_cfg = h.cfg; agent.config = crl.A2CConfig()
    for kw, field in ((dict(num_envs=0), "num_envs"), (dict(num_envs=2.0), "num_envs"), (dict(episodes_per_env=1025), "episodes_per_env"),
                      (dict(num_envs=65536, episodes_per_env=17), "num_envs \\* episodes_per_env"), (dict(seed=-1), "seed"), (dict(greedy=1), "greedy"),
                      (dict(trace_steps=202), "trace_steps"), (dict(num_envs=65536, episodes_per_env=2, trace_steps=257), "trace_steps \\* num_envs")):
        with pytest.raises(ValueError, match="a2c_evaluate: " + field):
            crl.a2c_evaluate(agent, **kw)
    with pytest.raises(TypeError, match="A2CAgent"):
        crl.a2c_evaluate(h)
    with pytest.raises(ValueError, match="a2c: eval_every"):
        crl.a2c(crl.A2CConfig(), eval_every=-1)
    with pytest.raises(ValueError, match="a2c: num_envs"):
        crl.a2c(crl.A2CConfig(), eval_every=10, eval_envs=0)
    h.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------- 7. entry points
def _records(path):
    return [json.loads(l) for l in open(path)]


def _strip(recs):
    """the records without what the wall clock writes into them"""
    drop = {"steps_per_sec", "time", "asctime", "created", "timestamp"}
    return [{k: v for k, v in r.items() if k not in drop} for r in recs]


def test_a2c_logs_evaluation_statistics_and_trains_the_same(crl, tmp_path):
    def run(name, **kw):
        cfg = crl.A2CConfig(run_name=name, total_timesteps=1500, lr=1e-3)
        agent = crl.a2c(cfg, seed=9, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(tmp_path), **kw)
        params, env = agent.handle.read_params(), agent.handle.env()
        ev = {g: crl.a2c_evaluate(agent, num_envs=3, episodes_per_env=2, greedy=g) for g in (True, False)}
        agent.close()
        return _records(os.path.join(tmp_path, f"a2c|{name}.json")), params, env, ev
    plain, p0, e0, _ = run("plain")
    evald, p1, e1, ev = run("evald", eval_every=500, eval_envs=8)
    assert all(r["msg"] != "Evaluation Statistics" for r in plain)
    evs = [(i, r) for i, r in enumerate(evald) if r["msg"] == "Evaluation Statistics"]
    assert [r["global_step"] for _, r in evs] == [500, 1000, 1500]
    assert all(set(r) >= {"eval_return_mean", "eval_return_std", "eval_v_bias", "global_step"} for _, r in evs)
    for i, r in evs:                                               # the record follows the records of its step
        assert all(q.get("global_step", 0) <= r["global_step"] for q in evald[:i] if "global_step" in q)
    assert _strip([r for r in evald if r["msg"] != "Evaluation Statistics"]) == _strip(plain) and len(plain) > 20
    assert any(r["msg"] == "Training Statistics" for r in plain), "the run crossed an update"
    assert np.array_equal(p0, p1) and np.array_equal(e0[0], e1[0]) and e0[1:] == e1[1:] and e0[1] == 1500
    assert evs[0][1]["eval_v_bias"] != evs[-1][1]["eval_v_bias"], "the evaluated parameters are the current ones"
    assert ev[True]["report"]["episodes"] == 6 and ev[True]["returns"].shape == ev[True]["lengths"].shape == ev[True]["v0"].shape == (2, 3)
    assert set(ev[True]["report"]) >= {"v0_mean", "v_bias_mean", "length_mean"}
    assert np.array_equal(ev[True]["v0"], ev[False]["v0"]) and not np.array_equal(ev[True]["lengths"], ev[False]["lengths"])
