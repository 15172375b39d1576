"""crl_dqn_evaluate (csrc/dqn.hip, dqn_eval_kernel; its episode loop is dqn_eval_episodes of csrc/dqn_loops.hpp) against its definition in include/cleanrl_hip.h: the device's trace is replayed through the
oracle's CartPole and every output is held bit for bit — actions against the argmax of h.q_values, sums against the replay, q0 against h.q_values,
the report against the formulas on the returned arrays (tests/value_eval_gpu.py). The Q-net has no transcendental in it and h.q_values is the
oracle's dqn_forward bit for bit, so the reference's own rollout (tests/value_eval_ref.py) must give the identical trace too."""
import json
import os

import numpy as np
import pytest

import oraclelib as O
import value_eval_gpu as G
import value_eval_ref as V

pytestmark = pytest.mark.gpu
ENVS_PER_BLOCK = 4      # dqn_eval_kernel's DQN_EVAL_WAVES: n = 5 below is "envs per block + 1"; 67 and 257 leave the last block partial
K = V.DQN


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _same_as_the_reference_rollout(out, params, n, E, seed, max_steps, gamma):
    ref = V.evaluate(K, params, n, E, seed, max_steps, gamma)
    assert np.array_equal(ref["trace_action"], out["trace_action"]) and np.array_equal(ref["v0"], out["q0"])
    assert all(np.array_equal(ref[k], out[k]) for k in G.ARRAYS)
    return ref


# ---------------------------------------------------------------------------------------------------- 1. trajectory, 2. unequal lengths
@pytest.mark.parametrize("max_steps,n,E", [(1, 1, 1), (5, ENVS_PER_BLOCK + 1, 3), (5, 67, 2), (5, 257, 3), (200, 3, 2)])
def test_trajectory_follows_the_definition(crl, max_steps, n, E):
    assert G.envs_per_block(crl, K) == ENVS_PER_BLOCK and 67 % ENVS_PER_BLOCK and 257 % ENVS_PER_BLOCK and 3 <= ENVS_PER_BLOCK
    params, seed, gamma = V.dqn_perturbed(2), 0xE7A1 + n, 0.97
    h = G.handle(crl, K, params, max_steps=max_steps, gamma=gamma)
    out, rp, _ = G.check_against_the_definition(crl, h, K, params, n, E, seed, max_steps, gamma)
    _same_as_the_reference_rollout(out, params, n, E, seed, max_steps, gamma)
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
@pytest.mark.parametrize("net,max_steps,ending", [(V.dqn_balancer, 60, "limit"), (V.dqn_constant, 200, "angle")])
def test_both_endings(crl, net, max_steps, ending):
    params, n, E, seed, gamma = net(), 6, 2, 3, 0.99
    h = G.handle(crl, K, params, max_steps=max_steps, gamma=gamma)
    out, rp, _ = G.check_against_the_definition(crl, h, K, params, n, E, seed, max_steps, gamma)
    _same_as_the_reference_rollout(out, params, n, E, seed, max_steps, gamma)
    if ending == "limit":
        assert (out["lengths"] == max_steps + 1).all() and (out["returns"] == max_steps).all() and (out["trace_action"] >= 0).all()
    else:
        assert (out["lengths"] < 20).all() and (out["trace_action"][out["trace_action"] >= 0] == 1).all()
        assert (out["q0"] == 1.0).all() and (out["trace_action"] == -1).sum() == out["trace_action"].size - out["lengths"].sum()
    h.close()


# ---------------------------------------------------------------------------------------------------- 5. read-only
def test_evaluation_reads_and_never_writes(crl):
    """tests/test_gpu_dqn.py's small-ring run (150 slots, an update every 3 steps, a target copy every 9), in chunks, with an evaluation before every
    chunk: parameters, target, status and every record stay those of the oracle run that never evaluated."""
    kw = dict(batch_size=32, min_buff_size=40, train_freq=3, target_net_freq=9, buffer_size=150, epsilon_duration=300.0)
    T, params = 1500, O.dqn_params(1)
    agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=T, lr=1e-3, log_frequencey=30, **kw), params=params, seed=21)
    st = O.DQNState(O.dqn_config(total_timesteps=T, lr=1e-3, seed=21, log_frequency=30, **kw), params)
    h, total, evals = agent.handle, 0, []
    for chunk in (1, 7, 200, 5, 1000, 100_000):
        before = (h.read_params(), h.status())
        evals.append(h.evaluate(ENVS_PER_BLOCK + 1, 2, 77, trace_steps=9))
        assert G.same(h.evaluate(ENVS_PER_BLOCK + 1, 2, 77, trace_steps=9), evals[-1], K, with_trace=True)
        after = (h.read_params(), h.status())
        assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0]))
        assert all(np.array_equal(before[1][k], after[1][k]) for k in before[1])
        tg, eps_g, ls_g = h.run(chunk)
        to, eps_o, ls_o = st.run(chunk)
        total += tg
        assert tg == to and eps_g == eps_o and ls_g == ls_o
        sg, so = h.status(), st.env()
        assert sg["global_step"] == so["global_step"] == total and sg["rb_size"] == so["rb_size"]
        assert sg["n_updates"] == so["n_updates"] and sg["last_loss"] == so["last_loss"] and np.array_equal(sg["state"], so["state"])
        (qg, tg_), (qo, to_) = h.read_params(), st.params()
        assert np.array_equal(qg, qo) and np.array_equal(tg_, to_)
    assert total == T and h.status()["n_updates"] > 100
    assert not np.array_equal(evals[0]["q0"], evals[-1]["q0"]), "the evaluated parameters are the current ones"
    q, t = h.read_params()
    assert not np.array_equal(q, t)                                  # the evaluation reads q_net, not the target
    twin = G.handle(crl, K, q, max_steps=200, gamma=0.99)
    assert G.same(twin.evaluate(ENVS_PER_BLOCK + 1, 2, 77), h.evaluate(ENVS_PER_BLOCK + 1, 2, 77), K)
    agent.close(); st.close(); twin.close()


# ---------------------------------------------------------------------------------------------------- 6. errors
def test_errors_name_the_field(crl):
    L = crl._lib
    h = G.handle(crl, K, V.dqn_constant(), max_steps=200)
    for args, field in (((0, 1), "num_envs"), ((65537, 1), "num_envs"), ((-1, 1), "num_envs"), ((1, 0), "episodes_per_env"), ((1, 1025), "episodes_per_env"),
                        ((65536, 17), r"num_envs \* episodes_per_env"), ((1, 1, 0, 202), "trace_steps"), ((2, 2, 0, 403), "trace_steps"),
                        ((65536, 2, 0, 257), r"trace_steps \* num_envs")):
        with pytest.raises(crl.CrlError, match="crl_dqn_evaluate: " + field):
            h.evaluate(*args)
    rep = L.CrlValueEvalReport(); buf = np.zeros(8, np.int32)
    ptr = buf.ctypes.data_as(L.C.POINTER(L.C.c_int32))
    for cfg, report, trace, msg in ((None, rep, None, "null cfg or report"), (L.CrlEvalConfig(2, 1, 0, 0, 1), None, None, "null cfg or report"),
                                    (L.CrlEvalConfig(2, 1, 2, 0, 1), rep, None, "mode must be"),
                                    (L.CrlEvalConfig(2, 1, -1, 0, 1), rep, None, "mode must be"),
                                    (L.CrlEvalConfig(2, 1, L.EVAL_SAMPLE, 0, 1), rep, None, "DQN has no sampling policy"),
                                    (L.CrlEvalConfig(2, 1, 0, -1, 1), rep, None, "trace_steps"),
                                    (L.CrlEvalConfig(2, 1, 0, 3, 1), rep, None, "trace_action must be given exactly when trace_steps > 0"),
                                    (L.CrlEvalConfig(2, 1, 0, 0, 1), rep, ptr, "trace_action must be given exactly when trace_steps > 0")):
        rc, err = G.raw_evaluate(crl, h, K, cfg, report, trace=trace)
        assert rc != 0 and "crl_dqn_evaluate: " in err and msg in err, (msg, err)
    assert h.evaluate(2, 1, 1, trace_steps=201)["trace_action"].shape == (201, 2)        # the largest trace of one episode is accepted
    fresh = G.handle(crl, K, None)
    with pytest.raises(crl.CrlError, match="crl_dqn_evaluate: parameters not set"):
        fresh.evaluate(2)
    # the Python-side validation raises before the library is touched: this agent has no handle to touch
    agent = object.__new__(crl.DQNAgent); agent.handle = None; agent.crl_cfg = h.cfg; agent.config = crl.DQNConfig()
    for kw, field in ((dict(num_envs=0), "num_envs"), (dict(num_envs=2.0), "num_envs"), (dict(episodes_per_env=1025), "episodes_per_env"),
                      (dict(num_envs=65536, episodes_per_env=17), "num_envs \\* episodes_per_env"), (dict(seed=-1), "seed"),
                      (dict(trace_steps=202), "trace_steps"), (dict(num_envs=65536, episodes_per_env=2, trace_steps=257), "trace_steps \\* num_envs")):
        with pytest.raises(ValueError, match="dqn_evaluate: " + field):
            crl.dqn_evaluate(agent, **kw)
    with pytest.raises(TypeError, match="DQNAgent"):
        crl.dqn_evaluate(h)
    with pytest.raises(ValueError, match="dqn: eval_every"):
        crl.dqn(crl.DQNConfig(), eval_every=-1)
    with pytest.raises(ValueError, match="dqn: num_envs"):
        crl.dqn(crl.DQNConfig(), eval_every=10, eval_envs=0)
    h.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------- 7. entry points
def _records(path):
    return [json.loads(l) for l in open(path)]


def _strip(recs):
    """the records without what the wall clock writes into them"""
    drop = {"steps_per_sec", "time", "asctime", "created", "timestamp"}
    return [{k: v for k, v in r.items() if k not in drop} for r in recs]


def test_dqn_logs_evaluation_statistics_and_trains_the_same(crl, tmp_path):
    def run(name, **kw):
        cfg = crl.DQNConfig(run_name=name, total_timesteps=1500, log_frequencey=100)
        agent = crl.dqn(cfg, seed=9, chunk=700, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(tmp_path), **kw)
        params, st = agent.handle.read_params(), agent.handle.status()
        ev = crl.dqn_evaluate(agent, num_envs=3, episodes_per_env=2)
        agent.close()
        return _records(os.path.join(tmp_path, f"dqn|{name}.json")), params, st, ev
    plain, p0, s0, _ = run("plain")
    evald, p1, s1, ev = run("evald", eval_every=500, eval_envs=8)
    assert all(r["msg"] != "Evaluation Statistics" for r in plain)
    evs = [(i, r) for i, r in enumerate(evald) if r["msg"] == "Evaluation Statistics"]
    assert [r["global_step"] for _, r in evs] == [500, 1000, 1500]
    assert all(set(r) >= {"eval_return_mean", "eval_return_std", "eval_q_bias", "global_step"} for _, r in evs)
    for i, r in evs:                                               # the record follows the records of its step
        assert all(q.get("global_step", 0) <= r["global_step"] for q in evald[:i] if "global_step" in q)
    assert _strip([r for r in evald if r["msg"] != "Evaluation Statistics"]) == _strip(plain) and len(plain) > 20
    assert all(np.array_equal(a, b) for a, b in zip(p0, p1)) and s0["global_step"] == s1["global_step"] == 1500
    assert all(np.array_equal(s0[k], s1[k]) for k in s0)
    assert evs[0][1]["eval_return_mean"] != evs[-1][1]["eval_return_mean"] or evs[0][1]["eval_q_bias"] != evs[-1][1]["eval_q_bias"]
    assert ev["report"]["episodes"] == 6 and ev["returns"].shape == ev["lengths"].shape == ev["q0"].shape == (2, 3)
    assert set(ev["report"]) >= {"q0_mean", "q_bias_mean", "length_mean"} and "v0_mean" not in ev["report"]
