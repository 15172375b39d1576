"""crl_ddpg_evaluate (csrc/ddpg.hip, ddpg_eval_kernel) against its definition in include/cleanrl_hip.h. The definition is stated in public calls —
the action of a step is what crl_ddpg_actor returns for the step's observation, q0 what crl_ddpg_q_values returns —, and the Pendulum and the sums
have no transcendental in them, so the device's trace is replayed through the numpy Pendulum of tests/ddpg_ref.py and everything is held bit for
bit: actions against h.actor, returns and discounted returns against the replay, q0 against h.q_values, the report against the formulas on the
returned arrays. Against the numpy forwards (whose exp differs from the device's in the last bit) the bar is ddpg_ref's own 1e-10."""
import json
import os

import numpy as np
import pytest

import ddpg_eval_ref as V
import ddpg_ref as R

pytestmark = pytest.mark.gpu
ENVS_PER_BLOCK = 4      # ddpg_eval_kernel's EVAL_WAVES: (5, 5, 3) below is "envs per block + 1", 67 and 257 leave the last block partial


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _handle(crl, external=False, params_seed=3, **kw):
    d = dict(total_timesteps=300, buffer_size=1000, min_buff_size=10, batch_size=7, warmup_steps=5, log_frequency=1, lr=1e-3, tau=0.005, gamma=0.99,
             exploration_noise=0.1, max_steps=200, noise_in_update=1, seed=0x5EED)
    d.update(kw)
    L = crl._lib
    c = L.CrlDDPGConfig(d["total_timesteps"], d["buffer_size"], d["min_buff_size"], d["batch_size"], d["warmup_steps"], d["log_frequency"], d["lr"],
                        d["tau"], d["gamma"], d["exploration_noise"], 3, 1, L.DDPG_ENV_EXTERNAL if external else L.DDPG_ENV_PENDULUM, d["max_steps"],
                        -2.0, 2.0, d["noise_in_update"], 0, d["seed"])
    h = L.DDPGHandle(c, 0)
    if params_seed is not None:
        h.write_params(*_params(crl, params_seed))
    return h


def _params(crl, seed):
    """perturbed glorot parameters (non-zero biases), as tests/test_gpu_ddpg.py"""
    rng = np.random.default_rng(seed)
    a, c = crl.make_ddpg_nn(3, 1, seed=seed)
    return (a + (0.05 * rng.standard_normal(a.size)).astype(np.float32), c + (0.05 * rng.standard_normal(c.size)).astype(np.float32))


def _check_against_the_definition(h, actor, critic, n, E, seed, max_steps, gamma):
    """Runs the evaluation with a full trace and holds every output to the header's definition. → (device result, the replay)"""
    rows = E * max_steps
    out = h.evaluate(n, E, seed, trace_steps=rows)
    trace = out["trace_action"]
    assert trace.shape == (rows, n) and out["returns"].shape == out["disc_returns"].shape == out["q0"].shape == (E, n)
    rp = V.evaluate(actor, critic, n, E, seed, max_steps, gamma, actions=trace)       # the device's actions through the reference's Pendulum
    obs = rp["obs"].reshape(rows * n, 3).T                                             # column row·n + e
    assert np.array_equal(trace.reshape(-1), h.actor(obs)[0]), "every action is crl_ddpg_actor of the replayed observation, bit for bit"
    assert np.abs(trace.reshape(-1) - R.actor_mean(actor, 3, 1, obs)[0]).max() <= 1e-10
    assert np.array_equal(out["returns"], rp["returns"]) and np.array_equal(out["disc_returns"], rp["disc_returns"])
    first = np.array([j * max_steps for j in range(E)])
    obs0 = rp["obs"][first].reshape(E * n, 3).T; a0 = trace[first].reshape(1, E * n)
    assert np.array_equal(out["q0"].reshape(-1), h.q_values(obs0, a0)), "q0 is crl_ddpg_q_values of (obs0, a0), bit for bit"
    assert np.abs(out["q0"] - rp["q0"]).max() <= 1e-10 * np.abs(rp["q0"]).max()
    want = V.report(out["returns"], out["disc_returns"], out["q0"], max_steps)
    assert out["report"] == want and out["report"]["episodes"] == n * E and out["report"]["env_steps"] == n * E * max_steps
    return out, rp


# ---------------------------------------------------------------------------------------------------- 1. trajectory
@pytest.mark.parametrize("max_steps,n,E", [(1, 1, 1), (5, 5, 3), (5, 67, 2), (5, 257, 3), (200, 3, 2)])
def test_trajectory_follows_the_definition(crl, max_steps, n, E):
    assert ENVS_PER_BLOCK + 1 == 5 and 67 % ENVS_PER_BLOCK and 257 % ENVS_PER_BLOCK
    actor, critic = _params(crl, 3)
    h = _handle(crl, max_steps=max_steps, gamma=0.97)
    out, rp = _check_against_the_definition(h, actor, critic, n, E, 0xE7A1 + n, max_steps, 0.97)
    assert len(np.unique(rp["theta"][0])) == n, "every env starts somewhere else"
    if max_steps > 1:
        assert (np.abs(out["disc_returns"]) < np.abs(out["returns"])).all()
    else:
        assert np.array_equal(out["disc_returns"], out["returns"])
    # without the trace, and with NULL arrays, the same numbers
    again = h.evaluate(n, E, 0xE7A1 + n)
    assert "trace_action" not in again and again["report"] == out["report"] and all(np.array_equal(again[k], out[k]) for k in ("returns", "disc_returns", "q0"))
    L = crl._lib
    cfg = L.CrlDDPGEvalConfig(n, E, 0, 0, 0xE7A1 + n); rep = L.CrlDDPGEvalReport()
    L.check(L.load().crl_ddpg_evaluate(h._h, cfg, rep, None, None, None, None))
    assert rep.as_dict() == out["report"]
    h.close()


# ---------------------------------------------------------------------------------------------------- 2. saturation, wrap, clamp
def test_saturated_actions_wrap_and_clamp(crl):
    """The case tests/test_ddpg_eval_cpu.py pins by the reference alone, through the same assertions on the device."""
    actor = V.hard_actor()
    critic = _params(crl, 5)[1]
    c = V.HARD
    h = _handle(crl, params_seed=None, max_steps=c["max_steps"], gamma=c["gamma"])
    h.write_params(actor, critic)
    out, rp = _check_against_the_definition(h, actor, critic, c["n"], c["E"], c["seed"], c["max_steps"], c["gamma"])
    assert set(np.unique(out["trace_action"])) == {-2.0, 2.0}
    assert rp["wrapped"] >= 1 and rp["clamped"] >= 1 and np.abs(rp["theta_dot"]).max() == 8.0
    ref = V.evaluate(actor, None, **c)                                                 # the reference's own rollout takes the same actions
    assert np.array_equal(ref["trace_action"], out["trace_action"]) and np.array_equal(ref["returns"], out["returns"])
    h.close()


# ---------------------------------------------------------------------------------------------------- 3. read-only
def _snapshot(h):
    return h.read_params(), h.status(), h.buffer()


def _same(a, b):
    (pa, sa, ba), (pb, sb, bb) = a, b
    return all(np.array_equal(x, y) for x, y in zip(pa, pb)) and sa == sb and all(np.array_equal(ba[k], bb[k]) for k in ba)


def test_evaluation_reads_and_never_writes(crl):
    kw = dict(total_timesteps=420, warmup_steps=100, min_buff_size=150, batch_size=16, seed=5, params_seed=6)
    h, twin = _handle(crl, **kw), _handle(crl, **kw)
    recs, twin_recs = [h.run(230)], [twin.run(230)]
    st = h.status()
    assert st["global_step"] == 230 and st["n_updates"] == 80 and st["env_t"] == 30, "mid-training: updates running, an episode open"
    before = _snapshot(h)
    e1 = h.evaluate(37, 2, 99, trace_steps=11)
    e2 = h.evaluate(37, 2, 99, trace_steps=11)
    assert e1["report"] == e2["report"] and all(np.array_equal(e1[k], e2[k]) for k in ("returns", "disc_returns", "q0", "trace_action"))
    assert _same(before, _snapshot(h))
    assert np.array_equal(e1["trace_action"][0], h.actor(np.stack([R.pendulum_obs(*R.pendulum_reset(99, e, V.S_EVAL)) for e in range(37)], 1))[0])
    recs.append(h.run(1000)); twin_recs.append(twin.run(1000))
    assert recs == twin_recs and h.status()["global_step"] == 420 and len(recs[1][2]) == 190 and len(recs[0][1]) + len(recs[1][1]) == 2
    assert _same(_snapshot(h), _snapshot(twin)), "training goes on as if the evaluation had not happened"
    h.close(); twin.close()


# ---------------------------------------------------------------------------------------------------- 4. parameters and seed
def test_it_follows_the_parameters_and_the_seed(crl):
    a = _handle(crl, total_timesteps=200, warmup_steps=20, min_buff_size=30, batch_size=8, max_steps=40, params_seed=2)
    a.run(120)                                                     # the actor has moved away from its target and from its initial values
    actor, critic, actor_t, _ = a.read_params()
    assert not np.array_equal(actor, actor_t)
    b = _handle(crl, params_seed=None, max_steps=40)
    b.write_params(actor, critic)
    ea, eb = a.evaluate(9, 2, 1234), b.evaluate(9, 2, 1234)
    assert ea["report"] == eb["report"] and all(np.array_equal(ea[k], eb[k]) for k in ("returns", "disc_returns", "q0"))
    other = a.evaluate(9, 2, 1235)
    assert not np.array_equal(other["returns"], ea["returns"]) and (other["returns"] != ea["returns"]).all()
    assert (ea["returns"][0] != ea["returns"][1]).all(), "episodes 0 and 1 of one env start somewhere else"
    c = _handle(crl, params_seed=7, max_steps=40)                  # other parameters, same seed: other actions
    assert not np.array_equal(c.evaluate(9, 2, 1234)["returns"], ea["returns"])
    a.close(); b.close(); c.close()


# ---------------------------------------------------------------------------------------------------- 5. errors
def test_errors_name_the_field(crl):
    L = crl._lib
    h = _handle(crl, max_steps=200)
    for args, field in (((0, 1), "num_envs"), ((65537, 1), "num_envs"), ((-1, 1), "num_envs"), ((1, 0), "episodes_per_env"), ((1, 1025), "episodes_per_env"),
                        ((65536, 17), r"num_envs \* episodes_per_env"), ((1, 1, 0, 201), "trace_steps"), ((2, 2, 0, 401), "trace_steps"),
                        ((65536, 2, 0, 257), r"trace_steps \* num_envs")):
        with pytest.raises(crl.CrlError, match="crl_ddpg_evaluate: " + field):
            h.evaluate(*args)
    lib = L.load()
    rep = L.CrlDDPGEvalReport(); buf = np.zeros(8)
    ptr = buf.ctypes.data_as(L.C.POINTER(L.C.c_double))
    for cfg, report, trace, msg in ((None, rep, None, "null cfg or report"), (L.CrlDDPGEvalConfig(2, 1, 0, 0, 1), None, None, "null cfg or report"),
                                    (L.CrlDDPGEvalConfig(2, 1, -1, 0, 1), rep, None, "trace_steps"),
                                    (L.CrlDDPGEvalConfig(2, 1, 3, 0, 1), rep, None, "trace_action must be given exactly when trace_steps > 0"),
                                    (L.CrlDDPGEvalConfig(2, 1, 0, 0, 1), rep, ptr, "trace_action must be given exactly when trace_steps > 0")):
        assert lib.crl_ddpg_evaluate(h._h, cfg, report, None, None, None, trace) != 0
        assert msg in lib.crl_last_error().decode(), msg
    assert h.evaluate(2, 1, 1, trace_steps=200)["trace_action"].shape == (200, 2)      # the largest trace of one episode is accepted
    fresh = _handle(crl, params_seed=None)
    with pytest.raises(crl.CrlError, match="crl_ddpg_evaluate: parameters not set"):
        fresh.evaluate(2)
    ext = _handle(crl, external=True)
    with pytest.raises(crl.CrlError, match="crl_ddpg_evaluate.*crl_ddpg_actor"):
        ext.evaluate(2)
    agent = object.__new__(crl.DDPGAgent); agent.handle = ext; agent.crl_cfg = ext.cfg; agent.config = crl.DDPGConfig()
    with pytest.raises(crl.CrlError, match="crl_ddpg_actor"):                          # env=None on an external handle: the library's message
        crl.ddpg_evaluate(agent, num_envs=2)
    h.close(); fresh.close(); ext.close()


# ---------------------------------------------------------------------------------------------------- 6. entry points
def _records(path):
    return [json.loads(l) for l in open(path)]


def _strip(recs):
    """the records without what the wall clock writes into them"""
    drop = {"steps_per_sec", "time", "asctime", "created", "timestamp"}
    return [{k: v for k, v in r.items() if k not in drop} for r in recs]


def test_ddpg_logs_evaluation_statistics_and_trains_the_same(crl, tmp_path):
    def run(name, **kw):
        cfg = crl.DDPGConfig(run_name=name, total_timesteps=450, warmup_steps=120, min_buff_size=100, batch_size=16, log_frequencey=50)
        agent = crl.ddpg(cfg, "pendulum", seed=9, chunk=170, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(tmp_path), **kw)
        params = agent.handle.read_params(); st = agent.handle.status()
        ev = crl.ddpg_evaluate(agent, num_envs=3, episodes_per_env=1)
        agent.close()
        return _records(os.path.join(tmp_path, f"ddpg|{name}.json")), params, st, ev
    plain, p0, s0, _ = run("plain")
    evald, p1, s1, ev = run("evald", eval_every=100, eval_envs=3, eval_episodes=1)
    assert all(r["msg"] != "Evaluation Statistics" for r in plain)
    evs = [(i, r) for i, r in enumerate(evald) if r["msg"] == "Evaluation Statistics"]
    assert [r["global_step"] for _, r in evs] == [100, 200, 300, 400]
    assert all(set(r) >= {"eval_return_mean", "eval_return_std", "eval_q_bias", "global_step"} for _, r in evs)
    for i, r in evs:                                               # the record follows the records of its step
        assert all(q.get("global_step", 0) <= r["global_step"] for q in evald[:i] if "global_step" in q)
    assert _strip([r for r in evald if r["msg"] != "Evaluation Statistics"]) == _strip(plain) and len(plain) > 6
    assert all(np.array_equal(a, b) for a, b in zip(p0, p1)) and s0 == s1 and s0["global_step"] == 450
    assert evs[0][1]["eval_return_mean"] != evs[-1][1]["eval_return_mean"], "the evaluated parameters are the current ones"
    assert ev["report"]["episodes"] == 3 and ev["returns"].shape == (1, 3)


def test_host_env_routes(crl, tmp_path):
    cfg = crl.DDPGConfig(run_name="host", total_timesteps=260, warmup_steps=60, min_buff_size=50, batch_size=8, log_frequencey=50)
    eval_env = R.Pendulum(seed=77, max_steps=25)
    agent = crl.ddpg(cfg, R.Pendulum(seed=3, max_steps=40), seed=9, eval_every=100, eval_episodes=2, eval_env=eval_env,
                     to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(tmp_path))
    recs = _records(os.path.join(tmp_path, "ddpg|host.json"))
    assert [r["global_step"] for r in recs if r["msg"] == "Evaluation Statistics"] == [100, 200] and eval_env.n_resets == 4
    assert agent.handle.status()["global_step"] == 260
    # ddpg_evaluate(agent, env=...) is a loop over h.actor and h.q_values on that env
    h = agent.handle
    got = crl.ddpg_evaluate(agent, episodes_per_env=2, env=R.Pendulum(seed=5, max_steps=25))
    env = R.Pendulum(seed=5, max_steps=25)
    ret, disc_ret, q0 = np.zeros((2, 1)), np.zeros((2, 1)), np.zeros((2, 1))
    for j in range(2):
        obs, disc, term, t = env.reset(), np.float64(1.0), False, 0
        while not term:
            a = h.actor(obs)[:, 0]
            if t == 0:
                q0[j, 0] = h.q_values(obs, a)[0]
            r, obs, term = env.step(a)
            ret[j, 0] = ret[j, 0] + r; disc_ret[j, 0] = disc_ret[j, 0] + disc * np.float64(r); disc = disc * np.float64(cfg.gamma); t += 1
        assert t == 25
    assert np.array_equal(got["returns"], ret) and np.array_equal(got["disc_returns"], disc_ret) and np.array_equal(got["q0"], q0)
    want = V.report(ret, disc_ret, q0, 25)
    assert got["report"] == want and want["env_steps"] == 50 and "trace_action" not in got
    agent.close()
