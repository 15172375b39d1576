"""What tests/test_gpu_dqn_eval.py and tests/test_gpu_a2c_eval.py share: handles, and the check of one crl_*_evaluate call against its definition
in include/cleanrl_hip.h. The definition is stated in public calls — the action of a step is the argmax (or the sampled index) of what
crl_dqn_q_values / crl_a2c_forward return for the step's observation, v0 what they return on the first —, and the CartPole and the sums have no
transcendental in them, so the device's trace is replayed through the oracle's CartPole (tests/value_eval_ref.py) and everything is held bit for bit."""
import numpy as np

import value_eval_ref as V

ARRAYS = ("returns", "lengths", "disc_returns")


def v0_name(kind):
    return "q0" if kind == V.DQN else "v0"


def handle(crl, kind, params=None, max_steps=200, gamma=0.99, **kw):
    """a low-level handle with `params` written (None: a fresh handle, parameters never set)"""
    L = crl._lib
    if kind == V.DQN:
        d = dict(log_frequency=1000, total_timesteps=10_000, buffer_size=1000, min_buff_size=200, lr=1e-4, train_freq=10, target_net_freq=100,
                 batch_size=120, epsilon_start=1.0, epsilon_end=0.05, epsilon_duration=10_000.0, seed=0x5EED)
        d.update(kw)
        h = L.DQNHandle(L.CrlDQNConfig(d["log_frequency"], d["total_timesteps"], d["buffer_size"], d["min_buff_size"], d["lr"], d["train_freq"],
                                       d["target_net_freq"], d["batch_size"], gamma, d["epsilon_start"], d["epsilon_end"], d["epsilon_duration"],
                                       max_steps, 0, d["seed"]), 0)
    else:
        d = dict(lr=1e-4, total_timesteps=10_000, min_replay_size=max(512, max_steps + 1), seed=0x5EED)
        d.update(kw)
        h = L.A2CHandle(L.CrlA2CConfig(d["lr"], d["total_timesteps"], d["min_replay_size"], max_steps, gamma, d["seed"]), 0)
    if params is not None:
        h.write_params(params)
    return h


def envs_per_block(crl, kind):
    return crl._lib.dqn_eval_envs_per_block() if kind == V.DQN else crl._lib.a2c_eval_envs_per_block()


def evaluate(h, kind, n, E, seed, mode=V.GREEDY, trace_steps=0):
    return h.evaluate(n, E, seed, trace_steps) if kind == V.DQN else h.evaluate(n, E, mode, seed, trace_steps)


def raw_evaluate(crl, h, kind, cfg, report, arrays=(None, None, None, None), trace=None):
    """the C call itself → (return code, last error)"""
    L = crl._lib
    lib = L.load()
    fn = lib.crl_dqn_evaluate if kind == V.DQN else lib.crl_a2c_evaluate
    rc = fn(h._h, cfg, report, *arrays, trace)
    return rc, lib.crl_last_error().decode()


def same(a, b, kind, with_trace=False):
    keys = ARRAYS + (v0_name(kind),) + (("trace_action",) if with_trace else ())
    return a["report"] == b["report"] and all(np.array_equal(a[k], b[k]) for k in keys)


def forward_bar(h, params, obs):
    """A2C's public forward against the oracle's: tests/test_gpu_a2c.py's bar for Float64 quantities, 1e-9 relative (tanh_fast has an exp in it)."""
    z_ref = np.stack([V.a2c_forward(params, 0, np.ascontiguousarray(o)) for o in obs], 1)      # (2, steps)
    v_ref = np.array([V.a2c_forward(params, 1, np.ascontiguousarray(o))[0] for o in obs])
    for got, ref in ((h.forward(0, obs.T), z_ref), (h.forward(1, obs.T), v_ref)):
        assert got.shape == ref.shape and (np.abs(got - ref) <= 1e-9 * np.maximum(1.0, np.abs(ref))).all()


def check_against_the_definition(crl, h, kind, params, n, E, seed, max_steps, gamma, mode=V.GREEDY):
    """Runs the evaluation with a full trace and holds every output to the header's definition. → (device result, the replay, left-out decisions)"""
    rows, name = E * (max_steps + 1), v0_name(kind)
    out = evaluate(h, kind, n, E, seed, mode, trace_steps=rows)
    trace = out["trace_action"]
    assert trace.shape == (rows, n) and trace.dtype == np.int32 and out["lengths"].dtype == np.int32
    assert all(out[k].shape == (E, n) for k in ARRAYS + (name,))
    rp = V.evaluate(kind, params, n, E, seed, max_steps, gamma, mode, actions=trace)    # the device's actions through the oracle's CartPole; it
    used = trace >= 0                                                                   # also asserts 0/1 inside the quota and −1 after it
    assert used.sum() == out["lengths"].sum() and np.array_equal(used.sum(0), out["lengths"].sum(0))
    obs = rp["obs"][used]                                                               # (steps, 4), row-major over (row, env)
    left_out = 0
    if kind == V.DQN:
        q = h.q_values(obs.T)
        assert np.array_equal(trace[used], (q[1] > q[0]).astype(np.int32)), "every action is the argmax of crl_dqn_q_values, bit for bit"
        assert np.array_equal(q, np.stack([V.q_values(params, np.ascontiguousarray(o)) for o in obs], 1)), "crl_dqn_q_values is the oracle's dqn_forward"
    elif mode == V.GREEDY:
        z = h.forward(0, obs.T)
        assert np.array_equal(trace[used], (z[1] > z[0]).astype(np.int32)), "every action is the argmax of crl_a2c_forward(0), bit for bit"
        forward_bar(h, params, obs)
    else:
        p0, draws = rp["p0"][used], rp["draws"][used]
        keep = np.abs(p0 - draws) > 1e-12                                               # the device's exp and libm's can differ in the last bit
        left_out = int((~keep).sum())
        assert left_out * 10_000 <= keep.size, "at most 1 decision in 10,000 may be left out"
        assert np.array_equal(trace[used][keep], (p0 <= draws).astype(np.int32)[keep]), "action = p0 <= draw, the draw from Philox stream 0x21"
    for k in ARRAYS:
        assert np.array_equal(out[k], rp[k]), k
    assert np.array_equal(out["returns"], out["lengths"] - 1.0)
    e_idx = np.tile(np.arange(n), E)
    obs0 = rp["obs"][rp["first"].reshape(-1), e_idx]                                     # (E·n, 4) in array order
    if kind == V.DQN:
        a0 = trace[rp["first"].reshape(-1), e_idx]
        assert np.array_equal(out[name].reshape(-1), h.q_values(obs0.T)[a0, np.arange(E * n)]), "q0 is crl_dqn_q_values(obs0)[a0], bit for bit"
        assert np.array_equal(out[name], rp["v0"])
    else:
        assert np.array_equal(out[name].reshape(-1), h.forward(1, obs0.T)), "v0 is crl_a2c_forward(1, obs0), bit for bit"
        assert (np.abs(out[name] - rp["v0"]) <= 1e-9 * np.maximum(1.0, np.abs(rp["v0"]))).all()
    want = V.report(out["returns"], out["lengths"], out["disc_returns"], out[name], prefix=name[0])
    assert out["report"] == want and want["episodes"] == n * E and want["env_steps"] == out["lengths"].sum()
    return out, rp, left_out


def check_without_trace_and_with_null_arrays(crl, h, kind, out, n, E, seed, mode=V.GREEDY):
    again = evaluate(h, kind, n, E, seed, mode)
    assert "trace_action" not in again and same(again, out, kind)
    L = crl._lib
    cfg = L.CrlEvalConfig(n, E, mode, 0, seed); rep = L.CrlValueEvalReport()
    rc, err = raw_evaluate(crl, h, kind, cfg, rep)
    assert rc == 0, err
    assert list(rep.as_dict().values()) == list(out["report"].values())


def check_envs_do_not_disturb_each_other(crl, h, kind, out, n, E, seed):
    """each env's results are those of an n = 1 call whose episodes start from the same reset draws: env e's episode j resets at gstep j·n + e, which
    is episode j·n + e of a single env"""
    name = v0_name(kind)
    solo = evaluate(h, kind, 1, (E - 1) * n + n, seed)
    for e in range(n):
        for j in range(E):
            for k in ARRAYS + (name,):
                assert solo[k][j * n + e, 0] == out[k][j, e], (k, j, e)
