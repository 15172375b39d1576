"""tests/value_eval_ref.py — the Float64 restatement of crl_dqn_evaluate / crl_a2c_evaluate that the GPU tests compare against — pinned by itself,
without a GPU: the reset draws, both endings of an episode, the sums in closed form, the report formulas, the trace's −1 tail, and the seeds for
which the sampled policy has no decision within the GPU test's tolerance."""
import os
import re

import numpy as np
import pytest

import value_eval_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from value_eval_ref import SAMPLE_CASE, SAMPLE_SEEDS


def test_reset_draws_are_small_and_distinct():
    n, E, seed = 7, 3, 0x51
    s = np.stack([V.reset(seed, j * n + e) for j in range(E) for e in range(n)])
    assert s.shape == (21, 4) and (s >= -0.05).all() and (s < 0.05).all()
    assert len({tuple(r) for r in s}) == 21 and len(np.unique(s)) == 84, "every (e, j) starts somewhere else, in every component"
    assert not np.array_equal(V.reset(seed + 1, 0), V.reset(seed, 0))
    out = V.evaluate(V.DQN, V.dqn_constant(), n, E, seed, 5, 0.9)
    assert np.array_equal(out["obs"][out["first"][1, 2], 2], V.reset(seed, 1 * n + 2)), "episode j of env e resets at gstep j·n + e"


@pytest.mark.parametrize("kind,net", [(V.DQN, V.dqn_constant), (V.A2C, V.a2c_constant)])
def test_constant_action_ends_every_episode_by_angle(kind, net):
    out = V.evaluate(kind, net(), 6, 2, 3, 200, 0.99)
    assert (out["lengths"] < 20).all() and (out["lengths"] > 3).all() and len(np.unique(out["lengths"])) > 1
    assert np.array_equal(out["returns"], out["lengths"] - 1.0), "the terminating step earns 0"
    used = out["trace_action"][out["trace_action"] >= 0]
    assert (used == 1).all() and used.size == out["lengths"].sum()
    last = out["first"] + out["lengths"] - 1                     # the observation the last action answered: one step before the fall
    for j in range(2):
        for e in range(6):
            s = out["obs"][last[j, e], e].copy()
            t, done = V.step(s, 0, 1, 200)
            assert done and abs(s[2]) > 12 * 2 * np.pi / 360 and abs(s[0]) < 2.4, "ended by the pole's angle"


@pytest.mark.parametrize("kind,net", [(V.DQN, V.dqn_balancer), (V.A2C, V.a2c_balancer)])
@pytest.mark.parametrize("max_steps", [1, 5])
def test_balancer_runs_into_the_step_limit(kind, net, max_steps):
    gamma = 0.9
    out = V.evaluate(kind, net(), 4, 2, 9, max_steps, gamma)
    assert (out["lengths"] == max_steps + 1).all() and (out["returns"] == max_steps).all()
    assert (out["trace_action"] >= 0).all(), "a full quota leaves no -1 in the trace"
    # all rewards but the last are 1: disc_return = 1 + γ + … + γ^(max_steps − 1), summed the way the definition sums it
    want, disc = np.float64(0.0), np.float64(1.0)
    for _ in range(max_steps):
        want = want + disc * np.float64(1.0); disc = disc * np.float64(gamma)
    assert (out["disc_returns"] == want).all() and abs(want - (1 - gamma ** max_steps) / (1 - gamma)) <= 4 * np.finfo(np.float64).eps * want


@pytest.mark.parametrize("max_steps", [200, 500])
def test_balancer_holds_for_whole_default_episodes(max_steps):
    out = V.evaluate(V.DQN, V.dqn_balancer(), 3, 1, 5, max_steps, 0.99)
    assert (out["lengths"] == max_steps + 1).all()
    assert np.abs(out["obs"] @ np.array(V.BALANCE)).max() < 1.0, "c/16 stays on tanh_fast's polynomial branch (|x| < 0.13)"
    a = V.evaluate(V.A2C, V.a2c_balancer(), 3, 1, 5, max_steps, 0.99)
    assert np.array_equal(a["trace_action"], out["trace_action"]), "both hand-made nets state the same rule"
    assert np.allclose(a["v0"], 0.5 + a["obs"][0, :, 2] / 4, atol=1e-4) and (a["v0"] != 0.5).all()


def test_dqn_v0_is_the_q_value_of_the_action_taken():
    p = V.dqn_balancer()
    out = V.evaluate(V.DQN, p, 5, 1, 2, 5, 0.99)
    for e in range(5):
        q = V.q_values(p, out["obs"][0, e])
        assert out["v0"][0, e] == q.max() == q[out["trace_action"][0, e]] and q.min() == 0.0


def test_report_formulas():
    ret = np.array([[1.0, 4.0], [2.0, 9.0]]); ln = np.array([[2, 5], [3, 10]], np.int32)
    disc = np.array([[0.5, 3.0], [1.5, 6.0]]); v0 = np.array([[1.0, 2.0], [3.0, 4.0]])
    rep = V.report(ret, ln, disc, v0)
    assert rep == dict(episodes=4, env_steps=20, return_mean=4.0, return_std=float(np.sqrt((9 + 0 + 4 + 25) / 4)), return_min=1.0, return_max=9.0,
                       length_mean=5.0, disc_return_mean=2.75, v0_mean=2.5, v_bias_mean=(0.5 - 1.0 + 1.5 - 2.0) / 4)
    q = V.report(ret, ln, disc, v0, prefix="q")
    assert q["q0_mean"] == rep["v0_mean"] and q["q_bias_mean"] == rep["v_bias_mean"] and "v0_mean" not in q


def test_trace_carries_minus_one_after_the_quota():
    out = V.evaluate(V.DQN, V.dqn_constant(), 3, 2, 3, 200, 0.99)
    tr, total = out["trace_action"], out["lengths"].sum(0)
    assert tr.shape == (2 * 201, 3)
    for e in range(3):
        assert (tr[:total[e], e] == 1).all() and (tr[total[e]:, e] == -1).all()
        assert out["first"][1, e] == out["lengths"][0, e], "rows count the env's steps across its episodes"
    again = V.evaluate(V.DQN, V.dqn_constant(), 3, 2, 3, 200, 0.99, actions=tr)               # replaying its own trace changes nothing
    assert all(np.array_equal(again[k], out[k]) for k in ("returns", "lengths", "disc_returns", "v0", "trace_action"))
    bad = tr.copy(); bad[total[1], 1] = 0
    with pytest.raises(AssertionError, match="after its quota"):
        V.evaluate(V.DQN, V.dqn_constant(), 3, 2, 3, 200, 0.99, actions=bad)


def test_sample_seeds_leave_no_decision_out():
    """The GPU test may leave out sampled decisions with |p0 − draw| <= 1e-12 (the device's exp and libm's can differ in the last bit); for its
    seeds the reference has none, so nothing is left out there. Two seeds give two traces; the draws lie in [0, 1) and differ per (env, step)."""
    p = V.a2c_perturbed(4)
    outs = [V.evaluate(V.A2C, p, seed=s, mode=V.SAMPLE, **SAMPLE_CASE) for s in SAMPLE_SEEDS]
    for out in outs:
        used = out["trace_action"] >= 0
        assert used.sum() == out["lengths"].sum() > 60
        margin = np.abs(out["p0"][used] - out["draws"][used])
        assert margin.min() > 1e-9, "no decision of the reference lies within the tolerance"
        d = out["draws"][used]
        assert (d >= 0).all() and (d < 1).all() and len(np.unique(d)) == d.size
        assert np.array_equal(out["trace_action"][used], (out["p0"][used] <= d).astype(np.int32))
        assert 0.05 < out["p0"][used].min() and out["p0"][used].max() < 0.95 and len(np.unique(out["trace_action"][used])) == 2
    assert not np.array_equal(outs[0]["trace_action"], outs[1]["trace_action"])
    greedy = V.evaluate(V.A2C, p, seed=SAMPLE_SEEDS[0], **SAMPLE_CASE)
    assert not np.array_equal(greedy["trace_action"], outs[0]["trace_action"]), "sampling is not the argmax"


# ---------------------------------------------------------------------------------------------------- the surface, without a device
class _NoDevice:
    """stands where an agent's handle would: any call into the library is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were validated")


@pytest.mark.parametrize("algo", ["dqn", "a2c"])
def test_evaluate_rejects_bad_arguments_before_any_device(algo):
    import cleanrl_jl_amd as crl
    L = crl._lib
    agent = object.__new__(crl.DQNAgent if algo == "dqn" else crl.A2CAgent)
    agent.handle = _NoDevice()
    agent.crl_cfg = L.CrlDQNConfig(max_steps=200) if algo == "dqn" else L.CrlA2CConfig(max_steps=500)
    fn, per_episode = (crl.dqn_evaluate, 201) if algo == "dqn" else (crl.a2c_evaluate, 501)
    for kw, field in ((dict(num_envs=0), "num_envs"), (dict(num_envs=65537), "num_envs"), (dict(num_envs=True), "num_envs"),
                      (dict(episodes_per_env=0), "episodes_per_env"), (dict(num_envs=65536, episodes_per_env=17), r"num_envs \* episodes_per_env"),
                      (dict(seed=2 ** 64), "seed"), (dict(trace_steps=-1), "trace_steps"),
                      (dict(episodes_per_env=2, trace_steps=2 * per_episode + 1), r"trace_steps must be <= episodes_per_env \* \(max_steps \+ 1\) = %d" % (2 * per_episode)),
                      (dict(num_envs=65536, episodes_per_env=2, trace_steps=257), r"trace_steps \* num_envs")):
        with pytest.raises(ValueError, match=f"{algo}_evaluate: " + field):
            fn(agent, **kw)
    with pytest.raises(AssertionError, match="the library was touched"):        # the largest trace passes the checks and reaches the handle
        fn(agent, episodes_per_env=2, trace_steps=2 * per_episode)
    with pytest.raises(TypeError):
        fn(object())
    train = crl.dqn if algo == "dqn" else crl.a2c
    for kw, msg in ((dict(eval_every=-1), "eval_every"), (dict(eval_every=1.5), "eval_every"), (dict(eval_every=10, eval_envs=0), "num_envs"),
                    (dict(eval_every=10, eval_episodes=1025), "episodes_per_env")):
        with pytest.raises(ValueError, match=f"{algo}: " + msg):
            train(None, **kw)


def test_mirrors_and_header_agree():
    import ctypes as C
    import cleanrl_jl_amd as crl
    L = crl._lib
    assert C.sizeof(L.CrlValueEvalReport) == 80 and [n for n, _ in L.CrlValueEvalReport._fields_] == [
        "episodes", "env_steps", "return_mean", "return_std", "return_min", "return_max", "length_mean", "disc_return_mean", "v0_mean", "v_bias_mean"]
    header = open(os.path.join(ROOT, "include", "cleanrl_hip.h")).read()
    for name in ("crl_dqn_evaluate", "crl_a2c_evaluate", "crl_a2c_forward", "crl_dqn_eval_envs_per_block", "crl_a2c_eval_envs_per_block"):
        assert re.search(r"int32_t %s\(" % name, header) and name in L.EXPORTS, name
    fields = re.search(r"typedef struct crl_value_eval_report \{([^}]*)\}", header).group(1)
    assert re.findall(r"\w+(?=[,;])", fields) == [n for n, _ in L.CrlValueEvalReport._fields_]
    assert "0x20" in header and "0x21" in header


def test_the_rest_of_the_surface_names_the_calls():
    jl = open(os.path.join(ROOT, "julia", "CleanRLHip.jl")).read()
    exports = jl[jl.index("export"):jl.index("const libcrl")]
    for name in ("dqn_evaluate", "a2c_evaluate", "a2c_forward"):
        assert name in exports and re.search(r"function %s\(" % name, jl), name
    for sym in (":crl_dqn_evaluate", ":crl_a2c_evaluate", ":crl_a2c_forward"):
        assert sym in jl, sym
    assert jl.count("(Ptr{Cvoid}, Ref{CrlEvalConfig}, Ref{CrlValueEvalReport}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32})") == 2
    mirror = jl[jl.index("struct CrlValueEvalReport"):]
    mirror = mirror[:mirror.index("\nend")]
    assert re.findall(r"(\w+)::(\w+)", mirror) == [("episodes", "Int64"), ("env_steps", "Int64")] + [(n, "Float64") for n in (
        "return_mean", "return_std", "return_min", "return_max", "length_mean", "disc_return_mean", "v0_mean", "v_bias_mean")]
    for fn in ("function dqn(", "function a2c("):
        sig = jl[jl.index(fn):]
        assert "eval_every::Integer=0, eval_envs::Integer=256, eval_episodes::Integer=1" in sig[:sig.index(")\n")], fn
    run = open(os.path.join(ROOT, "scripts", "run.py")).read()
    for algo in ('algo == "a2c"', "else:"):
        branch = run[run.rindex(algo):]
        for flag in ("--eval_every", "--eval_envs", "--eval_episodes"):
            assert f'("{flag}", int)' in branch[:branch.index(".close()")], (algo, flag)
        assert "**kw" in branch[:branch.index(".close()")]
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert all(name in text for name in ("crl_dqn_evaluate", "crl_a2c_evaluate", "crl_a2c_forward")), doc
    assert "dqn_evaluate" in open(os.path.join(ROOT, "VERIFY_WITH_JULIA.md")).read()
