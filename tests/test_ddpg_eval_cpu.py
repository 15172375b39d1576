"""CPU-side checks of the DDPG evaluation entry (crl_ddpg_evaluate): the header declares it, the ctypes and Julia mirrors follow the header, the
Python shell validates its arguments before any device is touched, and the reference of tests/ddpg_eval_ref.py — the yardstick of
tests/test_gpu_ddpg_eval.py — is itself checked against hand-written loops, including the saturated wrap-and-clamp case the GPU test reuses."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ddpg_eval_ref as V
import ddpg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cleanrl_hip.h")
CONFIG_FIELDS = ["num_envs", "episodes_per_env", "trace_steps", "pad", "seed"]
REPORT_FIELDS = ["episodes", "env_steps", "return_mean", "return_std", "return_min", "return_max", "disc_return_mean", "q0_mean", "q_bias_mean"]


@pytest.fixture(scope="module")
def crl():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "cleanrl.jl_amd", "libcleanrl_hip.so")):
        g.build()
    import cleanrl_jl_amd as crl
    return crl


def _header_fields(cname):
    hdr = open(HDR).read()
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S)
    assert m, f"{cname} is not declared in the header"
    names = []
    for ctype, decl in re.findall(r"(int64_t|int32_t|double|uint64_t)\s+([a-z_0-9, ]+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)):
        names += [(n.strip(), ctype) for n in decl.split(",")]
    return names


# ---------------------------------------------------------------------------------------------------- the surface
def test_header_declares_the_function_and_both_structs():
    hdr = open(HDR).read()
    assert re.search(r"int32_t crl_ddpg_evaluate\(crl_ddpg\* h, const crl_ddpg_eval_config\* cfg, crl_ddpg_eval_report\* report,\s*"
                     r"double\* returns, double\* disc_returns, double\* q0, double\* trace_action\);", hdr)
    assert [n for n, _ in _header_fields("crl_ddpg_eval_config")] == CONFIG_FIELDS
    assert [n for n, _ in _header_fields("crl_ddpg_eval_report")] == REPORT_FIELDS
    doc = hdr[hdr.index("int32_t crl_ddpg_q_values("):hdr.index("int32_t crl_ddpg_evaluate(")]
    for must in ("0x16", "crl_ddpg_actor", "crl_ddpg_q_values", "1..65536", "1..1024", "1048576", "16777216", "population standard deviation"):
        assert must in doc, must


def test_ctypes_mirrors_follow_the_header(crl, tmp_path):
    L = crl._lib
    ctmap = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
    for cname, mirror in (("crl_ddpg_eval_config", L.CrlDDPGEvalConfig), ("crl_ddpg_eval_report", L.CrlDDPGEvalReport)):
        assert [(n, ctmap[t]) for n, t in _header_fields(cname)] == list(mirror._fields_), cname
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "cleanrl_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(crl_ddpg_eval_config), sizeof(crl_ddpg_eval_report)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(L.CrlDDPGEvalConfig), C.sizeof(L.CrlDDPGEvalReport)] == [24, 72]
    assert "crl_ddpg_evaluate" in L.EXPORTS and L.load().crl_ddpg_evaluate.restype is C.c_int32


def test_julia_shell_mirrors_and_ccall():
    jl = open(os.path.join(ROOT, "julia", "CleanRLHip.jl")).read()
    jt = {"int32_t": "Int32", "int64_t": "Int64", "uint64_t": "UInt64", "double": "Float64"}
    for jname, cname in (("CrlDDPGEvalConfig", "crl_ddpg_eval_config"), ("CrlDDPGEvalReport", "crl_ddpg_eval_report")):
        m = re.search(r"struct %s\b(.*?)\bend" % jname, jl, re.S)
        assert m, jname
        got = re.findall(r"([A-Za-z_][A-Za-z_0-9]*)::([A-Za-z0-9]+)", re.sub(r"#.*", "", m.group(1)))
        assert got == [(n, jt[t]) for n, t in _header_fields(cname)], jname
    call = re.search(r"ccall\(\(:crl_ddpg_evaluate, libcrl\), Int32,\s*\((.*?)\),", jl, re.S)
    assert call and [a.strip() for a in call.group(1).split(",")] == ["Ptr{Cvoid}", "Ref{CrlDDPGEvalConfig}", "Ref{CrlDDPGEvalReport}", "Ptr{Float64}",
                                                                      "Ptr{Float64}", "Ptr{Float64}", "Ptr{Float64}"]
    assert re.search(r"function ddpg_evaluate\(agent::DDPGAgent; num_envs::Integer=256, episodes_per_env::Integer=1, seed::Integer=EVAL_SEED, "
                     r"trace_steps::Integer=0\)", jl)
    assert "ddpg_evaluate" in jl[jl.index("export"):jl.index("const libcrl")]


def test_the_rest_of_the_surface_names_the_call():
    run = open(os.path.join(ROOT, "scripts", "run.py")).read()
    ddpg_branch = run[run.index('algo == "ddpg"'):]
    ddpg_branch = ddpg_branch[:ddpg_branch.index("else:")]
    for flag in ("--eval_every", "--eval_envs", "--eval_episodes"):
        assert f'("{flag}", int)' in ddpg_branch, flag
    assert "**kw" in ddpg_branch
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "crl_ddpg_evaluate" in open(os.path.join(ROOT, doc)).read(), doc


class _NoDevice:
    """stands where an agent's handle would: any call into the library is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were validated")


def _agent(crl):
    agent = object.__new__(crl.DDPGAgent)
    agent.handle = _NoDevice()
    agent.config = crl.DDPGConfig()
    agent.crl_cfg = crl._lib.CrlDDPGConfig(max_steps=200)
    return agent


def test_ddpg_evaluate_rejects_bad_arguments_before_any_device(crl):
    agent = _agent(crl)
    bad = [dict(num_envs=0), dict(num_envs=-3), dict(num_envs=2.5), dict(num_envs=True), dict(num_envs=65537), dict(episodes_per_env=0),
           dict(episodes_per_env="2"), dict(episodes_per_env=1025), dict(num_envs=65536, episodes_per_env=17), dict(trace_steps=-1),
           dict(trace_steps=201), dict(episodes_per_env=2, trace_steps=401), dict(num_envs=65536, episodes_per_env=2, trace_steps=257),
           dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5)]
    for kw in bad:
        with pytest.raises(ValueError, match="ddpg_evaluate"):
            crl.ddpg_evaluate(agent, **kw)
    env = R.Pendulum(seed=1)
    for kw in (dict(num_envs=2), dict(seed=5), dict(trace_steps=1), dict(episodes_per_env=0)):   # a host env: one env, seeded and traced by its owner
        with pytest.raises(ValueError, match="ddpg_evaluate"):
            crl.ddpg_evaluate(agent, env=env, **kw)
    with pytest.raises(ValueError, match="host env object"):
        crl.ddpg_evaluate(agent, env="pendulum")
    with pytest.raises(TypeError, match="DDPGAgent"):
        crl.ddpg_evaluate(object())
    with pytest.raises(TypeError):
        crl.ddpg_evaluate(agent, 64)                                    # keywords only
    sig = inspect.signature(crl.ddpg_evaluate)
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} == \
        dict(num_envs=256, episodes_per_env=1, seed=0xE7A1, trace_steps=0, env=None)
    for kw in (dict(num_envs=8), dict(num_envs=65536, episodes_per_env=16, trace_steps=256), dict(env=env)):   # good arguments do reach the handle
        with pytest.raises(AssertionError, match="library was touched"):
            crl.ddpg_evaluate(agent, **kw)


def test_ddpg_rejects_bad_eval_arguments_before_any_device(crl, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a handle was created before the arguments were validated")
    monkeypatch.setattr(crl._lib, "DDPGHandle", no_device)
    p = inspect.signature(crl.ddpg).parameters
    assert (p["eval_every"].default, p["eval_envs"].default, p["eval_episodes"].default, p["eval_env"].default) == (0, 256, 1, None)
    cfg = crl.DDPGConfig(run_name="never", total_timesteps=10)
    for kw in (dict(eval_every=-1), dict(eval_every=2.5), dict(eval_every=True), dict(eval_every=5, eval_envs=0), dict(eval_every=5, eval_envs=65537),
               dict(eval_every=5, eval_episodes=0), dict(eval_every=5, eval_episodes=1025)):
        with pytest.raises(ValueError, match="ddpg"):
            crl.ddpg(cfg, "pendulum", **kw)
    env = R.Pendulum(seed=1)
    with pytest.raises(ValueError, match="eval_env"):                   # evaluating on the training env would break its episode
        crl.ddpg(cfg, env, eval_every=5)
    with pytest.raises(ValueError, match="eval_env"):
        crl.ddpg(cfg, env, eval_every=5, eval_env=env)
    with pytest.raises(AssertionError, match="handle was created"):     # good arguments do go on to the device
        crl.ddpg(cfg, "pendulum", eval_every=5, log_dir=None, to_json=False, to_tensorboard=False)


# ---------------------------------------------------------------------------------------------------- the reference
def test_a_zero_actor_gives_the_free_pendulum():
    """An all-zero actor answers exactly 0.0 to every observation, and the reference's returns are those of a hand-written torque-free loop."""
    na, _ = R.param_count(3, 1)
    actor = np.zeros(na, np.float32)
    n, E, seed, T, gamma = 3, 2, 21, 30, 0.97
    out = V.evaluate(actor, None, n, E, seed, T, gamma)
    assert not out["trace_action"].any() and not np.signbit(out["trace_action"]).any()
    for e in range(n):
        for j in range(E):
            u = R.uniform(seed, np.arange(2), j * n + e, 0x16)
            th, thd = np.float64(-R.PI + (2.0 * R.PI) * u[0]), np.float64(-1.0 + 2.0 * u[1])
            ret, disc_ret, disc = np.float64(0.0), np.float64(0.0), np.float64(1.0)
            for _ in range(T):
                r = -(th * th + 0.1 * (thd * thd) + 0.001 * 0.0)
                thd = min(max(thd + (15.0 * R.pend_sin(th) + 0.0) * 0.05, -8.0), 8.0)
                th = th + thd * 0.05
                th = th - 2.0 * R.PI if th >= R.PI else (th + 2.0 * R.PI if th < -R.PI else th)
                ret = ret + r; disc_ret = disc_ret + disc * r; disc = disc * np.float64(gamma)
            assert out["returns"][j, e] == ret and out["disc_returns"][j, e] == disc_ret, (e, j)
    assert len(set(out["returns"].reshape(-1))) == n * E                # every (env, episode) starts somewhere else


def test_the_report_formulas_on_a_hand_made_array():
    ret = np.array([[-4.0, -2.0], [-1.0, -5.0]]); disc = np.array([[-3.0, -1.5], [-0.5, -4.0]]); q0 = np.array([[-2.0, -2.5], [1.5, -4.0]])
    rep = V.report(ret, disc, q0, 7)
    assert rep == dict(episodes=4, env_steps=28, return_mean=-3.0, return_std=float(np.sqrt(2.5)), return_min=-5.0, return_max=-1.0,
                       disc_return_mean=-2.25, q0_mean=-1.75, q_bias_mean=0.5)
    from cleanrl_jl_amd.ddpg import eval_report
    assert eval_report(ret, disc, q0, 28) == rep                        # the shell's helper (host-env route) states the same formulas
    rng = np.random.default_rng(0)
    r, d, q = rng.standard_normal((3, 5, 67)) * 100.0
    assert eval_report(r, d, q, 5 * 67 * 9) == V.report(r, d, q, 9)
    assert V.report(r, d, q, 9)["return_mean"] == pytest.approx(r.mean(), rel=1e-12)
    assert V.report(r, d, q, 9)["return_std"] == pytest.approx(r.std(), rel=1e-12)


def test_the_evaluation_reset_stream_is_its_own():
    seed = 0xE7A1
    for g in (0, 1, 5, 2 ** 33):
        draws = [R.pendulum_reset(seed, g, s) for s in (V.S_EVAL, R.S_RESET, R.S_RESET0)]
        assert len({d for d in draws}) == 3, g
        th, thd = draws[0]
        assert -R.PI <= th < R.PI and -1.0 <= thd < 1.0
    assert V.S_EVAL == 0x16 and V.S_EVAL not in (R.S_BEHAVE, R.S_WARMUP, R.S_TARGET, R.S_ACTOR, R.S_RESET, R.S_RESET0, R.S_SAMPLE)


def test_the_hard_case_saturates_wraps_and_clamps():
    """The case tests/test_gpu_ddpg_eval.py runs on the device, pinned here by the reference alone: the head saturates to exactly ±2 (tanh_fast's
    sign branch), and the rollout wraps θ and clamps θ̇ — so the GPU twin cannot pass without meeting those branches."""
    actor = V.hard_actor()
    out = V.evaluate(actor, None, **V.HARD)
    acts = out["trace_action"]
    assert set(np.unique(acts)) == {-2.0, 2.0}
    assert out["wrapped"] >= 1 and out["clamped"] >= 1
    assert np.abs(out["theta_dot"]).max() == 8.0 and (out["theta"] >= -R.PI).all() and (out["theta"] < R.PI).all()
    W3, b3 = R.split(actor, 3, 1)[4:]
    h2 = R.actor_forward(actor, 3, 1, out["obs"].reshape(-1, 3).T)[1]
    assert (np.abs(R.dense(W3, b3, h2)) > 30.0).all(), "every head pre-activation is in the sign branch (x² > 900)"
