"""CPU-side checks of the evaluation entry (crl_ppo_evaluate): the header declares it, the ctypes and Julia mirrors follow the header, the
Python shell validates its arguments before any device is touched, eval_every = 0 leaves the record stream alone, and without a GPU the call
fails loudly."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cleanrl_hip.h")


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
    for ctype, decl in re.findall(r"(int64_t|int32_t|double|uint64_t)\s+([a-z_, ]+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)):
        names += [(n.strip(), ctype) for n in decl.split(",")]
    return names


def test_header_declares_the_function_and_both_structs():
    hdr = open(HDR).read()
    assert re.search(r"int32_t crl_ppo_evaluate\(crl_ppo\* h, const crl_eval_config\* cfg, crl_eval_report\* report,\s*float\* returns, "
                     r"int32_t\* lengths, int32_t\* trace_action\);", hdr)
    assert "#define CRL_EVAL_GREEDY 0" in hdr and "#define CRL_EVAL_SAMPLE 1" in hdr
    assert [n for n, _ in _header_fields("crl_eval_config")] == ["num_envs", "episodes_per_env", "mode", "trace_steps", "seed"]
    assert [n for n, _ in _header_fields("crl_eval_report")] == ["episodes", "env_steps", "return_mean", "return_std", "return_min", "return_max",
                                                                  "length_mean"]
    assert "num_envs <= 1048576" in hdr, "the header states the caps"


def test_ctypes_mirrors_follow_the_header(crl, tmp_path):
    L = crl._lib
    ctmap = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double}
    for cname, mirror in (("crl_eval_config", L.CrlEvalConfig), ("crl_eval_report", L.CrlEvalReport)):
        want = _header_fields(cname)
        assert [(n, ctmap[t]) for n, t in want] == list(mirror._fields_), cname
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "cleanrl_hip.h"\n'
                   'int main(void) { printf("%zu %zu %d %d\\n", sizeof(crl_eval_config), sizeof(crl_eval_report), CRL_EVAL_GREEDY, CRL_EVAL_SAMPLE); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in out] == [C.sizeof(L.CrlEvalConfig), C.sizeof(L.CrlEvalReport), L.EVAL_GREEDY, L.EVAL_SAMPLE] == [24, 56, 0, 1]
    assert "crl_ppo_evaluate" in L.EXPORTS and L.load().crl_ppo_evaluate.restype is C.c_int32


def test_julia_shell_mirrors_and_ccall(crl):
    jl = open(os.path.join(ROOT, "julia", "CleanRLHip.jl")).read()
    jt = {"int32_t": "Int32", "int64_t": "Int64", "uint64_t": "UInt64", "double": "Float64"}
    for jname, cname in (("CrlEvalConfig", "crl_eval_config"), ("CrlEvalReport", "crl_eval_report")):
        m = re.search(r"struct %s\b(.*?)\bend" % jname, jl, re.S)
        assert m, jname
        got = re.findall(r"([A-Za-z_][A-Za-z_0-9]*)::([A-Za-z0-9]+)", re.sub(r"#.*", "", m.group(1)))
        assert got == [(n, jt[t]) for n, t in _header_fields(cname)], jname
    call = re.search(r"ccall\(\(:crl_ppo_evaluate, libcrl\), Int32,\s*\((.*?)\),", jl, re.S)
    assert call and [a.strip() for a in call.group(1).split(",")] == ["Ptr{Cvoid}", "Ref{CrlEvalConfig}", "Ref{CrlEvalReport}", "Ptr{Float32}",
                                                                      "Ptr{Int32}", "Ptr{Int32}"]
    assert re.search(r"function evaluate\(a::Agent; num_envs::Integer=256, episodes_per_env::Integer=1, greedy::Bool=true", jl)
    assert re.search(r"function ppo\(config::PPOConfig=PPOConfig\(\);.*?eval_every::Integer=0, eval_envs::Integer=256, eval_episodes::Integer=1, shape\.\.\.\)", jl, re.S)
    assert '@info "Evaluation Statistics" eval_return_mean' in jl and "evaluate" in jl[jl.index("export"):jl.index("const libcrl")]


class _NoDevice:
    """stands where an Agent's handle would: any call into the library is a test failure"""
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the arguments were validated")


def test_evaluate_rejects_bad_arguments_before_any_device(crl):
    agent = object.__new__(crl.Agent)
    agent.handle = _NoDevice()
    bad = [dict(num_envs=0), dict(num_envs=-3), dict(num_envs=2.5), dict(num_envs=True), dict(episodes_per_env=0), dict(episodes_per_env="2"),
           dict(trace_steps=-1), dict(seed=-1), dict(seed=2 ** 64), dict(greedy=1), dict(num_envs=(1 << 20) + 1), dict(episodes_per_env=4097),
           dict(num_envs=1 << 20, episodes_per_env=32), dict(num_envs=1 << 20, trace_steps=128)]
    for kw in bad:
        with pytest.raises((ValueError, TypeError), match="evaluate"):
            crl.evaluate(agent, **kw)
    with pytest.raises(TypeError, match="Agent"):
        crl.evaluate(object())
    with pytest.raises(TypeError):
        crl.evaluate(agent, 64)                                       # keywords only
    sig = inspect.signature(crl.evaluate)
    assert {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty} | {"seed": None} == \
        dict(num_envs=256, episodes_per_env=1, greedy=True, seed=None, trace_steps=0)
    with pytest.raises(AssertionError, match="library was touched"):   # good arguments do reach the handle
        crl.evaluate(agent, num_envs=8)


def test_eval_every_zero_adds_no_record_type(crl):
    """ppo(eval_every=0) is today's loop: the defaults are 0 / 256 / 1, train() with 0 never reaches the evaluation branch (a handle without an
    evaluate method serves it), and bad eval arguments are refused before any launch."""
    import logging
    for fn in (crl.ppo, crl.train):
        p = inspect.signature(fn).parameters
        assert (p["eval_every"].default, p["eval_envs"].default, p["eval_episodes"].default) == (0, 256, 1)

    class Handle:
        iteration = 0
        calls = 0

        def env_reset(self):
            pass

        def iterate_async(self, want_stats=True):
            self.calls += 1
            return None if self.calls == 1 else self._rep(self.calls - 2)

        def drain(self, want_stats=True):
            return self._rep(self.calls - 1)

        @staticmethod
        def _rep(it):
            s = dict(loss=1.0, pg_loss=0.5, v_loss=0.25, entropy_loss=0.125)
            return {"iteration": it, "stats": [s, s], "episodes": dict(episodes=0, return_sum=0.0, length_sum=0.0, return_max=0.0), "records": [], "n_episodes": 0}

    class Collect(logging.Handler):
        def __init__(self):
            super().__init__()
            self.msgs = []

        def emit(self, record):
            self.msgs.append(record.getMessage())

    agent = object.__new__(crl.Agent)
    agent.config = crl.PPOConfig(num_envs=4, num_steps=8, total_timesteps=4 * 8 * 3)
    agent.handle = Handle()
    lg = logging.getLogger("CleanRL"); col = Collect(); lg.addHandler(col); old = lg.level; lg.setLevel(logging.INFO)
    try:
        crl.train(agent, eval_every=0)
        assert set(col.msgs) == {"Training Statistics"} and len(col.msgs) == 6
        with pytest.raises(ValueError):
            crl.train(agent, eval_every=-1)
        with pytest.raises(ValueError, match="num_envs"):
            crl.train(agent, eval_every=2, eval_envs=0)
        with pytest.raises(AttributeError, match="evaluate"):           # eval_every > 0 does go to the handle's evaluate
            crl.train(agent, eval_every=1)
    finally:
        lg.removeHandler(col); lg.setLevel(old)


def test_run_script_takes_the_eval_flags():
    src = open(os.path.join(ROOT, "scripts", "run.py")).read()
    for flag in ("--eval_every", "--eval_envs", "--eval_episodes"):
        assert f'("{flag}", int)' in src, flag


def test_without_a_gpu_the_call_fails_loudly(crl):
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present")
    L = crl._lib
    cfg = L.CrlEvalConfig(8, 1, 0, 0, 1); rep = L.CrlEvalReport()
    assert L.load().crl_ppo_evaluate(None, C.byref(cfg), C.byref(rep), None, None, None) != 0
    assert b"null crl_ppo handle" in L.load().crl_last_error()
    with pytest.raises(crl.CrlError):                                   # no handle can exist without a device: nothing evaluates on the CPU
        crl.evaluate(crl.Agent(crl.PPOConfig()), num_envs=8)
