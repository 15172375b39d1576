"""CPU-side checks of the diagnostics entry (crl_ppo_diagnose): the Float64 reference of tests/diag_ref.py on cases worked by hand, the header,
the ctypes and Julia mirrors, and the Python shell's argument checks, which run before any device is touched."""
import ctypes as C
import inspect
import logging
import math
import os
import re

import numpy as np
import pytest

import diag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cleanrl_hip.h")
FIELDS = ["n", "n_clipped", "sum_logratio", "sum_kl", "sum_entropy", "ratio_min", "ratio_max", "sum_ret", "sum_ret2", "sum_res_old", "sum_res_old2",
          "sum_res_new", "sum_res_new2", "old_approx_kl", "approx_kl", "clipfrac", "entropy", "explained_variance", "explained_variance_new"]


@pytest.fixture(scope="module")
def crl():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "cleanrl.jl_amd", "libcleanrl_hip.so")):
        g.build()
    import cleanrl_jl_amd as crl
    return crl


def test_reference_on_a_hand_computed_case():
    """three samples, two actions; every figure below is written out from the definitions, not taken from the function"""
    f = np.float32
    lp_old = np.array([-0.5, -1.0, -0.25], f)
    lp_new = np.array([-0.25, -1.5, -0.25], f)                       # log-ratios 0.25, -0.5, 0: all exact in Float32
    ent = np.array([[0.25, 0.5, 0.125], [0.25, 0.125, 0.0]], f)      # per-sample entropies 0.5, 0.625, 0.125
    ret = np.array([1.0, 2.0, 3.0], f); value = np.array([0.5, 2.0, 4.0], f); v_new = np.array([1.0, 1.0, 3.0], f)
    d, tol = R.diag_ref(lp_new, ent, v_new, lp_old, value, ret, 0.2)
    ratios = [math.exp(0.25), math.exp(-0.5), 1.0]
    assert d["n"] == 3 and d["n_clipped"] == 2                       # e^0.25 - 1 = 0.284 and 1 - e^-0.5 = 0.393 are past 0.2, 0 is not
    assert d["sum_logratio"] == -0.25 and d["old_approx_kl"] == 0.25 / 3
    assert d["sum_kl"] == pytest.approx((ratios[0] - 1 - 0.25) + (ratios[1] - 1 + 0.5), rel=1e-15)
    assert d["approx_kl"] == d["sum_kl"] / 3 and d["clipfrac"] == 2 / 3
    assert d["sum_entropy"] == 1.25 and d["entropy"] == 1.25 / 3
    assert d["ratio_min"] == ratios[1] and d["ratio_max"] == ratios[0]
    assert (d["sum_ret"], d["sum_ret2"]) == (6.0, 14.0)              # Var(ret) = 14/3 - 4 = 2/3
    assert (d["sum_res_old"], d["sum_res_old2"]) == (-0.5, 1.25)     # residuals 0.5, 0, -1: Var = 1.25/3 - 1/36 = 7/18
    assert (d["sum_res_new"], d["sum_res_new2"]) == (1.0, 1.0)       # residuals 0, 1, 0: Var = 1/3 - 1/9 = 2/9
    assert d["explained_variance"] == pytest.approx(1 - (7 / 18) / (2 / 3), rel=1e-14)
    assert d["explained_variance_new"] == pytest.approx(1 - (2 / 9) / (2 / 3), rel=1e-14)
    assert tol["old_approx_kl"] == pytest.approx((1e-5 * (0.25 + 1.5 + 0.25) / 3) + 1e-6, rel=1e-12)
    assert tol["undecided"] == 0
    assert R.derived(d) == {k: d[k] for k in ("old_approx_kl", "approx_kl", "clipfrac", "entropy", "explained_variance", "explained_variance_new")}


def test_identical_logprobs_and_constant_returns():
    rng = np.random.default_rng(0)
    lp = np.log(rng.uniform(0.1, 0.9, 40)).astype(np.float32)
    ent = rng.uniform(0, 0.3, (3, 40)).astype(np.float32)
    ret = np.full(40, 1.0, np.float32); value = rng.normal(size=40).astype(np.float32)
    d, tol = R.diag_ref(lp, ent, value, lp, value, ret, 0.2)
    assert d["sum_kl"] == 0.0 and d["approx_kl"] == 0.0 and d["old_approx_kl"] == 0.0 and d["clipfrac"] == 0.0 and d["n_clipped"] == 0
    assert d["ratio_min"] == 1.0 and d["ratio_max"] == 1.0
    assert math.isnan(d["explained_variance"]) and math.isnan(d["explained_variance_new"]) and math.isnan(tol["explained_variance_new"])
    ret2 = rng.normal(size=40).astype(np.float32)
    d2, _ = R.diag_ref(lp, ent, ret2, lp, ret2, ret2, 0.2)          # a critic that predicts the returns exactly explains all of their variance
    assert d2["explained_variance"] == 1.0 and d2["explained_variance_new"] == 1.0


def test_header_ctypes_and_julia_mirrors_agree(crl):
    hdr = open(HDR).read()
    assert re.search(r"int32_t crl_ppo_diagnose\(crl_ppo\* h, crl_ppo_diag\* out, float\* new_logprob, float\* new_value\);", hdr)
    m = re.search(r"typedef struct crl_ppo_diag \{(.*?)\} crl_ppo_diag;", hdr, re.S)
    assert m, "crl_ppo_diag is not declared in the header"
    want = []
    for ctype, decl in re.findall(r"(int64_t|double)\s+([a-z_0-9, ]+);", m.group(1)):
        want += [(n.strip(), ctype) for n in decl.split(",")]
    assert [n for n, _ in want] == FIELDS
    L = crl._lib
    ctmap = {"int64_t": C.c_int64, "double": C.c_double}
    assert [(n, ctmap[t]) for n, t in want] == list(L.CrlDiag._fields_)
    assert C.sizeof(L.CrlDiag) == 8 * len(FIELDS)
    assert "crl_ppo_diagnose" in L.EXPORTS and L.load().crl_ppo_diagnose.restype is C.c_int32
    for phrase in ("no reference counterpart", "n_act times the reference's entropy_loss", "post-update parameters"):
        assert phrase in hdr, phrase
    jl = open(os.path.join(ROOT, "julia", "CleanRLHip.jl")).read()
    jm = re.search(r"struct CrlDiag\b[^\n]*\n(.*?)\nend", jl, re.S)
    assert jm, "julia/CleanRLHip.jl has no CrlDiag"
    jfields = re.findall(r"([a-z_0-9]+)::(Int64|Float64)", jm.group(1))
    assert jfields == [(n, "Int64" if t == "int64_t" else "Float64") for n, t in want]
    assert ":crl_ppo_diagnose" in jl and "function diagnose(a::Agent" in jl


def test_diag_every_is_validated_before_any_device_is_touched(crl, monkeypatch):
    for fn in (crl.ppo, crl.train):
        assert inspect.signature(fn).parameters["diag_every"].default == 0
    monkeypatch.setattr(crl.Agent, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was touched")))

    class Handle:                                                      # anything train() could do to a device raises
        def __getattr__(self, name):
            raise AssertionError("the library was touched")

    agent = object.__new__(crl.Agent)
    agent.config = crl.PPOConfig(num_envs=4, num_steps=8, total_timesteps=4 * 8 * 3)
    agent.handle = Handle()
    for bad in (-1, 1.5, "2", True, None.__class__):
        with pytest.raises(ValueError, match="diag_every"):
            crl.train(agent, diag_every=bad)
        with pytest.raises(ValueError, match="diag_every"):
            crl.ppo(crl.PPOConfig(num_envs=4, num_steps=8, total_timesteps=96), diag_every=bad, logger_kw=dict(to_tensorboard=False))
    with pytest.raises(AssertionError, match="library was touched"):   # a good value does go on to the device
        crl.train(agent, diag_every=2)
    with pytest.raises(TypeError, match="Agent"):
        crl.diagnose(object())
    with pytest.raises(TypeError, match="per_sample"):
        crl.diagnose(agent, per_sample=1)


def test_diag_every_places_the_record_behind_the_updates_own(crl):
    """train() against a stand-in handle: diag_every = 2 over three updates gives one "Policy Diagnostics" record, right behind the second update's
    records, with the documented keys; diag_every = 0 gives none."""
    class Handle:
        iteration = 0
        calls = 0
        diagnosed = 0

        def env_reset(self):
            pass

        def iterate_async(self, want_stats=True):
            self.calls += 1
            return None if self.calls == 1 or self.drained == self.calls - 1 else self._rep(self.calls - 2)

        drained = 0

        def drain(self, want_stats=True):
            if self.drained == self.calls:
                return None
            self.drained = self.calls
            return self._rep(self.calls - 1)

        def diagnose(self):
            self.diagnosed += 1
            return dict(approx_kl=0.01, old_approx_kl=0.02, clipfrac=0.1, entropy=0.6, explained_variance=0.5, explained_variance_new=0.6)

        @staticmethod
        def _rep(it):
            s = dict(loss=1.0, pg_loss=0.5, v_loss=0.25, entropy_loss=0.125)
            return {"iteration": it, "stats": [s, s], "episodes": dict(episodes=0, return_sum=0.0, length_sum=0.0, return_max=0.0), "records": [], "n_episodes": 0}

    class Collect(logging.Handler):
        def __init__(self):
            super().__init__()
            self.recs = []

        def emit(self, record):
            self.recs.append((record.getMessage(), getattr(record, "crl", None)))

    lg = logging.getLogger("CleanRL"); old = lg.level; lg.setLevel(logging.INFO)
    out = {}
    for every in (0, 2):
        agent = object.__new__(crl.Agent)
        agent.config = crl.PPOConfig(num_envs=4, num_steps=8, total_timesteps=4 * 8 * 3)
        agent.handle = Handle()
        col = Collect(); lg.addHandler(col)
        try:
            crl.train(agent, diag_every=every)
        finally:
            lg.removeHandler(col)
        out[every] = col.recs
    lg.setLevel(old)
    assert [m for m, _ in out[0]] == ["Training Statistics"] * 6
    assert [m for m, _ in out[2]] == ["Training Statistics"] * 4 + ["Policy Diagnostics"] + ["Training Statistics"] * 2
    rec = out[2][4][1]
    assert set(rec) == {"approx_kl", "old_approx_kl", "clipfrac", "entropy", "explained_variance", "global_step"} and rec["global_step"] == 2 * 32


def test_run_script_takes_the_diag_flag():
    src = open(os.path.join(ROOT, "scripts", "run.py")).read()
    assert '("--diag_every", int)' in src
