"""crl_ppo_diagnose (csrc/diag.hip) on the GPU against the CPU oracle: per-sample log-probabilities and values, every scalar of the report within the
tolerance tests/diag_ref.py derives for it, the derived fields from the sums exactly, determinism, non-interference with training at bit level,
independence of the handle's routes, errors, and ppo(diag_every=…).

A case fills the buffer (crl_env_reset / crl_rollout_run / crl_compute_gae; for the synthetic shapes the five fields are written), diagnoses it with
the parameters that drew it, then adds Gaussian noise (fixed seed, SIGMA per shape) to actor and critic through a CRL_F_PARAMS write and diagnoses
again. SIGMA was chosen on the CPU with the oracle so that the reference clip fraction lies in [0.05, 0.5] and the undecided samples stay under 1 % of
the batch; both are asserted on the reference. Each case is built once per module and shared by the tests that read it.

Every GPU step runs under its own watchdog (`limit`)."""
import json
import logging
import math

import numpy as np
import pytest

import diag_ref as R
import oraclelib as O
from test_gpu_eval import limit
from test_gpu_parity import crl  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
SEED = 0x5EED
# name: env (None = synthetic, buffer written), kind, obs_dim, n_act, hidden, num_envs, num_steps, sigma
CASES = {
    "cartpole-65": ("cartpole", 0, 4, 2, 64, 5, 13, 0.1),             # fused path, two full tiles and one sample
    "cartpole-8192-tiles": ("cartpole", 0, 4, 2, 64, 2048, 128, 0.1),  # more tiles than any grid of <= 4 blocks per CU: every block loops
    "mountaincar-64": ("mountaincar", 3, 2, 3, 64, 48, 16, 0.15),
    "acrobot-128": ("acrobot", 4, 6, 3, 128, 48, 16, 0.05),
    "synthetic-8-4-256": (None, 1, 8, 4, 256, 48, 16, 0.04),
    "synthetic-33-16-128": (None, 1, 33, 16, 128, 48, 16, 0.03),     # obs_dim odd and > 8, the largest n_act
    # hidden 256 with W1 too large for LDS: layer 1 reads it from the parameters (the critic's starts at an offset that is no multiple of four floats) —
    "synthetic-33-16-256": (None, 1, 33, 16, 256, 48, 16, 0.02),
    "synthetic-64-16-256": (None, 1, 64, 16, 256, 48, 16, 0.02),     # — and the largest LDS footprint of any shape crl_ppo_create accepts
}
SCALARS = ("old_approx_kl", "approx_kl", "entropy", "explained_variance_new", "explained_variance", "sum_ret", "sum_ret2", "sum_res_old", "sum_res_old2")
_built = {}


def _ocfg(D, A, H, nt, k):
    return O.make_config(num_envs=nt, num_steps=k, obs_dim=D, n_act=A, hidden=H, env_kind=1, seed=SEED)


def _reference(ocfg, params, buf, clip):
    obs = np.asfortranarray(buf["obs"].reshape(ocfg.obs_dim, -1, order="F"))
    act = buf["action"].ravel(order="F")
    lp, ent = O.logprob_actions(ocfg, params, obs, act)
    _, _, v, _ = O.get_action(ocfg, params, obs, np.zeros(act.size), with_value=True)
    ref, tol = R.diag_ref(lp, ent, v, buf["logprob"], buf["value"], buf["ret"], clip)
    return dict(lp=lp, v=v, ref=ref, tol=tol)


def _case(crl, name):   # noqa: F811
    """the handle with its buffer filled, the report with the parameters that drew the buffer, the report after the noise, and the oracle's reference for both"""
    if name in _built:
        return _built[name]
    F = crl._lib
    env, kind, D, A, H, nt, k, sigma = CASES[name]
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 10, num_minibatches=1 if nt * k < 128 else 4)
    p0 = F.make_actor_critic_host(D, A, H, 3)
    agent = crl.Agent(cfg, params=p0, obs_dim=D, n_act=A, hidden=H, env_kind=kind, seed=SEED)
    h = agent.handle; ocfg = _ocfg(D, A, H, nt, k); B = nt * k
    with limit(120):
        if env is not None:
            h.env_reset(); h.rollout_run(); h.compute_gae()
        else:
            rng = np.random.default_rng(1)
            obs = np.asfortranarray(rng.normal(size=(D, B)).astype(np.float32))
            act, lp, val, _ = O.get_action(ocfg, p0, obs, rng.random(B))
            h.write(F.F_OBS, obs); h.write(F.F_ACTION, act); h.write(F.F_LOGPROB, lp); h.write(F.F_VALUE, val)
            h.write(F.F_RETURN, (val + 0.5 * rng.normal(size=B)).astype(np.float32))
        buf = dict(obs=h.read(F.F_OBS), action=h.read(F.F_ACTION), logprob=h.read(F.F_LOGPROB), value=h.read(F.F_VALUE), ret=h.read(F.F_RETURN))
        clean = h.diagnose(per_sample=True)
        p1 = (p0 + np.random.default_rng(11).normal(size=p0.size) * sigma).astype(np.float32)
        h.write(F.F_PARAMS, p1)
        noisy = h.diagnose(per_sample=True)
    clip = agent.crl_cfg.clip_coef
    _built[name] = dict(agent=agent, buf=buf, clean=clean, noisy=noisy, ref_clean=_reference(ocfg, p0, buf, clip), ref_noisy=_reference(ocfg, p1, buf, clip), B=B)
    return _built[name]


def _bits(d):
    return {k: (np.float64(v).view(np.uint64).item() if isinstance(v, float) else v) for k, v in d.items() if not isinstance(v, np.ndarray)}


def _check_against(name, got, want, B):
    ref, tol = want["ref"], want["tol"]
    lp, v = got["new_logprob"].ravel(order="F"), got["new_value"].ravel(order="F")
    e_lp = np.abs(lp.astype(np.float64) - want["lp"]) / R.eps(want["lp"]); e_v = np.abs(v.astype(np.float64) - want["v"]) / R.eps(want["v"])
    print(f"{name}: worst per-sample error / bar: logprob {e_lp.max():.3f} (sample {e_lp.argmax()}), value {e_v.max():.3f} (sample {e_v.argmax()})")
    for key in SCALARS:
        print(f"  {key}: device {got[key]!r} reference {ref[key]!r} |diff| {abs(got[key] - ref[key]):.3e} tolerance {tol[key]:.3e}")
    print(f"  n_clipped: device {got['n_clipped']} reference {ref['n_clipped']} undecided {tol['undecided']}; ratio in [{got['ratio_min']:.4f}, {got['ratio_max']:.4f}]")
    assert e_lp.max() <= 1.0, f"new_logprob of sample {e_lp.argmax()} (tile {e_lp.argmax() // 32})"
    assert e_v.max() <= 1.0, f"new_value of sample {e_v.argmax()} (tile {e_v.argmax() // 32})"
    assert got["n"] == B == ref["n"]
    for key in SCALARS:
        assert abs(got[key] - ref[key]) <= tol[key], key
    assert abs(got["n_clipped"] - ref["n_clipped"]) <= tol["undecided"]
    for key in ("ratio_min", "ratio_max"):                            # d ratio = ratio d lp, doubled like the clip decision's margin, at the largest eps of the case
        assert abs(got[key] - ref[key]) <= 2.0 * ref[key] * R.eps(want["lp"]).max(), key
    derived = R.derived(got)
    for key, val in derived.items():                                  # the header's formulas on the returned sums, exactly
        assert np.float64(val).view(np.uint64) == np.float64(got[key]).view(np.uint64), key


@pytest.mark.parametrize("name", list(CASES))
def test_report_matches_the_oracle(crl, name):   # noqa: F811
    c = _case(crl, name)
    ref, tol = c["ref_noisy"]["ref"], c["ref_noisy"]["tol"]
    print(f"{name}: reference clipfrac {ref['clipfrac']:.4f}, undecided {tol['undecided']} of {c['B']}")
    assert 0.05 <= ref["clipfrac"] <= 0.5 and tol["undecided"] <= 0.01 * c["B"], "SIGMA puts the case where the clip decision is tested"
    _check_against(name, c["noisy"], c["ref_noisy"], c["B"])


@pytest.mark.parametrize("name", list(CASES))
def test_unperturbed_parameters_show_no_drift(crl, name):   # noqa: F811
    c = _case(crl, name)
    got = c["clean"]
    print(f"{name}: clipfrac {got['clipfrac']}, old_approx_kl {got['old_approx_kl']:.3e}, approx_kl {got['approx_kl']:.3e}")
    assert got["clipfrac"] == 0.0 and got["n_clipped"] == 0
    assert abs(got["old_approx_kl"]) <= c["ref_clean"]["tol"]["old_approx_kl"]
    assert 0.0 <= got["approx_kl"] <= 1e-9


@pytest.mark.parametrize("name", ["cartpole-65", "cartpole-8192-tiles", "synthetic-33-16-128", "synthetic-64-16-256"])
def test_two_calls_and_null_outputs_give_the_same_bits(crl, name):   # noqa: F811
    c = _case(crl, name); h = c["agent"].handle
    with limit(60):
        a = h.diagnose(per_sample=True); b = h.diagnose(per_sample=True); n = h.diagnose()
    assert _bits(a) == _bits(b) == _bits(n) == _bits(c["noisy"])
    assert np.array_equal(a["new_logprob"].view(np.uint32), b["new_logprob"].view(np.uint32))
    assert np.array_equal(a["new_value"].view(np.uint32), b["new_value"].view(np.uint32))
    assert set(n) == set(a) - {"new_logprob", "new_value"}
    assert 0 < h.get_option("diag_last_ns") < 10 ** 9, "the read-only option reports the launch's event time"


@pytest.mark.parametrize("name,options", [("cartpole-65", [("gemm", 1)]), ("synthetic-8-4-256", [("wide_gemm", 0), ("wide_gemm", 1)])])
def test_no_route_of_the_handle_changes_the_report(crl, name, options):   # noqa: F811
    c = _case(crl, name); h = c["agent"].handle
    for key, value in options:
        old = h.get_option(key)
        with limit(60):
            h.set_option(key, value)
            got = h.diagnose()
            h.set_option(key, old)
        assert _bits(got) == _bits({k: v for k, v in c["noisy"].items() if not isinstance(v, np.ndarray)}), (key, value)


@pytest.mark.parametrize("name", ["cartpole-65", "acrobot-128"])
def test_diagnose_leaves_the_handle_as_it_was(crl, name):   # noqa: F811
    """twin handles, one of which diagnoses twice (with and without per-sample outputs): every readable field, the iteration counter and the records of
    the next crl_ppo_iterate are the same bits"""
    F = crl._lib
    env, kind, D, A, H, nt, k, _ = CASES[name]
    fields = [f for f in dir(F) if f.startswith("F_") and isinstance(getattr(F, f), int)]
    snaps = []
    for diagnose in (False, True):
        cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 10, num_minibatches=1 if nt * k < 128 else 4)
        agent = crl.Agent(cfg, params=F.make_actor_critic_host(D, A, H, 3), obs_dim=D, n_act=A, hidden=H, env_kind=kind, seed=SEED)
        h = agent.handle
        with limit(120):
            h.env_reset(); h.rollout_run(); h.compute_gae()
            if diagnose:
                h.diagnose(per_sample=True); h.diagnose()
            snap = {f: h.read(getattr(F, f)).copy() for f in fields} | {"iteration": h.iteration, "episodes": h.episode_stats()}
            snap["records"] = json.dumps(h.iterate(1))
            snap["params_after"] = h.read(F.F_PARAMS).copy(); snap["iteration_after"] = h.iteration
        snaps.append(snap)
        agent.close()
    a, b = snaps
    assert a["iteration"] == 0 and a["iteration_after"] == 1
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key].view(np.uint8), b[key].view(np.uint8)), key
        else:
            assert a[key] == b[key], key


def test_errors(crl):   # noqa: F811
    F = crl._lib
    cfg = crl.PPOConfig(num_envs=8, num_steps=16, total_timesteps=8 * 16 * 10)
    donor = crl.Agent(cfg, seed=SEED)
    h = F.Handle(donor.crl_cfg, 0)                                     # a fresh handle: parameters never set
    donor.close()
    with pytest.raises(F.CrlError, match="parameters not set"):
        h.diagnose()
    import ctypes as C
    h.init_params(0)
    assert F.load().crl_ppo_diagnose(h._h, None, None, None) != 0 and b"null out" in F.load().crl_last_error()
    d = F.CrlDiag()
    assert F.load().crl_ppo_diagnose(None, C.byref(d), None, None) != 0 and b"null crl_ppo handle" in F.load().crl_last_error()
    with limit(60):
        assert h.diagnose()["n"] == 8 * 16                             # and the handle is still usable
    h.close()


def test_ppo_diag_every_emits_policy_diagnostics(crl, tmp_path):   # noqa: F811
    nt, k, updates = 8, 32, 4
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * updates)
    streams = []
    for every in (0, 2):
        run = f"diag-every-{every}"
        with limit(300):
            crl.ppo(cfg, diag_every=every, run_name=run, logger_kw=dict(to_tensorboard=False, to_json=True, log_dir=str(tmp_path)))
        logging.getLogger("CleanRL").handlers.clear()
        recs = [json.loads(line) for line in open(tmp_path / f"{run}.json")]
        for r in recs:
            r.pop("steps_per_sec", None)                             # wall-clock
        streams.append([(r.pop("msg"), r) for r in recs])
    base, withd = streams
    assert not [m for m, _ in base if m == "Policy Diagnostics"]
    ds = [kv for m, kv in withd if m == "Policy Diagnostics"]
    assert [kv["global_step"] for kv in ds] == [2 * nt * k, 4 * nt * k]
    for kv in ds:
        assert set(kv) == {"approx_kl", "old_approx_kl", "clipfrac", "entropy", "explained_variance", "global_step"}
        assert all(math.isfinite(kv[key]) for key in kv)
        assert kv["approx_kl"] >= 0 and 0 <= kv["clipfrac"] <= 1 and 0 < kv["entropy"] <= math.log(2) + 1e-6
    assert [r for r in withd if r[0] != "Policy Diagnostics"] == base, "the other records are those of diag_every = 0"
    pos = [i for i, (m, _) in enumerate(withd) if m == "Policy Diagnostics"]
    per_update = cfg.update_epochs * cfg.num_minibatches
    assert [sum(1 for m, _ in withd[:p] if m == "Training Statistics") for p in pos] == [2 * per_update, 4 * per_update]
