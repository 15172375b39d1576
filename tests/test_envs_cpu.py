"""CPU side of the on-device MountainCar / Acrobot envs: known answers for the numpy restatement the GPU tests compare against
(tests/envs_ref.py), the share of the single-step grid on which Float32 and Float64 may disagree about `done`, and the host-side
wiring (constants, export, binding, ppo(env=...))."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import envs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ known answers
def test_mountaincar_known_step_from_minus_half():
    """By hand: v = 0 + (2 - 1)*0.001 + cos(-1.5)*(-0.0025) = 0.001 - 0.0025*0.0707372017 = 0.000823156996; x = -0.5 + v."""
    s, t, r, d, _ = R.mountaincar_step(np.array([[-0.5], [0.0]]), np.array([0]), np.array([2]))
    v = 0.001 - 0.0025 * 0.0707372016677029
    assert abs(s[1, 0] - v) < 1e-15 and abs(s[0, 0] - (-0.5 + v)) < 1e-15
    assert t[0] == 1 and r[0] == -1.0 and not d[0]


def test_mountaincar_left_wall_zeroes_v_and_goal_and_time_limit():
    s, _, _, d, _ = R.mountaincar_step(np.array([[-1.19], [-0.07]]), np.array([0]), np.array([0]))
    assert s[0, 0] == -1.2 and s[1, 0] == 0.0 and not d[0]
    s, _, r, d, _ = R.mountaincar_step(np.array([[0.49], [0.07]]), np.array([0]), np.array([2]))
    assert s[0, 0] >= 0.5 and d[0] and r[0] == 0.0
    s, t, r, d, _ = R.mountaincar_step(np.array([[-0.5], [0.0]]), np.array([R.MAX_STEPS - 1]), np.array([1]))
    assert t[0] == R.MAX_STEPS and d[0] and r[0] == 0.0
    s, t, r, d, _ = R.mountaincar_step(np.array([[-0.5], [0.0]]), np.array([R.MAX_STEPS - 2]), np.array([1]))
    assert not d[0] and r[0] == -1.0
    s, _, _, _, _ = R.mountaincar_step(np.array([[0.0], [0.069]]), np.array([0]), np.array([2]))
    assert s[1, 0] <= 0.07                                          # velocity clamp (cos(0)*(-0.0025) pulls down first, then +0.001)


def test_acrobot_at_rest_stays_at_rest():
    s, t, r, d, m = R.acrobot_step(np.zeros((4, 1)), np.array([0]), np.array([1]))
    assert np.abs(s).max() < 1e-14 and t[0] == 1 and r[0] == -1.0 and not d[0]
    assert abs(m[0] - (-3.0)) < 1e-12                               # hanging down: -cos 0 - cos 0 - 1


def test_acrobot_energy_drift_within_rk4_bound():
    """tau = 0 conserves energy; one classical RK4 step of size h has local error O(h^5). With |f^(5)| of order g^2.5 (pendulum frequency
    sqrt(g) ~ 3.1, h*omega ~ 0.63) the relative drift of a swing of amplitude <= 1 rad is below (h*omega)^5 / 120 ~ 8e-4 of the ~30 J energy
    scale; bar: 0.05 J. Halving the step (two steps of h/2 through the same function is not available — dt is fixed — so the bound is the check)."""
    rng = np.random.default_rng(1)
    s0 = np.stack([rng.uniform(-1, 1, 256), rng.uniform(-1, 1, 256), rng.uniform(-1, 1, 256), rng.uniform(-1, 1, 256)])
    s1, _, _, _, _ = R.acrobot_step(s0, np.zeros(256, int), np.ones(256, int))
    drift = np.abs(R.acrobot_energy(s1) - R.acrobot_energy(s0))
    assert drift.max() < 0.05, drift.max()
    # and torque does work: energy moves with tau != 0 from a moving state
    s2, _, _, _, _ = R.acrobot_step(s0, np.zeros(256, int), np.full(256, 2))
    assert np.abs(R.acrobot_energy(s2) - R.acrobot_energy(s0)).max() > 0.05


def test_acrobot_wrap_and_clamp_edges():
    assert R.wrap_pi(np.array([np.pi]))[0] == -np.pi and R.wrap_pi(np.array([-np.pi]))[0] == -np.pi
    w = R.wrap_pi(np.array([3 * np.pi + 0.25, -3 * np.pi - 0.25, 0.5]))
    assert np.allclose(w, [-np.pi + 0.25, np.pi - 0.25, 0.5], atol=1e-12) and np.all((w >= -np.pi) & (w < np.pi))
    s, _, _, _, _ = R.acrobot_step(np.array([[0.3], [0.2], [R.AC_MAX_W1], [R.AC_MAX_W2]]), np.array([0]), np.array([2]))
    assert abs(s[2, 0]) <= R.AC_MAX_W1 and abs(s[3, 0]) <= R.AC_MAX_W2 and np.all((s[:2] >= -np.pi) & (s[:2] < np.pi))
    s, _, r, d, m = R.acrobot_step(np.array([[np.pi - 0.01], [0.0], [0.0], [0.0]]), np.array([5]), np.array([1]))
    assert d[0] and r[0] == 0.0 and m[0] > 0                        # both links up: the goal
    o = R.acrobot_obs(np.array([[0.5], [-0.25], [1.0], [-2.0]]))
    assert np.allclose(o[:, 0], [np.cos(0.5), np.sin(0.5), np.cos(-0.25), np.sin(-0.25), 1.0, -2.0])


def test_reset_maps_are_exact_in_float32():
    """0.2 * u with a 24-bit u rounds once (0.2f is not a power of two); the subtraction of the constant is then exact or rounds once more: the GPU
    and this map perform the same two Float32 operations, so the reset test compares bits."""
    u = R.uniforms24(np.array([[0, 1 << 8, 0xFFFFFFFF, 0x80000000]], np.uint32))[:, 0]
    assert u.dtype == np.float32 and u[0] == 0 and u[2] == np.float32(1 - 2.0 ** -24)
    a = R.acrobot_reset(np.stack([u] * 1, 1))
    assert a.dtype == np.float32 and a.min() >= -0.1 and a.max() < 0.1
    m = R.mountaincar_reset(np.stack([u] * 1, 1))
    assert -0.6 <= m[0, 0] < -0.4 and m[1, 0] == 0


# ------------------------------------------------------------------------------------------------ the grid of the GPU single-step test
@pytest.mark.parametrize("name", ["mountaincar", "acrobot"])
def test_single_step_grid_float32_float64_agree_on_done(name):
    """The GPU test requires done / reward / t exactly equal to the Float64 restatement except where the Float64 goal margin is within the float
    tolerance of the threshold, and that exception may cover at most 0.1 % of the cases. Here: the restatement alone, Float32 against Float64, on
    the same grid x every action, stays inside that share — and covers both outcomes and the time limit."""
    e = R.ENVS[name]
    s, t = R.state_grid(name)
    assert s.shape[1] >= 4096
    tot = bad = 0
    for a in range(e["n_act"]):
        act = np.full(s.shape[1], a)
        s64, t64, r64, d64, m64 = e["step"](s.astype(np.float64), t, act, np.float64)
        s32, t32, r32, d32, m32 = e["step"](s, t, act, np.float32)
        bad += int(np.sum(d64 != d32)); tot += d64.size
        assert np.array_equal(t64, t32)
        goal = d64 & (t64 < R.MAX_STEPS)
        assert goal.sum() >= 16 and (~d64).sum() >= 1024 and (t64 >= R.MAX_STEPS).sum() >= 128
    assert bad <= 1e-3 * tot, (bad, tot)


# ------------------------------------------------------------------------------------------------ host wiring
def test_env_constants_match_the_header():
    from cleanrl_jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cleanrl_hip.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(CRL_ENV_\w+)\s+(\d+)", hdr)}
    assert defs["CRL_ENV_MOUNTAINCAR"] == 3 == L.ENV_MOUNTAINCAR and defs["CRL_ENV_ACROBOT"] == 4 == L.ENV_ACROBOT
    assert (defs["CRL_ENV_CARTPOLE"], defs["CRL_ENV_SYNTHETIC"], defs["CRL_ENV_EXTERNAL"]) == (0, 1, 2) == (L.ENV_CARTPOLE, L.ENV_SYNTHETIC, L.ENV_EXTERNAL)
    assert R.ENVS["mountaincar"]["kind"] == L.ENV_MOUNTAINCAR and R.ENVS["acrobot"]["kind"] == L.ENV_ACROBOT


def test_crl_env_step_is_declared_exported_and_bound():
    from cleanrl_jl_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "cleanrl_hip.h")).read()
    assert re.search(r"int32_t\s+crl_env_step\(crl_ppo\*\s*h,\s*const int32_t\*\s*action,\s*uint64_t\s+gstep,\s*float\*\s*next_obs,\s*float\*\s*reward,\s*uint8_t\*\s*done\);", hdr)
    assert "crl_env_step" in L.EXPORTS
    lib = L.load()                                                   # dlopen only: no GPU needed
    assert lib.crl_env_step.argtypes == [C.c_void_p, C.POINTER(C.c_int32), C.c_uint64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
    assert callable(getattr(L.Handle, "env_step"))
    jl = open(os.path.join(ROOT, "julia", "CleanRLHip.jl")).read()
    assert ":crl_env_step" in jl and "env" in jl


def test_ppo_env_keyword_resolves_shapes():
    from cleanrl_jl_amd import _lib as L
    import importlib
    P = importlib.import_module("cleanrl_jl_amd.ppo")
    assert P.env_shape("acrobot") == dict(env_kind=L.ENV_ACROBOT, obs_dim=6, n_act=3)
    assert P.env_shape("mountaincar", hidden=256) == dict(hidden=256, env_kind=L.ENV_MOUNTAINCAR, obs_dim=2, n_act=3)
    assert P.env_shape("cartpole") == dict(env_kind=L.ENV_CARTPOLE, obs_dim=4, n_act=2)
    assert P.env_shape(None, env_kind=L.ENV_SYNTHETIC, obs_dim=8, n_act=4) == dict(env_kind=L.ENV_SYNTHETIC, obs_dim=8, n_act=4)   # explicit env_kind keeps working
    with pytest.raises(ValueError):
        P.env_shape("lunarlander")
    with pytest.raises(ValueError):
        P.env_shape("acrobot", obs_dim=4)
    with pytest.raises(ValueError):
        P.ppo(P.PPOConfig(), env="pendulum")                        # rejected before any device is touched
