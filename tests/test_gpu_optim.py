"""Optimiser(ClipNorm(0.5), Adam(η)) (ppo.jl:93,250) on every route of the library, bit for bit against orc_clipnorm_adam.

Four kernels implement the step: clipnorm_adam_kernel (one block per array; with a thirteenth statistics block under a communicator),
clipnorm_partial_kernel + adam_slice_kernel (slices of 4096, P > 32768) and reduce_optim_kernel (the one-launch step). Each case drives
one of them through crl_ppo_update_minibatch for a schedule of steps in which every array's gradient norm crosses the clip threshold in
both directions (optimlib.py; shown good on the CPU by test_optim_cpu.py), reads CRL_F_GRADS — the message the optimiser consumed — after
each step, feeds exactly those bits to the oracle on a host copy of the state, and requires parameters, m, v and the β powers to be equal
as bits. Whole-iteration bars cannot do this: Adam's step m̂ / (√v̂ + ε) is invariant under a rescaling of the gradient, so a wrong clip
scale shows only through how m and v mix differently scaled gradients — far inside 1e-6.

Why bit equality is fair for clipped arrays: the routes add Σg² in different orders, which moves the Float64 sum by at most n·2⁻⁵² relative;
the Float32 norm differs only if √Σg² lies that close to a rounding midpoint. check_step_inputs asserts, as a precondition on the input,
that it does not.

The β powers are compared with exact equality: kernels and oracle multiply the same doubles in the same order."""
import numpy as np
import pytest

import optimlib as L
import oraclelib as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1, "HIP library loaded but no GPU visible"
    return crl


def make_agent(crl, route, params):
    F = crl._lib
    cfg = crl.PPOConfig(num_envs=route.nt, num_steps=route.k, num_minibatches=route.nmb, total_timesteps=route.nt * route.k * 10,
                        clip_value_loss=route.clipv, ent_coeff=route.ent_coeff, clip_coef=route.clip_coef)
    agent = crl.Agent(cfg, params=params, shuffle_mode=0, obs_dim=route.D, n_act=route.A, hidden=route.H,
                      env_kind=F.ENV_SYNTHETIC if route.wide else F.ENV_CARTPOLE, options=route.options)
    h = agent.handle
    assert h.P == route.P
    if route.comm:
        h.comm_init(crl.comm_unique_id(), 1, 0)
    h.prof_enable(True)
    return agent


def write_buffer(crl, h, buf):
    F = crl._lib
    for f, key in ((F.F_OBS, "obs"), (F.F_ACTION, "action"), (F.F_LOGPROB, "logprob"), (F.F_VALUE, "value"), (F.F_ADVANTAGE, "advantage"),
                   (F.F_RETURN, "ret"), (F.F_PERM, "perm")):
        h.write(f, buf[key])
    h.adv_stats()


def assert_route(crl, route, h, n_steps):
    """Each case ran the kernel it names. launch_optim counts under CRL_K_OPTIM, the one-launch step (inside the reduce scope) does not.
    The counters cannot tell one block per array from slices, nor 12 blocks from 13: there the deciding quantities of launch_optim / update_step
    are asserted instead — P against 32768; a communicator (one gradient all-reduce per step), no inline value-loss fix-up and no one-launch step."""
    prof = h.prof_read()
    if route.fused:
        assert h.get_option("fuse_optim") == 1 and not route.clipv
        assert prof["optim"][1] == 0 and prof["reduce"][1] == n_steps, prof
        return
    assert prof["optim"][1] == n_steps, prof
    if route.name.startswith("slices"):
        assert h.P > 32768 and route.wide
    else:
        assert h.P <= 32768
        assert route.wide == ((route.D, route.A, route.H) != (4, 2, 64))
    if route.comm:
        assert prof["allreduce"][1] == n_steps and h.get_option("fuse_optim") == 0 and h.get_option("comm_force") == 1 and not route.clipv, prof
    else:
        assert prof["allreduce"][1] == 0, prof


def compare_state(crl, route, h, want, flags, where):
    F = crl._lib
    p, m, v, betap = want
    for name, f, ref in (("params", F.F_PARAMS, p), ("adam_m", F.F_ADAM_M, m), ("adam_v", F.F_ADAM_V, v)):
        got = h.read(f)
        msg = L.first_mismatch(route, name, got, ref, flags)
        assert msg is None, f"{where}: {msg}"
    bp = h.read(F.F_BETAP)
    assert np.array_equal(bp, betap), f"{where}: β powers differ: array {int(np.flatnonzero(bp != betap)[0]) // 2}: got {bp}, oracle {betap}"


def run_case(crl, route, steps, state, where):
    """The method of the module docstring; returns (clip flags per step, the gradients read, final host state)."""
    F = crl._lib
    p, m, v, betap, info = state
    cfgo = route.ocfg()
    agent = make_agent(crl, route, p)
    h = agent.handle
    h.write(F.F_ADAM_M, m); h.write(F.F_ADAM_V, v); h.write(F.F_BETAP, betap)
    flags, grads = [], []
    for s, (critic, actor, eta) in enumerate(steps):
        write_buffer(crl, h, L.step_buffer(route, s, (critic, actor, eta), p, info.get("zero_obs")))
        h.update_minibatch(s % route.nmb, eta, apply_update=True)
        g = h.read(F.F_GRADS).copy()
        assert np.all(np.isfinite(g)), f"{where} step {s}: non-finite gradient"
        fl = L.check_step_inputs(route, g, s, where)
        flags.append(fl); grads.append(g)
        O.clipnorm_adam(cfgo, p, g.copy(), m, v, betap, eta)
        compare_state(crl, route, h, (p, m, v, betap), fl, f"{where} step {s} ({critic} critic, {actor} actor, eta {eta})")
    assert_route(crl, route, h, len(steps))
    agent.close()
    return flags, grads, (p, m, v, betap)


FRESH = lambda route: (L.base_params(route), np.zeros(route.P, np.float32), np.zeros(route.P, np.float32), np.array([0.9, 0.999] * 12), {})
SEQUENCE_ROUTES = [n for n in L.ROUTES if n != "two-launch"]


@pytest.mark.parametrize("name", SEQUENCE_ROUTES)
def test_optimiser_route_matches_oracle_bit_for_bit(crl, name):
    """The routes of DESIGN.md's paragraph "Optimiser: four routes, one arithmetic": eight steps whose critic and actor gradients are switched between ≫ 0.5 and ≪ 0.5,
    η varying and once 0. The crossing conditions are asserted on the gradients the GPU produced."""
    route = L.ROUTES[name]
    flags, _, _ = run_case(crl, route, L.SCHEDULE, FRESH(route), name)
    L.check_schedule(flags, name)


@pytest.mark.parametrize("edge", L.EDGES)
@pytest.mark.parametrize("name", L.EDGE_ROUTES)
def test_optimiser_state_edges_match_oracle_bit_for_bit(crl, name, edge):
    """late: β powers (0.9ⁿ, 0.999ⁿ), n = 20000 — the first is 0 in Float64; early: the 1 − 0.999 division; eps: a dead input's entries hold Float32
    subnormal (and zero) v with |m| 1e-12 … 1e-6 and must stay subnormal — no flush when v is widened or stored; dead: all-zero parameters — ten
    arrays have a norm of exactly 0, do not clip and stay at m = v = 0, the two head biases step as the oracle says, everything finite (on the
    hidden-256 route max|w| = 0 also passes through the layer-wise path's weight-scale kernels)."""
    route = L.ROUTES[name]
    state = L.edge_state(route, edge)
    info = state[4]
    where = f"{name}/{edge}"
    flags, grads, (p, m, v, betap) = run_case(crl, route, L.EDGE_STEPS, state, where)
    assert all(np.all(np.isfinite(x)) for x in (p, m, v, betap))   # the host copy is bit-equal to the device's
    if edge == "eps":
        idx, sub = info["idx"], info["subnormal"]
        for s, g in enumerate(grads):
            assert not g[idx].any(), f"{where} input precondition: step {s}: a dead input's entries must see a gradient of exactly zero"
        assert np.all(v[sub] != 0) and np.all(np.abs(v[sub]) < L.F32_MIN_NORMAL), f"{where}: stored v left the subnormal range"
    if edge == "dead":
        off = O.param_offsets(route.ocfg())
        for s, (g, fl) in enumerate(zip(grads, flags)):
            zero = [a for a in range(12) if not g[off[a]:off[a + 1]].any()]
            assert zero == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10], f"{where} step {s}: arrays with an all-zero gradient: {zero}"
            assert not any(fl[a] for a in zero)
        for a in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10):
            sl = slice(off[a], off[a + 1])
            assert not p[sl].any() and not m[sl].any() and not v[sl].any(), f"{where}: array {a} moved"
        assert p[off[5]:off[6]].any() and p[off[11]:off[12]].any()


def test_one_launch_and_two_launch_steps_agree_bit_for_bit(crl):
    """reduce_optim_kernel against reduce_kernel + clipnorm_adam_kernel on the 4/2/64 shape: same parameters, buffer and schedule, clip_value_loss = 0,
    fuse_optim 1 and 0. After every step the gradient message, m, v, the parameters and the β powers are the same bits — the sharp version of
    test_fused_and_two_launch_optimiser_steps_agree_at_c2_size; it follows from the midpoint precondition, asserted per step."""
    F = crl._lib
    r1, r0 = L.ROUTES["fused,gemm=2"], L.ROUTES["two-launch"]
    assert (r1.D, r1.A, r1.H, r1.clipv, r1.seed) == (r0.D, r0.A, r0.H, r0.clipv, r0.seed)
    p = L.base_params(r1)
    a1, a0 = make_agent(crl, r1, p), make_agent(crl, r0, p)
    flags = []
    for s, spec in enumerate(L.SCHEDULE):
        buf = L.step_buffer(r1, s, spec, a1.handle.read(F.F_PARAMS))
        for a in (a1, a0):
            write_buffer(crl, a.handle, buf)
            a.handle.update_minibatch(s % r1.nmb, spec[2], apply_update=True)
        g = a1.handle.read(F.F_GRADS)
        fl = L.check_step_inputs(r1, g, s, "cross-route")
        flags.append(fl)
        for name, f in (("grads", F.F_GRADS), ("adam_m", F.F_ADAM_M), ("adam_v", F.F_ADAM_V), ("params", F.F_PARAMS)):
            msg = L.first_mismatch(r1, name, a1.handle.read(f), a0.handle.read(f), fl)
            assert msg is None, f"step {s}: one-launch (got) against two-launch (as 'oracle'): {msg}"
        assert np.array_equal(a1.handle.read(F.F_BETAP), a0.handle.read(F.F_BETAP)), f"step {s}: β powers differ"
    L.check_schedule(flags, "cross-route")
    assert_route(crl, r1, a1.handle, len(L.SCHEDULE)); assert_route(crl, r0, a0.handle, len(L.SCHEDULE))
    a1.close(); a0.close()
