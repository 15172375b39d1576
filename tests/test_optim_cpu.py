"""The inputs of test_gpu_optim.py, shown good without a GPU: every route's schedule and every state edge is replayed through the oracle
alone (orc_loss_grad standing in for the update kernels, orc_clipnorm_adam stepping) and must meet the conditions the GPU test asserts
again on the gradients it reads back — the three crossing conditions, no norm inside [0.45, 0.55], no clipped norm within
(array length)·2⁻⁵² of a Float32 rounding midpoint."""
import numpy as np
import pytest

import optimlib as L
import oraclelib as O


def replay(route, steps, params, m, v, betap, where, zero_obs=None):
    flags, grads = [], []
    for s, spec in enumerate(steps):
        buf = L.step_buffer(route, s, spec, params, zero_obs)
        g = L.oracle_grad(route, params, buf, s % route.nmb)
        assert np.all(np.isfinite(g))
        flags.append(L.check_step_inputs(route, g, s, where))
        grads.append(g.copy())
        O.clipnorm_adam(route.ocfg(), params, g, m, v, betap, spec[2])
        assert np.all(np.isfinite(params)) and np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    return flags, grads


@pytest.mark.parametrize("name", list(L.ROUTES))
def test_schedule_crosses_the_clip_threshold_both_ways_on_every_array(name):
    route = L.ROUTES[name]
    assert len(L.SCHEDULE) >= 8 and any(eta == 0.0 for _, _, eta in L.SCHEDULE)
    p = L.base_params(route)
    assert p.size == route.P == O.lib().orc_param_count(route.ocfg())
    flags, _ = replay(route, L.SCHEDULE, p, np.zeros_like(p), np.zeros_like(p), np.array([0.9, 0.999] * 12), name)
    L.check_schedule(flags, name)


def test_route_shapes_are_the_ones_the_kernels_switch_on():
    R = L.ROUTES
    assert R["block"].P == 9155 and R["block,layerwise"].P <= 32768
    assert R["slices,128"].P == 34691 > 32768 and R["slices,256,wide_gemm=2"].P == 142342
    off = O.param_offsets(R["slices,128"].ocfg())
    sizes = np.diff(off)
    assert sizes[2] == 4 * 4096 and all(s < 4096 for i, s in enumerate(sizes) if i not in (2, 8))   # W2: four full slices, the rest ragged
    sizes = np.diff(O.param_offsets(R["slices,256,wide_gemm=2"].ocfg()))
    assert sizes[0] == 4352 == 4096 + 256 and sizes[2] == 16 * 4096 and sizes[5] == 5 and sizes[11] == 1
    off = O.param_offsets(R["block"].ocfg())
    assert off[6] == 4610 and off[6] % 64 != 0       # the critic starts mid-chunk: a 64-float chunk of the one-launch step feeds up to three arrays


@pytest.mark.parametrize("edge", L.EDGES)
@pytest.mark.parametrize("name", L.EDGE_ROUTES)
def test_state_edges_meet_their_preconditions(name, edge):
    route = L.ROUTES[name]
    p, m, v, betap, info = L.edge_state(route, edge)
    v0 = v.copy()
    flags, grads = replay(route, L.EDGE_STEPS, p, m, v, betap, f"{name}/{edge}", info.get("zero_obs"))
    if edge == "eps":
        idx, sub = info["idx"], info["subnormal"]
        assert idx.size > 0 and sub.size > 0 and np.any(v0[idx] == 0)
        for g in grads:
            assert not g[idx].any(), "a dead input's entries must see a gradient of exactly zero"
        assert np.all(v[sub] != 0) and np.all(np.abs(v[sub]) < L.F32_MIN_NORMAL), "their v stays a Float32 subnormal through the steps"
    if edge == "dead":
        off = O.param_offsets(route.ocfg())
        for g, fl in zip(grads, flags):
            zero = [a for a in range(12) if not g[off[a]:off[a + 1]].any()]
            assert zero == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10], zero
            assert not any(fl[a] for a in zero)
        for a in (0, 1, 2, 3, 4, 6, 7, 8, 9, 10):
            sl = slice(off[a], off[a + 1])
            assert not p[sl].any() and not m[sl].any() and not v[sl].any()
        assert p[off[5]:off[6]].any() and p[off[11]:off[12]].any()
