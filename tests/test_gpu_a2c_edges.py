"""The A2C update kernels (csrc/a2c.hip: a2c_forward_kernel, a2c_loss_kernel, a2c_backward_kernel, a2c_wgrad_kernel) at the batch and ring edges,
against the C oracle on the same trajectories: fewer samples than a wave, exactly 64 and 65, the full ring (n = cap, ptr wrapped), exactly the loss
kernel's block of 1024, its stride loop's second pass, ragged sizes above it, gamma 0 and 1, a policy near 50/50 — and 4101 episodes in one call, five
more than the record buffer holds. The cases are tests/a2c_bar.py's table, the bars profiles/a2c_bar.json's: on the CPU (tests/test_a2c_bar_cpu.py)
every case was shown to tell six one-line mutants of tests/a2c_ref.py from it by at least ten bars. The raw gradients (crl_a2c_read_grads) are compared
directly: Adam's first step is blind to a gradient's scale, so the parameters alone cannot see a cotangent that is off by a factor."""
import numpy as np
import pytest

import a2c_bar as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _handle(crl, case):
    L = crl._lib
    h = L.A2CHandle(L.CrlA2CConfig(case["lr"], case["total_timesteps"], case["min_replay_size"], case["max_steps"], case["gamma"], case["seed"]), 0)
    h.write_params(B.case_params(case))
    return h


@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_update_edges_match_the_oracle(crl, name):
    case = B.CASE[name]
    calls, updates = B.oracle_run(name)
    assert B.n_matches(case, updates)
    h = _handle(crl, case)
    with pytest.raises(crl.CrlError, match="no update yet"):
        h.read_grads()
    got, u, total = [], 0, 0
    for taken, ts, eps, gstep in calls:
        tg, ts_g, eps_g = h.run_until_update(max_eps=2 * B.A2C_MAX_EPS)
        total += tg
        assert tg == taken and ts_g["trained"] == ts["trained"] and ts_g["n"] == ts["n"], "same trajectories, same batch"
        assert eps_g == eps[:B.A2C_MAX_EPS], "same episode records, the first 4096 of a call"
        s, g, size = h.env()
        assert g == gstep == total
        if not ts["trained"]:                                               # the call that ran into total_timesteps
            continue
        assert size == 0, "Buffer.clear! after the update (a2c.jl:102)"
        assert np.array_equal(s, updates[u]["reset_state"]), "the env was reset after the update"
        got.append(dict(critic_loss=ts_g["critic_loss"], actor_loss=ts_g["actor_loss"], grads=h.read_grads(), params=h.read_params()))
        for k in B.LOSSES:                                                  # tests/test_gpu_a2c.py's bars
            assert abs(ts_g[k] - ts[k]) <= B.OLD_LOSS_BAR * max(1.0, abs(ts[k])), (k, ts_g[k], ts[k])
        assert np.max(np.abs(got[-1]["params"] - updates[u]["params"])) < B.OLD_PARAM_BAR
        u += 1
    assert u == len(updates) and h.run_until_update()[0] == 0
    if name == "n8202_eps4101":
        assert [len(c[2]) for c in calls] == [4101, 4101], "each call saw 4101 episodes: the second call's records started clean"
    out = B.distances(got, updates)
    print(name, out, "per update:", [B.distances([g], [r]) for g, r in zip(got, updates)])
    B.record_device(name, dict(out, n=[r["n"] for r in updates]))
    loss_bar, param_bar = B.load_bars()
    for k in B.OBSERVABLES:
        assert out[k] <= B.bar_of(k, loss_bar, param_bar), (k, out[k])
    h.close()


def test_read_grads_changes_nothing(crl):
    """two handles on one case, one of them read after every call: parameters, env and the next update's results are the same bits"""
    case = B.CASE["n65"]
    a, b = _handle(crl, case), _handle(crl, case)
    trained = 0
    while True:
        ra, rb = a.run_until_update(), b.run_until_update()
        assert ra == rb
        if ra[0] == 0:
            break
        if ra[1]["trained"]:
            trained += 1
            g1, g2 = a.read_grads(), a.read_grads()
            assert np.array_equal(g1, g2) and np.any(g1 != 0)
        sa, sb = a.env(), b.env()
        assert np.array_equal(sa[0], sb[0]) and sa[1:] == sb[1:]
        assert np.array_equal(a.read_params(), b.read_params())
    assert trained == 3
    assert np.array_equal(a.read_grads(), b.read_grads())
    with pytest.raises(crl.CrlError, match="crl_a2c_read_grads"):
        crl._lib.check(a._L.crl_a2c_read_grads(a._h, None, a.param_count))
    g = np.zeros(a.param_count - 1, np.float32)
    with pytest.raises(crl.CrlError, match="expected 9155 floats"):
        crl._lib.check(a._L.crl_a2c_read_grads(a._h, g.ctypes.data_as(crl._lib.C.POINTER(crl._lib.C.c_float)), g.size))
    a.close(); b.close()
