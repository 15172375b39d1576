"""The yardstick of the categorical-DQN parity tests, without a GPU. C51 has no Julia reference, so tests/c51_ref.py's hand-written gradient is
proved first, by central finite differences of its own loss in Float64. Then the projection (an independent scatter form, mass, mean), the mutants and
the recorded bars of tests/c51_bar.py, and the Python layer.

The agreement bound of the gradient check is tests/test_sac_cpu.py's, for the same step h = 1e-5, and its reasoning carries over: a loss here is a
mean of k cross-entropies of size <= log(N) + a few < 10, each behind dot products of at most 84·120 + 84·2N < 21,000 terms, so the worst-case
rounding 21,000 · 1.1e-16 · 10 / h = 2.3e-6 stays the order of TOL while the random-walk figure is sqrt(21,000) · 1.1e-16 · 10 / h = 1.6e-8; the
softmax's third derivative along a logit is below 1, so the truncation h²/6 is 2e-11. EXPECTED below is test_sac_cpu.EXPECTED."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import c51_bar as B
import c51_ref as Z
import test_sac_cpu as SC

H = 1e-5


# ---------------------------------------------------------------------------------------------------- the gradient
def _loss64(qp64, N, state, a, m, w):
    """c51_ref's loss with Float64 parameters (split without the Float32 projection: the perturbation has to survive)"""
    def split64(p, N_):
        out, o = [], 0
        for n, shape in zip(Z.sizes(N_), ((120, 4), (120,), (84, 120), (84,), (2 * N_, 84), (2 * N_,))):
            out.append(np.asarray(p[o:o + n], np.float64).reshape(shape, order="F")); o += n
        return out
    with B.patched(split=split64):
        return Z.loss_grads(qp64, N, state, a, m, w)


def _setup(N, k, seed):
    rng = np.random.default_rng(seed)
    qp = np.asarray(B.case_params(dict(c51=dict(n_atoms=N))), np.float64)
    state = rng.uniform(-1, 1, (4, k))
    a = rng.integers(0, 2, k)
    m = rng.random((N, k)); m = m / m.sum(axis=0)
    w = rng.uniform(0.3, 1.0, k)
    return qp, state, a, m, w


@pytest.mark.parametrize("N,k,seed", [(5, 7, 1), (51, 4, 1)])
def test_the_hand_written_gradient_agrees_with_central_differences(N, k, seed):
    qp, state, a, m, w = _setup(N, k, seed)
    loss, grad, _ = _loss64(qp, N, state, a, m, w)
    h1, h2, _ = Z.forward(qp.astype(np.float32), N, state)
    rng = np.random.default_rng(9)
    off = np.cumsum([0] + Z.sizes(N))
    worst, checked = 0.0, 0
    for arr in range(6):
        for p in rng.choice(np.arange(off[arr], off[arr + 1]), 6, replace=False):
            up, dn = qp.copy(), qp.copy()
            up[p] += H; dn[p] -= H
            fd = (_loss64(up, N, state, a, m, w)[0] - _loss64(dn, N, state, a, m, w)[0]) / (2 * H)
            worst = max(worst, abs(fd - grad[p])); checked += 1
    print(f"N {N} k {k}: {checked} entries, worst |fd - grad| {worst:.3e} (expected <= {SC.EXPECTED}, proved <= {SC.TOL})")
    assert worst <= SC.EXPECTED
    assert np.abs(grad).max() > 1e-3 and loss > 0.0
    # the other action's head rows of a one-action batch get exactly 0.0
    a0 = np.zeros(k, np.int64)
    g0 = _loss64(qp, N, state, a0, m, w)[1]
    W3g = g0[off[4]:off[5]].reshape(2 * N, 84, order="F")
    assert np.all(W3g[N:] == 0.0) and np.all(g0[off[5] + N:] == 0.0) and np.any(W3g[:N] != 0.0)


def test_a_wrong_sign_is_far_outside_the_bound():
    N, k = 5, 7
    qp, state, a, m, w = _setup(N, k, 1)
    good = _loss64(qp, N, state, a, m, w)[1]
    with B.patched(**B.MUTANTS["M7"][1]()):
        bad = _loss64(qp, N, state, a, m, w)[1]
    assert np.abs(good - bad).max() > 1e-3 > 100 * SC.TOL


# ---------------------------------------------------------------------------------------------------- the projection
def _scatter(pp, R_, disc, term, c51):
    """the textbook form, written independently: every source atom adds to its one or two targets, sources ascending, one scalar at a time"""
    N, v_min, v_max = c51["n_atoms"], float(c51["v_min"]), float(c51["v_max"])
    delta = (v_max - v_min) / float(N - 1)
    m = np.zeros_like(pp)
    clamped = np.zeros_like(pp)
    for j in range(pp.shape[1]):
        for s in range(N):
            z = v_min + float(s) * delta
            Tz = float(R_[j]) + ((float(disc[j]) * z) * (1.0 - float(term[j])))
            Tz = v_min if Tz < v_min else (v_max if Tz > v_max else Tz)
            clamped[s, j] = Tz
            b = (Tz - v_min) / delta
            b = float(N - 1) if b > float(N - 1) else b
            lo, up = int(np.floor(b)), int(np.ceil(b))
            if lo == up:
                m[lo, j] = m[lo, j] + pp[s, j]
            else:
                m[lo, j] = m[lo, j] + pp[s, j] * (float(up) - b)
                m[up, j] = m[up, j] + pp[s, j] * (b - float(lo))
    return m, clamped


def hand_made_rows(N, k, v_min, v_max, seed=0):
    """rows for the projection: the first six are Tz exactly on an atom (R = 2Δ, disc = 1), both clamps, a terminal, disc = γ³ and disc = 0; the
    rest random. Shared with tests/test_gpu_c51.py."""
    rng = np.random.default_rng(seed)
    delta = (v_max - v_min) / (N - 1)
    pp = rng.random((N, k)) ** 3; pp = pp / pp.sum(axis=0)
    R_ = rng.uniform(0.0, 3.0, k); disc = np.full(k, 0.99 ** 3); term = (rng.random(k) < 0.3).astype(np.uint8)
    special = [(2 * delta, 1.0, 0), (v_max + 7.0, 0.99, 0), (v_min - 50.0, 0.5, 0), (1.0, 0.99, 1), (2.0, 0.99 ** 3, 0), (0.5 * delta + v_min, 0.0, 0)]
    for j, (r, d, t) in enumerate(special[:k]):
        R_[j], disc[j], term[j] = r, d, t
    return pp, R_, disc, term


@pytest.mark.parametrize("N,k", [(2, 1), (51, 65), (64, 65), (33, 9)])
def test_projection_gather_is_the_scatter_form_and_keeps_mass_and_mean(N, k):
    for v_min, v_max in ((0.0, 100.0), (1.0, 5.0), (-3.0, 2.5)):
        c51 = dict(n_atoms=N, v_min=v_min, v_max=v_max)
        pp, R_, disc, term = hand_made_rows(N, k, v_min, v_max)
        m = Z.project(pp, R_, disc, term, c51)
        ms, clamped = _scatter(pp, R_, disc, term, c51)
        assert np.array_equal(m, ms), "gather and scatter agree to the last bit"
        assert np.all(m >= 0.0)
        mass, want = m.sum(axis=0), pp.sum(axis=0)
        assert np.all(np.abs(mass - want) <= N * np.spacing(1.0)), "rows of m sum to Σp' within N ulp"
        z = Z.atoms(c51)[0]
        mean, mean_want = (m * z[:, None]).sum(axis=0), (pp * clamped).sum(axis=0)
        scale = max(abs(v_min), abs(v_max))
        assert np.all(np.abs(mean - mean_want) <= 4 * N * np.spacing(scale)), "Σ m·z = Σ p'·clamp(Tz) within rounding"
    # the special rows do what they say (N >= 3, v = 0..100)
    if N >= 33 and k >= 6:
        c51 = dict(n_atoms=N, v_min=0.0, v_max=100.0)
        pp, R_, disc, term = hand_made_rows(N, k, 0.0, 100.0)
        m = Z.project(pp, R_, disc, term, c51)
        assert np.all(m[:2, 0] == 0.0) and m[2, 0] == pp[0, 0], "Tz on an atom: a shift by two atoms; atom 2 receives p'_0 whole"
        assert m[N - 1, 1] == Z.sum_atoms(pp[:, 1:2])[0] and np.all(m[:N - 1, 1] == 0.0), "the upper clamp collects everything"
        assert m[0, 2] == Z.sum_atoms(pp[:, 2:3])[0] and np.all(m[1:, 2] == 0.0), "the lower clamp collects everything"
        assert np.count_nonzero(m[:, 3]) <= 2 and np.count_nonzero(m[:, 5]) == 2, "a terminal and gamma = 0 put all mass between two atoms"


# ---------------------------------------------------------------------------------------------------- the bars as recorded, the mutants, the cheapest cases
@pytest.fixture(scope="module")
def prof():
    return json.load(open(B.BAR_JSON))


def test_recorded_bars_come_from_the_floor_and_every_case_keeps_its_trajectory(prof):
    assert set(prof["cases"]) == {c["name"] for c in B.CASES} and len(B.CASES) >= 12
    assert prof["jitter_ulp"] == B.JITTER_ULP == 2 and prof["loss_factor"] == B.LOSS_FACTOR and prof["param_bar"] == B.PARAM_BAR
    assert prof["loss_bar"] == B.LOSS_FACTOR * max(r["floor"]["loss"] for r in prof["cases"].values())
    assert prof["proj_bar"] == B.LOSS_FACTOR * max(r["floor"]["proj"] for r in prof["cases"].values())
    assert 0.0 < prof["loss_bar"] < 1e-12 and 0.0 < prof["proj_bar"] < 1e-12
    for n, rec in prof["cases"].items():
        assert rec["ties_ok"], (n, "a jittered twin left the reference's trajectory: the case needs another seed")
        assert rec["floor"]["q"] <= B.PARAM_BAR and rec["floor"]["target"] <= B.PARAM_BAR, n
        assert rec["stats"]["updates"] >= 3 and rec["stats"]["greedy_steps"] > 0, n
        assert B.case_cfg(B.CASE[n]).seed == rec["seed"] and B.case_c51(B.CASE[n]) == rec["c51"], (n, "the table is the recorded one")
    seen = prof["cases"]
    assert 0 < seen["k31_n51"]["stats"]["greedy_ones"] < seen["k31_n51"]["stats"]["greedy_steps"], "both greedy actions occur"
    assert B.case_cfg(B.CASE["k5"]).batch_size == B.TD_WAVES + 1


def test_every_mutant_lies_far_outside_the_bars_where_it_is_seen_best(prof):
    assert set(prof["mutants"]) == set(B.MUTANTS) and len(B.MUTANTS) == 7
    for m, rec in prof["mutants"].items():
        assert rec["best_ratio"] >= B.MUTANT_FACTOR, (m, rec)
    assert prof["mutants"]["M2"]["best_case"] == "vmin1", "only a live lower clamp shows a missing clamp: b's own cap hides the upper one"


@pytest.mark.parametrize("name", B.CHEAPEST)
def test_the_cheapest_cases_recompute_to_the_recorded_figures(prof, name):
    rec, got = prof["cases"][name], B.measure(B.CASE[name])
    assert got["ties_ok"] and got["floor"] == rec["floor"] and got["stats"] == rec["stats"]
    assert got["mutants"] == rec["mutants"]


# ---------------------------------------------------------------------------------------------------- the Python layer and the header
def test_python_layer_and_header():
    import cleanrl_jl_amd as crl
    L = crl._lib
    assert C.sizeof(L.CrlDQNC51Options) == 24
    assert [f for f, _ in L.CrlDQNC51Options._fields_] == ["n_atoms", "pad", "v_min", "v_max"]
    d = crl.C51Options()
    assert (d.n_atoms, d.v_min, d.v_max) == (51, 0.0, 100.0)
    assert L.dqn_c51_param_count(51) == 19434 == Z.param_count(51) and L.dqn_c51_param_count(2) == 10764 + 340
    header = open(os.path.join(B.B.ROOT, "include", "cleanrl_hip.h")).read()
    for name in ("crl_dqn_c51_create", "crl_dqn_param_count", "crl_dqn_c51_make_nn", "crl_dqn_c51_probs", "crl_dqn_c51_read", "crl_dqn_c51_project_probe"):
        assert re.search(r"int32_t\s+" + name + r"\(", header), name
        assert name in L.EXPORTS, name
    assert re.search(r"typedef struct crl_dqn_c51_options \{ int32_t n_atoms; int32_t pad; double v_min, v_max; \}", header)
    nn = crl.make_nn_c51(3, 33)
    assert nn.dtype == np.float32 and nn.size == Z.param_count(33)
    assert np.array_equal(nn[:480], crl.make_nn(3)[:480]), "the same trunk draws for the same seed"
    assert np.all(nn[480:600] == 0.0) and np.all(nn[-66:] == 0.0) and np.all(nn[Z.TRUNK:-66] != 0.0)
    assert np.abs(nn[Z.TRUNK:-66]).max() <= np.sqrt(6.0 / (66 + 84))
    # validation happens before the library is touched
    for bad, what in ((dict(n_atoms=1), "n_atoms"), (dict(n_atoms=65), "n_atoms"), (dict(n_atoms=51.0), "n_atoms"), (dict(n_atoms=True), "n_atoms"),
                      (dict(v_min=5.0, v_max=5.0), "v_min"), (dict(v_min=6.0, v_max=5.0), "v_min"), (dict(v_max=float("inf")), "v_max"),
                      (dict(v_min=float("nan")), "v_min"), (dict(v_max="100"), "v_max")):
        with pytest.raises(ValueError, match=what):
            crl.DQNAgent(crl.DQNConfig(), dist=crl.C51Options(**bad))
    with pytest.raises(TypeError, match="C51Options"):
        crl.DQNAgent(crl.DQNConfig(), dist=dict(n_atoms=51))
