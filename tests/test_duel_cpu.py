"""The yardstick of the dueling-DQN parity tests, without a GPU. The dueling heads have no Julia reference, so tests/duel_ref.py's hand-written
gradient is proved first, by central finite differences of its own loss in Float64, on both heads. Then the mutants, the reductions to the plain net,
the recorded bars of tests/duel_bar.py, and the Python layer.

The agreement bound of the gradient check is tests/test_sac_cpu.py's, for the same step h = 1e-5, and its reasoning carries over: a loss here is a
mean of k values of size < 10 (a squared TD error against targets in 0..2, or a cross-entropy <= log(N) + a few), each behind dot products of at most
480 + 2·84·120 + 3R·84 < 22,000 terms at R <= 5, so the worst-case rounding 22,000 · 1.1e-16 · 10 / h = 2.4e-6 stays the order of TOL while the
random-walk figure is sqrt(22,000) · 1.1e-16 · 10 / h = 1.6e-8 — tests/test_c51_cpu.py's figures, whose net is the same size to within the second
stream —; the combine is linear and the softmax's third derivative along a logit is below 1, so the truncation h²/6 is 2e-11. EXPECTED below is
test_sac_cpu.EXPECTED, and as there no relu pre-activation may lie within test_sac_cpu.KINK of zero: the setup takes the first seed for which none
does."""
import json
import os
import re

import numpy as np
import pytest

import c51_ref as Z
import ddpg_ref as R
import dqn_per_ref as P
import duel_bar as B
import duel_ref as D
import test_sac_cpu as SC

H = SC.H_STEP


# ---------------------------------------------------------------------------------------------------- the gradient
def split64(p, Rr):
    """duel_ref.split without the Float32 projection: the perturbation has to survive"""
    out, o = [], 0
    for n, shape in zip(D.sizes(Rr), D.shapes(Rr)):
        out.append(np.asarray(p[o:o + n], np.float64).reshape(shape, order="F")); o += n
    return out


def _loss64(head, qp64, Rr, state, a, tgt, w):
    with D.replaced(D, split=split64):
        if head == "scalar":
            return D.scalar_loss_grads(qp64, state, a, tgt, w)
        return D.c51_loss_grads(qp64, Rr, state, a, tgt, w)


def _pre_activations(qp, Rr, state):
    W1, b1, W2v, b2v, _, _, W2a, b2a, _, _ = split64(qp, Rr)
    z1 = R.dense(W1, b1, state)
    h1 = P.relu(z1)
    return np.concatenate([z1.ravel(), R.dense(W2v, b2v, h1).ravel(), R.dense(W2a, b2a, h1).ravel()])


def _setup(head, Rr, k, seed):
    while True:
        rng = np.random.default_rng(seed)
        qp = np.asarray(B.params_for(Rr), np.float64)
        state = rng.uniform(-1, 1, (4, k))
        a = rng.integers(0, 2, k)
        if head == "scalar":
            tgt = rng.uniform(0.0, 2.0, k)
        else:
            tgt = rng.random((Rr, k)); tgt = tgt / tgt.sum(axis=0)
        w = rng.uniform(0.3, 1.0, k)
        if np.abs(_pre_activations(qp, Rr, state)).min() > SC.KINK and a.min() != a.max():
            return qp, state, a, tgt, w
        seed += 1


@pytest.mark.parametrize("head,Rr,k", [("scalar", 1, 7), ("c51", 5, 7), ("c51", 2, 4)])
def test_the_hand_written_gradient_agrees_with_central_differences(head, Rr, k):
    qp, state, a, tgt, w = _setup(head, Rr, k, 1)
    loss, grad, _ = _loss64(head, qp, Rr, state, a, tgt, w)
    rng = np.random.default_rng(9)
    off = np.cumsum([0] + D.sizes(Rr))
    worst, checked = 0.0, 0
    for arr in range(10):
        for p in rng.choice(np.arange(off[arr], off[arr + 1]), min(6, off[arr + 1] - off[arr]), replace=False):
            up, dn = qp.copy(), qp.copy()
            up[p] += H; dn[p] -= H
            fd = (_loss64(head, up, Rr, state, a, tgt, w)[0] - _loss64(head, dn, Rr, state, a, tgt, w)[0]) / (2 * H)
            worst = max(worst, abs(fd - grad[p])); checked += 1
    print(f"{head} R {Rr} k {k}: {checked} entries over the ten arrays, worst |fd - grad| {worst:.3e} (expected <= {SC.EXPECTED}, proved <= {SC.TOL})")
    assert worst <= SC.EXPECTED
    assert np.abs(grad).max() > 1e-3 and loss > 0.0 and loss < 10.0
    # unlike the plain head, both actions' advantage rows get a term from every sample (dA = ±g/2): b3a's two halves are exact negatives
    gb3a = grad[off[9]:off[10]]
    assert np.all(gb3a != 0.0) and np.array_equal(gb3a[:Rr], -gb3a[Rr:])


@pytest.mark.parametrize("m", ["M3", "M4", "M5"])
def test_a_wrong_backward_line_is_far_outside_the_bound(m):
    qp, state, a, tgt, w = _setup("c51", 5, 7, 1)
    good = _loss64("c51", qp, 5, state, a, tgt, w)[1]
    with D.replaced(D, **B.MUTANTS[m][1]()):
        bad = _loss64("c51", qp, 5, state, a, tgt, w)[1]
    print(f"{m}: the gradient moves by {np.abs(good - bad).max():.3e}")
    assert np.abs(good - bad).max() > 1e-3 > 100 * SC.TOL


# ---------------------------------------------------------------------------------------------------- reductions to the plain net
def plain_in_advantage_stream(plain, Rr=1):
    """a dueling net whose value head is zero and whose advantage stream is the plain net's layers 2-3 (W1 b1 shared); shared with tests/test_gpu_duel.py"""
    assert Rr == 1
    out = np.array(B.params_for(1), np.float32)
    off = np.cumsum([0] + D.sizes(1))
    out[off[0]:off[2]] = plain[:600]                        # W1 b1
    out[off[4]:off[6]] = 0.0                                # W3v b3v
    out[off[6]:off[8]] = plain[600:10764]                   # W2a b2a = W2 b2
    out[off[8]:off[10]] = plain[10764:]                     # W3a b3a = W3 b3
    return out


def test_with_a_zero_value_head_the_net_is_the_centred_plain_net():
    import cleanrl_jl_amd as crl
    plain = crl.make_nn(3) + (0.05 * np.random.default_rng(4).standard_normal(10934)).astype(np.float32)
    X = np.random.default_rng(5).uniform(-2.4, 2.4, (4, 40))
    q = P.forward(plain, X)[2]
    got = D.scalar_forward(plain_in_advantage_stream(plain), X)[2]
    assert np.array_equal(got, q - ((q[0] + q[1]) * 0.5)[None]), "Q = 0 + (A − mean A), bit for bit"
    assert np.array_equal(np.where(got[1] > got[0], 1, 0), np.where(q[1] > q[0], 1, 0)) or np.any(q[0] == q[1])
    for n_atoms, Rr in ((None, 1), (33, 33)):
        nn = crl.make_nn_dueling(3, n_atoms)
        off = np.cumsum([0] + D.sizes(Rr))
        assert nn.dtype == np.float32 and nn.size == D.param_count(Rr)
        assert np.array_equal(nn[:480], crl.make_nn(3)[:480]) and np.array_equal(nn[600:10680], crl.make_nn(3)[600:10680]), "the trunk draws are make_nn's"
        for i in range(10):
            seg = nn[off[i]:off[i + 1]]
            if i % 2:
                assert np.all(seg == 0.0), "zero biases"
            else:
                rows, cols = D.shapes(Rr)[i]
                assert np.all(seg != 0.0) and np.abs(seg).max() <= np.sqrt(6.0 / (rows + cols))


# ---------------------------------------------------------------------------------------------------- the bars as recorded, the mutants, the cheapest cases
@pytest.fixture(scope="module")
def prof():
    return json.load(open(B.BAR_JSON))


def test_recorded_bars_come_from_the_floor_and_every_case_keeps_its_trajectory(prof):
    assert set(prof["cases"]) == {c["name"] for c in B.CASES} and len(B.CASES) == 14
    assert prof["jitter_ulp"] == B.JITTER_ULP == 2 and prof["loss_factor"] == B.LOSS_FACTOR and prof["param_bar"] == B.PARAM_BAR
    assert prof["loss_bar"] == B.LOSS_FACTOR * max(r["floor"]["loss"] for r in prof["cases"].values())
    assert prof["proj_bar"] == B.LOSS_FACTOR * max(r["floor"]["proj"] for r in prof["cases"].values())
    assert 0.0 < prof["loss_bar"] < 1e-12 and 0.0 < prof["proj_bar"] < 1e-12
    for n, rec in prof["cases"].items():
        assert rec["ties_ok"], (n, "a jittered twin left the reference's trajectory: the case needs another seed")
        assert rec["floor"]["q"] <= B.PARAM_BAR and rec["floor"]["target"] <= B.PARAM_BAR, n
        assert rec["stats"]["updates"] >= 3 and rec["stats"]["greedy_steps"] > 0, n
        assert B.case_cfg(B.CASE[n]).seed == rec["seed"] and B.case_c51(B.CASE[n]) == rec["c51"], (n, "the table is the recorded one")
        if n in B.SCALAR_UNIFORM:
            assert all(rec["floor"][o] == 0.0 for o in B.OBSERVABLES), (n, "no transcendental, nothing for the jitter to move")
    assert len(B.SCALAR_UNIFORM) == 8
    seen = prof["cases"]
    assert 0 < seen["k31"]["stats"]["greedy_ones"] < seen["k31"]["stats"]["greedy_steps"], "both greedy actions occur"
    assert B.case_cfg(B.CASE["c51_n51"]).batch_size == B.TD_WAVES + 1


def test_every_mutant_lies_far_outside_the_bars_where_it_is_seen_best(prof):
    assert set(prof["mutants"]) == set(B.MUTANTS) and len(B.MUTANTS) == 6
    for m, rec in prof["mutants"].items():
        print(f"{m} ({rec['what']}): {rec['best_ratio']:.3e} bars on {rec['best_case']}, at least {rec['worst_ratio']:.3e} on the other {rec['cases'] - 1}")
        assert rec["best_ratio"] >= B.MUTANT_FACTOR, (m, rec)


@pytest.mark.parametrize("name", B.CHEAPEST)
def test_the_cheapest_cases_recompute_to_the_recorded_figures(prof, name):
    rec, got = prof["cases"][name], B.measure(B.CASE[name])
    assert got["ties_ok"] and got["floor"] == rec["floor"] and got["stats"] == rec["stats"]
    assert got["mutants"] == rec["mutants"]


# ---------------------------------------------------------------------------------------------------- the Python layer and the header
def test_python_layer_and_header():
    import cleanrl_jl_amd as crl
    L = crl._lib
    assert L.dqn_dueling_param_count() == 21183 == D.param_count(1) and L.dqn_dueling_param_count(51) == 33933 == D.param_count(51)
    assert L.dqn_dueling_param_count(64) * 4 == 148992 and L.dqn_dueling_param_count(2) == 20928 + 510
    header = open(os.path.join(B.B.ROOT, "include", "cleanrl_hip.h")).read()
    for name in ("crl_dqn_dueling_create", "crl_dqn_dueling_make_nn", "crl_dqn_dueling_streams"):
        assert re.search(r"int32_t\s+" + name + r"\(", header), name
        assert name in L.EXPORTS, name
    assert "W1(120,4) b1  W2v(84,120) b2v  W3v(R,84) b3v  W2a(84,120) b2a  W3a(2R,84) b3a" in header
    # validation happens before the library is touched
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="dueling"):
            crl.DQNAgent(crl.DQNConfig(), dueling=bad)
    with pytest.raises(ValueError, match="n_atoms"):
        crl.DQNAgent(crl.DQNConfig(), dist=crl.C51Options(n_atoms=65), dueling=True)
    with pytest.raises(TypeError, match="PEROptions"):
        crl.DQNAgent(crl.DQNConfig(), per=dict(alpha=0.6), dueling=True)
