"""The noisy-layer restatement tests/noisy_ref.py on the CPU: its mu- and sigma-gradients against central finite differences, the factorised
structure of eps, the generation schedule, the init bounds, the ±2 ulp robustness of the xi probe, the mutants of tests/noisy_bar.py, and the recorded
bars. No GPU."""
import json
import os

import numpy as np
import pytest

import c51_ref as Z
import ddpg_ref as R
import dqn_per_ref as P
import dqn_target_ref as T
import duel_ref as D
import noisy_bar as B
import noisy_ref as N


# ---------------------------------------------------------------------------------------------------- gradients by finite differences
def _dyadic(x, bits):
    return np.round(np.asarray(x, np.float64) * 2.0 ** bits) / 2.0 ** bits


def _fd_setup(dueling):
    """a net whose every image stays EXACT in Float32 under the perturbations below: mu on the 2^-10 grid, sigma on 2^-4, xi on 2^-3 (so eps on 2^-6
    and sigma·eps on 2^-10), steps of 2^-12 / 2^-13 in mu and 2^-6 / 2^-7 in sigma (times eps: 2^-12 / 2^-13). |w| < 4 needs 15 bits: no rounding
    anywhere between (mu, sigma) and the image, so the finite difference sees the loss at exactly the points it asks for."""
    lay = N.layers(dueling)
    rng = np.random.default_rng(3)
    Pn = N.param_count(lay)
    mu = _dyadic(np.concatenate([rng.uniform(-1, 1, o * (i + 1)) / np.sqrt(i) for i, o in lay]), 10)
    sigma = _dyadic(rng.uniform(0.05, 0.3, Pn), 4) + 2.0 ** -4
    xi = _dyadic(np.clip(rng.standard_normal(N.n_xi(lay)), -1.9, 1.9), 3).astype(np.float32)
    k = 6
    state = rng.uniform(-1.0, 1.0, (4, k)); a = rng.integers(0, 2, k); td = rng.uniform(0.0, 3.0, k); w = rng.uniform(0.5, 1.0, k)
    loss_grads = D.scalar_loss_grads if dueling else T.loss_grads
    return lay, Pn, mu, sigma, N.eps_of(lay, xi), (state, a, td, w), loss_grads


@pytest.mark.parametrize("dueling", [False, True])
def test_mu_and_sigma_gradients_match_central_finite_differences(dueling):
    """d/dmu L(mu + sigma·eps) = g and d/dsigma = g·eps, g the wrapped restatement's gradient at the image. The loss is a piecewise polynomial of the
    weights (relu, mse), so a central difference with step h is off by h²·|L'''|/6 inside a piece; that term is MEASURED from the differences' own
    convergence, |FD(h) − FD(h/2)|·4/3 (Richardson: the h² term drops by 4), without looking at the gradient under test. Rounding adds at most
    2^-40·|L|/h per difference (every sum here has < 2^12 Float64 terms of one sign scale), and the Float32 projection of g and of g·eps in split_grad
    adds 2^-23 + 2^-23 relative per entry. Expected agreement: |FD − analytic| <= 2·Richardson + rounding + projection; the bound itself must lie under
    1e-3 of the derivative, else the check would show nothing."""
    lay, Pn, mu, sigma, eps, data, loss_grads = _fd_setup(dueling)
    state, a, td, w = data
    eps64 = eps.astype(np.float64)
    assert np.array_equal(N.image(mu, sigma, eps).astype(np.float64), mu + sigma * eps64), "the image is exact on this grid"

    def loss(m, s):
        img = N.image(m, s, eps)
        assert np.array_equal(img.astype(np.float64), m + s * eps64)
        return float(loss_grads(img, state, a, td, w)[0])

    L0, g64, _ = loss_grads(N.image(mu, sigma, eps), state, a, td, w)
    full = N.split_grad(g64, eps).astype(np.float64)
    rng = np.random.default_rng(4)
    checked = 0
    for trial in range(12):
        d_mu, d_sg = np.zeros(Pn), np.zeros(Pn)
        live = np.flatnonzero(g64 != 0.0)
        pick = rng.choice(live, 8, replace=False)
        (d_mu if trial % 2 == 0 else d_sg)[pick] = rng.choice([-1.0, 1.0], 8)
        analytic = float(d_mu @ full[:Pn] + d_sg @ full[Pn:])
        fd = []
        for h_mu, h_sg in ((2.0 ** -12, 2.0 ** -6), (2.0 ** -13, 2.0 ** -7)):
            h = h_mu if trial % 2 == 0 else h_sg
            fd.append((loss(mu + h_mu * d_mu, sigma + h_sg * d_sg) - loss(mu - h_mu * d_mu, sigma - h_sg * d_sg)) / (2.0 * h))
        h_small = 2.0 ** -13 if trial % 2 == 0 else 2.0 ** -7
        richardson = abs(fd[0] - fd[1]) * 4.0 / 3.0
        rounding = 2.0 ** -40 * abs(float(L0)) / h_small
        projection = 2.0 ** -22 * float(np.abs(d_mu) @ np.abs(full[:Pn]) + np.abs(d_sg) @ np.abs(full[Pn:]))
        bound = 2.0 * richardson + rounding + projection
        print(f"{'mu' if trial % 2 == 0 else 'sigma'} direction {trial}: analytic {analytic:.6e}, FD(h/2) {fd[1]:.6e}, |diff| {abs(fd[1] - analytic):.2e}, bound {bound:.2e}")
        assert abs(fd[1] - analytic) <= bound
        if bound <= 1e-3 * abs(analytic):
            checked += 1
    assert checked >= 8, "most directions cross no relu kink: the bound is sharp there"


# ---------------------------------------------------------------------------------------------------- the structure of eps
@pytest.mark.parametrize("dueling,n_atoms", [(False, None), (False, 33), (True, None), (True, 64)])
def test_eps_is_factorised_and_the_bias_noise_is_xi_out(dueling, n_atoms):
    lay = N.layers(dueling, n_atoms)
    assert N.n_xi(lay) == (700 + 3 * (n_atoms or 1) if dueling else 412 + (2 * n_atoms if n_atoms else 2)) <= 892
    twin = D.param_count(n_atoms or 1) if dueling else (Z.param_count(n_atoms) if n_atoms else 10934)
    assert N.param_count(lay) == twin and sum(N.array_sizes(lay)) == twin
    xi = N.xi_table(21, lay, 5, 0)
    eps = N.eps_of(lay, xi)
    assert eps.dtype == np.float32 and eps.size == twin
    at = x = 0
    for i, o in lay:
        Wm = eps[at:at + o * i].reshape((o, i), order="F").astype(np.float64)
        # each entry is one Float32 product, off its exact value by at most 2^-24 of itself, so what lies beyond rank 1 is below 2^-24·‖eps‖_F
        assert np.linalg.matrix_rank(Wm, tol=2.0 ** -23 * np.linalg.norm(Wm)) == 1, "rank 1 up to the Float32 rounding of the products"
        assert np.array_equal(Wm.astype(np.float32), (xi[x + i:x + i + o, None] * xi[None, x:x + i])), "xi_out[i] * xi_in[j], one Float32 multiply"
        assert np.array_equal(eps[at + o * i:at + o * (i + 1)], xi[x + i:x + i + o]), "bias noise = xi_out"
        at += o * (i + 1); x += i + o
    z = N.normal(21, np.arange(N.n_xi(lay)), 5, N.S_NOISY[0])
    assert np.array_equal(z, R.normal(21, np.arange(N.n_xi(lay)), 5, 0x22)), "the Box–Muller form DDPG's noise uses, stream 0x22"
    assert np.array_equal(xi, (np.sign(z) * np.sqrt(np.abs(z))).astype(np.float32))
    assert not np.array_equal(xi, N.xi_table(21, lay, 5, 1)) and not np.array_equal(xi, N.xi_table(21, lay, 6, 0))
    assert not np.array_equal(xi, N.xi_table(21, lay, 5 + 2 ** 32, 0)), "the generation's high word enters the counter"


def test_the_probe_set_survives_two_ulp_in_log_and_cos():
    """tests/test_gpu_noisy.py allows 2 of its probed xi not to be bit-equal to the restatement and every one to be one Float32 ulp off; here the
    restatement with its log and cos results nudged by ±2 ulp stays within that on the same inputs"""
    import test_gpu_noisy as G
    worst = 0
    for seed in B.JITTER_SEEDS:
        off = total = 0
        for name, n_xi in G.PROBE_TABLES:
            case = B.CASE[name]
            lay, s = B.case_layers(case), B.case_cfg(case).seed
            for gen in G.PROBE_GENS:
                for net in (0, 1):
                    want = N.xi_table(s, lay, gen, net)
                    with B.nudged(seed):
                        got = N.xi_table(s, lay, gen, net)
                    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)))
                    off += int((got != want).sum()); total += n_xi
        assert total == 16072
        worst = max(worst, off)
    print(f"nudged by ±2 ulp: at most {worst} of 16072 probed values change their Float32 rounding")
    assert worst <= 2


# ---------------------------------------------------------------------------------------------------- the schedule
def test_generation_schedule():
    """generation = completed updates for both nets; the target's mu and sigma move only with a copy, its image with every update"""
    case = B.CASE["wrap_cap31_duel"]
    cfg = B.case_cfg(case)
    ref = B.make_ref(case)
    assert ref.gens == [(0, 0, 0)] and np.array_equal(ref.pq, ref.pt) and not np.array_equal(ref.q, ref.t), "one mu and sigma, two streams"
    Pn = ref.P
    assert np.array_equal(ref.q, N.image(ref.pq[:Pn], ref.pq[Pn:], N.eps_of(ref.lay, N.xi_table(cfg.seed, ref.lay, 0, 0))))
    ref.run(41)
    assert ref.n_updates == 0 and ref.gens == [(0, 0, 0)]
    seen_t = []
    for stop in (42, 45, 48, 150):
        pt, t = ref.pt.copy(), ref.t.copy()
        ref.run(stop - ref.global_step)
        seen_t.append((np.array_equal(pt, ref.pt), np.array_equal(t, ref.t)))
        u = ref.n_updates
        assert ref.gens[-1] == (u, u, u)
        assert np.array_equal(ref.t, N.image(ref.pt[:Pn], ref.pt[Pn:], N.eps_of(ref.lay, N.xi_table(cfg.seed, ref.lay, u, 1))))
        assert np.array_equal(ref.q, N.image(ref.pq[:Pn], ref.pq[Pn:], N.eps_of(ref.lay, N.xi_table(cfg.seed, ref.lay, u, 0))))
    assert seen_t == [(True, False), (True, False), (True, False), (False, False)], "no copy before step 150, yet a new target image every update"
    assert np.array_equal(ref.pq, ref.pt) and [g[0] for g in ref.gens] == list(range(38))
    keep = ref.pq.copy()
    ref.write_params(keep)
    assert ref.gens[-1] == (37, 37, 37), "write_params rebuilds at the current generation"


def test_a_tape_replaces_the_draw():
    case = B.CASE["k1_cap1"]
    lay, seed = B.case_layers(case), B.case_cfg(case).seed
    tape = {(g, net): N.xi_table(seed, lay, g, net) for g in range(120) for net in (0, 1)}
    a, b = B.run_ref(case), B.run_ref(case, None, tape)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2]))


# ---------------------------------------------------------------------------------------------------- init
def test_init_bounds():
    import cleanrl_jl_amd as crl
    for dueling, n_atoms in ((False, None), (False, 51), (True, None), (True, 51)):
        lay = N.layers(dueling, n_atoms)
        Pn = N.param_count(lay)
        for p in (crl.make_nn_noisy(3, 0.5, dueling, n_atoms), crl._lib.dqn_noisy_make_nn_host(3, 0.5, dueling, n_atoms)):
            assert p.dtype == np.float32 and p.size == 2 * Pn
            at = 0
            for i, o in lay:
                n, lim = o * (i + 1), 1.0 / np.sqrt(float(i))
                mu, sg = p[at:at + n], p[Pn + at:Pn + at + n]
                assert np.abs(mu).max() <= np.float32(lim) and mu.max() > 0.8 * lim and mu.min() < -0.8 * lim, "U(−1/√in, +1/√in), biases included"
                assert np.all(mu[-o:] != 0.0), "the biases draw as well"
                assert np.all(sg == np.float32(0.5 * lim)), "sigma = sigma0/√in"
                at += n
    z = crl._lib.dqn_noisy_make_nn_host(3, 0.0)
    assert np.all(z[10934:] == 0.0) and np.array_equal(z[:10934], crl._lib.dqn_noisy_make_nn_host(3, 0.5)[:10934])
    assert not np.array_equal(z, crl._lib.dqn_noisy_make_nn_host(4, 0.0))


# ---------------------------------------------------------------------------------------------------- mutants and bars
@pytest.mark.parametrize("m", [m for m, v in B.MUTANTS.items() if v[1] == "run"])
def test_run_mutants_differ_from_the_restatement(m):
    case = B.CASE["logfreq7" if m == "M4" else "k1_cap1"]   # k1_cap1 copies with every update: there M4 changes nothing, as it should
    base = B.run_ref(case)
    dist, _ = B.variant_distance(case, B.mutant(m), base)
    print(m, B.MUTANTS[m][0], dist)
    assert max(dist.values()) > 0.0


def test_noise_and_evaluation_mutants_differ():
    lay = N.layers()
    want = [N.xi_table(21, lay, 1, net) for net in (0, 1)]
    with B.mutant("M2"):
        assert not np.array_equal(N.xi_table(21, lay, 1, 0), want[0])
    with B.mutant("M3"):
        assert np.array_equal(N.xi_table(21, lay, 1, 0), want[0]) and np.array_equal(N.xi_table(21, lay, 1, 1), want[0])
    ref = B.make_ref(B.CASE["c51_n2"])
    X = np.zeros((4, 1)) + 0.01
    q = ref.greedy_q_values(X)
    assert np.array_equal(q, Z.q_of(Z.forward(ref.pq[:ref.P], 2, X)[2], ref.z)), "the twin's Q on the mu half"
    with B.mutant("M8"):
        assert not np.array_equal(ref.greedy_q_values(X), q)


def test_recorded_bars_are_reproducible():
    prof = json.load(open(B.BAR_JSON))
    assert set(prof["cases"]) == {c["name"] for c in B.CASES} - set(B.EXACT) and prof["exact_cases"] == list(B.EXACT)
    assert prof["loss_bar"] == B.LOSS_FACTOR * prof["loss_floor"] and prof["proj_bar"] == B.LOSS_FACTOR * prof["proj_floor"] and prof["param_bar"] == B.PARAM_BAR
    assert all(rec["same_episodes"] and all(rec["floor"][o] <= prof["param_bar"] for o in ("q", "target", "image_q", "image_t")) for rec in prof["cases"].values())
    got = B.measure(B.CASE["c51_n2"])
    assert got["floor"] == prof["cases"]["c51_n2"]["floor"] and got["same_episodes"]
    # a uniform scalar case runs no transcendental: jittering exp, log and pow moves nothing
    exact = B.CASE["k1_cap1"]
    dist, same = B.variant_distance(exact, B.jitter(1), B.run_ref(exact))
    assert same and all(v == 0.0 for v in dist.values())


# ---------------------------------------------------------------------------------------------------- scripts/run.py
def test_run_script_defaults_epsilon_to_zero_with_noisy(monkeypatch):
    """`scripts/run.py dqn --noisy` is the NoisyNet setting unless the two are given; without --noisy the reference's schedule stays"""
    import importlib.util
    import sys

    import cleanrl_jl_amd as crl
    spec = importlib.util.spec_from_file_location("run_script", os.path.join(B.B.ROOT, "scripts", "run.py"))
    run = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(run)
    calls = []

    class _Agent:
        def close(self):
            pass

    def fake_dqn(config, per, target, dist, dueling, noisy, **kw):
        calls.append((config, per, target, dist, dueling, noisy))
        return _Agent()
    monkeypatch.setattr(run.crl, "dqn", fake_dqn)
    for argv in (["dqn", "--noisy"], ["dqn", "--sigma0", "0.25", "--dueling"], ["dqn", "--noisy", "--epsilon_start", "0.5", "--epsilon_end", "0.01"], ["dqn"]):
        monkeypatch.setattr(sys, "argv", ["run.py"] + argv)
        run.main()
    (c0, *_, n0), (c1, _, _, _, d1, n1), (c2, *_, n2), (c3, *_, n3) = calls
    assert (c0.epsilon_start, c0.epsilon_end) == (0.0, 0.0) and n0 == crl.NoisyOptions(0.5)
    assert (c1.epsilon_start, c1.epsilon_end) == (0.0, 0.0) and n1 == crl.NoisyOptions(0.25) and d1 is True
    assert (c2.epsilon_start, c2.epsilon_end) == (0.5, 0.01) and n2 == crl.NoisyOptions(0.5)
    assert (c3.epsilon_start, c3.epsilon_end) == (1.0, 0.05) and n3 is None
