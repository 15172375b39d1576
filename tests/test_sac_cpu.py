"""The yardstick of the SAC parity tests, without a GPU. SAC has no Julia reference, so tests/sac_ref.py's hand-written gradients are proved first, by
central finite differences in Float64: the actor loss against every actor array, the alpha loss against log_alpha, each critic's loss against its
arrays. Then the pieces the header pins (the draw's component word and streams, the squash at and past saturation, autotune = 0) and the
behaviour policy.

The agreement bound, from the step h = 1e-5 alone. fd = (f(w + h) − f(w − h)) / 2h differs from the derivative f1(w) by the truncation h²·|f3|/6 (f3
the third derivative along that weight) and by the rounding (e₊ + e₋)/2h, e± the absolute errors of the two loss evaluations.
  rounding    a loss is a mean of k values of size <= 10, each behind dot products of at most 64·(64 + D + A) + 2·64 < 4500 terms; accumulating
              every one of them in the worst direction gives e <= 4500 · 1.1e-16 · 10 = 5e-12, so (e₊ + e₋)/2h <= 5e-7.
  truncation  f3 carries the cube of the weight's input (|x| <= 4 for the observations, <= 1 behind a tanh, <= 6 behind a relu on these nets), a
              third derivative of tanh (<= 2 in magnitude) and the gains of the layers after it (each <= 10 here): |f3| <= 6³ · 2 · 10 · 10 < 5e4,
              so h²·|f3|/6 < 9e-7.
TOL = 2e-6 is their sum, rounded up; both terms are worst cases. What to EXPECT is far smaller, and is asserted beside it (EXPECTED = 1e-8): rounding
errors that accumulate as a random walk give e = sqrt(4500) · 1.1e-16 · 10 = 7.4e-14, so 7.4e-9 after the division by h, and a weight whose input
and downstream gains are of size 1 has |f3| <= 2 · 10, a truncation of 3e-10. The proof rests on TOL; EXPECTED keeps the measured agreement (a few
1e-10 on both shapes) from degrading unseen. The gradients checked are of size 1e-3 .. 1, and
a wrong factor, sign, index or a missing term moves them by more than 1e-3 (test_a_wrong_gradient_is_far_outside_the_bound). The step moves no
pre-activation by more than h · 6 = 6e-5: the test asserts that no relu pre-activation and no q1 − q2 lies within 1e-4 of zero, so no kink and
no switch of the selected critic sits inside a difference."""
import numpy as np
import pytest

import ddpg_bar as DB
import ddpg_ref as R
import sac_bar as B
import sac_ref as S

H_STEP, TOL, EXPECTED, KINK = 1e-5, 2e-6, 1e-8, 1e-4


def split64(p, n_in, n_out):
    """ddpg_ref.split without the Float32 projection: a finite difference needs the Float64 perturbation to survive"""
    out, o = [], 0
    for n, shape in zip(R.net_sizes(n_in, n_out), ((R.H, n_in), (R.H,), (R.H, R.H), (R.H,), (n_out, R.H), (n_out,))):
        out.append(np.asarray(p[o:o + n], np.float64).reshape(shape, order="F")); o += n
    return out


def _setup(D, A, k, seed):
    case = dict(D=D, A=A, mu_gain=1.0, s_gain=1.0, mu_shift=0.0)
    actor, c1, c2 = (np.asarray(p, np.float64) for p in B.case_params(case))
    rng = np.random.default_rng(seed)
    batch = dict(state=rng.standard_normal((D, k)), action=rng.uniform(-2, 2, (A, k)), reward=rng.standard_normal(k),
                 next_state=rng.standard_normal((D, k)), terminal=(rng.random(k) < 0.3).astype(np.uint8))
    eps = S.draws(0x5EED, 77, k, A, S.S_PI)
    td = rng.standard_normal(k)
    return actor, c1, c2, batch, eps, td


def _relu_margin(critic, D, A, X):
    W1, b1, W2, b2, _, _ = split64(critic, D + A, 1)
    z1 = R.dense(W1, b1, X)
    z2 = R.dense(W2, b2, np.maximum(z1, 0.0))
    return min(np.abs(z1).min(), np.abs(z2).min())


def _fd(f, w, idx):
    out = []
    for i in idx:
        wp, wm = w.copy(), w.copy()
        wp[i] += H_STEP; wm[i] -= H_STEP
        out.append((f(wp) - f(wm)) / (2.0 * H_STEP))
    return np.array(out)


def _entries(sizes, rng, per_array=6):
    """per_array entries of every array of a flat parameter vector (all of an array that has fewer)"""
    idx, o = [], 0
    for n in sizes:
        idx += (o + (np.arange(n) if n <= per_array else rng.choice(n, per_array, replace=False))).tolist(); o += n
    return idx


# the seeds are the first for which the no-kink precondition below holds on the shape
@pytest.mark.parametrize("D,A,k,seed", [(3, 1, 7, 1), (5, 3, 4, 1)])
def test_the_hand_written_gradients_agree_with_central_differences(D, A, k, seed):
    actor, c1, c2, batch, eps, td = _setup(D, A, k, seed)
    alpha, te, (scale, bias) = 0.37, -float(A), S.scale_bias(-1.0, 0.5)
    rng = np.random.default_rng(9)
    with DB.patched(split=split64):
        logp, qmin, ga, smp, gap = S.actor_pass(actor, c1, c2, D, A, batch, eps, alpha, scale, bias)
        # the precondition: no kink inside a difference
        Xa, Xc = np.vstack([batch["state"], smp["a"]]), np.vstack([batch["state"], batch["action"]])
        margin = min(_relu_margin(c, D, A, X) for c in (c1, c2) for X in (Xa, Xc))
        assert margin > KINK and np.abs(gap).min() > KINK, (margin, np.abs(gap).min())
        assert (gap > 0).any() and (gap < 0).any(), "both critics are selected somewhere in the batch"
        # the actor loss against every actor array
        idx = _entries(R.net_sizes(D, 2 * A), rng)
        fd = _fd(lambda w: S.actor_loss(alpha, *S.actor_pass(w, c1, c2, D, A, batch, eps, alpha, scale, bias)[:2]), actor, idx)
        err = np.abs(fd - ga[idx]).max()
        print("actor", err, np.abs(ga[idx]).max())
        assert err <= EXPECTED < TOL and np.abs(ga[idx]).max() > 1e-3
        # each critic's loss against its arrays
        for c in (c1, c2):
            _, gc = R.critic_loss_grad(c, D, A, batch, td)
            idx = _entries(R.net_sizes(D + A, 1), rng)
            fd = _fd(lambda w: R.critic_loss_grad(w, D, A, batch, td)[0], c, idx)
            err = np.abs(fd - gc[idx]).max()
            print("critic", err, np.abs(gc[idx]).max())
            assert err <= EXPECTED < TOL and np.abs(gc[idx]).max() > 1e-3
        # the alpha loss against log_alpha: its own value
        la = np.array([np.log(alpha)])
        fd = _fd(lambda w: S.alpha_loss(S.alpha_of(w[0]), logp, te), la, [0])[0]
        assert abs(fd - S.alpha_loss(alpha, logp, te)) <= EXPECTED and abs(fd) > 1e-3


def test_a_wrong_gradient_is_far_outside_the_bound():
    """what the bound tells apart: each gradient mutant of tests/sac_bar.py moves the checked entries by orders of magnitude more than TOL"""
    D, A, k = 3, 1, 7
    actor, c1, c2, batch, eps, _ = _setup(D, A, k, 1)
    scale, bias = S.scale_bias(-1.0, 0.5)
    with DB.patched(split=split64):
        good = S.actor_pass(actor, c1, c2, D, A, batch, eps, 0.37, scale, bias)[2]
        for m in ("S5", "S6"):
            with B.patched(**B.MUTANTS[m][2]()):
                bad = S.actor_pass(actor, c1, c2, D, A, batch, eps, 0.37, scale, bias)[2]
            assert np.abs(bad - good).max() > 1e-3 > 100 * TOL, m


def test_the_draws_are_per_sample_on_their_own_streams():
    z = S.draws(0x5EED, 77, 5, 3, S.S_NEXT)
    assert z.shape == (3, 5) and len(set(z.reshape(-1).tolist())) == 15
    for b in range(5):
        assert np.array_equal(z[:, b], R.normal(0x5EED, 16 * b + np.arange(3), 77, 0x18))
    assert (S.S_NEXT, S.S_PI) == (0x18, 0x19) and not np.array_equal(z, S.draws(0x5EED, 77, 5, 3, S.S_PI))
    assert not {0x18, 0x19} & {R.S_BEHAVE, R.S_WARMUP, R.S_TARGET, R.S_ACTOR, R.S_RESET, R.S_RESET0, 0x16, 0x17, R.S_SAMPLE}


def test_the_squash_is_well_defined_at_and_past_saturation():
    D, A = 3, 1
    actor = B.actor_params(D, A, 1, mu_gain=0.0, mu_shift=40.0)                 # μ = 40 everywhere: u > 30, tanh_fast returns exactly 1
    X = np.random.default_rng(0).standard_normal((D, 6))
    s = S.sample(actor, D, A, X, np.zeros((A, 6)), 0.75, -0.25)
    assert np.all(s["y"] == 1.0) and np.all(s["a"] == 0.5)
    assert np.array_equal(s["logp"], ((-s["log_std"][0]) - S.HALF_LOG_2PI) - np.log(1e-6)) and np.all(np.isfinite(s["logp"]))
    assert np.all((s["log_std"] >= -5.0) & (s["log_std"] <= 2.0))
    assert np.array_equal(S.mean_action(actor, D, A, X, 0.75, -0.25), np.full((A, 6), 0.5))
    # and there the gradient with respect to μ is exactly zero, the direct term of log_std stays
    c1, c2 = DB.case_params(dict(D=D, A=A), 1)[1], DB.case_params(dict(D=D, A=A), 2)[1]
    batch = dict(state=X)
    g = S.actor_pass(actor, c1, c2, D, A, batch, np.zeros((A, 6)), 0.5, 0.75, -0.25)[2]
    o = sum(R.net_sizes(D, 2 * A)[:5])
    assert g[o] == 0.0 and g[o + 1] != 0.0                                     # b3: the μ row, the s row


def test_autotune_off_keeps_log_alpha_and_its_beta_powers():
    case = B.CASE["autotune_off"]
    ref = S.SAC(B.case_cfg(case), *B.case_params(case)); ref.run_transitions(B.case_transitions(case))
    assert ref.n_updates == 100 and ref.log_alpha[0] == np.float32(np.log(0.2)) and np.array_equal(ref.opt_alpha.bp[0], [R.B1, R.B2])
    assert all(r[1] == ref.alpha_records[0][1] for r in ref.alpha_records) and ref.alpha_records[0][2] != 0.0
    on = S.SAC(dict(B.case_cfg(case), autotune=1), *B.case_params(case)); on.run_transitions(B.case_transitions(case))
    assert on.log_alpha[0] != ref.log_alpha[0] and [r[0] for r in on.alpha_records] == [l[0] for l in on.losses] == list(range(11, 111))


def test_the_behaviour_policy_is_the_warm_up_draw_then_a_sample():
    case = B.CASE["bounds_asym"]
    d = B.case_cfg(case)
    ref = S.SAC(d, *B.case_params(case))
    obs = np.array([0.3, -1.2, 0.5])
    assert np.array_equal(ref.act(obs), -1.0 + 1.5 * R.uniform(d["seed"], np.arange(1), 1, R.S_WARMUP))
    ref.global_step = 20
    a = ref.act(obs)
    eps = R.normal(d["seed"], np.arange(1), 21, R.S_BEHAVE)[:, None]
    assert np.array_equal(a, S.sample(ref.actor, 3, 1, obs[:, None], eps, 0.75, -0.25)["a"][:, 0]) and -1.0 < a[0] < 0.5
