"""The quantile-regression head without a GPU: QROptions is validated before the library is touched, and the restatement's cotangent (tests/qr_ref.py)
agrees with central differences of its own loss."""
import numpy as np
import pytest

import qr_ref as Q

H = 2.0 ** -10


def test_qr_options_are_validated_before_the_library_is_touched():
    import cleanrl_jl_amd as crl
    assert crl.QROptions() == crl.QROptions(n_quantiles=51, kappa=1.0)
    for bad in (1, 65, True, 2.5):
        with pytest.raises(ValueError, match="n_quantiles"):
            crl.DQNAgent(crl.DQNConfig(), dist=crl.QROptions(n_quantiles=bad))
    for bad in (0, -1, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="kappa"):
            crl.DQNAgent(crl.DQNConfig(), dist=crl.QROptions(kappa=bad))
    for bad in (dict(n_quantiles=51), 51, "qr"):
        with pytest.raises(TypeError, match="QROptions"):
            crl.DQNAgent(crl.DQNConfig(), dist=bad)


@pytest.mark.parametrize("N,kappa,seed", [(2, 1.0, 1), (5, 0.25, 2), (51, 1.0, 3), (64, 0.25, 4)])
def test_dtheta_agrees_with_central_differences_of_the_loss(N, kappa, seed):
    """θ lies on multiples of 1/64 and T on odd multiples of 1/128, so every u = T_j − θ_i is an odd multiple of 1/128 and κ an even one: |u| and
    ||u| − κ| are at least 1/128 > 2h, no pair changes its branch or its indicator between θ − h and θ + h, loss_s is a quadratic in θ_i there and its
    central difference has no truncation error; θ ± h is exact. What is left is rounding. Each of the N² terms (wt·h)/κ is non-negative and carries at
    most 5 roundings (0.5·u or au − 0.5κ, the product, wt, wt·h, /κ; u and τ − 1 are exact or one more), a row sum N − 1 more, /N one, the sum over rows
    N − 1: a relative error below (2N + 6)·2^-53 on a sum of non-negative terms, i.e. below (2N + 6)·spacing(loss)/2 per evaluation. Two evaluations
    over 2h give (2N + 6)·spacing(loss)/(2h); dθ itself (a sum of N terms of mixed sign bounded by κ, two divisions) adds (N + 2)·spacing(κ)."""
    rng = np.random.default_rng(seed)
    k = 3
    theta = rng.integers(-192, 192, (N, k)) / 64.0
    T = rng.integers(-192, 192, (N, k)) / 64.0 + 1.0 / 128.0
    u = T[None] - theta[:, None]
    assert np.abs(u).min() > 2 * H and np.abs(np.abs(u) - kappa).min() > 2 * H and (np.abs(u) <= kappa).any() and (np.abs(u) > kappa).any()
    loss, G = Q.pair(theta, T, kappa)
    d = Q.dtheta(G, kappa)
    assert np.all(loss >= 0.0)
    worst = 0.0
    for i in range(N):
        e = np.zeros((N, 1)); e[i] = H
        up, dn = Q.pair(theta + e, T, kappa)[0], Q.pair(theta - e, T, kappa)[0]
        bound = (2 * N + 6) * np.spacing(np.maximum(up, dn)) / (2 * H) + (N + 2) * np.spacing(kappa)
        err = np.abs((up - dn) / (2 * H) - d[i])
        assert np.all(err <= bound), (i, err, bound)
        worst = max(worst, float((bound / np.abs(d[i]).max()).max()))
    print(f"N = {N}, kappa = {kappa}: the bound is at most {worst:.2e} of the largest |dtheta| of its row")
    assert worst < 1e-6, "the bound is sharp enough to see a wrong sign or a missing 1/N"
