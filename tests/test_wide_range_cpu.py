"""The precondition of test_gpu_wide_range.py, without a GPU: on every case of wide_range_cases.py the float32 oracle ALONE (orc_loss_grad) is
within RTOL / 2 of the float64 restatement on all twelve gradient arrays and the four loss scalars, and orc_get_action within RTOL per sample.
Only then is a miss of the HIP kernels on that case the kernels' own: a case that fails here measures the conditioning of the problem in float32
and does not belong in the table (change its inputs, not the bar). Every figure is printed (pytest -s shows them)."""
import numpy as np
import pytest

import oraclelib as O
import wide_range_cases as W
from test_gpu_fp16x2_range import LOSSES, _float64, _l2
from test_gpu_parity import RTOL, loss_close, rel_err
from test_gpu_wide import rel_err_s


def oracle_errors(case, D, A, mb):
    """(worst gradient array's relative L2 error, {loss: (oracle, float64)}, float64 gradient) of the float32 oracle on minibatch `mb`."""
    cfgo, _, params, b = W.build(case, D, A)
    g_o, so, g64, l64 = W.reference(case, D, A, mb)
    off = O.param_offsets(cfgo)
    errs = [_l2(g_o[off[i]:off[i + 1]], g64[off[i]:off[i + 1]]) for i in range(12)]
    return errs, {key: (so[key], l64[key]) for key in LOSSES}, g64


@pytest.mark.parametrize("case,D,A", [(c, D, A) for c in W.CASES for D, A in W.shapes_of(c)])
def test_oracle_meets_half_the_bar_against_float64_on_every_update_case(case, D, A):
    for mb in (0, 2):
        errs, losses, g64 = oracle_errors(case, D, A, mb)
        print(f"{case} obs {D} act {A} mb {mb}: oracle vs float64, worst gradient array {max(errs):.2e} (array {int(np.argmax(errs))}); "
              + ", ".join(f"{k} {abs(o - w) / max(abs(w), 1e-300):.1e}" for k, (o, w) in losses.items()))
        assert np.isfinite(g64).all()
        for i, e in enumerate(errs):
            assert e < RTOL / 2, (case, mb, i, e)
        for key, (o, w) in losses.items():
            assert loss_close(key, o, w, RTOL / 2), (case, mb, key, o, w)
        if case == "obs*1e6":      # every first-layer unit of every sample saturated: what the GPU test asks as exact zeros is exactly zero
            off = O.param_offsets(W.build(case, D, A)[0])
            assert not g64[off[W.A_W1]:off[W.A_W1 + 1]].any() and not g64[off[W.C_W1]:off[W.C_W1 + 1]].any()


def test_big_samples_of_the_slab_ladder_carry_no_cotangent():
    """The construction of ladder 6: the float64 gradient of a minibatch equals that of the same minibatch WITHOUT its eight big samples
    (same advantage statistics, same 1 / M) — the big samples sit one per 32-sample slab and contribute nothing, so whatever a kernel loses
    on the small samples by scaling a slab for its big one shows in full."""
    import torch
    for case in W.SLAB_LADDER:
        cfgo, _, params, b = W.build(case, 8, 4)
        off = O.param_offsets(cfgo)
        idx = b["perm"][:W.M]
        big = W.big_mask(b)[idx]
        assert big.sum() == 8 and all(big[32 * t + W.BIG_POS] for t in range(8))
        g64, _ = _float64(cfgo, params, b, idx)
        a = b["adv"][idx].astype(np.float64)
        sub = idx[~big]
        t = torch.tensor(params.astype(np.float64), requires_grad=True)
        loss = O.torch_loss(t, cfgo, off, b["obs"][:, sub], b["action"][sub], b["logprob"][sub], b["value"][sub], b["adv"][sub], b["ret"][sub],
                            adv_stats=(a.mean(), a.std(ddof=1)))[0]
        (loss * len(sub) / W.M).backward()
        errs = [_l2(g64[off[i]:off[i + 1]], t.grad.numpy()[off[i]:off[i + 1]]) for i in range(12)]
        print(f"{case}: gradient with and without the big samples differs by {max(errs):.2e} (array {int(np.argmax(errs))})")
        assert max(errs) < RTOL / 10, (case, errs)


@pytest.mark.parametrize("case,D,A", [(c, D, A) for c in W.FORWARD_CASES for D, A in W.shapes_of(c)])
def test_oracle_forward_meets_the_bar_against_float64_per_sample(case, D, A):
    """orc_get_action on the forward consumers' inputs: values and log-probabilities within RTOL of the float64 forward PER SAMPLE (rel_err /
    rel_err_s, the bar the kernels are held to: where the float32 statement of the same arithmetic misses it, a kernel's miss says nothing; a
    per-sample maximum over 128 samples of float32 rounding sits at 1e-6 … 6e-6 on plain data already, so half the bar is not asked here),
    and the same actions wherever the draw is more than 1e-6 away from a CDF knot (at most 1 % of the samples may be that close)."""
    for n in (33, W.NT * 16):
        cfgo, params, obs, u = W.forward_inputs(case, D, A, n)
        a_o, lp_o, v_o, margin = O.get_action(cfgo, params, obs, u)
        lp64, v64 = W.forward64(cfgo, params, obs)
        a64 = W.sample64(lp64, u)
        safe = margin > 1e-6
        same = a_o == a64
        e_lp, e_v = rel_err_s(lp_o[same], lp64[a64, np.arange(n)][same]), rel_err(v_o, v64)
        print(f"{case} obs {D} act {A} n {n}: oracle vs float64, logprob {e_lp:.2e} value {e_v:.2e}, {np.sum(~safe)} draws near a knot, "
              f"actions seen {sorted(set(a_o.tolist()))}")
        assert np.array_equal(a_o[safe], a64[safe]) and (~safe).sum() <= n // 100
        assert e_lp < RTOL and e_v < RTOL
