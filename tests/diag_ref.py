"""Float64 numpy restatement of crl_ppo_diagnose's definitions (include/cleanrl_hip.h) and the tolerances a device result is held to.

The inputs are per-sample quantities of the CPU oracle (tests/oraclelib.py: logprob_actions for lp_new and the entropy elements, get_action(...,
with_value=True) for v_new) next to the buffer fields the device read; nothing the library computed goes in.

Tolerances. The project's per-value bar is eps(x) = 1e-5 |x| + 1e-6 (tests/test_gpu_parity.py): a device lp_new, entropy element or v_new may sit
that far from the oracle's. Propagated to the report:
  old_approx_kl           -mean(lp_new - lp_old): mean eps(lp_new)
  approx_kl               kl = (ratio - 1) - r, d kl / d r = ratio - 1: 2 mean(|ratio - 1| eps(lp_new)), the first-order bound doubled for the second-order term
  entropy                 mean over the samples of sum_a eps(entropy element)
  n_clipped               a sample is undecided when | |ratio - 1| - clip | <= 2 ratio eps(lp_new) (d ratio = ratio d r, doubled); the count may differ by the
                          number of undecided samples
  explained_variance_new  EV = 1 - Vn / Vr, Vn = mean(e^2) - mean(e)^2, e = ret - v_new: |dVn| <= mean(2 |e - mean(e)| eps(v_new)), |dEV| = |dVn| / Vr
  explained_variance, sum_ret, sum_ret2, sum_res_old, sum_res_old2
                          device and reference read the same Float32 inputs, so only the order of the Float64 additions differs: 1e-10 relative on the sums
                          (against the sum of the magnitudes, which is what bounds a reordering error), 1e-7 absolute on the explained variance
"""
import numpy as np


def eps(x):
    return 1e-5 * np.abs(np.asarray(x, np.float64)) + 1e-6


def _ev(sum_ret, sum_ret2, sum_res, sum_res2, n):
    m_ret = sum_ret / n
    var_ret = sum_ret2 / n - m_ret * m_ret
    m = sum_res / n
    var = sum_res2 / n - m * m
    return 1.0 - var / var_ret if var_ret > 0.0 else float("nan")


def derived(d):
    """the derived fields from the raw sums of a report (dict), by the header's formulas — the device's report must satisfy them exactly"""
    n = float(d["n"])
    return dict(old_approx_kl=-d["sum_logratio"] / n, approx_kl=d["sum_kl"] / n, clipfrac=float(d["n_clipped"]) / n, entropy=d["sum_entropy"] / n,
                explained_variance=_ev(d["sum_ret"], d["sum_ret2"], d["sum_res_old"], d["sum_res_old2"], n),
                explained_variance_new=_ev(d["sum_ret"], d["sum_ret2"], d["sum_res_new"], d["sum_res_new2"], n))


def diag_ref(lp_new, ent_elems, v_new, lp_old, value, ret, clip_coef):
    """lp_new, v_new, lp_old, value, ret: (B,) float32 in flat buffer order; ent_elems: (n_act, B) float32. Returns (report, tolerances)."""
    lp_new = np.asarray(lp_new, np.float32).ravel(order="F"); lp_old = np.asarray(lp_old, np.float32).ravel(order="F")
    v_new = np.asarray(v_new, np.float32).ravel(order="F").astype(np.float64)
    value = np.asarray(value, np.float32).ravel(order="F").astype(np.float64); ret = np.asarray(ret, np.float32).ravel(order="F").astype(np.float64)
    ent_elems = np.asarray(ent_elems, np.float32)
    n = lp_new.size
    r = (lp_new - lp_old).astype(np.float64)                   # the Float32 difference of ppo.jl:224, Float64 from here on
    ratio = np.exp(r)
    kl = (ratio - 1.0) - r
    clip = float(np.float32(clip_coef))
    clipped = np.abs(ratio - 1.0) > clip
    H = ent_elems.astype(np.float64).sum(axis=0)
    eo, en = ret - value, ret - v_new
    d = dict(n=n, n_clipped=int(clipped.sum()), sum_logratio=float(r.sum()), sum_kl=float(kl.sum()), sum_entropy=float(H.sum()),
             ratio_min=float(ratio.min()), ratio_max=float(ratio.max()), sum_ret=float(ret.sum()), sum_ret2=float((ret * ret).sum()),
             sum_res_old=float(eo.sum()), sum_res_old2=float((eo * eo).sum()), sum_res_new=float(en.sum()), sum_res_new2=float((en * en).sum()))
    d.update(derived(d))

    e_lp = eps(lp_new)
    var_ret = d["sum_ret2"] / n - (d["sum_ret"] / n) ** 2
    tol = dict(
        old_approx_kl=float(e_lp.mean()),
        approx_kl=float(2.0 * (np.abs(ratio - 1.0) * e_lp).mean()),
        entropy=float(eps(ent_elems).sum(axis=0).mean()),
        undecided=int((np.abs(np.abs(ratio - 1.0) - clip) <= 2.0 * ratio * e_lp).sum()),
        explained_variance_new=float((2.0 * np.abs(en - en.mean()) * eps(v_new)).mean() / var_ret) if var_ret > 0.0 else float("nan"),
        explained_variance=1e-7,
        sum_ret=1e-10 * float(np.abs(ret).sum()), sum_ret2=1e-10 * d["sum_ret2"],
        sum_res_old=1e-10 * float(np.abs(eo).sum()), sum_res_old2=1e-10 * d["sum_res_old2"],
    )
    return d, tol
