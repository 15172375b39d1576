"""References for the GAE scan (csrc/gae.hip), numpy and the standard library only.

Arrays are (nt, k), env first: value, reward Float32, term uint8; nv (nt,) Float32 is the bootstrap value behind the last step, nd (nt,) uint8 the
done flag that gates the last step. mode 0 = compat (the last slot is defined as 0), 1 = fixed (bootstrap live). The flag that gates step t is
term[t + 1] (nd behind the buffer); ANY non-zero byte is a terminal.

serial64     the recurrence of oracle/ppo_oracle.c:orc_gae in numpy Float64, in its expression order: gl = float32(γ)·float32(λ) as a Float32
             product, delta = (r + (γ·nonterm)·v') − v, A = delta + ((gl·nonterm)·A). Returns the Float64 values BEFORE the cast to Float32.
exact        the same recurrence for one env in fractions.Fraction: Float32 inputs are dyadic rationals, so nothing rounds.
scale        S_t = m_t + c_t·S_{t+1}, m_t = |r_t| + γ·nonterm·|v_{t+1}| + |v_t|: the magnitude that the recurrence's roundings are relative to
             (|A_t| <= S_t, |delta_t| <= m_t).
segmented64  gae_kernel's affine-map composition in numpy Float64: (D, C) per segment of L steps, the fold from the last segment down, the replay.
             For CPU checks and mutants only.
bound        4·(k − t)·2^-53·S_t, derived here, not measured.

The bound (u = 2^-53, first order in u; the neglected terms are below k·u < 2e-13 of it, and S itself is summed in Float64 to the same relative accuracy).
One serial step rounds five times. With g = γ·nonterm (exact: nonterm is 0 or 1) and c = gl·nonterm (exact):
    p = fl(g·v')        error <= u·g|v'|
    s = fl(r + p)       error <= u·(|r| + g|v'|)
    d = fl(s − v)       error <= u·(|r| + g|v'| + |v|)
    q = fl(c·A')        error <= u·c|A'|
    A = fl(d + q)       error <= u·(|delta| + c|A'|) <= u·(m_t + c|A'|)
so the step adds at most l_t = u·(3|r| + 4g|v'| + 2|v|) + 2u·c|A'| <= 4u·m_t + 2u·c·S_{t+1} to the error it inherits, e_t <= c_t·e_{t+1} + l_t, and with
C(t→j) = c_t···c_{j−1} and C(t→j)·S_j <= S_t:
    e_t <= Σ_{j>=t} C(t→j)·(4u·m_j + 2u·c_j·S_{j+1}) = 4u·Σ_{j>=t} C(t→j)·S_j − 2u·Σ_{j>t} C(t→j)·S_j <= 4u·(k − t)·S_t.
The segmented kernels replay each segment with the same five roundings from a carry that was folded over the later segments. For a segment s = [T, T'):
D_s is L serial steps from a zero carry (errors l'_j with S' = S − C(·→T')·S_T' in place of S), C_s is a product of L factors (at most L − 1 roundings: the
"one rounding per step to the carry's coefficient"), and the fold fl(D_s + fl(C_s·A_T')) rounds twice, at most 2u·S_T. Against the serial steps' budget over
the same segment this saves 2u·L·C_s·S_T' in D_s, spends (L − 1)u·C_s·S_T' on C_s and 2u·S_T on the fold: at most 2u·C(t→T)·S_T more per boundary T crossed,
and the boundaries are among the j > t whose 2u·C(t→j)·S_j the last inequality above gave away. Padding steps (delta 0, c 1) round nothing. So the same bound
holds for gae_kernel and gae_seg2_kernel at every L, and any two of {kernel, serial64, segmented64} lie within 2·bound of each other.
tests/test_gae_cpu.py measures how much of the bound the references use against `exact` (profiles/gae_edges.json: under a tenth)."""
from fractions import Fraction

import numpy as np

U53 = 2.0 ** -53
MUTANTS = ("flag_and_1", "pair_first_byte", "no_fold", "boundary_value_0", "compat_last_live", "no_next_done")
SEGMENTED_ONLY = ("no_fold", "boundary_value_0")


def coeffs(gamma, lam):
    """(γ, γλ) as the kernels see them: Float32 γ, and the Float32 product of Float32 γ and λ."""
    g32, l32 = np.float32(gamma), np.float32(lam)
    return float(g32), float(np.float32(g32 * l32))


def _flags(term, nd, mutant):
    """(nt, k) 0 / 1: the flag that gates step t."""
    f = np.concatenate([np.asarray(term, np.uint8)[:, 1:], np.asarray(nd, np.uint8)[:, None]], axis=1)
    if mutant == "no_next_done":
        f[:, -1] = 0
    if mutant == "pair_first_byte":
        n2 = f.shape[0] // 2
        f[1:2 * n2:2] = f[0:2 * n2:2]
    if mutant == "flag_and_1":
        return (f & 1).astype(np.float64)
    return (f != 0).astype(np.float64)


def terms(value, reward, term, nv, nd, gamma, lam, mode, mutant=None, L=0):
    """delta_t, c_t, m_t as (nt, k) Float64, in orc_gae's expression order. L is the segment length (only the boundary_value_0 mutant reads it)."""
    g, gl = coeffs(gamma, lam)
    v = np.asarray(value, np.float32).astype(np.float64); r = np.asarray(reward, np.float32).astype(np.float64)
    k = v.shape[1]
    vn = np.concatenate([v[:, 1:], np.asarray(nv, np.float32).astype(np.float64)[:, None]], axis=1)
    if mutant == "boundary_value_0" and L:
        vn[:, L - 1:k - 1:L] = 0.0
    nonterm = 1.0 - _flags(term, nd, mutant)
    gn = g * nonterm
    delta = (r + gn * vn) - v
    c = gl * nonterm
    m = np.abs(r) + gn * np.abs(vn) + np.abs(v)
    if mode == 0 and mutant != "compat_last_live":
        delta[:, -1] = 0.0; c[:, -1] = 0.0; m[:, -1] = 0.0
    return delta, c, m


def serial64(value, reward, term, nv, nd, gamma, lam, mode, mutant=None):
    delta, c, _ = terms(value, reward, term, nv, nd, gamma, lam, mode, None if mutant in SEGMENTED_ONLY else mutant)
    out = np.empty_like(delta)
    A = np.zeros(delta.shape[0])
    for t in range(delta.shape[1] - 1, -1, -1):
        A = delta[:, t] + (c[:, t] * A)
        out[:, t] = A
    return out


def scale(value, reward, term, nv, nd, gamma, lam, mode):
    _, c, m = terms(value, reward, term, nv, nd, gamma, lam, mode)
    out = np.empty_like(m)
    S = np.zeros(m.shape[0])
    for t in range(m.shape[1] - 1, -1, -1):
        S = m[:, t] + c[:, t] * S
        out[:, t] = S
    return out


def bound(value, reward, term, nv, nd, gamma, lam, mode):
    """(nt, k) Float64: 4·(k − t)·2^-53·S_t."""
    S = scale(value, reward, term, nv, nd, gamma, lam, mode)
    k = S.shape[1]
    return 4.0 * U53 * (k - np.arange(k))[None, :] * S


def segmented64(value, reward, term, nv, nd, gamma, lam, mode, L, mutant=None):
    delta, c, _ = terms(value, reward, term, nv, nd, gamma, lam, mode, mutant, L)
    nt, k = delta.shape
    S = (k + L - 1) // L
    pad = S * L - k
    if pad:                                                     # padding steps are the identity map
        delta = np.concatenate([delta, np.zeros((nt, pad))], axis=1); c = np.concatenate([c, np.ones((nt, pad))], axis=1)
    d3 = delta.reshape(nt, S, L); c3 = c.reshape(nt, S, L)
    D = np.zeros((nt, S)); C = np.ones((nt, S))
    for i in range(L - 1, -1, -1):
        D = d3[:, :, i] + c3[:, :, i] * D
        C = c3[:, :, i] * C
    carry = np.zeros((nt, S))                                   # carry[:, s]: what segment s starts its replay from
    if mutant != "no_fold":
        for s in range(S - 1, 0, -1):
            carry[:, s - 1] = D[:, s] + C[:, s] * carry[:, s]
    out = np.empty((nt, S, L))
    A = carry
    for i in range(L - 1, -1, -1):
        A = d3[:, :, i] + (c3[:, :, i] * A)
        out[:, :, i] = A
    return out.reshape(nt, S * L)[:, :k]


def exact(value, reward, term, nv, nd, gamma, lam, mode):
    """One env (1-D value / reward / term, scalar nv / nd): the k advantages as Fractions."""
    g, gl = (Fraction(x) for x in coeffs(gamma, lam))
    v = [Fraction(float(x)) for x in np.asarray(value, np.float32)] + [Fraction(float(np.float32(nv)))]
    r = [Fraction(float(x)) for x in np.asarray(reward, np.float32)]
    f = [int(x) for x in np.asarray(term, np.uint8)][1:] + [int(nd)]
    k = len(r)
    out = [Fraction(0)] * k
    A = Fraction(0)
    for t in range(k - 1 if mode else k - 2, -1, -1):
        if f[t]:
            A = r[t] - v[t]
        else:
            A = r[t] + g * v[t + 1] - v[t] + gl * A
        out[t] = A
    return out


def _ordered(x32):
    """Float32 → int64, monotone in the value (−0.0 and +0.0 both map to 0): adjacent floats are adjacent integers."""
    b = np.asarray(x32, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def rn32(x):
    """Round-to-nearest-even Float32 of a Fraction, exactly (float(Fraction) is correctly rounded to Float64; the second rounding is redone here)."""
    y = np.float32(float(x))
    best, best_d = y, abs(Fraction(float(y)) - x)
    for cand in (np.nextafter(y, np.float32(-np.inf)), np.nextafter(y, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        d = abs(Fraction(float(cand)) - x)
        if d < best_d or (d == best_d and (int(cand.view(np.int32)) & 1) == 0 and (int(best.view(np.int32)) & 1) == 1):
            best, best_d = cand, d
    return best


def interval_exact(x, b):
    """[RN32(x − b), RN32(x + b)] for a list of Fractions x and Float64 bounds b, as two Float32 arrays."""
    lo = np.array([rn32(xi - Fraction(float(bi))) for xi, bi in zip(x, b)], np.float32)
    hi = np.array([rn32(xi + Fraction(float(bi))) for xi, bi in zip(x, b)], np.float32)
    return lo, hi


def interval64(x64, b, factor=2.0):
    """[RN32(x − factor·b), RN32(x + factor·b)] around a Float64 reference (x ∓ factor·b is itself a Float64 sum: a rounding of 2^-53·|x|, against a bound of which the references use under a tenth)."""
    with np.errstate(over="ignore"):
        return (x64 - factor * b).astype(np.float32), (x64 + factor * b).astype(np.float32)


def outside(adv32, lo, hi):
    """Boolean mask: adv32 not in [lo, hi] (−0.0 equals +0.0; anything non-finite is outside)."""
    a = np.asarray(adv32, np.float32)
    return ~((a >= lo) & (a <= hi))


def width(lo, hi):
    """How many adjacent Float32 values [lo, hi] holds."""
    return _ordered(hi) - _ordered(lo) + 1
