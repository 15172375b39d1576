"""The epoch shuffles and the per-minibatch advantage sums at their bucket and route edges, against tests/shuffle_ref.py and the CPU oracle.

Permutations are bit-equal: blocked Fisher–Yates to orc_shuffle_blocked_fy, serial Fisher–Yates to orc_shuffle_fy (host-driven calls shuffle what
the slot holds; crl_ppo_iterate / crl_ppo_update start from the identity), the keyed bijection to shuffle_ref.bij_forward — at every size and key of
tests/shuffle_cases.py.

Sums. Chosen advantages reach crl_ppo_update as rewards: with gamma = gae_lambda = 0, values and terminal flags 0 the fixed-mode GAE leaves A = r,
which is asserted bit for bit before anything else; lr = 0 keeps the parameters. With integer-valued advantages (|a| <= 2046) every partial sum of a and a² is an
integer below 2^53, so CRL_F_ADV_SUMS must equal the exact integer sums over the permutation READ BACK, on every route — a sample dropped, counted
twice or put into the neighbouring minibatch changes them. With Float32 advantages the device adds M exact Float64 terms in some fixed order, so
   |Σ_dev − Σ| <= γ_{M−1} · Σ|x|,   γ_k = k·u / (1 − k·u),   u = 2^-53                        (Higham, eq. 4.4 — any order)
against math.fsum (correctly rounded), for Σa and Σa²; two fresh handles must agree bit for bit.

Mean and standard deviation (adv_finish_kernel, read through update_minibatch(mb, 0.0, apply_update=False)), from the sums S1, S2 the device itself
holds, n = M >= 2 samples. mean = fl(S1 / n) is one IEEE division; rounded to Float32 it has ONE admissible value: equality is asserted. For the
deviation the kernel computes, in Float64, q = n·mean·mean (with mean's own rounding: relative error <= 4u + O(u²), and S1² / n <= S2 by
Cauchy–Schwarz, so |q − S1²/n| <= 4u·S2), d = S2 − q (one rounding, or none when it contracts to an fma: <= u·|d|), var = d / (n − 1) (u·var), clamps
at 0 and takes sqrt (u·σ). Hence |var_dev − var| <= E := (6u·S2 + 3u·(n − 1)·var) / (n − 1), the constants rounded up over the O(u²) terms, and since
|√a − √b| <= min(|a − b| / √b, √|a − b|) — the second form also covers the clamp —
   |σ_dev64 − σ| <= e64 := min(E / σ, √E) + 2u·σ,     |σ_dev32 − σ| <= e64 + 2^-24·(σ + e64) + 2^-150,
the last two terms being the half-ulp of the one Float32 rounding. E / σ is the u·S2 / ((n − 1)·σ) term: for a mean of 100 and a spread of 1 it is
7e-12, so the Float32 result is pinned to its nearest or next value; for a constant advantage every step is exact and the deviation must be 0.0.

Every test prints what it compared; test_report prints the totals (largest fraction of the bars used, sums / permutations compared and differing)."""
import math
import time
from fractions import Fraction

import numpy as np
import pytest

import oraclelib as O
import shuffle_cases as SC
import shuffle_ref as R

pytestmark = pytest.mark.gpu

TALLY = dict(perms=0, perms_differ=0, sums_exact=0, sums_exact_differ=0, sums_float=0, sums_float_over=0, sum_frac=0.0, stats=0, std_frac=0.0,
             mean_differ=0, big_seconds={})
SMALL, BIG = SC.perm_cases()


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1, "HIP library loaded but no GPU visible"
    return crl


def perm_agent(crl, nt, k, mode, seed, offset):
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 10, num_minibatches=1, update_epochs=1)
    return crl.Agent(cfg, shuffle_mode=mode, seed=seed, env_id_offset=offset)


def is_permutation(p):
    return p.min() >= 0 and p.max() < p.size and bool(np.all(np.bincount(p, minlength=p.size) == 1))


def reference_perm(mode, n, key, epoch, start=None):
    if mode == R.BLOCKED:
        return O.shuffle_blocked_fy(n, key, epoch)
    if mode == R.BIJECTION:
        return R.bij_forward(n, key, epoch).astype(np.int32)
    return O.shuffle_fy(np.arange(n, dtype=np.int32) if start is None else start.copy(), key, epoch)


def count_perm(got, want):
    TALLY["perms"] += 1
    same = np.array_equal(got, want)
    TALLY["perms_differ"] += 0 if same else 1
    return same


# ------------------------------------------------------------------------------------------------------------------ permutations
@pytest.mark.parametrize("mode,n,nt,k", SMALL, ids=[f"mode{m}-n{n}" for m, n, _, _ in SMALL])
def test_permutation_bits_at_every_size_and_key(crl, mode, n, nt, k):
    F = crl._lib
    ident = np.arange(n, dtype=np.int32)
    for seed in SC.SEEDS:
        for offset in SC.OFFSETS:
            agent = perm_agent(crl, nt, k, mode, seed, offset)
            h = agent.handle
            key = R.shuffle_seed(seed, offset)
            seen = {}
            for ep in SC.EPOCHS:
                if mode == R.SERIAL:
                    h.write(F.F_PERM, ident)
                h.shuffle(ep)
                p = h.read(F.F_PERM)
                assert count_perm(p, reference_perm(mode, n, key, ep)), (seed, offset, ep)
                assert is_permutation(p)
                if mode == R.SERIAL:                       # b_inds = shuffle(b_inds): a second call shuffles the first one's result
                    h.shuffle(ep)
                    assert count_perm(h.read(F.F_PERM), reference_perm(mode, n, key, ep, start=p)), (seed, offset, ep, "cumulative")
                    h.write(F.F_PERM, ident)
                h.shuffle(ep)
                assert np.array_equal(h.read(F.F_PERM), p), (seed, offset, ep, "the same call twice")
                seen[ep] = p
            if n >= 255:                                    # (below that two epochs may draw the same permutation by chance)
                assert not np.array_equal(seen[5], seen[(1 << 32) + 5]) and not np.array_equal(seen[0], seen[5])
            agent.close()
        if n >= 255:
            a0 = reference_perm(mode, n, R.shuffle_seed(seed, 0), 5); a3 = reference_perm(mode, n, R.shuffle_seed(seed, 3), 5)
            assert not np.array_equal(a0, a3)               # env_id_offset is part of the key
    print(f"mode {mode} n {n}: {len(SC.KEYS)} keys bit-equal")


@pytest.mark.parametrize("n,nt,k,seed,offset,epoch", BIG, ids=[f"n{c[0]}-seed{c[3] >> 32 and 'hi' or 'lo'}-off{c[4]}-ep{c[5]}" for c in BIG])
def test_blocked_permutation_bits_at_the_big_sizes(crl, n, nt, k, seed, offset, epoch):
    """2^22 − 128: the last bfy_l1_kernel<256> size at 128 steps; 2^22: the first <1024>; 2^24: the last packed size."""
    F = crl._lib
    t0 = time.time()
    agent = perm_agent(crl, nt, k, R.BLOCKED, seed, offset)
    h = agent.handle
    h.shuffle(epoch)
    p = h.read(F.F_PERM)
    assert count_perm(p, O.shuffle_blocked_fy(n, R.shuffle_seed(seed, offset), epoch))
    assert is_permutation(p)
    h.shuffle(epoch)
    assert np.array_equal(h.read(F.F_PERM), p)
    agent.close()
    dt = time.time() - t0
    TALLY["big_seconds"][n] = max(TALLY["big_seconds"].get(n, 0.0), dt)
    print(f"n {n}: {dt:.2f} s")


# ------------------------------------------------------------------------------------------------------------------ advantage sums
def adv_agent(crl, c, chosen):
    """chosen: the advantages come from the rewards (gamma = lambda = 0) and nothing learns (lr = 0)."""
    kw = dict(lr=0.0, gamma=0.0, gae_lambda=0.0) if chosen else {}
    cfg = crl.PPOConfig(num_envs=c.nt, num_steps=c.k, total_timesteps=c.nt * c.k * 1000, num_minibatches=c.nmb, update_epochs=c.epochs,
                        anneal_lr=False, **kw)
    # fixed-mode GAE: the compat mode defines the last step's advantage as 0 (ppo.jl:66), which would not hand the last rewards through
    shape = dict(gae_mode=crl._lib.GAE_FIXED) if chosen else {}
    return crl.Agent(cfg, shuffle_mode=c.mode, seed=SC.SEED, options={"adv_seq": c.seq}, **shape)


def case_perm(c, call, n):
    """The permutation the current slot must hold after call `call` of the case."""
    ep = SC.last_epoch(c, call)
    if c.mode == R.SERIAL:                                   # only through iterate / update here: identity, then one shuffle per epoch
        p = np.arange(n, dtype=np.int32)
        for e in range(call * c.epochs, call * c.epochs + c.epochs):
            p = O.shuffle_fy(p, SC.SEED, e)
        return p
    return reference_perm(c.mode, n, SC.SEED, ep)


def hot_sample(c, call, ref, n):
    """One-hot position: the first sample past the boundary inside a bucket that straddles it (blocked), else the first sample of the last minibatch."""
    M = n // c.nmb
    if c.mode == R.BLOCKED and c.how != "write_perm":
        dg = R.bfy_digits(n, SC.SEED, SC.last_epoch(c, call))
        s = R.straddlers(dg.off, M)
        if s:
            return int(ref[(dg.off[s[0]] // M + 1) * M])
    return int(ref[(c.nmb - 1) * M])


def check_sums(c, fam, adv, perm, sums):
    n = adv.size; M = n // c.nmb
    ref = R.exact_sums(adv, perm, c.nmb)
    if fam in SC.EXACT_FAMILIES:
        for mb in range(c.nmb):
            for j in (0, 1):
                TALLY["sums_exact"] += 1
                same = float(sums[mb, j]) == float(ref[mb][j]) and abs(ref[mb][j]) < 2 ** 53
                TALLY["sums_exact_differ"] += 0 if same else 1
                assert same, (SC.case_id(c), fam, mb, j, sums[mb, j], ref[mb][j])
        return 0.0
    scale = R.abs_sums(adv, perm, c.nmb)
    worst = 0.0
    for mb in range(c.nmb):
        for j in (0, 1):
            bar = R.sum_bar(M, scale[mb][j])
            frac = abs(float(sums[mb, j]) - ref[mb][j]) / bar if bar > 0 else (0.0 if sums[mb, j] == ref[mb][j] else math.inf)
            worst = max(worst, frac)
            TALLY["sums_float"] += 1; TALLY["sums_float_over"] += 1 if frac > 1 else 0
    TALLY["sum_frac"] = max(TALLY["sum_frac"], worst)
    print(f"  {fam}: largest fraction of the summation bar used {worst:.3g}")
    assert worst <= 1.0, (SC.case_id(c), fam, worst)
    return worst


def check_stats(h, c, fam, sums):
    M = h.B // c.nmb
    if M < 2:
        return
    worst = 0.0
    for mb in range(c.nmb):
        st = h.update_minibatch(mb, 0.0, apply_update=False)
        S1, S2 = float(sums[mb, 0]), float(sums[mb, 1])
        ref = R.stats_exact(Fraction(S1), Fraction(S2), M)
        TALLY["stats"] += 1
        TALLY["mean_differ"] += 0 if np.float32(st["adv_mean"]) == ref.mean32 else 1
        assert np.float32(st["adv_mean"]) == ref.mean32 and st["adv_mean"] == float(np.float32(st["adv_mean"])), (fam, mb, st["adv_mean"], ref.mean64)
        assert not math.isnan(st["adv_std"]) and not math.isnan(st["loss"]), (fam, mb, st)
        bar = R.std_bar(S2, M, ref)
        worst = max(worst, abs(st["adv_std"] - ref.std64) / bar)
        if fam == "constant":
            assert st["adv_std"] == 0.0, (mb, st["adv_std"])
    TALLY["std_frac"] = max(TALLY["std_frac"], worst)
    print(f"  {fam}: largest fraction of the deviation bar used {worst:.3g}")
    assert worst <= 1.0, (SC.case_id(c), fam, worst)


def feed(h, F, adv):
    n = adv.size
    h.write(F.F_REWARD, adv); h.write(F.F_VALUE, np.zeros(n, np.float32)); h.write(F.F_TERMINAL, np.zeros(n, np.uint8))


def run_chosen(crl, c, families, stats=True):
    """One handle of a case with chosen advantages, family after family; returns {family: sums} for the fixed-order comparison."""
    F = crl._lib
    n = c.nt * c.k
    agent = adv_agent(crl, c, chosen=True)
    h = agent.handle
    rng = np.random.default_rng(n * 31 + c.nmb)
    out = {}
    written = None
    if c.how == "shuffle" and c.slot:                        # leave the handle where an iterate with `epochs` epochs leaves it
        h.env_reset(); h.iterate(1, want_stats=False)
    if c.how == "write_perm":
        h.shuffle(SC.HOST_EPOCH); h.adv_stats()              # tables (or the bijection's key) valid for this slot ...
        written = np.random.default_rng(5).permutation(n).astype(np.int32)
        h.write(F.F_PERM, written)                           # ... and dropped
    for call, fam in enumerate(families):
        want = written if written is not None else case_perm(c, call, n)
        adv = SC.FAMILIES[fam](n, rng, hot_sample(c, call, want, n))
        if c.how == "update":
            feed(h, F, adv)
            h.update(want_stats=False)
            back = h.read(F.F_ADVANTAGE).reshape(-1, order="F")
            assert back.tobytes() == adv.tobytes(), "the GAE with gamma = lambda = 0 and zero values must hand the rewards through"
        else:
            h.write(F.F_ADVANTAGE, adv)
            if c.how == "shuffle":
                h.shuffle(SC.last_epoch(c, call))
            h.adv_stats()
        perm = h.read(F.F_PERM)
        assert count_perm(perm, want), (SC.case_id(c), fam)
        sums = h.read(F.F_ADV_SUMS).reshape(c.nmb, 2)
        check_sums(c, fam, adv, perm, sums)
        if stats:
            check_stats(h, c, fam, sums)
        out[fam] = sums.copy()
    agent.close()
    return out


def run_iterate(crl, c):
    F = crl._lib
    n = c.nt * c.k
    agent = adv_agent(crl, c, chosen=False)
    h = agent.handle
    h.env_reset(); h.iterate(1, want_stats=False)
    adv = h.read(F.F_ADVANTAGE).reshape(-1, order="F")
    perm = h.read(F.F_PERM)
    assert count_perm(perm, case_perm(c, 0, n)), SC.case_id(c)
    sums = h.read(F.F_ADV_SUMS).reshape(c.nmb, 2)
    check_sums(c, "gae", adv, perm, sums)
    agent.close()
    return adv, sums


@pytest.mark.parametrize("c", SC.ADV_CASES, ids=[SC.case_id(c) for c in SC.ADV_CASES])
def test_advantage_sums_follow_the_permutation_on_every_route(crl, c, monkeypatch):
    if c.path == "wide":
        monkeypatch.setenv("CRL_FORCE_WIDE", "1")            # the 4/2/64 net down the layer-wise path
    n = c.nt * c.k
    assert R.adv_route(c.path, c.mode, n, c.nmb, c.seq, c.how, c.slot) == c.route
    print(f"{SC.case_id(c)} -> {c.route}")
    if c.how == "iterate":                                   # the GAE's own advantages: the Float64 bar, and the fixed order
        a1, s1 = run_iterate(crl, c)
        a2, s2 = run_iterate(crl, c)
        assert a1.tobytes() == a2.tobytes() and s1.tobytes() == s2.tobytes(), "two fresh handles must give the same bits"
        return
    first = run_chosen(crl, c, SC.ORDER)
    again = run_chosen(crl, c, SC.ORDER[:2], stats=False)
    assert first["normal"].tobytes() == again["normal"].tobytes(), "two fresh handles must give the same bits"


def test_report():
    """The totals of this run (printed; the assertions above are what fails)."""
    print("shuffle edges: " + ", ".join(f"{k} = {v}" for k, v in TALLY.items()))
    assert TALLY["perms_differ"] == 0 and TALLY["sums_exact_differ"] == 0 and TALLY["sums_float_over"] == 0 and TALLY["mean_differ"] == 0
