"""No GPU: tests/shuffle_ref.py against the CPU oracle and against itself, tests/shuffle_cases.py against its purposes, the uniformity of both exact
shuffles, the mutants of the restatement, and the recorded kernel trace (profiles/shuffle_route_trace.json) against shuffle_ref.adv_route."""
import itertools
import math
import re
from collections import Counter

import numpy as np
import pytest
from scipy.stats import chi2

import oraclelib as O
import shuffle_cases as SC
import shuffle_ref as R

HI_SEED = SC.SEEDS[1]
KEYS3 = [(99, 0), (99, 5), (HI_SEED, (1 << 32) + 5)]
TABLE_SIZES = sorted(set(SC.SIZES_ALL) | set(SC.SIZES_BLOCKED))


def test_shuffle_seed_wraps_at_64_bits():
    assert R.shuffle_seed(99, 0) == 99
    assert R.shuffle_seed(99, 3) == (99 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64 and R.shuffle_seed(99, 3) < 99 + 3 * 0x9E3779B97F4A7C15
    assert R.shuffle_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C15 - 1
    assert R.shuffle_seed(5, -1) == (5 + 0xFFFFFFFF * 0x9E3779B97F4A7C15) % 2 ** 64       # the offset is taken as a uint32


def test_inv_odd_inverts_every_kind_of_odd_word():
    for a in [1, 3, 0xFFFFFFFF, 0x9E3779B1, 0x80000001] + [int(x) | 1 for x in np.random.default_rng(0).integers(0, 2 ** 32, 200)]:
        assert (a * R.inv_odd(a)) & R.M32 == 1
    assert R.inv_odd(0x9E3779B1) == 0x0E8B2F51                                             # the constant bij_round_inv carries


@pytest.mark.parametrize("seed,epoch", KEYS3)
def test_bijection_is_a_permutation_and_its_inverse_undoes_it(seed, epoch):
    longest = 0
    for n in list(range(1, 301)) + TABLE_SIZES + [(1 << 20) + 1]:
        f, rounds = R.bij_forward(n, seed, epoch, want_rounds=True)
        longest = max(longest, rounds)
        assert np.array_equal(np.sort(f), np.arange(n)), n
        assert np.array_equal(R.bij_inverse(n, seed, epoch, f), np.arange(n)), n
        if n <= 300:                                                                       # and the inverse of an arbitrary subset, not of the whole range
            assert np.array_equal(R.bij_forward(n, seed, epoch, R.bij_inverse(n, seed, epoch, np.arange(n)[::3])), np.arange(n)[::3])
    assert longest < 64


def test_bijection_key_takes_both_halves_of_seed_and_epoch():
    n = 4097
    base = R.bij_forward(n, 99, 5)
    for seed, epoch in ((99, (1 << 32) + 5), (99 + (1 << 32), 5), (100, 5), (99, 6)):
        assert not np.array_equal(base, R.bij_forward(n, seed, epoch))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9, 257, 4097, 8193, 12289, 16385])
def test_restated_shuffles_equal_the_oracle(n):
    for seed, epoch in KEYS3:
        assert np.array_equal(R.blocked_fy(n, seed, epoch), O.shuffle_blocked_fy(n, seed, epoch))
        start = np.random.default_rng(n).permutation(n).astype(np.int32)
        assert np.array_equal(R.fy_serial(start, seed, epoch), O.shuffle_fy(start, seed, epoch))


@pytest.mark.parametrize("n", [4097, 8193, 12289, 16385, 65537])
def test_digits_rebuild_the_oracles_bucket_layout(n):
    """Every L1 bucket's position range holds exactly the samples with that first digit."""
    for seed, epoch in KEYS3:
        dg = R.bfy_digits(n, seed, epoch)
        perm = O.shuffle_blocked_fy(n, seed, epoch)
        assert dg.K1 > 1 and dg.off[-1] == n
        for b, (lo, hi) in enumerate(dg.ranges):
            assert np.array_equal(np.sort(perm[lo:hi]), np.nonzero(dg.d1 == b)[0]), (n, b)
        assert max(hi - lo for lo, hi in dg.ranges) <= R.BFY_CAP


def chi2_uniform(shuffle, n, epochs):
    perms = list(itertools.permutations(range(n)))
    c = Counter(tuple(int(v) for v in shuffle(ep)) for ep in range(epochs))
    assert set(c) <= set(perms)
    want = epochs / len(perms)
    return sum((c.get(p, 0) - want) ** 2 / want for p in perms)


@pytest.mark.parametrize("n", [3, 4])
def test_both_exact_shuffles_are_uniform_over_s_n(n):
    """χ² of 1000·n! epochs (seed 99) against the uniform law on S_n, held to the 1 − 10^-6 quantile of χ²(n! − 1): a fixed-seed computation.
    The device is bit-equal to the oracle (tests/test_gpu_shuffle_edges.py), so this is the device's law too."""
    nf = math.factorial(n)
    bar = chi2.ppf(1 - 1e-6, nf - 1)
    fy = chi2_uniform(lambda ep: O.shuffle_fy(np.arange(n, dtype=np.int32), 99, ep), n, 1000 * nf)
    bf = chi2_uniform(lambda ep: O.shuffle_blocked_fy(n, 99, ep), n, 1000 * nf)
    print(f"chi2 n = {n}: serial {fy:.2f}, blocked {bf:.2f}, bar {bar:.2f} ({nf - 1} degrees of freedom)")
    assert fy < bar and bf < bar
    if n == 4:
        assert abs(bar - 70.5) < 0.5


# ---------------------------------------------------------------------------------------------------------------- the case table
def test_every_route_is_reached_and_named():
    got = Counter()
    for c in SC.ADV_CASES:
        r = R.adv_route(c.path, c.mode, c.nt * c.k, c.nmb, c.seq, c.how, c.slot)
        assert r in R.ROUTES and r == c.route, (SC.case_id(c), r, c.route)
        got[r] += 1
    # bucket<4|8>/stored-scalar cannot exist (n % nmb == 0); the recomputed branch is one loop for every NMB
    reachable = R.ROUTES - {"bucket<4>/stored-scalar", "bucket<8>/stored-scalar"}
    need = {r for r in reachable if not r.endswith("recomputed")} | {"bucket<2>/recomputed"}
    assert need <= set(got), need - set(got)
    assert len({SC.case_id(c) for c in SC.ADV_CASES}) == len(SC.ADV_CASES)
    for c in SC.ADV_CASES:
        assert (c.nt * c.k) % c.nmb == 0 and c.k <= 1024


def test_route_rule_at_its_thresholds():
    A = R.adv_route
    assert A("wide", 2, 11264, 2, 1, "update") == R.LEAF and A("wide", 2, 11262, 2, 1, "update") == R.SUMS
    assert A("wide", 2, 11264, 2, 1, "shuffle") == R.SUMS and A("wide", 1, 1024, 4, 1, "shuffle") == R.INV4
    assert A("wide", 1, 1024, 4, 1, "write_perm") == R.SUMS and A("wide", 1, 1024, 8, 1, "update") == R.SUMS
    assert A("fused", 2, 1024, 4, 1, "shuffle", slot=1) == R.GATHER and A("fused", 2, 1024, 4, 1, "iterate") == "bucket<4>/stored-vec"
    assert A("fused", 2, 4096 * 256, 256, 1, "update") == R.GATHER and A("fused", 2, 1024, 4, 0, "update") == R.GATHER


def test_sizes_cover_the_named_edges():
    small, big = SC.perm_cases()
    for mode, n, nt, k in small:
        assert nt * k == n and k <= 1024
    for n in (4096, 4097, 8192, 8193, 16384, 16385):
        assert R.bfy_k1(n) == {4096: 1, 4097: 2, 8192: 2, 8193: 4, 16384: 4, 16385: 8}[n]
    assert [c[0] for c in big[::len(SC.KEYS)]] == [(1 << 22) - 128, 1 << 22, 1 << 24] and all(c[1] * c[2] == c[0] for c in big)
    assert any(s >> 32 for s in SC.SEEDS) and any(e >> 32 for e in SC.EPOCHS) and 3 in SC.OFFSETS


def test_straddling_cases_straddle():
    """A condition on the inputs: a case listed as straddling has a bucket across a minibatch boundary at the epoch its first call reads back — and
    one that is not, where there is more than one bucket — so both branches of the per-bucket table are taken."""
    seen = {}
    for c in SC.ADV_CASES:
        if c.mode != R.BLOCKED or c.straddle is None:
            continue
        s, span, buckets = SC.straddle_count(c)
        seen[(c.nt * c.k, c.nmb, SC.last_epoch(c))] = (s, buckets)
        assert s >= 1, SC.case_id(c)
        if c.straddle == "mixed":
            assert buckets == 1 or s < buckets, SC.case_id(c)
        else:
            assert s == buckets and span >= 3, SC.case_id(c)
    # the counts at seed 99, epoch 0
    for key, want in {(1024, 4, 0): (1, 1), (8194, 2, 0): (1, 4), (11264, 2, 0): (1, 4), (16896, 3, 0): (2, 8), (16384, 8, 0): (4, 4), (49152, 16, 0): (15, 16)}.items():
        assert seen[key] == want, (key, seen[key])


def test_integer_family_stays_exact():
    a = SC.adv_integers(1 << 24).astype(np.float64)
    assert np.all(a == np.rint(a)) and np.abs(a).max() <= 2046 and np.abs(a).sum() < 2 ** 53 and (a * a).sum() < 2 ** 53
    assert len(np.unique(a[:4093])) == 4093


def test_stats_exact_and_its_bars():
    st = R.stats_exact(10, 30, 4)                         # 1, 2, 3, 4
    assert st.mean == 2.5 and abs(st.std64 - math.sqrt(5 / 3)) < 1e-15 and st.std32 == np.float32(math.sqrt(5 / 3))
    st = R.stats_exact(25, 62.5, 10)                      # ten times 2.5: the variance is exactly 0
    assert st.var == 0 and st.std64 == 0.0
    assert R.stats_exact(10, 9.999, 10).var == 0          # S2 below S1² / n (sums that carry rounding): the clamp
    assert 5.9e-8 < R.std_bar(62.5, 10, R.stats_exact(25, 63.5, 10)) / R.stats_exact(25, 63.5, 10).std64 < 6.1e-8   # one Float32 half-ulp, relative
    assert abs(R.sum_bar(1025, 1.0) - 1024 * 2.0 ** -53) < 1e-25


# ---------------------------------------------------------------------------------------------------------------- mutants
def test_mutant_bijection_without_cycle_walking_is_no_permutation():
    bad = [n for n in range(1, 301) if not np.array_equal(np.sort(R.bij_forward(n, 99, 0, mutant="mod_n")), np.arange(n))]
    assert len(bad) > 200 and all(n & (n - 1) for n in bad)            # only powers of two survive


def test_mutant_inverse_with_exchanged_round_keys_does_not_invert():
    for n in (257, 4097):
        f = R.bij_forward(n, 99, 0)
        assert not np.array_equal(R.bij_inverse(n, 99, 0, f, mutant="swap_round_keys"), np.arange(n))


def test_mutant_fisher_yates_drawing_below_i_is_caught():
    assert not np.array_equal(R.fy_serial(np.arange(257), 99, 0, mutant="draw_below_i"), O.shuffle_fy(np.arange(257, dtype=np.int32), 99, 0))
    x2 = chi2_uniform(lambda ep: R.fy_serial(np.arange(3), 99, ep, mutant="draw_below_i"), 3, 6000)
    assert x2 > chi2.ppf(1 - 1e-6, 5)                                    # Sattolo's algorithm: the two 3-cycles only


@pytest.mark.parametrize("mutant", ["unsorted", "swap_digits"])
def test_mutant_blocked_shuffles_are_caught(mutant):
    n = 8193
    assert not np.array_equal(R.blocked_fy(n, 99, 0, mutant=mutant), O.shuffle_blocked_fy(n, 99, 0))
    if mutant == "swap_digits":                                          # and by the layout check that owns it
        dg = R.bfy_digits(n, 99, 0, mutant=mutant)
        perm = O.shuffle_blocked_fy(n, 99, 0)
        assert any(not np.array_equal(np.sort(perm[lo:hi]), np.nonzero(dg.d1 == b)[0]) for b, (lo, hi) in enumerate(dg.ranges))


def test_mutant_straddling_bucket_in_one_minibatch_changes_every_straddling_case():
    for c in SC.ADV_CASES:
        if c.mode != R.BLOCKED or c.straddle is None:
            continue
        n = c.nt * c.k
        ep = SC.last_epoch(c)
        perm = O.shuffle_blocked_fy(n, SC.SEED, ep)
        adv = SC.adv_integers(n)
        bad = R.minibatch_of(perm, n // c.nmb, off=R.bfy_digits(n, SC.SEED, ep).off, mutant="straddle_first")
        assert R.exact_sums(adv, perm, c.nmb) != R.exact_sums(adv, perm, c.nmb, mb=bad), SC.case_id(c)


# ---------------------------------------------------------------------------------------------------------------- the recorded trace
NEEDED = ["bfy_l1_kernel<256>", "bfy_l1_kernel<1024>", "bfy_leaf_kernel", "adv_bucket_sums_kernel<1>", "adv_bucket_sums_kernel<2>", "adv_bucket_sums_kernel<4>",
          "adv_bucket_sums_kernel<8>", "adv_gather_sums_kernel", "adv_sums_kernel", "adv_sums_inv_kernel<4>"]


def test_recorded_kernel_trace_agrees_with_the_route_rule():
    """scripts/shuffle_route_trace.py ran the advantage-sum cases once under a kernel trace and wrote, per case, the shuffle and advantage kernels of the
    call that produced the sums. Each must be what adv_route names, and together they must name every kernel of the family."""
    tr = SC.load_trace()
    assert set(tr["cases"]) == {SC.case_id(c) for c in SC.ADV_CASES}
    names = set(tr["big"]["kernels"])
    for c in SC.ADV_CASES:
        rec = tr["cases"][SC.case_id(c)]
        route = R.adv_route(c.path, c.mode, c.nt * c.k, c.nmb, c.seq, c.how, c.slot)
        assert rec["route"] == route
        adv = [k for k in rec["kernels"] if re.match(r"adv_(bucket_sums|gather_sums|sums|sums_inv)_kernel", k)]
        if route == R.LEAF:
            assert adv == [] and "bfy_leaf_kernel" in rec["kernels"], (SC.case_id(c), rec["kernels"])
        else:
            assert adv == [R.ROUTE_KERNEL[route]], (SC.case_id(c), rec["kernels"])
        shuffled = {R.BLOCKED: "bfy_leaf_kernel", R.SERIAL: "fy_serial_kernel", R.BIJECTION: "bijection_kernel"}[c.mode]
        assert c.how == "write_perm" or shuffled in rec["kernels"], (SC.case_id(c), rec["kernels"])
        names |= set(rec["kernels"])
    assert set(NEEDED) <= names, set(NEEDED) - names
