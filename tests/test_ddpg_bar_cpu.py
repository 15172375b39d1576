"""The yardstick of the DDPG parity bars, without a GPU: profiles/ddpg_bar.json (scripts/ddpg_bar.py) is reproduced exactly for the two cheapest
cases of tests/ddpg_bar.py's table — the jitter is seeded —, the two conditions the table has to meet hold over the whole file (every parameter
floor exactly 0.0; every applicable mutant at least 10 bars away on some observable in every case), and the bars follow their formulas."""
import json

import numpy as np
import pytest

import ddpg_bar as B
import ddpg_ref as R


@pytest.fixture(scope="module")
def prof():
    return json.load(open(B.BAR_JSON))


@pytest.mark.parametrize("name", B.CHEAPEST)
def test_floor_and_mutants_reproduce_the_committed_profile(prof, name):
    got = B.measure(B.CASE[name])
    rec = prof["cases"][name]
    assert got["floor"] == rec["floor"]
    assert got["mutants"] == rec["mutants"]
    assert {m: B.mutant_ratio(d, prof["loss_bar"]) for m, d in got["mutants"].items()} == rec["mutant_ratio"]


def test_the_profile_covers_the_table_and_every_applicable_mutant(prof):
    assert list(prof["cases"]) == sorted(c["name"] for c in B.CASES)
    for c in B.CASES:
        rec = prof["cases"][c["name"]]
        assert sorted(rec["mutants"]) == sorted(rec["mutant_ratio"]) == sorted(B.applicable(c)), c["name"]
        assert set(rec["floor"]) == set(B.OBSERVABLES) and all(set(d) == set(B.OBSERVABLES) for d in rec["mutants"].values())
        d = B.case_cfg(c)
        assert (rec["D"], rec["A"], rec["batch_size"], rec["updates"]) == (c["D"], c["A"], d["batch_size"], c["T"] - B.threshold(d))
    # which mutant is left out where, and why: the line it breaks is switched off there
    left_out = {c["name"]: sorted(set(B.MUTANTS) - set(B.applicable(c)), key=lambda m: int(m[1:])) for c in B.CASES}
    assert left_out["d64a16_k61"] == ["M10"] and left_out["ni64_k30"] == ["M4", "M10"] and left_out["ring200_k199"] == ["M4"]
    assert left_out["kmax_ring_eq_batch"] == ["M3", "M4", "M5", "M10"]          # A = 1; NI = 4; k = n: a wrong counter only reorders the sums
    assert left_out["gamma0"] == left_out["none_terminal"] == ["M1", "M3", "M4", "M5", "M10"]
    assert left_out["noise0"] == ["M3", "M4", "M5", "M9", "M10"]
    assert all(left_out[n] == ["M3", "M4", "M5", "M10"] for n in ("d1a1_k2", "k120_default", "tau1", "all_terminal", "logfreq7"))
    assert sorted(prof["mutants"]) == sorted(B.MUTANTS) and all(prof["mutants"][m]["cases"] >= 1 for m in B.MUTANTS)


def test_every_parameter_floor_is_exactly_zero(prof):
    for name, rec in prof["cases"].items():
        for o in B.PARAMS:
            assert rec["floor"][o] == 0.0, (name, o)
        # the twin IS jittered, in the last bits (with gamma = 0 or terminal data alone the critic loss meets no transcendental function)
        assert 0.0 < rec["floor"]["actor_loss"] < 1e-14 and 0.0 <= rec["floor"]["critic_loss"] < 1e-14, name
        assert (rec["floor"]["critic_loss"] == 0.0) == (name in ("gamma0", "all_terminal")), name


def test_every_mutant_is_ten_bars_away_in_every_case_it_applies_to(prof):
    assert prof["mutant_factor"] == B.MUTANT_FACTOR == 10
    for name, rec in prof["cases"].items():
        for m, dist in rec["mutants"].items():
            ratio = max(dist[o] / (prof["loss_bar"] if o in B.LOSSES else prof["param_bar"]) for o in B.OBSERVABLES)
            assert ratio == rec["mutant_ratio"][m] and ratio >= 10, (name, m, ratio)
    for m, rec in prof["mutants"].items():
        ratios = {n: c["mutant_ratio"][m] for n, c in prof["cases"].items() if m in c["mutant_ratio"]}
        assert rec["worst_ratio"] == min(ratios.values()) == ratios[rec["worst_case"]] and rec["cases"] == len(ratios), m


def test_the_bars_follow_their_formulas(prof):
    floor = max(rec["floor"][o] for rec in prof["cases"].values() for o in B.LOSSES)
    assert prof["loss_floor"] == floor and prof["loss_factor"] == B.LOSS_FACTOR == 32
    assert prof["loss_bar"] == 32 * floor
    assert prof["param_bar"] == B.PARAM_BAR == 2.0 ** -21 == 4 * float(np.spacing(np.float32(1.0)))
    assert prof["jitter_ulp"] == {"exp": 2, "log": 2, "cos": 2} and prof["jitter_seeds"] == [1, 2, 3]
    assert B.load_bars() == (prof["loss_bar"], prof["param_bar"])
    assert prof["loss_bar"] < 1e-12 < B.PARAM_BAR < B.OLD_BAR


def test_the_jitter_moves_results_by_whole_ulps_within_its_amplitude():
    x = np.linspace(-3.0, 3.0, 4001)
    j = B.JitterNumpy(5)
    for name, arg in (("exp", x), ("cos", x), ("log", np.exp(x))):
        y = getattr(np, name)(arg)
        steps = (getattr(j, name)(arg) - y) / np.spacing(np.abs(y))
        assert set(np.unique(steps)) == {-2.0, -1.0, 0.0, 1.0, 2.0}              # whole ulps of the unjittered result, every amplitude drawn
    assert j.sqrt is np.sqrt and np.array_equal(j.exp(np.array([np.inf, -np.inf])), [np.inf, 0.0])
    with B.jitter(1):
        assert isinstance(R.np, B.JitterNumpy)
    assert R.np is np


def test_mutants_leave_the_reference_as_it_was():
    before = {n: getattr(R, n) for n in ("td_target", "critic_loss_grad", "actor_loss_grad", "normal", "_sum_samples", "polyak", "sample_indices")}
    step = R.Adam.step
    for m, (_, _, make) in B.MUTANTS.items():
        with B.patched(**make()):
            assert any(getattr(R, n) is not f for n, f in before.items()), m
        assert all(getattr(R, n) is f for n, f in before.items()) and R.Adam.step is step, m


@pytest.mark.parametrize("n,k", [(50, 50), (200, 200), (200, 199), (1024, 1024), (1000, 7)])
def test_candidates_needed_counts_what_the_draw_looks_at(n, k):
    seed, gstep = 0x5EED, 207
    need = B.candidates_needed(seed, gstep, n, k)
    idx = R.sample_indices(seed, gstep, n, k)
    x = R.philox(np.arange(need), gstep, 0, R.S_SAMPLE, seed & R.M32, seed >> 32)[0]
    slots = ((x * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    assert len(set(slots.tolist())) == k and len(set(slots[:-1].tolist())) == k - 1 and slots[-1] == idx[-1]
    assert need >= k and (k == 1 or B.candidates_needed(seed, gstep, n, k - 1) < need)


def test_the_multi_round_cases_need_more_than_one_round(prof):
    for name in B.MULTI_ROUND:
        worst = max(B.case_candidates(B.CASE[name]))
        assert worst > 1024 and worst == prof["cases"][name]["candidates_max"], name
    assert all(max(B.case_candidates(c)) <= 1024 for c in B.CASES if c["name"] not in B.MULTI_ROUND and B.case_cfg(c)["batch_size"] <= 31)
