"""The yardstick of the A2C parity bars, without a GPU: tests/a2c_ref.py agrees with the C oracle within the bars on every case of tests/a2c_bar.py's
table, the table's batch sizes are the ones it names and cover the edges of csrc/a2c.hip's kernels, profiles/a2c_bar.json (scripts/a2c_bar.py) is
reproduced exactly for the two cheapest cases — the jitter is seeded —, every applicable mutant is at least 10 bars away on some observable in every
case, and the bars follow their formulas."""
import json

import numpy as np
import pytest

import a2c_bar as B
import a2c_ref as R
import oraclelib as O


@pytest.fixture(scope="module")
def prof():
    return json.load(open(B.BAR_JSON))


@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_twin_agrees_with_the_oracle_within_the_bars(prof, name):
    case = B.CASE[name]
    calls, updates = B.oracle_run(name)
    assert B.n_matches(case, updates) and [u["n"] for u in updates] == prof["cases"][name]["n"]
    out = B.distances(B.run_twin(case), updates)
    assert out == prof["cases"][name]["oracle_to_twin"]
    for k in B.OBSERVABLES:
        assert out[k] <= B.bar_of(k, prof["loss_bar"], prof["param_bar"]), (k, out[k])
    for u in updates:                                       # an update happens at an episode end: the batch ends terminal, with the reward of a terminal step
        assert u["terminals"][-1] == 1 and u["rewards"][-1] == 0.0 and u["states"].shape == (4, u["n"])
        assert np.all(u["rewards"][u["terminals"] == 1] == 0.0) and np.all(u["rewards"][u["terminals"] == 0] == 1.0)
    assert sum(c[0] for c in calls) == case["total_timesteps"] and calls[-1][3] == case["total_timesteps"]


def test_the_table_covers_the_edges_of_the_kernels():
    n = {c["name"]: [u["n"] for u in B.oracle_run(c["name"])[1]] for c in B.CASES}
    cap = {c["name"]: 2 * c["min_replay_size"] for c in B.CASES}
    flat = [x for v in n.values() for x in v]
    assert any(x < 64 for x in flat) and 64 in flat and 65 in flat and 1024 in flat, "under a wave, one wave, one more; the loss kernel's block"
    assert any(1024 < x < 1024 + 64 for x in flat) and any(x > 1024 and x % 8 for x in flat), "the stride loop's second pass; a ragged size in it"
    assert all(x == cap[k] for k in ("n12_cap", "n16_cap", "n12_gamma0", "n12_gamma1") for x in n[k]), "n = cap: the ring is full at every update"
    assert n["n1024"] == [1024, 1024] and n["n1032"] == [1032, 1032] and n["n64"] == [64] * 3 and n["n65"] == [65] * 3
    assert all(len(v) >= 2 for v in n.values()), "Adam's second step enters everywhere"
    calls = B.oracle_run("n8202_eps4101")[0]
    assert [len(c[2]) for c in calls] == [4101, 4101] and 4101 > B.A2C_MAX_EPS, "one call sees more episodes than the record buffer holds"
    assert {c["gamma"] for c in B.CASES} >= {0.0, 0.99, 1.0} and {c["head"] for c in B.CASES} == {1.0, 20.0}
    # the head's scale is what it is there for: x 20 leans (a few per cent off 50/50), x 1 is 50/50 to a tenth of a per cent
    for name, lo, hi in (("default", 0.51, 0.6), ("default_head1", 0.5, 0.502)):
        u = B.oracle_run(name)[1][0]
        z = np.stack([O.a2c_forward(B.case_cfg(B.CASE[name]), u["params_before"], 0, u["states"][:, b]) for b in range(u["n"])])
        p = 1.0 / (1.0 + np.exp(-np.abs(z[:, 0] - z[:, 1])))
        assert lo < np.median(p) < hi, (name, np.median(p))


@pytest.mark.parametrize("name", B.CHEAPEST)
def test_floor_and_mutants_reproduce_the_committed_profile(prof, name):
    got = B.measure(B.CASE[name])
    rec = prof["cases"][name]
    assert got["floor"] == rec["floor"] and got["oracle_to_twin"] == rec["oracle_to_twin"]
    assert got["mutants"] == rec["mutants"]
    assert {m: B.mutant_ratio(d, prof["loss_bar"]) for m, d in got["mutants"].items()} == rec["mutant_ratio"]


def test_every_mutant_is_ten_bars_away_in_every_case_it_applies_to(prof):
    assert prof["mutant_factor"] == B.MUTANT_FACTOR == 10
    assert list(prof["cases"]) == sorted(c["name"] for c in B.CASES)
    for c in B.CASES:
        rec = prof["cases"][c["name"]]
        assert sorted(rec["mutants"]) == sorted(rec["mutant_ratio"]) == sorted(B.applicable(c)), c["name"]
        for m, dist in rec["mutants"].items():
            assert set(dist) == set(B.OBSERVABLES)
            ratio = B.mutant_ratio(dist, prof["loss_bar"], prof["param_bar"])
            assert ratio == rec["mutant_ratio"][m] and ratio >= 10, (c["name"], m, ratio)
            assert rec["mutant_ratio_without_grads"][m] == B.mutant_ratio(dist, prof["loss_bar"], prof["param_bar"], without=("grads",))
    # gamma = 0 switches the returns' recursion off: the two mutants that break it are left out there, and nowhere else
    assert {c["name"] for c in B.CASES if len(B.applicable(c)) < len(B.MUTANTS)} == {"n12_gamma0"}
    assert sorted(set(B.MUTANTS) - set(B.applicable(B.CASE["n12_gamma0"]))) == ["M4", "M6"]
    assert sorted(prof["mutants"]) == sorted(B.MUTANTS)
    for m, rec in prof["mutants"].items():
        ratios = {n: c["mutant_ratio"][m] for n, c in prof["cases"].items() if m in c["mutant_ratio"]}
        assert rec["worst_ratio"] == min(ratios.values()) == ratios[rec["worst_case"]] and rec["cases"] == len(ratios) >= 11, m
        blind = sorted(n for n, c in prof["cases"].items() if m in c["mutant_ratio"] and c["mutant_ratio_without_grads"][m] < 10)
        assert rec["only_read_grads"] == blind and rec["synthetic_open_end"] == (m in B.SYNTHETIC)
    # what crl_a2c_read_grads is for: at the default shape the halved critic cotangent leaves losses AND parameters where they were (both steps
    # are clipped: ClipNorm rescales the halved gradient to the same vector), and only the gradients show it
    assert prof["mutants"]["M1"]["only_read_grads"] == ["default"]
    assert prof["cases"]["default"]["mutant_ratio_without_grads"]["M1"] == 0.0 and prof["cases"]["default"]["mutants"]["M1"]["grads"] == 0.5


def test_the_reset_state_mutant_is_invisible_to_the_loop():
    """final_value never reaches a result of the loop: every batch ends terminal, and a2c.jl:15 then drops it. So M6 is measured on batches whose last
    transition was made non-terminal (profiles/a2c_bar.json, synthetic_open_end), and on the real ones it moves nothing."""
    case = B.CASE["n12_cap"]
    base = B.run_twin(case)
    with_m6 = B.run_twin(case, B.patched(**B.MUTANTS["M6"][2]()))
    assert B.distances(with_m6, base) == dict.fromkeys(B.OBSERVABLES, 0.0)
    u = B.oracle_run("n12_cap")[1][0]
    assert not np.array_equal(u["final_state"], u["reset_state"])
    fv = R.final_value(u["params_before"], u["final_state"])
    assert fv == O.a2c_forward(B.case_cfg(case), u["params_before"], 1, u["final_state"])[0]
    t = u["terminals"].copy(); t[-1] = 0
    G = R.discounted_future_rewards(u["rewards"], t, fv, 0.5)
    assert G[-1] == 0.5 * fv and np.array_equal(G, O.a2c_discounted_future_rewards(u["rewards"], t, fv, 0.5))


def test_the_bars_follow_their_formulas(prof):
    floor = max(rec["floor"][o] for rec in prof["cases"].values() for o in B.LOSSES)
    assert prof["loss_floor"] == floor and prof["loss_factor"] == B.LOSS_FACTOR == 32 and prof["loss_bar"] == 32 * floor
    assert prof["param_bar"] == B.PARAM_BAR == 2.0 ** -21 == 4 * float(np.spacing(np.float32(1.0)))
    assert prof["jitter_ulp"] == {"exp": 2, "log": 2} and prof["jitter_seeds"] == [1, 2, 3]
    assert B.load_bars() == (prof["loss_bar"], prof["param_bar"])
    assert 0.0 < prof["loss_bar"] < 1e-12 < B.OLD_LOSS_BAR < B.PARAM_BAR < B.OLD_PARAM_BAR
    for name, rec in prof["cases"].items():                 # the twin IS jittered; the Float32 projections do not move
        assert 0.0 < rec["floor"]["actor_loss"] < 1e-15 and 0.0 <= rec["floor"]["critic_loss"] < 1e-15, name
        assert rec["floor"]["grads"] == 0.0 and rec["floor"]["params"] == 0.0, name


def test_patches_leave_the_reference_as_it_was():
    names = ("critic_loss", "actor_loss", "dtanh", "discounted_future_rewards", "softmax_cotangent", "final_value")
    before = {n: getattr(R, n) for n in names}
    for m, (_, _, make) in B.MUTANTS.items():
        with B.patched(**make()):
            assert sum(getattr(R, n) is not f for n, f in before.items()) == 1, m
        assert all(getattr(R, n) is f for n, f in before.items()), m
    with B.jitter(1):
        assert isinstance(R.np, B.JitterNumpy)
    assert R.np is np


def test_tanh_fast64_restates_the_oracle():
    x = np.concatenate([np.linspace(-40.0, 40.0, 4001), [-400.0, -31.0, -30.0, -0.1304, -0.1303, 0.0, 1e-9, 0.1303, 0.1304, 29.9, 30.0, 30.1, 800.0]])
    want = np.array([O.a2c_lib().a2c_tanh_fast(float(v)) for v in x])
    got = R.tanh_fast64(x)
    assert np.abs(got - want).max() <= 2.0 ** -52 and np.array_equal(got[np.abs(x) < 0.13], want[np.abs(x) < 0.13])      # exp differs, the polynomial does not
    assert R.tanh_fast64(np.array([31.0, -31.0, 800.0])).tolist() == [1.0, -1.0, 1.0]
