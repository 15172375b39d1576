"""The yardstick of tests/test_gpu_td3_edges.py, without a GPU: profiles/td3_edges_bar.json (scripts/td3_bar.py --table edges) over tests/td3_bar.py's
second table, EDGE_CASES — batches past 64 up to the largest, rings that wrap, log_frequency > 1 against policy_delay. The profile covers exactly
that table and the mutants T1 to T11 where they apply, its bars follow their formulas, the conditions the script checks hold over the whole file,
and measure() reproduces it exactly for the two cheapest cases.

Why the table exists is T10: the smoothing draw's component word 16·b + c taken modulo 1024, so that batch position 64 redraws position 0's noise.
It is EXACTLY the reference on every case of the first table (k <= 61 there: no word reaches 1024) and at least ten bars away on every edge case
with k > 64."""
import json

import pytest

import ddpg_bar as DB
import td3_bar as B
import td3_ref as T


@pytest.fixture(scope="module")
def prof():
    return json.load(open(B.EDGE_BAR_JSON))


def test_the_profile_covers_the_edge_table_and_every_applicable_mutant(prof):
    assert list(prof["cases"]) == sorted(c["name"] for c in B.EDGE_CASES) and len(B.EDGE_CASES) == 12
    assert B.TABLES["edges"] == (B.EDGE_CASES, B.ALL_MUTANTS, B.EDGE_BAR_JSON) and B.TABLES["cases"] == (B.CASES, B.MUTANTS, B.BAR_JSON)
    assert list(B.ALL_MUTANTS) == list(B.MUTANTS) + ["T10", "T11"] and list(B.MUTANTS) == [f"T{i}" for i in range(1, 10)]
    for c in B.EDGE_CASES:
        rec = prof["cases"][c["name"]]
        assert sorted(rec["mutants"]) == sorted(rec["mutant_ratio"]) == sorted(B.applicable(c, rec["stats"], B.ALL_MUTANTS)), c["name"]
        assert set(rec["floor"]) == set(B.OBSERVABLES) and all(set(d) == set(B.OBSERVABLES) for d in rec["mutants"].values())
        d = B.case_cfg(c)
        assert (rec["D"], rec["A"], rec["batch_size"], rec["updates"], rec["policy_delay"]) == (
            c["D"], c["A"], d["batch_size"], c["T"] - B.threshold(d), d["policy_delay"])
        assert rec["stats"]["n_actor_steps"] == sum(g % d["policy_delay"] == 0 for g in range(B.threshold(d) + 1, c["T"] + 1)) > 0
        assert rec["stats"]["n_noise"] == rec["stats"]["n_target_actions"] == c["A"] * d["batch_size"] * rec["updates"]
    # which mutant is left out where: T10 where no component word reaches 1024, T3 where the reference's own target actions stayed inside the bounds
    left_out = {c["name"]: sorted(set(B.ALL_MUTANTS) - set(prof["cases"][c["name"]]["mutants"])) for c in B.EDGE_CASES}
    for c in B.EDGE_CASES:
        want = (["T10"] if B.case_cfg(c)["batch_size"] <= 64 else []) + (["T3"] if prof["cases"][c["name"]]["stats"]["n_target_clamped"] == 0 else [])
        assert left_out[c["name"]] == sorted(want), c["name"]
    assert [n for n in left_out if "T10" not in left_out[n]] == ["k65", "k120_default", "kmax_ring_eq_batch", "kmax_a16", "ring200_full", "ring200_k199"]
    assert left_out["kmax_a16"] == left_out["ring200_full"] == left_out["ring200_k199"] == []
    assert sorted(prof["mutants"]) == sorted(B.ALL_MUTANTS)
    assert prof["mutants"]["T10"]["cases"] == 6 and prof["mutants"]["T11"]["cases"] == 12 and all(prof["mutants"][m]["cases"] >= 6 for m in B.ALL_MUTANTS)


def test_the_edge_bars_follow_their_formulas(prof):
    floor = max(rec["floor"][o] for rec in prof["cases"].values() for o in B.LOSSES)
    assert prof["loss_floor"] == floor > 0.0 and prof["loss_factor"] == B.LOSS_FACTOR == 32
    assert prof["loss_bar"] == 32 * floor
    assert prof["param_bar"] == B.PARAM_BAR == 2.0 ** -21
    assert prof["jitter_ulp"] == DB.JITTER_ULP and prof["jitter_seeds"] == list(DB.JITTER_SEEDS)
    assert B.load_bars(B.EDGE_BAR_JSON) == (prof["loss_bar"], prof["param_bar"]) and B.load_bars() == B.load_bars(B.BAR_JSON)
    assert prof["loss_bar"] < 1e-12 < B.PARAM_BAR < B.OLD_BAR
    # the one floor measured before the table was built, at the largest batch
    assert prof["cases"]["kmax_ring_eq_batch"]["floor"]["critic_loss"] == pytest.approx(4.07e-16, rel=0.01)


def test_every_parameter_floor_is_exactly_zero_and_every_mutant_ten_bars_away(prof):
    assert prof["mutant_factor"] == B.MUTANT_FACTOR == 10
    for name, rec in prof["cases"].items():
        for o in B.PARAMS:
            assert rec["floor"][o] == 0.0, (name, o)
        assert all(0.0 <= rec["floor"][o] < 1e-14 for o in B.LOSSES), name
        for m, dist in rec["mutants"].items():
            ratio = max(dist[o] / (prof["loss_bar"] if o in B.LOSSES else prof["param_bar"]) for o in B.OBSERVABLES)
            assert ratio == rec["mutant_ratio"][m] and ratio >= 10, (name, m, ratio)
    for m, rec in prof["mutants"].items():
        ratios = {n: c["mutant_ratio"][m] for n, c in prof["cases"].items() if m in c["mutant_ratio"]}
        assert rec["worst_ratio"] == min(ratios.values()) == ratios[rec["worst_case"]] and rec["cases"] == len(ratios), m


def test_the_edge_cases_met_their_edges_on_the_reference(prof):
    st = prof["cases"]["kmax_a16"]["stats"]                    # policy_noise = 1, noise_clip = 0.5: P(|z| > 0.5) = 0.62
    assert st["n_noise"] == 16 * 1024 * 4 and 0.1 * st["n_noise"] <= st["n_noise_clipped"] <= 0.9 * st["n_noise"] and st["n_target_clamped"] > 0
    assert 16 * 1023 + 15 == 16383                             # the largest component word, at act_dim 16 and k = 1024
    st = prof["cases"]["bounds_a6"]["stats"]
    assert st["n_target_actions"] == 6 * 7 * 100 and 0 < st["n_target_clamped"] < st["n_target_actions"]
    assert 2 * st["n_noise_clipped"] > st["n_noise"] and 2 * st["n_target_clamped"] > st["n_target_actions"], "both bind on more than half"
    for n in B.EDGE_MULTI_ROUND:                               # a draw went past the first round of 1024 candidates, and the ring wrapped
        c = B.EDGE_CASE[n]
        assert max(DB.case_candidates(c)) > 1024, n
        assert B.case_cfg(c)["buffer_size"] < c["T"], n
    assert prof["cases"]["kmax_ring_eq_batch"]["stats"]["n_actor_steps"] == 4 and prof["cases"]["kmax_ring_eq_batch"]["updates"] == 8
    assert B.case_cfg(B.EDGE_CASE["ring200_k199"])["batch_size"] % 2 == 1 and B.EDGE_CASE["none_terminal"]["terminal"] == "none"
    c = B.EDGE_CASE["ni64_k30"]
    assert c["D"] + c["A"] == 64 and B.case_cfg(c)["batch_size"] == 30
    c = B.EDGE_CASE["d64a1_k7"]
    assert (c["D"], c["A"]) == (64, 1)
    # log_frequency against policy_delay = 3: which records fall on an actor step
    for n, first_due in (("logfreq7_delay3", [False, True, False]), ("logfreq4_delay3", [True, False, False])):
        c = B.EDGE_CASE[n]; d = B.case_cfg(c)
        logged = [g for g in range(B.threshold(d) + 1, c["T"] + 1) if g % d["log_frequency"] == 0]
        assert logged[0] == (14 if d["log_frequency"] == 7 else 12) and [g % 3 == 0 for g in logged[:3]] == first_due


@pytest.mark.parametrize("name", B.EDGE_CHEAPEST)
def test_floor_and_mutants_reproduce_the_committed_edge_profile(prof, name):
    got = B.measure(B.EDGE_CASE[name], B.ALL_MUTANTS)
    rec = prof["cases"][name]
    assert got["floor"] == rec["floor"] and got["stats"] == rec["stats"]
    assert got["mutants"] == rec["mutants"]
    ratios = {m: B.mutant_ratio(d, prof["loss_bar"]) for m, d in got["mutants"].items()}
    assert ratios == rec["mutant_ratio"] and all(r >= B.MUTANT_FACTOR for r in ratios.values())


def carried_actor_loss(case):
    """→ {g: the actor_loss of the latest actor step <= g} from the reference run of `case` with every update logged"""
    every = B.run_ref(dict(case, kw=dict(case["kw"], log_frequency=1)))[0]
    delay, out, latest = B.case_cfg(case)["policy_delay"], {}, 0.0
    for g, actor_loss, _ in every:
        if g % delay == 0:
            latest = actor_loss
        assert actor_loss == latest
        out[g] = latest
    return out


@pytest.mark.parametrize("name,steps", [("logfreq7_delay3", list(range(14, 111, 7))), ("logfreq4_delay3", list(range(12, 111, 4)))])
def test_a_record_on_a_step_without_an_actor_step_carries_the_latest_one(name, steps):
    case = B.EDGE_CASE[name]
    losses = B.run_ref(case)[0]
    carried = carried_actor_loss(case)
    assert [l[0] for l in losses] == steps
    assert [l[1] for l in losses] == [carried[g] for g in steps] and all(l[1] != 0.0 for l in losses)
    off = [g for g in steps if g % 3 != 0]
    assert len(off) > len(steps) // 2 and all(carried[g] == carried[g - g % 3] for g in off)
    assert all(carried[g] != carried[g - 3] for g in range(15, 111)), "every actor step logs a new value"


# ---------------------------------------------------------------------------------------------------- why the table exists
_T10_OLD = [c["name"] for c in B.CASES if B._noise_on(c)]


def test_t10_would_apply_to_most_of_the_first_table_but_for_its_batches():
    assert sorted(set(c["name"] for c in B.CASES) - set(_T10_OLD)) == ["all_terminal", "clip0", "gamma0"] and len(_T10_OLD) == 12
    assert max(B.case_cfg(c)["batch_size"] for c in B.CASES) == 61 and 16 * 60 + 15 < 1024


@pytest.mark.parametrize("name", _T10_OLD)
def test_t10_is_exactly_the_reference_on_the_first_table(name):
    case = B.CASE[name]
    base = B.run_ref(case)
    assert base[2]["n_noise"] > base[2]["n_noise_clipped"] >= 0
    dist = B.variant(case, "T10", base)
    assert set(dist) == set(B.OBSERVABLES) and len(dist) == 8
    assert all(v == 0.0 for v in dist.values()), dist


def test_t10_is_ten_bars_away_in_every_edge_case_past_64(prof):
    past = [c["name"] for c in B.EDGE_CASES if B.case_cfg(c)["batch_size"] > 64]
    assert past == ["k65", "k120_default", "kmax_ring_eq_batch", "kmax_a16", "ring200_full", "ring200_k199"]
    for n in past:
        assert prof["cases"][n]["mutant_ratio"]["T10"] >= 10, n
    assert prof["mutants"]["T10"]["worst_ratio"] >= 10
    # and one of them recomputed: the smallest batch that reaches word 1024
    case = B.EDGE_CASE["k65"]
    dist = B.variant(case, "T10", B.run_ref(case))
    assert dist == prof["cases"]["k65"]["mutants"]["T10"] and B.mutant_ratio(dist, prof["loss_bar"]) >= 10


def test_the_edge_mutants_leave_the_reference_as_it_was():
    names = ("smoothing_draws", "smoothing_noise", "target_action", "next_q", "actor_due", "targets_due", "critic2_cotangent_td", "critic2_step",
             "actor_loss_critic", "polyak_targets")
    before = {n: getattr(T, n) for n in names}
    for m, (_, _, make) in B.EDGE_MUTANTS.items():
        with B.patched(**make()):
            assert sum(getattr(T, n) is not f for n, f in before.items()) == 1, m     # one wrong line each
        assert all(getattr(T, n) is f for n, f in before.items()), m
    with B.patched(**B.EDGE_MUTANTS["T10"][2]()):                                      # the wrapped word: position 64 is position 0
        z = T.smoothing_draws(0x5EED, 77, 66, 3)
    ref = T.smoothing_draws(0x5EED, 77, 66, 3)
    assert (z[:, :64] == ref[:, :64]).all() and (z[:, 64:] == ref[:, :2]).all() and not (ref[:, 64:] == ref[:, :2]).any()
