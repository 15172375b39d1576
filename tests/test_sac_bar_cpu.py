"""What the SAC parity bars are worth, without a GPU: profiles/sac_bar.json and profiles/sac_edges_bar.json (scripts/sac_bar.py) are reproduced
exactly for the two cheapest cases of each of tests/sac_bar.py's tables, and the conditions the tables have to meet hold over the whole files: no
parameter floor above PARAM_BAR, every mutant at least 10 bars away on a case it applies to, the cases built around an edge met it on the
reference's own counters."""
import json

import pytest

import ddpg_bar as DB
import sac_bar as B
import sac_ref as S

TABLES = {"cases": (B.CASES, B.CHEAPEST), "edges": (B.EDGE_CASES, B.EDGE_CHEAPEST)}


@pytest.fixture(scope="module")
def profs():
    return {t: json.load(open(B.TABLES[t][1])) for t in TABLES}


@pytest.mark.parametrize("table,name", [(t, n) for t, (_, cheapest) in TABLES.items() for n in cheapest])
def test_floor_and_mutants_reproduce_the_committed_profile(profs, table, name):
    prof = profs[table]
    got = B.measure(next(c for c in TABLES[table][0] if c["name"] == name))
    rec = prof["cases"][name]
    assert got["floor"] == rec["floor"] and got["stats"] == rec["stats"]
    assert got["mutants"] == rec["mutants"]
    assert {m: B.mutant_ratio(d, prof["loss_bar"]) for m, d in got["mutants"].items()} == rec["mutant_ratio"]


@pytest.mark.parametrize("table", sorted(TABLES))
def test_the_profile_covers_the_table_and_its_conditions_hold(profs, table):
    prof, cases = profs[table], TABLES[table][0]
    assert list(prof["cases"]) == sorted(c["name"] for c in cases)
    for c in cases:
        rec = prof["cases"][c["name"]]
        assert sorted(rec["mutants"]) == sorted(rec["mutant_ratio"]) == sorted(B.applicable(c)), c["name"]
        assert set(rec["floor"]) == set(B.OBSERVABLES) and all(set(d) == set(B.OBSERVABLES) for d in rec["mutants"].values())
        d = B.case_cfg(c)
        assert (rec["D"], rec["A"], rec["batch_size"], rec["updates"]) == (c["D"], c["A"], d["batch_size"], c["T"] - B.threshold(d))
        assert all(rec["floor"][o] <= prof["param_bar"] for o in B.PARAMS + ("log_alpha",)), c["name"]
        assert rec["loss_floor"] == max(rec["floor"][o] for o in B.LOSSES) <= prof["loss_floor"]
        assert B.edge_met(c["name"], rec["stats"]), c["name"]
    floor = max(rec["floor"][o] for rec in prof["cases"].values() for o in B.LOSSES)
    assert prof["loss_floor"] == floor > 0.0 and prof["loss_bar"] == B.LOSS_FACTOR * floor and prof["loss_factor"] == B.LOSS_FACTOR == 32
    assert prof["param_bar"] == B.PARAM_BAR == 2.0 ** -21 and prof["mutant_factor"] == B.MUTANT_FACTOR == 10
    assert prof["jitter_ulp"] == DB.JITTER_ULP and prof["jitter_seeds"] == list(DB.JITTER_SEEDS)
    assert B.load_bars(B.TABLES[table][1]) == (prof["loss_bar"], prof["param_bar"]) and prof["loss_bar"] < B.PARAM_BAR < B.OLD_BAR
    # every mutant is at least ten bars away on a case it applies to
    for m, rec in prof["mutants"].items():
        ratios = {n: c["mutant_ratio"][m] for n, c in prof["cases"].items() if m in c["mutant_ratio"]}
        assert rec["best_ratio"] == max(ratios.values()) == ratios[rec["best_case"]] >= 10 and rec["cases"] == len(ratios), m
    want = set(B.MUTANTS) if table == "cases" else set(B.MUTANTS) - {"S12"}       # no edge case switches autotune off
    assert set(prof["mutants"]) == want


def test_the_first_table_is_the_tight_one(profs):
    assert profs["cases"]["loss_bar"] < 1e-12 and profs["cases"]["loss_bar"] < profs["edges"]["loss_bar"]
    assert profs["edges"]["loss_floor"] == profs["edges"]["cases"]["saturated"]["loss_floor"], "the edge table's bar is the saturated case's"
    easy = [n for n in profs["edges"]["cases"] if n not in ("saturated", "logstd_ends")]
    assert all(profs["edges"]["cases"][n]["loss_floor"] < profs["cases"]["loss_floor"] for n in easy)
    st = profs["edges"]["cases"]["saturated"]["stats"]
    assert st["n_y_one"] >= 0.5 * st["n_samples"] and st["n_y_near"] >= 0.02 * st["n_samples"]
    st = profs["edges"]["cases"]["logstd_ends"]["stats"]
    assert st["n_ls_low"] >= 0.05 * st["n_samples"] and st["n_ls_high"] >= 0.05 * st["n_samples"]


def test_the_rejected_settings_are_recorded_with_their_floors_above_the_bar(profs):
    """PARAM_BAR was not loosened for the denser settings of `saturated`: their floors are on record, reproduce, and are above it"""
    rej = profs["edges"]["rejected"]
    assert list(rej) == sorted(c["name"] for c in B.REJECTED) and "rejected" not in profs["cases"]
    for c in B.REJECTED:
        rec = rej[c["name"]]
        assert rec["above_param_bar"] == sorted(o for o in B.PARAMS + ("log_alpha",) if rec["floor"][o] > B.PARAM_BAR) and "actor" in rec["above_param_bar"]
        assert rec["stats"]["n_y_near"] >= 0.05 * rec["stats"]["n_samples"] and c["name"] not in B.EDGE_CASE
    c = B.REJECTED[0]                                                              # the 15-update one: cheap
    got = B.measure_floor(c)
    assert got["floor"] == rej[c["name"]]["floor"] and got["stats"] == rej[c["name"]]["stats"]
    assert B.case_loss_bar("saturated") == profs["edges"]["loss_bar"] and B.case_loss_bar("logstd_ends") < 1e-11


def test_mutants_leave_the_reference_as_it_was():
    names = ("draws", "actor_stream", "next_obs", "head_rows", "squash_term", "entropy_term", "grad_critic", "direct_term", "alpha_due",
             "reported_alpha", "polyak_sources")
    before = {n: getattr(S, n) for n in names}
    for m, (_, _, make) in B.MUTANTS.items():
        with B.patched(**make()):
            assert sum(getattr(S, n) is not f for n, f in before.items()) == 1, m     # one wrong line each
        assert all(getattr(S, n) is f for n, f in before.items()), m
