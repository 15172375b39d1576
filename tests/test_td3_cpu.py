"""The yardstick of the TD3 parity tests, without a GPU. tests/td3_ref.py is pinned against tests/ddpg_ref.py in the one setting where TD3 IS DDPG
(policy_delay = 1, policy_noise = 0, critic 2 = critic 1, bounds ±2: bit for bit, critic_loss exactly 2x); profiles/td3_bar.json
(scripts/td3_bar.py) is reproduced exactly for the two cheapest cases of tests/td3_bar.py's table; and the conditions the table has to meet hold
over the whole file: every parameter floor exactly 0.0, every applicable mutant at least 10 bars away in every case, the cases built around an
edge met it on the reference's own numbers."""
import json

import numpy as np
import pytest

import ddpg_bar as DB
import ddpg_ref as R
import td3_bar as B
import td3_ref as T


@pytest.fixture(scope="module")
def prof():
    return json.load(open(B.BAR_JSON))


# ---------------------------------------------------------------------------------------------------- the degenerate setting is DDPG
@pytest.mark.parametrize("D,A,k", [(3, 1, 7), (5, 3, 4)])
def test_the_degenerate_setting_is_ddpg_bit_for_bit(D, A, k):
    d = DB.cfg_dict(D, A, total_timesteps=60, batch_size=k, noise_in_update=0)
    case = dict(D=D, A=A)
    actor, critic = DB.case_params(case)
    trs = DB.transitions(D, A, 60, 7)
    ddpg = R.DDPG(d, actor, critic); ddpg.run_transitions(trs)
    td3 = T.TD3(dict(d, policy_delay=1, policy_noise=0.0, noise_clip=0.5), actor, critic, critic); td3.run_transitions(trs)
    assert ddpg.n_updates == td3.n_updates == td3.n_actor_steps == 50 and td3.n_target_clamped == 0
    a, c1, c2, ta, tc1, tc2 = td3.params()
    assert np.array_equal(a, ddpg.actor) and np.array_equal(ta, ddpg.actor_t)
    assert np.array_equal(c1, ddpg.critic) and np.array_equal(c2, ddpg.critic) and np.array_equal(tc1, ddpg.critic_t) and np.array_equal(tc2, ddpg.critic_t)
    assert [l[0] for l in td3.losses] == [l[0] for l in ddpg.losses] == list(range(11, 61))
    assert [l[1] for l in td3.losses] == [l[1] for l in ddpg.losses]
    assert [l[2] for l in td3.losses] == [2.0 * l[2] for l in ddpg.losses]
    # and it stops being DDPG as soon as one of the three parts is switched on
    for kw in (dict(policy_delay=2), dict(policy_noise=0.2)):
        other = T.TD3({**d, "policy_delay": 1, "policy_noise": 0.0, "noise_clip": 0.5, **kw}, actor, critic, critic); other.run_transitions(trs)
        assert not np.array_equal(other.critic, ddpg.critic)
    other = T.TD3(dict(d, policy_delay=1, policy_noise=0.0, noise_clip=0.5), actor, critic, DB.case_params(case, seed=2)[1]); other.run_transitions(trs)
    assert not np.array_equal(other.critic, ddpg.critic)


def test_the_smoothing_draw_is_per_sample_on_its_own_stream():
    z = T.smoothing_draws(0x5EED, 77, 5, 3)
    assert z.shape == (3, 5) and len(set(z.reshape(-1).tolist())) == 15
    for b in range(5):
        assert np.array_equal(z[:, b], R.normal(0x5EED, 16 * b + np.arange(3), 77, T.S_SMOOTH))
    assert T.S_SMOOTH == 0x17 and T.S_SMOOTH not in (R.S_BEHAVE, R.S_WARMUP, R.S_TARGET, R.S_ACTOR, R.S_RESET, R.S_RESET0, 0x16, R.S_SAMPLE)
    assert np.array_equal(T.smoothing_noise(np.array([-9.0, -1.0, 0.0, 1.0, 9.0]), 0.5, 0.5), [-0.5, -0.5, 0.0, 0.5, 0.5])
    assert np.array_equal(T.target_action(np.array([-1.0, 0.1, 1.0]), np.array([-0.5, 0.0, 0.5]), -2.0, 2.0), [-2.0, 0.2, 2.0])
    assert np.array_equal(T.next_q(np.array([1.0, -2.0]), np.array([0.5, 3.0])), [0.5, -2.0])


def test_the_delayed_actor_leaves_actor_and_targets_alone():
    case = B.CASE["delay_never"]
    actor, c1, c2 = B.case_params(case)
    ref = T.TD3(B.case_cfg(case), actor, c1, c2); ref.run_transitions(B.case_transitions(case))
    a, q1, q2, ta, t1, t2 = ref.params()
    assert ref.n_updates == 100 and ref.n_actor_steps == 0
    assert all(np.array_equal(x, y) for x, y in ((a, actor), (ta, actor), (t1, c1), (t2, c2)))
    assert not np.array_equal(q1, c1) and not np.array_equal(q2, c2)
    assert all(l[1] == 0.0 for l in ref.losses) and np.array_equal(ref.opt_a.bp, np.tile([R.B1, R.B2], (6, 1)))


# ---------------------------------------------------------------------------------------------------- the committed profile
@pytest.mark.parametrize("name", B.CHEAPEST)
def test_floor_and_mutants_reproduce_the_committed_profile(prof, name):
    got = B.measure(B.CASE[name])
    rec = prof["cases"][name]
    assert got["floor"] == rec["floor"] and got["stats"] == rec["stats"]
    assert got["mutants"] == rec["mutants"]
    ratios = {m: B.mutant_ratio(d, prof["loss_bar"]) for m, d in got["mutants"].items()}
    assert ratios == rec["mutant_ratio"] and all(r >= B.MUTANT_FACTOR for r in ratios.values())


def test_the_profile_covers_the_table_and_every_applicable_mutant(prof):
    assert list(prof["cases"]) == sorted(c["name"] for c in B.CASES)
    for c in B.CASES:
        rec = prof["cases"][c["name"]]
        assert sorted(rec["mutants"]) == sorted(rec["mutant_ratio"]) == sorted(B.applicable(c, rec["stats"])), c["name"]
        assert set(rec["floor"]) == set(B.OBSERVABLES) and all(set(d) == set(B.OBSERVABLES) for d in rec["mutants"].values())
        d = B.case_cfg(c)
        assert (rec["D"], rec["A"], rec["batch_size"], rec["updates"], rec["policy_delay"]) == (
            c["D"], c["A"], d["batch_size"], c["T"] - B.threshold(d), d["policy_delay"])
        assert c["T"] <= 150
    # which mutant is left out where, and why: the line it breaks is switched off there
    left_out = {c["name"]: sorted(set(B.MUTANTS) - set(prof["cases"][c["name"]]["mutants"])) for c in B.CASES}
    assert left_out["gamma0"] == left_out["all_terminal"] == ["T1", "T2", "T3", "T4"]      # the next-state value never reaches the TD target
    assert left_out["delay1"] == ["T5", "T6"]                                              # nothing is delayed
    assert left_out["delay_never"] == ["T3", "T9"]                                         # no actor step to send through critic 2
    assert left_out["clip0"] == ["T3", "T4"]                                               # all noise is 0: position 0's is every position's
    assert left_out["bounds"] == left_out["ni65_k31"] == left_out["d64a16_k61"] == left_out["tau1"] == []
    # T3 applies exactly where the reference's own target actions left the bounds
    assert all(("T3" in left_out[c["name"]]) == (prof["cases"][c["name"]]["stats"]["n_target_clamped"] == 0 or c["name"] in ("gamma0", "all_terminal"))
               for c in B.CASES)
    assert sorted(prof["mutants"]) == sorted(B.MUTANTS) and all(prof["mutants"][m]["cases"] >= 3 for m in B.MUTANTS)


def test_the_edge_cases_met_their_edges_on_the_reference(prof):
    st = prof["cases"]["noise1_clip05"]["stats"]                # P(|z| > 0.5) = 0.62
    assert st["n_noise"] == 7 * 100 and 0.1 * st["n_noise"] <= st["n_noise_clipped"] <= 0.9 * st["n_noise"]
    st = prof["cases"]["bounds"]["stats"]
    assert st["n_target_actions"] == 700 and 0 < st["n_target_clamped"] < 700
    st = prof["cases"]["clip0"]["stats"]
    assert st["n_noise_clipped"] == st["n_noise"] == 700       # every non-zero draw is cut to 0
    assert prof["cases"]["delay_never"]["stats"]["n_actor_steps"] == 0
    steps = {n: prof["cases"][n]["stats"]["n_actor_steps"] for n in ("delay1", "delay2_on", "delay2_off", "delay3_on", "delay3_off")}
    assert steps == {"delay1": 100, "delay2_on": 50, "delay2_off": 49, "delay3_on": 33, "delay3_off": 33}
    for n, on in (("delay2_on", True), ("delay2_off", False), ("delay3_on", True), ("delay3_off", False)):
        c = B.CASE[n]
        assert (c["T"] % B.case_cfg(c)["policy_delay"] == 0) == on


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


def test_the_bars_follow_their_formulas(prof):
    floor = max(rec["floor"][o] for rec in prof["cases"].values() for o in B.LOSSES)
    assert prof["loss_floor"] == floor > 0.0 and prof["loss_factor"] == B.LOSS_FACTOR == 32
    assert prof["loss_bar"] == 32 * floor
    assert prof["param_bar"] == B.PARAM_BAR == 2.0 ** -21
    assert prof["jitter_ulp"] == DB.JITTER_ULP and prof["jitter_seeds"] == list(DB.JITTER_SEEDS)
    assert B.load_bars() == (prof["loss_bar"], prof["param_bar"])
    assert prof["loss_bar"] < 1e-12 < B.PARAM_BAR < B.OLD_BAR


def test_mutants_leave_the_reference_as_it_was():
    names = ("smoothing_draws", "smoothing_noise", "target_action", "next_q", "actor_due", "targets_due", "critic2_cotangent_td", "critic2_step",
             "actor_loss_critic", "polyak_targets")
    before = {n: getattr(T, n) for n in names}
    for m, (_, _, make) in B.MUTANTS.items():
        with B.patched(**make()):
            assert sum(getattr(T, n) is not f for n, f in before.items()) == 1, m     # one wrong line each
        assert all(getattr(T, n) is f for n, f in before.items()), m
