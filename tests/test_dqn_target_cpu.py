"""The anchors of tests/dqn_target_ref.py, the restatement that tests/test_gpu_dqn_target.py holds the device's n-step / double-Q targets against —
no GPU.

(a) with {n_step = 1, double_q = 0} and the oracle's uniform draw the whole loop IS oracle/dqn_oracle.c, bit for bit; (b) double Q-learning with a
target that is copied at every update is the plain run, bit for bit; (c) the walk is the n-step return of a brute-force definition over an explicit
time-ordered list of transitions, on random small rings, wrapped ones included; (d) the case table of tests/dqn_target_bar.py reaches every edge it
names — a condition on the table, asserted from the restatement alone; (e) each one-line mutant moves a compared observable by more than the bar;
(f) DQNTargetOptions is validated on the host."""
import importlib

import numpy as np
import pytest

import dqn_per_bar as PB
import dqn_target_bar as TB
import dqn_target_ref as T
import oraclelib as O


# ---------------------------------------------------------------------------------------------------- (a) the oracle anchor
@pytest.mark.parametrize("kw", [dict(total_timesteps=400, batch_size=31, buffer_size=64, min_buff_size=40, train_freq=3, target_net_freq=30),
                                dict(total_timesteps=150, batch_size=1, buffer_size=1, min_buff_size=1, train_freq=1, target_net_freq=1),
                                dict(total_timesteps=330, batch_size=120, buffer_size=1000, min_buff_size=200, log_frequency=7)])
def test_one_step_max_target_with_the_oracles_draw_is_the_oracle(kw):
    cfg = O.dqn_config(**{"lr": 1e-3, "log_frequency": 1, "seed": 21, **kw})
    params = TB.case_params(None)
    ref, st = T.DQNTarget(cfg, None, dict(n_step=1, double_q=False), params), O.DQNState(cfg, params)
    for chunk in (1, 7, cfg.total_timesteps):
        assert ref.run(chunk) == st.run(chunk), "steps taken, episode records, logged losses"
        so, sr = st.env(), ref.status()
        assert all(so[f] == sr[f] for f in ("global_step", "rb_size", "n_updates", "last_loss")) and np.array_equal(so["state"], sr["state"])
        q, t = st.params()
        assert np.array_equal(ref.q, q) and np.array_equal(ref.t, t)
    assert ref.n_updates >= 10
    assert (ref.m == 1).all() and np.array_equal(ref.last, ref.idx) and (ref.ndisc == cfg.gamma).all() and np.array_equal(ref.nret, ref.reward[ref.idx])
    st.close()


# ---------------------------------------------------------------------------------------------------- the table, run once
@pytest.fixture(scope="module")
def runs():
    return {c["name"]: TB.run_ref(c) for c in TB.CASES}


# ---------------------------------------------------------------------------------------------------- (b)
def test_double_q_with_a_target_copied_at_every_update_is_the_plain_run(runs):
    case = TB.CASE["double_copy_each"]
    cfg = TB.case_cfg(case)
    assert cfg.target_net_freq == cfg.train_freq
    plain = TB.run_ref(dict(case, tgt=dict(n_step=1, double_q=False)))
    got = runs["double_copy_each"]
    assert got["losses"] == plain["losses"] and len(got["losses"]) == 20
    assert np.array_equal(got["params"][0], plain["params"][0]) and np.array_equal(got["params"][1], plain["params"][1])
    assert np.array_equal(got["ref"].td, plain["ref"].td) and np.array_equal(got["ref"].astar, plain["ref"].astar)
    assert got["counts"]["disagree"] == 0
    assert got["losses"] != runs["double"]["losses"], "a lagging target makes double Q-learning a different run"


# ---------------------------------------------------------------------------------------------------- (c) the walk against brute force
def _brute(reward, terminal, order, pos, n_step, gamma):
    """order: the filled slots from the oldest to the newest; the n-step return of the transition at position pos, as a sum over that list"""
    window = []
    for slot in order[pos:pos + n_step]:
        window.append(slot)
        if terminal[slot]:
            break
    return window[-1], len(window), sum(gamma ** i * reward[s] for i, s in enumerate(window)), gamma ** len(window)


@pytest.mark.parametrize("gamma,exact", [(0.5, True), (0.99, False)])
def test_walk_is_the_brute_force_n_step_return(gamma, exact):
    rng = np.random.default_rng(7)
    seen_wrap = seen_head = seen_term = 0
    for trial in range(300):
        cap = int(rng.integers(1, 12))
        full = bool(rng.integers(0, 2))
        ptr = int(rng.integers(0, cap)) if full else int(rng.integers(1, cap)) if cap > 1 else 0
        size = cap if full or cap == 1 else ptr
        order = [(ptr + i) % cap for i in range(cap)] if size == cap else list(range(size))
        reward = rng.integers(0, 2, cap).astype(np.float64) if exact else rng.standard_normal(cap)
        terminal = (rng.random(cap) < 0.2).astype(np.uint8)
        n_step = int(rng.integers(1, 17))
        for pos, s in enumerate(order):
            T.reset_counts()
            last, m, R, disc = T.walk(reward, terminal, cap, ptr, s, n_step, gamma)
            bl, bm, bR, bdisc = _brute(reward, terminal, order, pos, n_step, gamma)
            assert (last, m) == (bl, bm), (cap, ptr, s, n_step)
            if exact:
                assert R == bR and disc == bdisc, "powers of 0.5 and 0/1 rewards: every operation is exact"
            else:
                assert R == pytest.approx(bR, rel=1e-13, abs=1e-13) and disc == pytest.approx(bdisc, rel=1e-13)
            seen_wrap += T.COUNTS["wraps"]; seen_head += T.COUNTS["head_stops"]; seen_term += T.COUNTS["terminal_stops"]
    assert seen_wrap > 50 and seen_head > 50 and seen_term > 50, "the random rings wrap, end at the head and hold terminals"


def test_walk_by_hand():
    r, t = np.array([1.0, 1.0, 0.0, 1.0]), np.array([0, 0, 1, 0], np.uint8)
    assert T.walk(r, t, 4, 0, 0, 1, 0.5) == (0, 1, 1.0, 0.5)
    assert T.walk(r, t, 4, 0, 0, 3, 0.5) == (2, 3, 1.5, 0.125), "the terminal is the third and last step"
    assert T.walk(r, t, 4, 0, 0, 16, 0.5) == (2, 3, 1.5, 0.125), "and stops a longer horizon"
    assert T.walk(r, t, 4, 0, 3, 3, 0.5) == (3, 1, 1.0, 0.5), "slot 3 is the newest: never wrapped into slot 0, the oldest"
    assert T.walk(r, t, 4, 2, 3, 3, 0.5) == (1, 3, 1.75, 0.125), "ptr = 2: 3 → 0 → 1 crosses the wrap; slot 1 is the newest"
    assert T.walk(r, t, 1, 0, 0, 5, 0.9) == (0, 1, 1.0, 0.9), "one slot"
    assert T.walk(r, t, 4, 0, 0, 3, 0.0) == (2, 3, 1.0, 0.0), "gamma = 0: disc is 0.0 after one step"


# ---------------------------------------------------------------------------------------------------- (d) the table reaches its edges
def test_every_counted_event_occurs_and_every_lagging_double_case_disagrees(runs):
    for c in TB.CASES:
        print(c["name"], runs[c["name"]]["counts"], runs[c["name"]]["ref"].n_updates, "updates")
    for e in T.EVENTS:
        assert sum(r["counts"][e] for r in runs.values()) >= 1, e
    lagging = [c["name"] for c in TB.CASES if TB.lagging_double(c)]
    assert set(lagging) == {"double", "n3_double", "n3_double_k1024_cap1024", "per_n3_double_k31_cap31", "per_n3_double_k120"}
    for name in lagging:
        assert runs[name]["counts"]["disagree"] >= 1, name
    assert runs["double_copy_each"]["counts"]["disagree"] == 0
    # the edges the table names, each in the case that names it
    assert runs["n5_cap31"]["counts"]["wraps"] >= 1 and runs["per_n3_double_k31_cap31"]["counts"]["wraps"] >= 1
    assert runs["n16"]["counts"]["terminal_stops"] >= 1
    assert runs["n16_cap8_k4"]["counts"]["head_stops"] >= 1 and runs["n16_cap8_k4"]["ref"].m.max() <= 8
    assert runs["n3_freq1"]["counts"]["head_stops"] >= 1
    assert runs["n3_cap1_k1"]["counts"]["head_stops"] >= 1
    assert (runs["n3_gamma0"]["ref"].ndisc == 0.0).all()
    assert all(r["ref"].n_updates >= 3 and len(r["losses"]) >= 3 for r in runs.values())
    assert all(sum(r["counts"].values()) == 0 for n, r in runs.items() if n in ("n1_plain", "double_copy_each"))


# ---------------------------------------------------------------------------------------------------- (e) mutants
@pytest.mark.parametrize("name", sorted(TB.MUTANTS))
def test_each_mutant_moves_a_compared_observable_by_more_than_the_bar(runs, name):
    case_name = TB.MUTANTS[name][2]
    ratio, dist = TB.mutant_ratio(name, runs[case_name])
    print(f"{name} ({TB.MUTANTS[name][0]}) on {case_name}: {dist}, {ratio:.3g} x the bar")
    assert ratio >= PB.MUTANT_FACTOR, "the mutant is further from the restatement than the bar by the factor tests/dqn_per_bar.py asks of its own"


# ---------------------------------------------------------------------------------------------------- (f) host validation
def test_target_options_are_validated_on_the_host():
    D = importlib.import_module("cleanrl_jl_amd.dqn")      # the package attribute `dqn` is the function
    import cleanrl_jl_amd as crl
    assert crl.DQNTargetOptions is D.DQNTargetOptions
    d = D.DQNTargetOptions()
    assert (d.n_step, d.double_q) == (1, False)
    assert D._check_target(D.DQNTargetOptions(16, True)).n_step == 16 and D._check_target(D.DQNTargetOptions(np.int64(3), np.bool_(True))).double_q
    for bad in (0, 17, -1, 3.0, True, "3", None):
        with pytest.raises(ValueError, match="n_step"):
            crl.DQNAgent(crl.DQNConfig(), target=D.DQNTargetOptions(n_step=bad))
    for bad in (2, 1, 0, "yes", None):
        with pytest.raises(ValueError, match="double_q"):
            crl.DQNAgent(crl.DQNConfig(), target=D.DQNTargetOptions(double_q=bad))
    for bad in (dict(n_step=3), (3, True), 3):
        with pytest.raises(TypeError, match="DQNTargetOptions"):
            crl.DQNAgent(crl.DQNConfig(), target=bad)
