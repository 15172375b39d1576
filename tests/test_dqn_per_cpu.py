"""The anchors of tests/dqn_per_ref.py, the restatement that tests/test_gpu_dqn_per.py holds the device's prioritized replay against — no GPU.

The oracle anchor: with the draw replaced by the oracle's and unit weights the whole loop IS oracle/dqn_oracle.c, bit for bit, and with beta = 0 the
gradient on a batch with duplicates is dqn_loss_grads'. The tree: the incremental repair equals the full rebuild, the draw is proportional to the
leaves (chi-square), no slot past n is ever drawn, and the zero test is what keeps a constructed target out of the empty subtree. The schedule clips
from both sides. The bar and mutant statements of tests/dqn_per_bar.py hold on its two cheapest cases against profiles/dqn_per_bar.json."""
import json

import numpy as np
import pytest

import dqn_per_bar as B
import dqn_per_ref as P
import oraclelib as O

PER = dict(alpha=0.6, beta_start=0.4, beta_end=1.0, beta_duration=400.0, eps=1e-6)


# ---------------------------------------------------------------------------------------------------- the oracle anchor
@pytest.mark.parametrize("kw", [dict(total_timesteps=400, batch_size=31, buffer_size=64, min_buff_size=40, train_freq=3, target_net_freq=30),
                                dict(total_timesteps=150, batch_size=1, buffer_size=1, min_buff_size=1, train_freq=1, target_net_freq=1),
                                dict(total_timesteps=330, batch_size=120, buffer_size=1000, min_buff_size=200, log_frequency=7)])
def test_with_the_oracles_draw_and_unit_weights_the_loop_is_the_oracle(kw):
    cfg = O.dqn_config(**{"lr": 1e-3, "log_frequency": 1, "seed": 21, **kw})
    params = B.case_params(None)
    ref, st = P.DQNPER(cfg, PER, params, sampler=P.uniform_sampler), O.DQNState(cfg, params)
    for chunk in (1, 7, cfg.total_timesteps):
        assert ref.run(chunk) == st.run(chunk), "steps taken, episode records, logged losses"
        so, sr = st.env(), ref.status()
        assert all(so[f] == sr[f] for f in ("global_step", "rb_size", "n_updates", "last_loss")) and np.array_equal(so["state"], sr["state"])
        q, t = st.params()
        assert np.array_equal(ref.q, q) and np.array_equal(ref.t, t)
    assert ref.n_updates >= 10 and len(ref.seen) == ref.n_updates
    assert np.array_equal(ref.tree, P.build_tree(ref.leaves, ref.C)), "the tree was kept up under the foreign sampler too"
    st.close()


def test_beta_zero_gradient_on_a_batch_with_duplicates_is_the_oracles():
    rng = np.random.default_rng(5)
    k = 17
    q, t = B.case_params(None), O.dqn_params(3)
    base = dict(state=rng.standard_normal((4, 9)) * 0.1, next_state=rng.standard_normal((4, 9)) * 0.1, action=rng.integers(0, 2, 9),
                reward=rng.integers(0, 2, 9).astype(np.float64), terminal=(rng.random(9) < 0.3).astype(np.uint8))
    idx = rng.integers(0, 9, k)
    assert len(set(idx.tolist())) < k, "duplicates"
    batch = {f: (v[:, idx] if v.ndim == 2 else v[idx]) for f, v in base.items()}
    tree = P.build_tree(rng.uniform(0.1, 3.0, 9).astype(np.float32).astype(np.float64))
    w = P.weights(tree, 16, 9, idx, 0.0)
    assert (w == 1.0).all()
    loss, grad, diff = P.loss_grads(q, t, batch, 0.99, w)
    oloss, ograd = O.dqn_loss_grads(q, t, batch["state"], batch["next_state"], batch["action"], batch["reward"], batch["terminal"], 0.99)
    assert float(loss) == oloss and np.array_equal(grad.astype(np.float32), ograd)
    new = P.leaf_of(np.abs(diff), PER)
    for s in set(idx.tolist()):
        assert len(set(new[idx == s].tolist())) == 1, "duplicate indices write identical leaves"


# ---------------------------------------------------------------------------------------------------- the tree
def test_incremental_tree_equals_the_full_rebuild():
    rng = np.random.default_rng(11)
    for cap in (1, 2, 31, 64, 1000):
        C = P.tree_leaves(cap)
        assert C >= cap and C & (C - 1) == 0 and (C == 1 or C // 2 < cap)
        leaves, tree = np.zeros(cap), np.zeros(2 * C)
        for _ in range(40):
            slots = rng.integers(0, cap, int(rng.integers(1, 50)))
            vals = (2.0 ** rng.uniform(-20, 20, slots.size)).astype(np.float32).astype(np.float64)
            for s, v in zip(slots, vals):                       # duplicates: the last write wins on both sides
                leaves[s] = v; tree[C + s] = v
            P.repair(tree, C, slots)
            assert np.array_equal(tree, P.build_tree(leaves, C))
        assert tree[0] == 0.0


def test_draw_frequencies_are_proportional_to_the_leaves():
    """chi-square at the 0.1 % level, fixed seed: 200 000 stratified draws (200 updates of 1000) over 12 slots with leaves spanning 1..40"""
    leaves = np.array([1, 2, 3, 5, 8, 13, 21, 34, 40, 4, 6, 7], np.float32)
    tree = P.build_tree(leaves.astype(np.float64))
    C = P.tree_leaves(leaves.size)
    counts = np.zeros(leaves.size)
    for g in range(1, 201):
        idx = P.sample(tree, C, 0xC0FFEE, g, 1000)
        assert idx.min() >= 0 and idx.max() < leaves.size
        counts += np.bincount(idx, minlength=leaves.size)
    N = counts.sum()
    assert N == 200_000
    expect = N * leaves.astype(np.float64) / tree[1]
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    # stratification only lowers the variance of the counts below the multinomial's, so the multinomial quantile is an upper bound:
    # chi-square with 11 degrees of freedom exceeds 31.26 with probability 0.001
    print(f"chi2 = {chi2:.3f} over 11 degrees of freedom")
    assert chi2 < 31.26
    assert np.abs(counts / N - leaves / tree[1]).max() < 2e-3


@pytest.mark.parametrize("C", [2, 64, 1024])
def test_no_slot_past_n_is_ever_drawn(C):
    rng = np.random.default_rng(C)
    for n in (C // 2 + 1, C - 1):
        if n < 1 or n > C:
            continue
        leaves = (2.0 ** rng.uniform(-20, 20, n)).astype(np.float32)
        tree = P.build_tree(leaves.astype(np.float64), C)
        for g in range(1, 30):
            idx = P.sample(tree, C, 7, g, 257)
            assert idx.min() >= 0 and idx.max() < n
        for target in (tree[1], np.nextafter(tree[1], np.inf), 2.0 * tree[1], np.nextafter(tree[1], 0.0)):   # rounding put target at or past the total
            s = P.descend(tree, C, target)
            assert 0 <= s < n and leaves[s] > 0


def test_the_zero_test_is_what_keeps_a_target_at_the_total_out_of_the_empty_subtree():
    leaves = np.array([1.0, 2.0, 3.0], np.float32)              # C = 4: slot 3 is empty
    tree = P.build_tree(leaves.astype(np.float64))
    assert P.descend(tree, 4, tree[1]) == 2, "the last filled slot"
    with B.patched(**B.MUTANTS["M8"][2]()):
        assert P.descend(tree, 4, tree[1]) == 3, "without the zero test the empty slot comes back"
    half = P.build_tree(np.array([1.0, 2.0], np.float32).astype(np.float64), 4)   # n = C/2: the whole right half is empty
    assert P.descend(half, 4, half[1]) == 1
    with B.patched(**B.MUTANTS["M8"][2]()):
        assert P.descend(half, 4, half[1]) >= 2


# ---------------------------------------------------------------------------------------------------- schedule, weights, leaves
def test_beta_schedule_clips_from_both_sides():
    up = dict(beta_start=0.4, beta_end=1.0, beta_duration=100.0)
    assert P.beta_schedule(up, 0) == 0.4 and P.beta_schedule(up, 50) == (1.0 - 0.4) / 100.0 * 50.0 + 0.4
    assert P.beta_schedule(up, 100) <= 1.0 and P.beta_schedule(up, 101) == 1.0 and P.beta_schedule(up, 10 ** 9) == 1.0
    down = dict(beta_start=1.0, beta_end=0.4, beta_duration=100.0)
    assert P.beta_schedule(down, 0) == 1.0 and 0.4 < P.beta_schedule(down, 50) < 1.0
    assert P.beta_schedule(down, 101) == 0.4 and P.beta_schedule(down, 10 ** 9) == 0.4
    flat = dict(beta_start=0.7, beta_end=0.7, beta_duration=5.0)
    assert all(P.beta_schedule(flat, g) == 0.7 for g in (0, 3, 1000))
    vals = [P.beta_schedule(up, g) for g in range(0, 300)]
    assert all(a <= b for a, b in zip(vals, vals[1:]))
    import importlib
    D = importlib.import_module("cleanrl_jl_amd.dqn")      # the package attribute `dqn` is the function
    for sched in (up, down, flat):
        per = D.PEROptions(alpha=0.6, eps=1e-6, **sched)
        assert all(D.per_beta(per, g) == P.beta_schedule(sched, g) for g in (0, 1, 50, 99, 100, 101, 5000)), "the host mirror's expression"


def test_weights_and_leaves():
    tree = P.build_tree(np.array([1, 2, 4, 8], np.float32).astype(np.float64))
    w = P.weights(tree, 4, 4, np.array([0, 3, 3, 1]), 1.0)
    assert w.max() == 1.0 and w[0] == 1.0 and w[1] == w[2] == pytest.approx(0.125, rel=1e-15) and w[3] == pytest.approx(0.5, rel=1e-15)
    assert (P.weights(tree, 4, 4, np.array([0, 3]), 0.0) == 1.0).all()
    lv = P.leaf_of(np.array([0.0, 1.0, 1e40, 3.0]), dict(PER, alpha=1.0))
    assert lv[0] == np.float32(1e-6) and lv[2] == 2.0 ** 100 and lv[3] == np.float64(np.float32(3.0 + 1e-6))
    assert (P.leaf_of(np.array([0.0, 5.0, 1e300]), dict(PER, alpha=0.0)) == 1.0).all()
    assert P.leaf_of(np.array([0.0]), dict(PER, alpha=1.0, eps=1e-6))[0] > 2.0 ** -100
    assert (P.leaf_of(np.array([0.3, 7.0]), PER) == np.power(np.array([0.3, 7.0]) + 1e-6, 0.6).astype(np.float32)).all()


# ---------------------------------------------------------------------------------------------------- the bar
@pytest.fixture(scope="module")
def prof():
    return json.load(open(B.BAR_JSON))


def test_profile_states_the_bars_and_every_case(prof):
    assert prof["loss_bar"] == B.LOSS_FACTOR * prof["loss_floor"] and prof["param_bar"] == B.PARAM_BAR and prof["jitter_ulp"] == B.JITTER_ULP == 16
    assert set(prof["cases"]) == set(B.CASE) and prof["loss_floor"] == max(rec["floor"]["loss"] for rec in prof["cases"].values())
    for name, rec in prof["cases"].items():
        assert rec["ties_ok"], f"{name}: a jittered twin left the reference's idx or leaves — change the case's seed"
        assert all(rec["floor"][p] == 0.0 for p in B.PARAMS)
        assert all(r >= B.MUTANT_FACTOR for r in rec["mutant_ratio"].values()), name
        assert rec["seed"] == B.CASE[name]["seed"]
    for m, rec in prof["mutants"].items():
        assert rec["cases"] >= 1 or (m == "M8" and rec["unobservable"]), m
    assert all(rec["stats"]["zero_saves"] == 0 for rec in prof["cases"].values())
    assert any(rec["stats"]["duplicates"] > 0 for rec in prof["cases"].values()), "draws are with replacement"


@pytest.mark.parametrize("name", B.CHEAPEST)
def test_bar_and_mutants_hold_on_the_cheapest_cases(prof, name):
    got, rec = B.measure(B.CASE[name]), prof["cases"][name]
    assert got["ties_ok"] and got["stats"] == rec["stats"]
    assert got["floor"] == rec["floor"], "seeded: the recomputed floor is the recorded one"
    assert sorted(got["mutants"]) == sorted(rec["mutants"])
    assert got["floor"]["loss"] <= prof["loss_floor"] and all(got["floor"][p] == 0.0 for p in B.PARAMS)
    for m, dist in got["mutants"].items():
        assert B.mutant_ratio(dist, prof["loss_bar"]) >= B.MUTANT_FACTOR, (name, m, dist)
