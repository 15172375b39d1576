"""Categorical (C51) DQN on the GPU (crl_dqn_c51_create; csrc/dqn_c51.hpp and the dqn_c51_*_kernel family of csrc/dqn.hip) against the numpy
restatement tests/c51_ref.py, on the case table of tests/c51_bar.py.

What is bit-equal and what is under a bar. exp and log are the feature's two transcendentals, and nobody has measured how far the device's lie from
numpy's, so everything downstream of them sits under the bars of profiles/c51_bar.json (measured on the CPU from the restatement's own jitter floor,
never from the device): the logged losses, loss_j and the projected targets m. Everything that is a DECISION or has no transcendental in it is
bit-equal: the episodes (hence every greedy action), idx, last, the steps summed, R, disc, a*, and under PER the Float32 leaves and the tree. The
parameters sit under ddpg_bar.PARAM_BAR; how many cases came out bit-equal in them is printed. The projection probe runs no transcendental at all and
is bit-equal to the restatement."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import c51_bar as B
import c51_ref as Z
import dqn_per_bar as PB
import dqn_target_bar as TB
import dqn_target_ref as T
import oraclelib as O
import value_eval_ref as V
from test_c51_cpu import hand_made_rows

pytestmark = pytest.mark.gpu

BIT_EQUAL = {}                                             # case → were both parameter arrays bit-equal (printed by the last table case)


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


@pytest.fixture(scope="module")
def bars():
    return B.load_bars()


def _crl_cfg(L, ocfg):
    assert [f for f, _ in L.CrlDQNConfig._fields_] == [f for f, _ in O.DQNConfigC._fields_]
    return L.CrlDQNConfig(*[getattr(ocfg, f) for f, _ in O.DQNConfigC._fields_])


def _handle(crl, ocfg, per, tgt, c51, params=None):
    L = crl._lib
    h = L.DQNHandle(_crl_cfg(L, ocfg), 0,
                    per=None if per is None else L.CrlDQNPEROptions(per["alpha"], per["beta_start"], per["beta_end"], per["beta_duration"], per["eps"]),
                    target=None if tgt is None else L.CrlDQNTargetOptions(int(tgt["n_step"]), int(tgt["double_q"])),
                    c51=L.CrlDQNC51Options(int(c51["n_atoms"]), 0, float(c51["v_min"]), float(c51["v_max"])))
    if params is not None:
        h.write_params(params)
    return h


def _case_handle(crl, case):
    return _handle(crl, B.case_cfg(case), B.case_per(case), B.case_tgt(case), B.case_c51(case), B.case_params(case))


# ---------------------------------------------------------------------------------------------------- the projection alone
@pytest.mark.parametrize("N", [2, 51, 64])
def test_projection_probe_is_bit_equal_to_the_restatement(crl, N):
    for v_min, v_max in ((0.0, 100.0), (1.0, 5.0)):
        c51 = dict(n_atoms=N, v_min=v_min, v_max=v_max)
        h = _handle(crl, O.dqn_config(seed=21), None, None, c51)
        for k in (1, 65):
            pp, R_, disc, term = hand_made_rows(N, k, v_min, v_max, seed=k)
            got = h.c51_project_probe(pp, R_, disc, term)
            want = Z.project(pp, R_, disc, term, c51)
            assert np.array_equal(got, want), (N, k, v_min, v_max, np.abs(got - want).max())
            assert np.all(np.abs(got.sum(axis=0) - 1.0) <= 2 * N * np.spacing(1.0))
        h.close()


# ---------------------------------------------------------------------------------------------------- the case table
def _compare(h, ref, case, losses, ref_losses, bars, label):
    N = B.case_c51(case)["n_atoms"]
    sg, so = h.status(), ref.status()
    for f in ("global_step", "rb_size", "n_updates"):
        assert sg[f] == so[f], (label, f, sg[f], so[f])
    assert np.array_equal(sg["state"], so["state"]), (label, "env state")
    qg, tg = h.read_params()
    if so["n_updates"] == 0:
        assert np.array_equal(qg, ref.q) and np.array_equal(tg, ref.t)
        return None
    got, want, r = h.target_read(), ref.target_read(), h.c51_read()
    for f in ("last", "m", "nret", "ndisc", "astar"):
        assert np.array_equal(got[f], want[f]), (label, f)
    if case["per"]:
        pr = h.per_read()
        pg, po = h.per_status(), ref.per_status()
        assert np.array_equal(pr["idx"], ref.idx), (label, "idx")
        assert np.array_equal(pr["leaves"], ref.leaves.astype(np.float32)) and np.array_equal(pr["tree"], ref.tree), (label, "leaves and tree")
        assert pg["beta"] == po["beta"] and pg["max_leaf"] == po["max_leaf"] and pg["total"] == po["total"], (label, pg, po)
        assert np.abs(pr["abs_td"] - ref.sample_loss).max() <= bars["loss"] * np.abs(ref.sample_loss).max(), (label, "abs_td holds loss_j")
    elif B.case_tgt(case)["n_step"] == 1:
        assert np.array_equal(got["last"], ref.idx), (label, "with one step the bootstrap slot is the drawn slot: idx")
    dist = B.distances(losses, (qg, tg), r["proj"], ref_losses, (ref.q, ref.t), ref.proj, N)
    sl = float(np.abs(r["sample_loss"] - ref.sample_loss).max() / np.abs(ref.sample_loss).max())
    ll = abs(sg["last_loss"] - so["last_loss"]) / abs(so["last_loss"])
    td = float(np.abs(got["td"] - want["td"]).max() / max(np.abs(want["td"]).max(), 1.0))
    exact = np.array_equal(qg, ref.q) and np.array_equal(tg, ref.t)
    print(f"{case['name']} {label}: {so['n_updates']} updates; loss {dist['loss']:.3e}, last_loss {ll:.3e}, loss_j {sl:.3e}, td {td:.3e} (bar "
          f"{bars['loss']:.3e}); proj {dist['proj']:.3e} (bar {bars['proj']:.3e}); q {dist['q']:.3e}, target {dist['target']:.3e} (bar "
          f"{bars['q']:.3e}); parameters bit-equal: {exact}")
    assert np.all(r["sample_loss"] >= 0.0) and np.all(r["proj"] >= 0.0)
    assert dist["loss"] <= bars["loss"] and ll <= bars["loss"] and sl <= bars["loss"] and td <= bars["loss"]
    assert dist["proj"] <= bars["proj"]
    assert dist["q"] <= bars["q"] and dist["target"] <= bars["target"]
    return exact


@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_case_table_matches_the_restatement(crl, bars, name):
    case = B.CASE[name]
    cfg = B.case_cfg(case)
    h, ref = _case_handle(crl, case), B.make_ref(case)
    assert h.param_count() == Z.param_count(B.case_c51(case)["n_atoms"])
    Tn = cfg.total_timesteps
    losses, ref_losses, total, exact = [], [], 0, None
    for chunk in PB.CHUNKS + (Tn,):
        tg, eps_g, ls_g = h.run(chunk)
        to, eps_o, ls_o = ref.run(chunk)
        total += tg
        assert tg == to and eps_g == eps_o, "same trajectories, same episode records (return, length, step, ϵ): every greedy action agreed"
        losses += ls_g; ref_losses += ls_o
        if ref_losses or ref.n_updates == 0:
            exact = _compare(h, ref, case, losses, ref_losses, bars, f"after {total} steps")
    steps = PB.update_steps(cfg)
    assert total == Tn and h.status()["n_updates"] == len(steps) >= 3
    assert len(losses) == len([g for g in steps if g % cfg.log_frequency == 0]) > 0
    assert not np.array_equal(h.read_params()[0], B.case_params(case))
    assert len(ref.greedy) > 0, "the run acted greedily on the expected values"
    BIT_EQUAL[name] = bool(exact)
    if name == B.CASES[-1]["name"]:
        print(f"cases whose parameters came out bit-equal: {sum(BIT_EQUAL.values())} of {len(BIT_EQUAL)}: {sorted(n for n, e in BIT_EQUAL.items() if e)}")
    h.close()


# ---------------------------------------------------------------------------------------------------- the public calls agree with each other
def test_q_values_probs_and_evaluation_are_one_computation(crl, bars):
    case = B.CASE["per_n3_double"]
    cfg = B.case_cfg(case)
    c51 = B.case_c51(case)
    N = c51["n_atoms"]
    h, ref = _case_handle(crl, case), B.make_ref(case)
    h.run(cfg.total_timesteps)
    ref.run(cfg.total_timesteps)
    before = (h.per_read(), h.target_read(), h.c51_read(), h.per_status(), h.status(), h.read_params())
    n_envs = 2 * crl._lib.dqn_eval_envs_per_block() + 1
    ev = h.evaluate(n_envs, 2, seed=3, trace_steps=4)
    assert ev["report"]["episodes"] == 2 * n_envs
    # the first observation of every evaluation episode, as the kernel resets it
    obs = np.stack([V.reset(3, j * n_envs + e) for j in range(2) for e in range(n_envs)], axis=1)
    X = np.concatenate([obs, np.random.default_rng(5).uniform(-2.4, 2.4, (4, 28))], axis=1)
    q, p = h.q_values(X), h.c51_probs(X)
    assert p.shape == (N, 2, X.shape[1]) and q.shape == (2, X.shape[1])
    z = Z.atoms(c51)[0]
    for a in range(2):
        assert np.array_equal(q[a], Z.sum_atoms(z[:, None] * p[:, a, :])), "crl_dqn_q_values is Σ z·p of crl_dqn_c51_probs, bit for bit"
        assert np.all(np.abs(Z.sum_atoms(p[:, a, :]) - 1.0) <= N * np.spacing(1.0)), "every row of probs sums to 1 within N ulp"
    assert np.all(p > 0.0)
    rq, rp = ref.q_values(X), ref.probs(X)
    print(f"q_values against the restatement: {np.abs(q - rq).max() / np.abs(rq).max():.3e}; probs: {np.abs(p - rp).max():.3e}")
    assert np.abs(p - rp).max() <= bars["proj"] and np.abs(q - rq).max() <= bars["loss"] * np.abs(rq).max()
    n0 = obs.shape[1]
    act = np.where(q[1, :n0] > q[0, :n0], 1, 0).reshape(2, n_envs)
    assert np.array_equal(ev["trace_action"][0], act[0]), "evaluation's first actions are the argmax of crl_dqn_q_values, bit for bit"
    assert np.array_equal(ev["q0"], q[act.reshape(-1), np.arange(n0)].reshape(2, n_envs)), "and every v0 is its value, bit for bit"
    after = (h.per_read(), h.target_read(), h.c51_read(), h.per_status(), h.status(), h.read_params())
    for b, a in zip(before[:3], after[:3]):
        assert all(np.array_equal(b[f], a[f]) for f in b)
    assert before[3] == after[3] and all(np.array_equal(before[4][f], after[4][f]) for f in before[4])
    assert np.array_equal(before[5][0], after[5][0]) and np.array_equal(before[5][1], after[5][1]), "evaluation leaves every training array untouched"
    h.close()


# ---------------------------------------------------------------------------------------------------- the other handles
def test_old_handles_are_unchanged_beside_a_c51_handle(crl):
    """in one process, interleaved with a running C51 handle: a crl_dqn_create handle is still bit-identical to oracle/dqn_oracle.c and a
    crl_dqn_create_with handle to dqn_target_ref; the c51_* calls fail on both with a message naming crl_dqn_c51_create"""
    L = crl._lib
    c51case = B.CASE["per_n3_double"]
    hc = _case_handle(crl, c51case)
    case = PB.CASE["k61_cap64"]
    cfg, params = PB.case_cfg(case), PB.case_params(case)
    h = L.DQNHandle(_crl_cfg(L, cfg), 0)
    h.write_params(params)
    st = O.DQNState(cfg, params)
    tcase = TB.CASE["n3_double"]
    tcfg, tparams = TB.case_cfg(tcase), TB.case_params(tcase)
    assert TB.case_per(tcase) is None
    ht = L.DQNHandle(_crl_cfg(L, tcfg), 0, target=L.CrlDQNTargetOptions(int(tcase["tgt"]["n_step"]), int(tcase["tgt"]["double_q"])))
    ht.write_params(tparams)
    rt = T.DQNTarget(tcfg, None, tcase["tgt"], tparams)
    for chunk in (1, 7, max(cfg.total_timesteps, tcfg.total_timesteps)):
        hc.run(chunk)
        assert h.run(chunk) == st.run(chunk)
        sg, so = h.status(), st.env()
        assert all(sg[f] == so[f] for f in ("global_step", "rb_size", "n_updates", "last_loss")) and np.array_equal(sg["state"], so["state"])
        qg, tg = h.read_params(); qo, to = st.params()
        assert np.array_equal(qg, qo) and np.array_equal(tg, to)
        assert ht.run(chunk) == rt.run(chunk)
        qg, tg = ht.read_params()
        assert np.array_equal(qg, rt.q) and np.array_equal(tg, rt.t) and ht.status()["last_loss"] == rt.status()["last_loss"]
        got, want = ht.target_read(), rt.target_read()
        assert all(np.array_equal(got[f], want[f]) for f in TB.TARGET_ARRAYS)
    assert h.status()["n_updates"] >= 3 and ht.status()["n_updates"] >= 3 and hc.status()["n_updates"] >= 3
    assert h.param_count() == ht.param_count() == L.DQN_PARAM_COUNT
    for old in (h, ht):
        for call in (lambda: old.c51_probs(np.zeros(4)), old.c51_read, lambda: old.c51_project_probe(np.ones((1, 1)), np.ones(1), np.ones(1), np.zeros(1))):
            with pytest.raises(crl.CrlError, match="crl_dqn_c51_create"):
                call()
    h.close(); ht.close(); hc.close(); st.close()


def test_c51_handles_of_different_heads_live_side_by_side(crl):
    """the dynamic LDS size is a property of the kernel, not of the handle: a handle with the largest head still runs and evaluates after one with the
    smallest was made, to the bits of a run on its own"""
    big, small = B.CASE["n64"], B.CASE["n2"]
    cfg = B.case_cfg(big)
    alone = _case_handle(crl, big)
    alone.run(cfg.total_timesteps)
    want, want_ev = alone.read_params(), alone.evaluate(5, 1, seed=3)
    alone.close()
    h64, h2 = _case_handle(crl, big), _case_handle(crl, small)
    for chunk in (150, 150):
        h2.run(chunk); h64.run(chunk)
    got, got_ev = h64.read_params(), h64.evaluate(5, 1, seed=3)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got_ev["q0"], want_ev["q0"]) and np.array_equal(got_ev["returns"], want_ev["returns"])
    assert h2.status()["n_updates"] == h64.status()["n_updates"] == 20 and h2.evaluate(5, 1, seed=3)["report"]["episodes"] == 5
    h64.close(); h2.close()


def test_errors(crl):
    L = crl._lib
    cfg = O.dqn_config(seed=21)
    good = dict(n_atoms=51, v_min=0.0, v_max=100.0)
    for bad, field in ((dict(n_atoms=1), "n_atoms"), (dict(n_atoms=65), "n_atoms"), (dict(v_min=100.0), "v_min"), (dict(v_min=101.0), "v_min"),
                       (dict(v_max=float("inf")), "v_max"), (dict(v_min=float("-inf")), "v_min"), (dict(v_max=float("nan")), "v_max"),
                       (dict(v_min=float("nan")), "v_min")):
        with pytest.raises(crl.CrlError, match=field):
            _handle(crl, cfg, None, None, {**good, **bad})
    with pytest.raises(crl.CrlError, match="n_step"):
        _handle(crl, cfg, None, dict(n_step=17, double_q=0), good)
    with pytest.raises(crl.CrlError, match="alpha"):
        _handle(crl, cfg, dict(alpha=2.0, beta_start=0.4, beta_end=1.0, beta_duration=10.0, eps=1e-6), None, good)
    lib, out = L.load(), C.c_void_p()
    ccfg, copt = _crl_cfg(L, cfg), L.CrlDQNC51Options(51, 0, 0.0, 100.0)
    for args in ((None, C.byref(copt), None, None, 0, C.byref(out)), (C.byref(ccfg), None, None, None, 0, C.byref(out)),
                 (C.byref(ccfg), C.byref(copt), None, None, 0, None)):
        assert lib.crl_dqn_c51_create(*args) != 0 and b"null" in lib.crl_last_error()
    assert lib.crl_dqn_c51_create(C.byref(ccfg), C.byref(copt), None, None, 0, C.byref(out)) == 0, "per NULL = uniform, tgt NULL = {1, 0}"
    n = C.c_size_t()
    assert lib.crl_dqn_param_count(out, C.byref(n)) == 0 and n.value == 19434
    assert lib.crl_dqn_param_count(out, None) != 0 and lib.crl_dqn_param_count(None, C.byref(n)) != 0
    assert lib.crl_dqn_c51_read(out, None, None) == 0, "either pointer may be NULL"
    assert lib.crl_dqn_c51_probs(out, None, 1, None) != 0
    assert lib.crl_dqn_c51_project_probe(out, None, None, None, None, 1, None) != 0 and b"null" in lib.crl_last_error()
    assert lib.crl_dqn_destroy(out) == 0
    h = _handle(crl, cfg, None, None, good)
    with pytest.raises(crl.CrlError, match="parameters not set"):
        h.run(10)
    with pytest.raises(crl.CrlError, match="parameters not set"):
        h.c51_probs(np.zeros(4))
    for size in (L.DQN_PARAM_COUNT, 19433, 19435):
        with pytest.raises(crl.CrlError, match="expected 19434 floats"):
            h.write_params(np.zeros(size, np.float32))
    with pytest.raises(crl.CrlError, match="k must"):
        h.c51_project_probe(np.ones((51, 1025)), np.ones(1025), np.ones(1025), np.zeros(1025, np.uint8))
    h.init_params(3)
    q, t = h.read_params()
    assert q.size == 19434 and np.array_equal(q, t) and np.array_equal(q, L.dqn_c51_make_nn_host(3, 51))
    assert np.array_equal(q[:Z.TRUNK], L.dqn_make_nn_host(3)[:Z.TRUNK]), "crl_dqn_make_nn's trunk for the same seed"
    with pytest.raises(crl.CrlError, match="n_atoms"):
        L.dqn_c51_make_nn_host(0, 65)
    plain = L.DQNHandle(_crl_cfg(L, cfg), 0)
    with pytest.raises(crl.CrlError, match="expected 10934 floats"):
        plain.write_params(np.zeros(19434, np.float32))
    plain.close(); h.close()


# ---------------------------------------------------------------------------------------------------- the entry point
def _records(path):
    return [json.loads(l) for l in open(path)]


def test_entry_point_logs_and_is_repeatable(crl, tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / str(i); d.mkdir()
        cfg = crl.DQNConfig(run_name="t", total_timesteps=2500)
        agent = crl.dqn(cfg, dist=crl.C51Options(), seed=9, chunk=700, eval_every=1250, eval_envs=16, to_terminal=False, to_json=True,
                        to_tensorboard=False, log_dir=str(d))
        assert agent.handle.status()["global_step"] == 2500 and agent.handle.param_count() == 19434
        recs = _records(os.path.join(d, "dqn|t.json"))
        tr = [r for r in recs if r["msg"] == "Training Statistics"]
        ev = [{k: v for k, v in r.items() if k not in ("time", "timestamp")} for r in recs if r["msg"] == "Evaluation Statistics"]
        ep = [{k: v for k, v in r.items() if k not in ("steps_per_sec", "time", "timestamp")} for r in recs if r["msg"] == "Episode Statistics"]
        runs.append((tr, ep, ev, agent.handle.read_params(), agent.handle.c51_read()))
        agent.close()
    (tr_a, ep_a, ev_a, p_a, c_a), (tr_b, ep_b, ev_b, p_b, c_b) = runs
    assert len(tr_a) == 2 and all(r["loss"] > 0.0 and "beta" not in r for r in tr_a), "the loss record carries the cross-entropy"
    assert [r["loss"] for r in tr_a] == [r["loss"] for r in tr_b] and len(ep_a) == len(ep_b) > 0
    assert [r["episode_return"] for r in ep_a] == [r["episode_return"] for r in ep_b]
    assert len(ev_a) == 2 and [r["eval_return_mean"] for r in ev_a] == [r["eval_return_mean"] for r in ev_b]
    assert [r["eval_q_bias"] for r in ev_a] == [r["eval_q_bias"] for r in ev_b]
    assert np.array_equal(p_a[0], p_b[0]) and np.array_equal(p_a[1], p_b[1]) and all(np.array_equal(c_a[f], c_b[f]) for f in c_a)
    assert np.all(np.abs(c_a["proj"].sum(axis=0) - 1.0) <= 1e-12)


LEARN_JSON = os.path.join(B.B.ROOT, "profiles", "c51_learn.json")
LEARN_SEEDS = (1, 2, 3)


def test_c51_agent_learns(crl):
    """After 20,000 steps at lr = 1e-3 (the step count and the rate of test_per_agent_learns, for its reasons) dqn_evaluate of the agent with
    C51Options() returns strictly more than the same evaluation of its initial network. Measured first (scripts/c51_learn.py →
    profiles/c51_learn.json, eight seeds); the seeds run here are taken from those the profile shows learning."""
    prof = json.load(open(LEARN_JSON))
    rows = prof["runs"]["c51"]
    assert prof["steps"] == 20_000 and prof["lr"] == 1e-3 and len(rows) == 8
    learned = [s for s, r in rows.items() if r[-1] > r[0]]
    print(f"seeds that learned in the profile: {sorted(learned)} of 8")
    assert all(str(s) in learned for s in LEARN_SEEDS)
    for seed in LEARN_SEEDS:
        agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=20_000, lr=1e-3), seed=seed, init_seed=seed, dist=crl.C51Options())
        before = crl.dqn_evaluate(agent, num_envs=256)["report"]["return_mean"]
        agent.handle.run(20_000)
        after = crl.dqn_evaluate(agent, num_envs=256)["report"]["return_mean"]
        print(f"seed {seed}: held-out return_mean {before} -> {after}")
        assert agent.handle.status()["global_step"] == 20_000 and after > before
        assert before == rows[str(seed)][0], "the recorded run's initial network"
        agent.close()
