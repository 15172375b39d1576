"""n-step returns and double Q-learning for DQN on the GPU (crl_dqn_create_with; csrc/dqn_target.hpp, dqn_tgt_sample_kernel and dqn_td_kernel<true, PER>
in csrc/dqn.hip) against the numpy restatement tests/dqn_target_ref.py, on the case table of tests/dqn_target_bar.py.

What is bit-equal and what is under a bar. A uniform case holds no transcendental anywhere: the episodes, the status with last_loss, every loss
record, both parameter arrays and target_read's arrays are the restatement's bit for bit. A PER case has one rounding freedom, PER's pow, so it sits
under the existing bars of tests/dqn_per_bar.py (profiles/dqn_per_bar.json) — no new bar: the tree, idx, the Float32 leaves, last, m, nret, ndisc and
astar are bit-equal, the losses, the weights, td and the parameters under the bars; whether the parameters were in fact bit-equal is printed.

crl_dqn_target_read returns six arrays (last, m, nret, ndisc, astar, td); idx, the seventh thing an update leaves, is read through crl_dqn_per_read
on the PER cases and is implied by `last` where m == 1 on the others."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import dqn_per_bar as PB
import dqn_per_ref as P
import dqn_target_bar as TB
import dqn_target_ref as T
import oraclelib as O

pytestmark = pytest.mark.gpu

SEED = 21


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


@pytest.fixture(scope="module")
def bars():
    return PB.load_bars()


def _crl_cfg(L, ocfg):
    assert [f for f, _ in L.CrlDQNConfig._fields_] == [f for f, _ in O.DQNConfigC._fields_]
    return L.CrlDQNConfig(*[getattr(ocfg, f) for f, _ in O.DQNConfigC._fields_])


def _per_opts(L, per):
    return None if per is None else L.CrlDQNPEROptions(per["alpha"], per["beta_start"], per["beta_end"], per["beta_duration"], per["eps"])


def _handle(crl, ocfg, per, tgt, params=None):
    L = crl._lib
    h = L.DQNHandle(_crl_cfg(L, ocfg), 0, per=_per_opts(L, per), target=L.CrlDQNTargetOptions(int(tgt["n_step"]), int(tgt["double_q"])))
    if params is not None:
        h.write_params(params)
    return h


PER = dict(alpha=0.6, beta_start=0.4, beta_end=1.0, beta_duration=1000.0, eps=1e-6)
N3D = dict(n_step=3, double_q=True)


@pytest.fixture(scope="module")
def prober(crl):
    h = _handle(crl, O.dqn_config(seed=SEED), None, N3D)
    yield h
    h.close()


# ---------------------------------------------------------------------------------------------------- the walk alone
def _ring(cap, ptr, n_step, k, rng, terminals):
    """a hand-made full ring. With `terminals`: sparse random ones, then for three drawn slots a terminal at the first, a middle and the last slot of
    their window; without: none at all (on the smallest rings the placed terminals would end every walk). idx holds those three slots, the newest
    slot, the oldest, slot 0 and slot cap − 1, the rest random (duplicates allowed)"""
    reward = rng.standard_normal(cap)
    terminal = (rng.random(cap) < 0.05).astype(np.uint8) if terminals else np.zeros(cap, np.uint8)
    starts = [int(s) for s in rng.integers(0, cap, 3)]
    for s, off in zip(starts, (0, n_step // 2, n_step - 1)):
        terminal[(s + off) % cap] = 1 if terminals else 0
    special = starts + [(ptr - 1) % cap, ptr, 0, cap - 1]
    idx = np.concatenate([np.array(special, np.int64), rng.integers(0, cap, max(k - len(special), 0))])[:k].astype(np.int32)
    if k >= 4:
        assert (ptr - 1) % cap in idx.tolist(), "the newest slot is drawn"
    return reward, terminal, idx


@pytest.mark.parametrize("cap", [1, 2, 31, 64, 65536])
def test_nstep_probe_matches_the_restatements_walk(prober, cap):
    rng = np.random.default_rng(cap)
    T.reset_counts()
    for ptr in sorted({0, cap // 2, cap - 1}):
        for n_step in (1, 16):
            for k in (1, 31, 1024):
                for gamma, terminals in ((0.99, True), (0.99, False), (0.0, True)):
                    reward, terminal, idx = _ring(cap, ptr, n_step, k, rng, terminals)
                    got = prober.nstep_probe(reward, terminal, ptr, idx, n_step, gamma)
                    last, m, nret, ndisc = T.walk_batch(reward, terminal, cap, ptr, idx, n_step, gamma)
                    label = (cap, ptr, n_step, k, gamma, terminals)
                    assert np.array_equal(got["last"], last) and np.array_equal(got["m"], m), label
                    assert np.array_equal(got["nret"], nret) and np.array_equal(got["ndisc"], ndisc), label
                    assert got["m"].min() >= 1 and got["m"].max() <= min(n_step, cap) and 0 <= got["last"].min() and got["last"].max() < cap
    print(f"cap {cap}: {T.COUNTS}")
    assert T.COUNTS["head_stops"] > 0 and T.COUNTS["terminal_stops"] > 0 and (cap == 1 or T.COUNTS["wraps"] > 0)


def test_nstep_probe_on_a_ring_that_is_not_full(prober):
    """ptr = size < cap: the slots from ptr on are empty and the walk never reaches them"""
    rng = np.random.default_rng(3)
    cap, ptr = 64, 20
    reward, terminal = rng.standard_normal(cap), np.zeros(cap, np.uint8)
    idx = np.arange(ptr, dtype=np.int32)
    got = prober.nstep_probe(reward, terminal, ptr, idx, 16, 0.5)
    last, m, nret, ndisc = T.walk_batch(reward, terminal, cap, ptr, idx, 16, 0.5)
    assert np.array_equal(got["last"], last) and np.array_equal(got["m"], m) and np.array_equal(got["nret"], nret) and np.array_equal(got["ndisc"], ndisc)
    assert got["last"].max() == ptr - 1 and np.array_equal(got["m"], np.minimum(16, ptr - np.arange(ptr)))


# ---------------------------------------------------------------------------------------------------- the case table
def _check_uniform(h, ref, losses, ref_losses, label):
    sg, so = h.status(), ref.status()
    for f in ("global_step", "rb_size", "n_updates", "last_loss"):
        assert sg[f] == so[f], (label, f, sg[f], so[f])
    assert np.array_equal(sg["state"], so["state"]), (label, "env state")
    assert losses == ref_losses, (label, "every loss record, bit for bit")
    qg, tg = h.read_params()
    assert np.array_equal(qg, ref.q) and np.array_equal(tg, ref.t), (label, "both parameter arrays, bit for bit")
    got, want = h.target_read(), ref.target_read()
    for f in TB.TARGET_ARRAYS:
        assert np.array_equal(got[f], want[f]), (label, f)


def _check_per(h, ref, losses, ref_losses, loss_bar, param_bar, name, label):
    sg, so = h.status(), ref.status()
    for f in ("global_step", "rb_size", "n_updates"):
        assert sg[f] == so[f], (label, f)
    assert np.array_equal(sg["state"], so["state"]), (label, "env state")
    qg, tg = h.read_params()
    got, want, r = h.target_read(), ref.target_read(), h.per_read()
    if so["n_updates"] == 0:
        assert np.array_equal(qg, ref.q) and np.array_equal(tg, ref.t) and not any(got[f].any() for f in got)
        return
    pg, po = h.per_status(), ref.per_status()
    assert pg["beta"] == po["beta"] and pg["max_leaf"] == po["max_leaf"] and pg["total"] == po["total"], (label, pg, po)
    assert np.array_equal(r["idx"], ref.idx), (label, "idx")
    assert np.array_equal(r["leaves"], ref.leaves.astype(np.float32)) and np.array_equal(r["tree"], ref.tree), (label, "leaves and tree")
    for f in ("last", "m", "nret", "ndisc", "astar"):
        assert np.array_equal(got[f], want[f]), (label, f)
    wd = np.abs(r["weight"] - ref.w).max()
    tdd = np.abs(got["td"] - want["td"]).max() / np.abs(want["td"]).max()
    ll = abs(sg["last_loss"] - so["last_loss"]) / abs(so["last_loss"])
    dist = PB.distances(losses, (qg, tg), ref_losses, (ref.q, ref.t))
    exact = np.array_equal(qg, ref.q) and np.array_equal(tg, ref.t)
    print(f"{name} {label}: {so['n_updates']} updates; loss {dist['loss']:.3e}, last_loss {ll:.3e}, weights {wd:.3e}, td {tdd:.3e} (bar {loss_bar:.3e}); "
          f"q {dist['q']:.3e}, target {dist['target']:.3e} (bar {param_bar:.3e}); parameters bit-equal: {exact}")
    assert wd <= loss_bar and ll <= loss_bar and dist["loss"] <= loss_bar and tdd <= loss_bar
    assert dist["q"] <= param_bar and dist["target"] <= param_bar


@pytest.mark.parametrize("name", [c["name"] for c in TB.CASES])
def test_case_table_matches_the_restatement(crl, bars, name):
    loss_bar, param_bar = bars
    case = TB.CASE[name]
    cfg, per, params = TB.case_cfg(case), TB.case_per(case), TB.case_params(case)
    h = _handle(crl, cfg, per, case["tgt"], params)
    ref = T.DQNTarget(cfg, per, case["tgt"], params)
    Tn = cfg.total_timesteps
    losses, ref_losses, total = [], [], 0
    for chunk in TB.CHUNKS + (Tn,):
        tg, eps_g, ls_g = h.run(chunk)
        to, eps_o, ls_o = ref.run(chunk)
        total += tg
        assert tg == to and eps_g == eps_o, "same trajectories, same episode records (return, length, step, ϵ)"
        losses += ls_g; ref_losses += ls_o
        if per is None:
            _check_uniform(h, ref, losses, ref_losses, f"{name} after {total} steps")
        elif ref_losses or ref.n_updates == 0:
            _check_per(h, ref, losses, ref_losses, loss_bar, param_bar, name, f"after {total} steps")
    steps = PB.update_steps(cfg)
    assert total == Tn and h.status()["n_updates"] == len(steps) >= 3 and len(losses) == len(steps)
    assert not np.array_equal(h.read_params()[0], params)
    h.close()


@pytest.mark.parametrize("name", ["n1_plain", "double_copy_each"])
def test_the_one_step_cases_are_the_plain_handle_and_the_oracle(crl, name):
    """{1, 0}, and double_q with a target copied at every update, through the new kernels: bit for bit a crl_dqn_create handle and oracle/dqn_oracle.c"""
    case = TB.CASE[name]
    cfg, params = TB.case_cfg(case), TB.case_params(case)
    L = crl._lib
    hn, hp, st = _handle(crl, cfg, None, case["tgt"], params), L.DQNHandle(_crl_cfg(L, cfg), 0), O.DQNState(cfg, params)
    hp.write_params(params)
    for chunk in (1, 7, cfg.total_timesteps):
        rn, rp, ro = hn.run(chunk), hp.run(chunk), st.run(chunk)
        assert rn == rp == ro, "steps, episode records, loss records"
        sn, sp, so = hn.status(), hp.status(), st.env()
        assert all(sn[f] == sp[f] == so[f] for f in ("global_step", "rb_size", "n_updates", "last_loss"))
        assert np.array_equal(sn["state"], sp["state"]) and np.array_equal(sn["state"], so["state"])
        (qn, tn), (qp, tp), (qo, to) = hn.read_params(), hp.read_params(), st.params()
        assert np.array_equal(qn, qp) and np.array_equal(tn, tp) and np.array_equal(qn, qo) and np.array_equal(tn, to)
    assert hn.status()["n_updates"] == 20 and (hn.target_read()["m"] == 1).all()
    hn.close(); hp.close(); st.close()


# ---------------------------------------------------------------------------------------------------- the other paths
def test_new_handles_leave_the_old_paths_alone(crl, bars):
    """in one process: new handles run (uniform and PER), then a crl_dqn_create handle still matches the C oracle bit for bit and a crl_dqn_per_create
    handle its restatement; the two new calls fail on both with a message naming crl_dqn_create_with"""
    loss_bar, param_bar = bars
    case = PB.CASE["k61_cap64"]
    cfg, per, params = PB.case_cfg(case), PB.case_per(case), PB.case_params(case)
    for p in (None, per):
        hn = _handle(crl, cfg, p, N3D, params)
        hn.run(cfg.total_timesteps)
        assert hn.status()["n_updates"] >= 3
        hn.close()
    L = crl._lib
    h = L.DQNHandle(_crl_cfg(L, cfg), 0)
    h.write_params(params)
    st = O.DQNState(cfg, params)
    for chunk in (1, 7, cfg.total_timesteps):
        assert h.run(chunk) == st.run(chunk)
        sg, so = h.status(), st.env()
        assert all(sg[f] == so[f] for f in ("global_step", "rb_size", "n_updates", "last_loss")) and np.array_equal(sg["state"], so["state"])
        qg, tg = h.read_params(); qo, to = st.params()
        assert np.array_equal(qg, qo) and np.array_equal(tg, to)
    hp = L.DQNHandle(_crl_cfg(L, cfg), 0, per=_per_opts(L, per))
    hp.write_params(params)
    ref = P.DQNPER(cfg, per, params)
    rg, ro = hp.run(cfg.total_timesteps), ref.run(cfg.total_timesteps)
    assert rg[:2] == ro[:2]
    r = hp.per_read()
    assert np.array_equal(r["idx"], ref.idx) and np.array_equal(r["tree"], ref.tree) and np.array_equal(r["leaves"], ref.leaves.astype(np.float32))
    dist = PB.distances(rg[2], hp.read_params(), ro[2], (ref.q, ref.t))
    assert dist["loss"] <= loss_bar and dist["q"] <= param_bar and dist["target"] <= param_bar, dist
    for old in (h, hp):
        for call in (old.target_read, lambda: old.nstep_probe(np.ones(4), np.zeros(4, np.uint8), 0, np.zeros(2, np.int32), 3, 0.9)):
            with pytest.raises(crl.CrlError, match="crl_dqn_create_with"):
                call()
    with pytest.raises(crl.CrlError, match="crl_dqn_create"):
        _handle(crl, cfg, None, N3D, params).per_read()                 # a uniform crl_dqn_create_with handle is no PER handle
    h.close(); hp.close(); st.close()


def test_evaluate_on_a_new_handle_touches_nothing(crl):
    case = TB.CASE["per_n3_alpha1"]
    cfg = TB.case_cfg(case)
    h = _handle(crl, cfg, TB.case_per(case), N3D, TB.case_params(case))
    h.run(cfg.total_timesteps)
    before, tb, pb, sb, qb = h.per_read(), h.target_read(), h.per_status(), h.status(), h.read_params()
    ev = h.evaluate(8, 2, seed=3)
    assert ev["report"]["episodes"] == 16
    assert h.q_values(np.zeros(4)).shape == (2, 1)
    after, ta, pa, sa, qa = h.per_read(), h.target_read(), h.per_status(), h.status(), h.read_params()
    assert all(np.array_equal(before[f], after[f]) for f in before) and all(np.array_equal(tb[f], ta[f]) for f in tb) and pb == pa
    assert all(np.array_equal(sb[f], sa[f]) for f in sb) and np.array_equal(qb[0], qa[0]) and np.array_equal(qb[1], qa[1])
    assert tb["m"].max() > 1 and tb["td"].any(), "the run did form n-step targets"
    h.close()


def test_errors(crl):
    L = crl._lib
    cfg = O.dqn_config(seed=SEED)
    for tgt, field in ((dict(n_step=0, double_q=0), "n_step"), (dict(n_step=17, double_q=0), "n_step"), (dict(n_step=-1, double_q=1), "n_step"),
                       (dict(n_step=3, double_q=2), "double_q"), (dict(n_step=3, double_q=-1), "double_q")):
        with pytest.raises(crl.CrlError, match=field):
            _handle(crl, cfg, None, tgt)
    with pytest.raises(crl.CrlError, match="alpha"):
        _handle(crl, cfg, {**PER, "alpha": 2.0}, N3D)
    with pytest.raises(crl.CrlError, match="batch_size"):
        _handle(crl, O.dqn_config(batch_size=5000), None, N3D)
    lib, out = L.load(), C.c_void_p()
    ccfg, topt = _crl_cfg(L, cfg), L.CrlDQNTargetOptions(3, 1)
    for args in ((None, None, C.byref(topt), 0, C.byref(out)), (C.byref(ccfg), None, C.byref(topt), 0, None)):
        assert lib.crl_dqn_create_with(*args) != 0 and b"null" in lib.crl_last_error()
    assert lib.crl_dqn_create_with(C.byref(ccfg), None, None, 0, C.byref(out)) == 0, "tgt NULL = {1, 0}, per NULL = uniform"
    assert lib.crl_dqn_target_read(out, None, None, None, None, None, None) == 0, "any pointer may be NULL"
    assert lib.crl_dqn_destroy(out) == 0
    assert lib.crl_dqn_target_read(None, None, None, None, None, None, None) != 0
    h = _handle(crl, cfg, None, N3D)
    r, t = np.ones(4), np.zeros(4, np.uint8)
    idx, last, m, nret, ndisc = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2), np.zeros(2)
    dp, ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    good = [dp(r), t.ctypes.data_as(C.POINTER(C.c_uint8)), 4, 0, ip(idx), 2, 3, 0.9, ip(last), ip(m), dp(nret), dp(ndisc)]
    assert lib.crl_dqn_nstep_probe(h._h, *good) == 0
    for i in (0, 1, 4, 8, 9, 10, 11):
        args = list(good); args[i] = None
        assert lib.crl_dqn_nstep_probe(h._h, *args) != 0 and b"null" in lib.crl_last_error()
    assert lib.crl_dqn_nstep_probe(None, *good) != 0
    for reward, ptr, ix, n_step, what in ((np.ones(65537), 0, [0], 3, "cap must"), (np.ones(0), 0, [0], 3, "cap must"), (np.ones(4), 0, [], 3, "k must"),
                                          (np.ones(4), 0, [0] * 1025, 3, "k must"), (np.ones(4), 4, [0], 3, "ptr must"), (np.ones(4), -1, [0], 3, "ptr must"),
                                          (np.ones(4), 0, [0], 0, "n_step must"), (np.ones(4), 0, [0], 17, "n_step must"),
                                          (np.ones(4), 0, [0, 4], 3, "idx must"), (np.ones(4), 0, [-1], 3, "idx must")):
        with pytest.raises(crl.CrlError, match=what):
            h.nstep_probe(reward, np.zeros(reward.size, np.uint8), ptr, np.array(ix, np.int32), n_step, 0.9)
    with pytest.raises(crl.CrlError, match="parameters not set"):
        h.run(10)
    with pytest.raises(ValueError, match="n_step"):
        crl.DQNAgent(crl.DQNConfig(), target=crl.DQNTargetOptions(n_step=17))
    with pytest.raises(TypeError, match="DQNTargetOptions"):
        crl.DQNAgent(crl.DQNConfig(), target=dict(n_step=3))
    h.close()


# ---------------------------------------------------------------------------------------------------- the entry point
def _records(path):
    return [json.loads(l) for l in open(path)]


def test_entry_point_is_repeatable_and_none_is_the_uniform_loop(crl, tmp_path):
    runs = []
    for i, target in enumerate((crl.DQNTargetOptions(3, True), crl.DQNTargetOptions(3, True), None)):
        d = tmp_path / str(i); d.mkdir()
        cfg = crl.DQNConfig(run_name="t", total_timesteps=2500)
        agent = crl.dqn(cfg, target=target, seed=9, chunk=700, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(d))
        assert agent.handle.status()["global_step"] == 2500
        recs = _records(os.path.join(d, "dqn|t.json"))
        tr = [r for r in recs if r["msg"] == "Training Statistics"]
        ep = [{k: v for k, v in r.items() if k not in ("steps_per_sec", "time", "timestamp")} for r in recs if r["msg"] == "Episode Statistics"]
        runs.append((tr, ep, agent.handle.read_params(), agent.handle.target_read() if target else None))
        agent.close()
    (tr_a, ep_a, p_a, t_a), (tr_b, ep_b, p_b, t_b), (tr_u, _, p_u, _) = runs
    assert len(tr_a) == 2 and all("loss" in r and "beta" not in r for r in tr_a), "the log records are unchanged"
    assert [r["loss"] for r in tr_a] == [r["loss"] for r in tr_b] and len(ep_a) == len(ep_b) > 0, "repeatable bit for bit: the records"
    assert [r["episode_return"] for r in ep_a] == [r["episode_return"] for r in ep_b]
    assert np.array_equal(p_a[0], p_b[0]) and np.array_equal(p_a[1], p_b[1]) and all(np.array_equal(t_a[f], t_b[f]) for f in t_a)
    assert t_a["m"].max() == 3
    ref = O.DQNState(O.dqn_config(total_timesteps=2500, seed=9), crl.make_nn(0)); ref.run(2500)
    assert np.array_equal(p_u[0], ref.params()[0]) and np.array_equal(p_u[1], ref.params()[1]), "target=None is the uniform loop"
    assert len(tr_u) == 2 and not np.array_equal(p_u[0], p_a[0])
    ref.close()


LEARN_JSON = os.path.join(PB.B.ROOT, "profiles", "dqn_target_learn.json")
LEARN_SEEDS = (1, 2, 3)


def test_n3_double_agent_learns(crl):
    """After 20,000 steps at lr = 1e-3 (the step count and the rate of test_per_agent_learns, for its reasons) dqn_evaluate of the agent with
    DQNTargetOptions(3, True) returns strictly more than the same evaluation of its initial network. Measured first (scripts/dqn_target_learn.py →
    profiles/dqn_target_learn.json, eight seeds); the seeds run here are taken from those the profile shows learning."""
    prof = json.load(open(LEARN_JSON))
    rows = prof["runs"]["n3_double"]
    assert prof["steps"] == 20_000 and prof["lr"] == 1e-3 and len(rows) == 8
    learned = [s for s, r in rows.items() if r[-1] > r[0]]
    print(f"seeds that learned in the profile: {sorted(learned)} of 8")
    assert all(str(s) in learned for s in LEARN_SEEDS)
    for seed in LEARN_SEEDS:
        agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=20_000, lr=1e-3), seed=seed, init_seed=seed, target=crl.DQNTargetOptions(3, True))
        before = crl.dqn_evaluate(agent, num_envs=256)["report"]["return_mean"]
        agent.handle.run(20_000)
        after = crl.dqn_evaluate(agent, num_envs=256)["report"]["return_mean"]
        print(f"seed {seed}: held-out return_mean {before} -> {after}")
        assert agent.handle.status()["global_step"] == 20_000 and after > before
        assert before == rows[str(seed)][0], "the recorded run's initial network"
        agent.close()
