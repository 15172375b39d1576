"""Dueling heads on the GPU (crl_dqn_dueling_create; csrc/dqn_duel.hpp and the dqn_duel_*_kernel family of csrc/dqn.hip) against the numpy restatement
tests/duel_ref.py, on the case table of tests/duel_bar.py.

What is bit-equal and what is under a bar. The scalar head with uniform replay runs no transcendental (halving is exact), so those cases are bit-equal
in EVERYTHING: episodes, every loss record, last_loss, both parameter arrays and crl_dqn_target_read's arrays. pow (PER) and exp / log (the categorical
head) are the device library's, and nobody has measured how far they lie from numpy's, so in those cases everything downstream of them sits under the
bars of profiles/duel_bar.json (measured on the CPU from the restatement's own jitter floor, never from the device), while every DECISION stays
bit-equal: the episodes (hence every greedy action), idx, last, the steps summed, R, disc, a*, and under PER the Float32 leaves and the tree. The
parameters sit under ddpg_bar.PARAM_BAR; how many cases came out bit-equal in them is printed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import c51_bar as CB
import c51_ref as Z
import dqn_per_bar as PB
import dqn_per_ref as P
import dqn_target_bar as TB
import dqn_target_ref as T
import duel_bar as B
import duel_ref as D
import oraclelib as O
import value_eval_ref as V
from test_duel_cpu import plain_in_advantage_stream

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


def _per_opt(L, per):
    return None if per is None else L.CrlDQNPEROptions(per["alpha"], per["beta_start"], per["beta_end"], per["beta_duration"], per["eps"])


def _c51_opt(L, c51):
    return None if c51 is None else L.CrlDQNC51Options(int(c51["n_atoms"]), 0, float(c51["v_min"]), float(c51["v_max"]))


def _handle(crl, ocfg, per, tgt, c51, params=None, dueling=True):
    L = crl._lib
    h = L.DQNHandle(_crl_cfg(L, ocfg), 0, per=_per_opt(L, per), target=None if tgt is None else L.CrlDQNTargetOptions(int(tgt["n_step"]), int(tgt["double_q"])),
                    c51=_c51_opt(L, c51), dueling=dueling)
    if params is not None:
        h.write_params(params)
    return h


def _case_handle(crl, case):
    return _handle(crl, B.case_cfg(case), B.case_per(case), B.case_tgt(case), B.case_c51(case), B.case_params(case))


# ---------------------------------------------------------------------------------------------------- 1. the case table
def _compare(h, ref, case, losses, ref_losses, bars, label):
    Rr, exact_case = B.case_R(case), case["name"] in B.SCALAR_UNIFORM
    sg, so = h.status(), ref.status()
    for f in ("global_step", "rb_size", "n_updates"):
        assert sg[f] == so[f], (label, f, sg[f], so[f])
    assert np.array_equal(sg["state"], so["state"]), (label, "env state")
    qg, tg = h.read_params()
    if so["n_updates"] == 0:
        assert np.array_equal(qg, ref.q) and np.array_equal(tg, ref.t)
        return None
    got, want = h.target_read(), ref.target_read()
    for f in ("last", "m", "nret", "ndisc", "astar"):
        assert np.array_equal(got[f], want[f]), (label, f)
    if exact_case:
        assert losses == ref_losses and sg["last_loss"] == so["last_loss"], (label, "every loss record and last_loss, bit for bit")
        assert np.array_equal(qg, ref.q) and np.array_equal(tg, ref.t), (label, "both parameter arrays, bit for bit")
        assert np.array_equal(got["td"], want["td"]), (label, "td")
        if B.case_tgt(case)["n_step"] == 1:
            assert np.array_equal(got["last"], ref.idx), (label, "with one step the bootstrap slot is the drawn slot: idx")
        return True
    if case["per"]:
        pr = h.per_read()
        pg, po = h.per_status(), ref.per_status()
        assert np.array_equal(pr["idx"], ref.idx), (label, "idx")
        assert np.array_equal(pr["leaves"], ref.leaves.astype(np.float32)) and np.array_equal(pr["tree"], ref.tree), (label, "leaves and tree")
        assert pg["beta"] == po["beta"] and pg["max_leaf"] == po["max_leaf"] and pg["total"] == po["total"], (label, pg, po)
        assert np.abs(pr["abs_td"] - ref.abs_td).max() <= bars["loss"] * np.abs(ref.abs_td).max(), (label, "abs_td")
    elif B.case_tgt(case)["n_step"] == 1:
        assert np.array_equal(got["last"], ref.idx), (label, "with one step the bootstrap slot is the drawn slot: idx")
    proj = sl = None
    if case["c51"] is not None:
        r = h.c51_read()
        proj = r["proj"]
        sl = float(np.abs(r["sample_loss"] - ref.sample_loss).max() / np.abs(ref.sample_loss).max())
        assert np.all(r["sample_loss"] >= 0.0) and np.all(proj >= 0.0)
    dist = B.distances(losses, (qg, tg), proj, ref_losses, (ref.q, ref.t), None if proj is None else ref.proj, Rr)
    ll = abs(sg["last_loss"] - so["last_loss"]) / abs(so["last_loss"])
    td = float(np.abs(got["td"] - want["td"]).max() / max(np.abs(want["td"]).max(), 1.0))
    exact = np.array_equal(qg, ref.q) and np.array_equal(tg, ref.t)
    print(f"{case['name']} {label}: {so['n_updates']} updates; loss {dist['loss']:.3e}, last_loss {ll:.3e}, loss_j {sl if sl is None else format(sl, '.3e')}, "
          f"td {td:.3e} (bar {bars['loss']:.3e}); proj {dist['proj']:.3e} (bar {bars['proj']:.3e}); q {dist['q']:.3e}, target {dist['target']:.3e} "
          f"(bar {bars['q']:.3e}); parameters bit-equal: {exact}")
    assert dist["loss"] <= bars["loss"] and ll <= bars["loss"] and td <= bars["loss"] and (sl is None or sl <= bars["loss"])
    assert dist["proj"] <= bars["proj"]
    assert dist["q"] <= bars["q"] and dist["target"] <= bars["target"]
    return exact


@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_case_table_matches_the_restatement(crl, bars, name):
    case = B.CASE[name]
    cfg = B.case_cfg(case)
    h, ref = _case_handle(crl, case), B.make_ref(case)
    assert h.param_count() == D.param_count(B.case_R(case))
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
    assert len(ref.greedy) > 0, "the run acted greedily on the combined head"
    BIT_EQUAL[name] = bool(exact)
    if name == B.CASES[-1]["name"]:
        print(f"cases whose parameters came out bit-equal: {sum(BIT_EQUAL.values())} of {len(BIT_EQUAL)}: {sorted(n for n, e in BIT_EQUAL.items() if e)}")
    h.close()


# ---------------------------------------------------------------------------------------------------- 2. the public calls agree with each other
def _combine(s):
    """the header's expression on the host: out (R, 2, n) = V + (A − (A0 + A1)·0.5)"""
    V_, A = s["value"], s["adv"]
    return V_[:, None, :] + (A - ((A[:, 0, :] + A[:, 1, :]) * 0.5)[:, None, :])


def _snapshot(h, case):
    out = [h.target_read(), h.status(), h.read_params()]
    if case["per"]:
        out += [h.per_read(), h.per_status()]
    if case["c51"] is not None:
        out.append(h.c51_read())
    return out


def _same(a, b):
    if isinstance(a, dict):
        return all(_same(a[f], b[f]) for f in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("name", ["per_n3_double", "c51_n33_per_n3_double"])
def test_streams_q_values_and_evaluation_are_one_computation(crl, bars, name):
    case = B.CASE[name]
    cfg, c51 = B.case_cfg(case), B.case_c51(case)
    Rr = B.case_R(case)
    h, ref = _case_handle(crl, case), B.make_ref(case)
    h.run(cfg.total_timesteps)
    ref.run(cfg.total_timesteps)
    before = _snapshot(h, case)
    n_envs = 2 * crl._lib.dqn_eval_envs_per_block() + 1
    ev = h.evaluate(n_envs, 2, seed=3, trace_steps=4)
    assert ev["report"]["episodes"] == 2 * n_envs
    obs = np.stack([V.reset(3, j * n_envs + e) for j in range(2) for e in range(n_envs)], axis=1)
    X = np.concatenate([obs, np.random.default_rng(5).uniform(-2.4, 2.4, (4, 28))], axis=1)
    q, s = h.q_values(X), h.dueling_streams(X)
    assert s["value"].shape == (Rr, X.shape[1]) and s["adv"].shape == (Rr, 2, X.shape[1]) and q.shape == (2, X.shape[1])
    out = _combine(s)
    # the restatement on the DEVICE's parameters: nothing transcendental lies between them and the streams, so these are bit-equal on both heads
    ref.q = h.read_params()[0].copy()
    rs = ref.streams(X)
    assert np.array_equal(s["value"], rs["value"]) and np.array_equal(s["adv"], rs["adv"]), "the restatement's streams from the same parameters, bit for bit"
    if c51 is None:
        assert np.array_equal(out[0], q), "crl_dqn_q_values is the header's combination of crl_dqn_dueling_streams, bit for bit"
        assert np.array_equal(q, ref.q_values(X)), "and the restatement's Q from the same parameters"
    else:
        p = h.c51_probs(X)
        z = Z.atoms(c51)[0]
        for a in range(2):
            want_p = Z.softmax(out[:, a, :])[0]
            assert np.abs(p[:, a, :] - want_p).max() <= bars["proj"], "crl_dqn_c51_probs is the softmax of the combined streams"
            assert np.array_equal(q[a], Z.sum_atoms(z[:, None] * p[:, a, :])), "crl_dqn_q_values is Σ z·p of crl_dqn_c51_probs, bit for bit"
        rp, rq = ref.probs(X), ref.q_values(X)
        print(f"from the same parameters, probs against the restatement: {np.abs(p - rp).max():.3e}; q_values: {np.abs(q - rq).max() / np.abs(rq).max():.3e}")
        assert np.abs(p - rp).max() <= bars["proj"] and np.abs(q - rq).max() <= bars["loss"] * np.abs(rq).max()
    n0 = obs.shape[1]
    act = np.where(q[1, :n0] > q[0, :n0], 1, 0).reshape(2, n_envs)
    assert np.array_equal(ev["trace_action"][0], act[0]), "evaluation's first actions are the argmax of crl_dqn_q_values, bit for bit"
    assert np.array_equal(ev["q0"], q[act.reshape(-1), np.arange(n0)].reshape(2, n_envs)), "and every q0 is its value, bit for bit"
    assert _same(before, _snapshot(h, case)), "evaluation leaves every training array untouched"
    h.close()


# ---------------------------------------------------------------------------------------------------- 3. reduction to the plain net
def test_a_zero_value_head_reduces_to_the_plain_handle(crl):
    L = crl._lib
    cfg = B.case_cfg(B.CASE["k31"])
    plain = PB.case_params(PB.CASE["gamma0"])
    hp = L.DQNHandle(_crl_cfg(L, cfg), 0)
    hp.write_params(plain)
    hd = _handle(crl, cfg, None, None, None, plain_in_advantage_stream(plain))
    X = np.random.default_rng(6).uniform(-2.4, 2.4, (4, 50))
    qp, qd = hp.q_values(X), hd.q_values(X)
    assert np.array_equal(qd, qp - ((qp[0] + qp[1]) * 0.5)[None]), "Q = 0 + (A − mean A) with A the plain net's Q, bit for bit"
    s = hd.dueling_streams(X)
    assert np.all(s["value"] == 0.0) and np.array_equal(s["adv"][0], qp)
    n_envs = 2 * L.dqn_eval_envs_per_block() + 1
    ep, ed = hp.evaluate(n_envs, 2, seed=3, trace_steps=200), hd.evaluate(n_envs, 2, seed=3, trace_steps=200)
    # centring moves both Q by the same amount: the order of the two survives unless the plain net's Q tie to the last few bits, which no step here does
    assert np.array_equal(ed["trace_action"], ep["trace_action"]) and np.array_equal(ed["returns"], ep["returns"])
    assert np.array_equal(ed["lengths"], ep["lengths"]) and ep["report"]["env_steps"] > 2 * n_envs
    hp.close(); hd.close()


# ---------------------------------------------------------------------------------------------------- 4. the other handles
def test_old_handles_are_unchanged_beside_a_dueling_handle(crl):
    """in one process, interleaved with a running dueling handle: a crl_dqn_create handle is still bit-identical to oracle/dqn_oracle.c, a
    crl_dqn_per_create handle to dqn_per_ref and a crl_dqn_c51_create handle to c51_ref under their own bars, a crl_dqn_create_with handle
    bit-identical to dqn_target_ref; dueling_streams fails on all four with a message naming crl_dqn_dueling_create"""
    L = crl._lib
    hd = _case_handle(crl, B.CASE["c51_n33_per_n3_double"]) if hasattr(L.DQNHandle, "dueling_streams") else None
    case = PB.CASE["k61_cap64"]
    cfg, params = PB.case_cfg(case), PB.case_params(case)
    h = L.DQNHandle(_crl_cfg(L, cfg), 0)
    h.write_params(params)
    st = O.DQNState(cfg, params)
    pcase = PB.CASE["gamma0"]
    pcfg, pparams, pper = PB.case_cfg(pcase), PB.case_params(pcase), PB.case_per(pcase)
    hper = L.DQNHandle(_crl_cfg(L, pcfg), 0, per=_per_opt(L, pper))
    hper.write_params(pparams)
    rper = P.DQNPER(pcfg, pper, pparams)
    per_loss_bar, per_param_bar = PB.load_bars()
    tcase = TB.CASE["n3_double"]
    tcfg, tparams = TB.case_cfg(tcase), TB.case_params(tcase)
    assert TB.case_per(tcase) is None
    ht = L.DQNHandle(_crl_cfg(L, tcfg), 0, target=L.CrlDQNTargetOptions(int(tcase["tgt"]["n_step"]), int(tcase["tgt"]["double_q"])))
    ht.write_params(tparams)
    rt = T.DQNTarget(tcfg, None, tcase["tgt"], tparams)
    ccase = CB.CASE["n2"]
    ccfg, cc51 = CB.case_cfg(ccase), CB.case_c51(ccase)
    hc = L.DQNHandle(_crl_cfg(L, ccfg), 0, target=L.CrlDQNTargetOptions(1, 0), c51=_c51_opt(L, cc51))
    hc.write_params(CB.case_params(ccase))
    rc = CB.make_ref(ccase)
    cbars = CB.load_bars()
    lp, lpr, lc, lcr = [], [], [], []
    for chunk in (1, 7, max(cfg.total_timesteps, pcfg.total_timesteps, tcfg.total_timesteps, ccfg.total_timesteps)):
        if hd is not None:
            hd.run(chunk)
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
        a, b = hper.run(chunk), rper.run(chunk)
        assert a[:2] == b[:2]
        lp += a[2]; lpr += b[2]
        a, b = hc.run(chunk), rc.run(chunk)
        assert a[:2] == b[:2]
        lc += a[2]; lcr += b[2]
    dist = PB.distances(lp, hper.read_params(), lpr, (rper.q, rper.t))
    assert dist["loss"] <= per_loss_bar and dist["q"] <= per_param_bar and dist["target"] <= per_param_bar
    pr = hper.per_read()
    assert np.array_equal(pr["idx"], rper.idx) and np.array_equal(pr["leaves"], rper.leaves.astype(np.float32)) and np.array_equal(pr["tree"], rper.tree)
    dist = CB.distances(lc, hc.read_params(), hc.c51_read()["proj"], lcr, (rc.q, rc.t), rc.proj, cc51["n_atoms"])
    assert all(dist[o] <= cbars[o] for o in CB.OBSERVABLES), dist
    assert all(x.status()["n_updates"] >= 3 for x in (h, hper, ht, hc))
    assert h.param_count() == ht.param_count() == hper.param_count() == L.DQN_PARAM_COUNT and hc.param_count() == Z.param_count(2)
    if hd is not None:
        assert hd.status()["n_updates"] >= 3
        for old in (h, hper, ht, hc):
            with pytest.raises(crl.CrlError, match="crl_dqn_dueling_create"):
                old.dueling_streams(np.zeros(4))
        hd.close()
    for x in (h, hper, ht, hc, st):
        x.close()


# ---------------------------------------------------------------------------------------------------- 5. side by side
def test_dueling_handles_of_different_heads_live_side_by_side(crl):
    """the dynamic LDS size is a property of the kernel, not of the handle: handles with N = 64, N = 2 and the scalar head, made in that order and run
    interleaved, each reproduce the bits of a run on their own, an evaluation included"""
    names = ("c51_n64", "c51_n2", "k31")
    want = {}
    for n in names:
        alone = _case_handle(crl, B.CASE[n])
        alone.run(B.case_cfg(B.CASE[n]).total_timesteps)
        want[n] = (alone.read_params(), alone.evaluate(5, 1, seed=3))
        alone.close()
    hs = {n: _case_handle(crl, B.CASE[n]) for n in names}
    for chunk in (150, 150):
        for n in reversed(names):
            hs[n].run(chunk)
    for n in names:
        got, got_ev = hs[n].read_params(), hs[n].evaluate(5, 1, seed=3)
        assert hs[n].status()["n_updates"] == 20
        assert np.array_equal(got[0], want[n][0][0]) and np.array_equal(got[1], want[n][0][1]), n
        assert all(np.array_equal(got_ev[f], want[n][1][f]) for f in ("q0", "returns", "lengths", "disc_returns")), n
        hs[n].close()


# ---------------------------------------------------------------------------------------------------- 6. errors
def test_errors(crl):
    L = crl._lib
    cfg = O.dqn_config(seed=21)
    good = dict(n_atoms=51, v_min=0.0, v_max=100.0)
    for bad, field in ((dict(n_atoms=1), "n_atoms"), (dict(n_atoms=65), "n_atoms"), (dict(v_min=100.0), "v_min"), (dict(v_max=float("inf")), "v_max")):
        with pytest.raises(crl.CrlError, match=field):
            _handle(crl, cfg, None, None, {**good, **bad})
    for c51 in (None, good):
        with pytest.raises(crl.CrlError, match="n_step"):
            _handle(crl, cfg, None, dict(n_step=17, double_q=0), c51)
        with pytest.raises(crl.CrlError, match="double_q"):
            _handle(crl, cfg, None, dict(n_step=1, double_q=2), c51)
        with pytest.raises(crl.CrlError, match="alpha"):
            _handle(crl, cfg, dict(alpha=2.0, beta_start=0.4, beta_end=1.0, beta_duration=10.0, eps=1e-6), None, c51)
    lib, out = L.load(), C.c_void_p()
    ccfg, copt = _crl_cfg(L, cfg), L.CrlDQNC51Options(51, 0, 0.0, 100.0)
    for args in ((None, C.byref(copt), None, None, 0, C.byref(out)), (C.byref(ccfg), C.byref(copt), None, None, 0, None), (None, None, None, None, 0, None)):
        assert lib.crl_dqn_dueling_create(*args) != 0 and b"null" in lib.crl_last_error()
    n = C.c_size_t()
    assert lib.crl_dqn_dueling_create(C.byref(ccfg), C.byref(copt), None, None, 0, C.byref(out)) == 0, "per NULL = uniform, tgt NULL = {1, 0}"
    assert lib.crl_dqn_param_count(out, C.byref(n)) == 0 and n.value == 33933
    assert lib.crl_dqn_destroy(out) == 0
    assert lib.crl_dqn_dueling_create(C.byref(ccfg), None, None, None, 0, C.byref(out)) == 0, "c51 NULL = the scalar head"
    assert lib.crl_dqn_param_count(out, C.byref(n)) == 0 and n.value == 21183
    assert lib.crl_dqn_dueling_streams(out, None, 1, None, None) != 0
    assert lib.crl_dqn_dueling_streams(None, None, 0, None, None) != 0 and b"null" in lib.crl_last_error()
    assert lib.crl_dqn_destroy(out) == 0
    h = _handle(crl, cfg, None, None, None)
    for call in (lambda: h.run(10), lambda: h.q_values(np.zeros(4)), lambda: h.dueling_streams(np.zeros(4)), lambda: h.evaluate(4)):
        with pytest.raises(crl.CrlError, match="parameters not set"):
            call()
    for size in (21182, 21184, 10934):
        with pytest.raises(crl.CrlError, match="expected 21183 floats"):
            h.write_params(np.zeros(size, np.float32))
    assert h.target_read()["last"].shape == (cfg.batch_size,), "a dueling handle always carries target options"
    for call in (h.per_status, h.c51_read):
        with pytest.raises(crl.CrlError):
            call()
    h.init_params(3)
    q, t = h.read_params()
    assert q.size == 21183 and np.array_equal(q, t) and np.array_equal(q, L.dqn_dueling_make_nn_host(3))
    assert np.array_equal(q[:480], L.dqn_make_nn_host(3)[:480]), "crl_dqn_make_nn's W1 draws for the same seed"
    assert np.array_equal(h.dueling_streams(np.zeros(4))["adv"].shape, (1, 2, 1))
    hc = _handle(crl, cfg, None, None, good)
    hc.init_params(3)
    q, t = hc.read_params()
    assert q.size == 33933 and np.array_equal(q, t) and np.array_equal(q, L.dqn_dueling_make_nn_host(3, 51))
    with pytest.raises(crl.CrlError, match="expected 33933 floats"):
        hc.write_params(np.zeros(19434, np.float32))
    with pytest.raises(crl.CrlError, match="n_atoms"):
        L.dqn_dueling_make_nn_host(0, 65)
    with pytest.raises(crl.CrlError, match="n_atoms"):
        L.dqn_dueling_make_nn_host(0, 1)
    plain = L.DQNHandle(_crl_cfg(L, cfg), 0)
    with pytest.raises(crl.CrlError, match="expected 10934 floats"):
        plain.write_params(np.zeros(21183, np.float32))
    plain.close(); h.close(); hc.close()


# ---------------------------------------------------------------------------------------------------- 7. the entry point
def _records(path):
    return [json.loads(l) for l in open(path)]


@pytest.mark.parametrize("head", ["scalar", "c51"])
def test_entry_point_logs_and_is_repeatable(crl, tmp_path, head):
    runs = []
    for i in range(2):
        d = tmp_path / str(i); d.mkdir()
        cfg = crl.DQNConfig(run_name="t", total_timesteps=2500)
        agent = crl.dqn(cfg, dist=crl.C51Options() if head == "c51" else None, dueling=True, seed=9, chunk=700, eval_every=1250, eval_envs=16,
                        to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(d))
        assert agent.handle.status()["global_step"] == 2500 and agent.handle.param_count() == (33933 if head == "c51" else 21183)
        recs = _records(os.path.join(d, "dqn|t.json"))
        tr = [r for r in recs if r["msg"] == "Training Statistics"]
        ev = [{k: v for k, v in r.items() if k not in ("time", "timestamp")} for r in recs if r["msg"] == "Evaluation Statistics"]
        ep = [{k: v for k, v in r.items() if k not in ("steps_per_sec", "time", "timestamp")} for r in recs if r["msg"] == "Episode Statistics"]
        runs.append((tr, ep, ev, agent.handle.read_params(), agent.handle.target_read()))
        agent.close()
    (tr_a, ep_a, ev_a, p_a, t_a), (tr_b, ep_b, ev_b, p_b, t_b) = runs
    assert len(tr_a) == 2 and all(r["loss"] > 0.0 and "beta" not in r for r in tr_a)
    assert [r["loss"] for r in tr_a] == [r["loss"] for r in tr_b] and len(ep_a) == len(ep_b) > 0
    assert [r["episode_return"] for r in ep_a] == [r["episode_return"] for r in ep_b]
    assert len(ev_a) == 2 and [r["eval_return_mean"] for r in ev_a] == [r["eval_return_mean"] for r in ev_b]
    assert [r["eval_q_bias"] for r in ev_a] == [r["eval_q_bias"] for r in ev_b]
    assert np.array_equal(p_a[0], p_b[0]) and np.array_equal(p_a[1], p_b[1]) and all(np.array_equal(t_a[f], t_b[f]) for f in t_a)
    assert not np.array_equal(p_a[0], crl.make_nn_dueling(0, 51 if head == "c51" else None))


# ---------------------------------------------------------------------------------------------------- 8. learns
LEARN_JSON = os.path.join(B.B.ROOT, "profiles", "duel_learn.json")
LEARN_SEEDS = (1, 2, 3)


@pytest.mark.parametrize("arm", ["duel", "duel_c51_per_n3_double"])
def test_duel_agent_learns(crl, arm):
    """After 20,000 steps at lr = 1e-3 (the step count and the rate of test_per_agent_learns, for its reasons) dqn_evaluate of the dueling agent returns
    strictly more than the same evaluation of its initial network: the scalar dueling head, and dueling + C51 + PER + 3-step + double. Measured first
    (scripts/duel_learn.py → profiles/duel_learn.json, eight seeds); the seeds run here are taken from those the profile shows learning."""
    prof = json.load(open(LEARN_JSON))
    rows = prof["runs"][arm]
    assert prof["steps"] == 20_000 and prof["lr"] == 1e-3 and len(rows) == 8
    learned = [s for s, r in rows.items() if r[-1] > r[0]]
    print(f"seeds that learned in the profile: {sorted(learned)} of 8")
    assert all(str(s) in learned for s in LEARN_SEEDS)
    kw = {} if arm == "duel" else dict(per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True), dist=crl.C51Options())
    for seed in LEARN_SEEDS:
        agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=20_000, lr=1e-3), seed=seed, init_seed=seed, dueling=True, **kw)
        before = crl.dqn_evaluate(agent, num_envs=256)["report"]["return_mean"]
        agent.handle.run(20_000)
        after = crl.dqn_evaluate(agent, num_envs=256)["report"]["return_mean"]
        print(f"seed {seed}: held-out return_mean {before} -> {after}")
        assert agent.handle.status()["global_step"] == 20_000 and after > before
        assert before == rows[str(seed)][0], "the recorded run's initial network"
        agent.close()
