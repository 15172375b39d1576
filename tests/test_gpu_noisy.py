"""Noisy linear layers on the GPU (crl_dqn_noisy_create; csrc/dqn_noisy.hpp, dqn_noisy_adam_step of csrc/dqn_loops.hpp, dqn_noisy_*_kernel of
csrc/dqn.hip) against the numpy restatement tests/noisy_ref.py, on the case table of tests/noisy_bar.py.

What is bit-equal and what is under a bar. The noise itself is compared apart from learning: xi runs log, cos and sqrt of the device library, which may
differ from numpy's by a few Float64 ulp, and that flips the Float32 rounding of a value with probability about 1e-15 / 6e-8 ≈ 2e-8; so every probed
value lies within one Float32 ulp and at most 2 of the ≈ 2·10⁴ probed values are not bit-equal. Everything after that runs on the DEVICE's xi tape,
fetched per generation through the stateless probe, so noise jitter cannot enter: the uniform scalar cases (plain and dueling, any target option) have
no transcendental left and are bit-equal in everything; the PER and C51 cases sit under the bars of profiles/noisy_bar.json (measured on the CPU from
the restatement's own ±2 ulp jitter floor), with every decision — the episodes, idx, a*, the walk, the Float32 PER leaves — bit-equal."""
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
import duel_bar as DB
import noisy_bar as B
import noisy_ref as N
import oraclelib as O
import value_eval_ref as V

pytestmark = pytest.mark.gpu

BIT_EQUAL = {}
PROBE_GENS = (0, 1, 2 ** 32 + 1, 2 ** 40 + 1)
PROBE_TABLES = (("k65_eps0", 414), ("k120_duel", 703), ("rainbow_n64", 892))


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


@pytest.fixture(scope="module")
def bars():
    return B.load_bars()


def _crl_cfg(L, ocfg):
    return L.CrlDQNConfig(*[getattr(ocfg, f) for f, _ in O.DQNConfigC._fields_])


def _opts(L, per, tgt, c51):
    return dict(per=None if per is None else L.CrlDQNPEROptions(per["alpha"], per["beta_start"], per["beta_end"], per["beta_duration"], per["eps"]),
                target=None if tgt is None else L.CrlDQNTargetOptions(int(tgt["n_step"]), int(tgt["double_q"])),
                c51=None if c51 is None else L.CrlDQNC51Options(int(c51["n_atoms"]), 0, float(c51["v_min"]), float(c51["v_max"])))


def _handle(crl, ocfg, per=None, tgt=None, c51=None, dueling=False, params=None, sigma0=B.SIGMA0, noisy=True):
    L = crl._lib
    h = L.DQNHandle(_crl_cfg(L, ocfg), 0, dueling=dueling, noisy=L.CrlDQNNoisyOptions(sigma0) if noisy else None, **_opts(L, per, tgt, c51))
    if params is not None:
        h.write_params(params)
    return h


def _case_handle(crl, case, **kw):
    return _handle(crl, B.case_cfg(case), B.case_per(case), B.case_tgt(case), B.case_c51(case), case["dueling"], B.case_params(case), **kw)


def _tape(h, n_gens):
    return {(g, net): h.noisy_noise(g, net) for g in range(n_gens) for net in (0, 1)}


def _images_are_mu_plus_sigma_eps(h, lay, label):
    """crl_dqn_noisy_weights = mu + sigma·eps formed in numpy Float32 from the device's own xi and read_params, bit for bit, at the current generation"""
    gen = h.status()["n_updates"]
    q, t = h.read_params()
    P_ = q.size // 2
    for net, p in ((0, q), (1, t)):
        want = N.image(p[:P_], p[P_:], N.eps_of(lay, h.noisy_noise(gen, net)))
        assert np.array_equal(h.noisy_weights(net), want), (label, "image of net", net, "generation", gen)


# ---------------------------------------------------------------------------------------------------- 1. the noise apart from learning
def test_noise_matches_the_restatement_within_a_float32_ulp(crl):
    total = off = 0
    for name, n_xi in PROBE_TABLES:
        case = B.CASE[name]
        lay, seed = B.case_layers(case), B.case_cfg(case).seed
        h = _case_handle(crl, case)
        assert N.n_xi(lay) == n_xi
        for gen in PROBE_GENS:
            tabs = [h.noisy_noise(gen, net) for net in (0, 1)]
            assert not np.array_equal(tabs[0], tabs[1]), "each net on its own stream word"
            for net in (0, 1):
                want = N.xi_table(seed, lay, gen, net)
                got = tabs[net]
                assert got.shape == want.shape == (n_xi,)
                assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))), (name, gen, net, "within one Float32 ulp")
                total += n_xi; off += int((got != want).sum())
        h.close()
    print(f"xi probe: {off} of {total} values not bit-equal to the restatement")
    assert total == 8 * (414 + 703 + 892) and off <= 2


def test_images_are_mu_plus_sigma_eps_at_create_after_write_and_after_updates(crl):
    case = B.CASE["wrap_cap31_duel"]                      # target_net_freq 50, train_freq 3: updates with and without a copy
    cfg, lay = B.case_cfg(case), B.case_layers(case)
    h = _handle(crl, cfg, None, B.case_tgt(case), None, True)
    q, t = h.read_params()
    assert np.all(q == 0.0) and np.all(h.noisy_weights(0) == 0.0), "a fresh handle holds zeros"
    h.write_params(B.case_params(case))
    _images_are_mu_plus_sigma_eps(h, lay, "after write_params")
    assert not np.array_equal(h.noisy_weights(0), h.noisy_weights(1)) and np.array_equal(*h.read_params())
    copies = 0
    for stop in (42, 45, 48, 51, 54, 150):               # updates at 42, 45, 48, 51, ...; copies at 150 only
        h.run(stop - h.status()["global_step"])
        _images_are_mu_plus_sigma_eps(h, lay, f"after step {stop}")
        q, t = h.read_params()
        copies += int(np.array_equal(q, t))
    assert copies == 1 and h.status()["n_updates"] == 37
    h.write_params(B.case_params(case))
    _images_are_mu_plus_sigma_eps(h, lay, "after write_params at generation 37")
    h.close()


# ---------------------------------------------------------------------------------------------------- 2. the case table on the device's tape
def _compare(h, ref, case, losses, ref_losses, bars, label):
    exact_case = case["name"] in B.EXACT
    sg, so = h.status(), ref.status()
    for f in ("global_step", "rb_size", "n_updates"):
        assert sg[f] == so[f], (label, f, sg[f], so[f])
    assert np.array_equal(sg["state"], so["state"]), (label, "env state")
    pg, imgs = h.read_params(), (h.noisy_weights(0), h.noisy_weights(1))
    if so["n_updates"] == 0 or exact_case:
        assert np.array_equal(pg[0], ref.pq) and np.array_equal(pg[1], ref.pt), (label, "mu and sigma of both nets, bit for bit")
        assert np.array_equal(imgs[0], ref.q) and np.array_equal(imgs[1], ref.t), (label, "both effective images, bit for bit")
        assert losses == ref_losses and sg["last_loss"] == so["last_loss"], (label, "every loss record and last_loss, bit for bit")
        return True
    if case["tgt"] is not None or case["c51"] is not None or case["dueling"]:
        got, want = h.target_read(), ref.target_read()
        for f in ("last", "m", "nret", "ndisc", "astar"):
            assert np.array_equal(got[f], want[f]), (label, f)
    if case["per"]:
        pr = h.per_read()
        assert np.array_equal(pr["idx"], ref.idx), (label, "idx")
        assert np.array_equal(pr["leaves"], ref.leaves.astype(np.float32)) and np.array_equal(pr["tree"], ref.tree), (label, "leaves and tree")
    proj = None
    if case["c51"] is not None:
        proj = h.c51_read()["proj"]
    dist = B.distances(losses, pg, imgs, proj, ref_losses, (ref.pq, ref.pt), (ref.q, ref.t), None if proj is None else ref.proj, B.case_layers(case))
    exact = all(np.array_equal(a, b) for a, b in zip(pg + imgs, (ref.pq, ref.pt, ref.q, ref.t)))
    print(f"{case['name']} {label}: {so['n_updates']} updates; " + ", ".join(f"{o} {dist[o]:.3e}" for o in B.OBSERVABLES) +
          f" (bars: loss {bars['loss']:.3e}, proj {bars['proj']:.3e}, parameters {bars['q']:.3e}); parameters bit-equal: {exact}")
    assert all(dist[o] <= bars[o] for o in B.OBSERVABLES), dist
    return exact


@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_case_table_matches_the_restatement_on_the_device_tape(crl, bars, name):
    case = B.CASE[name]
    cfg = B.case_cfg(case)
    h = _case_handle(crl, case)
    steps = PB.update_steps(cfg)
    ref = B.make_ref(case, _tape(h, len(steps) + 1))
    assert h.param_count() == 2 * N.param_count(B.case_layers(case)) == ref.pq.size
    losses, ref_losses, total, exact = [], [], 0, None
    for chunk in PB.CHUNKS + (cfg.total_timesteps,):
        tg, eps_g, ls_g = h.run(chunk)
        to, eps_o, ls_o = ref.run(chunk)
        total += tg
        assert tg == to and eps_g == eps_o, "same trajectories, same episode records: every action taken on the noisy image agreed"
        losses += ls_g; ref_losses += ls_o
        if ref_losses or ref.n_updates == 0:
            exact = _compare(h, ref, case, losses, ref_losses, bars, f"after {total} steps")
    assert total == cfg.total_timesteps and h.status()["n_updates"] == len(steps) >= 3
    assert len(losses) == len([g for g in steps if g % cfg.log_frequency == 0]) > 0
    assert ref.gens[-1] == (len(steps), len(steps), len(steps)), "generation = completed updates, for both nets"
    P_ = ref.P
    assert not np.array_equal(ref.pq[:P_], B.case_params(case)[:P_]) and not np.array_equal(ref.pq[P_:], B.case_params(case)[P_:]), "mu and sigma both moved"
    BIT_EQUAL[name] = bool(exact)
    if name == B.CASES[-1]["name"]:
        print(f"cases whose parameters came out bit-equal: {sum(BIT_EQUAL.values())} of {len(BIT_EQUAL)}: {sorted(n for n, e in BIT_EQUAL.items() if e)}")
    h.close()


# ---------------------------------------------------------------------------------------------------- 3. mutants
MUTANT_CASE = {"M1": "wrap_cap31_duel", "M4": "wrap_cap31_duel", "M5": "tf_equal_n3_double", "M6": "tf_equal_n3_double", "M7": "wrap_cap31_duel"}


def test_every_mutant_is_far_from_the_device(crl, bars):
    """each one-line mutant of the restatement against the device on the case that sees it: the run mutants on a bit-equal case (the bar is zero there:
    one bit suffices, the distance is printed), the noise mutants on the probe, the evaluation mutant on crl_dqn_q_values"""
    runs = {}
    for m, name in MUTANT_CASE.items():
        case = B.CASE[name]
        assert name in B.EXACT
        if name not in runs:
            cfg = B.case_cfg(case)
            h = _case_handle(crl, case)
            tape = _tape(h, len(PB.update_steps(cfg)) + 1)
            ls = h.run(cfg.total_timesteps)[2]
            runs[name] = (ls, h.read_params(), (h.noisy_weights(0), h.noisy_weights(1)), tape)
            base = B.run_ref(case, None, tape)
            assert base[0] == ls and all(np.array_equal(a, b) for a, b in zip(base[1] + base[2], runs[name][1] + runs[name][2])), "the unmutated restatement"
            h.close()
        ls, params, imgs, tape = runs[name]
        got = B.run_ref(case, B.mutant(m), tape)
        same_steps = [l[0] for l in got[0]] == [l[0] for l in ls]
        dist = B.distances(got[0], got[1], got[2], None, ls, params, imgs, None, B.case_layers(case)) if same_steps else {"steps": float("inf")}
        print(f"{m} ({B.MUTANTS[m][0]}) on {name}: " + ", ".join(f"{o} {v:.3e}" for o, v in dist.items()))
        assert max(dist.values()) > 0.0, m
    case = B.CASE["k65_eps0"]
    h = _case_handle(crl, case)
    lay, seed = B.case_layers(case), B.case_cfg(case).seed
    for m in ("M2", "M3"):
        with B.mutant(m):
            want = np.concatenate([N.xi_table(seed, lay, 1, net) for net in (0, 1)])
        got = np.concatenate([h.noisy_noise(1, net) for net in (0, 1)])
        d = float(np.abs(got - want).max())
        print(f"{m} ({B.MUTANTS[m][0]}) on the xi probe: max |xi - xi_mutant| = {d:.3e} ({d / np.spacing(np.float32(1)):.3e} Float32 ulp of 1)")
        assert d >= 1e3 * np.spacing(np.float32(1))
    h.run(150)
    ref = B.make_ref(case, _tape(h, 10))
    ref.run(150)
    X = np.random.default_rng(5).uniform(-2.4, 2.4, (4, 16))
    q = h.q_values(X)
    assert np.array_equal(q, np.stack([ref.greedy_q_values(X[:, j]) for j in range(16)], axis=1)), "crl_dqn_q_values is the restatement's Q on the mu half"
    with B.mutant("M8"):
        qm = np.stack([ref.greedy_q_values(X[:, j]) for j in range(16)], axis=1)
    print(f"M8 ({B.MUTANTS['M8'][0]}) on crl_dqn_q_values: max |Q - Q_mutant| = {np.abs(q - qm).max():.3e}")
    assert np.abs(q - qm).max() > 0.0
    h.close()


# ---------------------------------------------------------------------------------------------------- 4. the noise-free calls are the twin's
def _snapshot(h):
    return [h.status(), h.read_params(), h.noisy_weights(0), h.noisy_weights(1), h.target_read(), h.per_read(), h.per_status(), h.c51_read()]


def _same(a, b):
    if isinstance(a, dict):
        return all(_same(a[f], b[f]) for f in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


def test_noise_free_calls_equal_a_twin_handle_on_the_mu_half(crl):
    case = B.CASE["rainbow_n64"]
    cfg = B.case_cfg(case)
    h = _case_handle(crl, case)
    h.run(cfg.total_timesteps)
    assert h.status()["n_updates"] == 20
    before = _snapshot(h)
    mu = h.read_params()[0][:h.param_count() // 2]
    twin = _handle(crl, cfg, B.case_per(case), B.case_tgt(case), B.case_c51(case), True, mu, noisy=False)
    X = np.random.default_rng(5).uniform(-2.4, 2.4, (4, 37))
    assert np.array_equal(h.q_values(X), twin.q_values(X)) and np.array_equal(h.c51_probs(X), twin.c51_probs(X))
    assert _same(h.dueling_streams(X), twin.dueling_streams(X))
    assert not np.array_equal(h.noisy_weights(0), mu), "the image collect acts on is not the mu half"
    per_block = crl._lib.dqn_eval_envs_per_block()
    for n_envs in (1, per_block, per_block + 1, 2 * per_block + 1):
        a, b = h.evaluate(n_envs, 2, seed=3, trace_steps=6), twin.evaluate(n_envs, 2, seed=3, trace_steps=6)
        assert _same(a, b), n_envs
        obs = np.stack([V.reset(3, j * n_envs + e) for j in range(2) for e in range(n_envs)], axis=1)
        q = h.q_values(obs)
        act = np.where(q[1] > q[0], 1, 0).reshape(2, n_envs)
        assert np.array_equal(a["trace_action"][0], act[0]), "every evaluated action is the argmax of crl_dqn_q_values on that observation, bit for bit"
    assert _same(before, _snapshot(h)), "evaluation leaves mu, sigma, both images, the PER tree and the generation untouched"
    g0 = h.status()["global_step"]
    # Adam's m, v and β powers have no read call: a second handle is evaluated and queried MID-RUN, after 5 of the 20 updates, and must end where the
    # uninterrupted run ended — the 15 updates behind the evaluation would carry any change to the optimiser state into mu and sigma
    h2 = _case_handle(crl, case)
    h2.run(150)
    assert h2.status()["n_updates"] == 5
    h2.evaluate(2 * per_block + 1, 2, seed=3, trace_steps=6); h2.q_values(X); h2.c51_probs(X); h2.dueling_streams(X)
    h2.run(cfg.total_timesteps - 150)
    assert _same(before, _snapshot(h2)), "evaluation in the middle of a run leaves the Adam state untouched as well: the run ends on the same bits"
    h.close(); h2.close(); twin.close()
    assert g0 == cfg.total_timesteps


# ---------------------------------------------------------------------------------------------------- 5. sigma0 = 0: the first update is the twin's
@pytest.mark.parametrize("name", ["k65_eps0", "rainbow_n64"])
def test_with_sigma_zero_the_first_update_is_the_twins(crl, name):
    case = B.CASE[name]
    cfg, lay = B.case_cfg(case), B.case_layers(case)
    P_ = N.param_count(lay)
    mu = B.case_params(case)[:P_]
    kw = dict(per=B.case_per(case), tgt=B.case_tgt(case), c51=B.case_c51(case), dueling=case["dueling"])
    twin = _handle(crl, cfg, params=mu, noisy=False, **kw)
    h = _handle(crl, cfg, params=np.concatenate([mu, np.zeros(P_, np.float32)]), sigma0=0.0, **kw)
    assert np.array_equal(h.noisy_weights(0), mu) and np.array_equal(h.noisy_weights(1), mu)
    first = PB.update_steps(cfg)[0]
    a, b = h.run(first), twin.run(first)
    assert a == b and h.status()["n_updates"] == 1 and a[2], "episodes up to the first update and its loss, bit for bit"
    q, t = h.read_params()
    assert np.array_equal(q[:P_], twin.read_params()[0]), "mu after the first update is the twin's q_net"
    # sigma took one Adam step from zero on gs = g·eps of generation 0: m̂ = gs, v̂ = gs², so sigma_1 = −lr·gs/(|gs| + 1e-8): its sign is −sign(g)·sign(eps)
    # and its size at most lr; sign(g) is read off mu's own first step, mu_1 − mu_0 = −lr·g/(|g| + 1e-8)
    sigma = q[P_:].astype(np.float64)
    eps = N.eps_of(lay, h.noisy_noise(0, 0)).astype(np.float64)
    sign_g = np.sign(mu.astype(np.float64) - q[:P_].astype(np.float64))
    moved = sign_g != 0.0                                  # a parameter behind dead units has g = 0 and moves in neither half
    assert np.all(eps != 0.0) and moved.sum() > 0 and np.all(sigma[moved] != 0.0), "sigma is no longer zero wherever a gradient arrived"
    assert np.array_equal(np.sign(sigma[moved]), (-sign_g * np.sign(eps))[moved]), "sigma moved against g·eps"
    assert np.abs(sigma).max() <= cfg.lr * (1.0 + 2.0 ** -20), "one Adam step is at most lr long"
    if name in B.EXACT:
        # and the value itself: the restatement from the same start on the device's tape, whose sigma gradient is (float)g * eps, bit for bit
        ref = N.make(cfg, kw["per"], kw["tgt"], kw["c51"], kw["dueling"], np.concatenate([mu, np.zeros(P_, np.float32)]), _tape(h, 2))
        ref.run(first)
        assert np.array_equal(ref.pq, q) and np.array_equal(ref.pt, t) and np.array_equal(ref.q, h.noisy_weights(0)), "sigma_1 is Adam's step on g·eps"
    h.close(); twin.close()


# ---------------------------------------------------------------------------------------------------- 6. the older handles
def test_old_handles_are_unchanged_beside_a_noisy_handle(crl):
    """in one process, interleaved with a running noisy handle: a crl_dqn_create handle is still bit-identical to oracle/dqn_oracle.c, a
    crl_dqn_create_with handle to dqn_target_ref and a scalar crl_dqn_dueling_create handle to duel_ref, a crl_dqn_per_create handle to dqn_per_ref and
    a crl_dqn_c51_create handle to c51_ref under their own bars; the noisy calls fail on all five with a message naming crl_dqn_noisy_create"""
    L = crl._lib
    hn = _case_handle(crl, B.CASE["rainbow_n64"])
    case = PB.CASE["k61_cap64"]
    cfg, params = PB.case_cfg(case), PB.case_params(case)
    h = L.DQNHandle(_crl_cfg(L, cfg), 0)
    h.write_params(params)
    st = O.DQNState(cfg, params)
    pcase = PB.CASE["gamma0"]
    pcfg, pparams, pper = PB.case_cfg(pcase), PB.case_params(pcase), PB.case_per(pcase)
    hper = L.DQNHandle(_crl_cfg(L, pcfg), 0, **{**_opts(L, pper, None, None)})
    hper.write_params(pparams)
    rper = P.DQNPER(pcfg, pper, pparams)
    per_loss_bar, per_param_bar = PB.load_bars()
    tcase = TB.CASE["n3_double"]
    tcfg, tparams = TB.case_cfg(tcase), TB.case_params(tcase)
    ht = L.DQNHandle(_crl_cfg(L, tcfg), 0, **_opts(L, None, tcase["tgt"], None))
    ht.write_params(tparams)
    rt = T.DQNTarget(tcfg, None, tcase["tgt"], tparams)
    ccase = CB.CASE["n2"]
    ccfg, cc51 = CB.case_cfg(ccase), CB.case_c51(ccase)
    hc = L.DQNHandle(_crl_cfg(L, ccfg), 0, **_opts(L, None, dict(n_step=1, double_q=0), cc51))
    hc.write_params(CB.case_params(ccase))
    rc = CB.make_ref(ccase)
    cbars = CB.load_bars()
    dcase = DB.CASE["n3_double"]
    dcfg = DB.case_cfg(dcase)
    hd = L.DQNHandle(_crl_cfg(L, dcfg), 0, dueling=True, **_opts(L, None, DB.case_tgt(dcase), None))
    hd.write_params(DB.case_params(dcase))
    rd = DB.make_ref(dcase)
    lp, lpr, lc, lcr = [], [], [], []
    for chunk in (1, 7, max(x.total_timesteps for x in (cfg, pcfg, tcfg, ccfg, dcfg))):
        hn.run(chunk)
        assert h.run(chunk) == st.run(chunk)
        qg, tg = h.read_params(); qo, to = st.params()
        assert np.array_equal(qg, qo) and np.array_equal(tg, to)
        hn.run(3)
        assert ht.run(chunk) == rt.run(chunk)
        qg, tg = ht.read_params()
        assert np.array_equal(qg, rt.q) and np.array_equal(tg, rt.t) and ht.status()["last_loss"] == rt.status()["last_loss"]
        assert hd.run(chunk) == rd.run(chunk)
        qg, tg = hd.read_params()
        assert np.array_equal(qg, rd.q) and np.array_equal(tg, rd.t)
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
    assert all(x.status()["n_updates"] >= 3 for x in (h, hper, ht, hc, hd, hn))
    assert h.param_count() == L.DQN_PARAM_COUNT and hd.param_count() == 21183
    for old in (h, hper, ht, hc, hd):
        for call in (lambda: old.noisy_weights(0), lambda: old.noisy_noise(0, 0)):
            with pytest.raises(crl.CrlError, match="crl_dqn_noisy_create"):
                call()
    for x in (h, hper, ht, hc, hd, hn, st):
        x.close()


def test_noisy_handles_of_different_heads_live_side_by_side(crl):
    names = ("rainbow_n64", "c51_n2", "k65_eps0")
    want = {}
    for n in names:
        alone = _case_handle(crl, B.CASE[n])
        alone.run(300)
        want[n] = (alone.read_params(), alone.noisy_weights(0), alone.evaluate(5, 1, seed=3))
        alone.close()
    hs = {n: _case_handle(crl, B.CASE[n]) for n in names}
    for chunk in (150, 150):
        for n in reversed(names):
            hs[n].run(chunk)
    for n in names:
        assert hs[n].status()["n_updates"] == 20
        assert _same((hs[n].read_params(), hs[n].noisy_weights(0), hs[n].evaluate(5, 1, seed=3)), want[n]), n
        hs[n].close()


def test_graph_replay_gives_the_same_bits(crl, monkeypatch):
    """CRL_DQN_GRAPH=1 (read when the handle is made) replays the cycle as a captured graph; on a noisy handle the slot list is the only thing that
    differs, and the run is the plain launches' run, bit for bit"""
    case = B.CASE["tf_equal_n3_double"]
    cfg = B.case_cfg(case)
    plain = _case_handle(crl, case)
    want = (plain.run(cfg.total_timesteps), plain.read_params(), plain.noisy_weights(0), plain.noisy_weights(1))
    plain.close()
    monkeypatch.setenv("CRL_DQN_GRAPH", "1")
    h = _case_handle(crl, case)
    monkeypatch.delenv("CRL_DQN_GRAPH")
    got = (h.run(cfg.total_timesteps), h.read_params(), h.noisy_weights(0), h.noisy_weights(1))
    assert _same(got, want) and h.status()["n_updates"] == 20
    h.close()


# ---------------------------------------------------------------------------------------------------- 7. errors
def test_errors(crl):
    L = crl._lib
    lib, out = L.load(), C.c_void_p()
    cfg = O.dqn_config(seed=21)
    ccfg, nopt = _crl_cfg(L, cfg), L.CrlDQNNoisyOptions(0.5)
    for args in ((None, C.byref(nopt), 0, None, None, None, 0, C.byref(out)), (C.byref(ccfg), None, 0, None, None, None, 0, C.byref(out)),
                 (C.byref(ccfg), C.byref(nopt), 0, None, None, None, 0, None)):
        assert lib.crl_dqn_noisy_create(*args) != 0 and b"null" in lib.crl_last_error()
    for bad in (-0.1, 10.5, float("nan"), float("inf")):
        with pytest.raises(crl.CrlError, match="sigma0"):
            _handle(crl, cfg, sigma0=bad)
        with pytest.raises(crl.CrlError, match="sigma0"):
            L.dqn_noisy_make_nn_host(0, bad)
    assert lib.crl_dqn_noisy_create(C.byref(ccfg), C.byref(nopt), 2, None, None, None, 0, C.byref(out)) != 0 and b"dueling" in lib.crl_last_error()
    good = dict(n_atoms=51, v_min=0.0, v_max=100.0)
    for bad, field in ((dict(n_atoms=1), "n_atoms"), (dict(n_atoms=65), "n_atoms"), (dict(v_min=100.0), "v_min"), (dict(v_max=float("inf")), "v_max")):
        with pytest.raises(crl.CrlError, match=field):
            _handle(crl, cfg, c51={**good, **bad})
    with pytest.raises(crl.CrlError, match="n_step"):
        _handle(crl, cfg, tgt=dict(n_step=17, double_q=0))
    with pytest.raises(crl.CrlError, match="double_q"):
        _handle(crl, cfg, tgt=dict(n_step=1, double_q=2), dueling=True)
    with pytest.raises(crl.CrlError, match="alpha"):
        _handle(crl, cfg, per=dict(alpha=2.0, beta_start=0.4, beta_end=1.0, beta_duration=10.0, eps=1e-6))
    with pytest.raises(crl.CrlError, match="batch_size"):
        _handle(crl, O.dqn_config(seed=21, batch_size=2000))
    with pytest.raises(crl.CrlError, match="n_atoms"):
        L.dqn_noisy_make_nn_host(0, 0.5, False, 65)
    h = _handle(crl, cfg)
    assert h.param_count() == 2 * 10934
    for call in (lambda: h.run(10), lambda: h.q_values(np.zeros(4)), lambda: h.evaluate(4)):
        with pytest.raises(crl.CrlError, match="parameters not set"):
            call()
    for size in (10934, 21867, 21869):
        with pytest.raises(crl.CrlError, match="expected 21868 floats"):
            h.write_params(np.zeros(size, np.float32))
    n = C.c_size_t(10934)
    buf = np.zeros(21868, np.float32)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.crl_dqn_read_params(h._h, fp, None, 10934) != 0 and b"expected 21868" in lib.crl_last_error()
    assert lib.crl_dqn_noisy_weights(h._h, 0, fp, 21868) != 0 and b"expected 10934" in lib.crl_last_error()
    assert lib.crl_dqn_noisy_weights(h._h, 2, fp, 10934) != 0 and b"net" in lib.crl_last_error()
    assert lib.crl_dqn_noisy_weights(h._h, 0, None, 10934) != 0
    assert lib.crl_dqn_noisy_noise(h._h, 0, 0, fp, 413) != 0 and b"expected 414" in lib.crl_last_error()
    assert lib.crl_dqn_noisy_noise(h._h, 0, 3, fp, 414) != 0 and b"net" in lib.crl_last_error()
    assert lib.crl_dqn_noisy_noise(None, 0, 0, fp, 414) != 0 and b"null" in lib.crl_last_error()
    for call in (h.per_status, h.c51_read, h.target_read, lambda: h.dueling_streams(np.zeros(4))):
        with pytest.raises(crl.CrlError):
            call()
    h.init_params(3)
    q, t = h.read_params()
    assert np.array_equal(q, t) and np.array_equal(q, L.dqn_noisy_make_nn_host(3, 0.5))
    assert np.all(q[10934:10934 + 600] == np.float32(0.5 / np.sqrt(4.0))) and np.abs(q[:600]).max() <= 0.5
    assert np.array_equal(h.noisy_weights(0), N.image(q[:10934], q[10934:], N.eps_of(N.layers(), h.noisy_noise(0, 0))))
    hd = _handle(crl, cfg, c51=good, dueling=True, per=dict(alpha=0.6, beta_start=0.4, beta_end=1.0, beta_duration=10.0, eps=1e-6))
    assert hd.param_count() == 2 * 33933 and hd.noisy_noise(0, 1).size == 700 + 3 * 51
    hd.init_params(3)
    assert np.array_equal(hd.read_params()[0], L.dqn_noisy_make_nn_host(3, 0.5, True, 51)) and hd.per_status()["tree_leaves"] > 0
    h.close(); hd.close()


# ---------------------------------------------------------------------------------------------------- 8. the entry point
def _records(path):
    return [json.loads(l) for l in open(path)]


def _run_entry(crl, d, **kw):
    cfg = crl.DQNConfig(run_name="t", total_timesteps=2500, epsilon_start=0.0, epsilon_end=0.0) if kw.get("noisy") else crl.DQNConfig(run_name="t", total_timesteps=2500)
    agent = crl.dqn(cfg, seed=9, chunk=700, eval_every=1250, eval_envs=16, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(d), **kw)
    recs = _records(os.path.join(d, "dqn|t.json"))
    strip = lambda r: {k: v for k, v in r.items() if k not in ("steps_per_sec", "time", "timestamp")}
    return agent, [[strip(r) for r in recs if r["msg"] == m] for m in ("Training Statistics", "Episode Statistics", "Evaluation Statistics")]


def test_entry_point_logs_and_is_repeatable(crl, tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / str(i); d.mkdir()
        agent, recs = _run_entry(crl, d, noisy=crl.NoisyOptions())
        assert agent.handle.status()["global_step"] == 2500 and agent.handle.param_count() == 21868
        sig = crl.noisy_sigma(agent)
        assert len(sig) == 6 and all(s > 0.0 for s in sig)
        runs.append((recs, agent.handle.read_params(), sig))
        agent.close()
    (ra, pa, sa), (rb, pb, sb) = runs
    tr, ep, ev = ra
    assert ra == rb and sa == sb and np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert len(tr) == 2 and all(set(r) >= {"loss", "msg"} and r["loss"] > 0.0 and "beta" not in r for r in tr)
    assert len(ep) > 0 and all(r["ϵ"] == 0.0 and {"episode_return", "episode_length", "global_step"} <= set(r) for r in ep)
    assert len(ev) == 2 and all({"eval_return_mean", "eval_return_std", "eval_q_bias"} <= set(r) for r in ev)
    assert not np.array_equal(pa[0], crl.make_nn_noisy(0))
    with pytest.raises(TypeError, match="NoisyOptions"):
        crl.DQNAgent(crl.DQNConfig(), noisy=0.5)
    with pytest.raises(ValueError, match="sigma0"):
        crl.DQNAgent(crl.DQNConfig(), noisy=crl.NoisyOptions(sigma0=-1.0))


def test_entry_point_with_every_component(crl, tmp_path):
    """Rainbow through the entry point: noisy + dueling + C51 + PER + 3-step + double; the records keep their fields (beta comes with PER)"""
    d = tmp_path / "r"; d.mkdir()
    agent, (tr, ep, ev) = _run_entry(crl, d, noisy=crl.NoisyOptions(), dueling=True, dist=crl.C51Options(), per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True))
    assert agent.handle.param_count() == 2 * 33933 and len(crl.noisy_sigma(agent)) == 10
    assert len(tr) == 2 and all(r["loss"] > 0.0 and 0.4 <= r["beta"] <= 1.0 for r in tr) and len(ep) > 0 and len(ev) == 2
    agent.close()


def test_entry_point_without_noisy_is_the_stream_it_was(crl, tmp_path):
    """noisy=None makes a crl_dqn_create handle: its run is bit-identical to oracle/dqn_oracle.c from the same parameters, as it was"""
    d = tmp_path / "p"; d.mkdir()
    agent, (tr, ep, ev) = _run_entry(crl, d, noisy=None)
    assert agent.noisy is None and agent.handle.param_count() == 10934
    cfg = O.dqn_config(total_timesteps=2500, seed=9)
    st = O.DQNState(cfg, crl.make_nn(0))
    _, eps_o, ls_o = st.run(2500)
    assert [(r["episode_return"], r["episode_length"], r["global_step"], r["ϵ"]) for r in ep] == [tuple(e) for e in eps_o]
    assert [r["loss"] for r in tr] == [l[1] for l in ls_o] and len(tr) == 2
    qg, tg = agent.handle.read_params(); qo, to = st.params()
    assert np.array_equal(qg, qo) and np.array_equal(tg, to)
    agent.close(); st.close()


# ---------------------------------------------------------------------------------------------------- 9. learns
LEARN_JSON = os.path.join(B.B.ROOT, "profiles", "noisy_learn.json")
LEARN_SEEDS = (1, 2, 3)


@pytest.mark.parametrize("arm", ["noisy", "rainbow"])
def test_noisy_agent_learns(crl, arm):
    """After 20,000 steps at lr = 1e-3 (the step count and the rate of test_per_agent_learns, for its reasons) with epsilon_start = epsilon_end = 0 —
    exploration by the noise alone — dqn_evaluate of the noisy agent (the noise off) returns strictly more than the same evaluation of its initial
    network: dqn.jl's net with noisy layers, and noisy + dueling + C51 + PER + 3-step + double. Measured first (scripts/noisy_learn.py →
    profiles/noisy_learn.json, eight seeds: all eight learn on both arms; the plain noisy arm's seed 3 only from 8.3 to 23.4); the seeds run here are
    taken from those the profile shows learning."""
    prof = json.load(open(LEARN_JSON))
    rows = prof["runs"][arm]
    assert prof["steps"] == 20_000 and prof["lr"] == 1e-3 and len(rows) == 8
    learned = [s for s, r in rows.items() if r[-1] > r[0]]
    print(f"seeds that learned in the profile: {sorted(learned)} of 8")
    assert all(str(s) in learned for s in LEARN_SEEDS)
    kw = {} if arm == "noisy" else dict(dueling=True, per=crl.PEROptions(), target=crl.DQNTargetOptions(3, True), dist=crl.C51Options())
    for seed in LEARN_SEEDS:
        cfg = crl.DQNConfig(total_timesteps=20_000, lr=1e-3, epsilon_start=0.0, epsilon_end=0.0)
        agent = crl.DQNAgent(cfg, seed=seed, init_seed=seed, noisy=crl.NoisyOptions(), **kw)
        before = crl.dqn_evaluate(agent, num_envs=256)["report"]["return_mean"]
        sigma0 = crl.noisy_sigma(agent)
        agent.handle.run(20_000)
        after = crl.dqn_evaluate(agent, num_envs=256)["report"]["return_mean"]
        print(f"seed {seed}: held-out return_mean {before} -> {after}; mean |sigma| per array {[round(s, 4) for s in sigma0]} -> {[round(s, 4) for s in crl.noisy_sigma(agent)]}")
        assert agent.handle.status()["global_step"] == 20_000 and after > before
        assert before == rows[str(seed)][0] and after == rows[str(seed)][-1], "the recorded run, from its initial network to its last figure"
        agent.close()
