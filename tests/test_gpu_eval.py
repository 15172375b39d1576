"""crl_ppo_evaluate (csrc/eval.hip) on the GPU: teacher-forced parity of the one-launch evaluation against the public calls that define its
trajectory (a twin handle under crl_env_reset / crl_env_step) and the CPU oracle's logits, non-interference with training at bit level,
determinism and keys, bounds, errors, and ppo(eval_every=…).

Bars. Greedy: the traced action is an argmax of the oracle's logits unless the oracle's top-two gap is within twice the project's logit bar
(tests/test_gpu_parity.py: 1e-5 |z| + 1e-6) — then it is one of those two. Sampled: the traced action is the oracle sampler's on the same Philox
uniform unless the draw sits within the 1e-6 CDF-knot margin of tests/test_gpu_envs.py. Both exceptions together may cover at most 1 % of a
case's traced steps (the share is printed). Rewards, dones, returns and lengths are compared bit for bit.

Every GPU step runs under its own watchdog (`limit`): faulthandler ends the process if the step does not return, a hung launch included."""
import contextlib
import ctypes as C
import faulthandler
import json
import logging

import numpy as np
import pytest

import oraclelib as O
from test_gpu_parity import crl  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
SEED = 0x5EED
# cap: the bound the lengths are held to — 500 for CartPole, 200 for the other two. longest: the longest episode the env itself can produce, which
# sizes the trace. They differ for CartPole: RLEnvs ends an episode at t > max_steps = 500, so a pole balanced throughout ends its episode at step 501, and
# the kernel and the header bound the launch by that. The actors of this file (random weights, head scaled to gain 1) drop the pole long
# before either figure, so the bound of 500 holds for every case here; a policy that balances for a whole episode would
# produce 501 and miss it.
ENVS = {"cartpole": dict(kind=0, obs_dim=4, n_act=2, cap=500, longest=501), "mountaincar": dict(kind=3, obs_dim=2, n_act=3, cap=200, longest=200),
        "acrobot": dict(kind=4, obs_dim=6, n_act=3, cap=200, longest=200)}


@contextlib.contextmanager
def limit(seconds):
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _params(crl, name, hidden, seed=3, head=100.0):   # noqa: F811
    """crl_make_actor_critic with the actor head scaled from gain 0.01 to gain 1: logit gaps are O(1), near-ties rare"""
    e = ENVS[name]
    p = crl._lib.make_actor_critic_host(e["obs_dim"], e["n_act"], hidden, seed)
    off = O.param_offsets(_ocfg(name, hidden, 8))
    p[off[4]:off[6]] *= np.float32(head)
    return p


def _ocfg(name, hidden, n):
    e = ENVS[name]
    return O.make_config(num_envs=n, num_steps=8, obs_dim=e["obs_dim"], n_act=e["n_act"], hidden=hidden, env_kind=0 if name == "cartpole" else 1,
                         stale_obs=0, seed=SEED)


def _agent(crl, name, hidden, nt, k=8, params=None, wide=False, monkeypatch=None, **kw):   # noqa: F811
    e = ENVS[name]
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 10)
    if wide:
        monkeypatch.setenv("CRL_FORCE_WIDE", "1")
    try:
        return crl.Agent(cfg, params=params, obs_dim=e["obs_dim"], n_act=e["n_act"], hidden=hidden, env_kind=e["kind"], **({"seed": SEED} | kw))
    finally:
        if wide:
            monkeypatch.delenv("CRL_FORCE_WIDE")


def _oracle_logits(ocfg, params, obs):
    """actor logits of the CPU oracle (orc_mlp_forward, net 0) for the columns of obs (obs_dim, m) -> (m, n_act) float32"""
    m = obs.shape[1]
    x = np.ascontiguousarray(obs.T, np.float32); out = np.zeros((m, ocfg.n_act), np.float32)
    fp = C.POINTER(C.c_float)
    f = O.lib().orc_mlp_forward; cp = C.byref(ocfg); pp = O.fptr(params)
    xb, ob, xs, os_ = x.ctypes.data, out.ctypes.data, x.strides[0], out.strides[0]
    for i in range(m):
        f(cp, pp, 0, C.cast(xb + i * xs, fp), C.cast(ob + i * os_, fp), None, None)
    return out


# ------------------------------------------------------------------------------------------------------------- 1. teacher-forced parity
CASES = [("cartpole", 64, False, 37), ("cartpole", 64, True, 200), ("mountaincar", 64, False, 1000), ("acrobot", 128, False, 200),
         ("acrobot", 256, False, 70)]


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sample"])
@pytest.mark.parametrize("episodes", [1, 3])
@pytest.mark.parametrize("name,hidden,wide,n", CASES, ids=["cartpole-fused", "cartpole-wide", "mountaincar-64", "acrobot-128", "acrobot-256"])
def test_teacher_forced_parity(crl, monkeypatch, name, hidden, wide, n, episodes, greedy):   # noqa: F811
    F = crl._lib; e = ENVS[name]; A = e["n_act"]
    params = _params(crl, name, hidden)
    ocfg = _ocfg(name, hidden, n)
    agent = _agent(crl, name, hidden, 64, params=params, wide=wide, monkeypatch=monkeypatch, seed=99)   # the handle's own seed and size do not matter
    twin = _agent(crl, name, hidden, n, params=params, wide=wide, monkeypatch=monkeypatch, seed=SEED, stale_obs=False, env_id_offset=0)
    T = episodes * e["longest"]                                       # every step the launch can take is traced
    with limit(120):
        out = agent.handle.evaluate(n, episodes, F.EVAL_GREEDY if greedy else F.EVAL_SAMPLE, seed=SEED, trace_steps=T)
    trace, rets, lens = out["trace"], out["returns"], out["lengths"]
    th = twin.handle
    with limit(60):
        th.env_reset()
        cur = th.read(F.F_CUR_OBS)
    ep_idx = np.zeros(n, np.int64); run_ret = np.zeros(n, np.float32); run_len = np.zeros(n, np.int32)
    want_ret = np.zeros((episodes, n), np.float32); want_len = np.zeros((episodes, n), np.int32)
    traced = soft = 0
    for g in range(T):
        live = ep_idx < episodes
        act = trace[g]
        assert np.array_equal(act == -1, ~live), f"step {g}: the trace is -1 exactly for the envs that finished their quota"
        if not live.any():
            assert (trace[g:] == -1).all()
            break
        idx = np.flatnonzero(live); a_live = act[idx]
        assert ((a_live >= 0) & (a_live < A)).all()
        traced += idx.size
        if greedy:
            z = _oracle_logits(ocfg, params, cur[:, idx]).astype(np.float64)
            order = np.argsort(-z, axis=1, kind="stable")
            top, second = order[:, 0], order[:, 1]
            z1, z2 = z[np.arange(idx.size), top], z[np.arange(idx.size), second]
            undecided = (z1 - z2) <= 2 * (1e-5 * np.maximum(np.abs(z1), np.abs(z2)) + 1e-6)
            assert np.array_equal(a_live[~undecided], top[~undecided]), f"step {g}: greedy action is not the oracle's argmax"
            assert ((a_live == top) | (a_live == second))[undecided].all(), f"step {g}: an undecided step took neither of the top two"
            soft += int(undecided.sum())
        else:
            u = np.array([O.lib().orc_u53(SEED, int(i), g, 0) for i in idx])
            a_o, _, _, margin = O.get_action(ocfg, params, cur[:, idx], u, with_value=False)
            knot = margin <= 1e-6
            assert np.array_equal(a_live[~knot], a_o[~knot]), f"step {g}: sampled action differs from the oracle sampler away from a CDF knot"
            soft += int(knot.sum())
        with limit(60):
            cur, rew, done = th.env_step(np.where(live, act, 0).astype(np.int32), gstep=g)   # finished envs idle along: nobody looks at them again
        run_ret[idx] = run_ret[idx] + rew[idx]                                              # Float32 running sum in step order
        run_len[idx] += 1
        fin = idx[done[idx].astype(bool)]
        want_ret[ep_idx[fin], fin] = run_ret[fin]; want_len[ep_idx[fin], fin] = run_len[fin]
        ep_idx[fin] += 1; run_ret[fin] = 0; run_len[fin] = 0
    assert (ep_idx == episodes).all(), "every env finishes its quota inside the step bound"
    assert np.array_equal(want_ret, rets) and np.array_equal(want_len, lens), "the twin's rewards and dones reproduce returns and lengths exactly"
    share = soft / traced
    print(f"{name} {hidden} wide={wide} n={n} episodes={episodes} {'greedy' if greedy else 'sample'}: {traced} traced steps, "
          f"{soft} undecided / knot steps ({100 * share:.4f} %)")
    assert share <= 0.01
    agent.close(); twin.close()


# ------------------------------------------------------------------------------------------------------------- 2. non-interference
STATE_FIELDS = ("F_PARAMS", "F_ADAM_M", "F_ADAM_V", "F_BETAP", "F_ENV_STATE", "F_CUR_OBS", "F_ENV_T", "F_NEXT_DONE")


def _snapshot(crl, h):   # noqa: F811
    F = crl._lib
    return {f: h.read(getattr(F, f)).copy() for f in STATE_FIELDS} | {"episodes": h.episode_stats(), "iteration": h.iteration}


def _same(a, b):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
        else:
            assert a[k] == b[k], k


def _training_agent(crl, wide, monkeypatch, options=None):   # noqa: F811
    if wide:
        return _agent(crl, "acrobot", 128, 64, k=32, params=_params(crl, "acrobot", 128, head=1.0), options=options or {})
    return _agent(crl, "cartpole", 64, 64, k=32, params=_params(crl, "cartpole", 64, head=1.0), options=options or {})


@pytest.mark.parametrize("wide", [False, True], ids=["fused", "layer-wise"])
def test_evaluate_does_not_disturb_training(crl, monkeypatch, wide):   # noqa: F811
    """Three crl_ppo_iterate iterations, each with its loss records read back, with and without an evaluate call after each. Reading the records
    settles the speculation guard, so here every evaluate call meets a CLOSED guard window (the layer-wise path has none at all); the open window is
    test_evaluate_inside_an_open_guard_window's."""
    F = crl._lib
    runs = []
    for with_eval in (False, True):
        agent = _training_agent(crl, wide, monkeypatch); h = agent.handle
        records = []
        for it in range(3):
            with limit(120):
                records.append(h.iterate(1))
                if with_eval:
                    ev = h.evaluate(100, 2, F.EVAL_SAMPLE if it == 1 else F.EVAL_GREEDY, seed=7 + it, trace_steps=5 if it == 2 else 0)
                    assert ev["report"]["episodes"] == 200
        with limit(60):
            runs.append((records, _snapshot(crl, h)))
        agent.close()
    (rec0, snap0), (rec1, snap1) = runs
    assert json.dumps(rec0) == json.dumps(rec1), "loss records differ"
    assert snap0["iteration"] == 3
    _same(snap0, snap1)


@pytest.mark.parametrize("speculation", ["holds", "fails"])
def test_evaluate_inside_an_open_guard_window(crl, monkeypatch, speculation):   # noqa: F811
    """The fused path's speculation guard (the layer-wise path has none). With guard_window = 8, crl_ppo_iterate(1, stats = NULL) reads nothing back and
    leaves the window open: one, two, then three iterations deep when the three evaluate calls come. A fourth iteration then hands out its loss
    records — the first host read of the run without evaluate calls, which carried its window through all three iterations — and the state is
    compared bit for bit.

    holds: ordinary parameters, the speculation u = mean(v - R^2) <= 0 holds; settling reads the flag and changes nothing.
    fails: gamma = 0 and a critic bias of 5 (tests/test_gpu_parity.py) fail it in every iteration, which makes the open window observable:
    crl_ppo_exact_reruns stands still after crl_ppo_iterate (nothing settled: the window is open) and has grown by the one iteration of the window
    after the evaluate call (the call settled it first, like every entry point that reads state). The run without evaluate calls replays its
    three iterations in one go at the first read; the exact replay is deterministic, so both runs end in the same bits."""
    F = crl._lib; fails = speculation == "fails"
    nt, k = 64, 32
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 10, gamma=0.0 if fails else 0.99)
    params = _params(crl, "cartpole", 64, head=1.0)
    if fails:
        params[O.param_offsets(_ocfg("cartpole", 64, nt))[11]] = 5.0   # critic head bias
    runs = []
    for with_eval in (False, True):
        agent = crl.Agent(cfg, params=params, seed=SEED, options={"guard_window": 8}); h = agent.handle
        assert h.get_option("guard_window") == 8
        for it in range(3):
            with limit(120):
                assert h.iterate(1, want_stats=False) is None
                before = h.exact_reruns                                # a host counter: reading it settles nothing
                if with_eval:
                    assert before == (it if fails else 0), "crl_ppo_iterate without a read-back must leave the guard window open"
                    ev = h.evaluate(100, 2, F.EVAL_SAMPLE if it == 1 else F.EVAL_GREEDY, seed=7 + it, trace_steps=5 if it == 2 else 0)
                    assert ev["report"]["episodes"] == 200
                    assert h.exact_reruns == (it + 1 if fails else 0), "evaluate settles the open window before it reads the parameters"
                else:
                    assert before == 0, "three iterations deep and nothing settled: the window is open"
        with limit(120):
            records = h.iterate(1)                                     # the fourth iteration's loss records: everything before feeds them
            assert h.exact_reruns == (4 if fails else 0)
            if fails:
                assert max(r["n_unclipped_wins"] for r in records) > 0, "the case must take the u > q branch"
            runs.append((records, _snapshot(crl, h)))
        agent.close()
    (rec0, snap0), (rec1, snap1) = runs
    assert json.dumps(rec0) == json.dumps(rec1), "loss records differ"
    assert snap0["iteration"] == 4
    _same(snap0, snap1)


@pytest.mark.parametrize("wide", [False, True], ids=["fused", "layer-wise"])
def test_evaluate_between_async_iterations(crl, monkeypatch, wide):   # noqa: F811
    """crl_ppo_iterate_async hands out the records of the iteration before. An evaluate call between two of them comes while the status slot of the
    iteration just enqueued is staged and not yet handed over: the slot must survive it, so the stream — loss records, episode statistics and
    per-episode records of every report — is bit-equal to the run without evaluate calls and still exactly one iteration late, and so is the final
    state. On the fused path the default guard window of 8 stays open over all four iterations (crl_ppo_iterate_async settles only a window that is
    full or whose slot arrives with the flag up), so both evaluate calls of that leg also come one and two iterations into an open window and settle
    it; the layer-wise path has no guard."""
    F = crl._lib
    runs = []
    for with_eval in (False, True):
        agent = _training_agent(crl, wide, monkeypatch); h = agent.handle
        h.episode_ring_enable(256)
        stream = []
        for it in range(4):
            with limit(120):
                rep = h.iterate_async()
                assert (rep is None) == (it == 0) and (rep is None or rep["iteration"] == it - 1), "one iteration late"
                stream.append(rep)
                if with_eval and it in (0, 2):
                    ev = h.evaluate(64, 1, F.EVAL_GREEDY, seed=11)      # iteration `it` is pending in its slot
                    assert ev["report"]["episodes"] == 64 and h.iteration == it + 1
        with limit(120):
            last = h.drain()
            assert last["iteration"] == 3 and h.drain() is None
            stream.append(last)
            runs.append((stream, _snapshot(crl, h)))
        agent.close()
    assert [r and r["iteration"] for r in runs[1][0]] == [None, 0, 1, 2, 3]
    assert json.dumps(runs[0][0]) == json.dumps(runs[1][0]), "the pipelined record stream differs"
    _same(runs[0][1], runs[1][1])


# ------------------------------------------------------------------------------------------------------------- 3. determinism and keys
@pytest.mark.parametrize("name,hidden", [("cartpole", 64), ("acrobot", 256)])
def test_determinism_and_keys(crl, monkeypatch, name, hidden):   # noqa: F811
    F = crl._lib; n = 96
    params = _params(crl, name, hidden)
    agent = _agent(crl, name, hidden, 64, params=params); h = agent.handle
    with limit(120):
        a = h.evaluate(n, 2, F.EVAL_SAMPLE, seed=SEED, trace_steps=40)
        b = h.evaluate(n, 2, F.EVAL_SAMPLE, seed=SEED, trace_steps=40)
        c = h.evaluate(n, 2, F.EVAL_SAMPLE, seed=SEED + 1, trace_steps=40)
    for k in ("returns", "lengths", "trace"):
        assert np.array_equal(a[k], b[k]), k
    assert a["report"] == b["report"]
    assert not np.array_equal(a["trace"], c["trace"]), "another seed draws other initial states and uniforms"
    # the first sampled action is the one a same-seed rollout takes at step 0 of iteration 0 (same initial state, same Philox draw), away from knots
    twin = _agent(crl, name, hidden, n, k=8, params=params, seed=SEED, stale_obs=False); th = twin.handle
    with limit(120):
        th.env_reset()
        obs0 = th.read(F.F_CUR_OBS).copy()
        th.rollout_run()
        first = th.read(F.F_ACTION)[:, 0]
    u = np.array([O.lib().orc_u53(SEED, i, 0, 0) for i in range(n)])
    _, _, _, margin = O.get_action(_ocfg(name, hidden, n), params, obs0, u, with_value=False)
    away = margin > 1e-6
    assert away.mean() > 0.9 and np.array_equal(a["trace"][0][away], first[away])
    # other seed, other initial states: the twin of seed + 1 starts elsewhere
    other = _agent(crl, name, hidden, n, k=8, params=params, seed=SEED + 1, stale_obs=False)
    with limit(60):
        other.handle.env_reset()
        assert not np.array_equal(other.handle.read(F.F_CUR_OBS), obs0)
    for x in (agent, twin, other):
        x.close()


# ------------------------------------------------------------------------------------------------------------- 4. bounds and the report
@pytest.mark.parametrize("name,hidden,n,episodes", [("cartpole", 64, 257, 2), ("mountaincar", 128, 100, 1), ("acrobot", 64, 33, 3)])
@pytest.mark.parametrize("greedy", [True, False])
def test_bounds_and_report(crl, monkeypatch, name, hidden, n, episodes, greedy):   # noqa: F811
    F = crl._lib
    agent = _agent(crl, name, hidden, 64, params=_params(crl, name, hidden)); h = agent.handle
    with limit(120):
        out = h.evaluate(n, episodes, F.EVAL_GREEDY if greedy else F.EVAL_SAMPLE, seed=21)
    ret, length, rep = out["returns"], out["lengths"], out["report"]
    assert ret.shape == length.shape == (episodes, n)
    assert (length >= 1).all() and (length <= ENVS[name]["cap"]).all()
    assert rep["episodes"] == n * episodes and rep["env_steps"] == int(length.astype(np.int64).sum())
    # Float64 recomputation, sums in array order (np.cumsum adds sequentially, like the library's loops)
    r = ret.astype(np.float64).ravel(); N = r.size
    mean = np.cumsum(r)[-1] / N
    std = np.sqrt(np.cumsum((r - mean) * (r - mean))[-1] / N)
    assert rep["return_mean"] == mean and rep["return_std"] == std and rep["return_min"] == r.min() and rep["return_max"] == r.max()
    assert rep["length_mean"] == np.cumsum(length.astype(np.float64).ravel())[-1] / N
    if name == "cartpole":
        assert np.array_equal(ret, np.maximum(length - 1, 0).astype(np.float32))   # reward 1 per step but the last
    else:
        assert ((ret == -(length - 1)) | (ret == -length)).all()
    with limit(120):
        only = h.evaluate(n, episodes, F.EVAL_GREEDY if greedy else F.EVAL_SAMPLE, seed=21, want_arrays=False)   # NULL arrays: the report alone
    assert only == {"report": rep}
    agent.close()


# ------------------------------------------------------------------------------------------------------------- 5. errors
def test_errors_name_the_problem_and_leave_the_handle_usable(crl, monkeypatch):   # noqa: F811
    F = crl._lib; L = F.load()
    agent = _agent(crl, "acrobot", 64, 64, params=_params(crl, "acrobot", 64)); h = agent.handle

    def call(cfg, rep=True, ret=None, ln=None, tr=None, handle=None):
        r = F.CrlEvalReport()
        return L.crl_ppo_evaluate(h._h if handle is None else handle, None if cfg is None else C.byref(cfg), C.byref(r) if rep else None, ret, ln, tr)

    def cfg(n=8, e=1, mode=0, t=0):
        return F.CrlEvalConfig(n, e, mode, t, 1)

    tr = (C.c_int32 * 64)()
    cases = [(dict(cfg=None), "null cfg"), (dict(cfg=cfg(), rep=False), "null cfg or report"), (dict(cfg=cfg(n=0)), "num_envs"),
             (dict(cfg=cfg(e=0)), "episodes_per_env"), (dict(cfg=cfg(mode=2)), "unknown mode"), (dict(cfg=cfg(t=-1)), "trace_steps"),
             (dict(cfg=cfg(t=4)), "trace_action"), (dict(cfg=cfg(t=0), tr=tr), "trace_action"),
             (dict(cfg=cfg(n=(1 << 20) + 1)), "cap"), (dict(cfg=cfg(e=4097)), "cap"), (dict(cfg=cfg(n=1 << 20, e=32)), "cap"),
             (dict(cfg=cfg(n=1 << 20, t=128), tr=tr), "cap")]
    for kw, word in cases:
        with limit(60):
            assert call(**kw) != 0, kw
        assert word in L.crl_last_error().decode(), (word, L.crl_last_error())
    with limit(120):
        assert h.evaluate(8, 1)["report"]["episodes"] == 8          # still usable
    agent.close()
    pcfg = crl.PPOConfig(num_envs=64, num_steps=8, total_timesteps=64 * 8 * 10)
    for kind in (F.ENV_SYNTHETIC, F.ENV_EXTERNAL):
        a = crl.Agent(pcfg, obs_dim=6, n_act=3, hidden=64, env_kind=kind)
        with limit(60), pytest.raises(crl.CrlError, match="stateful on-device env"):
            a.handle.evaluate(8, 1)
        a.close()
    # a fresh handle holds zeros: refused, and usable once the parameters are there
    e = ENVS["acrobot"]
    fresh = F.Handle(F.CrlConfig(64 * 8 * 10, 8, 64, 4, 4, 2.5e-4, 0.99, 0.95, 0.2, 0.01, 0.5, 1, 1, 1, e["obs_dim"], e["n_act"], 64, F.GAE_COMPAT, e["kind"],
                                 1, 0, F.SHUFFLE_BLOCKED_FY, SEED), 0)
    with limit(60), pytest.raises(crl.CrlError, match="parameters not set"):
        fresh.evaluate(8, 1)
    with limit(120):
        fresh.init_params(1)
        assert fresh.evaluate(8, 1)["report"]["episodes"] == 8
    fresh.close()


# ------------------------------------------------------------------------------------------------------------- 6. ppo(eval_every=2)
def test_ppo_eval_every_emits_evaluation_records(crl, monkeypatch, tmp_path):   # noqa: F811
    nt, k, updates = 64, 32, 5
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * updates)
    streams = []
    for every in (0, 2):
        run = f"eval-every-{every}"
        with limit(300):
            crl.ppo(cfg, env="acrobot", hidden=64, eval_every=every, eval_envs=64, eval_episodes=1, run_name=run,
                    logger_kw=dict(to_tensorboard=False, to_json=True, log_dir=str(tmp_path)))
        logging.getLogger("CleanRL").handlers.clear()
        recs = [json.loads(line) for line in open(tmp_path / f"{run}.json")]
        for r in recs:
            r.pop("steps_per_sec", None)                             # wall-clock
        streams.append([(r.pop("msg"), r) for r in recs])
    base, withev = streams
    assert not [m for m, _ in base if m == "Evaluation Statistics"]
    evs = [kv for m, kv in withev if m == "Evaluation Statistics"]
    assert [kv["global_step"] for kv in evs] == [2 * nt * k, 4 * nt * k]
    for kv in evs:
        assert set(kv) == {"eval_return_mean", "eval_return_std", "eval_length_mean", "global_step"}
        assert -200 <= kv["eval_return_mean"] <= 0 and 1 <= kv["eval_length_mean"] <= 200 and kv["eval_return_std"] >= 0
    assert [r for r in withev if r[0] != "Evaluation Statistics"] == base, "the other records are those of eval_every = 0"
    # each evaluation record follows the training records of its own update
    pos = [i for i, (m, _) in enumerate(withev) if m == "Evaluation Statistics"]
    n_train = lambda upto: sum(1 for m, _ in withev[:upto] if m == "Training Statistics")   # noqa: E731
    per_update = cfg.update_epochs * cfg.num_minibatches
    assert [n_train(p) for p in pos] == [2 * per_update, 4 * per_update]
