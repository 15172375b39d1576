"""On-device SAC (csrc/sac.hpp: sac_critic_kernel, sac_actor_kernel, sac_actor_step, sac_collect_kernel, with csrc/ddpg.hip's td3_critic_step, through
the crl_sac_* C ABI). The reference has no SAC, so the anchor is tests/sac_ref.py, the numpy Float64 restatement whose gradients
tests/test_sac_cpu.py proves by finite differences: every case of tests/sac_bar.py's table under the bars of profiles/sac_bar.json
(tests/test_sac_bar_cpu.py shows on the CPU what those bars tell apart). Then the Pendulum handle (determinism, chunking, the warm-up, the
behaviour action), crl_ddpg_actor and crl_ddpg_evaluate on a SAC handle, the errors, the sac() entry point, and learning."""
import json
import os

import numpy as np
import pytest

import ddpg_bar as DB
import ddpg_ref as R
import sac_bar as B
import sac_ref as S
from test_gpu_ddpg import _cfg, _params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _sac(crl, D, A, external, **kw):
    """→ (config dict with the three SAC fields, SACHandle)"""
    full = dict(autotune=1, alpha=1.0, target_entropy=-float(A), noise_in_update=0)
    full.update(kw)
    opt = {k: full.pop(k) for k in ("autotune", "alpha", "target_entropy")}
    d, c = _cfg(crl, D, A, external, **full)
    d.update(opt)
    return d, crl._lib.SACHandle(c, crl._lib.CrlSACOptions(opt["autotune"], 0, opt["alpha"], opt["target_entropy"]), 0)


def _nets(crl, D, A, seed):
    """perturbed glorot parameters (non-zero biases): tests/sac_bar.py's actor, test_gpu_ddpg's critics of two draws"""
    return B.actor_params(D, A, seed), _params(crl, D, A, seed)[1], _params(crl, D, A, seed + 100)[1]


def _same(xs, ys):
    return len(xs) == len(ys) and all(np.array_equal(x, y) for x, y in zip(xs, ys))


def feed_case(crl, case, ends, **over):
    """the case's transitions through an external SAC handle and through sac_ref, read at the checkpoints `ends`; asserts the counters at each
    → (config dict, handle, reference, loss records, alpha records)"""
    d = dict(B.case_cfg(case), **over)
    nets = B.case_params(case)
    d2, h = _sac(crl, case["D"], case["A"], True, **{k: v for k, v in d.items() if k not in ("obs_dim", "act_dim")})
    assert d2 == d
    h.write_params(*nets)
    ref = S.SAC(d, *nets)
    trs = B.case_transitions(case)
    losses, arecs, i = [], [], 0
    for end in ends:
        for tr in trs[i:end]:
            h.observe(*tr)
        ref.run_transitions(trs[i:end]); i = end
        st = h.status()
        assert (st["global_step"], st["n_updates"], st["rb_size"], st["rb_ptr"]) == (ref.global_step, ref.n_updates, ref.rb.size, ref.rb.ptr)
        got = h.read_losses()
        losses += got; arecs += h.alpha_records()
        assert len(h.alpha_records()) == len(got)
    return d, h, ref, losses, arecs


def check_case(d, h, ref, losses, arecs, case, loss_bar, param_bar):
    """the ring bit for bit, the records at the reference's steps, every observable under its bar and under OLD_BAR → the distances"""
    D, A, n, thr = case["D"], case["A"], case["T"], B.threshold(d)
    rb = h.buffer()
    assert np.array_equal(rb["state"], ref.rb.state) and np.array_equal(rb["action"], ref.rb.action) and np.array_equal(rb["reward"], ref.rb.reward)
    assert np.array_equal(rb["next_state"], ref.rb.next_state) and np.array_equal(rb["terminal"], ref.rb.terminal)
    want = [g for g in range(thr + 1, n + 1) if g % d["log_frequency"] == 0]
    assert [l[0] for l in losses] == [r[0] for r in arecs] == [l[0] for l in ref.losses] == want and len(want) > 0
    assert ref.n_updates == n - thr
    params = h.read_params()
    out = B.distances(losses, arecs, params[:5], params[5], ref.losses, ref.alpha_records, ref.params(), ref.log_alpha[0], D, A)
    # alpha and the entropy of the records, and the status, against the reference's
    top = max(abs(r[3]) for r in ref.alpha_records)
    out["alpha_record"] = max(abs(a[1] - r[1]) / abs(r[1]) for a, r in zip(arecs, ref.alpha_records))
    out["entropy_record"] = max(abs(a[3] - r[3]) / top for a, r in zip(arecs, ref.alpha_records))
    print(case["name"], out)
    for k, v in out.items():
        assert v <= (loss_bar if k in B.LOSSES + ("alpha_record", "entropy_record") else param_bar), (k, v)
        assert v <= B.OLD_BAR, (k, v)
    st = h.sac_status()
    assert (st["alpha"], st["alpha_loss"], st["entropy"]) == arecs[-1][1:] or d["log_frequency"] > 1
    assert st["log_alpha"] == params[5]
    return out


# ---------------------------------------------------------------------------------------------------- 1. the case table against sac_ref
@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_the_case_table_matches_the_reference(crl, name):
    case = B.CASE[name]
    D, A, n = case["D"], case["A"], case["T"]
    thr = B.threshold(B.case_cfg(case))
    ends = sorted({1, thr, thr + 1, (thr + n) // 2, n})                  # the last quiet step, the first update, the middle, the end
    d, h, ref, losses, arecs = feed_case(crl, case, ends)
    loss_bar, param_bar = B.load_bars()
    check_case(d, h, ref, losses, arecs, case, loss_bar, param_bar)
    params, nets = h.read_params(), B.case_params(case)
    assert not np.array_equal(params[0], nets[0]) and not np.array_equal(params[1], nets[1]) and not np.array_equal(params[2], nets[2])
    if name == "autotune_off":
        assert params[5] == np.float32(np.log(0.2)) and all(r[1] == arecs[0][1] for r in arecs), "log_alpha keeps its initial bits"
        assert all(r[2] != 0.0 for r in arecs), "alpha_loss is still reported"
    else:
        assert params[5] != np.float32(np.log(d["alpha"]))
    if name == "tau1":
        assert _same(params[1:3], params[3:5]), "the targets are the online critics"
    if name == "bounds_asym":
        assert (ref.scale, ref.bias) == (0.75, -0.25)
    # crl_sac_q_values / crl_ddpg_q_values, crl_ddpg_actor
    rng = np.random.default_rng(5)
    obs, act = rng.standard_normal((D, 9)), rng.uniform(-2, 2, (A, 9))
    q1, q2 = h.q_values_both(obs, act)
    assert np.array_equal(q1, h.q_values(obs, act)) and not np.array_equal(q1, q2)
    assert np.abs(q1 - R.q_values(params[1], D, A, obs, act)).max() <= 1e-10 and np.abs(q2 - R.q_values(params[2], D, A, obs, act)).max() <= 1e-10
    mean = S.mean_action(params[0], D, A, obs, ref.scale, ref.bias)
    assert np.abs(h.actor(obs) - mean).max() <= 1e-12 and mean.min() >= d["act_low"] and mean.max() <= d["act_high"]
    h.close()


# ---------------------------------------------------------------------------------------------------- 2. the Pendulum handle
def _pendulum_run(crl, chunks, **kw):
    full = dict(total_timesteps=400, warmup_steps=100, min_buff_size=150, batch_size=32, seed=5)
    full.update(kw)
    _, h = _sac(crl, 3, 1, False, **full)
    h.write_params(*_nets(crl, 3, 1, 6))
    taken, eps, losses, arecs = 0, [], [], []
    for n in chunks:
        t, e, l = h.run(n)
        taken += t; eps += e; losses += l; arecs += h.alpha_records()
    out = (taken, h.read_params(), h.buffer(), eps, losses, h.status(), arecs, h.sac_status())
    h.close()
    return out


def test_pendulum_runs_are_deterministic_and_chunking_changes_no_bit(crl):
    whole = _pendulum_run(crl, (400,))
    again = _pendulum_run(crl, (400,))
    chunked = _pendulum_run(crl, (60, 89, 2, 1, 7, 100, 41, 100))       # ends mid-warm-up (60), on the last quiet step (149), mid-episode
    for other in (again, chunked):
        assert other[0] == whole[0] == 400 and _same(other[1], whole[1]) and other[3:] == whole[3:]
        assert all(np.array_equal(other[2][k], whole[2][k]) for k in whole[2])
    st = whole[5]
    assert st["n_updates"] == 250 and [l[0] for l in whole[4]] == [r[0] for r in whole[6]] == list(range(151, 401))
    assert [e[1:] for e in whole[3]] == [(200, 200), (200, 400)]
    acts = whole[2]["action"][0, :400]
    assert np.all((acts[100:] > -2.0) & (acts[100:] < 2.0)) and len(set(acts.tolist())) == 400
    # the updates follow the reference on the device's own transitions
    d = DB.cfg_dict(3, 1, total_timesteps=400, warmup_steps=100, min_buff_size=150, batch_size=32, seed=5, noise_in_update=0, autotune=1, alpha=1.0,
                    target_entropy=-1.0)
    rb = whole[2]
    ref = S.SAC(d, *_nets(crl, 3, 1, 6))
    ref.run_transitions([(rb["state"][:, s], rb["action"][:, s], rb["reward"][s], rb["next_state"][:, s], bool(rb["terminal"][s])) for s in range(400)])
    out = B.distances(whole[4], whole[6], whole[1][:5], whole[1][5], ref.losses, ref.alpha_records, ref.params(), ref.log_alpha[0], 3, 1)
    print(out)
    loss_bar, param_bar = B.load_bars()
    assert all(v <= B.bar_of(k, loss_bar, param_bar) for k, v in out.items()), out


def test_act_is_the_warm_up_draw_and_then_a_sample_of_the_actor(crl):
    D, A = 17, 6
    d, h = _sac(crl, D, A, True, warmup_steps=6, min_buff_size=3, batch_size=4, act_low=-1.5, act_high=0.75)
    h.write_params(*_nets(crl, D, A, 2))
    for g, tr in enumerate(DB.transitions(D, A, 12, 3), start=1):
        a = h.act(tr[0])
        assert np.array_equal(a, h.act(tr[0])), "asking twice advances nothing"
        if g <= 6:
            assert np.array_equal(a, -1.5 + (0.75 - -1.5) * R.uniform(d["seed"], np.arange(A), g, R.S_WARMUP)), "bit-exact during the warm-up"
        else:                                                   # a sample with ε on stream 0x10, component c, at step g
            ref = S.SAC(d, *h.read_params()[:3]); ref.global_step = g - 1
            want = ref.act(tr[0])
            assert np.abs(a - want).max() <= 1e-12 and np.all((a > -1.5) & (a < 0.75))
            eps = R.normal(d["seed"], np.arange(A), g, R.S_BEHAVE)[:, None]      # the chosen draw: the restatement's action is this ε's, bit for bit
            assert np.array_equal(want, S.sample(ref.actor, D, A, tr[0][:, None], eps, ref.scale, ref.bias)["a"][:, 0])
            other = S.sample(ref.actor, D, A, tr[0][:, None], R.normal(d["seed"], np.arange(A), g + 1, R.S_BEHAVE)[:, None], ref.scale, ref.bias)["a"][:, 0]
            assert np.abs(a - other).max() > 1e-6
        h.observe(*tr)
    assert h.status()["n_updates"] == 6
    h.close()


# ---------------------------------------------------------------------------------------------------- 3. errors
def test_errors_name_their_field(crl):
    L = crl._lib
    for kw, field in ((dict(alpha=0.0), "alpha"), (dict(alpha=-1.0), "alpha"), (dict(alpha=float("nan")), "alpha"),
                      (dict(target_entropy=float("inf")), "target_entropy"), (dict(target_entropy=float("nan")), "target_entropy"),
                      (dict(autotune=2), "autotune"), (dict(autotune=-1), "autotune"), (dict(noise_in_update=1), "noise_in_update"),
                      (dict(batch_size=0), "batch_size"), (dict(tau=0.0), "tau")):
        with pytest.raises(crl.CrlError, match=field):
            _sac(crl, 3, 1, True, **kw)
    d, c = _cfg(crl, 3, 1, True, noise_in_update=0)
    with pytest.raises(crl.CrlError, match="options"):
        L.SACHandle(c, None, 0)
    _sac(crl, 3, 1, True, alpha=1e-300, autotune=0, target_entropy=0.0)[1].close()
    _, s = _sac(crl, 3, 1, False)
    p = L.DDPGHandle(_cfg(crl, 3, 1, False)[1], 0)
    t = L.TD3Handle(_cfg(crl, 3, 1, False, noise_in_update=0)[1], L.CrlTD3Options(2, 0, 0.2, 0.5), 0)
    z, nets = np.zeros(3), _nets(crl, 3, 1, 1)
    dnets = _params(crl, 3, 1, 1)
    for call in (lambda: s.run(10), lambda: s.actor(z), lambda: s.q_values(z, np.zeros(1)), lambda: s.q_values_both(z, np.zeros(1)),
                 lambda: s.evaluate(4)):
        with pytest.raises(crl.CrlError, match="parameters not set — crl_sac_write_params or crl_sac_init_params"):
            call()
    # each kind of handle refuses the other kinds' parameter calls and names the twin
    for fn, twin, call in (("crl_ddpg_write_params", "crl_sac_write_params", lambda: L.DDPGHandle.write_params(s, *dnets)),
                           ("crl_ddpg_init_params", "crl_sac_init_params", lambda: L.DDPGHandle.init_params(s, 1)),
                           ("crl_ddpg_read_params", "crl_sac_read_params", lambda: L.DDPGHandle.read_params(s)),
                           ("crl_td3_write_params", "crl_sac_write_params", lambda: L.TD3Handle.write_params(s, *nets)),
                           ("crl_td3_init_params", "crl_sac_init_params", lambda: L.TD3Handle.init_params(s, 1)),
                           ("crl_td3_read_params", "crl_sac_read_params", lambda: L.TD3Handle.read_params(s)),
                           ("crl_td3_q_values", "crl_sac_q_values", lambda: L.TD3Handle.q_values_both(s, z, np.zeros(1))),
                           ("crl_sac_write_params", "crl_ddpg_write_params", lambda: L.SACHandle.write_params(p, *nets)),
                           ("crl_sac_init_params", "crl_td3_init_params", lambda: L.SACHandle.init_params(t, 1)),
                           ("crl_sac_read_params", "crl_ddpg_read_params", lambda: L.SACHandle.read_params(p)),
                           ("crl_sac_q_values", "crl_td3_q_values", lambda: L.SACHandle.q_values_both(t, z, np.zeros(1))),
                           ("crl_sac_status_read", "crl_ddpg_status_read", lambda: L.SACHandle.sac_status(p)),
                           ("crl_sac_status_read", "crl_ddpg_status_read", lambda: L.SACHandle.sac_status(t)),
                           ("crl_sac_alpha_records", "only a SAC handle", lambda: L.SACHandle.alpha_records(t))):
        with pytest.raises(crl.CrlError, match=f"{fn}.*{twin}"):
            call()
    with pytest.raises(crl.CrlError, match="expected"):
        s.write_params(nets[0][:-2], nets[1], nets[2])
    # crl_sac_init_params: crl_sac_make_nn(seed) — TD3's two critics for the seed, an actor of its own with zero biases
    s.init_params(4)
    a, c1, c2, t1, t2, la = s.read_params()
    ia, ic1, ic2 = L.sac_make_nn_host(3, 1, seed=4)
    assert _same((a, c1, c2), (ia, ic1, ic2)) and _same((c1, c2), (t1, t2)) and la == np.float32(0.0)
    assert np.array_equal(ic1, L.ddpg_make_nn_host(3, 1, seed=4)[1]) and np.array_equal(ic2, L.ddpg_make_nn_host(3, 1, seed=5)[1])
    assert a.size == 64 * 3 + 64 + 64 * 64 + 64 + 2 * 64 + 2 and not a[-2:].any() and a[-130:-2].all() and _same(L.sac_make_nn_host(3, 1, seed=4), (ia, ic1, ic2))
    assert s.sac_status() == dict(alpha=1.0, alpha_loss=0.0, entropy=0.0, log_alpha=np.float32(0.0)) and s.alpha_records() == []
    assert s.run(5)[0] == 5
    s.close(); p.close(); t.close()


# ---------------------------------------------------------------------------------------------------- 4. evaluation on a SAC handle
def test_evaluate_on_a_sac_handle_is_the_deterministic_actor_and_touches_nothing(crl):
    kw = dict(total_timesteps=300, warmup_steps=100, min_buff_size=50, batch_size=16, max_steps=25, seed=3)
    _, h = _sac(crl, 3, 1, False, **kw)
    h.write_params(*_nets(crl, 3, 1, 8))
    taken, _, pending = h.run(230)                                                  # mid-episode, 130 updates: Adam states, targets and alpha all moved
    pending_alpha = h.alpha_records()
    assert taken == 230 and len(pending) == len(pending_alpha) == 130
    before = (h.read_params(), h.buffer(), h.status(), h.sac_status())
    n, E = 9, 2
    ev = h.evaluate(n, E, seed=77, trace_steps=E * 25)
    after = (h.read_params(), h.buffer(), h.status(), h.sac_status())
    assert _same(before[0], after[0]) and before[2:] == after[2:] and all(np.array_equal(before[1][k], after[1][k]) for k in before[1])
    assert h.read_losses() == pending and h.alpha_records() == pending_alpha        # the pending records are still the ones run() left
    for e in range(n):
        for j in range(E):
            th, thd = R.pendulum_reset(77, j * n + e, 0x16)
            t = 0
            for s in range(25):
                obs = R.pendulum_obs(th, thd)
                a = h.actor(obs)[0, 0]
                assert a == ev["trace_action"][j * 25 + s, e]
                if s == 0:
                    q1, q2 = h.q_values_both(obs, np.array([a]))
                    assert ev["q0"][j, e] == q1[0] == h.q_values(obs, np.array([a]))[0] and q1[0] != q2[0]
                th, thd, t, _, _ = R.pendulum_step(th, thd, t, a, 25)
    obs = np.random.default_rng(1).standard_normal((3, 20))
    assert np.abs(h.actor(obs) - S.mean_action(before[0][0], 3, 1, obs, 2.0, 0.0)).max() <= 1e-12
    # Adam states and β powers are not readable; that they are untouched shows in training going on as if the evaluation had not happened
    _, twin = _sac(crl, 3, 1, False, **kw)
    twin.write_params(*_nets(crl, 3, 1, 8))
    assert twin.run(230)[0] == 230 and twin.run(70) == h.run(70) and _same(twin.read_params(), h.read_params()) and twin.status() == h.status()
    assert twin.alpha_records() == h.alpha_records() and twin.sac_status() == h.sac_status() and len(h.alpha_records()) == 70
    h.close(); twin.close()


# ---------------------------------------------------------------------------------------------------- 5. entry points
def _records(path):
    recs = [json.loads(l) for l in open(path)]
    return [[r for r in recs if r["msg"] == m] for m in ("Episode Statistics", "Training Statistics", "Evaluation Statistics")]


def test_sac_entry_point_logs_the_three_kinds_of_record(crl, tmp_path):
    cfg = crl.SACConfig(run_name="t", total_timesteps=1200, warmup_steps=300, log_frequencey=200)
    agent = crl.sac(cfg, "pendulum", seed=9, chunk=500, eval_every=600, eval_envs=8, to_terminal=False, to_json=True, to_tensorboard=False,
                    log_dir=str(tmp_path))
    assert isinstance(agent, crl.SACAgent) and isinstance(agent.handle, crl._lib.SACHandle) and agent.crl_opt.target_entropy == -1.0
    st = agent.handle.status()
    assert st["global_step"] == 1200 and st["n_updates"] == 900
    ep, tr, ev = _records(os.path.join(tmp_path, "sac|t.json"))
    assert [r["global_step"] for r in ep] == [200, 400, 600, 800, 1000, 1200] and set(ep[0]) >= {"episode_return", "episode_length", "steps_per_sec"}
    assert len(tr) == 5 and set(tr[0]) >= {"actor_loss", "critic_loss", "alpha", "alpha_loss", "entropy"}
    assert all(r["critic_loss"] > 0.0 and r["alpha"] > 0.0 for r in tr) and tr[0]["alpha"] != tr[-1]["alpha"] and tr[0]["alpha"] != 1.0
    assert [r["global_step"] for r in ev] == [600, 1200] and set(ev[0]) >= {"eval_return_mean", "eval_return_std", "eval_q_bias"}
    rep = crl.ddpg_evaluate(agent, num_envs=8)["report"]
    assert ev[1]["eval_return_mean"] == rep["return_mean"] and ev[1]["eval_q_bias"] == rep["q_bias_mean"]
    q = crl.get_q(agent, np.zeros((3, 2)), np.zeros((1, 2)))
    assert q.shape == (2,) and q[0] == q[1] == agent.handle.q_values_both(np.zeros(3), np.zeros(1))[0][0]
    agent.close()


def test_sac_entry_point_with_a_host_env(crl, tmp_path):
    cfg = crl.SACConfig(run_name="x", total_timesteps=1200, warmup_steps=300, log_frequencey=200, autotune=False, alpha=0.1, target_entropy=-0.5)
    env, eval_env = R.Pendulum(seed=3), R.Pendulum(seed=4, max_steps=20)
    agent = crl.sac(cfg, env, seed=9, eval_every=600, eval_env=eval_env, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(tmp_path))
    st = agent.handle.status()
    assert st["global_step"] == 1200 and st["n_updates"] == 900 and st["rb_size"] == 1200 and env.n_resets == 7 and eval_env.n_resets == 2
    ep, tr, ev = _records(os.path.join(tmp_path, "sac|x.json"))
    assert [r["global_step"] for r in ep] == [200, 400, 600, 800, 1000, 1200] and all(r["episode_length"] == 200 for r in ep)
    assert len(tr) == 5 and set(tr[0]) >= {"actor_loss", "critic_loss", "alpha", "alpha_loss", "entropy"}
    assert all(r["alpha"] == tr[0]["alpha"] for r in tr) and abs(tr[0]["alpha"] - 0.1) < 1e-8 and agent.handle.read_params()[5] == np.float32(np.log(0.1))
    assert [r["global_step"] for r in ev] == [600, 1200]
    rb = agent.handle.buffer()
    assert ep[0]["episode_return"] == pytest.approx(float(np.sum(rb["reward"][:200])), rel=1e-12)
    agent.close()


# ---------------------------------------------------------------------------------------------------- 6. it learns
def test_sac_learns_the_pendulum(crl):
    """Built as test_td3_learns_the_pendulum is. Measured first (scripts/sac_train.py → profiles/sac_pendulum_train.json, eight seeds, 20,000 steps,
    TD3 and DDPG beside it): the threshold is halfway between the random policy's level (the warm-up episodes) and the worst seed's last ten
    episodes; the block of ten episodes is the first one in which every recorded seed is above it; three of those seeds run up to the end of that
    block here."""
    prof = json.load(open(os.path.join(ROOT, "profiles", "sac_pendulum_train.json")))["sac"]
    threshold = 0.5 * (prof["random_level"] + prof["worst_last10"])
    blocks = [v["block10_mean_returns"] for v in prof["seeds"].values()]
    assert len(blocks) == 8
    first = next(i for i in range(len(blocks[0])) if all(b[i] > threshold for b in blocks))
    assert first >= 1 and not all(b[first - 1] > threshold for b in blocks)
    steps = 2000 * (first + 1)
    pc = prof["config"]
    for seed in (1, 2, 3):
        agent = crl.SACAgent(crl.SACConfig(total_timesteps=steps, warmup_steps=pc["warmup_steps"], lr=pc["lr"], autotune=pc["autotune"], alpha=pc["alpha"],
                                           target_entropy=pc["target_entropy"]), seed=seed, init_seed=seed)
        eps = []
        while True:
            taken, e, _ = agent.handle.run(4000)
            eps += e
            if taken == 0:
                break
        agent.close()
        ret = [r for r, _, _ in eps]
        assert len(ret) == steps // 200
        last10 = float(np.mean(ret[-10:]))
        print(seed, last10, threshold)
        assert last10 > threshold, (seed, last10, threshold)
