"""On-device TD3 (csrc/ddpg.hip: td3_critic_kernel, td3_critic_step, td3_actor_kernel, td3_actor_step, td3_collect_kernel through the crl_td3_* C
ABI). Two anchors, because the reference has no TD3: the degenerate setting in which TD3 IS DDPG (policy_delay = 1, policy_noise = 0, critic 2 =
critic 1, bounds ±2), bit for bit against a DDPG handle fed the same transitions; and tests/td3_ref.py, the numpy Float64 restatement, on every
case of tests/td3_bar.py's table under the bars of profiles/td3_bar.json (tests/test_td3_cpu.py shows on the CPU what those bars tell apart).
Then the Pendulum handle (determinism, chunking against policy_delay, the warm-up), the errors, crl_ddpg_evaluate on a TD3 handle, the td3()
entry point, and learning."""
import json
import os

import numpy as np
import pytest

import ddpg_bar as DB
import ddpg_ref as R
import td3_bar as B
import td3_ref as T
from test_gpu_ddpg import _cfg, _params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _opt(crl, d):
    return crl._lib.CrlTD3Options(d["policy_delay"], 0, d["policy_noise"], d["noise_clip"])


def _td3(crl, D, A, external, **kw):
    """→ (config dict with the three TD3 fields, TD3Handle)"""
    full = dict(policy_delay=2, policy_noise=0.2, noise_clip=0.5, noise_in_update=0)
    full.update(kw)
    d, c = _cfg(crl, D, A, external, **full)
    return d, crl._lib.TD3Handle(c, _opt(crl, d), 0)


def _nets(crl, D, A, seed):
    actor, c1 = _params(crl, D, A, seed)
    return actor, c1, _params(crl, D, A, seed + 100)[1]


def _same(xs, ys):
    return len(xs) == len(ys) and all(np.array_equal(x, y) for x, y in zip(xs, ys))


# ---------------------------------------------------------------------------------------------------- 1. the degenerate setting is DDPG
@pytest.mark.parametrize("D,A,k,thr", [(3, 1, 7, 10), (49, 16, 31, 40)])
def test_the_degenerate_setting_is_the_ddpg_path_bit_for_bit(crl, D, A, k, thr):
    n = thr + 40
    kw = dict(total_timesteps=n, batch_size=k, min_buff_size=thr, warmup_steps=thr - 5, noise_in_update=0)
    _, c = _cfg(crl, D, A, True, **kw)
    ddpg = crl._lib.DDPGHandle(c, 0)
    _, td3 = _td3(crl, D, A, True, policy_delay=1, policy_noise=0.0, noise_clip=0.5, **kw)
    actor, critic = _params(crl, D, A, 1)
    ddpg.write_params(actor, critic); td3.write_params(actor, critic, critic)
    for tr in DB.transitions(D, A, n, 7):
        ddpg.observe(*tr); td3.observe(*tr)
    a, c1, c2, ta, t1, t2 = td3.read_params()
    da, dc, dta, dtc = ddpg.read_params()
    assert not np.array_equal(a, actor) and not np.array_equal(c1, critic), "both trained"
    assert np.array_equal(a, da) and np.array_equal(ta, dta) and np.array_equal(c1, dc) and np.array_equal(t1, dtc)
    assert np.array_equal(c2, c1) and np.array_equal(t2, t1)
    lt, ld = td3.read_losses(), ddpg.read_losses()
    assert [l[0] for l in lt] == [l[0] for l in ld] == list(range(thr + 1, n + 1))
    assert [l[1] for l in lt] == [l[1] for l in ld]
    assert [l[2] for l in lt] == [2.0 * l[2] for l in ld]
    st, sd = td3.status(), ddpg.status()
    assert st["critic_loss"] == 2.0 * sd["critic_loss"] and {k: v for k, v in st.items() if k != "critic_loss"} == {k: v for k, v in sd.items() if k != "critic_loss"}
    ddpg.close(); td3.close()


# ---------------------------------------------------------------------------------------------------- 2. the case table against td3_ref
@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_the_case_table_matches_the_reference(crl, name):
    case = B.CASE[name]
    D, A, n = case["D"], case["A"], case["T"]
    d = B.case_cfg(case)
    thr = B.threshold(d)
    nets = B.case_params(case)
    d2, h = _td3(crl, D, A, True, **{k: v for k, v in d.items() if k not in ("obs_dim", "act_dim")})
    assert d2 == d
    h.write_params(*nets)
    ref = T.TD3(d, *nets)
    trs = B.case_transitions(case)
    losses, i = [], 0
    for end in sorted({1, thr, thr + 1, (thr + n) // 2, n}):              # the last quiet step, the first update, the middle, the end
        for tr in trs[i:end]:
            h.observe(*tr)
        ref.run_transitions(trs[i:end]); i = end
        st = h.status()
        assert (st["global_step"], st["n_updates"], st["rb_size"], st["rb_ptr"]) == (ref.global_step, ref.n_updates, ref.rb.size, ref.rb.ptr)
        losses += h.read_losses()
    assert ref.n_updates == n - thr and ref.n_actor_steps == sum(g % d["policy_delay"] == 0 for g in range(thr + 1, n + 1))
    rb = h.buffer()
    assert np.array_equal(rb["state"], ref.rb.state) and np.array_equal(rb["action"], ref.rb.action) and np.array_equal(rb["reward"], ref.rb.reward)
    assert np.array_equal(rb["next_state"], ref.rb.next_state) and np.array_equal(rb["terminal"], ref.rb.terminal)
    assert [l[0] for l in losses] == list(range(thr + 1, n + 1))
    params = h.read_params()
    # the edges, on the reference's own numbers and on the device's parameters
    if name == "noise1_clip05":
        assert 0.1 * ref.n_noise <= ref.n_noise_clipped <= 0.9 * ref.n_noise                  # P(|z| > 0.5) = 0.62
    if name == "bounds":
        assert 0 < ref.n_target_clamped < ref.n_target_actions
    if name == "delay_never":
        assert _same((params[0], params[3], params[4], params[5]), (nets[0], nets[0], nets[1], nets[2])), "actor and targets keep their initial bits"
        assert all(l[1] == 0.0 for l in losses) and not np.array_equal(params[1], nets[1]) and not np.array_equal(params[2], nets[2])
    if name == "tau1" and n % d["policy_delay"] == 0:                                          # the last update was an actor step: targets = nets
        assert _same(params[:3], params[3:])
    out = B.distances(losses, params, ref.losses, ref.params(), D, A)
    print(name, out)
    loss_bar, param_bar = B.load_bars()
    for k, v in out.items():
        assert v <= B.bar_of(k, loss_bar, param_bar), (k, v)
        assert v <= B.OLD_BAR, (k, v)
    # crl_td3_q_values / crl_ddpg_q_values
    rng = np.random.default_rng(5)
    obs, act = rng.standard_normal((D, 9)), rng.uniform(-2, 2, (A, 9))
    q1, q2 = h.q_values_both(obs, act)
    assert np.array_equal(q1, h.q_values(obs, act)) and not np.array_equal(q1, q2)
    assert np.abs(q1 - R.q_values(params[1], D, A, obs, act)).max() <= 1e-10 and np.abs(q2 - R.q_values(params[2], D, A, obs, act)).max() <= 1e-10
    h.close()


# ---------------------------------------------------------------------------------------------------- 3. the Pendulum handle
def _pendulum_run(crl, chunks, **kw):
    full = dict(total_timesteps=400, warmup_steps=100, min_buff_size=150, batch_size=32, seed=5, policy_delay=3)
    full.update(kw)
    _, h = _td3(crl, 3, 1, False, **full)
    h.write_params(*_nets(crl, 3, 1, 6))
    taken, eps, losses = 0, [], []
    for n in chunks:
        t, e, l = h.run(n)
        taken += t; eps += e; losses += l
    out = (taken, h.read_params(), h.buffer(), eps, losses, h.status())
    h.close()
    return out


def test_pendulum_runs_are_deterministic_and_chunking_changes_no_bit(crl):
    whole = _pendulum_run(crl, (400,))
    again = _pendulum_run(crl, (400,))
    # chunk sizes that are no multiples of policy_delay = 3, ending mid-warm-up, on and off actor steps
    chunked = _pendulum_run(crl, (149, 2, 1, 7, 100, 41, 100))
    for other in (again, chunked):
        assert other[0] == whole[0] == 400 and _same(other[1], whole[1]) and other[3:] == whole[3:]
        assert all(np.array_equal(other[2][k], whole[2][k]) for k in whole[2])
    st = whole[5]
    assert st["n_updates"] == 250 and [l[0] for l in whole[4]] == list(range(151, 401)) and [e[1:] for e in whole[3]] == [(200, 200), (200, 400)]
    assert whole[4][0][1] == 0.0 == whole[4][1][1] and whole[4][2][1] != 0.0, "actor_loss is 0.0 until the first actor step (g = 153)"
    assert all(whole[4][i][1] == whole[4][i - 1][1] for i in range(3, 250) if (151 + i) % 3 != 0), "and keeps the latest step's value in between"
    # the updates follow the reference on the device's own transitions
    d = DB.cfg_dict(3, 1, total_timesteps=400, warmup_steps=100, min_buff_size=150, batch_size=32, seed=5, policy_delay=3, policy_noise=0.2,
                    noise_clip=0.5, noise_in_update=0)
    rb = whole[2]
    ref = T.TD3(d, *_nets(crl, 3, 1, 6))
    ref.run_transitions([(rb["state"][:, s], rb["action"][:, s], rb["reward"][s], rb["next_state"][:, s], bool(rb["terminal"][s])) for s in range(400)])
    out = B.distances(whole[4], whole[1], ref.losses, ref.params(), 3, 1)
    print(out)
    loss_bar, param_bar = B.load_bars()
    assert all(v <= B.bar_of(k, loss_bar, param_bar) for k, v in out.items()), out


def test_act_during_the_warm_up_is_bit_exact(crl):
    D, A = 17, 6
    d, h = _td3(crl, D, A, True, warmup_steps=6, min_buff_size=3, batch_size=4, act_low=-1.5, act_high=0.75)
    h.write_params(*_nets(crl, D, A, 2))
    for g, tr in enumerate(DB.transitions(D, A, 10, 3), start=1):
        a = h.act(tr[0])
        assert np.array_equal(a, h.act(tr[0])), "asking twice advances nothing"
        if g <= 6:
            assert np.array_equal(a, -1.5 + (0.75 - -1.5) * R.uniform(d["seed"], np.arange(A), g, R.S_WARMUP))
        else:                                                   # DDPG's behaviour policy: one unclipped draw per call on stream 0x10
            ref = R.DDPG(d, *h.read_params()[:2]); ref.global_step = g - 1
            assert np.abs(a - ref.act(tr[0])).max() <= 1e-10
        h.observe(*tr)
    assert h.status()["n_updates"] == 4
    h.close()


# ---------------------------------------------------------------------------------------------------- 4. errors
def test_errors_name_their_field(crl):
    L = crl._lib
    for kw, field in ((dict(policy_delay=0), "policy_delay"), (dict(policy_delay=-3), "policy_delay"), (dict(policy_noise=-0.1), "policy_noise"),
                      (dict(noise_clip=-0.5), "noise_clip"), (dict(noise_in_update=1), "noise_in_update"), (dict(batch_size=0), "batch_size"),
                      (dict(tau=0.0), "tau")):
        with pytest.raises(crl.CrlError, match=field):
            _td3(crl, 3, 1, True, **kw)
    d, c = _cfg(crl, 3, 1, True, noise_in_update=0)
    with pytest.raises(crl.CrlError, match="options"):
        L.TD3Handle(c, None, 0)
    _td3(crl, 3, 1, True, policy_noise=0.0, noise_clip=0.0, policy_delay=1)[1].close()        # the smallest values are accepted
    # the parameter calls come in twins
    _, t = _td3(crl, 3, 1, False)
    p = L.DDPGHandle(_cfg(crl, 3, 1, False)[1], 0)
    z, nets = np.zeros(3), _nets(crl, 3, 1, 1)
    for call in (lambda: t.run(10), lambda: t.actor(z), lambda: t.q_values(z, np.zeros(1)), lambda: t.q_values_both(z, np.zeros(1)),
                 lambda: t.evaluate(4)):
        with pytest.raises(crl.CrlError, match="parameters not set"):
            call()
    for fn, twin, call in (("crl_ddpg_write_params", "crl_td3_write_params", lambda: L.DDPGHandle.write_params(t, nets[0], nets[1])),
                           ("crl_ddpg_init_params", "crl_td3_init_params", lambda: L.DDPGHandle.init_params(t, 1)),
                           ("crl_ddpg_read_params", "crl_td3_read_params", lambda: L.DDPGHandle.read_params(t)),
                           ("crl_td3_write_params", "crl_ddpg_write_params", lambda: L.TD3Handle.write_params(p, *nets)),
                           ("crl_td3_init_params", "crl_ddpg_init_params", lambda: L.TD3Handle.init_params(p, 1)),
                           ("crl_td3_read_params", "crl_ddpg_read_params", lambda: L.TD3Handle.read_params(p)),
                           ("crl_td3_q_values", "crl_ddpg_q_values", lambda: L.TD3Handle.q_values_both(p, z, np.zeros(1)))):
        with pytest.raises(crl.CrlError, match=f"{fn}.*{twin}"):
            call()
    with pytest.raises(crl.CrlError, match="expected"):
        t.write_params(nets[0], nets[1], nets[2][:-1])
    # crl_td3_init_params: make_nn(seed) for the actor and critic 1, the critic of make_nn(seed + 1) for critic 2
    t.init_params(4)
    a, c1, c2, ta, t1, t2 = t.read_params()
    ia, ic = L.ddpg_make_nn_host(3, 1, seed=4)
    assert np.array_equal(a, ia) and np.array_equal(c1, ic) and np.array_equal(c2, L.ddpg_make_nn_host(3, 1, seed=5)[1]) and not np.array_equal(c1, c2)
    assert _same((a, c1, c2), (ta, t1, t2))
    assert t.run(5)[0] == 5
    t.close(); p.close()


# ---------------------------------------------------------------------------------------------------- 5. evaluation on a TD3 handle
def test_evaluate_on_a_td3_handle_is_critic_1s_and_touches_nothing(crl):
    _, h = _td3(crl, 3, 1, False, total_timesteps=300, warmup_steps=100, min_buff_size=50, batch_size=16, max_steps=25, seed=3)
    h.write_params(*_nets(crl, 3, 1, 8))
    assert h.run(230)[0] == 230                                                     # mid-episode, 130 updates, Adam state and targets all moved
    before = (h.read_params(), h.buffer(), h.status())
    n, E = 9, 2
    ev = h.evaluate(n, E, seed=77, trace_steps=E * 25)
    after = (h.read_params(), h.buffer(), h.status())
    assert _same(before[0], after[0]) and before[2] == after[2] and all(np.array_equal(before[1][k], after[1][k]) for k in before[1])
    # follow the device's trajectory with the reference's Pendulum and the handle's own actor / critic calls
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
    # training goes on as if the evaluation had not happened
    _, twin = _td3(crl, 3, 1, False, total_timesteps=300, warmup_steps=100, min_buff_size=50, batch_size=16, max_steps=25, seed=3)
    twin.write_params(*_nets(crl, 3, 1, 8))
    assert twin.run(230)[0] == 230 and twin.run(70) == h.run(70) and _same(twin.read_params(), h.read_params()) and twin.status() == h.status()
    h.close(); twin.close()


# ---------------------------------------------------------------------------------------------------- 6. entry point
def _records(path):
    recs = [json.loads(l) for l in open(path)]
    return [[r for r in recs if r["msg"] == m] for m in ("Episode Statistics", "Training Statistics", "Evaluation Statistics")]


def test_td3_entry_point_logs_the_records_of_ddpg(crl, tmp_path):
    cfg = crl.TD3Config(run_name="t", total_timesteps=1200, warmup_steps=300, log_frequencey=200, policy_delay=2)
    agent = crl.td3(cfg, "pendulum", seed=9, chunk=500, eval_every=600, eval_envs=8, to_terminal=False, to_json=True, to_tensorboard=False,
                    log_dir=str(tmp_path))
    assert isinstance(agent, crl.TD3Agent) and isinstance(agent.handle, crl._lib.TD3Handle)
    st = agent.handle.status()
    assert st["global_step"] == 1200 and st["n_updates"] == 900
    ep, tr, ev = _records(os.path.join(tmp_path, "td3|t.json"))
    assert [r["global_step"] for r in ep] == [200, 400, 600, 800, 1000, 1200] and set(ep[0]) >= {"episode_return", "episode_length", "steps_per_sec"}
    assert len(tr) == 5 and set(tr[0]) >= {"actor_loss", "critic_loss"} and all(r["actor_loss"] != 0.0 and r["critic_loss"] > 0.0 for r in tr)
    assert [r["global_step"] for r in ev] == [600, 1200] and set(ev[0]) >= {"eval_return_mean", "eval_return_std", "eval_q_bias"}
    rep = crl.ddpg_evaluate(agent, num_envs=8)["report"]
    assert ev[1]["eval_return_mean"] == rep["return_mean"] and ev[1]["eval_q_bias"] == rep["q_bias_mean"]
    q = crl.get_q(agent, np.zeros((3, 2)), np.zeros((1, 2)))
    assert q.shape == (2,) and q[0] == q[1] == agent.handle.q_values_both(np.zeros(3), np.zeros(1))[0][0]
    agent.close()


def test_td3_entry_point_with_a_host_env(crl, tmp_path):
    cfg = crl.TD3Config(run_name="x", total_timesteps=1200, warmup_steps=300, log_frequencey=200, policy_delay=3)
    env, eval_env = R.Pendulum(seed=3), R.Pendulum(seed=4, max_steps=20)
    agent = crl.td3(cfg, env, seed=9, eval_every=600, eval_env=eval_env, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(tmp_path))
    st = agent.handle.status()
    assert st["global_step"] == 1200 and st["n_updates"] == 900 and st["rb_size"] == 1200 and env.n_resets == 7 and eval_env.n_resets == 2
    ep, tr, ev = _records(os.path.join(tmp_path, "td3|x.json"))
    assert [r["global_step"] for r in ep] == [200, 400, 600, 800, 1000, 1200] and all(r["episode_length"] == 200 for r in ep)
    assert len(tr) == 5 and set(tr[0]) >= {"actor_loss", "critic_loss"}
    assert [r["global_step"] for r in ev] == [600, 1200]
    rb = agent.handle.buffer()
    assert ep[0]["episode_return"] == pytest.approx(float(np.sum(rb["reward"][:200])), rel=1e-12)
    agent.close()


# ---------------------------------------------------------------------------------------------------- 7. it learns
def test_td3_learns_the_pendulum(crl):
    """Built as test_ddpg_learns_the_pendulum is. Measured first (scripts/td3_train.py → profiles/td3_pendulum_train.json, eight seeds, 20,000
    steps): the threshold is halfway between the random policy's level (the warm-up episodes) and the worst seed's last ten episodes; the block
    of ten episodes is the first one in which every recorded seed is above it; three of those seeds run up to the end of that block here."""
    prof = json.load(open(os.path.join(ROOT, "profiles", "td3_pendulum_train.json")))["td3"]
    threshold = 0.5 * (prof["random_level"] + prof["worst_last10"])
    blocks = [v["block10_mean_returns"] for v in prof["seeds"].values()]
    assert len(blocks) == 8
    first = next(i for i in range(len(blocks[0])) if all(b[i] > threshold for b in blocks))
    assert first >= 1 and not all(b[first - 1] > threshold for b in blocks)
    steps = 2000 * (first + 1)
    pc = prof["config"]
    for seed in (1, 2, 3):
        agent = crl.TD3Agent(crl.TD3Config(total_timesteps=steps, warmup_steps=pc["warmup_steps"], lr=pc["lr"], policy_delay=pc["policy_delay"],
                                           policy_noise=pc["policy_noise"], noise_clip=pc["noise_clip"]), seed=seed, init_seed=seed)
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
