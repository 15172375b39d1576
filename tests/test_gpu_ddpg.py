"""The on-device DDPG loop (csrc/ddpg.hip through the crl_ddpg_* C ABI) against the numpy Float64 restatement of ddpg.jl (tests/ddpg_ref.py).
The path has transcendental functions (exp in tanh_fast, log / cos in Box–Muller) whose last bit differs between the device's and the host's
math libraries. How far that may move a loss is measured (scripts/ddpg_bar.py → profiles/ddpg_bar.json: the reference against a twin of itself
with those functions jittered by ±2 ulp), and the bars come from it: losses within loss_bar = 32 × that floor, every parameter array within
2^-21 of its largest magnitude (tests/ddpg_bar.py) — and both within the project's float32 bar of 1e-5, which was the only one before. Everything
without a transcendental (the Pendulum, the ring, the counters, the warm-up actions) is bit-exact. The observed maxima go to
profiles/ddpg_parity.json."""
import json
import os

import numpy as np
import pytest

import ddpg_bar as B
import ddpg_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = B.OLD_BAR


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _record(key, value):
    path = os.path.join(ROOT, "profiles", "ddpg_parity.json")
    try:
        d = json.load(open(path))
    except (OSError, ValueError):
        d = {"bar": BAR, "what": "max |device - ddpg_ref| / max |ddpg_ref| per array (tests/test_gpu_ddpg.py)"}
    d[key] = value
    try:
        with open(path, "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:      # a read-only checkout: the figures were printed
        pass


def _cfg(crl, D, A, external, **kw):
    d = B.cfg_dict(D, A, **kw)
    L = crl._lib
    c = L.CrlDDPGConfig(d["total_timesteps"], d["buffer_size"], d["min_buff_size"], d["batch_size"], d["warmup_steps"], d["log_frequency"], d["lr"],
                        d["tau"], d["gamma"], d["exploration_noise"], D, A, L.DDPG_ENV_EXTERNAL if external else L.DDPG_ENV_PENDULUM, d["max_steps"],
                        d["act_low"], d["act_high"], d["noise_in_update"], 0, d["seed"])
    return d, c


def _params(crl, D, A, seed):
    """perturbed glorot parameters (non-zero biases)"""
    rng = np.random.default_rng(seed)
    a, c = crl.make_ddpg_nn(D, A, seed=seed)
    return (a + (0.05 * rng.standard_normal(a.size)).astype(np.float32), c + (0.05 * rng.standard_normal(c.size)).astype(np.float32))


def _compare(h, ref, D, A, losses):
    """→ dict of the observed maxima (tests/ddpg_bar.py's distances); asserts every logged loss and the four parameter vectors, array by array,
    under the measured loss bar, the 2^-21 parameter bar and the float32 bar"""
    out = B.distances(losses, h.read_params(), ref.losses, B.ref_params(ref), D, A)
    print(out)
    loss_bar, param_bar = B.load_bars()
    for k, v in out.items():
        assert v <= BAR, (k, v)
        assert v <= B.bar_of(k, loss_bar, param_bar), (k, v)
    return out


# ---------------------------------------------------------------------------------------------------- 1. forwards
@pytest.mark.parametrize("D,A", [(3, 1), (1, 1), (17, 6), (64, 16), (48, 16), (49, 16), (64, 1)])
def test_forwards_match_the_reference(crl, D, A):
    _, c = _cfg(crl, D, A, True)
    h = crl._lib.DDPGHandle(c, 0)
    actor, critic = _params(crl, D, A, 3)
    h.write_params(actor, critic)
    rng = np.random.default_rng(D)
    obs = rng.standard_normal((D, 33)); act = rng.uniform(-2, 2, (A, 33))
    obs[:, 0] = 0.0; obs[:, 1] *= 1e-3          # tiny pre-activations: tanh_fast's polynomial branch (x² < 0.017)
    obs[:, 2] *= 400.0; obs[:, 3] *= -400.0     # huge ones: its sign branch (x² > 900)
    h1 = R.actor_forward(actor, D, A, obs)
    W1, b1 = R.split(actor, D, A)[:2]
    z1 = R.dense(W1, b1, obs)
    assert (np.abs(z1[:, :2]) < 0.13).any() and (np.abs(z1[:, 2:4]) > 30).any(), "both branch edges of tanh_fast64 are exercised"
    assert np.abs(h.actor(obs) - h1[2] * 2.0).max() <= 1e-10
    assert np.abs(h.q_values(obs, act) - R.q_values(critic, D, A, obs, act)).max() <= 1e-10
    h.close()


# ---------------------------------------------------------------------------------------------------- 2. transition-fed free run
_transitions = B.transitions


@pytest.mark.parametrize("name,D,A,kw", [
    ("k1", 3, 1, dict(batch_size=1, warmup_steps=5, min_buff_size=10, noise_in_update=1)),                 # warmup_steps < min_buff_size
    ("k7", 3, 1, dict(batch_size=7, warmup_steps=12, min_buff_size=4, noise_in_update=0)),                 # the reverse; not a wave multiple
    ("k32_ring50", 17, 6, dict(batch_size=32, buffer_size=50, min_buff_size=40, warmup_steps=35, noise_in_update=1)),   # the ring wraps six times
])
def test_transition_fed_run_matches_the_reference(crl, name, D, A, kw):
    T = 300
    d, c = _cfg(crl, D, A, True, **kw)
    actor, critic = _params(crl, D, A, 1)
    h = crl._lib.DDPGHandle(c, 0); h.write_params(actor, critic)
    ref = R.DDPG(d, actor, critic)
    trs = _transitions(D, A, T, 7)
    losses, i = [], 0
    for chunk in (1, 7, 50, 100, 142):
        for tr in trs[i:i + chunk]:
            h.observe(*tr)
        ref.run_transitions(trs[i:i + chunk]); i += chunk
        st = h.status()
        assert (st["global_step"], st["n_updates"], st["rb_size"], st["rb_ptr"]) == (ref.global_step, ref.n_updates, ref.rb.size, ref.rb.ptr)
        losses += h.read_losses()
    assert i == T and ref.n_updates == T - max(d["min_buff_size"], d["warmup_steps"])
    rb = h.buffer()
    assert np.array_equal(rb["state"], ref.rb.state) and np.array_equal(rb["action"], ref.rb.action) and np.array_equal(rb["reward"], ref.rb.reward)
    assert np.array_equal(rb["next_state"], ref.rb.next_state) and np.array_equal(rb["terminal"], ref.rb.terminal)
    _record("transition_fed_" + name, _compare(h, ref, D, A, losses))
    with pytest.raises(crl.CrlError, match="total_timesteps"):
        h.observe(*trs[0])
    h.close()


# ---------------------------------------------------------------------------------------------------- 3. crl_ddpg_act
def test_act_warmup_is_bit_exact_and_the_actor_follows_the_reference(crl):
    D, A = 17, 6
    d, c = _cfg(crl, D, A, True, warmup_steps=6, min_buff_size=3, batch_size=4, act_low=-1.5, act_high=0.75)
    actor, critic = _params(crl, D, A, 2)
    h = crl._lib.DDPGHandle(c, 0); h.write_params(actor, critic)
    trs = _transitions(D, A, 12, 3)
    for g, tr in enumerate(trs, start=1):
        a = h.act(tr[0])
        assert np.array_equal(a, h.act(tr[0])), "asking twice advances nothing"
        if g <= 6:
            want = -1.5 + (0.75 - -1.5) * R.uniform(d["seed"], np.arange(A), g, R.S_WARMUP)
            assert np.array_equal(a, want) and (a >= -1.5).all() and (a < 0.75).all()
        else:
            ref = R.DDPG(d, *h.read_params()[:2]); ref.global_step = g - 1
            assert np.abs(a - ref.act(tr[0])).max() <= 1e-10
        assert h.status()["global_step"] == g - 1
        h.observe(*tr)
    assert h.status()["n_updates"] == 6
    h.close()


# ---------------------------------------------------------------------------------------------------- 4. Pendulum run
def test_pendulum_run_ring_is_bit_exact_and_the_updates_follow_the_reference(crl):
    T = 700
    d, c = _cfg(crl, 3, 1, False, total_timesteps=T, warmup_steps=250, min_buff_size=200, batch_size=16, buffer_size=1000, seed=11)
    actor, critic = _params(crl, 3, 1, 4)
    h = crl._lib.DDPGHandle(c, 0); h.write_params(actor, critic)
    st = h.status()
    th, thd = R.pendulum_reset(11, 0, R.S_RESET0)
    assert (st["theta"], st["theta_dot"], st["env_t"], st["global_step"]) == (th, thd, 0, 0)
    total, episodes, losses, ends = 0, [], [], []
    for chunk in (1, 7, 200, 5, 100000):
        taken, eps, ls = h.run(chunk)
        total += taken; episodes += eps; losses += ls
        st = h.status()
        assert st["global_step"] == total
        ends.append((total, st["theta"], st["theta_dot"], st["env_t"]))
    assert total == T and [e[0] for e in ends] == [1, 8, 208, 213, 700]
    rb = h.buffer()
    assert (rb["ptr"], rb["size"]) == (T, T) and h.status()["n_updates"] == T - 250
    # every stored transition reproduces bit-for-bit under the reference's Pendulum from the stored action
    t, ret, n, want_eps = 0, 0.0, 0, []
    ends = {e[0]: e[1:] for e in ends}
    for g in range(1, T + 1):
        s = g - 1
        assert np.array_equal(rb["state"][:, s], R.pendulum_obs(th, thd)), g
        if g <= 250:
            assert rb["action"][0, s] == -2.0 + 4.0 * R.uniform(11, np.arange(1), g, R.S_WARMUP)[0]
        th, thd, t, r, term = R.pendulum_step(th, thd, t, rb["action"][0, s], 200)
        assert rb["reward"][s] == r and rb["terminal"][s] == int(term) and np.array_equal(rb["next_state"][:, s], R.pendulum_obs(th, thd)), g
        ret += r; n += 1
        if term:
            want_eps.append((float(ret), n, g)); ret, n = 0.0, 0
            th, thd = R.pendulum_reset(11, g, R.S_RESET); t = 0
        if g in ends:
            assert ends[g] == (th, thd, t), g
    assert episodes == want_eps and [e[1:] for e in episodes] == [(200, 200), (200, 400), (200, 600)]
    assert not rb["state"][:, T:].any()
    # the same transitions through the reference's transition-fed loop
    ref = R.DDPG(d, actor, critic)
    ref.run_transitions([(rb["state"][:, s], rb["action"][:, s], rb["reward"][s], rb["next_state"][:, s], bool(rb["terminal"][s])) for s in range(T)])
    _record("pendulum_700", _compare(h, ref, 3, 1, losses))
    h.close()


# ---------------------------------------------------------------------------------------------------- 5. determinism
def test_two_runs_from_one_seed_are_bit_identical(crl):
    out = []
    for _ in range(2):
        _, c = _cfg(crl, 3, 1, False, total_timesteps=400, warmup_steps=100, min_buff_size=150, batch_size=32, seed=5)
        h = crl._lib.DDPGHandle(c, 0); h.write_params(*_params(crl, 3, 1, 6))
        recs = [h.run(n) for n in (150, 250)]
        out.append((h.read_params(), h.buffer(), recs, h.status()))
        h.close()
    (p0, b0, r0, s0), (p1, b1, r1, s1) = out
    assert all(np.array_equal(a, b) for a, b in zip(p0, p1)) and r0 == r1 and s0 == s1
    assert all(np.array_equal(b0[k], b1[k]) for k in b0)
    assert s0["n_updates"] == 250 and len(r0[1][2]) == 250


# ---------------------------------------------------------------------------------------------------- 6. edges and errors
def test_budget_and_total_timesteps_edges(crl):
    _, c = _cfg(crl, 3, 1, False, total_timesteps=130, warmup_steps=60, min_buff_size=90, batch_size=8)
    h = crl._lib.DDPGHandle(c, 0); h.write_params(*_params(crl, 3, 1, 1))
    assert h.run(0) == (0, [], [])
    assert h.run(40)[0] == 40 and h.status()["n_updates"] == 0            # the budget ends mid-warm-up
    assert h.run(55)[0] == 55 and h.status()["n_updates"] == 5            # 95 steps: updates at 91..95
    assert h.run(1000)[0] == 35                                            # total_timesteps reached inside the chunk
    st = h.status()
    assert st["global_step"] == 130 and st["n_updates"] == 130 - 90 and st["rb_size"] == 130
    assert h.run(10)[0] == 0
    h.close()
    _, c = _cfg(crl, 3, 1, False, total_timesteps=50, warmup_steps=60, min_buff_size=10)
    h = crl._lib.DDPGHandle(c, 0); h.write_params(*_params(crl, 3, 1, 1))
    assert h.run(1000)[0] == 50 and h.status()["n_updates"] == 0           # max(0, T − max(min_buff_size, warmup_steps))
    h.close()


def test_errors(crl):
    L = crl._lib
    for kw, field in ((dict(batch_size=0), "batch_size"), (dict(batch_size=1025), "batch_size"), (dict(buffer_size=6), "buffer_size"),
                      (dict(buffer_size=131073), "buffer_size"), (dict(min_buff_size=2, warmup_steps=3), "min_buff_size"),
                      (dict(min_buff_size=2, warmup_steps=3), "warmup_steps"), (dict(act_low=1.0, act_high=1.0), "act_low"),
                      (dict(tau=0.0), "tau"), (dict(tau=1.5), "tau")):
        _, c = _cfg(crl, 3, 1, True, **kw)
        with pytest.raises(crl.CrlError, match=field):
            L.DDPGHandle(c, 0)
    for D, A, ext, field in ((0, 1, True, "obs_dim"), (65, 1, True, "obs_dim"), (3, 0, True, "act_dim"), (3, 17, True, "act_dim"), (4, 1, False, "obs_dim")):
        _, c = _cfg(crl, D, A, ext)
        with pytest.raises(crl.CrlError, match=field):
            L.DDPGHandle(c, 0)
    _, c = _cfg(crl, 3, 1, True, buffer_size=131072)
    L.DDPGHandle(c, 0).close()                                             # the largest ring is accepted
    # a fresh handle holds zeros and refuses to run or evaluate
    _, cp = _cfg(crl, 3, 1, False)
    _, ce = _cfg(crl, 3, 1, True)
    hp, he = L.DDPGHandle(cp, 0), L.DDPGHandle(ce, 0)
    z = np.zeros(3)
    for call in (lambda: hp.run(10), lambda: hp.actor(z), lambda: hp.q_values(z, np.zeros(1)), lambda: he.act(z),
                 lambda: he.observe(z, np.zeros(1), 0.0, z, False)):
        with pytest.raises(crl.CrlError, match="parameters not set"):
            call()
    hp.init_params(2); he.init_params(2)
    a, cr, ta, tc = hp.read_params()
    ia, ic = L.ddpg_make_nn_host(3, 1, seed=2)
    assert np.array_equal(a, ia) and np.array_equal(cr, ic) and np.array_equal(a, ta) and np.array_equal(cr, tc)
    # wrong-mode calls
    with pytest.raises(crl.CrlError, match="crl_ddpg_run"):
        he.run(10)
    with pytest.raises(crl.CrlError, match="crl_ddpg_act"):
        hp.act(z)
    with pytest.raises(crl.CrlError, match="crl_ddpg_observe"):
        hp.observe(z, np.zeros(1), 0.0, z, False)
    with pytest.raises(crl.CrlError, match="expected"):
        hp.write_params(a[:-1], cr)
    hp.close(); he.close()


# ---------------------------------------------------------------------------------------------------- 7. entry point
def test_ddpg_entry_point_logs_reference_records(crl, tmp_path):
    cfg = crl.DDPGConfig(run_name="t", total_timesteps=1200, warmup_steps=300, log_frequencey=200)
    agent = crl.ddpg(cfg, "pendulum", seed=9, chunk=500, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(tmp_path))
    st = agent.handle.status()
    assert st["global_step"] == 1200 and st["n_updates"] == 900
    recs = [json.loads(l) for l in open(os.path.join(tmp_path, "ddpg|t.json"))]
    ep = [r for r in recs if r["msg"] == "Episode Statistics"]
    tr = [r for r in recs if r["msg"] == "Training Statistics"]
    assert len(ep) == 6 and set(ep[0]) >= {"episode_return", "episode_length", "steps_per_sec", "global_step"}          # ddpg.jl:97
    assert len(tr) == 5 and set(tr[0]) >= {"actor_loss", "critic_loss"}                                                  # steps 400 … 1200
    q = crl.get_q(agent, np.zeros((3, 2)), np.zeros((1, 2)))
    assert q.shape == (2,) and q[0] == q[1]
    t = crl.polyak_update(np.zeros(2, np.float32), np.ones(2, np.float32), 0.005)
    assert np.array_equal(t, np.full(2, np.float32(0.005)))
    agent.close()


def test_ddpg_entry_point_with_a_host_env(crl, tmp_path):
    cfg = crl.DDPGConfig(run_name="x", total_timesteps=1200, warmup_steps=300, log_frequencey=200)
    env = R.Pendulum(seed=3)
    agent = crl.ddpg(cfg, env, seed=9, to_terminal=False, to_json=True, to_tensorboard=False, log_dir=str(tmp_path))
    st = agent.handle.status()
    assert st["global_step"] == 1200 and st["n_updates"] == 900 and st["rb_size"] == 1200 and env.n_resets == 7
    recs = [json.loads(l) for l in open(os.path.join(tmp_path, "ddpg|x.json"))]
    ep = [r for r in recs if r["msg"] == "Episode Statistics"]
    tr = [r for r in recs if r["msg"] == "Training Statistics"]
    assert [r["global_step"] for r in ep] == [200, 400, 600, 800, 1000, 1200] and all(r["episode_length"] == 200 for r in ep)
    assert set(ep[0]) >= {"episode_return", "episode_length", "steps_per_sec", "global_step"}
    assert len(tr) == 5 and set(tr[0]) >= {"actor_loss", "critic_loss"}
    rb = agent.handle.buffer()
    assert ep[0]["episode_return"] == pytest.approx(float(np.sum(rb["reward"][:200])), rel=1e-12)
    agent.close()


# ---------------------------------------------------------------------------------------------------- 8. it learns
def test_ddpg_learns_the_pendulum(crl):
    """Measured first (scripts/ddpg_train.py → profiles/ddpg_pendulum_train.json, eight seeds, 20,000 steps): the random policy of the warm-up
    scores ≈ −1246 per episode, the worst seed's last ten episodes −212. The fourth block of ten episodes (steps 6,001–8,000) is the first in
    which every recorded seed is above the halfway mark, so three of those seeds run 8,000 steps here and the mean return of their last ten
    episodes must be above halfway between the random level and the worst recorded final level."""
    prof = json.load(open(os.path.join(ROOT, "profiles", "ddpg_pendulum_train.json")))
    threshold = 0.5 * (prof["random_level"] + prof["worst_last10"])
    assert all(v["block10_mean_returns"][3] > threshold for v in prof["seeds"].values())
    assert not all(v["block10_mean_returns"][2] > threshold for v in prof["seeds"].values())
    pc = prof["config"]
    for seed in (1, 2, 3):
        agent = crl.DDPGAgent(crl.DDPGConfig(total_timesteps=8000, warmup_steps=pc["warmup_steps"], lr=pc["lr"]), seed=seed, init_seed=seed)
        eps = []
        while True:
            taken, e, _ = agent.handle.run(4000)
            eps += e
            if taken == 0:
                break
        agent.close()
        ret = [r for r, _, _ in eps]
        assert len(ret) == 40
        last10 = float(np.mean(ret[-10:]))
        print(seed, last10, threshold)
        assert last10 > threshold, (seed, last10, threshold)
