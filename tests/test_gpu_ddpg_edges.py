"""The DDPG update kernels (csrc/ddpg.hip: ddpg_sample_kernel, ddpg_critic_kernel, ddpg_critic_step, ddpg_actor_kernel, ddpg_actor_step) at the edges
of what crl_ddpg_create accepts, against tests/ddpg_ref.py on identical transitions: NI = obs_dim + act_dim at 2, 64, 65 and 80 (the second trip
of the 64-stride loops), act_dim 16, batches that fill the 30-wide unrolled rounds with a remainder of 0 or 1, the default and the largest batch,
draws that need several rounds of 1024 candidates, buffer_size = batch_size, and the hyper-parameter edges. The cases are tests/ddpg_bar.py's table,
the bars profiles/ddpg_bar.json's: on the CPU (tests/test_ddpg_bar_cpu.py) every case was shown to tell ten one-line mutants of the reference
from it by at least ten bars. Then the record caps of crl_ddpg_run (4096 loss records, 8192 episode records per call, max_losses / max_eps)."""
import numpy as np
import pytest

import ddpg_bar as B
import ddpg_ref as R
from test_gpu_ddpg import _cfg, _record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _handle(crl, d, external=True):
    _, c = _cfg(crl, d["obs_dim"], d["act_dim"], external, **{k: v for k, v in d.items() if k not in ("obs_dim", "act_dim")})
    return crl._lib.DDPGHandle(c, 0)


@pytest.mark.parametrize("name", [c["name"] for c in B.CASES])
def test_update_edges_match_the_reference(crl, name):
    case = B.CASE[name]
    D, A, T = case["D"], case["A"], case["T"]
    d = B.case_cfg(case)
    thr = B.threshold(d)
    actor, critic = B.case_params(case)
    h = _handle(crl, d); h.write_params(actor, critic)
    ref = R.DDPG(d, actor, critic)
    trs = B.case_transitions(case)
    losses, i = [], 0
    for end in sorted({1, thr, thr + 1, (thr + T) // 2, T}):              # the last quiet step, the first update, the middle, the end
        for tr in trs[i:end]:
            h.observe(*tr)
        ref.run_transitions(trs[i:end]); i = end
        st = h.status()
        assert (st["global_step"], st["n_updates"], st["rb_size"], st["rb_ptr"]) == (ref.global_step, ref.n_updates, ref.rb.size, ref.rb.ptr)
        losses += h.read_losses()
        if d["tau"] == 1.0:                                                # polyak with tau = 1 copies: (float)(1·w + 0·t) = w
            a, c, ta, tc = h.read_params()
            assert np.array_equal(a, ta) and np.array_equal(c, tc)
            assert np.array_equal(ref.actor, ref.actor_t) and np.array_equal(ref.critic, ref.critic_t)
    assert ref.n_updates == T - thr and ref.rb.size == min(T, d["buffer_size"])
    rb = h.buffer()
    assert np.array_equal(rb["state"], ref.rb.state) and np.array_equal(rb["action"], ref.rb.action) and np.array_equal(rb["reward"], ref.rb.reward)
    assert np.array_equal(rb["next_state"], ref.rb.next_state) and np.array_equal(rb["terminal"], ref.rb.terminal)
    if case["terminal"] != "some":
        assert rb["terminal"][:ref.rb.size].all() if case["terminal"] == "all" else not rb["terminal"].any()
    if d["buffer_size"] < T:
        assert ref.rb.ptr == T % d["buffer_size"], "the ring wrapped"
    if name in B.MULTI_ROUND:
        assert max(B.case_candidates(case)) > 1024, "a draw went past the first round of candidates"
    want_steps = [g for g in range(thr + 1, T + 1) if g % d["log_frequency"] == 0]
    assert [l[0] for l in losses] == want_steps and len(want_steps) > 0    # log_frequency = 7: exactly the multiples of 7 past the threshold
    out = B.distances(losses, h.read_params(), ref.losses, B.ref_params(ref), D, A)
    print(name, out)
    _record("edge_" + name, out)
    loss_bar, param_bar = B.load_bars()
    for k, v in out.items():
        assert v <= B.bar_of(k, loss_bar, param_bar), (k, v)
        assert v <= B.OLD_BAR, (k, v)
    h.close()


# ---------------------------------------------------------------------------------------------------- the record caps (Pendulum handles)
def _pendulum(crl, **kw):
    d = B.cfg_dict(3, 1, **kw)
    h = _handle(crl, d, external=False)
    h.write_params(*B.case_params(B.CASE["tau1"], seed=4))                  # any (3, 1) nets
    return d, h


def test_loss_records_stop_at_4096_per_call_and_the_count_goes_on(crl):
    kw = dict(total_timesteps=4400, batch_size=1, min_buff_size=10, warmup_steps=5, buffer_size=1000, log_frequency=1, seed=21)
    thr = 10
    d, h = _pendulum(crl, **kw)
    taken, eps, losses = h.run(4300)
    assert taken == 4300 and h.status()["n_updates"] == 4300 - thr > 4096   # every update is counted
    assert len(losses) == 4096 and [l[0] for l in losses] == list(range(thr + 1, thr + 4097))
    assert [e[1:] for e in eps] == [(200, 200 * (j + 1)) for j in range(21)]
    taken2, eps2, losses2 = h.run(50)
    assert taken2 == 50 and [l[0] for l in losses2] == list(range(4301, 4351)), "the next call starts a fresh list"
    # a twin driven in chunks of 1000 holds every record: the capped call lost nothing but the records past its cap
    _, t = _pendulum(crl, **kw)
    t_eps, t_losses = [], []
    for n in (1000, 1000, 1000, 1000, 300, 50):
        tk, e, l = t.run(n)
        assert tk == n and len(l) <= 1000
        t_eps += e; t_losses += l
    assert len(t_losses) == 4340 and t_losses[:4096] == losses and t_losses[4290:] == losses2 and t_eps == eps + eps2
    assert all(np.array_equal(a, b) for a, b in zip(h.read_params(), t.read_params())) and h.status() == t.status()
    h.close(); t.close()


def test_episode_records_stop_at_8192_per_call(crl):
    seed, T = 33, 8200
    d, h = _pendulum(crl, total_timesteps=T, max_steps=1, warmup_steps=9000, min_buff_size=10, buffer_size=1000, seed=seed)
    taken, eps, losses = h.run(100000)
    st = h.status()
    assert taken == T and st["global_step"] == T and st["n_updates"] == 0 and losses == [] and len(eps) == 8192
    # one-step episodes in the warm-up: step g starts from the reset drawn at g - 1 (the first from stream S_RESET0) and takes the warm-up action
    for g, (ret, length, gs) in enumerate(eps, start=1):
        th, thd = R.pendulum_reset(seed, g - 1, R.S_RESET0 if g == 1 else R.S_RESET)
        a = -2.0 + 4.0 * R.uniform(seed, np.arange(1), g, R.S_WARMUP)[0]
        _, _, _, r, term = R.pendulum_step(th, thd, 0, a, 1)
        assert term and (ret, length, gs) == (float(r), 1, g), g
    th, thd = R.pendulum_reset(seed, T, R.S_RESET)
    assert (st["theta"], st["theta_dot"], st["env_t"]) == (th, thd, 0)     # the eight episodes past the cap were played all the same
    assert h.run(10) == (0, [], [])
    h.close()


def test_max_eps_and_max_losses_keep_the_first_records(crl):
    kw = dict(total_timesteps=100, max_steps=5, batch_size=4, min_buff_size=10, warmup_steps=5, seed=8)
    _, h = _pendulum(crl, **kw)
    _, t = _pendulum(crl, **kw)
    taken, eps, losses = h.run(60, max_eps=2, max_losses=3)
    t_taken, t_eps, t_losses = t.run(60)
    assert taken == t_taken == 60 and len(t_eps) == 12 and len(t_losses) == 50
    assert eps == t_eps[:2] and losses == t_losses[:3] and [l[0] for l in losses] == [11, 12, 13]
    assert h.run(0, max_eps=0, max_losses=0) == (0, [], [])
    assert h.run(40, max_eps=0, max_losses=0) == (40, [], [])               # nothing asked for, everything done
    assert t.run(40)[0] == 40
    assert all(np.array_equal(a, b) for a, b in zip(h.read_params(), t.read_params())) and h.status() == t.status()
    h.close(); t.close()
