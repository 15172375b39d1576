"""The TD3 update kernels (csrc/ddpg.hip: td3_critic_kernel, td3_critic_step, td3_actor_step, td3_finish_update) where they are indexed by the batch,
the ring and the record list — what tests/test_gpu_td3.py's table (k <= 61, no wrap, every step logged, no cap) leaves out. tests/td3_bar.py's
EDGE_CASES against tests/td3_ref.py under the bars of profiles/td3_edges_bar.json (tests/test_td3_edges_cpu.py shows on the CPU what those bars tell
apart: a smoothing draw whose component word wraps at 1024 is invisible at k <= 64 and 3e11 bars away here); the degenerate setting against a
DDPG handle, bit for bit, at the largest, an odd and the default batch — no reference, so a [2][k] stride error shows exactly; then the Pendulum
handle: the 4096-record cap of one call with actor_loss carried across calls, max_losses, and chunking across a wrapping ring."""
import numpy as np
import pytest

import ddpg_bar as DB
import td3_bar as B
import td3_ref as T
from test_gpu_ddpg import _cfg
from test_gpu_td3 import _nets, _pendulum_run, _same, _td3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _feed(crl, case, nets, ends, **over):
    """the case's transitions through a TD3 handle, read at the checkpoints `ends` → (config dict, handle, [status at each checkpoint], records)"""
    d = dict(B.case_cfg(case), **over)
    d2, h = _td3(crl, case["D"], case["A"], True, **{k: v for k, v in d.items() if k not in ("obs_dim", "act_dim")})
    assert d2 == d
    h.write_params(*nets)
    trs = B.case_transitions(case)
    status, losses, i = [], [], 0
    for end in ends:
        for tr in trs[i:end]:
            h.observe(*tr)
        i = end
        status.append(h.status())
        losses += h.read_losses()
    return d, h, status, losses


def _carried(every, delay):
    """[(g, actor_loss, critic_loss)] of a run that logs every update → {g: the actor_loss of the latest actor step <= g}; asserts the carry itself"""
    out, latest = {}, 0.0
    for g, actor_loss, _ in every:
        if g % delay == 0:
            latest = actor_loss
        assert actor_loss == latest, g
        out[g] = latest
    return out


# ---------------------------------------------------------------------------------------------------- 1. the edge table against td3_ref
@pytest.mark.parametrize("name", [c["name"] for c in B.EDGE_CASES])
def test_the_edge_table_matches_the_reference(crl, name):
    case = B.EDGE_CASE[name]
    D, A, n = case["D"], case["A"], case["T"]
    d = B.case_cfg(case)
    thr = B.threshold(d)
    nets = B.case_params(case)
    ends = sorted({1, thr, thr + 1, (thr + n) // 2, n})                   # the last quiet step, the first update, the middle, the end
    _, h, status, losses = _feed(crl, case, nets, ends)
    ref = T.TD3(d, *nets)
    trs = B.case_transitions(case)
    i = 0
    for end, st in zip(ends, status):
        ref.run_transitions(trs[i:end]); i = end
        assert (st["global_step"], st["n_updates"], st["rb_size"], st["rb_ptr"]) == (ref.global_step, ref.n_updates, ref.rb.size, ref.rb.ptr)
    assert ref.n_updates == n - thr and ref.n_actor_steps == sum(g % d["policy_delay"] == 0 for g in range(thr + 1, n + 1)) > 0
    assert ref.rb.size == min(n, d["buffer_size"])
    rb = h.buffer()
    assert np.array_equal(rb["state"], ref.rb.state) and np.array_equal(rb["action"], ref.rb.action) and np.array_equal(rb["reward"], ref.rb.reward)
    assert np.array_equal(rb["next_state"], ref.rb.next_state) and np.array_equal(rb["terminal"], ref.rb.terminal)
    if d["buffer_size"] < n:
        assert status[-1]["rb_ptr"] == n % d["buffer_size"] and status[-1]["rb_size"] == d["buffer_size"], "the ring wrapped"
    assert (d["buffer_size"] < n) == (name in ("kmax_ring_eq_batch", "kmax_a16") + B.EDGE_MULTI_ROUND)
    if case["terminal"] == "none":
        assert not rb["terminal"].any()
    want_steps = [g for g in range(thr + 1, n + 1) if g % d["log_frequency"] == 0]
    assert [l[0] for l in losses] == want_steps and len(want_steps) > 0    # exactly the multiples of log_frequency past the threshold
    params = h.read_params()
    h.close()
    # the edges, on the reference's own numbers
    if name == "kmax_a16":
        assert 0.1 * ref.n_noise <= ref.n_noise_clipped <= 0.9 * ref.n_noise and ref.n_target_clamped > 0
    if name == "bounds_a6":
        assert 0 < ref.n_target_clamped < ref.n_target_actions
    if name in B.EDGE_MULTI_ROUND:
        assert max(DB.case_candidates(case)) > 1024, "a draw went past the first round of candidates"
    out = B.distances(losses, params, ref.losses, ref.params(), D, A)
    print(name, out)
    loss_bar, param_bar = B.load_bars(B.EDGE_BAR_JSON)
    for k, v in out.items():
        assert v <= B.bar_of(k, loss_bar, param_bar), (k, v)
        assert v <= B.OLD_BAR, (k, v)
    if d["log_frequency"] > 1:
        # a record on a step on which the actor did not move carries the latest actor step's loss. The reference's own list first: logging every
        # update changes no number, so its log_frequency = 1 run holds the value every record has to carry
        every = T.TD3(dict(d, log_frequency=1), *nets); every.run_transitions(trs)
        carried = _carried(every.losses, d["policy_delay"])
        assert [l[1] for l in ref.losses] == [carried[g] for g in want_steps]
        off = [j for j, g in enumerate(want_steps) if g % d["policy_delay"] != 0]
        assert len(off) > len(want_steps) // 2 and all(carried[want_steps[j]] == carried[want_steps[j] - want_steps[j] % d["policy_delay"]] for j in off)
        top = max(abs(l[1]) for l in ref.losses)
        assert all(abs(losses[j][1] - carried[want_steps[j]]) / top <= loss_bar for j in off)
        # then the device's: a handle that logs every update holds, bit for bit, what the filtered one logged
        _, h1, _, dev_every = _feed(crl, case, nets, ends, log_frequency=1)
        assert _same(h1.read_params(), params)
        h1.close()
        assert [l[0] for l in dev_every] == list(range(thr + 1, n + 1))
        dev_carried = _carried(dev_every, d["policy_delay"])
        assert losses == [l for l in dev_every if l[0] % d["log_frequency"] == 0]
        assert [l[1] for l in losses] == [dev_carried[g] for g in want_steps] and all(l[1] != 0.0 for l in losses)


# ---------------------------------------------------------------------------------------------------- 2. the degenerate setting is DDPG
@pytest.mark.parametrize("name", ["kmax_ring_eq_batch", "ring200_k199", "k120_default"])
def test_the_degenerate_setting_is_the_ddpg_path_bit_for_bit_at_the_batch_edges(crl, name):
    """tests/test_gpu_td3.py's degenerate test at the shapes of three edge cases: the largest batch on a wrapping ring, an odd one, the default"""
    case = B.EDGE_CASE[name]
    D, A, n = case["D"], case["A"], case["T"]
    kw = dict(case["kw"], total_timesteps=n, noise_in_update=0)
    thr = max(kw["min_buff_size"], kw["warmup_steps"])
    _, c = _cfg(crl, D, A, True, **kw)
    ddpg = crl._lib.DDPGHandle(c, 0)
    _, td3 = _td3(crl, D, A, True, policy_delay=1, policy_noise=0.0, noise_clip=0.5, **kw)
    actor, critic = DB.case_params(case)
    ddpg.write_params(actor, critic); td3.write_params(actor, critic, critic)
    for tr in B.case_transitions(case):
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
    assert st["n_updates"] == n - thr and st["rb_ptr"] == n % kw.get("buffer_size", 1000)
    ddpg.close(); td3.close()


# ---------------------------------------------------------------------------------------------------- 3. the record caps (Pendulum handles)
def _pendulum(crl, **kw):
    _, h = _td3(crl, 3, 1, False, **kw)
    h.write_params(*_nets(crl, 3, 1, 6))
    return h


def test_loss_records_stop_at_4096_per_call_and_actor_loss_is_carried_across_calls(crl):
    kw = dict(total_timesteps=4400, batch_size=1, min_buff_size=10, warmup_steps=5, policy_delay=3, log_frequency=1)
    thr = 10
    h = _pendulum(crl, **kw)
    taken, eps, losses = h.run(4300)
    assert taken == 4300 and h.status()["n_updates"] == 4290 > 4096         # every update is counted
    assert len(losses) == 4096 and [l[0] for l in losses] == list(range(thr + 1, thr + 4097)) and losses[-1][0] == 4106
    taken2, eps2, losses2 = h.run(50)
    assert taken2 == 50 and [l[0] for l in losses2] == list(range(4301, 4351)), "the next call starts a fresh list"
    # a twin driven in chunks holds every record: the capped call lost nothing but the records past its cap
    t = _pendulum(crl, **kw)
    chunks = (1000, 1000, 1000, 1000, 300, 50)
    calls, t_eps = [], []
    for n in chunks:
        tk, e, l = t.run(n)
        assert tk == n and len(l) <= 1000
        t_eps += e; calls.append(l)
    t_losses = [l for call in calls for l in call]
    assert len(t_losses) == 4340 and t_losses[:4096] == losses and t_losses[4290:] == losses2 and t_eps == eps + eps2
    assert _same(h.read_params(), t.read_params()) and h.status() == t.status()
    h.close(); t.close()
    # actor_loss: 0.0 until the first actor step (g = 12), then the latest actor step's value — within a call and across calls
    assert [l[0] for l in t_losses] == list(range(11, 4351))
    assert t_losses[0][1] == 0.0 and t_losses[1][1] != 0.0
    assert all(t_losses[i][1] == t_losses[i - 1][1] for i in range(1, 4340) if t_losses[i][0] % 3 != 0), "it changes only at multiples of 3"
    assert sum(t_losses[i][1] != t_losses[i - 1][1] for i in range(1, 4340) if t_losses[i][0] % 3 == 0) > 1400, "and there it does"
    firsts = []
    for prev, nxt in zip(calls, calls[1:]):
        g = nxt[0][0]
        assert g == prev[-1][0] + 1
        firsts.append(g)
        if g % 3 != 0:                                                       # g = 2001 is an actor step: its record is the new value
            assert nxt[0][1] == prev[-1][1] != 0.0, g
    assert firsts == [1001, 2001, 3001, 4001, 4301] and [g % 3 for g in firsts] == [2, 0, 1, 2, 2]


def test_max_losses_keeps_the_first_records_and_trains_all_the_same(crl):
    kw = dict(total_timesteps=100, max_steps=5, batch_size=4, min_buff_size=10, warmup_steps=5, seed=8)
    h, t = _pendulum(crl, **kw), _pendulum(crl, **kw)
    taken, eps, losses = h.run(60, max_losses=3)
    t_taken, t_eps, t_losses = t.run(60)
    assert taken == t_taken == 60 and len(t_losses) == 50 and eps == t_eps and len(eps) == 12
    assert losses == t_losses[:3] and [l[0] for l in losses] == [11, 12, 13] and losses[0][1] == 0.0 != losses[1][1]
    assert _same(h.read_params(), t.read_params()) and h.status() == t.status() and h.status()["n_updates"] == 50
    rest = h.run(40, max_losses=0)
    assert rest[0] == 40 and rest[2] == [] and t.run(40)[0] == 40            # nothing asked for, everything done
    assert _same(h.read_params(), t.read_params()) and h.status() == t.status() and h.status()["n_updates"] == 90
    h.close(); t.close()


def test_chunking_across_a_wrapping_ring_changes_no_bit(crl):
    kw = dict(buffer_size=128, batch_size=128, min_buff_size=150, warmup_steps=130, policy_delay=3, total_timesteps=400)
    whole = _pendulum_run(crl, (400,), **kw)
    chunked = _pendulum_run(crl, (149, 2, 1, 7, 100, 41, 100), **kw)
    assert chunked[0] == whole[0] == 400 and _same(chunked[1], whole[1]) and chunked[3:] == whole[3:]
    assert all(np.array_equal(chunked[2][k], whole[2][k]) for k in whole[2])
    st = whole[5]
    assert st["n_updates"] == 250 and st["rb_size"] == 128 and st["rb_ptr"] == 400 % 128 == 16
    assert [l[0] for l in whole[4]] == list(range(151, 401)) and whole[4][0][1] == 0.0 == whole[4][1][1] and whole[4][2][1] != 0.0
