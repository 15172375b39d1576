"""The DQN update kernels (csrc/dqn.hip) and the minibatch draw (csrc/replay_sample.hpp) at the edges of what crl_dqn_create accepts, under the bar of
tests/test_gpu_dqn.py — BIT-EXACT against oracle/dqn_oracle.c: batch sizes 1 and 1024 (the `o / (QH·k)` decompositions of dqn_fwd* / dqn_bwd*, the
block of dqn_td_kernel<false, false>), remainders 29, 1 and 1 + two rounds of dqn_wgrad_kernel's 30-wide unrolled sample loops, draws of the whole ring and of all
but one slot that need several rounds of 1024 candidates, a ring of 65536 slots (the high words of the draw's bitmap), gamma 0, a greedy-only run.
Then the per-call record buffers, filled past their ends: 4096 loss records and 8192 episode records."""
import numpy as np
import pytest

import ddpg_bar as DB
import ddpg_ref as DR
import oraclelib as O

pytestmark = pytest.mark.gpu

DQN_MAX_EPS, DQN_MAX_LOSSES = 8192, 4096      # csrc/dqn.hip
SEED = 21

# name → (oracle config keywords, the edge). lr = 1e-3 as in tests/test_gpu_dqn.py; every update is logged unless the case says otherwise.
CASES = {
    "k1": (dict(total_timesteps=300, batch_size=1, buffer_size=1, min_buff_size=1, train_freq=1, target_net_freq=1), "smallest everything"),
    "k29": (dict(total_timesteps=600, batch_size=29, buffer_size=29, min_buff_size=29), "k = n; unroll remainder 29"),
    "k31": (dict(total_timesteps=600, batch_size=31, buffer_size=31, min_buff_size=40, train_freq=3), "unroll remainder 1; the ring wraps"),
    "k61": (dict(total_timesteps=700, batch_size=61, buffer_size=64), "two unrolled rounds + 1"),
    "k1024": (dict(total_timesteps=1400, batch_size=1024, buffer_size=1024, min_buff_size=1024, train_freq=25),
              "the largest batch; k = n; draws of several rounds"),
    "k1023": (dict(total_timesteps=1400, batch_size=1023, buffer_size=1024, min_buff_size=1024, train_freq=25), "k = n - 1 over several rounds"),
    "cap65536": (dict(total_timesteps=66_600, buffer_size=65_536, min_buff_size=65_000, train_freq=500, log_frequency=500),
                 "the largest ring: every word of the draw's bitmap"),
    "gamma0": (dict(total_timesteps=400, gamma=0.0), "gamma = 0: the TD target is the reward"),
    "eps0": (dict(total_timesteps=600, epsilon_start=0.0, epsilon_end=0.0), "every step greedy"),
}
MULTI_ROUND = ("k1024", "k1023")


def _ocfg(**kw):
    return O.dqn_config(**{"lr": 1e-3, "log_frequency": 1, "seed": SEED, **kw})


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


def _pair(crl, ocfg, params):
    """the library's handle and the oracle's state on one configuration (the two config structs have the same fields in the same order)"""
    L = crl._lib
    assert [f for f, _ in L.CrlDQNConfig._fields_] == [f for f, _ in O.DQNConfigC._fields_]
    h = L.DQNHandle(L.CrlDQNConfig(*[getattr(ocfg, f) for f, _ in O.DQNConfigC._fields_]), 0)
    h.write_params(params)
    return h, O.DQNState(ocfg, params)


def _same_state(h, st, total):
    sg, so = h.status(), st.env()
    assert sg["global_step"] == so["global_step"] == total and sg["rb_size"] == so["rb_size"]
    assert sg["n_updates"] == so["n_updates"] and sg["last_loss"] == so["last_loss"]
    assert np.array_equal(sg["state"], so["state"])
    qg, tg = h.read_params(); qo, to = st.params()
    assert np.array_equal(qg, qo) and np.array_equal(tg, to)


def _update_steps(c):
    return [g for g in range(c.min_buff_size + 1, c.total_timesteps + 1) if g % c.train_freq == 0]


@pytest.mark.parametrize("name", list(CASES))
def test_run_edges_match_oracle_bit_for_bit(crl, name):
    ocfg = _ocfg(**CASES[name][0])
    T = ocfg.total_timesteps
    params = O.dqn_params(1)
    h, st = _pair(crl, ocfg, params)
    total, n_losses = 0, 0
    for chunk in (1, 7, T):
        tg, eps_g, ls_g = h.run(chunk)
        to, eps_o, ls_o = st.run(chunk)
        total += tg
        assert tg == to and eps_g == eps_o, "same trajectories, same episode records (return, length, step, ϵ)"
        assert ls_g == ls_o, "logged losses bit-exact"
        n_losses += len(ls_g)
        _same_state(h, st, total)
    steps = _update_steps(ocfg)
    assert total == T and h.status()["n_updates"] == len(steps) >= 3
    assert n_losses == len([g for g in steps if g % ocfg.log_frequency == 0]) >= 1
    assert h.status()["rb_size"] == min(T, ocfg.buffer_size)
    assert not np.array_equal(h.read_params()[0], params)
    if name in MULTI_ROUND:      # the shared draw (replay_sample.hpp): ddpg_ref's restatement is the oracle's, and it counts the candidates
        need = []
        for g in steps:
            n = min(g, ocfg.buffer_size)
            assert np.array_equal(O.dqn_sample_indices(SEED, g, n, ocfg.batch_size), DR.sample_indices(SEED, g, n, ocfg.batch_size))
            need.append(DB.candidates_needed(SEED, g, n, ocfg.batch_size))
        assert max(need) > 1024, "at least one draw goes past the first round of 1024 candidates"
    if name == "cap65536":
        idx = np.concatenate([O.dqn_sample_indices(SEED, g, min(g, ocfg.buffer_size), ocfg.batch_size) for g in steps])
        assert idx.max() >= 32768 and steps[-1] > ocfg.buffer_size, "slots in the bitmap's high half were drawn, and the ring was full"
    h.close(); st.close()


def test_loss_records_stop_at_4096_per_call_and_the_count_goes_on(crl):
    ocfg = _ocfg(total_timesteps=4400, batch_size=1, buffer_size=8, min_buff_size=1, train_freq=1)
    h, st = _pair(crl, ocfg, O.dqn_params(1))
    taken, eps, losses = h.run(4300)
    to, eps_o, ls_o = st.run(4300, max_losses=8192)
    assert taken == to == 4300 and eps == eps_o
    assert len(ls_o) == 4299 and len(losses) == DQN_MAX_LOSSES and losses == ls_o[:DQN_MAX_LOSSES], "the first 4096 records; every update counted"
    _same_state(h, st, 4300)
    assert h.status()["n_updates"] == 4299
    taken, eps, losses = h.run(50)
    to, eps_o, ls_o = st.run(50)
    assert taken == to == 50 and eps == eps_o and losses == ls_o and [l[0] for l in losses] == list(range(4301, 4351)), "a fresh list"
    _same_state(h, st, 4350)
    h.close(); st.close()


def test_episode_records_stop_at_8192_per_call(crl):
    ocfg = _ocfg(total_timesteps=16_700, max_steps=1, train_freq=4000, log_frequency=4000)
    h, st = _pair(crl, ocfg, O.dqn_params(1))
    taken, eps, losses = h.run(16_600)
    to, eps_o, ls_o = st.run(16_600, max_eps=16_384)
    assert taken == to == 16_600 and losses == ls_o and len(losses) == 4
    assert len(eps_o) == 8300 and len(eps) == DQN_MAX_EPS and eps == eps_o[:DQN_MAX_EPS], "one-step pairs: 8300 episodes, the first 8192 kept"
    _same_state(h, st, 16_600)
    taken, eps, losses = h.run(60)
    to, eps_o, ls_o = st.run(60)
    assert taken == to == 60 and eps == eps_o and len(eps) == 30 and eps[0][2] == 16_602 and losses == ls_o == []
    _same_state(h, st, 16_660)
    h.close(); st.close()
