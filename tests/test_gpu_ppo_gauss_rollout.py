"""The one-launch rollout of a Gaussian handle at 2x256 (wide_rs_rollout_gauss_kernel, csrc/wide_rs_gauss.hpp) against the Float64 restatement
tests/ppo_gauss_ref.py and against its per-step twin (the same handle with wide_rollout_persist = 0). Bars: those of test_gpu_ppo_gauss.py's
test_rollout_logprob_and_noise_stream (RTOL, profiles/ppo_gauss_bar.json), which the per-step route meets."""
import numpy as np
import pytest

import ppo_gauss_ref as G
from test_gpu_parity import RTOL, crl, rel_err  # noqa: F401  (crl is the module fixture)
from test_gpu_ppo_gauss import BAR, LO, HI, make, spread_params
from test_gpu_wide import rel_err_s

pytestmark = pytest.mark.gpu

CASES = [(1, 3, "pendulum"), (1, 8, "synthetic"), (2, 12, "synthetic"), (3, 8, "synthetic"), (4, 16, "synthetic")]     # act_dim, obs_dim, env
SEED, K = 0x5EED, 16


def pair(crl, nt, k, D, ad, kind, Hd=256, **kw):
    """the default handle and its per-step twin on the same parameters and seed"""
    p = spread_params(crl, D, ad, Hd, 7)
    env = crl._lib.ENV_PENDULUM if kind == "pendulum" else None
    return p, [make(crl, nt, k, D, ad, Hd, params=p, env_kind=env, seed=SEED, **o, **kw) for o in ({}, {"options": {"wide_rollout_persist": 0}})]


@pytest.mark.parametrize("ad,D,kind", CASES)
@pytest.mark.parametrize("nt", [64, 192])
def test_route(crl, nt, ad, D, kind):
    _, (a, t) = pair(crl, nt, K, D, ad, kind)
    assert a.handle.rollout_route() == "rs_actor" and t.handle.rollout_route() == "stepwise"
    a.close(); t.close()


def test_route_falls_back_and_reports_discrete_handles(crl):
    for nt, D, ad, Hd in ((64, 8, 5, 256), (96, 8, 3, 256), (64, 8, 3, 128)):     # head 10 > 8, a ragged env count, another hidden size
        a = make(crl, nt, K, D, ad, Hd)
        assert a.handle.rollout_route() == "stepwise", (nt, D, ad, Hd)
        a.close()
    d = crl.Agent(crl.PPOConfig(num_envs=128, num_steps=K), obs_dim=8, n_act=4, hidden=256, env_kind=crl._lib.ENV_SYNTHETIC)
    assert d.handle.rollout_route() == "rs_actor"
    d.close()


@pytest.mark.parametrize("ad,D,kind", CASES)
@pytest.mark.parametrize("nt", [64, 192])
def test_rollout_matches_restatement(crl, nt, ad, D, kind):
    F = crl._lib
    p, (a, t) = pair(crl, nt, K, D, ad, kind)
    t.close()
    h = a.handle
    assert h.rollout_route() == "rs_actor"
    h.env_reset(); h.rollout_run()
    obs, act, lp, val = [h.read(f) for f in (F.F_OBS, F.FIELD_ACTION_F, F.F_LOGPROB, F.F_VALUE)]
    a.close()
    actor, critic = G.unpack(p, D, ad, 256)
    X = obs.reshape(D, -1, order="F").astype(np.float64)
    z = G.mlp(actor, X)[0]
    lp_o, _, xi_rec, _ = G.logprob_entropy(z, act.reshape(ad, -1, order="F").astype(np.float64), ad, LO, HI)
    e_lp, e_v = rel_err_s(lp.reshape(-1, order="F"), lp_o), rel_err(val.reshape(-1, order="F"), G.mlp(critic, X)[0][0])
    xi_pin = np.concatenate([G.rollout_xi(SEED, np.arange(nt), g, ad) for g in range(K)], axis=1)
    e_xi = np.max(np.abs(xi_rec - xi_pin))
    print(f"logprob {e_lp:.3e}, value {e_v:.3e} (bar {RTOL:.0e}); recovered xi {e_xi:.3e} (bar {BAR['xi_bar']:.3e})")
    assert e_lp < RTOL and e_v < RTOL and e_xi < BAR["xi_bar"]


@pytest.mark.parametrize("ad,D,kind", [c for c in CASES if c[2] == "synthetic"])
@pytest.mark.parametrize("nt", [64, 192])
def test_two_launches_equal_the_per_step_twin(crl, nt, ad, D, kind):
    """The synthetic env's draws do not depend on the action: everything but actions, log-probabilities and values is the twin's bit for bit, after the
    first launch and after the second, which continues from what the first wrote back."""
    F = crl._lib
    _, (a, t) = pair(crl, nt, K, D, ad, kind)
    a.handle.env_reset(); t.handle.env_reset()
    dones = 0
    for _ in range(2):
        a.handle.rollout_run(); t.handle.rollout_run()
        for f in (F.F_OBS, F.F_REWARD, F.F_TERMINAL, F.F_NEXT_DONE, F.F_CUR_OBS):
            assert np.array_equal(a.handle.read(f), t.handle.read(f)), f
        assert a.handle.episode_stats() == t.handle.episode_stats()
        assert rel_err_s(a.handle.read(F.FIELD_ACTION_F), t.handle.read(F.FIELD_ACTION_F)) < RTOL
        dones += int(t.handle.read(F.F_TERMINAL).sum())
    assert dones >= 1, "the twin saw no episode end: pick another seed"
    a.close(); t.close()


def test_pendulum_over_an_episode_boundary(crl):
    """64 envs x 256 steps: every Pendulum episode ends after 200 steps inside the launch; stale_obs = False, so the observation stored at the step
    after is the fresh reset state, which does not depend on the policy."""
    F = crl._lib
    _, (a, t) = pair(crl, 64, 256, 3, 1, "pendulum", stale_obs=False)
    for x in (a, t):
        x.handle.env_reset(); x.handle.rollout_run()
    term = t.handle.read(F.F_TERMINAL)
    s = int(np.argmax(term[0]))
    assert term.sum() == 64 and (term[:, s] == 1).all()
    assert np.array_equal(a.handle.read(F.F_TERMINAL), term)
    assert np.array_equal(a.handle.read(F.F_OBS)[:, :, s], t.handle.read(F.F_OBS)[:, :, s])
    ea, et = a.handle.episode_stats(), t.handle.episode_stats()
    assert et["episodes"] == 64 and ea["episodes"] == et["episodes"] and ea["length_sum"] == et["length_sum"]
    assert abs(ea["return_sum"] - et["return_sum"]) < 1e-4 * max(1, abs(et["return_sum"]))
    a.close(); t.close()
