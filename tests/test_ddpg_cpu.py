"""Pins the DDPG yardstick (tests/ddpg_ref.py) itself, without a GPU: its Philox and sampling against the C oracle, its hand-written gradients
against torch float64 autograd, its Pendulum at known points — and the host-side surface of the crl_ddpg_* block (config defaults and field
order in header / ctypes / Julia, make_ddpg_nn)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ddpg_ref as R
import oraclelib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def crl():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "cleanrl.jl_amd", "libcleanrl_hip.so")):
        g.build()
    import cleanrl_jl_amd as crl
    return crl


def test_philox_equals_the_oracle():
    rng = np.random.default_rng(0)
    words = rng.integers(0, 2 ** 32, (1000, 6), dtype=np.uint64)
    out = (C.c_uint32 * 4)()
    for w in words:
        O.lib().orc_philox(*[int(x) for x in w], out)
        got = [int(v[0]) for v in R.philox(np.array([w[0]]), int(w[1]), int(w[2]), int(w[3]), int(w[4]), int(w[5]))]
        assert got == list(out)


@pytest.mark.parametrize("n,k", [(1, 1), (7, 7), (150, 32), (100000, 120), (200, 200), (1024, 1024)])
def test_sampling_equals_the_oracle(n, k):
    for seed, gstep in ((0, 1), (0x5EED, 2501), (2 ** 40 + 3, 2 ** 33 + 5)):
        idx = R.sample_indices(seed, gstep, n, k)
        assert np.array_equal(idx, O.dqn_sample_indices(seed, gstep, n, k))
        assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < n


def _torch_losses(actor, critic, actor_t, critic_t, D, A, batch, gamma, noise_t, noise_a):
    """The closures of ddpg.jl:108-124 in torch float64 (exact tanh: tanh_fast differs from it by < 1e-12 relative in value and in slope — compared
    at 1e-9, so the reference's activations are fed in through a custom function instead)."""
    import torch

    class TanhFast(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            y = torch.from_numpy(R.tanh_fast64(x.detach().numpy()))
            ctx.save_for_backward(y)
            return y

        @staticmethod
        def backward(ctx, g):
            (y,) = ctx.saved_tensors
            return g * (1 - y * y)

    def net(p, n_in, n_out, req):
        return [torch.tensor(a, dtype=torch.float64, requires_grad=req) for a in R.split(p, n_in, n_out)]

    def actor_f(P, X, noise):
        h = TanhFast.apply(P[0] @ X + P[1][:, None]); h = TanhFast.apply(P[2] @ h + P[3][:, None])
        return TanhFast.apply(P[4] @ h + P[5][:, None]) * 2 + torch.tensor(noise)[:, None]

    def critic_f(P, X, Act):
        h = torch.relu(P[0] @ torch.cat([X, Act]) + P[1][:, None]); h = torch.relu(P[2] @ h + P[3][:, None])
        return (P[4] @ h + P[5][:, None])[0]

    t = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in batch.items()}
    with torch.no_grad():
        td = t["reward"] + gamma * critic_f(net(critic_t, D + A, 1, False), t["next_state"], actor_f(net(actor_t, D, A, False), t["next_state"], noise_t)) \
            * (1.0 - t["terminal"])
    Pc = net(critic, D + A, 1, True)
    lc = torch.mean((td - critic_f(Pc, t["state"], t["action"])) ** 2)
    lc.backward()
    Pa = net(actor, D, A, True); Pc2 = net(critic, D + A, 1, False)
    la = -torch.mean(critic_f(Pc2, t["state"], actor_f(Pa, t["state"], noise_a)))
    la.backward()
    return td.numpy(), lc.item(), [p.grad.numpy() for p in Pc], la.item(), [p.grad.numpy() for p in Pa]


@pytest.mark.parametrize("D,A,k", [(3, 1, 7), (17, 6, 5), (1, 1, 2), (49, 16, 3), (64, 16, 4)])
@pytest.mark.parametrize("noise_in_update", [0, 1])
def test_hand_written_gradients_match_float64_autograd(D, A, k, noise_in_update):
    rng = np.random.default_rng(D * 100 + k + noise_in_update)
    na, nc = R.param_count(D, A)
    nets = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in (na, nc, na, nc)]
    actor, critic, actor_t, critic_t = nets
    t1 = min(2, k - 1)
    term = np.zeros(k, np.uint8); term[t1] = 1
    batch = dict(state=rng.standard_normal((D, k)), action=rng.uniform(-2, 2, (A, k)), reward=rng.standard_normal(k),
                 next_state=rng.standard_normal((D, k)), terminal=term)
    on = float(noise_in_update)
    noise_t = R.normal(9, np.arange(A), 41, R.S_TARGET) * 0.1 * on; noise_a = R.normal(9, np.arange(A), 41, R.S_ACTOR) * 0.1 * on
    td = R.td_target(actor_t, critic_t, D, A, batch, 0.99, noise_t)
    lc, gc = R.critic_loss_grad(critic, D, A, batch, td)
    la, ga = R.actor_loss_grad(actor, critic, D, A, batch, noise_a)
    ttd, tlc, tgc, tla, tga = _torch_losses(actor, critic, actor_t, critic_t, D, A, batch, 0.99, noise_t, noise_a)
    assert np.allclose(td, ttd, rtol=1e-12, atol=1e-12)
    assert td[t1] == batch["reward"][t1]                     # terminal = 1: no bootstrap
    assert abs(lc - tlc) <= 1e-9 * abs(tlc) and abs(la - tla) <= 1e-9 * abs(tla)
    for mine, sizes, theirs in ((gc, R.net_sizes(D + A, 1), tgc), (ga, R.net_sizes(D, A), tga)):
        o = 0
        for n, t in zip(sizes, theirs):
            a, b = mine[o:o + n], t.reshape(-1, order="F"); o += n
            assert np.abs(b).max() > 0
            assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max()


def test_adam_and_polyak_keep_float32_state():
    opt = R.Adam(6, [1] * 6, 1e-3)
    p = np.ones(6, np.float32)
    p1 = opt.step(p, np.full(6, 0.5))
    # first Adam step moves by lr·g/(|g| + ε·…) ≈ lr
    assert p1.dtype == np.float32 and np.abs((p - p1).astype(np.float64) - 1e-3).max() < 1e-7
    assert np.allclose(opt.bp, [[0.81, 0.998001]] * 6)
    t = R.polyak(np.zeros(3, np.float32), np.ones(3, np.float32), 0.005)
    assert t.dtype == np.float32 and np.array_equal(t, np.full(3, np.float32(0.005)))


def test_pendulum_known_points():
    th, thd, t, r, term = R.pendulum_step(0.0, 0.0, 0, 0.0)
    assert (th, thd, t, term) == (0.0, 0.0, 1, False) and r == 0.0          # −0.0 == 0
    # torque clamp at ±2
    for a in (2.0, 5.0, 1e9):
        assert R.pendulum_step(0.3, 0.1, 0, a) == R.pendulum_step(0.3, 0.1, 0, 2.0)
        assert R.pendulum_step(0.3, 0.1, 0, -a) == R.pendulum_step(0.3, 0.1, 0, -2.0)
    assert R.pendulum_step(0.3, 0.1, 0, 1.9) != R.pendulum_step(0.3, 0.1, 0, 2.0)
    # speed clamp at ±8
    assert R.pendulum_step(1.5, 7.9, 0, 2.0)[1] == 8.0 and R.pendulum_step(-1.5, -7.9, 0, -2.0)[1] == -8.0
    # wrap across ±π: one conditional ±2π
    th, thd, *_ = R.pendulum_step(3.1, 4.0, 0, 0.0)
    assert -R.PI <= th < -2.9 and th == (3.1 + thd * 0.05) - 2.0 * R.PI
    th, thd, *_ = R.pendulum_step(-3.1, -4.0, 0, 0.0)
    assert 2.9 < th <= R.PI and th == (-3.1 + thd * 0.05) + 2.0 * R.PI
    # reward = −(θ² + 0.1·θ̇² + 0.001·u²) of the state before the step
    assert R.pendulum_step(1.0, 2.0, 0, 1.0)[3] == -(1.0 + 0.1 * 4.0 + 0.001 * 1.0)
    # terminal exactly at t = max_steps
    assert [R.pendulum_step(0.1, 0.0, t, 0.0, 200)[4] for t in (197, 198, 199, 200)] == [False, False, True, True]
    assert [R.pendulum_step(0.1, 0.0, t, 0.0, 3)[4] for t in (0, 1, 2)] == [False, False, True]
    th, thd = R.pendulum_reset(5, 17, R.S_RESET)
    assert -R.PI <= th < R.PI and -1.0 <= thd < 1.0
    assert np.array_equal(R.pendulum_obs(0.0, 0.5), [1.0, 0.0, 0.5])


# worst |plain-op polynomial − libm| measured on the grid below: 1.082e-15 (sin), 8.882e-16 (cos) — pinned at twice that
SIN_BOUND, COS_BOUND = 2 * 1.082e-15, 2 * 8.882e-16


def test_plain_op_sin_cos_on_minus_pi_pi():
    xs = np.concatenate([np.linspace(-np.pi, np.pi, 20001), [-R.PI, R.PI, 0.0, 1e-9, -1e-9]])
    es = max(abs(R.pend_sin(x) - math.sin(x)) for x in xs)
    ec = max(abs(R.pend_cos(x) - math.cos(x)) for x in xs)
    print(f"worst error: sin {es:.3e} cos {ec:.3e}")
    assert es <= SIN_BOUND and ec <= COS_BOUND
    assert R.pend_sin(0.0) == 0.0 and R.pend_cos(0.0) == 1.0


def test_ddpg_config_defaults_are_the_references(crl):
    c = crl.DDPGConfig()
    assert (c.total_timesteps, c.buffer_size, c.min_buff_size, c.batch_size, c.warmup_steps, c.log_frequencey) == (5_000_000, 100_000, 200, 120, 2500, 1000)
    assert (c.lr, c.tau, c.gamma, c.exploration_noise) == (0.0001, 0.005, 0.99, 0.1)
    from cleanrl_jl_amd.config_parser import argparse_struct
    d = argparse_struct(crl.DDPGConfig(), ["--log_frequencey", "50", "--tau", "0.01"])
    assert isinstance(d, crl.DDPGConfig) and d.log_frequencey == 50 and d.tau == 0.01


def test_ddpg_config_mirrors_follow_the_header(crl):
    L = crl._lib
    hdr = open(os.path.join(ROOT, "include", "cleanrl_hip.h")).read()
    body = hdr[hdr.index("typedef struct crl_ddpg_config {"):hdr.index("} crl_ddpg_config;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"(?:int64_t|int32_t|double|uint64_t)\s+([a-z_, ]+);", body):
        names += [n.strip() for n in decl.split(",")]
    want = [n for n, _ in L.CrlDDPGConfig._fields_]
    assert names == want and C.sizeof(L.CrlDDPGConfig) == 128
    jl = open(os.path.join(ROOT, "julia", "CleanRLHip.jl")).read()
    for jname, mirror in (("CrlDDPGConfig", L.CrlDDPGConfig), ("CrlDDPGEpisode", L.CrlDDPGEpisode), ("CrlDDPGLossRecord", L.CrlDDPGLossRecord),
                          ("CrlDDPGStatus", L.CrlDDPGStatus)):
        m = re.search(r"struct %s\b(.*?)\bend" % jname, jl, re.S)
        assert m, jname
        assert re.findall(r"([A-Za-z_][A-Za-z_0-9]*)::", re.sub(r"#.*", "", m.group(1))) == [n for n, _ in mirror._fields_], jname
    called = set(re.findall(r"ccall\(\(:(crl_ddpg_[a-z_0-9]+),", jl))
    assert {"crl_ddpg_create", "crl_ddpg_run", "crl_ddpg_act", "crl_ddpg_observe", "crl_ddpg_init_params", "crl_ddpg_write_params"} <= called
    assert called <= set(L.EXPORTS)
    for fn in ("function ddpg(config;", "function ddpg_external(config, env;"):
        src = jl[jl.index(fn):jl.index("\nend\n", jl.index(fn))]
        assert "_ddpg_start!(" in src and 'make_logger("ddpg|$(config.run_name)")' in src
    start = jl[jl.index("function _ddpg_start!("):]
    start = start[:start.index("\nend\n")]
    assert ":crl_ddpg_init_params" in start and ":crl_ddpg_write_params" in start and "init()" in start      # params, else the package's, else the library's


@pytest.mark.parametrize("D,A", [(3, 1), (17, 6), (64, 16)])
def test_make_ddpg_nn_is_glorot_with_zero_biases(crl, D, A):
    na, nc = crl._lib.ddpg_param_count(D, A)
    assert (na, nc) == R.param_count(D, A)
    for actor, critic in (crl.make_ddpg_nn(D, A, seed=1), crl._lib.ddpg_make_nn_host(D, A, seed=1)):
        assert actor.dtype == np.float32 and (actor.size, critic.size) == (na, nc)
        for p, n_in, n_out in ((actor, D, A), (critic, D + A, 1)):
            W1, b1, W2, b2, W3, b3 = R.split(p, n_in, n_out)
            for W in (W1, W2, W3):
                lim = math.sqrt(6.0 / sum(W.shape))
                assert np.abs(W).max() <= lim * (1 + 1e-6)
                if W.size >= 64:
                    assert np.abs(W).max() > 0.8 * lim and abs(W.mean()) < 0.2 * lim
            assert not b1.any() and not b2.any() and not b3.any()
    with pytest.raises(crl.CrlError, match="obs_dim"):
        crl._lib.ddpg_param_count(65, 1)
    with pytest.raises(crl.CrlError, match="act_dim"):
        crl._lib.ddpg_param_count(3, 17)
