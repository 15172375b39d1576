"""The fused 4/2/64 update pass (update_x2_kernel, update_x3_kernel, update_t16_kernel → reduce_kernel / reduce_optim_kernel, the exact value-loss
pass) across its block split and its scheduling options: actor_block_pct, update_xcd_align, update_stagger, update_prio_small. The launch
geometries are the table of tests/update_geometry.py (tests/test_update_geometry_cpu.py shows which edge each one is there for); the reference is
orc_loss_grad, which knows nothing of blocks, waves or tiles; the bars are those of tests/test_gpu_parity.py, unchanged.

  a. every case and flavour against the oracle: four losses, twelve gradient arrays, the advantage statistics;
  b. the exact value-loss pass (u > 0 live) behind an uneven main pass — it overwrites update_blocks critic partials where the main pass wrote nC;
  c. update_stagger and update_prio_small are timing only: gradients and losses keep their bits, also where the feedback rule runs by itself;
  d. a census no summation order can blur: with v = 0 and integer returns the critic's head-bias gradient is an exact Float32 in every partial sum;
  e. the one-launch optimiser step under uneven splits: the same gradient bits as the two-launch step, ClipNorm + Adam bit for bit on both.

With CRL_WRITE_PROFILES=1 every measured distance goes to profiles/update_geometry.json."""
import json
import os

import numpy as np
import pytest

import optimlib
import oraclelib as O
import update_geometry as G
from test_gpu_parity import LOSS_FLOOR, RTOL, _grad_close, _inject_batch, loss_close, make_agent

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITE = os.environ.get("CRL_WRITE_PROFILES") == "1"
FLAVOURS = {"gemm=2": {"gemm": 2}, "gemm=1": {"gemm": 1}, "update_tile=16": {"gemm": 2, "update_tile": 16}}
LOSS_KEYS = ("loss", "pg_loss", "v_loss", "entropy_loss")
C2 = (128, 128, 4)   # M = 4096: the shape of the tests that need one size only
MEASURED = {}


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1, "HIP library loaded but no GPU visible"
    return crl


class Batch:
    """One synthetic rollout buffer (perturbed orthogonal parameters, a random permutation: _inject_batch) in an oracle state and in one handle per
    flavour; the oracle's gradient of a minibatch is computed once and shared by every geometry and flavour."""

    def __init__(self, crl, shape, seed, ret_scale=10.0, clipv=True, edit_params=None, edit_state=None):
        self.crl, self.shape, self.clipv = crl, shape, clipv
        nt, k, nmb = shape
        self.M = G.minibatch_size(shape)
        rng = np.random.default_rng(seed)
        self.cfgo = O.make_config(num_envs=nt, num_steps=k, num_minibatches=nmb, clip_value_loss=clipv)
        self.off = O.param_offsets(self.cfgo)
        self.params = O.orthogonal_params(self.cfgo, 5) + (0.05 * rng.standard_normal(O.lib().orc_param_count(self.cfgo))).astype(np.float32)
        if edit_params:
            edit_params(self.params, self.off)
        self.st = O.State(self.cfgo); self.st.params[:] = self.params
        self.agents, self._oracle = {}, {}
        first = self._create(next(iter(FLAVOURS)))
        _inject_batch(crl, first, self.st, rng, ret_scale)
        if edit_state:
            edit_state(self.st, rng)
        self._load(first)

    def _create(self, flavour, **options):
        nt, k, nmb = self.shape
        agent = make_agent(self.crl, nt=nt, k=k, params=self.params, num_minibatches=nmb, clip_value_loss=self.clipv, options={**FLAVOURS[flavour], **options})
        self.agents[(flavour, tuple(sorted(options.items())))] = agent
        return agent

    def _load(self, agent):
        st, F, h = self.st, self.crl._lib, agent.handle
        for f, a in ((F.F_OBS, st.obs), (F.F_ACTION, st.action), (F.F_LOGPROB, st.logprob), (F.F_VALUE, st.value),
                     (F.F_ADVANTAGE, st.adv), (F.F_RETURN, st.ret), (F.F_PERM, st.perm)):
            h.write(f, a)
        h.adv_stats()

    def handle(self, flavour, **options):
        key = (flavour, tuple(sorted(options.items())))
        if key not in self.agents:
            self._load(self._create(flavour, **options))
        return self.agents[key].handle

    def oracle(self, mb):
        if mb not in self._oracle:
            st, M = self.st, self.M
            self._oracle[mb] = O.loss_grad(self.cfgo, self.params, st.obs.reshape(4, -1, order="F"), st.action, st.logprob, st.value, st.adv, st.ret,
                                           st.perm[mb * M:(mb + 1) * M])
        return self._oracle[mb]

    def close(self):
        for a in self.agents.values():
            a.close()
        self.st.close()


def _zero_critic(params, off):
    params[off[6]:off[12]] = 0.0


def _zero_critic_head(params, off):
    params[off[10]:off[12]] = 0.0


def _integer_returns(st, rng):
    st.ret[:] = rng.integers(1, 9, st.ret.shape).astype(np.float32)


def _live_u(params, off):
    params[off[11]] = 0.3   # with ret_scale = 0.05: u = mean(v − R²) > 0 (test_update_gradient_matches_oracle's recipe)


RECIPES = {
    "geometry": lambda crl, shape: Batch(crl, shape, seed=sum(shape)),
    "exact": lambda crl, shape: Batch(crl, shape, seed=1, ret_scale=0.05, edit_params=_live_u),
    "census, critic zero": lambda crl, shape: Batch(crl, shape, seed=7, clipv=False, edit_params=_zero_critic, edit_state=_integer_returns),
    "census, critic head zero": lambda crl, shape: Batch(crl, shape, seed=7, clipv=False, edit_params=_zero_critic_head, edit_state=_integer_returns),
    # seed and return scale chosen on the CPU (orc_loss_grad of minibatch 3): array norms 1.17, 0.07, 1.09, 0.05, 1.41, 0.02 in the critic — three arrays
    # clipped, three not — and 0.004 … 0.11 in the actor; test (e) asserts the distance from optimlib.BAND
    "optimiser": lambda crl, shape: Batch(crl, shape, seed=4, ret_scale=30.0, clipv=False),
}


@pytest.fixture(scope="module")
def batches(crl):
    made = {}

    def get(recipe, shape):
        if (recipe, shape) not in made:
            made[(recipe, shape)] = RECIPES[recipe](crl, shape)
        return made[(recipe, shape)]
    yield get
    for b in made.values():
        b.close()
    if WRITE:
        path = os.path.join(ROOT, "profiles", "update_geometry.json")
        json.dump(MEASURED, open(path, "w"), indent=1, sort_keys=True)


def set_geometry(h, case):
    h.set_option("actor_block_pct", case.pct)
    h.set_option("update_xcd_align", case.align)


def distances(gs, g, so, g_o, off):
    """Each figure as a fraction of its bar in tests/test_gpu_parity.py (loss_close at RTOL, _grad_close at RTOL): below 1 passes."""
    d = {key: abs(gs[key] - so[key]) / (RTOL * abs(so[key]) + (LOSS_FLOOR if key in ("loss", "pg_loss") else 0.0)) for key in LOSS_KEYS}
    for i in range(12):
        a, b = g[off[i]:off[i + 1]].astype(np.float64), g_o[off[i]:off[i + 1]].astype(np.float64)
        d[f"grad{i}"] = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12)) / RTOL
    d["adv_mean"] = abs(gs["adv_mean"] - so["adv_mean"]) / 1e-6
    d["adv_std"] = abs(gs["adv_std"] - so["adv_std"]) / (1e-5 * so["adv_std"])
    return d


def compare_with_oracle(b, h, mb, where, record):
    """One minibatch through the handle against the oracle, under the project's bars; prints and records the worst distance first."""
    F = b.crl._lib
    gs = h.update_minibatch(mb, 0.0, apply_update=False)
    g = h.read(F.F_GRADS)
    g_o, so = b.oracle(mb)
    d = distances(gs, g, so, g_o, b.off)
    worst, losses, grad = max(d, key=d.get), max(d[k] for k in LOSS_KEYS), max(d[f"grad{i}"] for i in range(12))
    print(f"{where} mb {mb}: worst {worst} at {d[worst]:.3f} of its bar; losses {losses:.3f}, gradient {grad:.3f}")
    record[f"mb{mb}"] = {"worst": worst, "worst_fraction_of_bar": round(d[worst], 4), "losses": round(losses, 4), "gradient": round(grad, 4),
                         "adv_stats": round(max(d["adv_mean"], d["adv_std"]), 4)}
    for key in LOSS_KEYS:
        assert loss_close(key, gs[key], so[key], RTOL), (where, mb, key, gs[key], so[key])
    assert abs(gs["adv_mean"] - so["adv_mean"]) < 1e-6 and abs(gs["adv_std"] - so["adv_std"]) < 1e-5 * so["adv_std"], (where, mb)
    _grad_close(g, g_o, b.off)
    return gs, so


# ---- a ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_every_geometry_matches_the_oracle(batches, case, flavour):
    """Minibatches 0 and 3 of every case of the table, on the fp16x2 kernel, the bf16x3 kernel and the 16-sample-tile kernel."""
    b = batches("geometry", case.shape)
    h = b.handle(flavour)
    set_geometry(h, case)
    rec = MEASURED.setdefault("geometry", {}).setdefault(flavour, {}).setdefault(case.id, {"blocks": list(case.blocks), "edges": sorted(case.edges)})
    for mb in (0, 3):
        compare_with_oracle(b, h, mb, f"{flavour} {case.id}", rec)


# ---- b ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("blocks,aligned", [((1, 31), False), ((31, 1), False), ((8, 24), True)])
def test_exact_value_pass_behind_an_uneven_main_pass(batches, blocks, aligned, flavour):
    """u = mean(v − R²) > 0: the speculative pass is redone by update_vfix_kernel on update_blocks = 32 critic blocks, over partials of which the
    main pass wrote 31, 1 or 24; reduce_kernel<1> then sums 32. The unclipped term wins somewhere, as often as the oracle says, and the result
    meets the bars of (a)."""
    b = batches("exact", C2)
    case = G.case_with_blocks(C2, *blocks, aligned)
    assert case.ub == 32
    h = b.handle(flavour)
    set_geometry(h, case)
    rec = MEASURED.setdefault("exact", {}).setdefault(flavour, {}).setdefault(case.id, {"blocks": list(case.blocks)})
    for mb in (0, 3):
        gs, so = compare_with_oracle(b, h, mb, f"exact pass, {flavour} {case.id}", rec)
        assert so["n_unclipped_wins"] > 0 and gs["n_unclipped_wins"] == so["n_unclipped_wins"], (gs["n_unclipped_wins"], so["n_unclipped_wins"])


# ---- c ---------------------------------------------------------------------------------------------------------------------------------
STAGGER_DEFAULT, PRIO_DEFAULT = 3, 0
SCHEDULES = {"gemm=2": [{"update_stagger": 0}, {"update_stagger": 64}, {"update_prio_small": 1}, {"update_prio_small": 2}, {"update_prio_small": 3},
                        {"update_stagger": 64, "update_prio_small": 1}],
             "gemm=1": [{"update_stagger": 0}, {"update_stagger": 64}]}   # the priority rules are fp16x2 code


@pytest.mark.parametrize("flavour", list(SCHEDULES))
@pytest.mark.parametrize("blocks,aligned", [((16, 16), True), ((1, 31), False), ((31, 1), False), ((8, 24), True), ((24, 8), True)])
def test_scheduling_options_keep_the_bits(batches, blocks, aligned, flavour):
    """update.hip calls the start delay and the three priority rules "timing only … the gradients keep their bits". Under (1, 31) and (31, 1) the
    feedback rule — eight progress counters in LDS where the staging flag was — runs by itself in the one-block role (16 tiles per wave) and, under
    update_prio_small = 1, in the other as well; under (16, 16) it runs only when asked. After one launch that settles the fp16x2 weight-gradient
    scale, every setting gives the gradient and the four losses of the defaults, bit for bit.
    (8, 24) and (24, 8): at an even split update_blocks gives every wave exactly one tile, and so does the larger role of an uneven one — a counter
    that lands in a wave's accumulator strip then overwrites a sum that is still zero and nothing shows. The 8-block role has two tiles per wave and
    the rule runs there only when asked, so its defaults are a clean baseline (tried: the counters moved 136 floats down, into the last wave's dW3
    strip, pass every (16, 16) case and fail here and under (1, 31))."""
    b = batches("geometry", C2)
    case = G.case_with_blocks(C2, *blocks, aligned)
    if not aligned:
        assert G.balance(b.M, 1, False) and not G.balance(b.M, 31, False) and G.small_prio(b.M, 31, False, 2) == 2 and G.small_prio(b.M, 1, False, 2) == 0
    tiles_per_wave = [max(len(t) for t in G.role_walk(n, b.M, aligned).values()) for n in blocks]
    assert tiles_per_wave == {(16, 16): [1, 1], (1, 31): [16, 1], (31, 1): [1, 16], (8, 24): [2, 1], (24, 8): [1, 2]}[blocks]
    h = b.handle(flavour); F = b.crl._lib
    set_geometry(h, case)
    assert (h.get_option("update_stagger"), h.get_option("update_prio_small")) == (STAGGER_DEFAULT, PRIO_DEFAULT)
    mb = 1

    def launch():
        gs = h.update_minibatch(mb, 0.0, apply_update=False)
        return h.read(F.F_GRADS), [gs[key] for key in LOSS_KEYS]
    try:
        launch()
        g0, l0 = launch()
        assert np.isfinite(g0).all() and np.linalg.norm(g0) > 0
        for sched in SCHEDULES[flavour]:
            for key, value in sched.items():
                h.set_option(key, value)
            g, l = launch()
            assert np.array_equal(g, g0), f"{flavour} {case.id} {sched}: {np.sum(g != g0)} gradient entries changed, first at {int(np.flatnonzero(g != g0)[0])}"
            assert l == l0, (flavour, case.id, sched, l, l0)
            h.set_option("update_stagger", STAGGER_DEFAULT); h.set_option("update_prio_small", PRIO_DEFAULT)
        g, l = launch()
        assert np.array_equal(g, g0) and l == l0, "back at the defaults"
    finally:
        h.set_option("update_stagger", STAGGER_DEFAULT); h.set_option("update_prio_small", PRIO_DEFAULT)


# ---- d ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("critic", ["critic zero", "critic head zero"])
def test_census_of_samples_is_exact_in_every_geometry(batches, critic, flavour):
    """clip_value_loss = False, v_coef = 0.5, M = 4096, v = 0 on every sample, returns integers 1 … 8: each term of the critic's head-bias
    gradient is −R / (2M), a multiple of 2^-13 below 2^-10, and every partial sum of them — per lane, wave, block, reduce group — is a multiple
    of 2^-13 of at most 4: exact in Float32 whatever the order. So the one number is the closed form −ΣR / (2M), bit for bit, in every geometry
    of the table; a dropped or doubled sample moves it by at least 2^-13, which is 2^10 ulp of a result near 2.
    `critic zero` is the all-zero critic: its hidden weights sit below the fp16 window, so the fp16x2 kernels hand that role to their bf16x3
    fallback (update_x2_kernel in the same launch, update_t16_kernel through update_repair_kernel). `critic head zero` zeroes only W3 and b3: v is
    still exactly 0 and the fp16x2 critic code itself walks the tiles (δ2 = 0 there, the weight-gradient product takes its own fallback).
    fp16x2: the head cotangent enters the db3 sum unscaled (the scale G goes on a copy: `dout[i] * Gdw` in phase 3 of update_role), so no
    flavour needs a looser statement than bit equality.
    The actor's entropy sum rides in the same launches: positive Float64 terms, so two geometries agree to 1e-12 relative before the sum is
    rounded once to Float32 for the statistics record (in practice: the same Float32), while one sample more or less moves it by 1 / M."""
    b = batches(f"census, {critic}", C2)
    assert b.M == 4096 and b.cfgo.v_coef == 0.5
    h = b.handle(flavour); F = b.crl._lib
    ret = b.st.ret.ravel(order="F").astype(np.float64)
    assert np.array_equal(ret, np.round(ret)) and ret.min() == 1 and ret.max() == 8
    rec = MEASURED.setdefault("census", {}).setdefault(critic, {}).setdefault(flavour, {})
    for mb in (0, 3):
        R = ret[b.st.perm[mb * b.M:(mb + 1) * b.M]]
        want = np.float32(-R.sum() / (2.0 * b.M))
        assert float(want) == -R.sum() / (2.0 * b.M), "the closed form is itself an exact Float32"
        assert b.oracle(mb)[0][b.off[11]] == want, "and the oracle agrees with it"
        ent = {}
        for case in (c for c in G.CASES if c.shape == C2):
            set_geometry(h, case)
            gs = h.update_minibatch(mb, 0.0, apply_update=False)
            got = h.read(F.F_GRADS)[b.off[11]]
            ulps = abs(int(np.float32(got).view(np.int32)) - int(want.view(np.int32)))
            print(f"census {critic} {flavour} {case.id} mb {mb}: db3 {got!r} want {want!r} ({ulps} ulp), entropy {gs['entropy_loss']!r}")
            rec[f"{case.id}/mb{mb}"] = {"db3_ulps": ulps, "entropy_loss": gs["entropy_loss"]}
            assert got == want, f"{flavour} {case.id} mb {mb}: critic head-bias gradient {got!r}, closed form {want!r}: {ulps} ulp = {(float(got) - float(want)) * 2 * b.M:+.3f} returns"
            ent[case.id] = gs["entropy_loss"]
        e0 = next(iter(ent.values()))
        assert e0 > 0.1
        for cid, e in ent.items():
            assert abs(e - e0) <= 1e-12 * e0, f"{flavour} mb {mb}: entropy sum {e!r} under {cid}, {e0!r} under {next(iter(ent))}: {(e - e0) / e0 * b.M:+.3e} samples"
        assert abs(e0 - b.oracle(mb)[1]["entropy_loss"]) <= RTOL * e0
    # which critic code walked the tiles: the bf16x3 fallback for the all-zero critic of the fp16x2 flavours, the flavour's own otherwise
    assert h.get_option("gemm_fallback_seen") == int(critic == "critic zero" and flavour != "gemm=1")


# ---- e ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks,aligned", [((1, 31), False), ((24, 8), True), ((16, 16), True)])
def test_one_launch_optimiser_step_under_uneven_splits(batches, blocks, aligned):
    """reduce_optim_kernel reads nA and nC partials per role like reduce_kernel does: the gradient message of the one-launch step (fuse_optim = 1) and
    of the two-launch step (fuse_optim = 0) is the same bits, and on each handle orc_clipnorm_adam applied to the handle's own gradient gives its
    parameters and Adam state bit for bit. Three critic arrays are clipped, nine arrays are not, every norm far outside optimlib.BAND (asserted
    on the oracle's gradient: the handles' differ from it by ~1e-5)."""
    b = batches("optimiser", C2)
    case = G.case_with_blocks(C2, *blocks, aligned)
    F = b.crl._lib
    mb, eta = 3, 2.5e-4
    route = optimlib.Route("update geometry", 4, 2, 64, False)
    route.nt, route.k, route.nmb = C2
    route.M = b.M
    g_o, _ = b.oracle(mb)
    flags = optimlib.check_step_inputs(route, g_o, 0, "update geometry, oracle gradient")
    assert any(flags) and not all(flags), "the step must clip some arrays and leave others"
    grads = {}
    for fuse in (1, 0):
        # a handle per case and route: the step changes the parameters
        agent = make_agent(b.crl, nt=C2[0], k=C2[1], params=b.params, num_minibatches=C2[2], clip_value_loss=False, options={"gemm": 2, "fuse_optim": fuse})
        try:
            b._load(agent)
            h = agent.handle
            assert h.get_option("fuse_optim") == fuse
            set_geometry(h, case)
            p, m, v = b.params.copy(), np.zeros_like(b.params), np.zeros_like(b.params)
            betap = np.array([0.9, 0.999] * 12)
            assert np.array_equal(h.read(F.F_PARAMS), p) and not h.read(F.F_ADAM_M).any() and not h.read(F.F_ADAM_V).any()
            assert np.array_equal(h.read(F.F_BETAP), betap)
            h.update_minibatch(mb, eta, apply_update=True)
            g = h.read(F.F_GRADS).copy()
            _grad_close(g, g_o, b.off)
            assert [bool(c) for _, _, c in optimlib.array_norms(route, g)] == flags
            O.clipnorm_adam(b.cfgo, p, g, m, v, betap, eta)
            for name, f, want in (("parameters", F.F_PARAMS, p), ("Adam m", F.F_ADAM_M, m), ("Adam v", F.F_ADAM_V, v)):
                msg = optimlib.first_mismatch(route, name, h.read(f), want, flags)
                assert msg is None, f"fuse_optim = {fuse}, {case.id}: {msg}"
            assert not np.array_equal(p, b.params)
            grads[fuse] = g
        finally:
            agent.close()
    assert np.array_equal(grads[1], grads[0]), f"{case.id}: {np.sum(grads[1] != grads[0])} gradient entries differ between the one-launch and the two-launch step"
