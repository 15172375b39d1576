"""The GAE scan at its kernel, horizon and terminal-flag edges: every row of tests/gae_cases.py's table — between them the rows reach each of the 50 kernels
that csrc/gae.hip:launch_gae can launch, the ragged edges, num_steps = 1024 on all three kernel families, both L 8 → 16 fallbacks — with both load flavours,
in both modes, on the input family the table deals the case (tests/test_gae_cpu.py: every family meets every kernel family at L / D = 8 and 16).

Bars, none taken from the kernels (tests/gae_ref.py derives the bound 4·(k − t)·2^-53·S_t; test_gae_cpu.py shows the references use under a tenth of it):
  streaming kernel     advantages and returns bit-equal to serial64 cast to Float32, on all envs;
  one-env, pair        RN32(x − bound) <= adv <= RN32(x + bound) with x = the exact rational recurrence on up to 16 envs (the first, the last, both sides of the
                       first and the last block edge) and RN32(x − 2·bound) <= adv <= RN32(x + 2·bound) with x = serial64 on the rest;
  all                  ret bit-equal to adv + value in Float32;
  pair                 bit-equal to the one-env kernel at the same L.
How many outputs differ from RN32(exact) is printed per case and, with CRL_WRITE_PROFILES=1, summed per kernel family into profiles/gae_edges.json ("gpu_outputs_differing_from_rn32")."""
import re

import numpy as np
import pytest

import gae_cases as G
import gae_ref as R
from gae_cases import WRITE, write_profile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1, "HIP library loaded but no GPU visible"
    return crl


@pytest.fixture(scope="module")
def profile():
    rec = {}
    yield rec
    if WRITE and rec:
        write_profile("gpu_outputs_differing_from_rn32", rec)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_segmented(adv, d, mode, r):
    """The interval checks of a one-env or pair launch; returns (outputs differing from RN32(exact), outputs held to exact)."""
    a = G.args(d, mode)
    x64, b = R.serial64(*a), R.bound(*a)
    assert np.isfinite(adv).all()
    lo, hi = R.interval64(x64, b, 2.0)
    out = R.outside(adv, lo, hi)
    assert not out.any(), f"{int(out.sum())} outputs outside serial64 ± 2·bound, first at (env, step) {tuple(np.argwhere(out)[0])}"
    differ = checked = 0
    for e in G.exact_envs(adv.shape[0], r):
        x = R.exact(d["value"][e], d["reward"][e], d["term"][e], d["nv"][e], d["nd"][e], d["gamma"], d["lam"], mode)
        lo, hi = R.interval_exact(x, b[e])
        out = R.outside(adv[e], lo, hi)
        assert not out.any(), f"env {e}: {int(out.sum())} outputs outside exact ± bound, first at step {int(np.argmax(out))}"
        differ += int(np.sum(bits(adv[e]) != bits(np.array([R.rn32(xi) for xi in x], np.float32)))); checked += len(x)
    return differ, checked


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_every_kernel_at_its_edges(crl, profile, case):
    row, r = case.row, case.route
    d = G.inputs(case.family, row.nt, row.k)
    a = G.args(d, case.mode)
    adv, ret = crl._lib.gae_host(*a, seg=row.seg, tile=row.tile, nt_loads=case.ntl)
    assert np.array_equal(bits(ret), bits(adv + d["value"])), "ret is not adv + value in Float32"
    rec = profile.setdefault(r[0], dict(differ_from_rn32_exact=0, held_to_exact=0, differ_from_rn32_serial64=0, outputs=0))
    a32 = R.serial64(*a).astype(np.float32)
    n_serial = int(np.sum(bits(adv) != bits(a32)))
    if r[0] == "stream":
        assert n_serial == 0, f"{n_serial} of {adv.size} advantages differ from serial64 in Float32"
        differ = checked = 0
    else:
        differ, checked = check_segmented(adv, d, case.mode, r)
    if r[0] == "pair":
        one = G.route(row.nt, row.k, r[2], 8)
        assert one == ("one", 8, r[2]), one
        adv1, ret1 = crl._lib.gae_host(*a, seg=r[2], tile=8, nt_loads=case.ntl)
        assert np.array_equal(bits(adv), bits(adv1)) and np.array_equal(bits(ret), bits(ret1)), "the pair kernel differs from the one-env kernel at the same L"
    print(f"{G.case_id(case)}: {differ} of {checked} differ from RN32(exact), {n_serial} of {adv.size} from RN32(serial64)")
    rec["differ_from_rn32_exact"] += differ; rec["held_to_exact"] += checked; rec["differ_from_rn32_serial64"] += n_serial; rec["outputs"] += adv.size


@pytest.mark.parametrize("row,err", G.ERROR_ROWS, ids=lambda p: p.why.replace(" ", "") if isinstance(p, G.Row) else None)
def test_error_rows_report_their_error_and_leave_nothing_behind(crl, row, err):
    """num_steps = 1025 on the one-env and the pair kernel (their own segment length or a forced one), an env count the vector accesses cannot take; the next
    launch — the streaming kernel at k = 1500, which has no limit — is bit-equal as if nothing had happened."""
    d = G.inputs("standard", row.nt, row.k)
    with pytest.raises(crl.CrlError, match=re.escape(err)):
        crl._lib.gae_host(*G.args(d, 1), seg=row.seg, tile=row.tile, nt_loads=0)
    d = G.inputs("flag_bytes", 4, 1500)
    for mode in (0, 1):
        adv, ret = crl._lib.gae_host(*G.args(d, mode), seg=16, tile=2, nt_loads=0)
        a32 = R.serial64(*G.args(d, mode)).astype(np.float32)
        assert np.array_equal(bits(adv), bits(a32)) and np.array_equal(bits(ret), bits(a32 + d["value"]))


def test_single_env_entry_point_passes_seg_and_tile_through(crl):
    """crl.gae (one env, values / terminals of k + 1 entries): gae_tile = 1 is the streaming kernel (bit-equal), gae_seg / gae_tile = 16 / 8 the one-env kernel
    with 16-step segments (exact ± bound), gae_tile = 128 needs an even env count, and k = 1025 is refused by the segmented kernels only."""
    k = 100
    d = G.inputs("flag_bytes", 1, k)
    values = np.concatenate([d["value"][0], d["nv"]]); terms = np.concatenate([d["term"][0], d["nd"]])
    for mode in (0, 1):
        a = G.args(d, mode)
        a32 = R.serial64(*a).astype(np.float32)[0]
        for seg in (4, 8, 16):
            got = crl.gae(values, d["reward"][0], terms, d["gamma"], d["lam"], mode=mode, seg=seg, tile=1, nt_loads=1)
            assert np.array_equal(bits(got), bits(a32))
        x = R.exact(d["value"][0], d["reward"][0], d["term"][0], d["nv"][0], d["nd"][0], d["gamma"], d["lam"], mode)
        lo, hi = R.interval_exact(x, R.bound(*a)[0])
        for seg, tile in ((16, 8), (8, 64), (0, 0)):
            got = crl.gae(values, d["reward"][0], terms, d["gamma"], d["lam"], mode=mode, seg=seg, tile=tile, nt_loads=0)
            assert not R.outside(got, lo, hi).any(), (mode, seg, tile)
        with pytest.raises(crl.CrlError, match="needs an even num_envs"):
            crl.gae(values, d["reward"][0], terms, d["gamma"], d["lam"], mode=mode, tile=128)
    d = G.inputs("standard", 1, 1025)
    values = np.concatenate([d["value"][0], d["nv"]]); terms = np.concatenate([d["term"][0], d["nd"]])
    with pytest.raises(crl.CrlError, match="num_steps > 1024"):
        crl.gae(values, d["reward"][0], terms, 0.99, 0.95)
    got = crl.gae(values, d["reward"][0], terms, 0.99, 0.95, mode=1, tile=1)
    assert np.array_equal(bits(got), bits(R.serial64(*G.args(d, 1)).astype(np.float32)[0]))


def test_handle_options_select_the_same_kernels_as_gae_host(crl):
    """One compat-mode handle with the flag_bytes family in its rollout buffers: crl_compute_gae under gae_seg x gae_tile x gae_nt_loads set through
    crl_ppo_set_option equals crl_gae_opt with the same three values bit for bit, and the values the option table has no kernel for are refused."""
    F = crl._lib
    nt, k = 8, 40
    cfg = crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 10, num_minibatches=1)
    agent = crl.Agent(cfg)
    h = agent.handle
    try:
        d = G.inputs("flag_bytes", nt, k)
        value, reward, term = (np.asfortranarray(d[n]) for n in ("value", "reward", "term"))
        h.write(F.F_VALUE, value); h.write(F.F_REWARD, reward); h.write(F.F_TERMINAL, term); h.write(F.F_NEXT_DONE, d["nd"])
        a32 = R.serial64(value, reward, term, np.zeros(nt, np.float32), d["nd"], cfg.gamma, cfg.gae_lambda, 0).astype(np.float32)
        seen = set()
        for seg in (8, 16):
            for tile in (1, 2, 8, 64, 128, 256):
                for ntl in (0, 1):
                    h.set_option("gae_seg", seg); h.set_option("gae_tile", tile); h.set_option("gae_nt_loads", ntl)
                    assert (h.get_option("gae_seg"), h.get_option("gae_tile"), h.get_option("gae_nt_loads")) == (seg, tile, ntl)
                    h.compute_gae()
                    adv_h, ret_h = h.read(F.F_ADVANTAGE), h.read(F.F_RETURN)
                    adv_g, ret_g = F.gae_host(value, reward, term, None, d["nd"], cfg.gamma, cfg.gae_lambda, 0, seg=seg, tile=tile, nt_loads=ntl)
                    assert np.array_equal(bits(adv_h), bits(adv_g)) and np.array_equal(bits(ret_h), bits(ret_g)), (seg, tile, ntl)
                    r = G.route(nt, k, seg, tile)
                    seen.add(r)
                    if r[0] == "stream":
                        assert np.array_equal(bits(adv_h), bits(a32)), (seg, tile, ntl)
        assert seen == {("stream", 1, 8), ("stream", 2, 8), ("stream", 1, 16), ("stream", 2, 16), ("one", 8, 8), ("one", 8, 16), ("pair", 32, 8), ("pair", 32, 16),
                        ("pair", 64, 8), ("pair", 64, 16)}
        for key, bad, msg in (("gae_seg", 3, "gae_seg is 0"), ("gae_tile", 3, "gae_tile is 0"), ("gae_nt_loads", 3, "outside")):
            before = h.get_option(key)
            with pytest.raises(crl.CrlError, match=msg):
                h.set_option(key, bad)
            assert h.get_option(key) == before
    finally:
        agent.close()
