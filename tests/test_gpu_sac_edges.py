"""The SAC kernels (csrc/sac.hpp) at their hard places: tests/sac_bar.py's EDGE_CASES against tests/sac_ref.py. Two cases sit where the squash is ill
conditioned (`saturated`: |y| = 1 exactly and 0 < 1 − y² < 1e-6; `logstd_ends`: log_std within 1e-3 of −5 and of 2) and have, each, 32 x its own
jitter floor of profiles/sac_edges_bar.json as its loss bar (9.1e-10 and 1.7e-12: the harder one does not loosen the other); the batch, ring and logging edges (k = 65, the default 120, k = n = 1024 on a wrapping ring,
log_frequency = 7) are as well conditioned as the first table's cases and have to meet its tighter bar too. Every edge is asserted on the
reference's own counters, so a case that stops meeting its edge fails whatever the device does."""
import pytest

import sac_bar as B
from test_gpu_sac import _same, check_case, feed_case

pytestmark = pytest.mark.gpu
HARD = ("saturated", "logstd_ends")


@pytest.fixture(scope="module")
def crl():
    import cleanrl_jl_amd as crl
    assert crl.device_count() >= 1
    return crl


@pytest.mark.parametrize("name", [c["name"] for c in B.EDGE_CASES])
def test_the_edge_table_matches_the_reference(crl, name):
    case = B.EDGE_CASE[name]
    n = case["T"]
    d0 = B.case_cfg(case)
    thr = B.threshold(d0)
    ends = sorted({1, thr, thr + 1, (thr + n) // 2, n})
    d, h, ref, losses, arecs = feed_case(crl, case, ends)
    # the edges, on the reference's own counters
    stats = {s: int(getattr(ref, s)) for s in B.STATS}
    assert B.edge_met(name, stats), stats
    if name == "saturated":
        assert stats["n_y_one"] > 0 and stats["n_y_near"] > 0
    if name == "logstd_ends":
        assert stats["n_ls_low"] > 0 and stats["n_ls_high"] > 0
    if name == "kmax_ring_eq_batch":
        assert d["batch_size"] == d["buffer_size"] == 1024 and ref.rb.ptr == n % 1024 and ref.rb.size == 1024, "k = n and the ring wrapped"
    if name == "k65":
        assert 16 * (d["batch_size"] - 1) >= 1024, "component words reach 1024"
    edge_loss_bar, param_bar = B.load_bars(B.EDGE_BAR_JSON)
    loss_bar = B.case_loss_bar(name) if name in HARD else min(edge_loss_bar, B.load_bars()[0])
    assert loss_bar <= edge_loss_bar
    check_case(d, h, ref, losses, arecs, case, loss_bar, param_bar)
    params = h.read_params()
    h.close()
    if d["log_frequency"] > 1:
        # logging changes no number: a handle that logs every update ends on the same bits, and its records at the logged steps are the filtered ones
        _, h1, _, every, every_alpha = feed_case(crl, case, ends, log_frequency=1)
        assert _same(h1.read_params(), params)
        h1.close()
        steps = [l[0] for l in losses]
        assert steps == [g for g in range(thr + 1, n + 1) if g % 7 == 0]
        assert [l for l in every if l[0] in steps] == losses and [r for r in every_alpha if r[0] in steps] == arecs
