"""Randomised whole-iteration parity in the GPU suite: 40 random small configurations (seed 1) of tests/fuzzlib.py on the CartPole path and
24 on the layer-wise path (random shape and kernel flavour) — permutations and actions bit-equal, losses within 2e-6 relative, parameters
within 1e-5 relative L2 — against the CPU oracle."""
import numpy as np
import pytest

import fuzzlib
import oraclelib as O

pytestmark = pytest.mark.gpu


def test_forty_random_configurations_match_the_oracle():
    import cleanrl_jl_amd as crl
    rng = np.random.default_rng(1)
    lines = [fuzzlib.run_case(crl, O, rng, case) for case in range(40)]
    bad = [l for l in lines if not l["ok"]]
    assert not bad, bad[:3]
    assert max(l["loss_rel"] for l in lines) <= fuzzlib.LOSS
    # the sweep must have covered both drivers and both GAE modes
    assert {l["blocked"] for l in lines} == {True, False} and {l["gae_mode"] for l in lines} == {0, 1}


def test_twenty_four_random_layer_wise_configurations_match_the_oracle():
    import cleanrl_jl_amd as crl
    rng = np.random.default_rng(1)
    lines = [fuzzlib.run_wide_case(crl, O, rng, case) for case in range(24)]
    bad = [l for l in lines if not l["ok"]]
    assert not bad, bad[:3]
    assert max(l["loss_rel"] for l in lines) <= fuzzlib.LOSS
    # the draw must have covered 2x256 past 8 actions, obs past 16 and all three GEMM flavours
    assert any(l["H"] == 256 and l["A"] > 8 for l in lines) and any(l["D"] > 16 for l in lines)
    assert {l["wide_gemm"] for l in lines} == {0, 1, 2}
