"""The update pass's launch geometry as integer work (no GPU): tests/update_geometry.py restates how csrc/api.cpp and csrc/update.hip turn
(M, actor_block_pct, update_xcd_align) into block counts and how the waves of update_role / update16_role walk the tiles; here every case of
the shared table, and a sweep far around it, is held to three invariants —
  every tile of [0, ntiles) is visited exactly once and none beyond it, by the plain, the XCD-aligned and the 16-sample walk (and by the exact
  value-loss pass and the reduce over the blocks);
  nA + nC == total and 1 <= nA, nC <= update_blocks, the capacity of the partial buffers;
  the aligned striding is chosen only when both counts are multiples of 8
— and the table is held to its purpose: every edge it is there for is met, by the case named for it.
tests/test_gpu_update_geometry.py runs the same cases through the kernels against the oracle, which knows nothing of geometry."""
import numpy as np
import pytest

import update_geometry as G


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_case_keeps_the_launch_invariants(case):
    nA, nC, aligned = G.check_launch(case.M, case.pct, case.align)
    assert (nA, nC) == case.blocks and aligned == case.aligned
    assert G.ceil_div(G.ntiles(case.M), 4) <= 64 < G.CUS, "the table's shapes are those where the CU count never decides"
    # per role, in full: the wave that owns a tile is unique, and the waves past the last tile own nothing
    for nblk in case.blocks:
        walk = G.role_walk(nblk, case.M, aligned)
        assert len(walk) == nblk * G.RW
        owner = {}
        for key, tiles in walk.items():
            for t in tiles:
                assert 0 <= t < G.ntiles(case.M) and t not in owner, (case.id, key, t, owner.get(t))
                owner[t] = key
        assert len(owner) == G.ntiles(case.M)
        # the sweep's vectorised counter is the same rule
        assert np.array_equal(G.visit_counts(nblk, case.M, aligned), np.bincount(sorted(owner), minlength=G.ntiles(case.M)))
        G.check_walk(G.role_walk16(nblk, case.M), G.ntiles(case.M, G.TILE16), f"{case.id}: 16-sample walk of {nblk} blocks")
    G.check_walk(G.exact_walk(case.ub, case.M), G.ntiles(case.M), f"{case.id}: exact value-loss pass")


def test_block_counts_of_the_table_are_the_ones_it_was_built_for():
    def splits(shape, align):
        return [c.blocks for c in G.CASES if c.shape == shape and c.align == align]
    assert [G.minibatch_size(s) for s in G.SHAPES] == [592, 4096, 8192]
    assert [(G.update_blocks(G.minibatch_size(s)), G.total_blocks(G.update_blocks(G.minibatch_size(s)))) for s in G.SHAPES] == [(5, 6), (32, 32), (64, 64)]
    assert splits((128, 128, 4), 0) == [(1, 31), (8, 24), (16, 16), (24, 8), (31, 1)]
    assert splits((128, 128, 4), 1) == [(8, 24), (8, 24), (16, 16), (24, 8), (24, 8)]
    assert splits((256, 128, 4), 1) == [(8, 56), (16, 48), (32, 32), (48, 16), (56, 8)]
    assert all(c.aligned == bool(c.align) for c in G.CASES if c.shape != (37, 64, 4))
    assert not any(c.aligned for c in G.CASES if c.shape == (37, 64, 4)), "6 blocks: below the 8-alignment's threshold"
    # the 8-alignment needs total % 8 == 0 and total >= 32: 121 tiles (M = 3841) is the first launch with 32 blocks, M = 4096 the first whole-tile shape of the table
    assert G.total_blocks(G.update_blocks(3841)) == 32 and G.main_pass_blocks(G.update_blocks(3841), 1, 1) == (8, 24)
    for M in range(1, 3841):
        ub = G.update_blocks(M)
        assert all(G.main_pass_blocks(ub, p, 1) == G.main_pass_blocks(ub, p, 0) for p in G.PCTS), M


@pytest.mark.parametrize("edge", G.EDGES)
def test_every_edge_of_the_table_is_met_by_its_case(edge):
    case = G.WITNESS[edge]
    assert case in G.CASES, f"the witness of '{edge}' is no case of the table"
    assert edge in case.edges, f"case {case.id} no longer meets its edge '{edge}' (it meets: {sorted(case.edges)})"


def test_edges_where_the_issue_places_them():
    e = {c.id: c.edges for c in G.CASES}
    at = lambda shape, pct, align: G.Case(shape, pct, align).edges
    # M = 4096 plain, one actor block: 8 waves x 16 tiles, so ntiles >= 16·tstride and the feedback rule turns itself on — in the actor only
    assert G.E_BALANCE_ACTOR in at((128, 128, 4), 1, 0) and G.E_BALANCE_CRITIC not in at((128, 128, 4), 1, 0)
    assert G.E_BALANCE_CRITIC in at((128, 128, 4), 99, 0) and G.E_BALANCE_ACTOR not in at((128, 128, 4), 99, 0)
    assert not any({G.E_BALANCE_ACTOR, G.E_BALANCE_CRITIC} & c.edges for c in G.CASES if c.aligned), "an aligned role has at least 8 blocks"
    # (8, 56) and (56, 8): groups 0-7 of the 56-block role run one unrolled round, groups 8-15 three tail rounds
    assert [G.reduce_rounds(56, g)[:2] for g in (0, 7, 8, 15)] == [(1, 0), (1, 0), (0, 3), (0, 3)]
    assert G.E_REDUCE_MIX in at((256, 128, 4), 1, 1) and G.E_REDUCE_MIX in at((256, 128, 4), 99, 1)
    assert not any(G.E_REDUCE_MIX in c.edges for c in G.CASES if c.M < 8192), "below 49 blocks in a role nobody reaches the unrolled loop"
    # M = 592 = 18 tiles of 32 and one of 16: 19 tiles for up to 40 waves
    assert all({G.E_IDLE_WAVES, G.E_RAGGED} <= c.edges or c.blocks[0] == c.blocks[1] for c in G.CASES if c.M == 592)
    assert len(e) == len(G.CASES) == 30, "case ids are unique"


def test_predicates_follow_update_role():
    # small_prio passes the option through only where balance is off by itself; option 1 turns balance on anywhere
    M = 4096
    for nblk, aligned in ((16, True), (1, False), (31, False)):
        big = G.ntiles(M) >= 16 * G.tstride(nblk, aligned)
        for mode in (0, 1, 2, 3):
            assert G.balance(M, nblk, aligned, mode) == (big or mode == 1)
            assert G.small_prio(M, nblk, aligned, mode) == (0 if big else mode)
            assert not G.balance(M, nblk, aligned, mode, x2=False) and G.small_prio(M, nblk, aligned, mode, x2=False) == 0
    assert G.tstride(16, True) == G.tstride(16, False) == 128 and G.tstride(24, True) == 192
    # the smallest launch at the default split that turns the feedback rule on by itself (the M ≈ 557k of the kernel's comment)
    first = next(M for M in range(32, 1 << 21, 32) if G.balance(M, G.main_pass_blocks(G.update_blocks(M), 53, 1)[0],
                                                                 G.xcd_align(*G.main_pass_blocks(G.update_blocks(M), 53, 1), 1)))
    assert 540_000 < first < 570_000, first


# M = 1 … 2100 in steps of 1 (every tile count up to 66, every ragged remainder twice over), then odd strides up to 20000 (tile counts to 625,
# update_blocks to 157: the aligned rule at many totals, reduce groups with one unrolled round, two, and a tail behind them).
SWEEP_M = list(range(1, 2101)) + list(range(2101, 20001, 251)) + [4096, 8192, 16384, 20000]


def test_sweep_of_sizes_and_options_keeps_the_launch_invariants():
    """Condition: sized to a few seconds of integer work — above M = 2100 only every 251st size is visited (plus the powers of two and 20000)."""
    launches = 0
    for M in SWEEP_M:
        for align in (0, 1):
            for pct in range(1, 100):
                G.check_launch(M, pct, align)
                launches += 1
    assert launches == len(SWEEP_M) * 2 * 99
    # the sweep met what it is for: aligned and plain launches, one-block roles, roles whose reduce runs both loops in one group
    assert any(G.reduce_rounds(n, 0)[0] > 0 and G.reduce_rounds(n, 0)[1] > 0 for n in range(1, 158))
    # and with fewer CUs than tiles ask for, the count decides and the invariants still hold
    for cus in (1, 2, 7, 8, 64, 255):
        for M in (1, 33, 592, 4096, 8192, 20000):
            for align in (0, 1):
                for pct in (1, 50, 53, 99):
                    G.check_launch(M, pct, align, cus)
