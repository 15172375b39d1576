"""Launch geometry of the fused 4/2/64 update pass, restated in plain Python, and the case table that
tests/test_update_geometry_cpu.py (integer work) and tests/test_gpu_update_geometry.py (the kernels against the oracle) share.

Restated, line by line and without sharing any code with the library:
  crl_ppo_create (csrc/api.cpp)       update_blocks = min(CUs, ceil(ceil(M / 32) / 4)), at least 1 — the capacity (blocks per role) of the partial buffers
  main_pass_blocks (csrc/update.hip)  the actor / critic block counts from option actor_block_pct, the multiples-of-8 rule of update_xcd_align and its clamps
  run_update (csrc/update.hip)        UpdateArgs::xcd_align: both counts multiples of 8 and the option on
  update_role (csrc/update.hip)       the two tile walks of a role's RW = 8 waves per block: plain (tile = rb·RW + wave, stride nblk·RW) and XCD-aligned
                                      (tile = (rb & 7) + 8·((rb >> 3)·RW + wave), stride 8·(nblk >> 3)·RW); the predicates `balance` and `small_prio`
  update16_role (csrc/update16.hpp)   the 16-sample-tile kernel's walk: RW16 = 12 waves per block, always plain
  reduce_partial_sums (update.hip)    which of its two loops (4·RG-unrolled, tail; RG = 16) thread group g runs for a role of nblk blocks

The CU count is taken as 256 (MI355X). Every shape of the table has ceil(ntiles / 4) <= 64, so the count never decides."""
import functools
from collections import namedtuple

import numpy as np

CUS = 256
TILE, RW = 32, 8        # update_x2_kernel / update_x3_kernel: samples per tile, waves per block
TILE16, RW16 = 16, 12   # update_t16_kernel
RW_EXACT = 4            # update_vfix_kernel (run_update mode 1): 256-thread blocks, critic only, update_blocks of them
RG = 16                 # reduce_kernel / reduce_optim_kernel: thread groups per output

PCTS = (1, 25, 53, 75, 99)
SHAPES = ((37, 64, 4), (128, 128, 4), (256, 128, 4))   # (num_envs, num_steps, num_minibatches): M = 592, 4096, 8192


def ceil_div(a, b):
    return -(-a // b)


def minibatch_size(shape):
    nt, k, nmb = shape
    assert (nt * k) % nmb == 0
    return nt * k // nmb


def ntiles(M, tile=TILE):
    return ceil_div(M, tile)


def update_blocks(M, cus=CUS):
    ub = cus
    if ub * 4 > ntiles(M):
        ub = ceil_div(ntiles(M), 4)
    return max(ub, 1)


def total_blocks(ub):
    return 2 * ((ub + 1) // 2)


def main_pass_blocks(ub, pct, align_opt):
    """(nA, nC) of the main pass."""
    total = total_blocks(ub)
    a = total * pct // 100
    a = max(a, 1)
    a = min(a, total - 1)
    if total < 2:
        return 1, 1
    if total % 8 == 0 and total >= 32 and align_opt:
        a = ((a + 4) // 8) * 8
        a = max(a, 8)
        a = min(a, total - 8)
    return a, total - a


def xcd_align(nA, nC, align_opt):
    return bool(nA % 8 == 0 and nC % 8 == 0 and align_opt)


def tstride(nblk, aligned, rw=RW):
    return 8 * (nblk >> 3) * rw if aligned else nblk * rw


def first_tile(rb, wave, aligned, rw=RW):
    return (rb & 7) + 8 * ((rb >> 3) * rw + wave) if aligned else rb * rw + wave


def role_walk(nblk, M, aligned, rw=RW, tile=TILE):
    """{(block, wave): [tiles, in the order the wave works on them]} of one role of the 32-sample kernels."""
    nt, st = ntiles(M, tile), tstride(nblk, aligned, rw)
    assert st > 0, "a role without a stride would never leave its first tile"
    return {(rb, w): list(range(first_tile(rb, w, aligned, rw), nt, st)) for rb in range(nblk) for w in range(rw)}


def role_walk16(nblk, M):
    """The same for update16_role: tile = rb·RW16 + wave, stride nblk·RW16, 16-sample tiles."""
    return role_walk(nblk, M, False, RW16, TILE16)


def exact_walk(ub, M):
    """The exact value-loss pass: update_blocks critic blocks of four waves, plain striding."""
    return role_walk(ub, M, False, RW_EXACT, TILE)


def balance(M, nblk, aligned, prio_mode=0, x2=True):
    """The feedback priority rule runs (update_role): by itself from 16 tiles per wave on, or under update_prio_small = 1."""
    return bool(x2 and (ntiles(M) >= 16 * tstride(nblk, aligned) or prio_mode == 1))


def small_prio(M, nblk, aligned, prio_mode, x2=True):
    return prio_mode if (x2 and ntiles(M) < 16 * tstride(nblk, aligned)) else 0


def reduce_rounds(nblk, g):
    """(rounds of the 4·RG-unrolled loop, rounds of the tail) that thread group g of reduce_partial_sums runs over a role of nblk blocks,
    and the blocks it adds, in order."""
    b, unrolled, tail, seen = g, 0, 0, []
    while b + 3 * RG < nblk:
        seen += [b, b + RG, b + 2 * RG, b + 3 * RG]
        b += 4 * RG
        unrolled += 1
    while b < nblk:
        seen.append(b)
        b += RG
        tail += 1
    return unrolled, tail, seen


def reduce_mixes_branches(nblk):
    """Some groups of this role's reduce take the unrolled loop and some only the tail."""
    r = [reduce_rounds(nblk, g)[:2] for g in range(RG)]
    return any(u > 0 for u, _ in r) and any(u == 0 and t > 0 for u, t in r)


# ---- the invariants every launch must keep (test_update_geometry_cpu.py sweeps them; the messages name what broke) -----------------
def check_walk(walk, n, what):
    seen = sorted(t for tiles in walk.values() for t in tiles)
    assert seen == list(range(n)), (f"{what}: the walk does not visit every tile of [0, {n}) exactly once: "
                                    f"missing {sorted(set(range(n)) - set(seen))[:8]}, beyond or repeated {[t for t in seen if t >= n or seen.count(t) > 1][:8]}")


def visit_counts(nblk, M, aligned, rw=RW, tile=TILE):
    """How often each tile of [0, ntiles) is visited — role_walk's rule (first_tile, then steps of tstride while below ntiles) on all waves at
    once, for the sweep: a walk of Python lists per (M, nblk) costs a hundred times as much."""
    n, st = ntiles(M, tile), tstride(nblk, aligned, rw)
    assert st > 0
    rb, wave = np.divmod(np.arange(nblk * rw), rw)
    t = first_tile(rb, wave, aligned, rw)
    counts = np.zeros(n, np.int64)
    while True:
        t = t[t < n]
        if not t.size:
            return counts
        counts += np.bincount(t, minlength=n)
        t = t + st


def _check_counts(nblk, M, aligned, rw, tile, what):
    if not np.all(visit_counts(nblk, M, aligned, rw, tile) == 1):
        check_walk(role_walk(nblk, M, aligned, rw, tile), ntiles(M, tile), what)   # the slow way, for its message
        raise AssertionError(f"{what}: visit_counts and role_walk disagree")


@functools.lru_cache(maxsize=None)
def check_role(M, nblk, aligned):
    _check_counts(nblk, M, aligned, RW, TILE, f"M = {M}, a role of {nblk} blocks, {'aligned' if aligned else 'plain'} walk")


@functools.lru_cache(maxsize=None)
def check_role16(M, nblk):
    _check_counts(nblk, M, False, RW16, TILE16, f"M = {M}, a role of {nblk} blocks, 16-sample walk")


@functools.lru_cache(maxsize=None)
def check_exact(M, ub):
    _check_counts(ub, M, False, RW_EXACT, TILE, f"M = {M}, exact value-loss pass on {ub} blocks")


@functools.lru_cache(maxsize=None)
def check_reduce(nblk):
    blocks = sorted(b for g in range(RG) for b in reduce_rounds(nblk, g)[2])
    assert blocks == list(range(nblk)), f"a role of {nblk} blocks: the reduce does not add every block's partial exactly once"


def check_launch(M, pct, align_opt, cus=CUS):
    """The three invariants of one launch — the walks cover [0, ntiles) exactly once (plain or aligned, 16-sample, exact pass, and the reduce
    over the blocks); nA + nC == total with both inside the partial buffers; aligned striding only on multiples of 8. Returns (nA, nC, aligned).
    (The per-role checks are pure functions of their arguments and cached: a sweep meets the same role many times.)"""
    ub = update_blocks(M, cus)
    nA, nC = main_pass_blocks(ub, pct, align_opt)
    def what():   # (built only for a failure: a sweep calls this function several hundred thousand times)
        return f"M = {M}, actor_block_pct = {pct}, update_xcd_align = {align_opt}: blocks ({nA}, {nC}) of {total_blocks(ub)}, capacity {ub}"
    assert nA + nC == total_blocks(ub), what()
    assert 1 <= nA <= ub and 1 <= nC <= ub, f"{what()}: a role outgrows the partial buffers or has no block"
    aligned = xcd_align(nA, nC, align_opt)
    assert not aligned or (nA % 8 == 0 and nC % 8 == 0 and nA >= 8 and nC >= 8), f"{what()}: aligned striding with a count that is no multiple of 8"
    for nblk in (nA, nC):
        check_role(M, nblk, aligned)
        check_role16(M, nblk)
        check_reduce(nblk)
    check_exact(M, ub)
    return nA, nC, aligned


# ---- the case table ----------------------------------------------------------------------------------------------------------------
E_ONE_BLOCK = "one block in a role"
E_IDLE_WAVES = "idle waves in a role"
E_IDLE_BLOCK = "an idle block in a role"          # all eight waves without a tile: the block must still write zero partials
E_RAGGED = "ragged tile under an uneven split"
E_BALANCE_ACTOR = "balance on in the actor"
E_BALANCE_CRITIC = "balance on in the critic"
E_REDUCE_MIX = "reduce: unrolled and tail in one launch"
E_PLAIN_UNEVEN = "plain striding with nA != nC"
E_ALIGNED_UNEVEN = "aligned striding with nA != nC"
EDGES = (E_ONE_BLOCK, E_IDLE_WAVES, E_IDLE_BLOCK, E_RAGGED, E_BALANCE_ACTOR, E_BALANCE_CRITIC, E_REDUCE_MIX, E_PLAIN_UNEVEN, E_ALIGNED_UNEVEN)


class Case(namedtuple("Case", "shape pct align")):
    """One launch geometry: a shape and the two options that decide the block split. Everything else is computed."""
    __slots__ = ()

    @property
    def M(self):
        return minibatch_size(self.shape)

    @property
    def ub(self):
        return update_blocks(self.M)

    @property
    def blocks(self):
        return main_pass_blocks(self.ub, self.pct, self.align)

    @property
    def aligned(self):
        return xcd_align(*self.blocks, self.align)

    @property
    def id(self):
        nA, nC = self.blocks
        return f"M{self.M}-pct{self.pct}-{'aligned' if self.aligned else 'align' + str(self.align)}-{nA}+{nC}"

    @property
    def edges(self):
        M, (nA, nC), al = self.M, self.blocks, self.aligned
        e = set()
        if nA == 1 or nC == 1:
            e.add(E_ONE_BLOCK)
        for nblk in (nA, nC):
            walk = role_walk(nblk, M, al)
            if any(not t for t in walk.values()):
                e.add(E_IDLE_WAVES)
            if any(all(not walk[(rb, w)] for w in range(RW)) for rb in range(nblk)):
                e.add(E_IDLE_BLOCK)
        if M % TILE and nA != nC:
            e.add(E_RAGGED)
        if balance(M, nA, al):
            e.add(E_BALANCE_ACTOR)
        if balance(M, nC, al):
            e.add(E_BALANCE_CRITIC)
        if reduce_mixes_branches(nA) or reduce_mixes_branches(nC):
            e.add(E_REDUCE_MIX)
        if nA != nC:
            e.add(E_ALIGNED_UNEVEN if al else E_PLAIN_UNEVEN)
        return frozenset(e)


CASES = tuple(Case(s, p, a) for s in SHAPES for p in PCTS for a in (0, 1))

# the case that stands for each edge: should a change to the restated rules (or to the table) stop it from meeting the edge, the CPU test says which
WITNESS = {
    E_ONE_BLOCK: Case((128, 128, 4), 1, 0),
    E_IDLE_WAVES: Case((37, 64, 4), 53, 1),
    E_IDLE_BLOCK: Case((37, 64, 4), 99, 0),
    E_RAGGED: Case((37, 64, 4), 25, 0),
    E_BALANCE_ACTOR: Case((128, 128, 4), 1, 0),
    E_BALANCE_CRITIC: Case((128, 128, 4), 99, 0),
    E_REDUCE_MIX: Case((256, 128, 4), 1, 1),
    E_PLAIN_UNEVEN: Case((128, 128, 4), 25, 0),
    E_ALIGNED_UNEVEN: Case((128, 128, 4), 75, 1),
}


def case_with_blocks(shape, nA, nC, aligned):
    """The table's case of this shape whose launch has these block counts and this striding."""
    hits = [c for c in CASES if c.shape == tuple(shape) and c.blocks == (nA, nC) and c.aligned == bool(aligned)]
    assert hits, f"no case of the table gives blocks ({nA}, {nC}), {'aligned' if aligned else 'plain'}, at shape {shape}"
    return hits[0]
