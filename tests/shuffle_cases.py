"""The shapes, keys, advantage families and routes at which the epoch shuffles (csrc/shuffle.hip, csrc/bijection.hpp) and the per-minibatch advantage
sums (shuffle.hip, optim.hip, records.hip) are held to tests/shuffle_ref.py. tests/test_shuffle_cpu.py holds this table to its purposes (every route
reached, the straddling cases really straddle); tests/test_gpu_shuffle_edges.py runs it; scripts/shuffle_route_trace.py traces it.

A shape is (num_envs, num_steps): num_steps <= 1024 and the batch must divide by num_minibatches, so odd and prime batch sizes are n envs of 1 step
or a factorisation (4097 = 241·17, 2405 = 37·65, 8194 = 241·34, 11262 = 1877·6)."""
import json
import os
from collections import namedtuple

import numpy as np

import shuffle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = os.path.join(ROOT, "profiles", "shuffle_route_trace.json")

# ---------------------------------------------------------------------------------------------------------------- permutation sizes
# every mode: the 1-, 2- and 3-bit words of the bijection, n = 2^b − 1, 2^b and 2^b + 1 (cycle walking is longest just above a power of two),
# K1 going 1 → 2 at 4096 / 4097, K1 = 16 → 32 at 65536 / 65537 (a prime number of samples)
SIZES_ALL = {1: (1, 1), 2: (1, 2), 3: (3, 1), 4: (1, 4), 5: (5, 1), 7: (7, 1), 8: (1, 8), 9: (3, 3), 255: (15, 17), 256: (2, 128), 257: (257, 1),
             4095: (63, 65), 4096: (32, 128), 4097: (241, 17), 65535: (255, 257), 65536: (512, 128), 65537: (65537, 1)}
# blocked mode only: the 8192-sample scatter block at 8191 / 8192 / 8193, K1 = 2 → 4 at 8192 / 8193, 12289 (prime, one sample into the fourth
# bucket's expected share), K1 = 4 → 8 at 16384 / 16385
SIZES_BLOCKED = {8191: (8191, 1), 8192: (64, 128), 8193: (2731, 3), 12289: (12289, 1), 16384: (128, 128), 16385: (3277, 5)}
# the last bfy_l1_kernel<256> size with 128 steps, the first <1024> size, the last size whose second digit rides in the entry's top byte (sample
# indices with bit 23 set under a digit). update_epochs = 1: the scatter workspace is K1·5632 words per epoch.
SIZES_BIG = {(1 << 22) - 128: (32767, 128), 1 << 22: (32768, 128), 1 << 24: (131072, 128)}

SEEDS = (99, (0x9E37 << 32) | 0x79B9)                   # the second one has a non-zero high word
EPOCHS = (0, 5, (1 << 32) + 5)                          # the last one must not collide with 5
OFFSETS = (0, 3)                                        # env_id_offset: the data-parallel shard's first env
KEYS = [(s, o, e) for s in SEEDS for o in OFFSETS for e in EPOCHS]


def perm_cases():
    """(mode, n, nt, k) for the small sizes — one GPU case each, all KEYS inside — and (n, nt, k, seed, offset, epoch) for the big ones, a case per
    key (the reference takes 1.3 s at 2^24)."""
    small = [(mode, n, nt, k) for mode in (R.SERIAL, R.BIJECTION, R.BLOCKED) for n, (nt, k) in SIZES_ALL.items()]
    small += [(R.BLOCKED, n, nt, k) for n, (nt, k) in SIZES_BLOCKED.items()]
    big = [(n, nt, k) + key for n, (nt, k) in SIZES_BIG.items() for key in KEYS]
    return small, big


# ---------------------------------------------------------------------------------------------------------------- advantage families
def adv_integers(n, rng=None, hot=None):
    """a_i = ((i·2654435761) mod 4093) − 2046: |a| <= 2046, so every partial sum of a (< 2^36) and of a² (< 2^47) over n <= 2^24 samples is an
    integer below 2^53 — every summation order gives the same Float64 bits."""
    i = np.arange(n, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) % np.uint64(4093)).astype(np.int64) - 2046).astype(np.float32)


def adv_one_hot(n, rng=None, hot=0):
    a = np.zeros(n, np.float32); a[hot] = 1.0
    return a


def adv_normal(n, rng, hot=None):
    return (3 * rng.standard_normal(n) + 0.7).astype(np.float32)


def adv_constant(n, rng=None, hot=None):
    return np.full(n, 2.5, np.float32)


def adv_offset(n, rng, hot=None):
    return (100 + rng.standard_normal(n)).astype(np.float32)


FAMILIES = dict(integers=adv_integers, one_hot=adv_one_hot, normal=adv_normal, constant=adv_constant, offset=adv_offset)
EXACT_FAMILIES = ("integers", "one_hot", "constant")          # sums that no summation order can change
ORDER = ("integers", "normal", "one_hot", "constant", "offset")   # call i of a handle runs family ORDER[i] (its epochs: i·E … i·E + E − 1)

# ---------------------------------------------------------------------------------------------------------------- advantage-sum cases
# straddle: None (no claim), "mixed" (at least one L1 bucket crosses a minibatch boundary and, where K1 > 1, at least one does not) or "all"
# (M < 4096: every bucket crosses one, some cross two). `slot`: the perm slot a host-driven crl_shuffle draws into (2: after an iterate with 3 epochs).
Case = namedtuple("Case", "path mode nt k nmb epochs seq how route straddle slot")


def _c(path, mode, nt, k, nmb, how, route, epochs=1, seq=1, straddle=None, slot=0):
    return Case(path, mode, nt, k, nmb, epochs, seq, how, route, straddle, slot)


B = R.BLOCKED
ADV_CASES = [
    # ---- 4/2/64 path, crl_ppo_update: the vector stored-digit branch, nmb 1 / 2 / 4 / 8 (n % 4 == 0)
    _c("fused", B, 8, 128, 1, "update", "bucket<1>/stored-vec"),
    _c("fused", B, 88, 128, 2, "update", "bucket<2>/stored-vec", straddle="mixed"),                 # 11264 / 2: 1 of 4
    _c("fused", B, 8, 128, 4, "update", "bucket<4>/stored-vec", straddle="mixed"),                  # 1024 / 4: 1 of 1, across three boundaries
    _c("fused", B, 512, 128, 8, "update", "bucket<8>/stored-vec", straddle="mixed"),                # 65536 / 8: M = 8192
    _c("fused", B, 128, 128, 8, "update", "bucket<8>/stored-vec", straddle="all"),                  # 16384 / 8: 4 of 4, M = 2048
    _c("fused", B, 88, 128, 2, "update", "bucket<2>/stored-vec", epochs=3, straddle="mixed"),       # the last of three slots is read back
    _c("fused", B, 8, 128, 4, "update", "bucket<4>/stored-vec", epochs=3, straddle="mixed"),
    # ---- the scalar stored-digit branch (n % 4 != 0)
    _c("fused", B, 37, 65, 1, "update", "bucket<1>/stored-scalar"),                                 # 2405
    _c("fused", B, 241, 34, 2, "update", "bucket<2>/stored-scalar", straddle="mixed"),              # 8194 / 2: 1 of 4
    _c("fused", B, 241, 34, 2, "update", "bucket<2>/stored-scalar", epochs=3, straddle="mixed"),
    # ---- adv_seq = 2: the digit recomputed
    _c("fused", B, 88, 128, 2, "update", "bucket<2>/recomputed", seq=2, straddle="mixed"),
    _c("fused", B, 241, 34, 2, "update", "bucket<2>/recomputed", seq=2, epochs=3, straddle="mixed"),
    # ---- the gather: nmb not 1 / 2 / 4 / 8, adv_seq = 0, the other shuffle modes
    _c("fused", B, 132, 128, 3, "update", R.GATHER, straddle="mixed"),                              # 16896 / 3: 2 of 8
    _c("fused", B, 384, 128, 16, "update", R.GATHER, straddle="mixed"),                             # 49152 / 16: 15 of 16
    _c("fused", B, 88, 128, 2, "update", R.GATHER, seq=0, epochs=3, straddle="mixed"),
    _c("fused", R.SERIAL, 8, 128, 4, "update", R.GATHER, epochs=3),
    _c("fused", R.BIJECTION, 8, 128, 4, "update", R.GATHER, epochs=3),
    _c("fused", R.BIJECTION, 241, 17, 1, "update", R.GATHER),                                       # 4097: the longest cycle walks
    # ---- crl_ppo_iterate (the GAE's own advantages: the Float64 bar)
    _c("fused", B, 88, 128, 2, "iterate", "bucket<2>/stored-vec", epochs=3, straddle="mixed"),
    _c("fused", B, 241, 34, 2, "iterate", "bucket<2>/stored-scalar", straddle="mixed"),
    _c("fused", B, 132, 128, 3, "iterate", R.GATHER, straddle="mixed"),
    _c("fused", R.SERIAL, 8, 128, 4, "iterate", R.GATHER, epochs=3),
    _c("fused", R.BIJECTION, 8, 128, 4, "iterate", R.GATHER, epochs=3),
    # ---- host-driven: crl_shuffle + crl_adv_stats on a fresh handle (the tables are valid) ...
    _c("fused", B, 88, 128, 2, "shuffle", "bucket<2>/stored-vec", straddle="mixed"),
    _c("fused", B, 241, 34, 2, "shuffle", "bucket<2>/stored-scalar", straddle="mixed"),
    _c("fused", B, 88, 128, 2, "shuffle", "bucket<2>/recomputed", seq=2, straddle="mixed"),
    _c("fused", B, 132, 128, 3, "shuffle", R.GATHER, straddle="mixed"),
    # ---- ... after crl_ppo_write(CRL_F_PERM) dropped them, and into slot 2, where an iterate with three epochs left the handle
    _c("fused", B, 88, 128, 2, "write_perm", R.GATHER),
    _c("fused", B, 88, 128, 2, "shuffle", R.GATHER, epochs=3, slot=2, straddle="mixed"),
    # ---- layer-wise path (CRL_FORCE_WIDE = 1 on the 4/2/64 net): the leaf-fused sums from M >= 5632 ...
    _c("wide", B, 44, 128, 1, "update", R.LEAF),                                                    # 5632 · 1
    _c("wide", B, 88, 128, 2, "update", R.LEAF, straddle="mixed"),                                  # M = the bucket capacity
    _c("wide", B, 132, 128, 3, "update", R.LEAF, epochs=3, straddle="mixed"),
    _c("wide", B, 88, 128, 2, "iterate", R.LEAF, straddle="mixed"),
    _c("wide", B, 1877, 6, 2, "update", R.SUMS, straddle="mixed"),                                  # M = 5631: one short
    _c("wide", B, 88, 128, 2, "shuffle", R.SUMS, straddle="mixed"),                                 # crl_shuffle never fuses
    # ---- ... the inverse bijection at nmb = 4 only, the walk through the permutation otherwise
    _c("wide", R.BIJECTION, 8, 128, 4, "update", R.INV4, epochs=3),
    _c("wide", R.BIJECTION, 241, 17, 1, "update", R.SUMS),
    _c("wide", R.BIJECTION, 1028, 4, 4, "update", R.INV4),                                          # 4112 = 2^12 + 16: cycle walks in the inverse
    _c("wide", R.BIJECTION, 37, 64, 4, "shuffle", R.INV4),
    _c("wide", R.BIJECTION, 37, 64, 4, "write_perm", R.SUMS),
    _c("wide", R.BIJECTION, 8, 128, 2, "update", R.SUMS),
    _c("wide", R.BIJECTION, 8, 128, 8, "update", R.SUMS, epochs=3),
    _c("wide", R.SERIAL, 8, 128, 4, "update", R.SUMS, epochs=3),
]
del B

SEED = 99
HOST_EPOCH = 7                                            # the epoch id of the host-driven crl_shuffle calls


def case_id(c):
    return f"{c.path}-mode{c.mode}-{c.nt}x{c.k}-nmb{c.nmb}-e{c.epochs}-seq{c.seq}-{c.how}" + (f"-slot{c.slot}" if c.slot else "")


def last_epoch(c, call=0):
    """The epoch id whose permutation the handle's current slot holds after call number `call` (0-based) of the case."""
    if c.how in ("iterate", "update"):
        return call * c.epochs + c.epochs - 1
    return HOST_EPOCH + call


def straddle_count(c, call=0, seed=SEED):
    """(buckets crossing a minibatch boundary, the most minibatches one bucket touches, non-empty buckets) of the case's blocked permutation."""
    n = c.nt * c.k
    dg = R.bfy_digits(n, seed, last_epoch(c, call))
    M = n // c.nmb
    s = R.straddlers(dg.off, M)
    span = max(((hi - 1) // M - lo // M + 1) for lo, hi in dg.ranges if hi > lo)
    return len(s), span, sum(1 for lo, hi in dg.ranges if hi > lo)


def load_trace():
    with open(TRACE) as f:
        return json.load(f)
