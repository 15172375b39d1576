"""The epoch permutation and the per-minibatch advantage sums, restated in numpy and Python integers: the yardstick of tests/test_shuffle_cpu.py and
tests/test_gpu_shuffle_edges.py. Written from csrc/bijection.hpp, csrc/shuffle.hip, the launch rules of csrc/records.hip / csrc/optim.hip / csrc/api.cpp
and ppo.jl:191-194,221 — integer arithmetic on 32-bit words held in uint64, so nothing here can round. Philox is ddpg_ref.philox.

  shuffle_seed                              the handle's key rule (ppo_ctx.hpp)
  bij_bits / bij_key / bij_forward / bij_inverse / inv_odd     CRL_SHUFFLE_BIJECTION
  fy_serial                                 CRL_SHUFFLE_FISHER_YATES (Random.shuffle!: for i = n:-1:2, swap with rand(1:i))
  bfy_digits / blocked_fy                   CRL_SHUFFLE_BLOCKED_FY: the two digits, the L1 bucket layout, the whole permutation
  minibatch_of / straddlers / exact_sums    Σadv, Σadv² per minibatch, exact
  stats_exact / std_bar / sum_bar           adv_finish_kernel in rationals, and the derived error bars
  adv_route                                 which kernel, and which branch of it, produces the sums of a call

`mutant=` switches on one deliberate mistake; tests/test_shuffle_cpu.py shows that the check owning each of them fails."""
import math
from collections import namedtuple
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

from ddpg_ref import philox

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
U = 2.0 ** -53
BFY_L1, BFY_CAP = 4096, 5632
SERIAL, BIJECTION, BLOCKED = 0, 1, 2


def shuffle_seed(seed, env_id_offset=0):
    """seed + 0x9E3779B97F4A7C15 · uint32(env_id_offset), wrapping at 2^64."""
    return (seed + 0x9E3779B97F4A7C15 * (env_id_offset & M32)) & M64


def _u64(v):
    return np.uint64(v & M64)


def _mulhi(hi, lo, m):
    """High 64 bits of ((hi << 32) | lo) · m for 32-bit words hi, lo and m < 2^32 (uint64 arrays): no intermediate passes 2^64."""
    return (hi * m + ((lo * m) >> np.uint64(32))) >> np.uint64(32)


# ---------------------------------------------------------------------------------------------------------------- keyed bijection
def bij_bits(n):
    bits = 1
    while (1 << bits) < n:
        bits += 1
    return bits


def inv_odd(a):
    """a · inv ≡ 1 (mod 2^32) for odd a: five Newton steps from x = a (three correct bits double each time)."""
    x = a & M32
    for _ in range(5):
        x = (x * ((2 - a * x) & M32)) & M32
    return x


BijKey = namedtuple("BijKey", "k inv mask bits")


def bij_key(n, seed, epoch):
    x, y, z, w = (int(v[0]) for v in philox(np.array([0x51]), epoch & M32, (epoch >> 32) & M32, 0xB1D, seed & M32, (seed >> 32) & M32))
    k = (x, y, z, w, y ^ 0xA5A5A5A5, x ^ 0x3C3C3C3C)
    bits = bij_bits(n)
    return BijKey(k, (inv_odd(k[1] | 1), inv_odd(k[3] | 1), inv_odd(k[5] | 1)), (1 << bits) - 1, bits)


def _round(x, key, k0, k1):
    mask, bits = np.uint64(key.mask), key.bits
    x = (x + np.uint64(k0)) & mask
    x = (x * np.uint64(k1 | 1)) & mask
    x = x ^ (x >> np.uint64((bits + 1) >> 1))
    x = (x * np.uint64(0x9E3779B1)) & mask
    x = x ^ (x >> np.uint64((bits + 2) // 3))
    return x & mask


def _unxorshift(x, s, bits):
    sh = s
    while sh < bits:
        x = x ^ (x >> np.uint64(sh))
        sh <<= 1
    return x


def _round_inv(x, key, k0, k1inv):
    mask, bits = np.uint64(key.mask), key.bits
    x = _unxorshift(x, (bits + 2) // 3, bits)
    x = (x * np.uint64(0x0E8B2F51)) & mask
    x = _unxorshift(x, (bits + 1) >> 1, bits)
    x = (x * np.uint64(k1inv)) & mask
    return (x + _u64(-k0)) & mask


def _walk(step, x, n):
    """Apply `step` until the word is below n (cycle walking), element by element. Returns the words and the longest walk."""
    x = x.copy()
    idx = np.arange(x.size)
    rounds = 0
    while idx.size:
        x[idx] = step(x[idx])
        idx = idx[x[idx] >= np.uint64(n)]
        rounds += 1
    return x, rounds


def bij_forward(n, seed, epoch, p=None, mutant=None, want_rounds=False):
    """perm[p] = π_key(p) for p in [0, n) (or the given positions), int64."""
    key = bij_key(n, seed, epoch)
    k = key.k
    p = np.arange(n, dtype=np.uint64) if p is None else np.asarray(p, np.uint64)

    def step(x):
        return _round(_round(_round(x, key, k[0], k[1]), key, k[2], k[3]), key, k[4], k[5])
    if mutant == "mod_n":                       # no cycle walking: fold the word into range instead
        return (step(p) % np.uint64(n)).astype(np.int64)
    x, rounds = _walk(step, p, n)
    return (x.astype(np.int64), rounds) if want_rounds else x.astype(np.int64)


def bij_inverse(n, seed, epoch, x=None, mutant=None):
    """The position p with π_key(p) = x, for x in [0, n) (or the given samples), int64."""
    key = bij_key(n, seed, epoch)
    k, inv = key.k, key.inv
    x = np.arange(n, dtype=np.uint64) if x is None else np.asarray(x, np.uint64)
    order = ((k[4], inv[2]), (k[2], inv[1]), (k[0], inv[0]))
    if mutant == "swap_round_keys":             # the keys of the last two forward rounds undone in the wrong order
        order = (order[1], order[0], order[2])

    def step(v):
        for k0, ki in order:
            v = _round_inv(v, key, k0, ki)
        return v
    return _walk(step, x, n)[0].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- serial Fisher–Yates
def fy_serial(perm, seed, epoch, mutant=None):
    """Shuffles `perm` (a copy) like fy_serial_kernel: for i = n − 1 … 1, j = ⌊r·(i + 1) / 2^64⌋ from Philox(i; epoch; 0x5FF; seed), swap."""
    perm = np.array(perm, np.int64)
    n = perm.size
    i = np.arange(n, dtype=np.uint64)
    x, y, _, _ = philox(i, epoch & M32, (epoch >> 32) & M32, 0x5FF, seed & M32, (seed >> 32) & M32)
    j = _mulhi(x, y, i if mutant == "draw_below_i" else i + np.uint64(1))          # the mutant draws from 0 … i − 1 (Sattolo: cycles only)
    j = j.astype(np.int64)
    for a in range(n - 1, 0, -1):
        b = j[a]
        perm[a], perm[b] = perm[b], perm[a]
    return perm


# ---------------------------------------------------------------------------------------------------------------- blocked Fisher–Yates
Digits = namedtuple("Digits", "K1 d1 d2 off ranges")


def bfy_k1(n):
    K1 = 1
    while K1 * BFY_L1 < n:
        K1 *= 2
    return K1


def bfy_digits(n, seed, epoch, mutant=None):
    """Every sample's two digits (d1 < K1 its L1 bucket, d2 < 256 its sub-bucket), the buckets' offsets (K1 + 1, an exclusive scan of their sizes)
    and the half-open position range of every bucket."""
    K1 = bfy_k1(n)
    x, y, _, _ = philox(np.arange(n, dtype=np.uint64), epoch & M32, (epoch >> 32) & M32, 0xB0C, seed & M32, (seed >> 32) & M32)
    if mutant == "swap_digits":
        x, y = y, x
    d1 = (x & np.uint64(K1 - 1)).astype(np.int64); d2 = (y & np.uint64(255)).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(np.bincount(d1, minlength=K1)))).astype(np.int64)
    return Digits(K1, d1, d2, off, [(int(off[b]), int(off[b + 1])) for b in range(K1)])


def blocked_fy(n, seed, epoch, mutant=None):
    """The whole permutation: sub-buckets in (d1, d2) order, each in ascending sample order, then Fisher–Yates inside each with the draws
    Philox(d1·256 + d2, j; epoch ^ constants; seed)."""
    dg = bfy_digits(n, seed, epoch, mutant)
    gid = dg.d1 * 256 + dg.d2
    i = np.arange(n, dtype=np.int64)
    perm = np.lexsort((-i if mutant == "unsorted" else i, gid)).astype(np.int64)      # the mutant leaves each sub-bucket in descending order
    G = dg.K1 * 256
    cnt = np.bincount(gid, minlength=G)
    off = np.concatenate(([0], np.cumsum(cnt)))[:G]
    e0 = (epoch & M32) ^ 0x9E3779B9; e1 = ((epoch >> 32) & M32) ^ 0xF15A7E5
    for j in range(int(cnt.max()) - 1, 0, -1):
        g = np.nonzero(cnt > j)[0]
        x, y, _, _ = philox(g.astype(np.uint64), j, e0, e1, seed & M32, (seed >> 32) & M32)
        t = _mulhi(x, y, np.uint64(j + 1)).astype(np.int64)
        a, b = off[g] + j, off[g] + t
        perm[a], perm[b] = perm[b].copy(), perm[a].copy()
    return perm


# ---------------------------------------------------------------------------------------------------------------- minibatches and sums
def straddlers(off, M):
    """The non-empty L1 buckets whose positions [off[b], off[b + 1]) cross a multiple of M."""
    return [b for b in range(len(off) - 1) if off[b + 1] > off[b] and off[b + 1] > (off[b] // M + 1) * M]


def minibatch_of(perm, M, off=None, mutant=None):
    """mb[s] = the minibatch sample s fell into: its position in perm divided by M."""
    perm = np.asarray(perm, np.int64)
    mb = np.empty(perm.size, np.int64)
    mb[perm] = np.arange(perm.size) // M
    if mutant == "straddle_first":              # every member of a straddling bucket counted in the bucket's first minibatch
        for b in straddlers(off, M):
            mb[perm[off[b]:off[b + 1]]] = off[b] // M
    return mb


def is_integral(adv):
    a = np.asarray(adv, np.float64)
    return bool(np.all(a == np.rint(a)) and np.all(np.abs(a) < 2 ** 26))


def exact_sums(adv, perm, nmb, mb=None):
    """[(Σa, Σa²)] per minibatch: exact Python integers when adv is integer-valued, else math.fsum of the Float64 values (a·a is exact in Float64
    for a Float32 a), i.e. the correctly rounded sums. `mb` overrides the assignment (the mutants)."""
    flat = np.asarray(adv, np.float32).reshape(-1, order="F").astype(np.float64)
    n = flat.size
    mb = minibatch_of(perm, n // nmb) if mb is None else mb
    out = []
    integral = is_integral(flat)
    for m in range(nmb):
        a = flat[mb == m]
        if integral:
            v = [int(t) for t in a]
            out.append((sum(v), sum(t * t for t in v)))
        else:
            out.append((math.fsum(a), math.fsum(a * a)))
    return out


def abs_sums(adv, perm, nmb):
    """[(Σ|a|, Σa²)] per minibatch (fsum): the scale of sum_bar."""
    flat = np.asarray(adv, np.float32).reshape(-1, order="F").astype(np.float64)
    mb = minibatch_of(perm, flat.size // nmb)
    return [(math.fsum(np.abs(flat[mb == m])), math.fsum(flat[mb == m] ** 2)) for m in range(nmb)]


def sum_bar(M, scale):
    """|fl(Σ x_i) − Σ x_i| <= γ_{M−1} · Σ|x_i| for M Float64 terms added in ANY order (Higham, Accuracy and Stability, eq. 4.4), γ_k = k·u / (1 − k·u),
    u = 2^-53. The terms themselves are exact: a Float32 widens exactly and its square has 48 bits."""
    k = (M - 1) * U
    return k / (1.0 - k) * scale


def _sqrt_fraction(q):
    """sqrt of a non-negative Fraction to 60 digits, then rounded to Float64."""
    with localcontext() as ctx:
        ctx.prec = 60
        return float((Decimal(q.numerator) / Decimal(q.denominator)).sqrt())


Stats = namedtuple("Stats", "mean var mean64 mean32 std64 std32")


def stats_exact(S1, S2, n):
    """adv_finish_kernel in rationals: mean = S1 / n, var = (S2 − n·mean²) / (n − 1) clamped at 0, and the two Float32 roundings the kernel ends with:
    mean32 = Float32(Float64(mean)) — one IEEE division, one conversion, so the device must give exactly this — and std32 = Float32(Float64(sqrt(var)))."""
    S1, S2 = Fraction(S1), Fraction(S2)
    mean = S1 / n
    var = (S2 - n * mean * mean) / (n - 1)
    var = var if var > 0 else Fraction(0)
    mean64 = float(mean); std64 = _sqrt_fraction(var)
    return Stats(mean, var, mean64, np.float32(mean64), std64, np.float32(std64))


def std_bar(S2, n, st):
    """How far adv_finish_kernel's Float32 std may lie from sqrt(var) when its input sums are taken as exact (see the docstring of
    tests/test_gpu_shuffle_edges.py for the derivation): e64 = min(E / σ, sqrt(E)) + 2u·σ with E = (6u·S2 + 3u·(n − 1)·var) / (n − 1), then one Float32
    rounding, 2^-24·(σ + e64) + 2^-150."""
    var = float(st.var); sd = st.std64
    E = (6 * U * float(S2) + 3 * U * (n - 1) * var) / (n - 1)
    e64 = min(E / sd if sd > 0 else math.inf, math.sqrt(E)) + 2 * U * sd
    return e64 + 2.0 ** -24 * (sd + e64) + 2.0 ** -150


# ---------------------------------------------------------------------------------------------------------------- which kernel sums
GATHER, SUMS, INV4, LEAF = "gather", "sums", "inv<4>", "leaf"
ROUTES = ({GATHER, SUMS, INV4, LEAF} | {f"bucket<{m}>/{br}" for m in (1, 2, 4, 8) for br in ("stored-vec", "stored-scalar", "recomputed")})
# the kernel a route's sums come from (bfy_leaf_kernel: its fused tail; nothing but the fold follows it)
ROUTE_KERNEL = {GATHER: "adv_gather_sums_kernel", SUMS: "adv_sums_kernel", INV4: "adv_sums_inv_kernel<4>", LEAF: "bfy_leaf_kernel"}
ROUTE_KERNEL.update({r: "adv_bucket_sums_kernel<%s>" % r[7] for r in ROUTES if r.startswith("bucket")})
HOWS = ("iterate", "update", "shuffle", "write_perm")


def adv_route(path, shuffle_mode, n, nmb, adv_seq, how, slot=0):
    """The kernel (and the branch inside it) that leaves Σadv, Σadv² of the current slot.
    path: "fused" (the 4/2/64 kernels) or "wide" (layer-wise). how: "iterate" / "update" (crl_ppo_iterate / crl_ppo_update draw the permutations
    themselves), "shuffle" (host-driven crl_shuffle + crl_adv_stats into perm slot `slot`), "write_perm" (the same after crl_ppo_write(CRL_F_PERM)).
    Restates launch_slot_adv_sums + launch_adv_bucket_sums + the `tables` condition of launch_blocked_fy for the fused path, and launch_adv_stats_sums +
    the `fuse` condition for the layer-wise path."""
    assert path in ("fused", "wide") and how in HOWS and n % nmb == 0
    M = n // nmb
    own = how in ("iterate", "update")                    # the library drew the permutation(s) of this call itself
    if path == "wide":
        # iterate_once: launch_shuffle(with_adv_sums = true) per epoch; crl_shuffle passes false; a written permutation clears both fast paths
        if shuffle_mode == BLOCKED and own and M >= BFY_CAP and nmb <= 256:
            return LEAF
        if shuffle_mode == BIJECTION and how != "write_perm" and nmb == 4:
            return INV4
        return SUMS
    if adv_seq == 0 or shuffle_mode != BLOCKED:
        return GATHER
    # the bucket tables exist for slots [0, nslots) of a draw that started at slot 0 (iterate: all epochs at once; crl_shuffle: the current slot alone)
    tables = nmb <= 255 and (own or (how == "shuffle" and slot == 0))
    if not tables or nmb not in (1, 2, 4, 8):
        return GATHER
    if adv_seq == 1:
        return f"bucket<{nmb}>/" + ("stored-vec" if n % 4 == 0 else "stored-scalar")
    return f"bucket<{nmb}>/recomputed"
