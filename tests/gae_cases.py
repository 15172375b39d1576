"""The GAE launch rule restated, the table of shapes that reach every kernel it can launch, and the input families.

csrc/gae.hip:launch_gae compiles 50 kernels — gae_kernel<EB, L, NTL> and gae_seg2_kernel<EB, L, NTL> for EB 8 / 16 / 32 / 64, L 8 / 16, and
gae_stream_kernel<E, D, NTL> for E 1 / 2 / 4, D 4 / 8 / 16, each with cached or nontemporal loads — and one rule with several silent fallbacks picks
among them. `route` is that rule as integers; GEOMETRY holds, per kernel, the smallest shape that reaches it, then the ragged edges, the horizon
(num_steps = 1024), both L 8 → 16 fallbacks and the error rows; FAMILIES are the input distributions; CASES crosses the rows with both load flavours and
both modes and deals the families round so that every family meets every kernel family at L / D = 8 and 16. tests/test_gae_cpu.py holds the table to
those purposes; tests/test_gpu_gae_edges.py runs it."""
import json
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "gae_edges.json")
WRITE = os.environ.get("CRL_WRITE_PROFILES") == "1"


def write_profile(section, rec):
    """Merge one section's entries into profiles/gae_edges.json (the tests call this only under CRL_WRITE_PROFILES=1)."""
    allrec = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as f:
            allrec = json.load(f)
    allrec.setdefault(section, {}).update(rec)
    with open(PROFILE, "w") as f:
        json.dump(allrec, f, indent=1, sort_keys=True)
        f.write("\n")


ERR_EMPTY = "gae: empty input"
ERR_STREAM = "gae: the streaming kernel (gae_tile = 4 / 2 / 1) needs num_envs % gae_tile == 0"
ERR_PAIR = "gae: gae_tile = 128 / 256 (two envs per thread) needs an even num_envs"
ERR_STEPS = "gae: num_steps > 1024 is not supported"
ERR_TILE = "gae: unsupported tile configuration"

SEGS = (0, 4, 8, 16)                                   # what crl_ppo_set_option accepts for gae_seg ...
TILES = (0, 1, 2, 4, 8, 16, 32, 64, 128, 256)          # ... and for gae_tile
COMPILED = ({("one", eb, l) for eb in (8, 16, 32, 64) for l in (8, 16)} | {("pair", eb, l) for eb in (8, 16, 32, 64) for l in (8, 16)} |
            {("stream", e, d) for e in (1, 2, 4) for d in (4, 8, 16)})
KERNELS = {r + (ntl,) for r in COMPILED for ntl in (0, 1)}      # the 50


def route(nt, k, seg, tile, aligned=True):
    """launch_gae's choice: ("stream", E, D), ("pair", EB, L), ("one", EB, L), or the error text. `aligned`: the buffers' addresses are multiples of
    16 bytes (4 for the flags), as every buffer of the library and of crl_gae is; what remains of the alignment rule is num_envs % E."""
    if nt <= 0 or k <= 0:
        return ERR_EMPTY

    def al(E):
        return aligned and nt % E == 0
    forced = tile in (1, 2, 4)
    if forced and not al(tile):
        return ERR_STREAM
    samples = nt * k
    auto_E = 4 if samples >= 1 << 26 else 2
    automatic = tile == 0 and al(auto_E) and samples >= 1 << 25 and nt >= 262144
    if forced or automatic:
        return ("stream", tile if forced else auto_E, seg if seg in (4, 8, 16) else (8 if forced else 4))
    if tile in (128, 256) and not al(2):
        return ERR_PAIR
    if tile in (128, 256) or (tile == 0 and nt >= 4096 and k <= 128 and al(2)):
        L = seg if seg in (8, 16) else (8 if k <= 128 else 16)
        S = (k + L - 1) // L
        EB = 64 if tile == 256 else 32
        while EB > 8 and S * EB > 512:
            EB >>= 1
        if S * EB > 512 and L == 8:
            L = 16; S = (k + L - 1) // L
        if S * EB > 512:
            return ERR_STEPS
        return ("pair", EB, L)
    L = (0 if seg == 4 else seg) or (8 if k <= 256 else 16)
    S = (k + L - 1) // L
    EB = tile or 64
    while EB > 8 and (S * EB > 512 or (nt + EB - 1) // EB < 1024):
        EB >>= 1
    if S * EB > 512 and L == 8:
        L = 16; S = (k + L - 1) // L
    if S * EB > 512:
        return ERR_STEPS
    if EB not in (8, 16, 32, 64) or L not in (8, 16):
        return ERR_TILE
    return ("one", EB, L)


def block_threads(r, k):
    """Threads per block of a routed launch."""
    return 256 if r[0] == "stream" else ((k + r[2] - 1) // r[2]) * r[1]


def envs_per_block(r):
    return {"stream": 256 * r[1], "pair": 2 * r[1], "one": r[1]}[r[0]]


Row = namedtuple("Row", "nt k seg tile why")
# ---- one row per compiled (family, EB / E, L / D); with nt_loads 0 and 1 these reach the 50 kernels. k = L + 1 where the shape is free: two segments,
# so the fold runs, and the second one is almost all padding. The one-env kernel halves EB until there are 1024 blocks, a forced gae_tile included:
# EB = 16 / 32 / 64 need 16369 / 32737 / 65473 envs (odd counts: 1024 blocks, the last with ONE env). The pair kernel's EB depends on S alone.
GEOMETRY = [
    Row(3, 9, 0, 8, "one<8,8>"), Row(3, 17, 16, 8, "one<8,16>"),
    Row(16369, 9, 0, 16, "one<16,8>"), Row(16369, 17, 16, 16, "one<16,16>"),
    Row(32737, 9, 0, 32, "one<32,8>"), Row(32737, 17, 16, 32, "one<32,16>"),
    Row(65473, 9, 0, 64, "one<64,8>"), Row(65473, 17, 16, 64, "one<64,16>"),
    Row(130, 9, 0, 256, "pair<64,8>"), Row(130, 17, 16, 256, "pair<64,16>"),
    Row(66, 9, 0, 128, "pair<32,8>"), Row(66, 17, 16, 128, "pair<32,16>"),
    Row(34, 129, 8, 128, "pair<16,8>: seg = 8 forced at k = 129..256"), Row(34, 257, 0, 128, "pair<16,16>"),
    Row(18, 257, 8, 128, "pair<8,8>: seg = 8 forced at k = 257..512"), Row(18, 513, 0, 128, "pair<8,16>"),
]
GEOMETRY += [Row(257 * E, 2 * D + 1, D, E, f"stream<{E},{D}>: nt = 256·E + E") for E in (1, 2, 4) for D in (4, 8, 16)]
GEOMETRY += [
    # ---- ragged edges: k = 1, L, L + 1 (above), S·L − 1; nt = E; the automatic gates
    Row(3, 1, 0, 8, "one, k = 1"), Row(3, 8, 0, 8, "one, k = L"), Row(3, 23, 0, 8, "one, k = S·L − 1"),
    Row(3, 16, 16, 8, "one, k = L = 16"), Row(3, 47, 16, 8, "one, k = S·L − 1, L = 16"),
    Row(6, 1, 0, 128, "pair, k = 1"), Row(6, 8, 0, 128, "pair, k = L"), Row(6, 23, 0, 128, "pair, k = S·L − 1"),
    Row(6, 16, 16, 128, "pair, k = L = 16"), Row(6, 47, 16, 128, "pair, k = S·L − 1, L = 16"),
    Row(1, 5, 0, 1, "stream, nt = E = 1"), Row(2, 5, 0, 2, "stream, nt = E = 2"), Row(4, 5, 0, 4, "stream, nt = E = 4"), Row(4, 1, 0, 4, "stream, k = 1"),
    Row(4096, 9, 0, 0, "automatic: the pair kernel from 4096 even envs at k <= 128"), Row(4098, 129, 0, 0, "automatic: k = 129 stays with the one-env kernel"),
    Row(4097, 9, 0, 0, "automatic: an odd num_envs stays with the one-env kernel"),
    # ---- the horizon and the L 8 → 16 fallbacks
    Row(5, 1024, 0, 0, "one, k = 1024: S = 64 at L = 16"), Row(6, 1024, 0, 128, "pair, k = 1024: 64 doubles of δ / c per thread at S = 64"),
    Row(8, 1024, 0, 4, "stream, k = 1024"),
    Row(5, 600, 8, 0, "one, seg = 8 at k > 512 falls back to L = 16"), Row(6, 600, 8, 128, "pair, seg = 8 at k > 512 falls back to L = 16"),
    Row(1, 1500, 0, 1, "stream, k = 1500: no limit"), Row(2, 1500, 0, 2, "stream, k = 1500: no limit"), Row(4, 1500, 0, 4, "stream, k = 1500: no limit"),
]
ERROR_ROWS = [
    (Row(5, 1025, 0, 0, "one, k = 1025"), ERR_STEPS), (Row(5, 1025, 8, 8, "one, k = 1025, seg = 8"), ERR_STEPS), (Row(6, 1025, 0, 128, "pair, k = 1025"), ERR_STEPS),
    (Row(6, 1025, 8, 256, "pair, k = 1025, seg = 8"), ERR_STEPS), (Row(6, 4, 0, 4, "stream, nt % 4"), ERR_STREAM), (Row(7, 4, 0, 128, "pair, nt odd"), ERR_PAIR),
]

# ---------------------------------------------------------------------------------------------------------------------------------------------
# input families: gen(nt, k, seed) → dict(value, reward, term, nv, nd, gamma, lam); every env has data of its own, so a lane mix-up shows
# ---------------------------------------------------------------------------------------------------------------------------------------------
FLAG_BYTES = np.array([1, 2, 0x80, 0xFF], np.uint8)


def _base(nt, k, seed, p_term=0.02):
    rng = np.random.default_rng(seed)
    value = rng.standard_normal((nt, k), dtype=np.float32) * 10
    reward = (rng.random((nt, k), dtype=np.float32) > 0.02).astype(np.float32)
    term = (rng.random((nt, k), dtype=np.float32) < p_term).astype(np.uint8)
    nv = (rng.standard_normal(nt) * 10).astype(np.float32); nd = (rng.random(nt) < 0.3).astype(np.uint8)
    return dict(value=value, reward=reward, term=term, nv=nv, nd=nd, gamma=0.99, lam=0.95), rng


def standard(nt, k, seed):
    return _base(nt, k, seed)[0]


def no_terminal_unit(nt, k, seed):
    d = _base(nt, k, seed)[0]
    d["term"][:] = 0; d["nd"][:] = 0; d["gamma"] = 1.0; d["lam"] = 1.0        # C ≡ 1: the carry crosses the whole rollout
    return d


def all_terminal(nt, k, seed):
    d = _base(nt, k, seed)[0]
    d["term"][:] = 1; d["nd"][:] = 1
    return d


def boundary_terminals(nt, k, seed):
    """Env e takes pattern e % 8 of: flags at every t = 8s − 1 | 8s | 8s + 1 | 16s − 1 | 16s | 16s + 1 | only t = 0 | only t = k − 1; next_done on every other
    env of each pattern."""
    d = _base(nt, k, seed)[0]
    e = np.arange(nt)[:, None]; t = np.arange(k)[None, :]
    p = e % 8
    d["term"] = (((p == 0) & (t % 8 == 7)) | ((p == 1) & (t % 8 == 0)) | ((p == 2) & (t % 8 == 1)) | ((p == 3) & (t % 16 == 15)) | ((p == 4) & (t % 16 == 0)) |
                 ((p == 5) & (t % 16 == 1)) | ((p == 6) & (t == 0)) | ((p == 7) & (t == k - 1))).astype(np.uint8)
    d["nd"] = ((np.arange(nt) + np.arange(nt) // 8) % 2).astype(np.uint8)
    return d


def flag_bytes(nt, k, seed):
    """Terminal bytes from {0, 1, 2, 0x80, 0xFF}. Column t (next_done is column k) of the aligned quad q of envs runs through 16 phases, (t + q) % 16:
    0..3: lane `phase` of the quad alone is non-zero (so is one byte of one aligned pair, in either position, while the other pair is clear);
    4: all clear; 5: all set; 6, 7: drawn per env; 8..15: clear, so that carries still travel. Which non-zero byte: (7t + 3e) % 4 → 1 / 2 / 0x80 / 0xFF."""
    d, rng = _base(nt, k, seed)
    e = np.arange(nt)[:, None]; t = np.arange(k + 1)[None, :]
    ph = (t + e // 4) % 16
    nz = ((ph < 4) & (e % 4 == ph)) | (ph == 5) | (((ph == 6) | (ph == 7)) & (rng.random((nt, k + 1)) < 0.5))
    f = np.where(nz, FLAG_BYTES[(7 * t + 3 * e) % 4], 0).astype(np.uint8)
    d["term"] = np.ascontiguousarray(f[:, :k]); d["nd"] = np.ascontiguousarray(f[:, k])
    return d


def gamma0(nt, k, seed):
    d = _base(nt, k, seed)[0]; d["gamma"] = 0.0
    return d


def lambda0(nt, k, seed):
    d = _base(nt, k, seed)[0]; d["lam"] = 0.0
    return d


def magnitudes(nt, k, seed):
    """Env e % 4: values and rewards of 1e30 | of 1e-30 | Float32 denormals (integers below 2^20 times 2^-149) | ordinary values with −0.0 rewards.
    Every output stays finite: inputs are clipped to 4e30, so |A| <= S <= 1.2e31 / (1 − 0.9405) = 2e32 < 3.4e38."""
    d, rng = _base(nt, k, seed)
    kind = np.arange(nt) % 4
    g = rng.standard_normal((nt, k + 1)); rw = rng.standard_normal((nt, k))
    den = np.float64(2.0 ** -149)
    v = np.where(kind[:, None] == 0, g * 1e30, np.where(kind[:, None] == 1, g * 1e-30, np.where(kind[:, None] == 2, np.rint(g * 2 ** 18) * den, g * 10)))
    r = np.where(kind[:, None] == 0, rw * 1e30, np.where(kind[:, None] == 1, rw * 1e-30, np.where(kind[:, None] == 2, np.rint(rw * 2 ** 18) * den, -0.0)))
    v = np.clip(v, -4e30, 4e30); r = np.clip(r, -4e30, 4e30)
    d["value"] = v[:, :k].astype(np.float32); d["nv"] = v[:, k].astype(np.float32); d["reward"] = r.astype(np.float32)
    return d


def cancellation(nt, k, seed):
    """Constant values of 1e6 (a constant of its own per env), rewards of 1e-3, γ = λ = 1, no terminals, fixed mode: every delta is the 1e-3 left over from
    1e6 − 1e6, so the outputs are small against the scale S and the derived interval holds many Float32 values (the one family outside the sharpness cap)."""
    e = np.arange(nt)
    c = (1e6 + 0.0625 + 64.0625 * (e % 997)).astype(np.float32)       # sixteenths: 1e-3 + 1e6 does not fit Float64 exactly
    return dict(value=np.repeat(c[:, None], k, axis=1), reward=np.repeat((1e-3 * (1 + e % 7)).astype(np.float32)[:, None], k, axis=1),
                term=np.zeros((nt, k), np.uint8), nv=c.copy(), nd=np.zeros(nt, np.uint8), gamma=1.0, lam=1.0)


FAMILIES = dict(standard=standard, no_terminal_unit=no_terminal_unit, all_terminal=all_terminal, boundary_terminals=boundary_terminals, flag_bytes=flag_bytes,
                gamma0=gamma0, lambda0=lambda0, magnitudes=magnitudes, cancellation=cancellation)
FIXED_ONLY = ("cancellation",)


def inputs(family, nt, k):
    """The family's inputs at a shape, seeded by the shape and the family."""
    return FAMILIES[family](nt, k, (nt * 4099 + k) * 16 + list(FAMILIES).index(family))


def args(d, mode):
    return (d["value"], d["reward"], d["term"], d["nv"], d["nd"], d["gamma"], d["lam"], mode)


def group(r):
    """(kernel family, L or D) — what the families are dealt over."""
    return (r[0], r[2])


Case = namedtuple("Case", "row ntl mode family route")


def _cases():
    out, dealt, held = [], {}, {}
    names = list(FAMILIES)
    for row in GEOMETRY:
        r = route(row.nt, row.k, row.seg, row.tile)
        for ntl in (0, 1):
            for mode in (0, 1):
                g = group(r)
                if mode == 1 and held.get(g):                # a fixed-mode-only family that came up at a compat case waits for the group's next fixed one
                    out.append(Case(row, ntl, mode, held.pop(g), r))
                    continue
                fam = names[dealt.get(g, 0) % len(names)]; dealt[g] = dealt.get(g, 0) + 1
                if fam in FIXED_ONLY and mode == 0:
                    held[g] = fam
                    fam = names[dealt[g] % len(names)]; dealt[g] += 1
                out.append(Case(row, ntl, mode, fam, r))
    return out


CASES = _cases()


def case_id(c):
    return f"{c.route[0]}{c.route[1]}x{c.route[2]}-{c.row.nt}x{c.row.k}-seg{c.row.seg}-tile{c.row.tile}-ntl{c.ntl}-mode{c.mode}-{c.family}"


def exact_envs(nt, r):
    """Up to 16 envs for the exact reference: the first, the last, and both sides of the first and the last block edge."""
    eb = envs_per_block(r)
    last_edge = ((nt - 1) // eb) * eb
    pick = [0, 1, 2, 3, eb - 2, eb - 1, eb, eb + 1, last_edge - 2, last_edge - 1, last_edge, last_edge + 1, nt - 4, nt - 3, nt - 2, nt - 1]
    return sorted({e for e in pick if 0 <= e < nt})[:16]
