"""The yardsticks of tests/test_gpu_gae_edges.py, without a GPU: tests/gae_ref.py's Float64 recurrence is the project's C oracle bit for bit and lies, like the
restated segmented scan, inside the derived bound of the exact rational recurrence; tests/gae_cases.py's restated launch rule reaches all 50 compiled
kernels from its table and never leaves the compiled set; the derived interval is sharp (it holds at most two adjacent Float32 values for all but 1 % of the
outputs of every family but `cancellation`); and each restated piece, broken on purpose, falls outside it on some case of the table.
With CRL_WRITE_PROFILES=1 the share of the bound that the references use and the share of wide intervals go to profiles/gae_edges.json ("cpu_worst_error_over_bound",
"cpu_share_of_intervals_wider_than_two_floats")."""
from fractions import Fraction

import numpy as np
import pytest

import gae_cases as G
import gae_ref as R
import oraclelib as O

WRITE, write_profile = G.WRITE, G.write_profile
SMALL = 20000                                    # samples: rows up to here meet every family on the CPU, larger ones the family the table deals them


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_serial64_cast_to_float32_is_the_c_oracle_bit_for_bit(family, mode):
    for nt, k in ((5, 1), (33, 17), (6, 300)):
        d = G.inputs(family, nt, k)
        adv_o, ret_o = O.gae_batch(d["value"], d["reward"], d["term"], d["nv"], d["nd"], d["gamma"], d["lam"], mode)
        a32 = R.serial64(*G.args(d, mode)).astype(np.float32)
        assert np.array_equal(a32.view(np.uint32), adv_o.view(np.uint32)), (family, nt, k)
        assert np.array_equal((a32 + d["value"]).view(np.uint32), ret_o.view(np.uint32)), (family, nt, k)


def test_exact_agrees_with_the_hand_derived_vectors():
    """tests/test_gpu_parity.py::test_gae_single_env_api_and_edges' known answers, and rn32 on ties and denormals."""
    v = [1, 2, 3, 4]; r = [1, 1, 1, 1]; t = [0, 0, 1, 0]
    assert [float(x) for x in R.exact(v, r, t, 5.0, 0, 0.5, 0.5, 0)] == [0.75, -1.0, 0.0, 0.0]
    assert [float(x) for x in R.exact(v, r, t, 5.0, 0, 0.5, 0.5, 1)] == [0.75, -1.0, -0.125, -0.5]
    one = Fraction(1); ulp = Fraction(1, 2 ** 23)
    assert R.rn32(one + ulp / 2) == np.float32(1.0) and R.rn32(one + 3 * ulp / 2) == np.float32(1.0) + np.float32(2.0 ** -22)      # ties to even
    assert R.rn32(one + ulp / 2 + Fraction(1, 2 ** 80)) == np.float32(1.0) + np.float32(2.0 ** -23)                                # beyond Float64's reach
    assert R.rn32(Fraction(3, 2 ** 150)) == np.float32(2.0 ** -148) and R.rn32(Fraction(1, 2 ** 150)) == np.float32(0.0)
    assert R.width(np.float32(-0.0), np.float32(0.0)) == 1 and R.width(np.float32(-2.0 ** -149), np.float32(2.0 ** -149)) == 3


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_references_lie_within_the_bound_of_the_exact_recurrence(family):
    """Every env of three shapes (k = 1024 among them), both modes: |reference − exact| <= bound, for the serial recurrence and for the segmented scan
    at L = 8 and 16. The worst ratio per family is the profile's "cpu_worst_error_over_bound"."""
    worst = {"serial64": 0.0, "segmented64_L8": 0.0, "segmented64_L16": 0.0}
    for nt, k in ((6, 37), (4, 129), (2, 1024)):
        d = G.inputs(family, nt, k)
        for mode in (0, 1):
            a = G.args(d, mode)
            b = R.bound(*a)
            refs = {"serial64": R.serial64(*a), "segmented64_L8": R.segmented64(*a, 8), "segmented64_L16": R.segmented64(*a, 16)}
            for e in range(nt):
                x = R.exact(d["value"][e], d["reward"][e], d["term"][e], d["nv"][e], d["nd"][e], d["gamma"], d["lam"], mode)
                for name, ref in refs.items():
                    for t in range(k):
                        err = abs(Fraction(float(ref[e, t])) - x[t])
                        if b[e, t] == 0.0:
                            assert err == 0, (family, name, nt, k, mode, e, t)
                        else:
                            worst[name] = max(worst[name], float(err / Fraction(float(b[e, t]))))
    print(family, worst)
    assert max(worst.values()) <= 1.0, worst
    if WRITE:
        write_profile("cpu_worst_error_over_bound", {family: worst})


def test_table_reaches_all_50_kernels_and_every_error_row_errs():
    reached = {}
    for row in G.GEOMETRY:
        r = G.route(row.nt, row.k, row.seg, row.tile)
        assert r in G.COMPILED, (row, r)
        assert row.nt * row.k <= 1.2e6, row
        for ntl in (0, 1):
            reached.setdefault(r + (ntl,), row)
    assert set(reached) == G.KERNELS and len(G.KERNELS) == 50, sorted(G.KERNELS - set(reached))
    for row, err in G.ERROR_ROWS:
        assert G.route(row.nt, row.k, row.seg, row.tile) == err, row
    # what the issue's reading of the rule says about the older tests' companion launches
    assert G.route(65536, 128, 0, 64) == ("one", 32, 8), "tile = 64 at (65536, 128) really runs EB = 32"
    assert all(G.route(nt, 9, 0, 64)[1] == 8 for nt in (1, 100, 4095, 16368)) and G.route(16369, 9, 0, 64)[1] == 16
    assert G.route(5, 600, 8, 0) == ("one", 8, 16) and G.route(6, 600, 8, 128) == ("pair", 8, 16), "the L 8 → 16 fallbacks"
    assert G.route(6, 1024, 0, 128) == ("pair", 8, 16) and G.block_threads(("pair", 8, 16), 1024) == 512
    assert G.route(524288, 128, 0, 0) == ("stream", 4, 4) and G.route(262144, 128, 0, 0) == ("stream", 2, 4) and G.route(262144, 127, 0, 0) == ("pair", 32, 8)
    assert G.route(262146, 128, 0, 0, aligned=False) == ("one", 32, 8) and G.route(262146, 64, 0, 0, aligned=False) == ("one", 64, 8)


def test_rule_never_leaves_the_compiled_set_or_512_threads():
    nts = sorted(set(list(range(1, 70)) + [2 ** i + j for i in range(7, 17) for j in (-1, 0, 1, 2)] + [4095, 4096, 4097, 4098, 16368, 16369, 16370, 32736, 32737, 32738,
                                                                                                        65472, 65473, 65474, 69999, 70000] + list(range(100, 70000, 3331))))
    ks = sorted(set(list(range(1, 140)) + list(range(250, 262)) + list(range(505, 520)) + list(range(1017, 1030)) + list(range(140, 1101, 37)) + [1100]))
    n = 0
    for nt in nts:
        for k in ks:
            for seg in G.SEGS:
                for tile in G.TILES:
                    r = G.route(nt, k, seg, tile)
                    n += 1
                    if isinstance(r, str):
                        assert r in (G.ERR_STREAM, G.ERR_PAIR, G.ERR_STEPS), (nt, k, seg, tile, r)
                        assert r != G.ERR_STEPS or k > 1024, (nt, k, seg, tile)
                        continue
                    assert r in G.COMPILED and G.block_threads(r, k) <= 512, (nt, k, seg, tile, r)
                    assert r[0] == "stream" or k <= 1024, (nt, k, seg, tile, r)
    assert n > 1_000_000


def test_families_are_dealt_to_every_kernel_family_at_both_lengths():
    met = {}
    for c in G.CASES:
        met.setdefault(G.group(c.route), set()).add(c.family)
        assert c.mode == 1 or c.family not in G.FIXED_ONLY
    for fam in ("one", "pair", "stream"):
        for l in (8, 16):
            assert met[(fam, l)] == set(G.FAMILIES), ((fam, l), set(G.FAMILIES) - met[(fam, l)])
    assert len({G.case_id(c) for c in G.CASES}) == len(G.CASES) == 4 * len(G.GEOMETRY)
    for c in G.CASES:
        assert 1 <= len(G.exact_envs(c.row.nt, c.route)) <= 16


def test_flag_bytes_family_isolates_every_byte_of_every_pair_and_quad():
    d = G.inputs("flag_bytes", 64, 40)
    f = np.concatenate([d["term"], d["nd"][:, None]], axis=1)
    assert set(np.unique(f)) == {0, 1, 2, 0x80, 0xFF}
    lone_bytes = [set() for _ in range(4)]
    for q in range(16):
        quad = f[4 * q:4 * q + 4] != 0
        for lane in range(4):
            alone = quad[lane] & (quad.sum(0) == 1)
            assert alone.any(), (q, lane)
            lone_bytes[lane] |= set(np.unique(f[4 * q + lane][alone]).tolist())
            pair = quad[lane & ~1:(lane & ~1) + 2]
            assert (pair[lane & 1] & (pair.sum(0) == 1)).any(), (q, lane)
    assert all(b == {1, 2, 0x80, 0xFF} for b in lone_bytes), lone_bytes          # every byte position sees every non-zero byte alone
    # the same arrangement reaches next_done: over the quads, every lane is the only non-zero byte of its quad's next_done
    nd = (f[:, -1] != 0).reshape(16, 4)
    assert all(((nd.sum(1) == 1) & nd[:, lane]).any() for lane in range(4))


def _cpu_pairs():
    """(row, family, mode) that the CPU-side conditions run over: the family the table deals each row, and every family on the rows of up to SMALL samples."""
    seen = set()
    for c in G.CASES:
        seen.add((c.row, c.family, c.mode))
        if c.row.nt * c.row.k <= SMALL:
            for fam in G.FAMILIES:
                if c.mode == 1 or fam not in G.FIXED_ONLY:
                    seen.add((c.row, fam, c.mode))
    return sorted(seen, key=lambda p: (G.GEOMETRY.index(p[0]), p[1], p[2]))


def test_interval_is_sharp():
    """A condition on the families, not a measurement of the kernels: over every (row, family) pair but `cancellation`'s, at most 1 % of a family's outputs have
    an interval [RN32(x − bound), RN32(x + bound)] that holds more than two adjacent Float32 values (x = serial64: the interval's width does not depend on
    which point inside the bound it is centred on)."""
    wide, total = {}, {}
    for row, fam, mode in _cpu_pairs():
        a = G.args(G.inputs(fam, row.nt, row.k), mode)
        lo, hi = R.interval64(R.serial64(*a), R.bound(*a), 1.0)
        w = R.width(lo, hi)
        assert np.all(w >= 1)
        wide[fam] = wide.get(fam, 0) + int(np.sum(w > 2)); total[fam] = total.get(fam, 0) + w.size
    share = {f: wide[f] / total[f] for f in total}
    print(share)
    assert all(share[f] <= 0.01 for f in share if f != "cancellation"), share
    assert sum(wide[f] for f in wide if f != "cancellation") <= 0.01 * sum(total[f] for f in total if f != "cancellation")
    if WRITE:
        write_profile("cpu_share_of_intervals_wider_than_two_floats", share)


def _fails(cand64, x64, b):
    lo, hi = R.interval64(x64, b, 2.0)
    return bool(R.outside(cand64.astype(np.float32), lo, hi).any())


def _small_pairs():
    return [(row, fam, mode) for row, fam, mode in _cpu_pairs() if row.nt * row.k <= SMALL]


def test_unbroken_references_pass_the_interval_check_on_every_case():
    for row, fam, mode in _cpu_pairs():
        a = G.args(G.inputs(fam, row.nt, row.k), mode)
        x, b = R.serial64(*a), R.bound(*a)
        r = G.route(row.nt, row.k, row.seg, row.tile)
        L = r[2] if r[0] != "stream" else 8
        assert not _fails(R.segmented64(*a, L), x, b), (row, fam, mode)
        assert not _fails(x, x, b)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_broken_piece_fails_the_interval_check_on_some_case(mutant):
    """flag tested with `& 1`; the second env of a pair reading the first env's byte; the carry not folded across segments; the boundary value v[L] taken as 0;
    compat's last slot not zeroed; next_done ignored. Each must fall outside [RN32(serial64 − 2·bound), RN32(serial64 + 2·bound)] somewhere in the table, in
    the segmented scan and (where it is a piece of the serial recurrence too) in serial64."""
    caught = {"segmented64": [], "serial64": []}
    for row, fam, mode in _small_pairs():
        a = G.args(G.inputs(fam, row.nt, row.k), mode)
        x, b = R.serial64(*a), R.bound(*a)
        r = G.route(row.nt, row.k, row.seg, row.tile)
        L = r[2] if r[0] != "stream" else 8
        if _fails(R.segmented64(*a, L, mutant=mutant), x, b):
            caught["segmented64"].append((row.why, fam, mode))
        if mutant not in R.SEGMENTED_ONLY and _fails(R.serial64(*a, mutant=mutant), x, b):
            caught["serial64"].append((row.why, fam, mode))
    print(mutant, {n: len(c) for n, c in caught.items()})
    assert caught["segmented64"], mutant
    assert mutant in R.SEGMENTED_ONLY or caught["serial64"], mutant
    if mutant == "flag_and_1":
        assert {f for _, f, _ in caught["segmented64"]} == {"flag_bytes"}, "only bytes other than 0 / 1 can tell"
    if mutant == "compat_last_live":
        assert {m for _, _, m in caught["segmented64"]} == {0}
    if mutant == "no_next_done":
        assert {m for _, _, m in caught["segmented64"]} == {1}
