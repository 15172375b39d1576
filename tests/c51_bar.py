"""What the categorical-DQN parity tests share (tests/test_c51_cpu.py, tests/test_gpu_c51.py, scripts/c51_bar.py), after tests/dqn_per_bar.py: the
ONE case table, the distances over the observables (logged losses, q_net, target_net, the last update's projected targets), and the two instruments
that say what a bar on them is worth — the jittered twin of tests/c51_ref.py (the FLOOR) and one-line wrong versions of it (the MUTANTS).

The jitter moves every exp and every log result by a seeded integer in −2..+2 ulp (ddpg_bar.JITTER_ULP). Nobody has measured how far the device's
Float64 exp and log lie from a correctly rounded result; 2 ulp is the amplitude the other parity bars of this suite assume for them.

The bars. loss_bar = ddpg_bar.LOSS_FACTOR x the largest loss floor over this table, proj_bar = the same factor x the largest floor of the projected
targets (a distance relative to 1: the rows of m sum to 1) — scripts/c51_bar.py measures both into profiles/c51_bar.json —; the parameter bar is
ddpg_bar.PARAM_BAR = 2^-21 per array.

A condition, not a measurement: device and restatement stay on one trajectory only while they agree bit for bit on every greedy action, every a*, every
drawn idx and every Float32 PER leaf. `measure` therefore also says whether every jittered twin of a case reproduced the reference's own ("ties_ok"); a
case that does not gets another seed."""
import contextlib
import json
import os

import numpy as np

import c51_ref as Z
import ddpg_bar as B
import dqn_per_bar as PB
import oraclelib as O

BAR_JSON = os.path.join(B.ROOT, "profiles", "c51_bar.json")
PARAM_BAR, LOSS_FACTOR, MUTANT_FACTOR, JITTER_SEEDS = B.PARAM_BAR, B.LOSS_FACTOR, B.MUTANT_FACTOR, B.JITTER_SEEDS
JITTER_ULP = max(B.JITTER_ULP["exp"], B.JITTER_ULP["log"])
LOSSES, PARAMS, PROJ = ("loss",), ("q", "target"), ("proj",)
OBSERVABLES = LOSSES + PARAMS + PROJ
TD_WAVES = 4                                               # samples per block of the TD kernel (csrc/dqn_c51.hpp C51_TD_WAVES)


# ---------------------------------------------------------------------------------------------------- the case table
def _case(name, edge, seed=21, per=False, tgt=None, c51=None, **kw):
    return dict(name=name, edge=edge, seed=seed, per=per, tgt=tgt or {}, c51=c51 or {}, kw=kw)


# dqn_per_bar._BASE (k = 31 in a ring of 1000, an update every 10 steps from step 110 on: 20 updates in 300 steps; lr = 1e-3, every update logged), and
# epsilon reaches 0.05 at step 300 instead of 10000, so that a third of the steps act greedily on the expected values
_BASE = dict(PB._BASE, epsilon_duration=300.0)
_N3D = dict(n_step=3, double_q=1)
CASES = [
    _case("k1_cap1", "k = 1 in a ring of 1", total_timesteps=120, batch_size=1, buffer_size=1, min_buff_size=1, train_freq=1, target_net_freq=1),
    _case("k31_n51", "the default support; k is no multiple of a TD block's four samples"),
    _case("k5", "one sample more than a block of the TD kernel holds: the second block has one live wave", batch_size=TD_WAVES + 1),
    _case("k120", "the reference's default batch", total_timesteps=400, batch_size=120, min_buff_size=200),
    _case("k1024_n64", "the largest batch with the largest head; k = n", c51=dict(n_atoms=64), total_timesteps=1100, batch_size=1024, buffer_size=1024,
          min_buff_size=1024, train_freq=25),
    _case("n2", "two atoms: every Tz lies between the only pair", c51=dict(n_atoms=2)),
    _case("n33", "an odd head that is no multiple of anything", c51=dict(n_atoms=33)),
    _case("n64", "every lane owns an atom", c51=dict(n_atoms=64)),
    _case("vmax5", "v_max = 5: the upper clamp is live on every late sample", c51=dict(v_max=5.0)),
    _case("vmin1", "v_min = 1: a terminal sample's Tz = 0 meets the lower clamp", c51=dict(v_min=1.0)),
    _case("gamma0", "gamma = 0: all mass lands between two atoms", gamma=0.0),
    _case("logfreq7", "log_frequency = 7: records at 140, 210, 280", log_frequency=7),
    _case("per", "prioritized replay alone: the leaf comes from loss_j", per=True),
    _case("n3_double", "3-step returns with double Q", tgt=_N3D),
    _case("per_n3_double", "all three together", per=True, tgt=_N3D),
    _case("wrap_cap31", "k = n in a ring that wraps 12 times", total_timesteps=400, buffer_size=31, min_buff_size=40, train_freq=3, tgt=dict(n_step=3)),
]
CASE = {c["name"]: c for c in CASES}
CHEAPEST = ("k1_cap1", "n2")                               # what tests/test_c51_cpu.py recomputes


def case_cfg(case):
    return O.dqn_config(**{"lr": 1e-3, "log_frequency": 1, "seed": case["seed"], **_BASE, **case["kw"]})


def case_per(case):
    if not case["per"]:
        return None
    return {"alpha": 0.6, "beta_start": 0.4, "beta_end": 1.0, "beta_duration": float(case_cfg(case).total_timesteps), "eps": 1e-6}


def case_tgt(case):
    return {"n_step": 1, "double_q": 0, **case["tgt"]}


def case_c51(case):
    return {"n_atoms": 51, "v_min": 0.0, "v_max": 100.0, **case["c51"]}


def case_params(case):
    """a perturbed glorot net with non-zero biases, as tests/dqn_per_bar.py makes; the head's rows get the Dense(84, 2N) limit"""
    N = case_c51(case)["n_atoms"]
    rng = np.random.default_rng(1)
    out = np.zeros(Z.param_count(N), np.float32)
    o = 0
    for n, (rows, cols) in zip(Z.sizes(N)[::2], ((120, 4), (84, 120), (2 * N, 84))):
        lim = np.sqrt(6.0 / (rows + cols))
        out[o:o + n] = rng.uniform(-lim, lim, n).astype(np.float32)
        o += n + rows
    return out + (0.05 * np.random.default_rng(2).standard_normal(out.size)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- distances
def distances(losses, params, proj, ref_losses, ref_params, ref_proj, N):
    """losses: [(global_step, loss)], params: (q, target), proj (N, k) of the last update → {observable: distance}"""
    assert [l[0] for l in losses] == [l[0] for l in ref_losses] and len(losses) > 0
    out = {"loss": PB.loss_distance([l[1] for l in losses], [l[1] for l in ref_losses])}
    for name, dev, rf in zip(PARAMS, params, ref_params):
        out[name] = B.rel_per_array(dev, rf, Z.sizes(N))
    out["proj"] = float(np.abs(np.asarray(proj) - np.asarray(ref_proj)).max())
    return out


def load_bars(path=BAR_JSON):
    prof = json.load(open(path))
    return {"loss": prof["loss_bar"], "q": prof["param_bar"], "target": prof["param_bar"], "proj": prof["proj_bar"]}


# ---------------------------------------------------------------------------------------------------- patching c51_ref for one run
@contextlib.contextmanager
def patched(**attrs):
    saved = []
    try:
        for name, new in attrs.items():
            saved.append((name, getattr(Z, name)))
            setattr(Z, name, new)
        yield
    finally:
        for name, old in reversed(saved):
            setattr(Z, name, old)


def jitter(seed, amp=JITTER_ULP):
    """c51_ref with every exp and log result moved by a seeded random integer in −amp..+amp ulp (exact results — exp(0) = 1 — move as well)"""
    rng = np.random.default_rng(seed)

    def moved(f):
        def g(x):
            v = np.asarray(f(x), np.float64)
            return v + rng.integers(-amp, amp + 1, v.shape).astype(np.float64) * np.spacing(np.abs(v))
        return g
    return patched(_exp=moved(np.exp), _log=moved(np.log))


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
def _no_terminal(R_, disc, z_s, term):
    return R_ + ((disc * z_s) * 1.0)


MUTANTS = {
    "M1": ("up − b and b − lo swapped", lambda: dict(split_weights=lambda pp, b, lo, up: (pp * (b - lo), pp * (up - b)))),
    "M2": ("no clamp", lambda: dict(clamp=lambda Tz, v_min, v_max: Tz)),
    "M3": ("no (1 − terminal)", lambda: dict(shifted=_no_terminal)),
    "M4": ("a* from the wrong net", lambda: dict(astar_source=lambda double_q, Qs, Qt: Qt if double_q else Qs)),
    "M5": ("p' from q_net", lambda: dict(pprime_source=lambda ls, lt: ls)),
    "M6": ("the other action's logits", lambda: dict(taken=lambda a: 1 - a)),
    "M7": ("the sign of dl", lambda: dict(cotangent=lambda w, p, m, k: -(w * (p - m) / np.float64(k)))),
}
MUTANT_MAX_BATCH = 31                                      # mutants run where a run is cheap: every case but k120 and k1024_n64


def applicable(case):
    return list(MUTANTS) if case_cfg(case).batch_size <= MUTANT_MAX_BATCH else []


# ---------------------------------------------------------------------------------------------------- one case, measured
def make_ref(case):
    return Z.C51(case_cfg(case), case_per(case), case_tgt(case), case_c51(case), case_params(case))


def run_ref(case, patch=None):
    """the case through c51_ref (under `patch`, a context manager) → (losses, (q, target), proj, trajectory)"""
    cfg = case_cfg(case)
    with (patch if patch is not None else contextlib.nullcontext()):
        ref = make_ref(case)
        losses = ref.run(cfg.total_timesteps)[2]
    return losses, (ref.q, ref.t), ref.proj, dict(greedy=ref.greedy, seen=ref.seen, per=case["per"])


def same_trajectory(tr, base):
    """every greedy action, and at every update idx, a* and (under PER) the Float32 leaves, are the base run's bit for bit"""
    if tr["greedy"] != base["greedy"] or len(tr["seen"]) != len(base["seen"]):
        return False
    return all(g == h and np.array_equal(i, j) and np.array_equal(a, b) and (not base["per"] or np.array_equal(u, v))
               for (g, i, a, u), (h, j, b, v) in zip(tr["seen"], base["seen"]))


def variant(case, what, base):
    """what: ("jitter", seed) or a mutant's name → (the distances of that variant from the base run, whether it stayed on the base run's trajectory)"""
    patch = jitter(what[1]) if isinstance(what, tuple) else patched(**MUTANTS[what][1]())
    losses, params, proj, tr = run_ref(case, patch)
    return distances(losses, params, proj, base[0], base[1], base[2], case_c51(case)["n_atoms"]), same_trajectory(tr, base[3])


def measure(case):
    """→ {"floor": {observable: max over the jitter seeds}, "ties_ok", "mutants": {name: {observable: distance}}, "stats"}"""
    base = run_ref(case)
    twins = [variant(case, ("jitter", s), base) for s in JITTER_SEEDS]
    seen = base[3]["seen"]
    stats = dict(updates=len(seen), greedy_steps=len(base[3]["greedy"]), greedy_ones=int(sum(a for _, a in base[3]["greedy"])),
                 astar_ones=int(sum(int(a.sum()) for _, _, a, _ in seen)))
    return {"floor": {o: max(t[0][o] for t in twins) for o in OBSERVABLES}, "ties_ok": all(t[1] for t in twins), "stats": stats,
            "mutants": {m: variant(case, m, base)[0] for m in applicable(case)}}


def mutant_ratio(dist, bars):
    """the largest distance / bar over the observables"""
    return max(dist[o] / bars[o] for o in OBSERVABLES)
