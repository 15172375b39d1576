"""What the prioritized-replay parity tests share (tests/test_dqn_per_cpu.py, tests/test_gpu_dqn_per.py, scripts/dqn_per_bar.py), after
tests/td3_bar.py: the ONE case table, the distances over the three observables (logged losses, q_net, target_net), and the two instruments that say what
a bar on them is worth — the jittered twin of tests/dqn_per_ref.py (the FLOOR) and one-line wrong versions of it (the MUTANTS).

The jitter moves every pow result by a seeded integer in −16..+16 ulp. The ROCm tree states no Float64 error bound for the device pow, so the amplitude
is the OpenCL full-profile bound for pow, 16 ulp; nobody has measured the real figure.

The bars. loss_bar = ddpg_bar.LOSS_FACTOR x the largest loss floor over this table (scripts/dqn_per_bar.py measures it into
profiles/dqn_per_bar.json); the parameter bar is ddpg_bar.PARAM_BAR = 2^-21 per array.

A condition, not a measurement: device and restatement have to agree bit for bit on idx and on the Float32 leaves, which holds only while no leaf
sits on a Float32 rounding tie of pow. `measure` therefore also says whether every jittered twin of a case reproduced the reference's own idx and
leaves after every update ("ties_ok"); a case that does not gets another seed."""
import contextlib
import json
import os

import numpy as np

import ddpg_bar as B
import dqn_per_ref as P
import oraclelib as O

BAR_JSON = os.path.join(B.ROOT, "profiles", "dqn_per_bar.json")
PARAM_BAR, LOSS_FACTOR, MUTANT_FACTOR, JITTER_SEEDS = B.PARAM_BAR, B.LOSS_FACTOR, B.MUTANT_FACTOR, B.JITTER_SEEDS
JITTER_ULP = 16                                            # OpenCL full profile: pow <= 16 ulp
LOSSES, PARAMS = ("loss",), ("q", "target")
OBSERVABLES = LOSSES + PARAMS
CHUNKS = (1, 7)                                            # then the rest, as tests/test_gpu_dqn_edges.py


# ---------------------------------------------------------------------------------------------------- the case table
def _case(name, edge, seed=21, per=None, **kw):
    return dict(name=name, edge=edge, seed=seed, per=per or {}, kw=kw)


# lr = 1e-3 and every update logged unless the case says otherwise, as tests/test_gpu_dqn_edges.py; the base shape is k = 31 in a ring of 1000 with
# an update every 10 steps from step 110 on (20 updates in 300 steps)
_BASE = dict(total_timesteps=300, batch_size=31, buffer_size=1000, min_buff_size=100, train_freq=10, target_net_freq=50)
CASES = [
    _case("k1_cap1", "smallest everything: C = 1, the leaf is the root", total_timesteps=120, batch_size=1, buffer_size=1, min_buff_size=1,
          train_freq=1, target_net_freq=1),
    _case("k31_cap31", "k = n; the ring wraps and is not a power of two", total_timesteps=400, buffer_size=31, min_buff_size=40, train_freq=3),
    _case("k61_cap64", "a ring that is a power of two; two unrolled rounds + 1", total_timesteps=300, batch_size=61, buffer_size=64, min_buff_size=70),
    _case("k120", "the reference's default batch", total_timesteps=400, batch_size=120, min_buff_size=200),
    _case("k1024_cap1024", "the largest batch; k = n = C", total_timesteps=1200, batch_size=1024, buffer_size=1024, min_buff_size=1024,
          train_freq=25),
    _case("first_1510", "the first update has 1510 new slots: more than one pass of the block's 1024 threads", total_timesteps=1600,
          buffer_size=2048, min_buff_size=1500),
    _case("freq_gt_ring", "train_freq 40 > buffer_size 31: every update finds the whole ring new", total_timesteps=480, buffer_size=31,
          min_buff_size=40, train_freq=40),
    _case("alpha0", "alpha = 0: every leaf is 1.0, the draw is uniform with replacement", per=dict(alpha=0.0)),
    _case("alpha05", "alpha = 0.5", per=dict(alpha=0.5)),
    _case("alpha1", "alpha = 1: the leaf is |δ| + eps", per=dict(alpha=1.0)),
    _case("beta_mid", "beta reaches beta_end at step 200 of 300", per=dict(beta_duration=200.0)),
    _case("beta_down", "a falling schedule, 1.0 to 0.4 by step 200", per=dict(beta_start=1.0, beta_end=0.4, beta_duration=200.0)),
    _case("gamma0", "gamma = 0: the TD target is the reward", gamma=0.0),
    _case("logfreq7", "log_frequency = 7: records at 140, 210, 280", log_frequency=7),
]
CASE = {c["name"]: c for c in CASES}
CHEAPEST = ("k1_cap1", "gamma0")                           # what tests/test_dqn_per_cpu.py recomputes


def case_cfg(case):
    return O.dqn_config(**{"lr": 1e-3, "log_frequency": 1, "seed": case["seed"], **_BASE, **case["kw"]})


def case_per(case):
    cfg = case_cfg(case)
    return {"alpha": 0.6, "beta_start": 0.4, "beta_end": 1.0, "beta_duration": float(cfg.total_timesteps), "eps": 1e-6, **case["per"]}


def case_params(case):
    """a perturbed glorot Q-net with non-zero biases, as tests/test_gpu_dqn.py makes"""
    return O.dqn_params(1) + (0.05 * np.random.default_rng(1).standard_normal(O.DQN_P)).astype(np.float32)


def update_steps(cfg):
    return [g for g in range(cfg.min_buff_size + 1, cfg.total_timesteps + 1) if g % cfg.train_freq == 0]


# ---------------------------------------------------------------------------------------------------- distances
def loss_distance(dev, ref):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(dev - ref).max() / np.abs(ref).max())


def distances(losses, params, ref_losses, ref_params):
    """losses: [(global_step, loss)], params: (q, target) → {observable: distance}; the logged steps have to be the reference's"""
    assert [l[0] for l in losses] == [l[0] for l in ref_losses] and len(losses) > 0
    out = {"loss": loss_distance([l[1] for l in losses], [l[1] for l in ref_losses])}
    for name, dev, rf in zip(PARAMS, params, ref_params):
        out[name] = B.rel_per_array(dev, rf, P.SIZES)
    return out


def load_bars(path=BAR_JSON):
    prof = json.load(open(path))
    return prof["loss_bar"], prof["param_bar"]


def bar_of(name, loss_bar, param_bar=PARAM_BAR):
    return loss_bar if name in LOSSES else param_bar


# ---------------------------------------------------------------------------------------------------- patching dqn_per_ref for one run
@contextlib.contextmanager
def patched(**attrs):
    saved = []
    try:
        for name, new in attrs.items():
            saved.append((name, getattr(P, name)))
            setattr(P, name, new)
        yield
    finally:
        for name, old in reversed(saved):
            setattr(P, name, old)


def jitter(seed, amp=JITTER_ULP):
    """dqn_per_ref with every pow result moved by a seeded random integer in −amp..+amp ulp (exact results — pow(x, 0) = 1 — move as well)"""
    rng = np.random.default_rng(seed)

    def _pow(x, y):
        v = np.asarray(np.power(x, y), np.float64)
        return v + rng.integers(-amp, amp + 1, v.shape).astype(np.float64) * np.spacing(np.abs(v))
    return patched(_pow=_pow)


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
def _unstratified(seed, g, k, total):
    return P.R.uniform(seed, np.arange(k), g, P.S_PER) * total


def _fixed_beta(per, g):
    return per["beta_start"]


def _spread(st):
    """some update drew from leaves that were not all equal: with equal leaves (one slot; a ring that is all new at every update; alpha = 0) the draw
    is uniform and every weight 1.0 whatever the leaves' common value"""
    return st["spread_updates"] > 0


# name → (what it mirrors, where it applies given the case and the reference's own statistics of it, the patch)
MUTANTS = {
    "M1": ("weights not normalised", lambda c, st: st["beta_max"] > 0.0 and st["weights_below_one"] > 0, lambda: dict(normalise=lambda w: w)),
    "M2": ("beta fixed at beta_start", lambda c, st: case_per(c)["beta_start"] != case_per(c)["beta_end"] and st["weights_below_one"] > 0,
           lambda: dict(beta_schedule=_fixed_beta)),
    "M3": ("target = u·total, unstratified", lambda c, st: case_cfg(c).batch_size > 1, lambda: dict(draw_targets=_unstratified)),
    "M4": ("new leaves without + eps", lambda c, st: case_per(c)["alpha"] > 0.0 and _spread(st), lambda: dict(priority=lambda abs_td, eps: abs_td)),
    "M5": ("max_leaf never raised", lambda c, st: st["max_leaf"] > 1.0 and _spread(st),
           lambda: dict(raise_max=lambda max_leaf, new: max_leaf)),
    "M6": ("new slots get 1.0 instead of max_leaf", lambda c, st: st["max_leaf"] > 1.0 and _spread(st),
           lambda: dict(new_slot_leaf=lambda max_leaf: 1.0)),
    "M7": ("dz without w", lambda c, st: st["weights_below_one"] > 0, lambda: dict(cotangent=lambda w, diff, k: -2.0 * diff / np.float64(k))),
    "M8": ("the zero test dropped", lambda c, st: st["zero_saves"] > 0, lambda: dict(go_left=lambda target, l, r: target < l)),
    "M9": ("leaves kept in Float64", lambda c, st: case_per(c)["alpha"] > 0.0 and _spread(st), lambda: dict(LEAF_T=np.float64)),
}


def applicable(case, stats):
    return [m for m, (_, applies, _) in MUTANTS.items() if applies(case, stats)]


# ---------------------------------------------------------------------------------------------------- one case, measured
def run_ref(case, patch=None, chunks=False):
    """the case through dqn_per_ref (under `patch`, a context manager) → (losses, (q, target), stats, seen)"""
    cfg = case_cfg(case)
    P.COUNTS["zero_saves"] = 0
    with (patch if patch is not None else contextlib.nullcontext()):
        ref = P.DQNPER(cfg, case_per(case), case_params(case))
        below, beta_max = 0, 0.0
        losses = []
        while ref.global_step < cfg.total_timesteps:
            n0 = ref.n_updates
            losses += ref.run(1)[2]
            if ref.n_updates > n0:
                below += int((ref.w < 1.0).sum()); beta_max = max(beta_max, ref.beta)
    stats = dict(max_leaf=float(ref.max_leaf), weights_below_one=below, beta_max=float(beta_max), zero_saves=int(P.COUNTS["zero_saves"]),
                 updates=ref.n_updates, spread_updates=ref.n_spread, duplicates=int(sum(len(i) - len(set(i.tolist())) for _, i, _ in ref.seen)))
    return losses, (ref.q, ref.t), stats, ref.seen


def same_draws(seen, base_seen):
    """every update drew the base run's idx and left the base run's leaves, bit for bit"""
    return len(seen) == len(base_seen) and all(g == h and np.array_equal(i, j) and np.array_equal(a, b)
                                               for (g, i, a), (h, j, b) in zip(seen, base_seen))


def variant(case, what, base):
    """what: ("jitter", seed) or a mutant's name → (the distances of that variant from the base run, whether it drew the base run's idx and leaves)"""
    patch = jitter(what[1]) if isinstance(what, tuple) else patched(**MUTANTS[what][2]())
    losses, params, _, seen = run_ref(case, patch)
    return distances(losses, params, base[0], base[1]), same_draws(seen, base[3])


def measure(case):
    """→ {"floor": {observable: max over the jitter seeds}, "ties_ok": every twin drew the reference's idx and leaves, "mutants": {name: {observable:
    distance}}, "stats": the base run's}"""
    base = run_ref(case)
    twins = [variant(case, ("jitter", s), base) for s in JITTER_SEEDS]
    return {"floor": {o: max(t[0][o] for t in twins) for o in OBSERVABLES}, "ties_ok": all(t[1] for t in twins), "stats": base[2],
            "mutants": {m: variant(case, m, base)[0] for m in applicable(case, base[2])}}


def mutant_ratio(dist, loss_bar, param_bar=PARAM_BAR):
    """the largest distance / bar over the three observables"""
    return max(dist[o] / bar_of(o, loss_bar, param_bar) for o in OBSERVABLES)
