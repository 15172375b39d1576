"""What the dueling-DQN parity tests share (tests/test_duel_cpu.py, tests/test_gpu_duel.py, scripts/duel_bar.py), after tests/c51_bar.py: the ONE case
table, the distances over the observables (logged losses, q_net, target_net, and on a categorical head the last update's projected targets), and the
two instruments that say what a bar on them is worth — the jittered twin of tests/duel_ref.py (the FLOOR) and one-line wrong versions of it (the
MUTANTS).

The scalar head with uniform replay runs no transcendental at all: those cases are bit-equal on the device and their floor is exactly 0. The jitter
moves every exp, log and pow result by a seeded integer in −2..+2 ulp (ddpg_bar.JITTER_ULP, the amplitude every parity bar of this suite assumes).
Nobody has measured how far the device's Float64 exp, log and pow lie from a correctly rounded result.

The bars. loss_bar = ddpg_bar.LOSS_FACTOR x the largest loss floor over this table, proj_bar = the same factor x the largest floor of the projected
targets — scripts/duel_bar.py measures both into profiles/duel_bar.json, from the restatement alone, never from the device —; the parameter bar is
ddpg_bar.PARAM_BAR = 2^-21 per array.

A condition, not a measurement: device and restatement stay on one trajectory only while they agree bit for bit on every greedy action, every a*, every
drawn idx and every Float32 PER leaf. `measure` therefore also says whether every jittered twin of a case reproduced the reference's own ("ties_ok"); a
case that does not gets another seed."""
import contextlib
import json
import os

import numpy as np

import c51_bar as CB
import c51_ref as Z
import ddpg_bar as B
import dqn_per_bar as PB
import dqn_per_ref as P
import duel_ref as D
import oraclelib as O

BAR_JSON = os.path.join(B.ROOT, "profiles", "duel_bar.json")
PARAM_BAR, LOSS_FACTOR, MUTANT_FACTOR, JITTER_SEEDS = B.PARAM_BAR, B.LOSS_FACTOR, B.MUTANT_FACTOR, B.JITTER_SEEDS
JITTER_ULP = max(B.JITTER_ULP["exp"], B.JITTER_ULP["log"])   # for pow as well
LOSSES, PARAMS, PROJ = ("loss",), ("q", "target"), ("proj",)
OBSERVABLES = LOSSES + PARAMS + PROJ
TD_WAVES = CB.TD_WAVES


# ---------------------------------------------------------------------------------------------------- the case table
def _case(name, edge, seed=21, per=False, tgt=None, c51=None, **kw):
    return dict(name=name, edge=edge, seed=seed, per=per, tgt=tgt or {}, c51=c51, kw=kw)


# dqn_per_bar._BASE (k = 31 in a ring of 1000, an update every 10 steps from step 110 on: 20 updates in 300 steps; lr = 1e-3, every update logged), and
# epsilon reaches 0.05 at step 300, so that a third of the steps act greedily on the combined head
_BASE = dict(PB._BASE, epsilon_duration=300.0)
_N3D = dict(n_step=3, double_q=1)
CASES = [
    _case("k1_cap1", "k = 1 in a ring of 1", total_timesteps=120, batch_size=1, buffer_size=1, min_buff_size=1, train_freq=1, target_net_freq=1),
    _case("k31", "the base shape: 168·31 hidden units are no multiple of a block"),
    _case("k120", "the reference's default batch", total_timesteps=400, batch_size=120, min_buff_size=200),
    _case("k1024", "the largest batch; k = n", total_timesteps=1100, batch_size=1024, buffer_size=1024, min_buff_size=1024, train_freq=25),
    _case("per", "prioritized replay: the leaf comes from |δ| of the combined Q", per=True),
    _case("n3_double", "3-step returns with double Q: three passes through both streams", tgt=_N3D),
    _case("per_n3_double", "all three together", per=True, tgt=_N3D),
    _case("wrap_cap31", "3-step returns, k = n in a ring that wraps 12 times", total_timesteps=400, buffer_size=31, min_buff_size=40, train_freq=3,
          tgt=dict(n_step=3)),
    _case("logfreq7", "log_frequency = 7: records at 140, 210, 280", log_frequency=7),
    _case("gamma0", "gamma = 0: the TD target is the reward", gamma=0.0),
    _case("c51_n2", "categorical, two atoms", c51=dict(n_atoms=2)),
    _case("c51_n51", "categorical, the default support; one sample more than a block of the TD kernel holds", c51=dict(n_atoms=51), batch_size=TD_WAVES + 1),
    _case("c51_n64", "categorical, every lane owns an atom: the largest LDS image", c51=dict(n_atoms=64)),
    _case("c51_n33_per_n3_double", "categorical with an odd head, prioritized replay, 3-step returns and double Q", c51=dict(n_atoms=33), per=True, tgt=_N3D),
]
CASE = {c["name"]: c for c in CASES}
SCALAR_UNIFORM = tuple(c["name"] for c in CASES if c["c51"] is None and not c["per"])   # no transcendental anywhere: bit-equal on the device
CHEAPEST = ("k1_cap1", "c51_n2")                           # what tests/test_duel_cpu.py recomputes


def case_cfg(case):
    return O.dqn_config(**{"lr": 1e-3, "log_frequency": 1, "seed": case["seed"], **_BASE, **case["kw"]})


def case_per(case):
    if not case["per"]:
        return None
    return {"alpha": 0.6, "beta_start": 0.4, "beta_end": 1.0, "beta_duration": float(case_cfg(case).total_timesteps), "eps": 1e-6}


def case_tgt(case):
    return {"n_step": 1, "double_q": 0, **case["tgt"]}


def case_c51(case):
    return None if case["c51"] is None else {"n_atoms": 51, "v_min": 0.0, "v_max": 100.0, **case["c51"]}


def case_R(case):
    return 1 if case["c51"] is None else case_c51(case)["n_atoms"]


def params_for(Rr):
    """a perturbed glorot net with non-zero biases in all ten arrays"""
    rng = np.random.default_rng(1)
    out = np.zeros(D.param_count(Rr), np.float32)
    o = 0
    for n, shape in zip(D.sizes(Rr), D.shapes(Rr)):
        if len(shape) == 2:
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[o:o + n] = rng.uniform(-lim, lim, n).astype(np.float32)
        o += n
    return out + (0.05 * np.random.default_rng(2).standard_normal(out.size)).astype(np.float32)


def case_params(case):
    return params_for(case_R(case))


# ---------------------------------------------------------------------------------------------------- distances
def distances(losses, params, proj, ref_losses, ref_params, ref_proj, Rr):
    """losses: [(global_step, loss)], params: (q, target), proj (N, k) of the last update or None on a scalar head → {observable: distance}"""
    assert [l[0] for l in losses] == [l[0] for l in ref_losses] and len(losses) > 0
    out = {"loss": PB.loss_distance([l[1] for l in losses], [l[1] for l in ref_losses])}
    for name, dev, rf in zip(PARAMS, params, ref_params):
        out[name] = B.rel_per_array(dev, rf, D.sizes(Rr))
    out["proj"] = 0.0 if ref_proj is None else float(np.abs(np.asarray(proj) - np.asarray(ref_proj)).max())
    return out


def load_bars(path=BAR_JSON):
    prof = json.load(open(path))
    return {"loss": prof["loss_bar"], "q": prof["param_bar"], "target": prof["param_bar"], "proj": prof["proj_bar"]}


# ---------------------------------------------------------------------------------------------------- the jittered twin
@contextlib.contextmanager
def jitter(seed, amp=JITTER_ULP):
    """every exp, log and pow result of the restatement moved by a seeded random integer in −amp..+amp ulp (exact results move as well)"""
    rng = np.random.default_rng(seed)

    def moved(f):
        def g(*x):
            v = np.asarray(f(*x), np.float64)
            return v + rng.integers(-amp, amp + 1, v.shape).astype(np.float64) * np.spacing(np.abs(v))
        return g
    with D.replaced(Z, _exp=moved(np.exp), _log=moved(np.log)), D.replaced(P, _pow=moved(np.power)):
        yield


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
MUTANTS = {
    "M1": ("no mean subtraction", lambda: dict(centre=lambda A: A)),
    "M2": ("the mean over the atoms instead of the actions", lambda: dict(centre=lambda A: A - A.mean(axis=1, keepdims=True))),
    "M3": ("dA of the other action with the wrong sign", lambda: dict(d_adv_other=lambda half: half)),
    "M4": ("dV scaled by 0.5", lambda: dict(d_value=lambda g: g * 0.5)),
    "M5": ("the streams swapped in d1", lambda: dict(d1_streams=lambda W2v, W2a: (W2a, W2v))),
    "M6": ("the value head fed from h2a", lambda: dict(value_input=lambda h2v, h2a: h2a)),
}
MUTANT_MAX_BATCH = 31                                      # mutants run where a run is cheap: every case but k120 and k1024


def applicable(case):
    return list(MUTANTS) if case_cfg(case).batch_size <= MUTANT_MAX_BATCH else []


# ---------------------------------------------------------------------------------------------------- one case, measured
def make_ref(case):
    return D.make(case_cfg(case), case_per(case), case_tgt(case), case_c51(case), case_params(case))


def run_ref(case, patch=None):
    """the case through duel_ref (under `patch`, a context manager) → (losses, (q, target), proj or None, trajectory)"""
    cfg = case_cfg(case)
    with (patch if patch is not None else contextlib.nullcontext()):
        ref = make_ref(case)
        losses = ref.run(cfg.total_timesteps)[2]
    return losses, (ref.q, ref.t), (None if case["c51"] is None else ref.proj), dict(greedy=ref.greedy, seen=ref.seen, per=case["per"])


def variant(case, what, base):
    """what: ("jitter", seed) or a mutant's name → (the distances of that variant from the base run, whether it stayed on the base run's trajectory)"""
    patch = jitter(what[1]) if isinstance(what, tuple) else D.replaced(D, **MUTANTS[what][1]())
    losses, params, proj, tr = run_ref(case, patch)
    return distances(losses, params, proj, base[0], base[1], base[2], case_R(case)), CB.same_trajectory(tr, base[3])


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
