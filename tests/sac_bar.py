"""What the SAC parity tests share (tests/test_sac_bar_cpu.py, tests/test_gpu_sac.py, tests/test_gpu_sac_edges.py, scripts/sac_bar.py), after
tests/td3_bar.py: the case table of what SAC adds to DDPG, the distances over its nine observables, and the two instruments that say what a bar on
them is worth — the jittered twin of the reference (ddpg_bar.JitterNumpy at the same amplitude and seeds: the FLOOR) and one-line wrong versions
of tests/sac_ref.py (the MUTANTS). Transitions, critic parameters, the config dict and the bars' constants are ddpg_bar's.

The bars. loss_bar = LOSS_FACTOR x the largest loss floor over THIS table (scripts/sac_bar.py measures it into profiles/sac_bar.json); PARAM_BAR =
2^-21 per array and OLD_BAR = 1e-5 as for DDPG; log_alpha is one Float32 scalar: |dev - ref| / max(1, |ref|) under PARAM_BAR.

A second table, EDGE_CASES (scripts/sac_bar.py --table edges → profiles/sac_edges_bar.json), holds the squash's saturation, both ends of log_std and
the batch, ring and logging edges with a loss bar of its own, so that the hard cases do not loosen the first; within it the two hard cases are held
to LOSS_FACTOR x their OWN floor (case_loss_bar), so that the harder one does not loosen the other."""
import contextlib
import json
import os

import numpy as np

import ddpg_bar as B
import ddpg_ref as R
import sac_ref as S

BAR_JSON = os.path.join(B.ROOT, "profiles", "sac_bar.json")
EDGE_BAR_JSON = os.path.join(B.ROOT, "profiles", "sac_edges_bar.json")
OLD_BAR, PARAM_BAR, LOSS_FACTOR, MUTANT_FACTOR, JITTER_ULP, JITTER_SEEDS = B.OLD_BAR, B.PARAM_BAR, B.LOSS_FACTOR, B.MUTANT_FACTOR, B.JITTER_ULP, B.JITTER_SEEDS
LOSSES = ("actor_loss", "critic_loss", "alpha_loss")
PARAMS = ("actor", "critic1", "critic2", "target_critic1", "target_critic2")
OBSERVABLES = LOSSES + PARAMS + ("log_alpha",)
STATS = ("n_samples", "n_y_one", "n_y_near", "n_ls_low", "n_ls_high")


# ---------------------------------------------------------------------------------------------------- the case tables
def _case(name, D, A, T_, edge, terminal="some", mu_gain=1.0, mu_shift=0.0, s_gain=1.0, **kw):
    return dict(name=name, D=D, A=A, T=T_, edge=edge, terminal=terminal, mu_gain=mu_gain, mu_shift=mu_shift, s_gain=s_gain, kw=kw)


# Updates are the steps past max(min_buff_size, warmup_steps) = 10 at (3, 1): g = 11..T. Every update steps both critics, the actor and (autotune) α.
CASES = [
    _case("d1a1_k2", 1, 1, 150, "smallest net and batch: two blocks of two waves; a head of two rows", batch_size=2, min_buff_size=10, warmup_steps=5),
    _case("ni65_k31", 49, 16, 110, "NI = 65: one element in the second pass of each wave's 64-stride loop; 32 head rows", batch_size=31,
          min_buff_size=40, warmup_steps=35),
    _case("d64a16_k61", 64, 16, 140, "both maxima; 2A = 32 head rows; component words up to 16·60 + 15", batch_size=61, min_buff_size=70,
          warmup_steps=65),
    # the SAC edges at (3, 1), k = 7
    _case("autotune_off", 3, 1, 110, "autotune = 0: log_alpha keeps its bits, the alpha β powers stay", autotune=0, alpha=0.2),
    _case("alpha_small", 3, 1, 110, "alpha = 1e-3: the entropy terms are three orders below the Q terms", alpha=1e-3),
    _case("target_entropy_pos", 3, 1, 110, "target_entropy = +1: the alpha gradient changes sign against the default", target_entropy=1.0),
    _case("gamma0", 3, 1, 110, "gamma = 0: the TD target is the reward", gamma=0.0),
    _case("tau1", 3, 1, 110, "tau = 1: the critic targets become the online critics on every update", tau=1.0),
    _case("all_terminal", 3, 1, 110, "every transition terminal", terminal="all"),
    _case("none_terminal", 3, 1, 110, "no transition terminal", terminal="none"),
    _case("bounds_asym", 3, 1, 110, "act_low = -1, act_high = 0.5: scale = 0.75, bias = -0.25", act_low=-1.0, act_high=0.5),
]
CASE = {c["name"]: c for c in CASES}
CHEAPEST = ("gamma0", "autotune_off")                    # what tests/test_sac_bar_cpu.py recomputes

EDGE_CASES = [
    # Where 0 < 1 - y² < 1e-6 the 1e-6 inside the log caps ∂logπ/∂y at 2e6·scale, so one ulp of y (1.1e-16) moves δ3 by 1e-10: gradients that the
    # unsaturated cases pin to 1e-16 are pinned to 1e-10 here, and Adam's normalisation turns that into Float32 flips. The case therefore keeps the
    # near-saturated share small, most samples past |u| > 18.4 (y = ±1 exactly: δ3 = 0 exactly) and the update count at 15; denser settings
    # (μ x10 + 20: 11 % near) measured an actor floor of 8e-6, above PARAM_BAR ("SAC on the DDPG handle").
    _case("saturated", 3, 1, 110, "the μ rows of the head x10 + 21: |y| = 1 exactly on most samples, 0 < 1 - y² < 1e-6 on a few per cent", mu_gain=10.0,
          mu_shift=21.0, min_buff_size=95, warmup_steps=90),
    _case("logstd_ends", 3, 1, 110, "the s rows of the head x25: log_std within 1e-3 of -5 and of 2", s_gain=25.0),
    _case("k65", 3, 1, 150, "the first batch position past 63; component word 1024", batch_size=65, min_buff_size=70, warmup_steps=66),
    _case("k120_default", 3, 1, 210, "the default batch; four unrolled rounds", batch_size=120, min_buff_size=130, warmup_steps=125),
    _case("kmax_ring_eq_batch", 3, 1, 1038, "largest k; k = n; the ring wraps", batch_size=1024, buffer_size=1024, min_buff_size=1030,
          warmup_steps=1025),
    _case("logfreq7", 3, 1, 110, "log_frequency = 7: loss and alpha records at 14, 21, ...", log_frequency=7),
]
EDGE_CASE = {c["name"]: c for c in EDGE_CASES}
EDGE_CHEAPEST = ("logfreq7", "saturated")

# Denser settings of `saturated` that were measured and are NOT cases: their parameter floors lie above PARAM_BAR, which is not loosened for them.
# scripts/sac_bar.py --table edges records their floors and counters in the "rejected" block of profiles/sac_edges_bar.json.
REJECTED = [
    _case("saturated_mu20", 3, 1, 110, "the μ rows x10 + 20, 15 updates: 0 < 1 - y² < 1e-6 on 11 % of the samples", mu_gain=10.0, mu_shift=20.0,
          min_buff_size=95, warmup_steps=90),
    _case("saturated_x150", 3, 1, 110, "the μ rows x150, 100 updates: 0 < 1 - y² < 1e-6 on 9 % of the samples", mu_gain=150.0),
]


def case_cfg(case):
    kw = dict(autotune=1, alpha=1.0, target_entropy=-float(case["A"]), noise_in_update=0)
    kw.update(case["kw"])
    return B.cfg_dict(case["D"], case["A"], total_timesteps=case["T"], **kw)


threshold = B.threshold


def actor_params(D, A, seed=1, mu_gain=1.0, s_gain=1.0, mu_shift=0.0):
    """Glorot-uniform weights plus a 0.05 normal perturbation on every element, Float32, head of 2A rows; the gains scale the head's μ / s rows, the
    shift is added to the μ rows' biases"""
    rng = np.random.default_rng([seed, 0x5AC])
    parts = []
    for fan_out, fan_in in ((R.H, D), (R.H, R.H), (2 * A, R.H)):
        lim = np.sqrt(6.0 / (fan_in + fan_out))
        parts += [rng.uniform(-lim, lim, fan_out * fan_in), np.zeros(fan_out)]
    p = np.concatenate(parts)
    p = p + 0.05 * rng.standard_normal(p.size)
    o = R.H * D + R.H + R.H * R.H + R.H
    W3 = p[o:o + 2 * A * R.H].reshape((2 * A, R.H), order="F"); b3 = p[o + 2 * A * R.H:]
    W3[:A] *= mu_gain; b3[:A] *= mu_gain; W3[A:] *= s_gain; b3[A:] *= s_gain
    b3[:A] += mu_shift
    p[o:o + 2 * A * R.H] = W3.reshape(-1, order="F")
    return p.astype(np.float32)


def case_params(case):
    """(actor, critic 1, critic 2): the critics are td3_bar's (ddpg_bar's perturbed Glorot nets of two draws)"""
    return (actor_params(case["D"], case["A"], 1, case["mu_gain"], case["s_gain"], case["mu_shift"]), B.case_params(case, seed=1)[1], B.case_params(case, seed=2)[1])


case_transitions = B.case_transitions


# ---------------------------------------------------------------------------------------------------- distances
def _loss_distance(dev, ref):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(dev - ref).max() / np.abs(ref).max())


def distances(losses, arecs, params, log_alpha, ref_losses, ref_arecs, ref_params, ref_log_alpha, D, A):
    """losses: [(global_step, actor_loss, critic_loss)], arecs: [(global_step, alpha, alpha_loss, entropy)], params: (actor, critic1, critic2,
    target_critic1, target_critic2); the logged steps have to be the reference's"""
    steps = [l[0] for l in ref_losses]
    assert [l[0] for l in losses] == steps and [r[0] for r in arecs] == steps and [r[0] for r in ref_arecs] == steps and len(steps) > 0
    out = {name: _loss_distance([l[col] for l in losses], [l[col] for l in ref_losses]) for col, name in ((1, "actor_loss"), (2, "critic_loss"))}
    out["alpha_loss"] = _loss_distance([r[2] for r in arecs], [r[2] for r in ref_arecs])
    sa, sc = R.net_sizes(D, 2 * A), R.net_sizes(D + A, 1)
    for name, dev, rf, sizes in zip(PARAMS, params, ref_params, (sa, sc, sc, sc, sc)):
        out[name] = B.rel_per_array(dev, rf, sizes)
    out["log_alpha"] = float(abs(float(log_alpha) - float(ref_log_alpha)) / max(1.0, abs(float(ref_log_alpha))))
    return out


def load_bars(path=BAR_JSON):
    prof = json.load(open(path))
    return prof["loss_bar"], prof["param_bar"]


def case_loss_bar(name, path=EDGE_BAR_JSON):
    """LOSS_FACTOR x the case's own loss floor: the bar of a hard case, which then loosens no neighbour"""
    return LOSS_FACTOR * json.load(open(path))["cases"][name]["loss_floor"]


def bar_of(name, loss_bar, param_bar=PARAM_BAR):
    return loss_bar if name in LOSSES else param_bar


@contextlib.contextmanager
def patched(**attrs):
    """sac_ref with the given module attributes replaced; restored on exit"""
    saved = []
    try:
        for name, new in attrs.items():
            saved.append((name, getattr(S, name)))
            setattr(S, name, new)
        yield
    finally:
        for name, old in reversed(saved):
            setattr(S, name, old)


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
def _s4():
    return dict(squash_term=lambda y, scale: R.np.log((1.0 - y * y) + S.SQUASH_EPS))


def _s9():
    orig = S.draws

    def draws(seed, gstep, k, act_dim, stream):
        return np.repeat(orig(seed, gstep, 1, act_dim, stream), k, axis=1)
    return dict(draws=draws)


def _live(c):
    """the next-state value reaches the TD target"""
    return case_cfg(c)["gamma"] != 0.0 and c["terminal"] != "all"


# name → (what it mirrors, where it applies, the patch)
MUTANTS = {
    "S1": ("the -alpha·logpi' term is missing from the TD target", _live, lambda: dict(entropy_term=lambda alpha, logp: 0.0 * logp)),
    "S2": ("a' is sampled on state instead of next_state", _live, lambda: dict(next_obs=lambda batch: batch["state"])),
    "S3": ("logpi without the squash term", lambda c: True, lambda: dict(squash_term=lambda y, scale: 0.0 * y)),
    "S4": ("scale omitted inside the log", lambda c: True, _s4),
    "S5": ("the actor gradient always runs through critic 1", lambda c: True, lambda: dict(grad_critic=lambda q1, q2: np.zeros(q1.shape, bool))),
    "S6": ("the direct -alpha/k term of d/dlog_std is missing", lambda c: True, lambda: dict(direct_term=lambda ak: 0.0)),
    "S7": ("log_std is read from head rows 0..A-1", lambda c: True, lambda: dict(head_rows=lambda z, A: (z[:A], z[:A]))),
    "S8": ("stream 0x18 is used in the actor pass", lambda c: True, lambda: dict(actor_stream=lambda: S.S_NEXT)),
    "S9": ("component word c instead of 16·b + c", lambda c: case_cfg(c)["batch_size"] > 1, _s9),
    "S10": ("alpha is read after the alpha step", lambda c: case_cfg(c)["autotune"] == 1,
            lambda: dict(reported_alpha=lambda before, la_after: S.alpha_of(la_after))),
    "S11": ("polyak before the critic step", lambda c: True, lambda: dict(polyak_sources=lambda agent: agent._pre)),
    "S12": ("the alpha step is taken with autotune = 0", lambda c: case_cfg(c)["autotune"] == 0, lambda: dict(alpha_due=lambda autotune: True)),
}

# table → (cases, where its profile goes)
TABLES = {"cases": (CASES, BAR_JSON), "edges": (EDGE_CASES, EDGE_BAR_JSON)}


def applicable(case):
    return [m for m, (_, applies, _) in MUTANTS.items() if applies(case)]


# ---------------------------------------------------------------------------------------------------- one case, measured
def run_ref(case, patch=None):
    """the case through sac_ref (under `patch`, a context manager) → (losses, alpha records, params, log_alpha, stats)"""
    d = case_cfg(case)
    with (patch if patch is not None else contextlib.nullcontext()):
        ref = S.SAC(d, *case_params(case))
        ref.run_transitions(case_transitions(case))
    return ref.losses, ref.alpha_records, ref.params(), ref.log_alpha[0], {s: int(getattr(ref, s)) for s in STATS}


def variant(case, what, base):
    """what: ("jitter", seed) or a mutant's name → the distances of that variant from the base run"""
    patch = B.jitter(what[1]) if isinstance(what, tuple) else patched(**MUTANTS[what][2]())
    v = run_ref(case, patch)
    return distances(v[0], v[1], v[2], v[3], base[0], base[1], base[2], base[3], case["D"], case["A"])


def measure_floor(case, base=None):
    """→ {"floor": {observable: max over the jitter seeds}, "stats": the base run's}"""
    base = run_ref(case) if base is None else base
    floors = [variant(case, ("jitter", s), base) for s in JITTER_SEEDS]
    return {"floor": {o: max(f[o] for f in floors) for o in OBSERVABLES}, "stats": base[4]}


def measure(case):
    """→ measure_floor's two and "mutants": {name: {observable: distance}}"""
    base = run_ref(case)
    return dict(measure_floor(case, base), mutants={m: variant(case, m, base) for m in applicable(case)})


def mutant_ratio(dist, loss_bar, param_bar=PARAM_BAR):
    """the largest distance / bar over the nine observables"""
    return max(dist[o] / bar_of(o, loss_bar, param_bar) for o in OBSERVABLES)


def edge_met(name, stats):
    """the edge a case is in the table for, on the reference's own counters"""
    if name == "saturated":
        return stats["n_y_one"] >= 0.5 * stats["n_samples"] and stats["n_y_near"] >= 0.02 * stats["n_samples"]
    if name == "logstd_ends":
        return stats["n_ls_low"] >= 0.05 * stats["n_samples"] and stats["n_ls_high"] >= 0.05 * stats["n_samples"]
    return True
