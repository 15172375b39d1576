"""What the TD3 parity tests share (tests/test_td3_cpu.py, tests/test_gpu_td3.py, scripts/td3_bar.py), after tests/ddpg_bar.py: the ONE case table of
what TD3 adds to DDPG, the per-array distances over its eight observables, and the two instruments that say what a bar on them is worth — the
jittered twin of the reference (ddpg_bar.JitterNumpy at the same amplitude and seeds: the FLOOR) and one-line wrong versions of tests/td3_ref.py
(the MUTANTS). Transitions, parameters, the config dict and the bars' constants are ddpg_bar's.

The bars. loss_bar = LOSS_FACTOR x the largest loss floor over THIS table (scripts/td3_bar.py measures it into profiles/td3_bar.json); PARAM_BAR =
2^-21 per array and OLD_BAR = 1e-5 as for DDPG.

A second table, EDGE_CASES (tests/test_td3_edges_cpu.py, tests/test_gpu_td3_edges.py, scripts/td3_bar.py --table edges), holds the batch, ring and
logging edges with a loss bar of its own in profiles/td3_edges_bar.json, and two more mutants that only those edges can see."""
import contextlib
import json
import os

import numpy as np

import ddpg_bar as B
import ddpg_ref as R
import td3_ref as T

BAR_JSON = os.path.join(B.ROOT, "profiles", "td3_bar.json")
EDGE_BAR_JSON = os.path.join(B.ROOT, "profiles", "td3_edges_bar.json")
OLD_BAR, PARAM_BAR, LOSS_FACTOR, MUTANT_FACTOR, JITTER_ULP, JITTER_SEEDS = B.OLD_BAR, B.PARAM_BAR, B.LOSS_FACTOR, B.MUTANT_FACTOR, B.JITTER_ULP, B.JITTER_SEEDS
LOSSES = ("actor_loss", "critic_loss")
PARAMS = ("actor", "critic1", "critic2", "target_actor", "target_critic1", "target_critic2")
OBSERVABLES = LOSSES + PARAMS
STATS = ("n_actor_steps", "n_noise", "n_noise_clipped", "n_target_actions", "n_target_clamped")


# ---------------------------------------------------------------------------------------------------- the case table
def _case(name, D, A, T_, edge, terminal="some", **kw):
    return dict(name=name, D=D, A=A, T=T_, edge=edge, terminal=terminal, kw=kw)


# Updates are the steps past max(min_buff_size, warmup_steps) = 10 at (3, 1): g = 11..T. The actor steps where g % policy_delay == 0.
CASES = [
    _case("d1a1_k2", 1, 1, 150, "smallest net and batch: two blocks of two waves", batch_size=2, min_buff_size=10, warmup_steps=5),
    _case("ni65_k31", 49, 16, 110, "NI = 65: one element in the second pass of each wave's 64-stride loop; 16 noise components per sample",
          batch_size=31, min_buff_size=40, warmup_steps=35),
    _case("d64a16_k61", 64, 16, 140, "both maxima; component words up to 16·60 + 15", batch_size=61, min_buff_size=70, warmup_steps=65),
    # the TD3 edges at (3, 1), k = 7
    _case("delay1", 3, 1, 110, "policy_delay = 1: the actor and the targets move on every update", policy_delay=1),
    _case("delay2_on", 3, 1, 110, "policy_delay = 2, the last update (g = 110) is an actor step", policy_delay=2),
    _case("delay2_off", 3, 1, 109, "policy_delay = 2, the last update (g = 109) is not", policy_delay=2),
    _case("delay3_on", 3, 1, 108, "policy_delay = 3, the last update (g = 108) is an actor step", policy_delay=3),
    _case("delay3_off", 3, 1, 110, "policy_delay = 3, the last update (g = 110) is not", policy_delay=3),
    _case("delay_never", 3, 1, 110, "policy_delay above every step: the actor and all three targets keep their initial values", policy_delay=1000),
    _case("clip0", 3, 1, 110, "noise_clip = 0: the smoothing noise is clipped away", noise_clip=0.0),
    _case("noise1_clip05", 3, 1, 110, "policy_noise = 1, noise_clip = 0.5: P(|z| > 0.5) = 0.62 of the draws are clipped", policy_noise=1.0, noise_clip=0.5),
    _case("bounds", 3, 1, 110, "act_low = -1, act_high = 0.5: the clamp of the target action binds", act_low=-1.0, act_high=0.5),
    _case("gamma0", 3, 1, 110, "gamma = 0: the TD target is the reward", gamma=0.0),
    _case("tau1", 3, 1, 110, "tau = 1: on an actor step the targets become the online nets", tau=1.0),
    _case("all_terminal", 3, 1, 110, "every transition terminal", terminal="all"),
]
CASE = {c["name"]: c for c in CASES}
CHEAPEST = ("gamma0", "delay2_off")                      # what tests/test_td3_cpu.py recomputes

# The second table: what the first leaves out. Everything td3_critic_kernel and td3_critic_step add is indexed by the batch position b — the [2][k]
# blocks of the two critic passes, the component word 16·b + c of the smoothing draw — and the first table stops at k = 61, never lets the ring wrap
# and logs every step. Measured by scripts/td3_bar.py --table edges into profiles/td3_edges_bar.json, with a loss bar of its own.
EDGE_CASES = [
    _case("ni64_k30", 48, 16, 110, "NI exactly 64; one full unrolled round of 30", batch_size=30, min_buff_size=40, warmup_steps=35),
    _case("d64a1_k7", 64, 1, 100, "the action alone sits in the second pass of the 64-stride loop", batch_size=7, min_buff_size=10, warmup_steps=5),
    _case("k65", 3, 1, 150, "the first batch position past 63; noise word 1024", batch_size=65, min_buff_size=70, warmup_steps=66),
    _case("k120_default", 3, 1, 210, "the reference's default batch; four unrolled rounds", batch_size=120, min_buff_size=130, warmup_steps=125),
    _case("kmax_ring_eq_batch", 3, 1, 1038, "largest k; k = n; the ring wraps; 4 actor steps in 8 updates", batch_size=1024, buffer_size=1024,
          min_buff_size=1030, warmup_steps=1025),
    _case("kmax_a16", 17, 16, 1034, "largest k at act_dim 16: noise words up to 16383; policy_noise = 1 so that clip and clamp bind", batch_size=1024,
          buffer_size=1024, min_buff_size=1030, warmup_steps=1025, policy_noise=1.0),
    _case("ring200_full", 17, 6, 225, "k = n with several sampling rounds; the ring wraps", batch_size=200, buffer_size=200, min_buff_size=205,
          warmup_steps=201),
    _case("ring200_k199", 17, 6, 235, "odd k: the second critic's half starts at 199·64", batch_size=199, buffer_size=200, min_buff_size=205,
          warmup_steps=201),
    _case("none_terminal", 3, 1, 110, "no transition is terminal", terminal="none"),
    _case("logfreq7_delay3", 3, 1, 110, "log_frequency = 7, policy_delay = 3: records at 14, 21, ...; only every third is an actor step",
          log_frequency=7, policy_delay=3),
    _case("logfreq4_delay3", 3, 1, 110, "log_frequency = 4, policy_delay = 3: the first record (g = 12) is an actor step, the second (g = 16) is not",
          log_frequency=4, policy_delay=3),
    _case("bounds_a6", 17, 6, 110, "act_low = -1, act_high = 0.5, policy_noise = 1: clip and clamp bind on more than half of a six-wide action",
          act_low=-1.0, act_high=0.5, policy_noise=1.0),
]
EDGE_CASE = {c["name"]: c for c in EDGE_CASES}
EDGE_CHEAPEST = ("none_terminal", "logfreq7_delay3")           # what tests/test_td3_edges_cpu.py recomputes: the shortest reference runs
EDGE_MULTI_ROUND = ("kmax_ring_eq_batch", "ring200_full", "ring200_k199")   # at least one draw needs more than one round of 1024 candidates


def case_cfg(case):
    kw = dict(policy_delay=2, policy_noise=0.2, noise_clip=0.5, noise_in_update=0)
    kw.update(case["kw"])
    return B.cfg_dict(case["D"], case["A"], total_timesteps=case["T"], **kw)


threshold = B.threshold


def case_params(case):
    """(actor, critic 1, critic 2): ddpg_bar's perturbed Glorot nets; critic 2 is the critic of a second draw"""
    actor, critic1 = B.case_params(case, seed=1)
    return actor, critic1, B.case_params(case, seed=2)[1]


case_transitions = B.case_transitions
case_candidates = B.case_candidates                      # reads the case through ddpg_bar.case_cfg: only fields the two share


# ---------------------------------------------------------------------------------------------------- distances
def _loss_distance(dev, ref):
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max()
    if top == 0.0:                                        # no actor step yet: the logged actor_loss is exactly 0.0; the distance is absolute
        return float(np.abs(dev).max())
    return float(np.abs(dev - ref).max() / top)


def distances(losses, params, ref_losses, ref_params, D, A):
    """losses: [(global_step, actor_loss, critic_loss)], params: (actor, critic1, critic2, target_actor, target_critic1, target_critic2)"""
    assert [l[0] for l in losses] == [l[0] for l in ref_losses] and len(losses) > 0
    out = {name: _loss_distance([l[col] for l in losses], [l[col] for l in ref_losses]) for col, name in ((1, "actor_loss"), (2, "critic_loss"))}
    sa, sc = R.net_sizes(D, A), R.net_sizes(D + A, 1)
    for name, dev, rf, sizes in zip(PARAMS, params, ref_params, (sa, sc, sc) * 2):
        out[name] = B.rel_per_array(dev, rf, sizes)
    return out


def load_bars(path=BAR_JSON):
    prof = json.load(open(path))
    return prof["loss_bar"], prof["param_bar"]


def bar_of(name, loss_bar, param_bar=PARAM_BAR):
    return loss_bar if name in LOSSES else param_bar


# ---------------------------------------------------------------------------------------------------- patching td3_ref / ddpg_ref for one run
@contextlib.contextmanager
def patched(**attrs):
    """td3_ref with the given module attributes replaced ("R.x" reaches ddpg_ref's x); restored on exit"""
    saved = []
    try:
        for name, new in attrs.items():
            obj, last = (R, name[2:]) if name.startswith("R.") else (T, name)
            saved.append((obj, last, getattr(obj, last)))
            setattr(obj, last, new)
        yield
    finally:
        for obj, last, old in reversed(saved):
            setattr(obj, last, old)


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
def _t1():                                                 # q2 > q1 ? q2 : q1
    return dict(next_q=lambda q1, q2: np.where(q2 > q1, q2, q1))


def _t2():                                                 # the noise is not clipped
    return dict(smoothing_noise=lambda z, policy_noise, noise_clip: policy_noise * z)


def _t3():                                                 # the target action is not clamped to the action bounds
    return dict(target_action=lambda y3, noise, lo, hi: y3 * 2.0 + noise)


def _t4():                                                 # component word c instead of 16·b + c: every sample draws position 0's noise
    orig = T.smoothing_draws

    def smoothing_draws(seed, gstep, k, act_dim):
        return np.repeat(orig(seed, gstep, 1, act_dim), k, axis=1)
    return dict(smoothing_draws=smoothing_draws)


def _t5():                                                 # the actor steps on every update
    return dict(actor_due=lambda g, delay: True)


def _t6():                                                 # the targets are polyak'd on every update
    return dict(targets_due=lambda g, delay: True)


def _t7():                                                 # critic 2's backward starts from critic 1's td − q
    def critic2_cotangent_td(td, critic1, critic2, D, A, batch):
        X = np.vstack([batch["state"], batch["action"]])
        return (td - R.critic_forward(critic1, D + A, X)[2]) + R.critic_forward(critic2, D + A, X)[2]
    return dict(critic2_cotangent_td=critic2_cotangent_td)


def _t8():                                                 # critic 2 reads and advances critic 1's β powers
    def critic2_step(agent, grad):
        agent.opt_c2.bp = agent.opt_c.bp
        new = agent.opt_c2.step(agent.critic2, grad)
        agent.opt_c.bp = agent.opt_c2.bp
        return new
    return dict(critic2_step=critic2_step)


def _t9():                                                 # the actor loss runs through critic 2
    return dict(actor_loss_critic=lambda agent: agent.critic2)


def _live(c):
    """the next-state value reaches the TD target"""
    return case_cfg(c)["gamma"] != 0.0 and c["terminal"] != "all"


# name → (what it mirrors, where it applies given the case and the reference's own statistics of it, the patch). A mutant applies where the line it
# breaks does something.
MUTANTS = {
    "T1": ("max instead of min of the two target critics", lambda c, st: _live(c), _t1),
    "T2": ("the smoothing noise is not clipped", lambda c, st: _live(c) and st["n_noise_clipped"] > 0, _t2),
    "T3": ("the target action is not clamped to the action bounds", lambda c, st: _live(c) and st["n_target_clamped"] > 0, _t3),
    "T4": ("every sample draws batch position 0's noise",
           lambda c, st: _live(c) and case_cfg(c)["batch_size"] > 1 and case_cfg(c)["policy_noise"] > 0 and case_cfg(c)["noise_clip"] > 0, _t4),
    "T5": ("the actor steps on every update", lambda c, st: case_cfg(c)["policy_delay"] > 1, _t5),
    "T6": ("the targets are polyak'd on every update", lambda c, st: case_cfg(c)["policy_delay"] > 1, _t6),
    "T7": ("critic 2 is trained on critic 1's cotangent", lambda c, st: True, _t7),
    "T8": ("critic 2 shares critic 1's beta powers", lambda c, st: True, _t8),
    "T9": ("the actor loss runs through critic 2", lambda c, st: st["n_actor_steps"] > 0, _t9),
}


def _t10():                                                # the component word wraps at 1024: batch position 64 redraws position 0's noise
    def smoothing_draws(seed, gstep, k, act_dim):
        comps = (16 * np.arange(k)[None, :] + np.arange(act_dim)[:, None]) % 1024
        return R.normal(seed, comps, gstep, T.S_SMOOTH)
    return dict(smoothing_draws=smoothing_draws)


def _t11():                                                # the grid of the critics' polyak is one block short: the last 2·nc mod 64 = 2 elements stay
    orig = T.polyak_targets

    def polyak_targets(agent, tau):
        kept = agent.critic2_t[-2:].copy()
        orig(agent, tau)
        agent.critic2_t[-2:] = kept
    return dict(polyak_targets=polyak_targets)


def _noise_on(c):
    return _live(c) and case_cfg(c)["policy_noise"] > 0 and case_cfg(c)["noise_clip"] > 0


# measured on EDGE_CASES only, together with T1 to T9: T10 is exactly the reference wherever k <= 64, so the first table cannot see it
EDGE_MUTANTS = {
    "T10": ("the component word of the smoothing draw wraps at 1024", lambda c, st: _noise_on(c) and case_cfg(c)["batch_size"] > 64, _t10),
    "T11": ("the last partial block of the critics' polyak is dropped", lambda c, st: st["n_actor_steps"] > 0, _t11),
}
ALL_MUTANTS = {**MUTANTS, **EDGE_MUTANTS}

# table → (cases, the mutants measured on it, where its profile goes)
TABLES = {"cases": (CASES, MUTANTS, BAR_JSON), "edges": (EDGE_CASES, ALL_MUTANTS, EDGE_BAR_JSON)}


def applicable(case, stats, mutants=MUTANTS):
    return [m for m, (_, applies, _) in mutants.items() if applies(case, stats)]


# ---------------------------------------------------------------------------------------------------- one case, measured
def run_ref(case, patch=None):
    """the case through td3_ref (under `patch`, a context manager) → (losses, params, stats)"""
    d = case_cfg(case)
    with (patch if patch is not None else contextlib.nullcontext()):
        ref = T.TD3(d, *case_params(case))
        ref.run_transitions(case_transitions(case))
    return ref.losses, ref.params(), {s: int(getattr(ref, s)) for s in STATS}


def variant(case, what, base):
    """what: ("jitter", seed) or a mutant's name → the distances of that variant from the base run"""
    patch = B.jitter(what[1]) if isinstance(what, tuple) else patched(**ALL_MUTANTS[what][2]())
    losses, params, _ = run_ref(case, patch)
    return distances(losses, params, base[0], base[1], case["D"], case["A"])


def measure(case, mutants=MUTANTS):
    """→ {"floor": {observable: max over the jitter seeds}, "mutants": {name: {observable: distance}}, "stats": the base run's}"""
    base = run_ref(case)
    floors = [variant(case, ("jitter", s), base) for s in JITTER_SEEDS]
    return {"floor": {o: max(f[o] for f in floors) for o in OBSERVABLES}, "stats": base[2],
            "mutants": {m: variant(case, m, base) for m in applicable(case, base[2], mutants)}}


def mutant_ratio(dist, loss_bar, param_bar=PARAM_BAR):
    """the largest distance / bar over the eight observables"""
    return max(dist[o] / bar_of(o, loss_bar, param_bar) for o in OBSERVABLES)
