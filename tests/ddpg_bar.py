"""What the DDPG parity tests share (tests/test_ddpg_bar_cpu.py, tests/test_gpu_ddpg.py, tests/test_gpu_ddpg_edges.py, scripts/ddpg_bar.py): the ONE
case table, the transition generator, the per-array distances, the candidate counter of the minibatch draw — and the two instruments that say what
a bar on those distances is worth: a twin of tests/ddpg_ref.py whose transcendental functions are jittered in their last bits (the FLOOR: how far
two correct implementations may be apart), and one-line wrong versions of it (the MUTANTS: how far a subtly wrong one is). Neither changes
ddpg_ref: both patch the imported module for the length of one run and put it back.

The bars. loss_bar = LOSS_FACTOR x the largest loss floor over the table (scripts/ddpg_bar.py measures it into profiles/ddpg_bar.json); PARAM_BAR =
2^-21 relative to each array's largest magnitude = four Float32 ulps of the largest element: the Float64 values in front of a Float32 projection
agree to about 1e-16, so a projection flips with a probability of about 1e-9 per element and step, and a flip costs one ulp."""
import contextlib
import json
import os

import numpy as np

import ddpg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_JSON = os.path.join(ROOT, "profiles", "ddpg_bar.json")
OLD_BAR = 1e-5                    # the project's Float32 bar, still asserted
PARAM_BAR = 2.0 ** -21
LOSS_FACTOR = 32                  # the loss is a mean of k terms with independent last-bit errors: the tail three jitter draws do not sample
MUTANT_FACTOR = 10                # every mutant has to move an observable past this many bars
JITTER_ULP = {"exp": 2, "log": 2, "cos": 2}   # a device cos may be 2 ulp off; one amplitude for the three
JITTER_SEEDS = (1, 2, 3)
OBSERVABLES = ("actor_loss", "critic_loss", "actor", "critic", "target_actor", "target_critic")
LOSSES, PARAMS = OBSERVABLES[:2], OBSERVABLES[2:]


# ---------------------------------------------------------------------------------------------------- the case table
def _case(name, D, A, T, edge, terminal="some", **kw):
    return dict(name=name, D=D, A=A, T=T, edge=edge, terminal=terminal, kw=kw)


# T transitions are fed; the updates are the steps past max(min_buff_size, warmup_steps). Every case keeps the update noise on (the noise streams
# are part of what is compared) except where the edge is its absence.
CASES = [
    _case("d1a1_k2", 1, 1, 150, "smallest net; NI = 2", batch_size=2, min_buff_size=10, warmup_steps=5),
    _case("ni64_k30", 48, 16, 110, "NI exactly 64; one full unrolled round", batch_size=30, min_buff_size=40, warmup_steps=35),
    _case("ni65_k31", 49, 16, 110, "one element in the second pass of the 64-stride loop; remainder 1", batch_size=31, min_buff_size=40, warmup_steps=35),
    _case("d64a1_k7", 64, 1, 100, "the action alone sits in the second pass", batch_size=7, min_buff_size=10, warmup_steps=5),
    _case("d64a16_k61", 64, 16, 140, "both maxima; two unrolled rounds + 1", batch_size=61, min_buff_size=70, warmup_steps=65),
    _case("k120_default", 3, 1, 210, "the reference's default batch, tau and gamma", batch_size=120, min_buff_size=130, warmup_steps=125),
    _case("kmax_ring_eq_batch", 3, 1, 1038, "maximum k; k = n on every draw; the ring wraps", batch_size=1024, buffer_size=1024, min_buff_size=1030,
          warmup_steps=1025),
    _case("ring200_full", 17, 6, 225, "k = n; several sampling rounds; the ring wraps", batch_size=200, buffer_size=200, min_buff_size=205,
          warmup_steps=201),
    _case("ring200_k199", 17, 6, 235, "k = n - 1: which slot a multi-round draw leaves out depends on every round's counters", batch_size=199,
          buffer_size=200, min_buff_size=205, warmup_steps=201),
    # hyper-parameter edges at (3, 1), k = 7
    _case("tau1", 3, 1, 110, "tau = 1: the targets are the online nets", tau=1.0),
    _case("gamma0", 3, 1, 110, "gamma = 0: the TD target is the reward", gamma=0.0),
    _case("all_terminal", 3, 1, 110, "every transition terminal", terminal="all"),
    _case("none_terminal", 3, 1, 110, "no transition terminal", terminal="none"),
    _case("noise0", 3, 1, 110, "exploration_noise = 0 with noise_in_update = 1", exploration_noise=0.0),
    _case("logfreq7", 3, 1, 110, "log_frequency = 7 in the transition-fed mode", log_frequency=7),
]
CASE = {c["name"]: c for c in CASES}
MULTI_ROUND = ("kmax_ring_eq_batch", "ring200_full", "ring200_k199")      # at least one draw needs more than one round of 1024 candidates
CHEAPEST = ("gamma0", "tau1")                             # what tests/test_ddpg_bar_cpu.py recomputes: the shortest reference runs


def cfg_dict(D, A, **kw):
    d = dict(total_timesteps=300, buffer_size=1000, min_buff_size=10, batch_size=7, warmup_steps=5, log_frequency=1, lr=1e-3, tau=0.005, gamma=0.99,
             exploration_noise=0.1, obs_dim=D, act_dim=A, max_steps=200, act_low=-2.0, act_high=2.0, noise_in_update=1, seed=0x5EED)
    d.update(kw)
    return d


def case_cfg(case):
    return cfg_dict(case["D"], case["A"], total_timesteps=case["T"], **case["kw"])


def threshold(d):
    return max(d["min_buff_size"], d["warmup_steps"])


def case_params(case, seed=1):
    """Glorot-uniform weights plus a 0.05 normal perturbation on every element (non-zero biases), Float32, from numpy alone"""
    rng = np.random.default_rng(seed)
    out = []
    for n_in, n_out in ((case["D"], case["A"]), (case["D"] + case["A"], 1)):
        parts = []
        for fan_out, fan_in in ((R.H, n_in), (R.H, R.H), (n_out, R.H)):
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            parts += [rng.uniform(-lim, lim, fan_out * fan_in), np.zeros(fan_out)]
        p = np.concatenate(parts)
        out.append((p + 0.05 * rng.standard_normal(p.size)).astype(np.float32))
    return tuple(out)


def transitions(D, A, n, seed, terminal="some"):
    """(obs, action, reward, next_obs, terminal) tuples; terminal: "some" (one in ten), "all" or "none" — the other draws are the same for all three"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        s, a, r, ns, t = rng.standard_normal(D), rng.uniform(-2, 2, A), float(rng.standard_normal()), rng.standard_normal(D), bool(rng.random() < 0.1)
        out.append((s, a, r, ns, True if terminal == "all" else False if terminal == "none" else t))
    return out


def case_transitions(case, seed=7):
    return transitions(case["D"], case["A"], case["T"], seed, case["terminal"])


# ---------------------------------------------------------------------------------------------------- distances
def rel_per_array(dev, ref, sizes):
    """max over the arrays of max |dev - ref| / max |ref|"""
    worst, o = 0.0, 0
    for n in sizes:
        a, b = np.asarray(dev[o:o + n], np.float64), np.asarray(ref[o:o + n], np.float64); o += n
        worst = max(worst, np.abs(a - b).max() / np.abs(b).max())
    return float(worst)


def distances(losses, params, ref_losses, ref_params, D, A):
    """losses: [(global_step, actor_loss, critic_loss)], params: (actor, critic, target_actor, target_critic) → {observable: distance}; the logged
    steps have to be the reference's"""
    assert [l[0] for l in losses] == [l[0] for l in ref_losses] and len(losses) > 0
    out = {}
    for col, name in ((1, "actor_loss"), (2, "critic_loss")):
        d = np.array([l[col] for l in losses]); r = np.array([l[col] for l in ref_losses])
        out[name] = float(np.abs(d - r).max() / np.abs(r).max())
    for name, dev, rf, sizes in zip(PARAMS, params, ref_params, (R.net_sizes(D, A), R.net_sizes(D + A, 1)) * 2):
        out[name] = rel_per_array(dev, rf, sizes)
    return out


def ref_params(ref):
    return (ref.actor, ref.critic, ref.actor_t, ref.critic_t)


def load_bars():
    """→ (loss_bar, param_bar) as profiles/ddpg_bar.json states them"""
    prof = json.load(open(BAR_JSON))
    return prof["loss_bar"], prof["param_bar"]


def bar_of(name, loss_bar, param_bar=PARAM_BAR):
    return loss_bar if name in LOSSES else param_bar


# ---------------------------------------------------------------------------------------------------- the draw
def candidates_needed(seed, gstep, n, k):
    """How many candidates R.sample_indices(seed, gstep, n, k) looks at before it holds k distinct slots (the device draws them 1024 at a time)"""
    seen, base = set(), 0
    while True:
        x = R.philox(np.arange(base, base + 1024), gstep & R.M32, gstep >> 32, R.S_SAMPLE, seed & R.M32, seed >> 32)[0]
        for i, j in enumerate(((x * np.uint64(n)) >> np.uint64(32)).tolist()):
            seen.add(j)
            if len(seen) == k:
                return base + i + 1
        base += 1024


def case_candidates(case):
    """the candidate counts of every draw of the case"""
    d = case_cfg(case)
    return [candidates_needed(d["seed"], g, min(g, d["buffer_size"]), d["batch_size"]) for g in range(threshold(d) + 1, case["T"] + 1)]


# ---------------------------------------------------------------------------------------------------- patching ddpg_ref for one run
@contextlib.contextmanager
def patched(**attrs):
    """ddpg_ref with the given module attributes ("Adam.step" reaches into the class) replaced; restored on exit"""
    saved = []
    try:
        for name, new in attrs.items():
            obj = R
            *path, last = name.split(".")
            for p in path:
                obj = getattr(obj, p)
            saved.append((obj, last, getattr(obj, last)))
            setattr(obj, last, new)
        yield
    finally:
        for obj, last, old in reversed(saved):
            setattr(obj, last, old)


class JitterNumpy:
    """numpy as ddpg_ref sees it, with every exp / log / cos result moved by a seeded random integer in -amp..+amp ulp"""

    def __init__(self, seed, amp=JITTER_ULP):
        self._rng, self._amp = np.random.default_rng(seed), amp

    def __getattr__(self, name):
        return getattr(np, name)

    def _jitter(self, y, amp):
        y = np.asarray(y, np.float64)
        n = self._rng.integers(-amp, amp + 1, y.shape).astype(np.float64)
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(y) & (y != 0.0), y + n * np.spacing(np.abs(y)), y)

    def exp(self, x):
        return self._jitter(np.exp(x), self._amp["exp"])

    def log(self, x):
        return self._jitter(np.log(x), self._amp["log"])

    def cos(self, x):
        return self._jitter(np.cos(x), self._amp["cos"])


def jitter(seed):
    return patched(np=JitterNumpy(seed))


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
def _last_two(store, item):
    store.append(item)
    del store[:-2]


def _m1():                                                 # td = reward + gamma * next_q, the (1 - terminal) factor lost
    orig = R.td_target

    def td_target(actor_t, critic_t, D, A, batch, gamma, noise_t):
        return orig(actor_t, critic_t, D, A, dict(batch, terminal=np.zeros_like(batch["terminal"])), gamma, noise_t)
    return dict(td_target=td_target)


def _m2():                                                 # dq = -4 * diff / k
    orig = R.critic_loss_grad

    def critic_loss_grad(critic, D, A, batch, td):
        loss, g = orig(critic, D, A, batch, td)
        return loss, 2.0 * g
    return dict(critic_loss_grad=critic_loss_grad)


def _m3():                                                 # ddpg_normal(seed, 0, ...) instead of (seed, lane, ...)
    orig = R.normal

    def normal(seed, comps, gstep, stream):
        return orig(seed, np.zeros_like(comps), gstep, stream)
    return dict(normal=normal)


def _m4():                                                 # `if (lane < NI)` instead of the 64-stride loop that fills xs and X
    orig = R.critic_loss_grad

    def critic_loss_grad(critic, D, A, batch, td):
        action = np.array(batch["action"], np.float64)
        action[max(0, 64 - D):] = 0.0                      # rows >= 64 of vcat(state, action) are action rows: obs_dim <= 64
        return orig(critic, D, A, dict(batch, action=action), td)
    return dict(critic_loss_grad=critic_loss_grad)


def _m5():                                                 # c = r / 64, j = r % 64 in the actor's W3 gradient
    orig = R.actor_loss_grad

    def actor_loss_grad(actor, critic, D, A, batch, noise_a):
        loss, g = orig(actor, critic, D, A, batch, noise_a)
        o = sum(R.net_sizes(D, A)[:4])
        g = g.copy()
        g[o:o + A * R.H] = g[o:o + A * R.H].reshape((A, R.H), order="F").reshape(-1, order="C")
        return loss, g
    return dict(actor_loss_grad=actor_loss_grad)


def _m6():                                                 # `b < k - 1` in every loop over the samples
    def _sum_samples(M):
        acc = np.zeros(M.shape[:-1], np.float64)
        for b in range(M.shape[-1] - 1):
            acc = acc + M[..., b]
        return acc
    return dict(_sum_samples=_sum_samples)


def _remembering_adam(store):
    orig = R.Adam.step

    def step(self, p, g64):
        new = orig(self, p, g64)
        _last_two(store, (new, p))                         # the two nets' latest steps
        return new
    return step


def _before_step(store, w):
    for new, old in store:
        if new is w:
            return old
    raise AssertionError("not the result of an Adam step")


def _m7():                                                 # t[p] = tau * w[p] + ... read before w[p] = wi
    orig, store = R.polyak, []

    def polyak(t, s, tau):
        return orig(t, _before_step(store, s), tau)
    return {"Adam.step": _remembering_adam(store), "polyak": polyak}


def _m8():                                                 # the actor pass launched before the critic step
    orig, store = R.actor_loss_grad, []

    def actor_loss_grad(actor, critic, D, A, batch, noise_a):
        return orig(actor, _before_step(store, critic), D, A, batch, noise_a)
    return {"Adam.step": _remembering_adam(store), "actor_loss_grad": actor_loss_grad}


def _m9():                                                 # S_TARGET in the actor pass
    orig = R.normal

    def normal(seed, comps, gstep, stream):
        return orig(seed, comps, gstep, R.S_TARGET if stream == R.S_ACTOR else stream)
    return dict(normal=normal)


def _m10():                                                # the second round of candidates starts at the wrong counter
    def sample_indices(seed, gstep, n, k):
        out, seen, base = [], set(), 0
        while len(out) < k:
            x = R.philox(np.arange(base, base + 1024), gstep & R.M32, gstep >> 32, R.S_SAMPLE, seed & R.M32, seed >> 32)[0]
            for j in ((x * np.uint64(n)) >> np.uint64(32)).tolist():
                if j not in seen:
                    seen.add(j); out.append(j)
                    if len(out) == k:
                        break
            base += 2048
        return np.array(out, np.int32)
    return dict(sample_indices=sample_indices)


def _noisy(c):
    d = case_cfg(c)
    return d["noise_in_update"] != 0 and d["exploration_noise"] != 0.0


# name → (what it mirrors, the cases it applies to, the patch). A mutant applies where the line it breaks does something: the hyper-parameter
# edges switch some lines off (gamma = 0 and terminal-free data make the terminal factor inert, zero noise makes the noise streams inert).
MUTANTS = {
    "M1": ("the terminal flag is ignored in the TD target", lambda c: case_cfg(c)["gamma"] != 0.0 and c["terminal"] != "none", _m1),
    "M2": ("the critic gradient is scaled x2", lambda c: True, _m2),
    "M3": ("every noise component draws component 0", lambda c: c["A"] > 1 and _noisy(c), _m3),
    "M4": ("critic inputs and W1-gradient columns at index >= 64 are dropped", lambda c: c["D"] + c["A"] > 64, _m4),
    "M5": ("the actor W3 gradient has (c, j) transposed", lambda c: c["A"] > 1, _m5),
    "M6": ("the last sample of the batch is left out of every sum over samples", lambda c: case_cfg(c)["batch_size"] > 1, _m6),
    "M7": ("polyak mixes the pre-step weights", lambda c: True, _m7),
    "M8": ("the actor pass reads the critic from before its step", lambda c: True, _m8),
    "M9": ("the target noise and the actor-loss noise share one stream", _noisy, _m9),
    # restarting at counter 0 proper would only offer the first round's candidates again, all taken: the draw would never end (a hang, not a wrong
    # number). The wrong-number form of the same slip is a second round that starts at another counter than 1024: here 2048. Where k = n the draw
    # is a permutation of the whole ring and a wrong counter only reorders the sums, which no bar above the rounding can see: k < n is needed.
    "M10": ("the second round of sampling candidates starts at the wrong counter",
            lambda c: c["name"] in MULTI_ROUND and case_cfg(c)["batch_size"] < case_cfg(c)["buffer_size"], _m10),
}


def applicable(case):
    return [m for m, (_, applies, _) in MUTANTS.items() if applies(case)]


# ---------------------------------------------------------------------------------------------------- one case, measured
def run_ref(case, patch=None):
    """the case through ddpg_ref (under `patch`, a context manager) → (losses, params)"""
    d = case_cfg(case)
    actor, critic = case_params(case)
    trs = case_transitions(case)
    with (patch if patch is not None else contextlib.nullcontext()):
        ref = R.DDPG(d, actor, critic)
        ref.run_transitions(trs)
    return ref.losses, ref_params(ref)


def variant(case, what, base=None):
    """what: "base", ("jitter", seed) or a mutant's name → the base run itself, or the distances of that variant from it"""
    if what == "base":
        return run_ref(case)
    base = base if base is not None else run_ref(case)
    patch = jitter(what[1]) if isinstance(what, tuple) else patched(**MUTANTS[what][2]())
    losses, params = run_ref(case, patch)
    return distances(losses, params, base[0], base[1], case["D"], case["A"])


def measure(case):
    """→ {"floor": {observable: max over the jitter seeds}, "mutants": {name: {observable: distance}}}"""
    base = run_ref(case)
    floors = [variant(case, ("jitter", s), base) for s in JITTER_SEEDS]
    return {"floor": {o: max(f[o] for f in floors) for o in OBSERVABLES}, "mutants": {m: variant(case, m, base) for m in applicable(case)}}


def mutant_ratio(dist, loss_bar, param_bar=PARAM_BAR):
    """the largest distance / bar over the six observables"""
    return max(dist[o] / bar_of(o, loss_bar, param_bar) for o in OBSERVABLES)
