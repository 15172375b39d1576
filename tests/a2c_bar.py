"""What the A2C parity tests share (tests/test_a2c_bar_cpu.py, tests/test_gpu_a2c_edges.py, scripts/a2c_bar.py): the ONE case table, the inputs of every
update of a case as the C oracle (oracle/a2c_oracle.c) plays it, the per-array distances, and the two instruments that say what a bar on those
distances is worth, as tests/ddpg_bar.py does for DDPG: a twin of tests/a2c_ref.py whose exp and log are jittered in their last bits (the FLOOR) and
one-line wrong versions of it (the MUTANTS). Neither changes a2c_ref: both patch the imported module for the length of one run and put it back.

The bars. loss_bar = LOSS_FACTOR x the largest loss floor over the table (scripts/a2c_bar.py measures it into profiles/a2c_bar.json); PARAM_BAR = 2^-21
relative to each array's largest magnitude = four Float32 ulps of the largest element, for the Float32 gradients and for the parameters after the
step: the Float64 sums in front of the Float32 projection agree to about 1e-15, so a projection flips rarely, and a flip costs one ulp.

An update's inputs. The loop trains at an episode end (a2c.jl:74-75), inside the call that takes the episode's last step, and clears the buffer after:
the batch is never visible from outside. It is rebuilt as tests/test_a2c_oracle.py::test_loop_invariants does: a second oracle stops one step before
the update, its buffer is the batch without the last sample, and the last sample (the env's state, the action drawn for it, reward 0, terminal) and
the env's state after that step follow from public pieces of the oracle. The rebuilt batch is checked: a2c_loss_grads on it returns the update's own
losses, bit for bit."""
import contextlib
import ctypes as C
import functools
import json
import os

import numpy as np

import a2c_ref as R
import oraclelib as O
from ddpg_bar import JITTER_ULP, JitterNumpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_JSON = os.path.join(ROOT, "profiles", "a2c_bar.json")
OLD_LOSS_BAR, OLD_PARAM_BAR = 1e-9, 1e-6      # tests/test_gpu_a2c.py's bars (losses relative to max(1, |loss|), parameters absolute), still asserted
PARAM_BAR = 2.0 ** -21
LOSS_FACTOR = 32                  # the loss is a mean of n terms with independent last-bit errors: the tail three jitter draws do not sample
MUTANT_FACTOR = 10
JITTER_SEEDS = (1, 2, 3)
LOSSES, ARRAYS = ("actor_loss", "critic_loss"), ("grads", "params")
OBSERVABLES = LOSSES + ARRAYS
A2C_MAX_EPS = 4096                # episode records one crl_a2c_run_until_update call keeps (csrc/a2c.hip)


# ---------------------------------------------------------------------------------------------------- the case table
def _case(name, max_steps, min_replay_size, total_timesteps, n, edge, gamma=0.99, lr=1e-3, head=20.0, seed=3, pseed=5):
    return dict(name=name, max_steps=max_steps, min_replay_size=min_replay_size, total_timesteps=total_timesteps, n=n, edge=edge, gamma=gamma, lr=lr,
                head=head, seed=seed, pseed=pseed)


# With max_steps <= 7 the pole cannot fall: every episode has max_steps + 1 steps and n is the first multiple of that above min_replay_size.
# n: the batch size of every update of the case (a pair: its range). total_timesteps gives each case two or three updates (Adam's second step).
CASES = [
    _case("n12_cap", 5, 6, 36, 12, "n = cap: full ring, ptr wrapped to 0, fewer samples than a wave"),
    _case("n16_cap", 7, 8, 48, 16, "n = cap again, another episode length", seed=4),
    _case("n12_gamma0", 5, 6, 36, 12, "gamma = 0: the returns are the rewards", gamma=0.0, seed=5),
    _case("n12_gamma1", 5, 6, 36, 12, "gamma = 1: undiscounted returns", gamma=1.0, seed=6),
    _case("n64", 3, 63, 192, 64, "exactly one wave of samples", seed=7),
    _case("n65", 4, 64, 195, 65, "one sample more than a wave", seed=8),
    _case("n1024", 7, 1023, 2048, 1024, "exactly the loss kernel's block", seed=9),
    _case("n1032", 7, 1024, 2064, 1032, "eight samples in the second pass of the loss kernel's stride loop", seed=10),
    _case("ragged_1100", 500, 1100, 3700, (1101, 1601), "ragged n above 1024, episodes of different lengths", seed=11),
    _case("default", 500, 512, 1750, (513, 1013), "the reference's default shape: carries the old bars", seed=3),
    _case("default_head1", 500, 512, 1750, (513, 1013), "the untrained head of networks.jl (gain 0.01): a policy near 50/50", head=1.0, seed=12),
    _case("n8202_eps4101", 1, 8200, 16404, 8202, "4101 episodes in one call: five more than the record buffer holds", seed=13),
]
CASE = {c["name"]: c for c in CASES}
CHEAPEST = ("n12_cap", "n12_gamma0")      # what tests/test_a2c_bar_cpu.py recomputes


def case_cfg(case):
    return O.a2c_config(lr=case["lr"], total_timesteps=case["total_timesteps"], min_replay_size=case["min_replay_size"], gamma=case["gamma"],
                        max_steps=case["max_steps"], seed=case["seed"])


def case_params(case):
    """networks.jl's orthogonal start with the actor's head scaled: x 20 makes a policy that is not 50/50 (tests/test_gpu_a2c.py)"""
    pc = O.make_config()
    p = O.orthogonal_params(pc, case["pseed"])
    off = O.param_offsets(pc)
    p[off[4]:off[5]] *= np.float32(case["head"])
    return p


# ---------------------------------------------------------------------------------------------------- the oracle's updates
def _last_step(cfg, params, s_pre, gstep):
    """the step the loop takes from env state s_pre at global step gstep (a2c.jl:55-60) → (action, env state after it)"""
    L = O.a2c_lib()
    L.orc_u53.restype = C.c_double; L.orc_u53.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32]
    z = O.a2c_forward(cfg, params, 0, s_pre)
    e = np.exp(z - z.max())
    action = 1 if e[0] / (e[0] + e[1]) <= L.orc_u53(cfg.seed, 0, gstep, 0) else 0
    s = np.array(s_pre, np.float64); t = np.zeros(1, np.int32); done = np.zeros(1, np.int32)
    L.a2c_cartpole_step(s.ctypes.data_as(C.POINTER(C.c_double)), t.ctypes.data_as(C.POINTER(C.c_int32)), action, cfg.max_steps,
                        done.ctypes.data_as(C.POINTER(C.c_int32)))
    return action, s


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The case through the C oracle → (calls, updates). calls: what each run_until_update() call returned, to total_timesteps: (taken, stats,
    episodes, global_step after it); updates: per update its inputs (states (4, n), actions, rewards, terminals, final_state, reset_state, returns, params_before) and
    results (critic_loss, actor_loss, grads, params, n, global_step). Shared by every test of a case: nothing in it may be written to."""
    case = CASE[name]
    cfg, params = case_cfg(case), case_params(case)
    st = O.A2CState(cfg, params)
    calls = []
    while True:
        taken, ts, eps = st.run_until_update(max_eps=2 * A2C_MAX_EPS)
        if taken == 0:
            break
        calls.append((taken, ts, eps, st.env()[1]))
    st.close()
    st = O.A2CState(cfg, params)
    updates = []
    for taken, ts, eps, gstep in calls:
        if not ts["trained"]:
            continue
        before = st.get_params()
        st.run_until_update(max_env_steps=gstep - 1 - st.env()[1])
        s_pre, g, size = st.env()
        assert g == gstep - 1 and size == ts["n"] - 1
        states, actions, rewards, terms = st.buffer()
        action, final_state = _last_step(cfg, before, s_pre, gstep)
        states = np.asfortranarray(np.concatenate([states, s_pre[:, None]], axis=1))
        actions = np.append(actions, np.int32(action)); rewards = np.append(rewards, 0.0); terms = np.append(terms, np.uint8(1))
        _, ts2, _ = st.run_until_update(max_env_steps=1)
        assert ts2 == ts, "the replay reaches the same update"
        fv = O.a2c_forward(cfg, before, 1, final_state)[0]
        G = O.a2c_discounted_future_rewards(rewards, terms, fv, cfg.gamma)
        grads, cl, al, _ = O.a2c_loss_grads(cfg, before, states, actions, G)
        assert (cl, al) == (ts["critic_loss"], ts["actor_loss"]), "the rebuilt batch is the update's batch"
        updates.append(dict(states=states, actions=actions, rewards=rewards, terminals=terms, final_state=final_state, reset_state=st.env()[0],
                            returns=G, params_before=before, critic_loss=cl, actor_loss=al, grads=grads, params=st.get_params(), n=ts["n"],
                            global_step=gstep))
    st.close()
    for u in updates:
        for v in u.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return calls, updates


def n_matches(case, updates):
    want = case["n"]
    return len(updates) >= 2 and all(u["n"] == want if isinstance(want, int) else want[0] <= u["n"] <= want[1] for u in updates)


# ---------------------------------------------------------------------------------------------------- distances
def rel_per_array(got, ref):
    """max over the twelve arrays of max |got - ref| / max |ref| (an all-zero reference array has to be met exactly)"""
    worst = 0.0
    for a in range(12):
        g, r = np.asarray(got[R.OFF[a]:R.OFF[a + 1]], np.float64), np.asarray(ref[R.OFF[a]:R.OFF[a + 1]], np.float64)
        top = np.abs(r).max()
        d = np.abs(g - r).max()
        worst = max(worst, d / top if top > 0.0 else (0.0 if d == 0.0 else np.inf))
    return float(worst)


def distances(got, ref):
    """got, ref: per update a dict with critic_loss, actor_loss, grads, params → {observable: distance}; the losses relative to the case's largest"""
    assert len(got) == len(ref) > 0
    out = {}
    for k in LOSSES:
        g, r = np.array([u[k] for u in got]), np.array([u[k] for u in ref])
        out[k] = float(np.abs(g - r).max() / np.abs(r).max())
    for k in ARRAYS:
        out[k] = max(rel_per_array(g[k], r[k]) for g, r in zip(got, ref))
    return out


def load_bars():
    """→ (loss_bar, param_bar) as profiles/a2c_bar.json states them"""
    prof = json.load(open(BAR_JSON))
    return prof["loss_bar"], prof["param_bar"]


def bar_of(name, loss_bar, param_bar=PARAM_BAR):
    return loss_bar if name in LOSSES else param_bar


def record_device(name, out):
    """the device's distances of one case into profiles/a2c_bar.json, under "device" """
    try:
        prof = json.load(open(BAR_JSON))
        prof.setdefault("device", {})[name] = out
        with open(BAR_JSON, "w") as f:
            json.dump(prof, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:      # a read-only checkout: the figures were printed
        pass


# ---------------------------------------------------------------------------------------------------- patching a2c_ref for one run
@contextlib.contextmanager
def patched(**attrs):
    saved = {k: getattr(R, k) for k in attrs}
    try:
        for k, v in attrs.items():
            setattr(R, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(R, k, v)


def jitter(seed):
    """a2c_ref with every exp / log result moved by a seeded random integer in -2..+2 ulp"""
    return patched(np=JitterNumpy(seed, JITTER_ULP))


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
def _m1():                                                 # dvc = -adv / n
    orig = R.critic_loss

    def critic_loss(params, states, G):
        loss, adv, dv, h1, h2 = orig(params, states, G)
        return loss, adv, 0.5 * dv, h1, h2
    return dict(critic_loss=critic_loss)


def _m2():                                                 # the actor's mean and cotangent over n - 1
    orig = R.actor_loss

    def actor_loss(params, states, actions, adv):
        loss, dz, h1, h2 = orig(params, states, actions, adv)
        n = len(adv)
        return loss * n / (n - 1), dz * n / (n - 1), h1, h2
    return dict(actor_loss=actor_loss)


def _m3():                                                 # d2 = s, the (1 - h2 * h2) factor lost; d1 keeps its own
    orig = R.dtanh
    return dict(dtanh=lambda h, layer: np.ones_like(h) if layer == 2 else orig(h, layer))


def _m4():                                                 # next = reward[j] + gamma * next, terminal[j] not looked at inside the scan
    orig = R.discounted_future_rewards

    def discounted_future_rewards(rewards, terminals, final_value, gamma):
        t = np.zeros_like(terminals); t[-1] = terminals[-1]
        return orig(rewards, t, final_value, gamma)
    return dict(discounted_future_rewards=discounted_future_rewards)


def _m5():                                                 # dza of the action not taken left at 0: the - p term only where onehot is 1
    def softmax_cotangent(p, actions, k):
        onehot = (np.arange(R.A)[:, None] == actions[None, :]).astype(np.float64)
        return k[None, :] * (onehot - p) * onehot
    return dict(softmax_cotangent=softmax_cotangent)


def _m6():                                                 # the critic evaluated after the env's reset
    orig = R.final_value
    return dict(final_value=lambda params, final_state, reset_state=None: orig(params, reset_state))


# name → (what it mirrors, the cases it applies to, the patch). gamma = 0 switches the lines of M4 and M6 off (a terminal step's reward is 0 already).
MUTANTS = {
    "M1": ("the critic's cotangent is -adv/n, not -2 adv/n", lambda c: True, _m1),
    "M2": ("the actor's mean runs over n - 1", lambda c: True, _m2),
    "M3": ("1 - h2^2 is dropped in the backward", lambda c: True, _m3),
    "M4": ("terminal[j] is ignored inside the returns scan", lambda c: c["gamma"] != 0.0, _m4),
    "M5": ("the softmax cotangent lacks the -p term of the action not taken", lambda c: True, _m5),
    "M6": ("final_value is taken from the reset state", lambda c: c["gamma"] != 0.0, _m6),
}
# M6 breaks a line that the loop never lets matter: it trains only at an episode end, so the last transition of every batch is terminal and
# discounted_future_rewards multiplies final_value out (a2c.jl:15). It is measured on the case's batches with the last transition made non-terminal,
# which no device run can be given; on the real batches its distance is 0.
SYNTHETIC = ("M6",)


def applicable(case):
    return [m for m, (_, applies, _) in MUTANTS.items() if applies(case)]


# ---------------------------------------------------------------------------------------------------- one case, measured
def run_twin(case, patch=None, open_end=False):
    """the case's updates through a2c_ref (under `patch`), each on the oracle's batch → per update {"critic_loss", "actor_loss", "grads", "params"};
    open_end: the last transition of every batch made non-terminal with reward 1 (see SYNTHETIC)"""
    _, updates = oracle_run(case["name"])
    with (patch if patch is not None else contextlib.nullcontext()):
        twin = R.A2C(case_params(case), case["lr"], case["gamma"])
        out = []
        for u in updates:
            rewards, terms = u["rewards"], u["terminals"]
            if open_end:
                rewards, terms = rewards.copy(), terms.copy()
                rewards[-1], terms[-1] = 1.0, 0
            out.append(twin.update(u["states"], u["actions"], rewards, terms, u["final_state"], u["reset_state"]))
    return out


def measure(case):
    """→ {"floor": {observable: max over the jitter seeds}, "oracle_to_twin": {...}, "mutants": {name: {observable: distance}}}"""
    base = run_twin(case)
    floors = [distances(run_twin(case, jitter(s)), base) for s in JITTER_SEEDS]
    mutants = {}
    for m in applicable(case):
        synth = m in SYNTHETIC
        ref = run_twin(case, open_end=True) if synth else base
        mutants[m] = distances(run_twin(case, patched(**MUTANTS[m][2]()), open_end=synth), ref)
    return {"floor": {o: max(f[o] for f in floors) for o in OBSERVABLES}, "oracle_to_twin": distances(base, oracle_run(case["name"])[1]),
            "mutants": mutants}


def mutant_ratio(dist, loss_bar, param_bar=PARAM_BAR, without=()):
    """the largest distance / bar over the observables (without those named)"""
    return max(dist[o] / bar_of(o, loss_bar, param_bar) for o in OBSERVABLES if o not in without)
