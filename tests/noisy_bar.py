"""The case table, the distances, the jittered twin and the one-line mutants of the noisy-layer tests (tests/test_noisy_cpu.py, tests/test_gpu_noisy.py),
by the method of tests/duel_bar.py: the bars of the cases that run a transcendental (pow under PER, exp / log on the categorical head) are measured on
the CPU from the restatement's OWN ±2 ulp jitter floor (scripts/noisy_bar.py → profiles/noisy_bar.json), never from the device. The uniform scalar
cases, plain and dueling with any target option, run no transcendental once xi is given (the device's tape is injected), so they are bit-equal in
everything and need no bar."""
import contextlib
import json
import os

import numpy as np

import ddpg_bar as B
import dqn_per_bar as PB
import duel_bar as DB
import duel_ref as D
import noisy_ref as N
import oraclelib as O

BAR_JSON = os.path.join(B.ROOT, "profiles", "noisy_bar.json")
PARAM_BAR, LOSS_FACTOR, MUTANT_FACTOR, JITTER_SEEDS, JITTER_ULP = B.PARAM_BAR, B.LOSS_FACTOR, 1000, B.JITTER_SEEDS, DB.JITTER_ULP
OBSERVABLES = ("loss", "q", "target", "image_q", "image_t", "proj")
SIGMA0 = 0.5


# ---------------------------------------------------------------------------------------------------- the case table
def _case(name, edge, seed=21, per=False, tgt=None, c51=None, dueling=False, **kw):
    return dict(name=name, edge=edge, seed=seed, per=per, tgt=tgt, c51=c51, dueling=dueling, kw=kw)


# duel_bar._BASE: k = 31 in a ring of 1000, an update every 10 steps from step 110 on (20 updates in 300 steps), a target copy every 50 steps, the ε
# schedule reaching 0.05 at step 300. EPS0 is the NoisyNet setting: the agent acts on the noisy image from its first step.
_BASE = DB._BASE
EPS0 = dict(epsilon_start=0.0, epsilon_end=0.0)
_N3D = dict(n_step=3, double_q=1)
CASES = [
    _case("k1_cap1", "k = 1 in a ring of 1, a copy with every update, the ε schedule on", total_timesteps=120, batch_size=1, buffer_size=1, min_buff_size=1,
          train_freq=1, target_net_freq=1),
    _case("k65_eps0", "k = 65: one parameter-stride past a wave; ε = 0", batch_size=65, **EPS0),
    _case("k120_duel", "the reference's default batch on the dueling net (five layers in the table)", dueling=True, total_timesteps=400, batch_size=120,
          min_buff_size=200, **EPS0),
    _case("k1024", "the largest batch, once", total_timesteps=1100, batch_size=1024, buffer_size=1024, min_buff_size=1024, train_freq=25),
    _case("wrap_cap31_duel", "a ring that wraps; target_net_freq 50 coprime with train_freq 3: most updates redraw the target image without a copy",
          dueling=True, total_timesteps=400, buffer_size=31, min_buff_size=40, train_freq=3, tgt=dict(n_step=3, double_q=0), **EPS0),
    _case("tf_equal_n3_double", "target_net_freq = train_freq: a copy with every update; 3-step returns and double Q (the online image serves two passes)",
          target_net_freq=10, tgt=_N3D, **EPS0),
    _case("logfreq7", "log_frequency = 7: records at 140, 210, 280", log_frequency=7),
    _case("per", "prioritized replay on the plain net", per=True, **EPS0),
    _case("per_duel", "prioritized replay on the dueling net, the ε schedule on", per=True, dueling=True),
    _case("c51_n2", "categorical, two atoms", c51=dict(n_atoms=2), **EPS0),
    _case("c51_n33_per", "categorical with an odd head and prioritized replay", c51=dict(n_atoms=33), per=True),
    _case("rainbow_n64", "dueling + C51 at 64 atoms (the 892-entry table) + PER + 3-step + double Q, ε = 0", c51=dict(n_atoms=64), per=True, dueling=True,
          tgt=_N3D, **EPS0),
]
CASE = {c["name"]: c for c in CASES}
EXACT = tuple(c["name"] for c in CASES if c["c51"] is None and not c["per"])       # no transcendental behind the tape: bit-equal on the device
CHEAPEST = ("k1_cap1", "c51_n2")


def case_cfg(case):
    return O.dqn_config(**{"lr": 1e-3, "log_frequency": 1, "seed": case["seed"], **_BASE, **case["kw"]})


def case_per(case):
    if not case["per"]:
        return None
    return {"alpha": 0.6, "beta_start": 0.4, "beta_end": 1.0, "beta_duration": float(case_cfg(case).total_timesteps), "eps": 1e-6}


def case_tgt(case):
    return None if case["tgt"] is None else {"n_step": 1, "double_q": 0, **case["tgt"]}


def case_c51(case):
    return None if case["c51"] is None else {"n_atoms": 51, "v_min": 0.0, "v_max": 100.0, **case["c51"]}


def case_layers(case):
    return N.layers(case["dueling"], None if case["c51"] is None else case["c51"]["n_atoms"])


def params_for(lay, sigma0=SIGMA0):
    """Fortunato's rule with a numpy stream, sigma spread by ±20 % so that no two entries of an array need agree: mu (P) then sigma (P)"""
    rng = np.random.default_rng(1)
    mu, sg = [], []
    for i, o in lay:
        n, lim = o * (i + 1), 1.0 / np.sqrt(float(i))
        mu.append(rng.uniform(-lim, lim, n)); sg.append(sigma0 * lim * rng.uniform(0.8, 1.2, n))
    return np.concatenate(mu + sg).astype(np.float32)


def case_params(case):
    return params_for(case_layers(case))


def make_ref(case, tape=None):
    return N.make(case_cfg(case), case_per(case), case_tgt(case), case_c51(case), case["dueling"], case_params(case), tape)


# ---------------------------------------------------------------------------------------------------- distances
def distances(losses, params, images, proj, ref_losses, ref_params, ref_images, ref_proj, lay):
    """losses [(g, loss)]; params (q, target) 2P each; images (q, target) P each; proj (N, k) or None → {observable: distance}"""
    assert [l[0] for l in losses] == [l[0] for l in ref_losses] and len(losses) > 0
    sizes = N.array_sizes(lay)
    out = {"loss": PB.loss_distance([l[1] for l in losses], [l[1] for l in ref_losses])}
    for name, dev, rf in zip(("q", "target"), params, ref_params):
        out[name] = B.rel_per_array(dev, rf, sizes * 2)
    for name, dev, rf in zip(("image_q", "image_t"), images, ref_images):
        out[name] = B.rel_per_array(dev, rf, sizes)
    out["proj"] = 0.0 if ref_proj is None else float(np.abs(np.asarray(proj) - np.asarray(ref_proj)).max())
    return out


def load_bars(path=BAR_JSON):
    prof = json.load(open(path))
    return {"loss": prof["loss_bar"], "proj": prof["proj_bar"], **{o: prof["param_bar"] for o in ("q", "target", "image_q", "image_t")}}


jitter = DB.jitter                                         # exp, log and pow of the wrapped restatements moved by ±2 ulp


@contextlib.contextmanager
def nudged(seed, amp=B.JITTER_ULP["cos"]):
    """log and cos of the xi draw moved by a seeded random integer in −amp..+amp ulp"""
    rng = np.random.default_rng(seed)

    def moved(f):
        def g(x):
            v = np.asarray(f(x), np.float64)
            return v + rng.integers(-amp, amp + 1, v.shape).astype(np.float64) * np.spacing(np.abs(v))
        return g
    with D.replaced(N, _log=moved(np.log), _cos=moved(np.cos)):
        yield


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
def _independent(xo, xi):
    """a full-rank eps: the factorised product with a fixed pseudo-random sign per entry"""
    return xo[:, None] * xi[None, :] * np.where(np.random.default_rng(7).integers(0, 2, (xo.size, xi.size)) == 1, np.float32(1), np.float32(-1))


MUTANTS = {
    "M1": ("independent instead of factorised eps", "run", lambda: dict(weight_eps=_independent)),
    "M2": ("f(x) = x", "noise", lambda: dict(squash=lambda z: z)),
    "M3": ("one stream word for both nets", "noise", lambda: dict(stream_of=lambda net: N.S_NOISY[0])),
    "M4": ("the target image not redrawn without a copy", "run", lambda: dict(target_gen=lambda n, copied, prev: n if copied else prev)),
    "M5": ("the online image not redrawn after an update", "run", lambda: dict(online_gen=lambda n: 0)),
    "M6": ("g_sigma without eps", "run", lambda: dict(sigma_grad=lambda g, eps: np.asarray(g, np.float32))),
    "M7": ("bias noise from xi_in", "run", lambda: dict(bias_eps=lambda xo, xi: np.resize(xi, xo.size))),
    "M8": ("evaluation on the noisy image", "eval", lambda: dict(greedy_image=lambda agent: agent.q)),
}


def mutant(name):
    return D.replaced(N, **MUTANTS[name][2]())


def run_ref(case, patch=None, tape=None):
    """the case through noisy_ref (under `patch`) → (losses, (pq, pt), (q, t), proj or None, episodes)"""
    cfg = case_cfg(case)
    with (patch if patch is not None else contextlib.nullcontext()):
        ref = make_ref(case, tape)
        _, eps, losses = ref.run(cfg.total_timesteps)
    return losses, (ref.pq, ref.pt), (ref.q, ref.t), (None if case["c51"] is None else ref.proj), eps


def variant_distance(case, patch, base, tape=None):
    got = run_ref(case, patch, tape)
    return distances(got[0], got[1], got[2], got[3], base[0], base[1], base[2], base[3], case_layers(case)), got[4] == base[4]


def measure(case):
    """→ {"floor": {observable: max over the jitter seeds}, "same_episodes": did every jittered twin replay the base run's episodes}"""
    base = run_ref(case)
    twins = [variant_distance(case, jitter(s), base) for s in JITTER_SEEDS]
    return {"floor": {o: max(t[0][o] for t in twins) for o in OBSERVABLES}, "same_episodes": all(t[1] for t in twins)}
