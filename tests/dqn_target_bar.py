"""What the n-step / double-Q parity tests share (tests/test_dqn_target_cpu.py, tests/test_gpu_dqn_target.py): the ONE case table, built on
tests/dqn_per_bar.py's _BASE shapes (k = 31 in a ring of 1000, an update every 10 steps from step 110 on, lr 1e-3, every update logged), the run of a
case through tests/dqn_target_ref.py, and one-line wrong versions of that restatement (the MUTANTS).

There is no new bar. A uniform case holds no transcendental, so device and restatement have to agree bit for bit; a PER case sits under
dqn_per_bar.load_bars(), because its one rounding freedom is still PER's pow. A mutant has to move a logged loss or a parameter array by more than those
bars on at least one case, which also means it breaks bit-equality there."""
import contextlib

import numpy as np

import dqn_per_bar as PB
import dqn_target_ref as T
import oraclelib as O

CHUNKS = PB.CHUNKS
PER_DEFAULT = dict(alpha=0.6, beta_start=0.4, beta_end=1.0, eps=1e-6)


def _case(name, edge, n_step, double_q, per=None, seed=21, **kw):
    return dict(name=name, edge=edge, seed=seed, per=per, tgt=dict(n_step=n_step, double_q=double_q), kw=kw)


_WRAP = dict(total_timesteps=400, buffer_size=31, min_buff_size=40, train_freq=3)
CASES = [
    _case("n1_plain", "{1, 0}, uniform: the crl_dqn_create run through the new kernels", 1, False),
    _case("double_copy_each", "target == q_net at every update, so a* picks the max: the plain run", 1, True, target_net_freq=10),
    _case("double", "double_q with a target that lags 50 steps", 1, True),
    _case("n3", "the Rainbow default horizon", 3, False),
    _case("n3_double", "both", 3, True),
    _case("n5_cap31", "ring 31, an update every 3 steps: walks cross the wrap", 5, False, **_WRAP),
    _case("n16", "a horizon longer than early random episodes: terminals inside the window", 16, False),
    _case("n16_cap8_k4", "a ring shorter than the horizon", 16, False, total_timesteps=200, batch_size=4, buffer_size=8, min_buff_size=10, train_freq=3),
    _case("n3_freq1", "an update after every step: the newest slot is drawn, head cut", 3, False, total_timesteps=200, train_freq=1),
    _case("n3_cap1_k1", "one slot", 3, False, total_timesteps=120, batch_size=1, buffer_size=1, min_buff_size=1, train_freq=1, target_net_freq=1),
    _case("n3_gamma0", "disc becomes 0.0 after one step", 3, False, gamma=0.0),
    _case("n3_double_k1024_cap1024", "the largest batch", 3, True, total_timesteps=1200, batch_size=1024, buffer_size=1024, min_buff_size=1024,
          train_freq=25),
    _case("per_n3_double_k31_cap31", "PER, k = n, the ring wraps", 3, True, per={}, **_WRAP),
    _case("per_n3_double_k120", "PER at the reference's default batch", 3, True, per={}, total_timesteps=400, batch_size=120, min_buff_size=200),
    _case("per_n3_alpha1", "PER with alpha = 1: the leaf is |δ| + eps of the n-step target", 3, False, per=dict(alpha=1.0)),
]
CASE = {c["name"]: c for c in CASES}
TARGET_ARRAYS = ("last", "m", "nret", "ndisc", "astar", "td")


def case_cfg(case):
    return O.dqn_config(**{"lr": 1e-3, "log_frequency": 1, "seed": case["seed"], **PB._BASE, **case["kw"]})


def case_per(case):
    if case["per"] is None:
        return None
    return {**PER_DEFAULT, "beta_duration": float(case_cfg(case).total_timesteps), **case["per"]}


case_params = PB.case_params


def lagging_double(case):
    """a double_q case whose target_net is not a copy of q_net at every update"""
    cfg = case_cfg(case)
    return case["tgt"]["double_q"] and cfg.target_net_freq > cfg.train_freq


# ---------------------------------------------------------------------------------------------------- one case through the restatement
@contextlib.contextmanager
def patched(**attrs):
    saved = []
    try:
        for name, new in attrs.items():
            saved.append((name, getattr(T, name)))
            setattr(T, name, new)
        yield
    finally:
        for name, old in reversed(saved):
            setattr(T, name, old)


def run_ref(case, patch=None):
    """→ dict(losses, params (q, target), counts, ref)"""
    cfg = case_cfg(case)
    T.reset_counts()
    with (patch if patch is not None else contextlib.nullcontext()):
        ref = T.DQNTarget(cfg, case_per(case), case["tgt"], case_params(case))
        _, eps, losses = ref.run(cfg.total_timesteps)
    return dict(losses=losses, params=(ref.q, ref.t), counts=dict(T.COUNTS), ref=ref, episodes=eps)


# ---------------------------------------------------------------------------------------------------- mutants: one wrong line each
# name → (what it mirrors, the patch, the case that has to show it)
MUTANTS = {
    "T1": ("bootstrap from next_state[s]", lambda: dict(boot_slot=lambda s, last: s), "n3"),
    "T2": ("gamma in place of disc", lambda: dict(td_disc=lambda disc, gamma: np.full_like(disc, gamma)), "n3"),
    "T3": ("terminal ignored inside the window", lambda: dict(window_terminal=lambda t: False), "n16"),
    "T4": ("head stop ignored", lambda: dict(head_stop=lambda nx, ptr: False), "n3_freq1"),
    "T5": ("a* from target_net under double_q", lambda: dict(astar_source=lambda double_q, sq, tq: tq), "double"),
    "T6": ("next_q from q_net", lambda: dict(next_q_source=lambda sq, tq: sq), "double"),
}


def mutant_ratio(name, base=None):
    """the largest distance / bar over (loss, q, target) of the mutant from the unpatched run of its case, under dqn_per_bar's bars"""
    what, patch, case_name = MUTANTS[name]
    case = CASE[case_name]
    base = base or run_ref(case)
    mut = run_ref(case, patched(**patch()))
    loss_bar, param_bar = PB.load_bars()
    dist = PB.distances(mut["losses"], mut["params"], base["losses"], base["params"])
    return PB.mutant_ratio(dist, loss_bar, param_bar), dist
