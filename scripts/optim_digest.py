#!/usr/bin/env python3
"""SHA-256 of the final parameter and optimiser-state bytes of five short runs, one per user of optim.hpp's ClipNorm + Adam: for comparing two
builds of the library bit for bit where no oracle test reaches (A2C's clipnorm_adam_kernel on arrays 6-11, then 0-5, has no gradient read-back).

    python scripts/optim_digest.py                                                          # this build
    CRL_LIB_PATH=cleanrl.jl_amd/variants/<name>/libcleanrl_hip.so python scripts/optim_digest.py   # another one (scripts/build_variant.sh, make OUT=…)

Equal lines = equal bits. Run it twice on one build first: a configuration whose digest does not reproduce there says nothing about two builds.
The A2C and DQN handles expose their parameters only; every one of them has gone through m, v and the β powers of all earlier steps."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cleanrl_jl_amd as crl
import oraclelib as O

F = crl._lib


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def a2c():
    """The run of tests/test_gpu_a2c.py::test_updates_match_oracle: 6000 steps, seed 3."""
    pc = O.make_config()
    p = O.orthogonal_params(pc, 5)
    off = O.param_offsets(pc)
    p[off[4]:off[5]] *= 20
    agent = crl.A2CAgent(crl.A2CConfig(total_timesteps=6000, lr=1e-3), params=p, seed=3)
    h, updates = agent.handle, 0
    while True:
        taken, ts, _ = h.run_until_update()
        updates += bool(ts["trained"])
        if taken == 0 or h.env()[1] >= 6000:
            break
    out = digest(h.read_params())
    agent.close()
    return out, f"{updates} updates"


def dqn():
    """The default run of tests/test_gpu_dqn.py::test_run_matches_oracle_bit_for_bit: 4000 steps, seed 21."""
    agent = crl.DQNAgent(crl.DQNConfig(total_timesteps=4000, lr=1e-3), params=O.dqn_params(1), seed=21)
    h = agent.handle
    h.run(4000)
    out = digest(h.read_params())
    n = h.status()["n_updates"]
    agent.close()
    return out, f"{n} updates"


def ppo(D, A, H, env_kind, options):
    """Three whole iterations of 4 envs x 32 steps, 4 minibatches (the sizes of tests/optimlib.py)."""
    cfg = crl.PPOConfig(num_envs=4, num_steps=32, num_minibatches=4, total_timesteps=4 * 32 * 10)
    agent = crl.Agent(cfg, seed=7, init_seed=3, obs_dim=D, n_act=A, hidden=H, env_kind=env_kind, options=options)
    h = agent.handle
    h.prof_enable(True)      # launch counters: launch_optim counts under "optim", the one-launch step (inside the reduce scope) does not
    h.iterate(3)
    out = digest(*(h.read(f) for f in (F.F_PARAMS, F.F_ADAM_M, F.F_ADAM_V, F.F_BETAP)))
    prof = h.prof_read()
    n_optim, n_reduce = prof["optim"][1], prof["reduce"][1]
    route = "reduce_optim_kernel" if n_optim == 0 else ("clipnorm_partial + adam_slice" if h.P > 32768 else "clipnorm_adam_kernel")
    note = f"{route}: {n_optim} optimiser launches, {n_reduce} reduce launches, fuse_optim {h.get_option('fuse_optim')}, P = {h.P}"
    agent.close()
    return out, note


CONFIGS = {
    "a2c": a2c,
    "dqn": dqn,
    "ppo-4/2/64-fused": lambda: ppo(4, 2, 64, F.ENV_CARTPOLE, {"fuse_optim": 1}),
    "ppo-4/2/64-two-launch": lambda: ppo(4, 2, 64, F.ENV_CARTPOLE, {"fuse_optim": 0}),
    "ppo-17/5/256-slices": lambda: ppo(17, 5, 256, F.ENV_SYNTHETIC, {"wide_gemm": 2}),
}

if __name__ == "__main__":
    print("library:", os.environ.get("CRL_LIB_PATH", "this build"), flush=True)
    for name in sys.argv[1:] or CONFIGS:
        d, note = CONFIGS[name]()
        print(f"{name:24s} {d}  ({note})", flush=True)
