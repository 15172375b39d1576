#!/usr/bin/env python3
"""SHA-256 of the gradient (F_GRADS) of two minibatches per configuration, one configuration per hidden-layer weight-gradient kernel of the layer-wise
path, shape and minibatch size: for comparing two builds of the library bit for bit (csrc/wide_wgrad.hpp; the oracle tests hold every build to a
tolerance only).

    python scripts/wgrad_digest.py                                                             # this build
    CRL_LIB_PATH=cleanrl.jl_amd/variants/<name>/libcleanrl_hip.so python scripts/wgrad_digest.py   # another one (scripts/build_variant.sh, make OUT=…)

Equal lines = equal bits. Run it twice on one build first: a line that does not reproduce there says nothing about two builds.
The buffers are injected as tests/test_gpu_wide.py::_flavour_case injects them; M = 4352 is three sample chunks (1472, 1472, 1408), M = 576 one."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ["CRL_FORCE_WIDE"] = "1"
import cleanrl_jl_amd as crl
import oraclelib as O
from test_gpu_wide import WGRAD_FLAVOURS, inject, make_wide, ocfg

# (obs_dim, n_act, hidden, num_envs, num_steps): M = num_envs * num_steps / 4
SHAPES_256 = [(D, A, 256, nt, k) for nt, k in ((136, 128), (24, 96)) for D, A in ((8, 4), (16, 8), (3, 2))]
SHAPES_SMALL = [(4, 2, 64, 136, 128), (6, 3, 128, 136, 128), (4, 2, 64, 24, 96), (6, 3, 128, 24, 96)]   # wide_wgrad_kernel<1> / <2>


def digests(opts, D, A, Hd, nt, k):
    rng = np.random.default_rng(nt + D)
    cfg = ocfg(nt, k, D, A, Hd)
    params = O.orthogonal_params(cfg, 5) + (0.05 * rng.standard_normal(O.lib().orc_param_count(cfg))).astype(np.float32)
    agent = make_wide(crl, nt, k, D, A, Hd, params=params)
    h = agent.handle
    for name, v in opts.items():
        h.set_option(name, v)
    st = O.State(cfg); st.params[:] = params
    inject(crl, agent, st, rng, D, A, 3.0)
    h.adv_stats()
    out = []
    for mb in (0, 3):
        h.update_minibatch(mb, 2.5e-4, apply_update=False)
        out.append(hashlib.sha256(np.ascontiguousarray(h.read(crl._lib.F_GRADS)).tobytes()).hexdigest())
    agent.close(); st.close()
    return out


if __name__ == "__main__":
    print("library:", os.environ.get("CRL_LIB_PATH", "this build"), flush=True)
    cases = [(o, s) for s in SHAPES_256 for o in WGRAD_FLAVOURS] + [({}, s) for s in SHAPES_SMALL]
    for opts, (D, A, Hd, nt, k) in cases:
        name = ",".join(f"{a}={b}" for a, b in opts.items()) or "default"
        for mb, d in zip((0, 3), digests(opts, D, A, Hd, nt, k)):
            print(f"{D}/{A}/{Hd} M={nt * k // 4:<5d} {name:32s} mb{mb} {d}", flush=True)
