"""Per-step cost of the running normaliser (crl_norm, csrc/norm.hip) on the device-pointer external-env path (recorded, not asserted), in the manner of
scripts/extenv_gauss_cost.py.

    python scripts/norm_cost.py [--out profiles/norm_step_cost.json] [--num_envs 16384]

At num_envs x 2x256, for the shapes 3 / 1 (Pendulum) and 17 / 6, in ONE run on one device with the arms ALTERNATING region by region:
  plain    crl_rollout_act_device_gaussian + crl_rollout_record_device_gaussian (enqueue only; one crl_sync per region)
  wrapped  the same pair with crl_norm_step_device between them on the handle's stream, the agent reading the normalised buffers
as wall microseconds per env step, median (min, max) over the regions; and the GPU time of one crl_norm_step_device alone (its two launches, update = 1)
and of its frozen form (one launch, update = 0), from HIP events around back-to-back calls on that stream. The comparison is wrapped against plain OF
THIS RUN. The shader clock under load is noted (crl_clock_probe) before and after."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cleanrl_jl_amd as crl  # noqa: E402
from extenv_cost import events  # noqa: E402

L = crl._lib
SHAPES = [(3, 1), (17, 6)]      # obs_dim, act_dim
H, STEPS, REGIONS = 256, 16, 15


def measure(D, ad, nt):
    cfg = crl.PPOConfig(num_envs=nt, num_steps=STEPS, num_minibatches=4, total_timesteps=nt * STEPS * 10)
    g = crl.Agent(cfg, action="gaussian", obs_dim=D, n_act=ad, hidden=H, env_kind=L.ENV_EXTERNAL)
    hg = g.handle
    norm, stream = L.Normalizer(L.NormOptions(nt, D)), hg.stream
    rng = np.random.default_rng(0)
    obs = np.asfortranarray(rng.standard_normal((D, nt)).astype(np.float32)); done = (rng.random(nt) < 0.005).astype(np.uint8)
    rew = -rng.random(nt).astype(np.float32)
    obs_d, done_d, rew_d = [L.DeviceBuffer(a.nbytes) for a in (obs, done, rew)]
    for b, a in zip((obs_d, done_d, rew_d), (obs, done, rew)):
        b.write(a)
    nobs_d, nrew_d, act_d = L.DeviceBuffer(obs.nbytes), L.DeviceBuffer(rew.nbytes), L.DeviceBuffer(4 * ad * nt)
    norm.reset_device(obs_d, nobs_d, stream=stream)

    def plain():
        for s in range(STEPS):
            hg.act_device_gaussian(s, obs_d, done_d, act_d); hg.record_device_gaussian(s, rew_d, obs_d, done_d)
        hg.sync()

    def wrapped():
        for s in range(STEPS):
            hg.act_device_gaussian(s, nobs_d, done_d, act_d)
            norm.step_device(obs_d, rew_d, done_d, nobs_d, nrew_d, stream=stream)
            hg.record_device_gaussian(s, nrew_d, nobs_d, done_d)
        hg.sync()

    arms = {"plain": plain, "wrapped": wrapped}
    wall = {k: [] for k in arms}
    for fn in arms.values():
        fn()   # warm-up
    for _ in range(REGIONS):     # alternating: a drift of the clock or of the host reaches every arm alike
        for k, fn in arms.items():
            t0 = time.perf_counter(); fn(); wall[k].append((time.perf_counter() - t0) / STEPS * 1e6)
    R, e0, e1 = events()
    kern = {"norm_step_update": [], "norm_step_frozen": []}
    for _ in range(REGIONS):
        for k, upd in (("norm_step_update", True), ("norm_step_frozen", False)):
            R.hipEventRecord(e0, C.c_void_p(stream))
            for s in range(STEPS):
                norm.step_device(obs_d, rew_d, done_d, nobs_d, nrew_d, update=upd, stream=stream)
            R.hipEventRecord(e1, C.c_void_p(stream)); R.hipEventSynchronize(e1)
            ms = C.c_float()
            R.hipEventElapsedTime(C.byref(ms), e0, e1)
            kern[k].append(ms.value / STEPS * 1e3)
    norm.close(); g.close()
    out = {k: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in (wall | kern).items()}
    out["wrapped_minus_plain_us"] = out["wrapped"]["median_us"] - out["plain"]["median_us"]
    out["wrapped_over_plain"] = out["wrapped"]["median_us"] / out["plain"]["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "norm_step_cost.json"))
    ap.add_argument("--num_envs", type=int, default=16384)
    args = ap.parse_args()
    res = dict(script="scripts/norm_cost.py", unit="microseconds per env step (wall: plain / wrapped) or per crl_norm_step_device (HIP events: norm_step_*)",
               num_envs=args.num_envs, hidden=H, steps_per_region=STEPS, regions=REGIONS, arms="alternating, one process, one device",
               clock_mhz_before=L.clock_probe(), shapes={})
    for D, ad in SHAPES:
        res["shapes"][f"{D}/{ad}"] = measure(D, ad, args.num_envs)
    res["clock_mhz_after"] = L.clock_probe()
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
