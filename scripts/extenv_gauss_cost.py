"""Per-step cost of the device-pointer external-env path on a Gaussian handle (recorded, not asserted), in the manner of scripts/extenv_cost.py.

    python scripts/extenv_gauss_cost.py [--out profiles/extenv_gauss_step_cost.json] [--num_envs 16384]

At num_envs x 2x256, for the shapes 3 / 1 (Pendulum) and 17 / 6, in ONE run on one device with the arms ALTERNATING region by region:
  device    crl_rollout_act_device_gaussian + crl_rollout_record_device_gaussian (enqueue only; one crl_sync per region)
  host      crl_policy_act_gaussian + crl_rollout_store_gaussian on host arrays (staging copies and a synchronisation per call)
  discrete  crl_rollout_act_device + crl_rollout_record_device on a softmax handle with n_act = 2·act_dim head rows (the same forward, the softmax tail)
as wall microseconds per env step, median (min, max) over the regions; and the GPU time of the two act launches alone, from HIP events around
back-to-back launches on the handle's stream. The shader clock under load is noted (crl_clock_probe) before and after."""
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
    d = crl.Agent(cfg, obs_dim=D, n_act=2 * ad, hidden=H, env_kind=L.ENV_EXTERNAL)
    hg, hd = g.handle, d.handle
    rng = np.random.default_rng(0)
    obs = np.asfortranarray(rng.standard_normal((D, nt)).astype(np.float32)); done = np.zeros(nt, np.uint8); rew = np.ones(nt, np.float32)
    xi = rng.standard_normal((ad, nt)).astype(np.float32)
    obs_d, done_d, rew_d = [L.DeviceBuffer(a.nbytes) for a in (obs, done, rew)]
    for b, a in zip((obs_d, done_d, rew_d), (obs, done, rew)):
        b.write(a)
    actf_d, acti_d = L.DeviceBuffer(4 * ad * nt), L.DeviceBuffer(4 * nt)

    def device():
        for s in range(STEPS):
            hg.act_device_gaussian(s, obs_d, done_d, actf_d); hg.record_device_gaussian(s, rew_d, obs_d, done_d)
        hg.sync()

    def host():
        for s in range(STEPS):
            a, lp, v = hg.policy_act_gaussian(obs, xi)
            hg.rollout_store_gaussian(s, obs, a, lp, rew, done, v)

    def discrete():
        for s in range(STEPS):
            hd.act_device(s, obs_d, done_d, acti_d); hd.record_device(s, rew_d, obs_d, done_d)
        hd.sync()

    arms = {"device": device, "host": host, "discrete": discrete}
    wall = {k: [] for k in arms}
    for fn in arms.values():
        fn()   # warm-up
    for _ in range(REGIONS):     # alternating: a drift of the clock or of the host reaches every arm alike
        for k, fn in arms.items():
            t0 = time.perf_counter(); fn(); wall[k].append((time.perf_counter() - t0) / STEPS * 1e6)
    R, e0, e1 = events()
    kern = {"act_gaussian": [], "act_discrete": []}
    launches = {"act_gaussian": (hg, lambda s: hg.act_device_gaussian(s, obs_d, done_d, actf_d)), "act_discrete": (hd, lambda s: hd.act_device(s, obs_d, done_d, acti_d))}
    for _ in range(REGIONS):
        for k, (h, launch) in launches.items():
            stream = C.c_void_p(h.stream)
            R.hipEventRecord(e0, stream)
            for s in range(STEPS):
                launch(s)
            R.hipEventRecord(e1, stream); R.hipEventSynchronize(e1)
            ms = C.c_float()
            R.hipEventElapsedTime(C.byref(ms), e0, e1)
            kern[k].append(ms.value / STEPS * 1e3)
    g.close(); d.close()
    out = {k: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in (wall | kern).items()}
    out["host_over_device"] = out["host"]["median_us"] / out["device"]["median_us"]
    out["device_over_discrete"] = out["device"]["median_us"] / out["discrete"]["median_us"]
    out["act_gaussian_over_act_discrete"] = out["act_gaussian"]["median_us"] / out["act_discrete"]["median_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "extenv_gauss_step_cost.json"))
    ap.add_argument("--num_envs", type=int, default=16384)
    args = ap.parse_args()
    res = dict(script="scripts/extenv_gauss_cost.py", unit="microseconds per env step (wall: device / host / discrete) or per launch (HIP events: act_*)",
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
