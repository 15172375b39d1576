"""Per-step cost of the device-pointer external-env path against the host-pointer one (recorded, not asserted).

    python scripts/extenv_cost.py [--out profiles/extenv_step_cost.txt]

For each size: the wall time per env step of crl_rollout_act_device + crl_rollout_record_device (enqueue only; one crl_sync per region) against
crl_policy_act + crl_rollout_store on host arrays (nine copies and two synchronisations per step), medians over repeated regions of `steps` steps; and the
GPU time of the act launch alone, from HIP events around a region of back-to-back launches on the handle's stream. The shader clock under load is noted
(crl_clock_probe) before and after."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cleanrl_jl_amd as crl  # noqa: E402

L = crl._lib
SIZES = [(4, 2, 64, 4096), (4, 2, 64, 65536), (8, 4, 256, 16384)]


def events():
    R = L.hip_runtime()
    R.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    R.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    R.hipEventSynchronize.argtypes = [C.c_void_p]
    R.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    a, b = C.c_void_p(), C.c_void_p()
    assert R.hipEventCreate(C.byref(a)) == 0 and R.hipEventCreate(C.byref(b)) == 0
    return R, a, b


def measure(D, A, H, nt, steps=16, regions=15):
    cfg = crl.PPOConfig(num_envs=nt, num_steps=steps, num_minibatches=4, total_timesteps=nt * steps * 10)
    agent = crl.Agent(cfg, obs_dim=D, n_act=A, hidden=H, env_kind=L.ENV_EXTERNAL)
    h = agent.handle
    rng = np.random.default_rng(0)
    obs = np.asfortranarray(rng.standard_normal((D, nt)).astype(np.float32)); done = np.zeros(nt, np.uint8); rew = np.ones(nt, np.float32)
    u = rng.random(nt)
    bufs = [L.DeviceBuffer(a.nbytes) for a in (obs, done, rew)]
    for b, a in zip(bufs, (obs, done, rew)):
        b.write(a)
    obs_d, done_d, rew_d = bufs
    act_d = L.DeviceBuffer(4 * nt)

    def device_region():
        for s in range(steps):
            h.act_device(s, obs_d, done_d, act_d)
            h.record_device(s, rew_d, obs_d, done_d)
        h.sync()

    def host_region():
        for s in range(steps):
            a, lp, v = h.policy_act(obs, u)
            h.rollout_store(s, obs, a, lp, rew, done, v)

    out = {}
    for name, fn in (("device", device_region), ("host", host_region)):
        fn()   # warm-up
        ts = []
        for _ in range(regions):
            t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) / steps * 1e6)
        out[name] = (statistics.median(ts), min(ts), max(ts))
    R, e0, e1 = events()
    stream = C.c_void_p(h.stream)
    ks = []
    for _ in range(regions):
        R.hipEventRecord(e0, stream)
        for s in range(steps):
            h.act_device(s, obs_d, done_d, act_d)
        R.hipEventRecord(e1, stream)
        R.hipEventSynchronize(e1)
        ms = C.c_float()
        R.hipEventElapsedTime(C.byref(ms), e0, e1)
        ks.append(ms.value / steps * 1e3)
    out["act_kernel"] = (statistics.median(ks), min(ks), max(ks))
    agent.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "extenv_step_cost.txt"))
    args = ap.parse_args()
    lines = ["# scripts/extenv_cost.py — microseconds per env step: median (min … max) over 15 regions of 16 steps",
             "# device = crl_rollout_act_device + crl_rollout_record_device (enqueue, one crl_sync per region); host = crl_policy_act + crl_rollout_store;",
             "# act_kernel = HIP events around 16 back-to-back act launches (GPU time per launch, launch gaps included)",
             "clock under load before: %.0f MHz (min %.0f, max %.0f)" % L.clock_probe()]
    for D, A, H, nt in SIZES:
        m = measure(D, A, H, nt)
        lines.append(f"{D}/{A}/2x{H} num_envs={nt}: " + "  ".join(f"{k} {v[0]:.1f} ({v[1]:.1f} … {v[2]:.1f})" for k, v in m.items())
                     + f"  host/device {m['host'][0] / m['device'][0]:.1f}x")
    lines.append("clock under load after: %.0f MHz (min %.0f, max %.0f)" % L.clock_probe())
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
