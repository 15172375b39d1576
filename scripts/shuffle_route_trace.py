"""Does tests/shuffle_ref.py:adv_route name the kernel that really leaves the advantage sums? The library has no hook that says which kernel ran, so the
restated rule is held against a rocprofv3 kernel trace (no counters), once, by hand:
   rocprofv3 --kernel-trace --output-format csv -d /tmp/kt -- python3 scripts/shuffle_route_trace.py run
   python3 scripts/shuffle_route_trace.py check /tmp/kt
`run` walks the advantage-sum cases of tests/shuffle_cases.py: each case's set-up, then ONE marker launch (a forced streaming GAE kernel, which no
handle of the table launches), the call that produces the sums, and a second marker; then one blocked shuffle at each of the three big sizes.
`check` cuts the trace at the markers, keeps the shuffle and advantage kernels of every case and writes them, with the route the rule names, to
profiles/shuffle_route_trace.json; tests/test_shuffle_cpu.py compares the two."""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import shuffle_cases as SC  # noqa: E402
import shuffle_ref as R  # noqa: E402

MARK = "gae_stream_kernel"
KEEP = r"(bfy_l1_kernel<\d+>|bfy_scan_kernel|bfy_leaf_kernel|fy_serial_kernel|bijection_kernel|iota_kernel|adv_bucket_sums_kernel<\d+>|adv_gather_sums_kernel|adv_sums_inv_kernel<\d+>|adv_sums_kernel|adv_sums_fold_kernel)"


def run():
    import numpy as np
    import cleanrl_jl_amd as crl
    F = crl._lib
    z = np.zeros((4, 2), np.float32, order="F")

    def mark():
        F.gae_host(z, z, np.zeros((4, 2), np.uint8, order="F"), np.zeros(4, np.float32), np.zeros(4, np.uint8), 0.99, 0.95, 1, seg=4, tile=4, nt_loads=0)

    for c in SC.ADV_CASES:
        n = c.nt * c.k
        os.environ["CRL_FORCE_WIDE"] = "1" if c.path == "wide" else "0"
        cfg = crl.PPOConfig(num_envs=c.nt, num_steps=c.k, total_timesteps=n * 1000, num_minibatches=c.nmb, update_epochs=c.epochs, anneal_lr=False)
        agent = crl.Agent(cfg, shuffle_mode=c.mode, seed=SC.SEED, options={"adv_seq": c.seq})
        h = agent.handle
        adv = SC.adv_integers(n)
        if c.how == "iterate" or (c.how == "shuffle" and c.slot):
            h.env_reset()
        if c.how == "shuffle" and c.slot:
            h.iterate(1, want_stats=False)
        if c.how == "write_perm":
            h.shuffle(SC.HOST_EPOCH); h.adv_stats()
            h.write(F.F_PERM, np.random.default_rng(5).permutation(n).astype(np.int32))
        if c.how != "iterate":
            h.write(F.F_REWARD if c.how == "update" else F.F_ADVANTAGE, adv)
        h.sync()
        mark()
        if c.how == "iterate":
            h.iterate(1, want_stats=False)
        elif c.how == "update":
            h.update(want_stats=False)
        else:
            if c.how == "shuffle":
                h.shuffle(SC.HOST_EPOCH)
            h.adv_stats()
        h.sync()
        mark()
        agent.close()
    os.environ["CRL_FORCE_WIDE"] = "0"
    for n, (nt, k) in SC.SIZES_BIG.items():
        agent = crl.Agent(crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=n * 10, num_minibatches=1, update_epochs=1), shuffle_mode=R.BLOCKED, seed=SC.SEED)
        agent.handle.shuffle(0); agent.handle.sync()
        agent.close()
    mark()


def check(path):
    f = glob.glob(path + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    spans, cur = [], []
    for r in rows:
        if MARK in r["Kernel_Name"]:
            spans.append(cur); cur = []
            continue
        m = re.search(KEEP, r["Kernel_Name"].replace(", ", ","))
        if m:
            cur.append(m.group(1))
    # spans[0]: before the first marker; spans[2i + 1]: case i's call; spans[2i + 2]: between cases; the last one: the big shuffles
    want = 2 * len(SC.ADV_CASES) + 1
    if len(spans) != want:
        print("expected %d markers, the trace holds %d" % (want, len(spans)))
        return 1
    out = {"cases": {}, "big": {"sizes": sorted(SC.SIZES_BIG), "kernels": sorted(set(spans[-1]) - {"iota_kernel"})}}
    bad = 0
    for i, c in enumerate(SC.ADV_CASES):
        route = R.adv_route(c.path, c.mode, c.nt * c.k, c.nmb, c.seq, c.how, c.slot)
        kernels = sorted(set(spans[2 * i + 1]))
        adv = [k for k in kernels if re.match(r"adv_(bucket_sums|gather_sums|sums|sums_inv)_kernel", k)]
        ok = (adv == [] and "bfy_leaf_kernel" in kernels) if route == R.LEAF else adv == [R.ROUTE_KERNEL[route]]
        if not ok:
            bad += 1
            print("%s: the rule says %s, the trace %s" % (SC.case_id(c), route, kernels))
        out["cases"][SC.case_id(c)] = {"route": route, "kernels": kernels}
    print("cases %d, mismatches %d, distinct kernels %d" % (len(SC.ADV_CASES), bad, len({k for v in out["cases"].values() for k in v["kernels"]} | set(out["big"]["kernels"]))))
    with open(SC.TRACE, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(run() if sys.argv[1] == "run" else check(sys.argv[2]))
