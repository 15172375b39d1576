"""Does tests/gae_cases.py:route name the kernel that csrc/gae.hip:launch_gae really launches? The library has no hook that says which kernel ran, so the
restated rule is held against a rocprofv3 kernel trace, once, by hand:
   rocprofv3 --kernel-trace --output-format csv -d /tmp/kt -- python3 scripts/gae_route_trace.py run
   python3 scripts/gae_route_trace.py check /tmp/kt
`run` launches every row of the table with both load flavours, in order (plus the handle-driven launches of the option test's grid); `check` reads the GAE
kernels of the trace in dispatch order, compares each with the rule's prediction and writes the tally to profiles/gae_edges.json ("route_trace")."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gae_cases as G  # noqa: E402

NAMES = {"one": "gae_kernel", "pair": "gae_seg2_kernel", "stream": "gae_stream_kernel"}
HANDLE = (8, 40)
HANDLE_GRID = [(seg, tile, ntl) for seg in (8, 16) for tile in (1, 2, 8, 64, 128, 256) for ntl in (0, 1)]


def expected():
    out = [(G.route(row.nt, row.k, row.seg, row.tile), ntl) for row in G.GEOMETRY for ntl in (0, 1)]
    return out + [(G.route(*HANDLE, seg, tile), ntl) for seg, tile, ntl in HANDLE_GRID]


def run():
    import numpy as np
    import cleanrl_jl_amd as crl
    for row in G.GEOMETRY:
        d = G.inputs("standard", row.nt, row.k)
        for ntl in (0, 1):
            crl._lib.gae_host(*G.args(d, 1), seg=row.seg, tile=row.tile, nt_loads=ntl)
    nt, k = HANDLE
    agent = crl.Agent(crl.PPOConfig(num_envs=nt, num_steps=k, total_timesteps=nt * k * 10, num_minibatches=1))
    h = agent.handle
    d = G.inputs("standard", nt, k)
    F = crl._lib
    h.write(F.F_VALUE, np.asfortranarray(d["value"])); h.write(F.F_REWARD, np.asfortranarray(d["reward"]))
    h.write(F.F_TERMINAL, np.asfortranarray(d["term"])); h.write(F.F_NEXT_DONE, d["nd"])
    for seg, tile, ntl in HANDLE_GRID:
        h.set_option("gae_seg", seg); h.set_option("gae_tile", tile); h.set_option("gae_nt_loads", ntl)
        h.compute_gae()
    h.sync()
    agent.close()


def check(path):
    f = glob.glob(path + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    seen = []
    for r in rows:
        m = re.search(r"(gae_kernel|gae_seg2_kernel|gae_stream_kernel)<(\d+), ?(\d+), ?(?:\(bool\))?(true|false|0|1)>", r["Kernel_Name"])
        if m:
            seen.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4) in ("true", "1"))))
    want = [(NAMES[r[0]], r[1], r[2], ntl) for r, ntl in expected()]
    bad = [(i, w, s) for i, (w, s) in enumerate(zip(want, seen)) if w != s]
    rec = dict(launches_expected=len(want), launches_traced=len(seen), mismatches=len(bad) + abs(len(want) - len(seen)), distinct_kernels_traced=len(set(seen)))
    print(rec)
    for b in bad[:20]:
        print("launch %d: the rule says %s, the trace %s" % b)
    G.write_profile("route_trace", rec)
    return 1 if rec["mismatches"] else 0


if __name__ == "__main__":
    sys.exit(run() if sys.argv[1] == "run" else check(sys.argv[2]))
