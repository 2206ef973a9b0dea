#!/usr/bin/env python3
"""Times a 200-point logarithmic AC sweep over 4 decades of rc_mesh(100, 100, 1, True), batch 1 and batch 8,
  (a) as a loop of pe_hip_analyze_ac + pe_hip_get_solution_ac with the PARENT commit's library, and
  (b) as one pe_hip_analyze_ac_sweep + pe_hip_get_ac_sweep with this tree's library,
alternating (a) and (b) `--repeats` times (>= 3) in one invocation.  Profiler off; every measurement is a fresh child process (one library
per process) that loads the circuit, solves the operating point, runs the work once to warm up (engines built, pivot orders of the first
pass made, memory allocated) and then times it with the host clock -- both calls return after a stream synchronise.  The yardstick is (a)
on the parent, never this tree's own loop.  The bar: (b) beats (a) by more than the spread between the repeats of (a).

    python scripts/ac_sweep_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/ac_sweep_timing.json]

Writes one JSON document: per batch the times of every repeat, their medians, the ratio, the spread of (a), the sweep's statistics
(n_passes, points_per_pass, n_analyses, ...) and the two build ids."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import ctypes as C, json, sys, time
root, mode, batch, points = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
sys.path.insert(0, root)
import numpy as np
import pe_load
pe = pe_load.load()
F = pe.ffi
lib = F.lib()
deck = pe.deck.rc_mesh(100, 100, 1, True)
w = np.logspace(7.0, 11.0, points)
e = F.Engine(device=0)
e.set_options(g_min=0.0)
e.load_deck(deck, batch)
e.reset()
e.analyze_dc(F.MODE_OP)
n = e.rows
stats = {}
if mode == "loop":
    lib.pe_hip_analyze_ac.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    lib.pe_hip_get_solution_ac.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    re = np.empty((points, batch, n)); im = np.empty_like(re)
    def work():
        for i, x in enumerate(w):
            rc = lib.pe_hip_analyze_ac(e._h, float(x), None)
            assert rc == 0, (i, x, rc)
            assert lib.pe_hip_get_solution_ac(e._h, 0, batch, F._dp(re[i]), F._dp(im[i])) == 0
        return re, im
else:
    re = np.empty((points, batch, n)); im = np.empty_like(re)
    st = F.AcSweepStats()
    status = np.zeros(points, dtype=np.int32)
    def work():
        rc = lib.pe_hip_analyze_ac_sweep(e._h, points, F._dp(w), F._ip(status), C.byref(st))
        assert rc == 0, (rc, lib.pe_hip_last_error(e._h))
        assert lib.pe_hip_get_ac_sweep(e._h, 0, points, 0, batch, F._dp(re), F._dp(im)) == 0
        return re, im
t0 = time.perf_counter(); work(); warm = time.perf_counter() - t0
t0 = time.perf_counter(); r, i = work(); dt = time.perf_counter() - t0
if mode == "sweep":
    stats = st.asdict()
assert np.all(np.isfinite(r)) and np.all(np.isfinite(i))
pick = list(range(0, points, max(1, points // 8)))
print(json.dumps({"mode": mode, "batch": batch, "seconds": dt, "warmup_seconds": warm, "build_id": F.build_id(), "stats": stats,
                  "check": [[float(r[k, 0, 5]), float(i[k, 0, 5])] for k in pick]}))
'''


def child(root, mode, batch, points, timeout):
    env = dict(os.environ)
    env.pop("PE_HIP_LIB", None)  # each tree loads its own in-tree library
    r = subprocess.run([sys.executable, "-c", CHILD, root, mode, str(batch), str(points)], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{mode} at batch {batch} in {root}: exit {r.returncode}")  # nothing more is started on the GPU after a failure
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--points", type=int, default=200)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--timeout", type=int, default=280, help="seconds per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ac_sweep_timing.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    doc = {"workload": f"rc_mesh(100, 100, 1, True), {a.points} log-spaced points, omega 1e7 .. 1e11 rad/s", "repeats": a.repeats, "results": []}
    for batch in [int(b) for b in a.batches.split(",")]:
        loops, sweeps = [], []
        for _ in range(a.repeats):
            loops.append(child(os.path.abspath(a.parent_root), "loop", batch, a.points, a.timeout))
            sweeps.append(child(ROOT, "sweep", batch, a.points, a.timeout))
        ta, tb = [x["seconds"] for x in loops], [x["seconds"] for x in sweeps]
        # both paths solved the same systems: the sampled phasors agree to the AC tolerance
        ca, cb = loops[0]["check"], sweeps[0]["check"]
        agree = all(abs(complex(*p) - complex(*q)) <= 1e-9 + 1e-6 * abs(complex(*p)) for p, q in zip(ca, cb))
        res = {"batch": batch, "loop_parent_seconds": ta, "sweep_seconds": tb, "loop_parent_median": statistics.median(ta),
               "sweep_median": statistics.median(tb), "ratio": statistics.median(ta) / statistics.median(tb),
               "loop_parent_spread_seconds": max(ta) - min(ta), "gain_seconds": statistics.median(ta) - statistics.median(tb),
               "beats_spread": statistics.median(ta) - max(tb) > max(ta) - min(ta), "sampled_phasors_agree": agree,
               "loop_parent_warmup_seconds": [x["warmup_seconds"] for x in loops], "sweep_warmup_seconds": [x["warmup_seconds"] for x in sweeps],
               # the split of (b): gpu_ms is the HIP-event time of the passes; the rest is host work, above all one symbolic analysis per band
               "sweep_pass_seconds": [x["stats"]["gpu_ms"] / 1e3 for x in sweeps],
               "sweep_host_seconds_outside_passes": [x["seconds"] - x["stats"]["gpu_ms"] / 1e3 for x in sweeps],
               "sweep_stats": sweeps[-1]["stats"], "parent_build_id": loops[0]["build_id"], "build_id": sweeps[0]["build_id"]}
        doc["results"].append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
