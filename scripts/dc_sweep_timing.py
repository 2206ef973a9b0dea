#!/usr/bin/env python3
"""Times a 200-point DC sweep of the source of rc_mesh(100, 100, 1, True) -- its VAC source replaced by a VDC in the same place, the only
kind of source a DC sweep steps -- over -1 .. 3 V, batch 1 and batch 8,
  (a) as the loop pe_hip_update_param -> pe_hip_analyze_dc -> pe_hip_get_solution with the PARENT commit's library,
  (b) as one pe_hip_analyze_dc_sweep (PARALLEL, continuation on) + pe_hip_get_dc_sweep with this tree's library,
  (c) as one pe_hip_analyze_dc_sweep (TRACE) + pe_hip_get_dc_sweep with this tree's library,
alternating (a), (b), (c) `--repeats` times (>= 3) in one invocation.  Profiler off; every measurement is a fresh child process (one
library per process) that loads the circuit, runs the work once to warm up (engines built, symbolic analyses made, memory allocated) and
then times it with the host clock -- every call returns after a stream synchronise.  The yardstick is (a) on the parent, never this
tree's own loop.  No ratio is fixed in advance: the script reports (a)/(b) and (a)/(c) beside the spread of (a), and where the time of
(b) outside its passes goes.

    python scripts/dc_sweep_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/dc_sweep_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import copy, ctypes as C, json, sys, time
root, mode, batch, points = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
sys.path.insert(0, root)
import numpy as np
import pe_load
pe = pe_load.load()
F = pe.ffi
lib = F.lib()
deck = pe.deck.rc_mesh(100, 100, 1, True)
(i,) = [i for i, (k, _, _) in enumerate(deck.devices) if k == "VAC"]
deck.devices[i] = ("VDC", deck.devices[i][1], (1.0,))
v = np.linspace(-1.0, 3.0, points)
e = F.Engine(device=0)
e.set_options(g_min=0.0)
e.load_deck(deck, batch)
e.reset()
n = e.rows
x = np.empty((points, batch, n))
stats = {}
if mode == "loop":
    blob = e.checkpoint()
    one = np.empty(1)
    def work():
        e.restore(blob)                                 # every run from the same state, as the sweeps start from the engine's
        for k in range(points):
            one[0] = v[k]
            assert lib.pe_hip_update_param(e._h, F.VDC, 0, 0, F._dp(one), 0) == 0
            rc = lib.pe_hip_analyze_dc(e._h, F.MODE_OP, None)
            assert rc == 0, (k, v[k], rc)
            assert lib.pe_hip_get_solution(e._h, 0, batch, F._dp(x[k])) == 0
        return x
else:
    st = F.DcSweepStats()
    status = np.zeros(points, dtype=np.int32)
    ctl = F.DcSweepControl(F.VDC, 0, 0, F.MODE_OP, F.DC_SWEEP_TRACE if mode == "trace" else F.DC_SWEEP_PARALLEL, 1, 0)
    def work():
        rc = lib.pe_hip_analyze_dc_sweep(e._h, points, F._dp(v), C.byref(ctl), F._ip(status), C.byref(st))
        assert rc == 0, (rc, lib.pe_hip_last_error(e._h))
        assert lib.pe_hip_get_dc_sweep(e._h, 0, points, 0, batch, F._dp(x)) == 0
        return x
t0 = time.perf_counter(); work(); warm = time.perf_counter() - t0
t0 = time.perf_counter(); r = work(); dt = time.perf_counter() - t0
if mode != "loop":
    stats = st.asdict()
assert np.all(np.isfinite(r))
pick = list(range(0, points, max(1, points // 8)))
print(json.dumps({"mode": mode, "batch": batch, "seconds": dt, "warmup_seconds": warm, "build_id": F.build_id(), "stats": stats,
                  "check": [float(r[k, 0, 5]) for k in pick]}))
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
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dc_sweep_timing.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    doc = {"workload": f"rc_mesh(100, 100, 1, True) with its source as a VDC, {a.points} points, -1 .. 3 V, mode OP, from the reset state",
           "repeats": a.repeats, "results": []}
    for batch in [int(b) for b in a.batches.split(",")]:
        runs = {"loop": [], "parallel": [], "trace": []}
        for _ in range(a.repeats):
            runs["loop"].append(child(os.path.abspath(a.parent_root), "loop", batch, a.points, a.timeout))
            runs["parallel"].append(child(ROOT, "parallel", batch, a.points, a.timeout))
            runs["trace"].append(child(ROOT, "trace", batch, a.points, a.timeout))
        t = {k: [x["seconds"] for x in v] for k, v in runs.items()}
        med = {k: statistics.median(v) for k, v in t.items()}
        tol = lambda p, q: abs(p - q) <= 1e-6 + 1e-5 * abs(p)  # noqa: E731  (the project's non-linear tolerance)
        res = {"batch": batch, "loop_parent_seconds": t["loop"], "parallel_seconds": t["parallel"], "trace_seconds": t["trace"],
               "loop_parent_median": med["loop"], "parallel_median": med["parallel"], "trace_median": med["trace"],
               "ratio_loop_over_parallel": med["loop"] / med["parallel"], "ratio_loop_over_trace": med["loop"] / med["trace"],
               "loop_parent_spread_seconds": max(t["loop"]) - min(t["loop"]),
               "sampled_values_agree": all(tol(p, q) and tol(p, r) for p, q, r in zip(runs["loop"][0]["check"], runs["parallel"][0]["check"], runs["trace"][0]["check"])),
               "warmup_seconds": {k: [x["warmup_seconds"] for x in v] for k, v in runs.items()},
               # the split of (b): gpu_ms is the HIP-event time of the passes (fill, seed, solves with their host round trips, classify, gather);
               # the rest is host work: slot tables, the copies of the result, a symbolic analysis when the sweep engine is rebuilt
               "parallel_pass_seconds": [x["stats"]["gpu_ms"] / 1e3 for x in runs["parallel"]],
               "parallel_host_seconds_outside_passes": [x["seconds"] - x["stats"]["gpu_ms"] / 1e3 for x in runs["parallel"]],
               "trace_pass_seconds": [x["stats"]["gpu_ms"] / 1e3 for x in runs["trace"]],
               "parallel_stats": runs["parallel"][-1]["stats"], "trace_stats": runs["trace"][-1]["stats"],
               "parent_build_id": runs["loop"][0]["build_id"], "build_id": runs["parallel"][0]["build_id"]}
        doc["results"].append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
