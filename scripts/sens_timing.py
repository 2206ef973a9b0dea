#!/usr/bin/env python3
"""Times the DC sensitivities of rc_mesh(100, 100, 1, True) with a 0.4 mA bias current into the node next to its centre, batch 8,
  (a) as what the PARENT commit offers for the same numbers: the loop pe_hip_update_param -> pe_hip_analyze_dc -> pe_hip_get_solution, one
      perturbed operating point per parameter, with the parent's library -- timed over a SAMPLE of `--sample` resistors spread over the
      table and SCALED to the n_params of the circuit (the figure in the file is an extrapolation and says so),
  (b) as one pe_hip_analyze_sens call with 1 output and with 8 outputs (every sensitivity kept, read back with pe_hip_get_sens) with
      this tree's library,
alternating (a), (b1), (b8) `--repeats` times (>= 3) in one invocation.  Profiler off; every measurement is a fresh child process (one
library per process) that loads the circuit, converges the operating point, runs the work once to warm up and then times it with the
host clock -- every call returns after a stream synchronise.  No ratio is fixed in advance.

    python scripts/sens_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/sens_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import ctypes as C, json, sys, time
root, mode, batch, count = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4])
sys.path.insert(0, root)
import numpy as np
import pe_load
pe = pe_load.load()
F = pe.ffi
lib = F.lib()
deck = pe.deck.rc_mesh(100, 100, 1, True)
deck.add("IDC", (0, 50 * 100 + 51), 4e-4)
e = F.Engine(device=0)
e.set_options(g_min=0.0)
e.load_deck(deck, batch)
e.reset()
e.analyze_dc(F.MODE_OP)
e.analyze_dc(F.MODE_OP)
n = e.rows
stats = {}
if mode == "loop":
    nR = deck.count("R")
    idx = [int(i) for i in np.linspace(0, nR - 1, count)]
    val = [p[0] for k, _, p in deck.devices if k == "R"]
    x0 = e.solution()
    x = np.empty((batch, n)); one = np.empty(1)
    def work():
        e.set_solution(x0)
        for i in idx:
            one[0] = val[i] * (1.0 + 1e-4)
            assert lib.pe_hip_update_param(e._h, F.R, i, 0, F._dp(one), 0) == 0
            assert lib.pe_hip_analyze_dc(e._h, F.MODE_OP, None) == 0
            assert lib.pe_hip_get_solution(e._h, 0, batch, F._dp(x)) == 0
            one[0] = val[i]
            assert lib.pe_hip_update_param(e._h, F.R, i, 0, F._dp(one), 0) == 0
        return x
else:
    pos = np.array([5050 + 101 * k for k in range(count)], dtype=np.int32) % deck.n_nodes
    def work():
        s, _, status, st = e.analyze_sens(pos, None)
        stats.update(st)
        return s
t0 = time.perf_counter(); work(); warm = time.perf_counter() - t0
t0 = time.perf_counter(); r = work(); dt = time.perf_counter() - t0
assert np.all(np.isfinite(r))
print(json.dumps({"mode": mode, "batch": batch, "count": count, "seconds": dt, "warmup_seconds": warm, "build_id": F.build_id(), "stats": stats}))
'''


def child(root, mode, batch, count, timeout):
    env = dict(os.environ)
    env.pop("PE_HIP_LIB", None)  # each tree loads its own in-tree library
    r = subprocess.run([sys.executable, "-c", CHILD, root, mode, str(batch), str(count)], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{mode} at batch {batch} in {root}: exit {r.returncode}")  # nothing more is started on the GPU after a failure
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=32, help="resistors the parent's loop is timed over")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sens_timing.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    runs = {"loop": [], "sens1": [], "sens8": []}
    for _ in range(a.repeats):
        runs["loop"].append(child(os.path.abspath(a.parent_root), "loop", a.batch, a.sample, a.timeout))
        runs["sens1"].append(child(ROOT, "sens", a.batch, 1, a.timeout))
        runs["sens8"].append(child(ROOT, "sens", a.batch, 8, a.timeout))
    n_params = runs["sens1"][0]["stats"]["n_params"]
    t = {k: [x["seconds"] for x in v] for k, v in runs.items()}
    med = {k: statistics.median(v) for k, v in t.items()}
    per_param = med["loop"] / a.sample
    doc = {"workload": "rc_mesh(100, 100, 1, True) + IDC 0.4 mA into node 5051, mode OP, batch %d, %d parameters" % (a.batch, n_params),
           "repeats": a.repeats,
           "loop_parent": {"what": "pe_hip_update_param -> pe_hip_analyze_dc -> pe_hip_get_solution -> pe_hip_update_param (back) per parameter, parent library",
                           "sampled_parameters": a.sample, "seconds": t["loop"], "median_seconds": med["loop"], "seconds_per_parameter": per_param,
                           "SCALED_to_n_params_seconds": per_param * n_params,
                           "note": "SCALED: measured over the sample only and multiplied by n_params / sample; one output or eight cost the loop the same",
                           "build_id": runs["loop"][0]["build_id"]},
           "analyze_sens_1_output": {"seconds": t["sens1"], "median_seconds": med["sens1"], "stats": runs["sens1"][-1]["stats"]},
           "analyze_sens_8_outputs": {"seconds": t["sens8"], "median_seconds": med["sens8"], "stats": runs["sens8"][-1]["stats"]},
           "ratio_scaled_loop_over_sens_1": per_param * n_params / med["sens1"], "ratio_scaled_loop_over_sens_8": per_param * n_params / med["sens8"],
           "warmup_seconds": {k: [x["warmup_seconds"] for x in v] for k, v in runs.items()},
           "build_id": runs["sens1"][0]["build_id"]}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
