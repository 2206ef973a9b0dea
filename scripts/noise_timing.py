#!/usr/bin/env python3
"""Times the noise analysis (pe_hip_analyze_noise) against the forward sweep it shares its body with, on rc_mesh(100, 100, 1, True) with
200 logarithmic points from 1e7 to 1e11 rad/s, at batch 1 and 8:
  (a) sweep    pe_hip_analyze_ac_sweep of the PARENT commit's library with two kept rows
  (b) noise    pe_hip_analyze_noise of this tree's library, contributions not kept
  (c) contrib  (b) with the contributions of every source kept
alternating (a), (b), (c) `--repeats` times (>= 3) in one invocation.  Profiler off; every measurement is a fresh child process (one library
per process) that loads the circuit, solves the operating point, runs the call once to warm up (engines built, memory allocated) and then
times a second call with the host clock.  Expectation, written down before measuring: (b) does the same number of analyses,
factorisations and solves as (a) on a system of the same pattern, so it should cost about the same; no threshold is fixed in advance.  The
direct method -- one forward sweep per source -- is n_sources x (a): an extrapolation, reported as such.

    python scripts/noise_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/noise_timing.json]

Writes one JSON document: per batch the wall and gpu_ms of every repeat, their medians, the spread of (a), (b)/(a), (c)/(b), the pass
statistics, the extrapolated direct method and the two build ids."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys, time
root, mode, batch = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, root)
import numpy as np
import pe_load
pe = pe_load.load()
F, D = pe.ffi, pe.deck
deck, r, c = D.rc_mesh_params(100, 100, list(range(1, batch + 1)), True)
w = np.logspace(7.0, 11.0, 200)
e = F.Engine(device=0)
e.set_options(g_min=0.0)
e.load_deck(deck, batch, {"R": r[:, :, None], "C": c[:, :, None]})
e.reset()
e.analyze_dc(F.MODE_OP)
if mode == "sweep":
    e.set_ac_sweep_rows([5049, 0])
    call = lambda: e.analyze_ac_sweep(w)[2]
else:
    call = lambda: e.analyze_noise(w, 5049, -1, contributions=(mode == "contrib"))[3]
call()
t0 = time.perf_counter()
st = call()
wall = (time.perf_counter() - t0) * 1e3
print(json.dumps({"wall_ms": wall, "stats": {k: (float(v) if isinstance(v, float) else int(v)) for k, v in st.items()}, "build_id": F.build_id()}))
'''


def child(root, mode, batch, timeout):
    env = dict(os.environ)
    env.pop("PE_HIP_LIB", None)  # each tree loads its own in-tree library through its own Python layer
    r = subprocess.run([sys.executable, "-c", CHILD, root, mode, str(batch)], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"{mode} batch {batch} in {root}: exit {r.returncode}\n{r.stderr[-3000:]}")  # nothing more is started on the GPU after a failure
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per measurement")
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    doc = {"circuit": "rc_mesh(100, 100, seeds 1.., True)", "points": "logspace(7, 11, 200) rad/s", "output": "row 5049", "repeats": a.repeats, "batches": {}}
    for batch in [int(b) for b in a.batches.split(",")]:
        runs = {"sweep": [], "noise": [], "contrib": []}
        for _ in range(a.repeats):
            for mode in ("sweep", "noise", "contrib"):
                runs[mode].append(child(os.path.abspath(a.parent_root) if mode == "sweep" else ROOT, mode, batch, a.timeout))
                print(batch, mode, runs[mode][-1]["wall_ms"], runs[mode][-1]["stats"], flush=True)
        med = {m: statistics.median(x["wall_ms"] for x in v) for m, v in runs.items()}
        gpu = {m: statistics.median(x["stats"]["gpu_ms"] for x in v) for m, v in runs.items()}
        sw = [x["wall_ms"] for x in runs["sweep"]]
        n_src = runs["noise"][0]["stats"]["n_sources"]
        doc["batches"][str(batch)] = {
            "wall_ms": {m: [x["wall_ms"] for x in v] for m, v in runs.items()},
            "gpu_ms": {m: [x["stats"]["gpu_ms"] for x in v] for m, v in runs.items()},
            "median_wall_ms": med, "median_gpu_ms": gpu,
            "spread_of_sweep": (max(sw) - min(sw)) / med["sweep"],
            "noise_over_sweep": med["noise"] / med["sweep"], "contrib_over_noise": med["contrib"] / med["noise"],
            "stats": {m: v[-1]["stats"] for m, v in runs.items()},
            "n_sources": n_src,
            "direct_method_extrapolated_s": n_src * med["sweep"] / 1e3,
        }
        doc["build_id_parent"] = runs["sweep"][0]["build_id"]
        doc["build_id"] = runs["noise"][0]["build_id"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["batches"], indent=1))


if __name__ == "__main__":
    main()
