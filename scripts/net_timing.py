#!/usr/bin/env python3
"""Times the network analysis (pe_hip_analyze_net) against the loop a user had to write before it existed, on rc_mesh(100, 100, 1, True)
with four ports (rows 0, 3366, 6733, 9999 against ground) and 200 logarithmic points from 1e7 to 1e11 rad/s, at batch 1 and 8:
  (a) loop   the PARENT commit's library: four AC current sources added at the ports, the mesh's own AC source set to zero; per port
             pe_hip_update_param switches the four amplitudes, one pe_hip_analyze_ac_sweep with pe_hip_set_ac_sweep_rows on the port rows
             gives a column of Z; Y and S in numpy
  (b) net    one pe_hip_analyze_net of this tree's library on the same circuit (it switches the sources off itself)
alternating (a), (b) `--repeats` times (>= 3) in one invocation.  Profiler off; every measurement is a fresh child process (one library per
process) that loads the circuit, solves the operating point, runs the whole measurement once to warm up (engines built, memory allocated)
and then times a second run with the host clock.  Expectation, written down before measuring: (b) pays one set of symbolic analyses and
numeric factorisations where (a) pays four, and the same number of triangular solves; the ratio (a)/(b) should therefore approach the number
of ports where the analyses dominate (batch 1) and be lower where the solves dominate.  No ratio is fixed in advance.

    python scripts/net_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/net_timing.json]

Writes one JSON document: per batch the wall and gpu_ms of every repeat, their medians, the spread of (a), the ratio (a)/(b), the statistics
of both, the largest difference between the two Z (relative to the largest entry) and the two build ids."""
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
rows = [0, 3366, 6733, 9999]
deck, r, c = D.rc_mesh_params(100, 100, list(range(1, batch + 1)), True)
for k in rows:
    deck.add("IAC", (0, k + 1), 0.0, 0.0, 0.0)       # a current into node k + 1 (row k); amplitude 0 until a port is excited
w = np.logspace(7.0, 11.0, 200)
z0 = np.full(4, 50.0)
e = F.Engine(device=0)
e.set_options(g_min=0.0)
e.load_deck(deck, batch, {"R": r[:, :, None], "C": c[:, :, None]})
e.reset()
e.analyze_dc(F.MODE_OP)
if mode == "loop":
    e.set_ac_sweep_rows(rows)
    e.update_param(F.VAC, 0, 0, 0.0)                 # the mesh's own AC source off (after the operating point, which it does not move)
    def call():
        Z = np.empty((len(w), batch, 4, 4), dtype=complex)
        gpu, st = 0.0, None
        for j in range(4):
            for k in range(4):
                e.update_param(F.IAC, k, 0, 1.0 if k == j else 0.0)
            x, _, st = e.analyze_ac_sweep(w)
            gpu += st["gpu_ms"]
            Z[:, :, :, j] = x
        Z0, Dm, Di = np.diag(z0), np.diag(np.sqrt(z0)), np.diag(1.0 / np.sqrt(z0))
        Y = np.linalg.inv(Z)
        S = Di @ (Z - Z0) @ np.linalg.inv(Z + Z0) @ Dm
        st = dict(st, gpu_ms=gpu, n_sweeps=4)
        return Z, st
else:
    def call():
        Z, Y, S, ys, ss, ps, st = e.analyze_net(w, [(k, -1) for k in rows], z0)
        return Z, st
call()
t0 = time.perf_counter()
Z, st = call()
wall = (time.perf_counter() - t0) * 1e3
pick = Z[[0, 99, 199]][:, 0]
print(json.dumps({"wall_ms": wall, "stats": {k: (float(v) if isinstance(v, float) else int(v)) for k, v in st.items()}, "build_id": F.build_id(),
                  "z_re": pick.real.tolist(), "z_im": pick.imag.tolist()}))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "net_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per measurement")
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    doc = {"circuit": "rc_mesh(100, 100, seeds 1.., True) + four IAC at the ports", "points": "logspace(7, 11, 200) rad/s",
           "ports": "rows 0, 3366, 6733, 9999 against ground, z0 = 50", "repeats": a.repeats, "batches": {}}
    for batch in [int(b) for b in a.batches.split(",")]:
        runs = {"loop": [], "net": []}
        for _ in range(a.repeats):
            for mode in ("loop", "net"):
                runs[mode].append(child(os.path.abspath(a.parent_root) if mode == "loop" else ROOT, mode, batch, a.timeout))
                print(batch, mode, runs[mode][-1]["wall_ms"], runs[mode][-1]["stats"], flush=True)
        med = {m: statistics.median(x["wall_ms"] for x in v) for m, v in runs.items()}
        gpu = {m: statistics.median(x["stats"]["gpu_ms"] for x in v) for m, v in runs.items()}
        lp = [x["wall_ms"] for x in runs["loop"]]
        za = [[complex(p, q) for p, q in zip(sum(sum(x["z_re"], []), []), sum(sum(x["z_im"], []), []))] for x in (runs["loop"][0], runs["net"][0])]
        gap = max(abs(p - q) for p, q in zip(*za)) / max(abs(q) for q in za[1])
        doc["batches"][str(batch)] = {
            "wall_ms": {m: [x["wall_ms"] for x in v] for m, v in runs.items()},
            "gpu_ms": {m: [x["stats"]["gpu_ms"] for x in v] for m, v in runs.items()},
            "median_wall_ms": med, "median_gpu_ms": gpu,
            "spread_of_loop": (max(lp) - min(lp)) / med["loop"],
            "loop_over_net": med["loop"] / med["net"], "loop_over_net_gpu_ms": gpu["loop"] / gpu["net"],
            "stats": {m: v[-1]["stats"] for m, v in runs.items()},
            "z_difference_relative": gap,
        }
        doc["build_id_parent"] = runs["loop"][0]["build_id"]
        doc["build_id"] = runs["net"][0]["build_id"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["batches"], indent=1))


if __name__ == "__main__":
    main()
