#!/usr/bin/env python3
"""Times the pole-zero analysis (pe_hip_analyze_pz) against what a user could do before it existed:
  (a) dense   the PARENT commit's library: pe_hip_analyze_ac at omega = 1 and omega = 2, pe_hip_get_matrix_ac after each (the real-equivalent
              2N system; G from its upper-left block, B from the difference of the lower-left blocks), scipy.linalg.eig of the dense pencil
              (-G, B) per instance -- O(N^3), feasible up to about a thousand rows
  (b) pz      one pe_hip_analyze_pz of this tree's library: poles only, n_wanted = 8, max_krylov = 32, omega0 = --omega0
on rc_mesh(32, 32, seeds 1.., True) at batch 1 and 8, alternating (a), (b) `--repeats` times (>= 3) in one invocation, and (b) alone on
rc_mesh(100, 100, seeds 1.., True) (10 002 rows: (a) is not feasible there -- a dense complex eigenproblem of that order takes hours and
1.6 GB per instance).  Profiler off; every measurement is a fresh child process (one library per process) that loads the circuit, solves the
operating point, runs the whole measurement once to warm up and then times a second run with the host clock.  The accuracy of both is
reported against each other: the 8 poles (b) returns, each against the nearest of (a)'s, relative to |s - s0|.

Expectation, written down before measuring: (b) costs one band analysis on the host, one factorisation and about 34 kept-factor solves with
their refinement rounds; every solve is a handful of launches and two host round trips (the refinement's one-int read, the solve's own
synchronisation), so at batch 1 the round trips should dominate and the time should hardly grow from batch 1 to 8.  No ratio is fixed in
advance.

    python scripts/pz_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/pz_timing.json]

Writes one JSON document: per circuit and batch the wall and gpu_ms of every repeat, their medians, the spread of (a), the ratio (a)/(b), the
statistics of (b), the accuracy figure and the two build ids."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys, time
root, mode, side, batch, w0 = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5])
sys.path.insert(0, root)
import numpy as np
import pe_load
pe = pe_load.load()
F, D = pe.ffi, pe.deck
deck, r, c = D.rc_mesh_params(side, side, list(range(1, batch + 1)), True)
e = F.Engine(device=0)
e.set_options(g_min=0.0)
e.load_deck(deck, batch, {"R": r[:, :, None], "C": c[:, :, None]})
e.reset()
e.analyze_dc(F.MODE_OP)
N = e.rows
if mode == "dense":
    import scipy.linalg as sl
    import scipy.sparse as sp
    def call():
        mats = []
        for w in (1.0, 2.0):
            e.analyze_ac(w)
            per = []
            for b in range(batch):
                rp, ci, vals, _ = e.matrix_ac(0, b, rhs=False)
                per.append(sp.csr_matrix((vals, ci, rp), shape=(2 * N, 2 * N)).toarray())
            mats.append(per)
        out = []
        for b in range(batch):
            G, B = mats[0][b][:N, :N], mats[1][b][N:, :N] - mats[0][b][N:, :N]
            ev = sl.eig(-G, B, right=False)
            ev = ev[np.isfinite(ev)]
            out.append(ev[np.argsort(np.abs(ev - 1j * w0))][:8])
        return np.array(out), {"gpu_ms": 0.0}
else:
    def call():
        st, stats = e.analyze_pz(w0, F.PZ_POLES, 8, 32)
        s, err, nf, nc, cp = e.pz(F.PZ_POLES, 32)
        return s[:, :8], dict(stats, n_converged=[int(v) for v in nc])
call()
t0 = time.perf_counter()
s, st = call()
wall = (time.perf_counter() - t0) * 1e3
print(json.dumps({"wall_ms": wall, "stats": st, "build_id": F.build_id(), "s_re": s.real.tolist(), "s_im": s.imag.tolist()}))
'''


def child(root, mode, side, batch, w0, timeout):
    env = dict(os.environ)
    env.pop("PE_HIP_LIB", None)  # each tree loads its own in-tree library through its own Python layer
    r = subprocess.run([sys.executable, "-c", CHILD, root, mode, str(side), str(batch), repr(w0)], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"{mode} side {side} batch {batch} in {root}: exit {r.returncode}\n{r.stderr[-3000:]}")  # nothing more is started on the GPU after a failure
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pz_timing.json"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--omega0", type=float, default=1e8)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per measurement")
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    doc = {"omega0": a.omega0, "pz": "poles, n_wanted 8, max_krylov 32", "repeats": a.repeats, "circuits": {}}
    for side, modes in ((32, ("dense", "pz")), (100, ("pz",))):
        per = {}
        for batch in [int(b) for b in a.batches.split(",")]:
            runs = {m: [] for m in modes}
            for _ in range(a.repeats):
                for mode in modes:
                    runs[mode].append(child(os.path.abspath(a.parent_root) if mode == "dense" else ROOT, mode, side, batch, a.omega0, a.timeout))
                    print(side, batch, mode, runs[mode][-1]["wall_ms"], runs[mode][-1]["stats"], flush=True)
            med = {m: statistics.median(x["wall_ms"] for x in v) for m, v in runs.items()}
            entry = {"wall_ms": {m: [x["wall_ms"] for x in v] for m, v in runs.items()}, "median_wall_ms": med,
                     "gpu_ms_pz": [x["stats"]["gpu_ms"] for x in runs["pz"]], "stats_pz": runs["pz"][-1]["stats"]}
            if "dense" in runs:
                dn = [x["wall_ms"] for x in runs["dense"]]
                entry["spread_of_dense"] = (max(dn) - min(dn)) / med["dense"]
                entry["dense_over_pz"] = med["dense"] / med["pz"]
                worst = 0.0
                for b in range(batch):
                    sa = [complex(p, q) for p, q in zip(runs["dense"][0]["s_re"][b], runs["dense"][0]["s_im"][b])]
                    sb = [complex(p, q) for p, q in zip(runs["pz"][0]["s_re"][b], runs["pz"][0]["s_im"][b])]
                    for v in sb:
                        if v == v:
                            worst = max(worst, min(abs(v - u) for u in sa) / abs(v - 1j * a.omega0))
                entry["pz_against_dense_relative"] = worst
                doc["build_id_parent"] = runs["dense"][0]["build_id"]
            doc["build_id"] = runs["pz"][0]["build_id"]
            per[str(batch)] = entry
        doc["circuits"]["rc_mesh(%d, %d, seeds 1.., True)" % (side, side)] = per
    doc["note"] = "the dense pencil is not feasible on rc_mesh(100, 100): a complex eigenproblem of order 10 002 per instance"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["circuits"], indent=1))


if __name__ == "__main__":
    main()
