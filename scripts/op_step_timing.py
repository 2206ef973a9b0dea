#!/usr/bin/env python3
"""Times the stepped operating point of rc_mesh(100, 100, 1, True) -- its VAC source replaced by a VDC in the same place -- at batch 1 and
batch 64, the source value spread over the instances (geometric, --v-lo .. --v-hi; batch 1: --v-hi) so that the low ones converge directly
and the others fail cold at the Newton cap --cap,
  (a) as the same source-stepping rule run by a host-side controller on the PARENT commit's library: pe_hip_update_param (the batched
      source values at every instance's own lambda) -> pe_hip_analyze_dc -> pe_hip_get_instance_state -> pe_hip_get_solution, and
      pe_hip_set_solution to put a rejected instance back on its last accepted solution.  The parent cannot park an instance, so every
      level solves the whole batch (a finished instance is solved again from its solution), and its junction state cannot be put back;
  (b) as one pe_hip_analyze_op_stepping (PE_HIP_STEP_SOURCE) with this tree's library,
alternating (a), (b) `--repeats` times (>= 3) in one invocation.  Profiler off; every measurement is a fresh child process (one library per
process) that loads the circuit, runs the work once from the reset state to warm up (symbolic analysis made, memory allocated) and then
times it from the reset state with the host clock.  The yardstick is (a) on the parent.  No ratio is fixed in advance: the script records
both times, the level, rejection and iteration counts, and where (b)'s time goes (its solves against its controller launches).

    python scripts/op_step_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/op_step_timing.json]
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
root, mode, batch, cap, v_lo, v_hi = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), float(sys.argv[5]), float(sys.argv[6])
sys.path.insert(0, root)
import numpy as np
import pe_load
pe = pe_load.load()
F = pe.ffi
lib = F.lib()
deck = pe.deck.rc_mesh(100, 100, 1, True)
(i,) = [i for i, (k, _, _) in enumerate(deck.devices) if k == "VAC"]
deck.devices[i] = ("VDC", deck.devices[i][1], (1.0,))
volts = np.geomspace(v_lo, v_hi, batch) if batch > 1 else np.array([v_hi])
e = F.Engine(device=0)
e.set_options(g_min=0.0, max_newton=cap)
e.load_deck(deck, batch, {"VDC": volts[:, None, None]})
n = e.rows
counts = {}
if mode == "host":
    DL, GROW, SHRINK, DLMIN, MAXLEV = 0.125, 2.0, 0.25, 2.0 ** -20, 200
    status = np.zeros(batch, dtype=np.int32)
    x = np.zeros((batch, n))
    def solve(lam):
        col = np.ascontiguousarray(lam * volts)
        assert lib.pe_hip_update_param(e._h, F.VDC, 0, 0, F._dp(col), 1) == 0
        lib.pe_hip_analyze_dc(e._h, F.MODE_OP, None)
        assert lib.pe_hip_get_instance_state(e._h, 0, batch, F._ip(status), None, None, None) == 0
        assert lib.pe_hip_get_solution(e._h, 0, batch, F._dp(x)) == 0
        return (status == 0) & np.isfinite(x).all(axis=1)
    def work():
        e.reset()
        ok = solve(np.ones(batch))
        step = ~ok                                   # instances that step; the others are solved again at lambda = 1 with every level
        direct = int(ok.sum())
        lam, delta, cand = np.where(step, 0.0, 1.0), np.full(batch, DL), np.where(step, 0.0, 1.0)
        first, failed = step.copy(), np.zeros(batch, dtype=bool)
        shadow = np.where(step[:, None], 0.0, x)
        levels = rejected = solves = 0
        if step.any():
            assert lib.pe_hip_set_solution(e._h, 0, batch, F._dp(np.ascontiguousarray(shadow))) == 0
        while step.any() and solves < MAXLEV:
            ok = solve(cand)
            solves += 1
            levels += int(step.sum())
            for b in np.nonzero(step)[0]:
                if ok[b]:
                    shadow[b], lam[b] = x[b], cand[b]
                    if first[b]:
                        first[b] = False
                    else:
                        delta[b] *= GROW
                    if cand[b] >= 1.0:
                        step[b] = False
                else:
                    rejected += 1
                    if first[b]:
                        failed[b] = True
                    else:
                        delta[b] *= SHRINK
                        failed[b] = delta[b] < DLMIN
                    if failed[b]:
                        step[b] = False
                if step[b]:
                    cand[b] = min(1.0, lam[b] + delta[b])
            # every instance back on its last accepted solution (the accepted ones are there already)
            assert lib.pe_hip_set_solution(e._h, 0, batch, F._dp(np.ascontiguousarray(shadow))) == 0
        assert lib.pe_hip_update_param(e._h, F.VDC, 0, 0, F._dp(np.ascontiguousarray(volts)), 1) == 0
        counts.update(n_levels=levels, n_rejected=rejected, n_solves=solves + 1, n_failed=int(failed.sum()), n_direct=direct)
        return shadow
else:
    st = F.OpStepStats()
    ctl = F.op_step_control(F.STEP_SOURCE, step_max_newton=cap, log_capacity=0)
    def work():
        e.reset()
        rc = lib.pe_hip_analyze_op_stepping(e._h, F.MODE_OP, C.byref(ctl), C.byref(st))
        assert rc == 0, (rc, lib.pe_hip_last_error(e._h))
        counts.update(st.asdict())
        return e.solution()
t0 = time.perf_counter(); work(); warm = time.perf_counter() - t0
i0 = int(e.state()["iters"].sum())     # (reset() clears the counters: this is the warm-up's count, the timed run's follows)
t0 = time.perf_counter(); r = work(); dt = time.perf_counter() - t0
counts["engine_newton_iters_converged_solves"] = int(e.state()["iters"].sum())
assert np.all(np.isfinite(r))
print(json.dumps({"mode": mode, "batch": batch, "seconds": dt, "warmup_seconds": warm, "build_id": F.build_id(), "counts": counts,
                  "check": [float(r[b, 5]) for b in sorted({0, batch // 2, batch - 1})]}))
'''


def child(root, mode, batch, a):
    env = dict(os.environ)
    env.pop("PE_HIP_LIB", None)  # each tree loads its own in-tree library
    r = subprocess.run([sys.executable, "-c", CHILD, root, mode, str(batch), str(a.cap), str(a.v_lo), str(a.v_hi)], env=env, capture_output=True, text=True,
                       timeout=a.timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{mode} at batch {batch} in {root}: exit {r.returncode}")  # nothing more is started on the GPU after a failure
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--cap", type=int, default=12, help="max_newton of the engine and of the stepping levels")
    ap.add_argument("--v-lo", type=float, default=0.3)
    ap.add_argument("--v-hi", type=float, default=40.0)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "op_step_timing.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    doc = {"workload": f"rc_mesh(100, 100, 1, True) with its source as a VDC, {a.v_lo} .. {a.v_hi} V spread geometrically over the batch (batch 1: {a.v_hi} V), "
                       f"mode OP from the reset state, max_newton {a.cap}, source stepping with the defaults of include/pe_hip.h",
           "repeats": a.repeats, "results": []}
    for batch in [int(b) for b in a.batches.split(",")]:
        runs = {"host": [], "device": []}
        for _ in range(a.repeats):
            runs["host"].append(child(os.path.abspath(a.parent_root), "host", batch, a))
            runs["device"].append(child(ROOT, "device", batch, a))
        t = {k: [x["seconds"] for x in v] for k, v in runs.items()}
        med = {k: statistics.median(v) for k, v in t.items()}
        tol = lambda p, q: abs(p - q) <= 1e-6 + 1e-5 * abs(p)  # noqa: E731  (the project's non-linear tolerance)
        dev = runs["device"]
        res = {"batch": batch, "host_controller_parent_seconds": t["host"], "device_controller_seconds": t["device"],
               "host_controller_parent_median": med["host"], "device_controller_median": med["device"],
               "ratio_host_over_device": med["host"] / med["device"], "host_controller_parent_spread_seconds": max(t["host"]) - min(t["host"]),
               "sampled_values_agree": all(tol(p, q) for p, q in zip(runs["host"][0]["check"], dev[0]["check"])),
               "warmup_seconds": {k: [x["warmup_seconds"] for x in v] for k, v in runs.items()},
               # where (b)'s time goes: gpu_ms is the HIP-event time of the whole call (solves with their host round trips + controller
               # launches), control_ms the host time of the controller launches with their read-backs, the rest of `seconds` host work
               # outside the stream (tables, uploads, the final status read)
               "device_call_gpu_seconds": [x["counts"]["gpu_ms"] / 1e3 for x in dev],
               "device_controller_launch_seconds": [x["counts"]["control_ms"] / 1e3 for x in dev],
               "device_seconds_outside_the_stream": [x["seconds"] - x["counts"]["gpu_ms"] / 1e3 for x in dev],
               "host_counts": runs["host"][-1]["counts"], "device_counts": dev[-1]["counts"],
               "parent_build_id": runs["host"][0]["build_id"], "build_id": dev[0]["build_id"]}
        doc["results"].append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
