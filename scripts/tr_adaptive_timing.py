#!/usr/bin/env python3
"""Times the variable-step transient (pe_hip_analyze_tr_adaptive) against the two things it has to be compared with, on four workloads:
the bridge rectifier 0 .. 40 ms, rc_mesh(100, 100, 1, True) at batch 1 and 8, and the Monte-Carlo sweep's size (1 024 instances of the
non-linear 100 x 100 mesh) -- the meshes for a fixed number of attempted steps.
  (a) host    a host-side controller with the same rule, written against the PARENT commit's library and its public calls only:
              checkpoint -> analyze_tr(h, 1) -> solution -> the LTE test in numpy -> restore on rejection (two state copies over the host
              link per step)
  (b) device  one pe_hip_analyze_tr_adaptive of this tree's library
  (c) floor   pe_hip_analyze_tr of this tree's library: as many steps as (b) attempted, of (b)'s mean step
alternating (a), (b), (c) `--repeats` times (>= 3) in one invocation.  Profiler off; every measurement is a fresh child process (one library
per process) that loads the circuit, runs the work once to warm up (symbolic analyses of the dt range made, memory allocated), resets and
then times it with the host clock -- every call returns after a stream synchronise.  No ratio is fixed in advance: the claim to confirm or
refute is that (b) sits close to (c) while (a) pays for its copies.

    python scripts/tr_adaptive_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/tr_adaptive_timing.json]

Writes one JSON document: per workload the times of every repeat, their medians and spreads, (a)/(b), (b)/(c), the step counts of (a) and
(b), the Newton iterations of (b) and (c) and the two build ids."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, sys, time
root, mode, case, n_att, mean_dt = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), float(sys.argv[5])
sys.path.insert(0, root)
import numpy as np
import pe_load
pe = pe_load.load()
F, D = pe.ffi, pe.deck
RELTOL, ABS_V, ABS_I, TRTOL = 1e-3, 1e-6, 1e-9, 7.0
if case == "bridge":
    deck, batch, ov, gmin, t_stop, dt_init, cap = D.bridge_rectifier(), 1, None, 1e-12, 0.04, 1e-6, 0
else:
    batch = {"mesh_b1": 1, "mesh_b8": 8, "sweep_b1024": 1024}[case]
    deck, r, c = D.rc_mesh_params(100, 100, list(range(1, batch + 1)), True)
    ov, gmin, t_stop, dt_init, cap = {"R": r[:, :, None], "C": c[:, :, None]}, 0.0, 1e-6, 2e-11, n_att
dt_max, dt_min = t_stop / 50, dt_init * 1e-9
e = F.Engine(device=0)
e.set_options(g_min=gmin)
e.load_deck(deck, batch, ov)
e.reset()
nn = deck.n_nodes
info = {}

def host_controller():
    """the rule of include/pe_hip.h with today's calls; returns (accepted, rejected)"""
    abstol = np.where(np.arange(e.rows) < nn, ABS_V, ABS_I)
    t, dt, T, X, n_acc, n_rej = 0.0, dt_init, [], [], 0, 0
    while t < t_stop * (1 - 1e-15) and (cap <= 0 or n_acc + n_rej < cap):
        h = min(dt, dt_max, t_stop - t)
        ck = e.checkpoint()
        rc = e.analyze_tr(h, 1, check=False)["rc"]
        if rc != 0:
            e.restore(ck); dt = max(h / 8, dt_min); n_rej += 1
            continue
        x = e.solution()
        tn = t + h
        q = None
        if len(T) >= 3:
            tt = T[-3:] + [tn]; xx = X[-3:] + [x]
            d10, d21, dn2 = (xx[1] - xx[0]) / (tt[1] - tt[0]), (xx[2] - xx[1]) / (tt[2] - tt[1]), (xx[3] - xx[2]) / (tt[3] - tt[2])
            dd3 = ((dn2 - d21) / (tt[3] - tt[1]) - (d21 - d10) / (tt[2] - tt[0])) / (tt[3] - tt[0])
            q = float(np.max(0.5 * h * h * h * np.abs(dd3) / (TRTOL * (RELTOL * np.maximum(np.abs(xx[3]), np.abs(xx[2])) + abstol))))
            if not q <= 1.0 and h > dt_min:
                e.restore(ck); n_rej += 1
                dt = max(h * max(0.1, 0.9 * q ** (-1.0 / 3.0)), dt_min)
                continue
        T.append(tn); X.append(x); T, X = T[-3:], X[-3:]
        t, n_acc = tn, n_acc + 1
        dt = h if q is None else h * (min(2.0, 0.9 * q ** (-1.0 / 3.0)) if q > 0 else 2.0)
    return n_acc, n_rej

if mode == "host":
    def work():
        a, r = host_controller()
        info.update(accepted=a, rejected=r)
elif mode == "device":
    def work():
        st = e.analyze_tr_adaptive(t_stop, dt_init, lte_reltol=RELTOL, lte_abstol_v=ABS_V, lte_abstol_i=ABS_I, trtol=TRTOL, max_steps=cap)
        info.update(accepted=st["n_accepted"], rejected=st["n_rejected_lte"] + st["n_rejected_newton"], mean_dt=float(np.mean(e.tr_step_log()[0])),
                    gpu_ms=st["run"]["gpu_ms"], n_analyses=st["n_analyses"], newton_iters=st["run"]["newton_iters"] + st["newton_iters_rejected"])
else:
    def work():
        st = e.analyze_tr(mean_dt, n_att, check=False)
        assert st["rc"] == 0 and st["steps"] == batch * n_att, st   # the floor took every one of its steps
        info.update(accepted=n_att, rejected=0, rc=st["rc"], newton_iters=st["newton_iters"])
t0 = time.perf_counter(); work(); warm = time.perf_counter() - t0
e.reset()
t0 = time.perf_counter(); work(); dt_s = time.perf_counter() - t0
assert np.all(np.isfinite(e.solution()))
print(json.dumps(dict(info, mode=mode, case=case, seconds=dt_s, warmup_seconds=warm, build_id=F.build_id())))
'''


def child(root, mode, case, n_att, mean_dt, timeout):
    env = dict(os.environ)
    env.pop("PE_HIP_LIB", None)  # each tree loads its own in-tree library
    r = subprocess.run([sys.executable, "-c", CHILD, root, mode, case, str(n_att), repr(mean_dt)], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{mode} on {case} in {root}: exit {r.returncode}")  # nothing more is started on the GPU after a failure
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cases", default="bridge,mesh_b1,mesh_b8,sweep_b1024")
    ap.add_argument("--mesh-steps", type=int, default=40, help="attempted steps of the mesh workloads")
    ap.add_argument("--sweep-steps", type=int, default=20, help="attempted steps at the sweep's size")
    ap.add_argument("--timeout", type=int, default=280, help="seconds per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tr_adaptive_timing.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    doc = {"tolerances": "lte_reltol 1e-3, abstol_v 1e-6, abstol_i 1e-9, trtol 7", "repeats": a.repeats, "results": []}
    med = statistics.median
    for case in a.cases.split(","):
        cap = 0 if case == "bridge" else (a.sweep_steps if case == "sweep_b1024" else a.mesh_steps)
        host, dev, floor = [], [], []
        for _ in range(a.repeats):
            host.append(child(os.path.abspath(a.parent_root), "host", case, cap, 0.0, a.timeout))
            dev.append(child(ROOT, "device", case, cap, 0.0, a.timeout))
            n_att = dev[-1]["accepted"] + dev[-1]["rejected"]
            floor.append(child(ROOT, "floor", case, n_att, dev[-1]["mean_dt"], a.timeout))
        ta, tb, tc = ([x["seconds"] for x in v] for v in (host, dev, floor))
        res = {"case": case, "host_parent_seconds": ta, "device_seconds": tb, "floor_seconds": tc,
               "host_parent_median": med(ta), "device_median": med(tb), "floor_median": med(tc),
               "host_over_device": med(ta) / med(tb), "device_over_floor": med(tb) / med(tc),
               "spread_seconds": {"host_parent": max(ta) - min(ta), "device": max(tb) - min(tb), "floor": max(tc) - min(tc)},
               "steps_host": [host[-1]["accepted"], host[-1]["rejected"]], "steps_device": [dev[-1]["accepted"], dev[-1]["rejected"]],
               "device_mean_dt": dev[-1]["mean_dt"], "device_gpu_ms": [x["gpu_ms"] for x in dev], "device_n_analyses": dev[-1]["n_analyses"],
               # solve_once-equivalents summed over instances: (b) incl. its rejected steps, (c) at the mean step -- the two do not do the same work
               "newton_iters_device": dev[-1]["newton_iters"], "newton_iters_floor": floor[-1]["newton_iters"], "floor_rc": floor[-1]["rc"],
               "parent_build_id": host[0]["build_id"], "build_id": dev[0]["build_id"]}
        doc["results"].append(res)
        print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
