#!/usr/bin/env python3
"""Times harmonics 0 .. 9 and the THD of 4 probes of the bench mesh (rc_mesh 100 x 100 with diodes, 1 024 Monte-Carlo instances, its
source at 100 MHz) over 2 periods of 64 steps (+ 2 steps past the window's end),
  fourier  with this tree's library: pe_hip_set_probes with capacity = 1, pe_hip_set_fourier, arm, transient, pe_hip_get_fourier;
  probes   with this tree's library and no Fourier analysis configured: capacity = steps + 1, arm, transient, pe_hip_get_probe_samples, and
           the same exact integral of the interpolant in numpy on the host -- what the same numbers cost without the feature;
  parent   the same as `probes` with the PARENT commit's library: what a probed transient cost before the recording launches had the branch,
alternating the three `--repeats` times (>= 3) in one invocation.  Profiler off; every measurement is a fresh child process (one library
per process) that loads the circuit, runs 8 warm-up steps, and then times with the host clock -- every call returns after a stream
synchronise.  `transient_seconds` is the pe_hip_analyze_tr call alone, `total_seconds` everything from arming to the coefficients on the
host.  No ratio is fixed in advance.

    python scripts/fourier_timing.py --parent-root <checkout of the parent commit with its libpe_hip.so built> [--out profiles/fourier_timing.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, math, sys, time
root, mode, batch = sys.argv[1], sys.argv[2], int(sys.argv[3])
sys.path.insert(0, root)
import numpy as np
import pe_load
pe = pe_load.load()
F = pe.ffi
W, H, NP, f0 = 100, 9, 2, 1e8
dt, n = 1.0 / f0 / 64, 2 * 64 + 2
rows = [0, W * W // 2 + W // 2, W * W - 1, W * W]
deck, r, c = pe.deck.rc_mesh_params(W, W, list(range(1, batch + 1)), True)
e = F.Engine(device=0)
e.set_options(g_min=0.0)
e.load_deck(deck, batch=batch, overrides={"R": r[:, :, None], "C": c[:, :, None]})
e.reset()
e.analyze_tr(dt, 8)
t_start = float(e.state()["t"][0])
t_end = t_start + NP / f0

def host_integral(t, v):
    """the exact integral of the interpolant over the clipped window, vectorised over instances, probes and harmonics"""
    k = np.arange(H + 1)[None, None, None, :]
    w = 2.0 * math.pi * f0 * k
    t0, t1 = t[:, :-1], t[:, 1:]
    ta, tb = np.clip(t0, t_start, t_end), np.clip(t1, t_start, t_end)
    ra, rb = ((ta - t0) / (t1 - t0))[:, :, None], ((tb - t0) / (t1 - t0))[:, :, None]
    va, vb = v[:, :-1] + (v[:, 1:] - v[:, :-1]) * ra, v[:, :-1] + (v[:, 1:] - v[:, :-1]) * rb
    h = (tb - ta)[:, :, None, None]
    tm = (0.5 * (ta + tb) - t_start)[:, :, None, None]
    phi = 0.5 * w * h
    with np.errstate(all="ignore"):
        A = np.where(phi != 0, np.sin(phi) / np.where(phi != 0, phi, 1), 1.0)
        q = phi * phi
        B = np.where(np.abs(phi) < 0.25, phi / 6 * (1 - q / 10 * (1 - q / 28 * (1 - q / 54 * (1 - q / 88)))), (np.sin(phi) - phi * np.cos(phi)) / np.where(phi != 0, 2 * q, 1))
    vm, d = 0.5 * (va + vb)[..., None], (vb - va)[..., None]
    z = h * (vm * A - 1j * d * B) * np.exp(-1j * w * tm)
    z = z.sum(1) * np.where(k[0] > 0, 2.0, 1.0) / (t_end - t_start)
    amp = np.abs(z)
    return z, np.sqrt((amp[..., 2:] ** 2).sum(-1)) / amp[..., 1]

t0 = time.perf_counter()
if mode == "fourier":
    e.set_probes(rows, 1, 1)
    e.set_fourier(f0, t_start, NP, H, [0, 1, 2, 3])
else:
    e.set_probes(rows, n + 1, 1)
e.arm_probes()
t1 = time.perf_counter()
st = e.analyze_tr(dt, n)
t2 = time.perf_counter()
if mode == "fourier":
    coef, thd, cov = e.fourier()
    amp1 = coef[:, :, 1, 2]
else:
    t, v, n_rec, n_drop = e.probe_samples()
    z, thd = host_integral(t, v)
    amp1 = np.abs(z[:, :, 1])
t3 = time.perf_counter()
assert np.all(np.isfinite(thd)) and np.all(amp1[:, 3] > 0.1)
print(json.dumps({"mode": mode, "batch": batch, "transient_seconds": t2 - t1, "total_seconds": t3 - t0, "read_back_seconds": t3 - t2, "gpu_ms": st["gpu_ms"],
                  "thd_instance0": [float(x) for x in thd[0]], "amp1_instance0": [float(x) for x in amp1[0]], "build_id": F.build_id()}))
'''


def child(root, mode, batch, timeout):
    env = dict(os.environ)
    env.pop("PE_HIP_LIB", None)  # each tree loads its own in-tree library
    r = subprocess.run([sys.executable, "-c", CHILD, root, mode, str(batch)], env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{mode} in {root}: exit {r.returncode}")  # nothing more is started on the GPU after a failure
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fourier_timing.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    runs = {"fourier": [], "probes": [], "parent": []}
    for _ in range(a.repeats):
        runs["parent"].append(child(os.path.abspath(a.parent_root), "parent", a.batch, a.timeout))
        runs["fourier"].append(child(ROOT, "fourier", a.batch, a.timeout))
        runs["probes"].append(child(ROOT, "probes", a.batch, a.timeout))
    med = {k: {q: statistics.median(x[q] for x in v) for q in ("transient_seconds", "total_seconds", "read_back_seconds", "gpu_ms")} for k, v in runs.items()}
    doc = {"workload": "rc_mesh_params(100, 100, seeds 1 .. %d, diodes), dt = 1 / (64 x 100 MHz), 130 steps after 8 warm-up steps, 4 probes, H = 9, 2 periods" % a.batch,
           "repeats": a.repeats,
           "median": med,
           "runs": {k: [{q: x[q] for q in ("transient_seconds", "total_seconds", "read_back_seconds", "gpu_ms")} for x in v] for k, v in runs.items()},
           "ratio_total_parent_over_fourier": med["parent"]["total_seconds"] / med["fourier"]["total_seconds"],
           "ratio_transient_fourier_over_probes": med["fourier"]["transient_seconds"] / med["probes"]["transient_seconds"],
           "ratio_transient_probes_over_parent": med["probes"]["transient_seconds"] / med["parent"]["transient_seconds"],
           "thd_instance0": {k: v[-1]["thd_instance0"] for k, v in runs.items()},
           "build_id": runs["fourier"][0]["build_id"], "parent_build_id": runs["parent"][0]["build_id"]}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
