"""Cost of the integration rules on the benchmark's workload: steps per second of the 100 x 100 diode mesh of bench.py (dt = 1e-10, per-instance
R and C) at 128 and 1 024 instances, 100 steps after 5 of warm-up, for
  - the trapezoidal rule on the PARENT commit (a tree of that commit with its library built, --parent-root),
  - the trapezoidal rule on this commit,
  - backward Euler and Gear-2 on this commit.
Each figure comes from a child process of its own (one library per process); the variants alternate over --rounds rounds so that what
else runs on the host hits them alike.  The time is that of HIP events around the launches of the call (run statistics, gpu_ms), and a
host clock around the call, which ends in a stream synchronise.  Writes profiles/integ_timing.json: every sample, the median per variant
and the ratios to the parent's median; the spread of a variant is (max - min) / median of its samples.

    python scripts/integ_timing.py --parent-root /path/to/parent/tree [--rounds 3] [--out profiles/integ_timing.json]
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = {"trap": 0, "be": 1, "gear2": 2}


def child(root, method, batch, steps, warmup):
    sys.path.insert(0, root)
    import pe_load
    pe = pe_load.load()
    seeds = list(range(1, batch + 1))
    deck, r, c = pe.deck.rc_mesh_params(100, 100, seeds, True)
    eng = pe.ffi.Engine(device=0)
    eng.set_options(g_min=0.0)
    if method != "trap":
        eng.set_tr_method(METHODS[method])
    eng.load_deck(deck, batch=batch, overrides={"R": r[:, :, None], "C": c[:, :, None]})
    eng.reset()
    eng.analyze_tr(1e-10, warmup)
    t0 = time.perf_counter()
    st = eng.analyze_tr(1e-10, steps)
    wall = time.perf_counter() - t0
    x = eng.solution()
    print("RESULT " + json.dumps({"gpu_ms": st["gpu_ms"], "wall_ms": wall * 1e3, "steps": st["steps"], "newton_iters": st["newton_iters"], "n_failed": st["n_failed"],
                                  "build_id": pe.ffi.build_id(), "x_abs_max": float(abs(x).max())}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None, help="tree of the parent commit with phy-engine_amd/libpe_hip.so built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integ_timing.json"))
    ap.add_argument("--child", nargs=3, metavar=("ROOT", "METHOD", "BATCH"), default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child[0], args.child[1], int(args.child[2]), args.steps, args.warmup)
        return
    variants = ([("parent_trap", args.parent_root, "trap")] if args.parent_root else []) + [("trap", ROOT, "trap"), ("be", ROOT, "be"), ("gear2", ROOT, "gear2")]
    out = {"workload": "rc_mesh 100 x 100, diodes, dt 1e-10, per-instance R and C", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "batches": {}}
    for batch in args.batches:
        samples = {name: [] for name, _, _ in variants}
        for _ in range(args.rounds):
            for name, root, method in variants:
                env = {k: v for k, v in os.environ.items() if k != "PE_HIP_LIB"}
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--child", root, method, str(batch)],
                                   env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise SystemExit(f"{name} at batch {batch} failed ({r.returncode}): {r.stdout[-2000:]} {r.stderr[-4000:]}")
                rec = json.loads(next(line for line in r.stdout.splitlines() if line.startswith("RESULT "))[7:])
                if rec["n_failed"] or rec["steps"] != batch * args.steps:
                    raise SystemExit(f"{name} at batch {batch}: {rec}")
                samples[name].append(rec)
        res = {}
        for name, recs in samples.items():
            rates = [batch * args.steps / (q["gpu_ms"] * 1e-3) for q in recs]
            walls = [batch * args.steps / (q["wall_ms"] * 1e-3) for q in recs]
            med = statistics.median(rates)
            res[name] = {"instance_steps_per_s": rates, "median": med, "spread": (max(rates) - min(rates)) / med, "median_wall": statistics.median(walls),
                         "newton_iters": recs[0]["newton_iters"], "build_id": recs[0]["build_id"]}
        base = res["parent_trap"]["median"] if "parent_trap" in res else res["trap"]["median"]
        for name in res:
            res[name]["ratio_to_" + ("parent_trap" if "parent_trap" in res else "trap")] = res[name]["median"] / base
        out["batches"][str(batch)] = res
        print(batch, {k: (round(v["median"]), round(v["spread"], 4)) for k, v in res.items()}, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
