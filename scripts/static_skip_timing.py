#!/usr/bin/env python3
"""Times the flagship benchmark of this tree against the parent commit's on one box (protocol of scripts/tr_adaptive_timing.py): every
measurement is a fresh process running the plain `bench.py --gpus 1 --steps 20 --warmup 5` of its tree, parent and child alternating
`--repeats` times (>= 3), profiler off.

    python scripts/static_skip_timing.py --parent-root <built checkout of the parent commit> [--out profiles/static_skip_timing.json]

Writes one JSON document: `value` (instance-steps/s), ms per step, the dominant pair's average launch and the Newton iterations per step of
every run, the gain of the child in every alternation, its median gain, the spread of the parent's own repeats, and the two acceptance
conditions: the child ahead in every alternation, and a median gain above twice the parent's spread."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = ["--gpus", "1", "--steps", "20", "--warmup", "5"]


def bench(root, timeout):
    env = dict(os.environ)
    env.pop("PE_HIP_LIB", None)  # each tree loads its own in-tree library
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + BENCH, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench.py of {root}: exit {r.returncode}")  # nothing more is started on the GPU after a failure
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return {"value": line["value"], "ms_per_step": line["ms_per_step"], "newton_iters_per_step": line["newton_iters_per_step"],
            "pair_avg_launch_ms": line["roofline"]["avg_launch_ms"], "stats_checksum": line["stats_checksum"], "build_id": line["build_id"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=280, help="seconds per measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "static_skip_timing.json"))
    a = ap.parse_args()
    if a.repeats < 3:
        raise SystemExit("--repeats must be at least 3")
    parent, child = [], []
    for k in range(a.repeats):
        parent.append(bench(os.path.abspath(a.parent_root), a.timeout))
        child.append(bench(ROOT, a.timeout))
        print(json.dumps({"alternation": k, "parent": parent[-1]["value"], "child": child[-1]["value"]}), flush=True)
    vp, vc = [x["value"] for x in parent], [x["value"] for x in child]
    gains = [c / p - 1.0 for p, c in zip(vp, vc)]
    spread = (max(vp) - min(vp)) / statistics.median(vp)
    doc = {"command": "bench.py " + " ".join(BENCH), "repeats": a.repeats, "parent": parent, "child": child,
           "parent_median": statistics.median(vp), "child_median": statistics.median(vc), "gain_per_alternation": gains,
           "median_gain": statistics.median(gains), "parent_spread": spread,
           "same_results": all(x["stats_checksum"] == parent[0]["stats_checksum"] and x["newton_iters_per_step"] == parent[0]["newton_iters_per_step"] for x in parent + child),
           "child_ahead_in_every_alternation": all(g > 0.0 for g in gains), "median_gain_above_twice_the_parent_spread": statistics.median(gains) > 2.0 * spread}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in doc.items() if k not in ("parent", "child")}))


if __name__ == "__main__":
    main()
