"""Static fronts of the lane-group kernel skipped after the first Newton iteration of a solve point: the checks shared by
tests/test_static_skip_emu.py (host emulation) and tests/test_gpu_static_skip.py (MI355X).

Everything runs rc_mesh(56, 56, seed, True) -- 3 138 rows, the smallest mesh the policy puts on the split schedule with the lane-group
kernel -- under GEOMETRY_BATCH = 1024, g_min = 0, batch 5 with per-instance R / C (one full quad + one quad with three invalid lanes).
The skip changes which fronts a launch walks, never a value: every comparison against STATIC_SKIP = 0 is for bit identity."""
import ctypes as C

import numpy as np

from parity_common import pe
from front_shapes_common import KNOBS_MANY_CHILDREN  # (another tree: many small static fronts)

MESH, BATCH, DT, STEPS = 56, 5, 1e-10, 6
_CASE = {}


def case(nonlinear=True):
    """deck + per-instance overrides (computed once per process)"""
    if nonlinear not in _CASE:
        deck, r, c = pe.deck.rc_mesh_params(MESH, MESH, list(range(1, BATCH + 1)), nonlinear)
        _CASE[nonlinear] = (deck, {"R": r[:, :, None], "C": c[:, :, None]})
    return _CASE[nonlinear]


def vac(amps):
    return np.array([[[a, 2.0 * np.pi * 1e8, 0.0]] for a in amps])


def engine(skip, knobs=None, residual_tol=0.0, prepare=None, nonlinear=True, amps=None):
    e = pe.ffi.Engine(device=0)
    e.set_options(g_min=0.0, residual_tol=residual_tol)
    e.set_knob("GEOMETRY_BATCH", 1024)
    e.set_knob("STATIC_SKIP", skip)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    if prepare:
        prepare(e)
    deck, ov = case(nonlinear)
    if amps is not None:
        ov = dict(ov, VAC=vac(amps))
    e.load_deck(deck, batch=BATCH, overrides=ov)
    e.reset()
    return e


def outcome(e):
    """everything that must not depend on the skip"""
    st = e.state()
    return {"x": e.solution(), "trace": e.newton_trace().tolist(), "iters": st["iters"].tolist(), "status": st["status"].tolist(),
            "stats": e.sweep_statistics()}


def same(a, b, what):
    assert a["trace"] == b["trace"] and a["iters"] == b["iters"] and a["status"] == b["status"], f"{what}: Newton counts differ: {a['trace']} {a['iters']} / {b['trace']} {b['iters']}"
    assert np.array_equal(a["x"], b["x"]), f"{what}: solutions differ by {float(np.max(np.abs(a['x'] - b['x'])))!r}"
    assert np.array_equal(a["stats"], b["stats"]), f"{what}: sweep statistics differ"


def run_pair(what, steps=STEPS, **kw):
    """the same run with STATIC_SKIP = 1 and 0 -> (outcome, skip statistics) of each; the outcomes are compared here"""
    res = []
    for skip in (1, 0):
        e = engine(skip, **kw)
        try:
            rc = e.analyze_tr(DT, steps, check=False)["rc"]
            res.append((dict(outcome(e), rc=rc), e.static_skip_stats(), e.safety_net()))
        finally:
            e.close()
    same(res[0][0], res[1][0], what)
    assert res[0][0]["rc"] == res[1][0]["rc"], what
    assert res[1][1]["skipped_launches"] == 0, f"{what}: STATIC_SKIP = 0 skipped: {res[1][1]}"
    return res


def check_bit_identity(knobs=None, what="bit identity"):
    """1. six transient steps: solutions, Newton counts and sweep statistics bit-identical; the first run did skip"""
    on, off = run_pair(what, knobs=knobs)
    assert on[0]["rc"] == 0 and all(s == 0 for s in on[0]["status"]), on[0]["status"]
    assert max(on[0]["trace"]) >= 2, on[0]["trace"]
    assert on[1]["skipped_launches"] > 0, on[1]
    # every point of the run: one full launch, then skipped ones (no refinement here)
    assert on[2]["refined"] == 0 and on[1]["full_launches"] == STEPS and on[1]["skipped_launches"] + on[1]["full_launches"] == off[1]["full_launches"], (on[1], off[1])


def front_classes(e):
    t, s = e.front_table(), e.static_fronts()
    par, quad = t["parent"], t["quad"]
    has = par >= 0
    ps, pq = np.where(has, s[np.maximum(par, 0)], 0), np.where(has, quad[np.maximum(par, 0)], 0)
    return {"static root under a dynamic quad parent": int(np.sum((s == 1) & has & (ps == 0) & (pq == 1))),
            "static root under a non-quad parent": int(np.sum((s == 1) & has & (ps == 0) & (pq == 0))),
            "static front inside a static subtree": int(np.sum((s == 1) & has & (ps == 1))),
            "dynamic front with a static parent": int(np.sum((s == 0) & has & (ps == 1))),
            "static quad fronts": int(np.sum((s == 1) & (quad == 1))), "static fronts outside the lane-group kernel": int(np.sum((s == 1) & (quad == 0)))}


def check_classification():
    """2. the deck reaches every case of the classification that can go wrong (checked on the CPU: the 56 x 56 mesh has all three as it is)"""
    e = engine(1)
    try:
        e.analyze_tr(DT, 1)
        got = front_classes(e)
    finally:
        e.close()
    for k in ("static root under a dynamic quad parent", "static root under a non-quad parent", "static front inside a static subtree"):
        assert got[k] > 0, f"the deck no longer has a {k}: {got}"
    assert got["dynamic front with a static parent"] == 0, got
    # (a static front outside the lane-group kernel would be factored again in every iteration above skipped static quad children, from their
    #  persistent slots: this deck has none -- the static roots under non-quad parents above cover that hand-over with a dynamic parent)
    assert got["static fronts outside the lane-group kernel"] == 0, got
    return got


def check_leaving():
    """3. one instance driven harder than its quad mates needs more iterations: the others leave the quad mid-point"""
    amps = [2.0, 2.0, 40.0, 2.0, 2.0]
    on, off = run_pair("instances leaving mid-point", amps=amps)
    assert on[0]["rc"] == 0 and on[1]["skipped_launches"] > 0, on[1]
    it = on[0]["iters"]
    assert it[2] > max(it[:2] + it[3:]), f"instance 2 was meant to need more iterations than the others: {it}"


REFINE_TOL = 2e-18  # below the backward error of most plain solves of this deck (1e-18 .. 1e-17), within reach of a refinement round


def check_refinement(residual_tol=REFINE_TOL):
    """4. a residual_tol so small that the iterates about to be accepted owe a refinement round: bit-identical step by step -- solutions,
    statuses (some solves end as INACCURATE and are re-matched: part of the path), Newton counts, refinement counters.  Instance 2 is driven
    hard and iterates on after its quad mates were accepted (and refined) in the same point: a refinement round refactors with the residual
    riding along, so a later launch of that point that skipped the static fronts would assemble residual-based update vectors and kept
    pivots into the real right-hand side.  The engine counts the iteration launches issued after a refinement round of their own point
    (whatever the knob says) and those of them that skipped: the first must be positive and equal in both runs -- the test reaches the rule --,
    the second zero."""
    amps = [2.0, 2.0, 40.0, 2.0, 2.0]
    runs = []
    for skip in (1, 0):
        e = engine(skip, residual_tol=residual_tol, amps=amps)
        try:
            steps, it0, sk0, net0 = [], np.zeros(BATCH, dtype=np.int64), e.static_skip_stats(), e.safety_net()
            for _ in range(STEPS):
                rc = e.analyze_tr(DT, 1, check=False)["rc"]
                it, sk, net, status = e.state()["iters"], e.static_skip_stats(), e.safety_net(), e.state()["status"].tolist()
                steps.append({"rc": rc, "x": e.solution(), "iters": (it - it0).tolist(), "status": status, "skipped": sk["skipped_launches"] - sk0["skipped_launches"],
                              "full": sk["full_launches"] - sk0["full_launches"], "after": sk["launches_after_refinement"] - sk0["launches_after_refinement"],
                              "skipped_after": sk["skipped_after_refinement"] - sk0["skipped_after_refinement"], "refined": net["refined"] - net0["refined"], "rematched": net["rematched"] - net0["rematched"]})
                it0, sk0, net0 = it, sk, net
            runs.append((steps, outcome(e)))
        finally:
            e.close()
    for k, a in enumerate(runs[0][0]):
        print(f"refinement, step {k}: " + ", ".join(f"{n} {a[n]}" for n in ("rc", "iters", "status", "skipped", "full", "after", "skipped_after", "refined", "rematched")))
    same(runs[0][1], runs[1][1], "refinement")
    for k, (a, b) in enumerate(zip(runs[0][0], runs[1][0])):
        for n in ("rc", "iters", "status", "refined", "rematched", "after"):
            assert a[n] == b[n], f"refinement, step {k}: {n} {a[n]} / {b[n]}"
        assert np.array_equal(a["x"], b["x"]), f"refinement, step {k}: solutions differ"
        assert b["skipped"] == 0 and a["skipped"] + a["full"] == b["full"], (k, a["skipped"], a["full"], b["full"])
        assert a["skipped_after"] == 0 and b["skipped_after"] == 0, f"refinement, step {k}: {a['skipped_after']} launches after a refinement of their point skipped the static fronts"
        assert a["after"] == 0 or a["refined"] + a["rematched"] > 0, (k, a["after"], a["refined"], a["rematched"])
    assert sum(a["refined"] + a["rematched"] for a in runs[0][0]) > 0, f"no refinement happened under residual_tol {residual_tol!r}"
    assert sum(a["skipped"] for a in runs[0][0]) > 0, "nothing was skipped"
    assert sum(a["after"] for a in runs[0][0]) > 0, "no iteration launch followed a refinement round of its own point: the rule was not reached"
    it = [sum(a["iters"][b] for a in runs[0][0]) for b in range(BATCH)]
    assert any(max(a["iters"]) > min(a["iters"]) for a in runs[0][0]), f"no step in which one instance iterated on after another was accepted: {it}"


def check_linear():
    """5a. a linear deck: no x-dependent entry anywhere, nothing is classified, nothing skipped"""
    on, off = run_pair("linear deck", nonlinear=False, steps=2)
    assert on[0]["rc"] == 0 and on[1]["skipped_launches"] == 0, on[1]


_KEEP = []


def _overlay(e):
    FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))

    def hook(user, event, mode, t, dt, x, a, b):
        if event == 1:  # PE_HIP_OVERLAY_ITERATE: a conductance to ground at node 1 that follows the iterate
            a[0] = 1e-3 * (1.0 + 0.1 * np.tanh(x[0]))
            b[0] = 0.0
        return 0
    cb = FN(hook)
    _KEEP.append(cb)
    lib = pe.ffi.lib()
    lib.pe_hip_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_int, FN, C.c_void_p]
    one, rep = np.array([0], dtype=np.int32), np.array([1e-3])
    ip, dp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double)))
    assert lib.pe_hip_set_overlay(e._h, 1, ip(one), ip(one), dp(rep), 1, ip(one), 1, cb, None) == 0


def check_overlay():
    """5b. a host-stamp overlay may write anywhere in A in every iteration: never skipped"""
    on, off = run_pair("host-stamp overlay", prepare=_overlay, steps=2)
    assert on[0]["rc"] == 0 and on[1]["skipped_launches"] == 0 and on[1]["full_launches"] > 2, on[1]


def check_full_stamp():
    """5c. PHY_ENGINE_HIP_FULL_STAMP=1 (read once per process: the caller sets it before the first solve): every iteration stamps everything"""
    import os
    assert os.environ.get("PHY_ENGINE_HIP_FULL_STAMP") == "1"
    on, off = run_pair("full stamp", steps=2)
    assert on[0]["rc"] == 0 and on[1]["skipped_launches"] == 0, on[1]
