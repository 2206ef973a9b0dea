"""Variable-step transient (pe_hip_analyze_tr_adaptive / pe_hip_get_tr_step_log, include/pe_hip.h) on the CPU: the controller and the
team-generic device text (pe_lte.hpp) through the host emulation library (tests/emu: test infrastructure), one child process per case.

The accuracy cases compare against references that are not the code under test: 1 - exp(-t / tau) for the RC step, and fine-step runs of
the reference binary (tests/golden/bridge_fine_tr, pulse_rc_fine_tr: every 100th step).  The goldens are sparse, so the variable-step
solution is evaluated AT the golden's sample times by `at_times` (PRE): a cubic through the four nearest accepted points that lie between
the same two source corners (x' jumps at a corner; a cubic across one rings), fewer points where a segment is short.  The trapezoidal
solution is second-order accurate and its accepted points are spaced by the controller so that h^3 x''' stays below the tolerance; the
cubic's own error, of order h^4 x'''' / 24, is below that again.  Bounds: twice the error and twice the number of attempted steps that a
host-side sketch of the same rule measured (RC 36 + 2 steps, 8.2e-4; bridge 507 + 174, 3.8e-4; pulse-RC 262 + 26, 4.3e-3)."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")
SCHEDULES = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS = ["resident", "split", "split_graph"]


@pytest.fixture(scope="module")
def emu():
    make("-C", os.path.join(ROOT, "tests", "emu"))
    return EMU


# shared by every child, and by tests/test_gpu_tr_adaptive.py (which runs the same bodies on the real library)
PRE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import ctypes as C
import numpy as np
import pe_load
pe = pe_load.load()
F, D = pe.ffi, pe.deck
from parity_common import golden
EPS4 = 4 * np.finfo(float).eps
TOL = dict(lte_reltol=1e-4, lte_abstol_v=1e-6, lte_abstol_i=1e-6, trtol=7.0)

def engine(deck, batch=1, ov=None, gmin=0.0, knobs=None, **opt):
    e = F.Engine()
    e.set_options(g_min=gmin, **opt)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, ov)
    e.reset()
    return e

def mesh5():
    deck, r, c = D.rc_mesh_params(6, 6, list(range(1, 6)), True)
    return deck, {"R": r[:, :, None], "C": c[:, :, None]}

def samples(e):
    """accepted points of the armed window: t [n], x [n][B][rows] (sample 0 = the point the window was armed at)"""
    t, v, n, drop = e.probe_samples()
    assert len(set(n.tolist())) == 1 and not drop.any(), (n, drop)
    assert np.array_equal(t[:, :n[0]], np.repeat(t[:1, :n[0]], len(t), 0)), "one step sequence for the whole batch"
    return t[0, :n[0]].copy(), np.transpose(v[:, :n[0]], (1, 0, 2)).copy()

def q_of(tt, xx, h, n_nodes, lte_reltol, lte_abstol_v, lte_abstol_i, trtol):
    """per-instance q of the candidate xx[3] at tt[3] against the three points before it (the formulas of include/pe_hip.h, in the
    operation order of pe_lte.hpp); xx [4][B][rows]"""
    d10, d21, dn2 = (xx[1] - xx[0]) / (tt[1] - tt[0]), (xx[2] - xx[1]) / (tt[2] - tt[1]), (xx[3] - xx[2]) / (tt[3] - tt[2])
    e0, e1 = (d21 - d10) / (tt[2] - tt[0]), (dn2 - d21) / (tt[3] - tt[1])
    dd3 = (e1 - e0) / (tt[3] - tt[0])
    abstol = np.where(np.arange(xx.shape[2]) < n_nodes, lte_abstol_v, lte_abstol_i)
    tol = trtol * (lte_reltol * np.maximum(np.abs(xx[3]), np.abs(xx[2])) + abstol)
    return np.max(0.5 * h * h * h * np.abs(dd3) / tol, axis=1)

def check_decisions(e, st, t, x, n_nodes, t0, t_stop, dt_init, dt_min, dt_max, tol, bps=(), n_pts=0):
    """every entry of the step log against the rule of include/pe_hip.h, from the recorded accepted points alone; returns the number of
    accepted steps whose q was recomputed"""
    dt, oc = e.tr_step_log()
    assert st["n_accepted"] + st["n_rejected_lte"] + st["n_rejected_newton"] == len(dt) == len(oc)
    assert (oc == 0).sum() == st["n_accepted"] == len(t) - 1 and (oc == 1).sum() == st["n_rejected_lte"] and (oc == 2).sum() == st["n_rejected_newton"]
    assert np.all(np.diff(t) > 0), "sample times strictly increase"
    bps = sorted([b for b in bps if t0 < b < t_stop]) + [t_stop]
    reached = lambda at, bp: at >= bp or abs(at - bp) <= EPS4 * abs(bp)
    now, a, expect, tested, hit = t0, 0, dt_init, 0, set()
    for k in range(len(dt)):
        bp = next(b for b in bps if not reached(now, b))
        h = dt[k]
        lands = h == bp - now
        assert h <= dt_max * (1 + 1e-12) and (h >= dt_min or lands), (k, h)
        if expect is not None:
            want = min(max(expect, dt_min), dt_max, bp - now)
            assert abs(h - want) <= 1e-9 * want, (k, h, want)
        else:
            assert 0.1 * prev_h * (1 - 1e-9) <= h <= max(0.9 * prev_h, dt_min) * (1 + 1e-9) or lands, (k, h, prev_h)   # an LTE rejection: q > 1 unknown
        if oc[k] == 2:
            expect = h / 8
        elif oc[k] == 1:
            assert n_pts >= 3 and h > dt_min
            expect, prev_h = None, h
        else:
            assert t[a + 1] == now + h, "the new time is t + h as the step forms it"
            q = None
            if n_pts >= 3 and tol["lte_reltol"] > 0:
                qs = q_of(t[a - 2:a + 2], x[a - 2:a + 2], h, n_nodes, **tol)
                q = float(np.max(qs))
                assert q <= 1 + 1e-9 or h <= dt_min, (k, q, h)
                tested += 1
            now, a = t[a + 1], a + 1
            at_bp = bp != t_stop and reached(now, bp)
            if reached(now, bp):
                hit.add(bp)
            n_pts = 1 if at_bp else min(n_pts + 1, 4)
            expect = dt_init if at_bp else (h if q is None else h * (min(2.0, 0.9 * q ** (-1.0 / 3.0)) if q > 0 else 2.0))
    if reached(now, t_stop):
        assert set(bps) == hit, "every breakpoint and t_stop is hit within 4 eps"
    assert st["t_end"] == now
    return tested

def replay(make_engine, dt, oc):
    """today's calls only: checkpoint, analyze_tr(dt_k, 1), restore where the log says rejected -> accepted t [n], x [n][B][rows], engine"""
    e = make_engine()
    ts, xs = [e.state()["t"][0]], [e.solution()]
    for h, o in zip(dt, oc):
        ck = e.checkpoint()
        e.analyze_tr(h, 1, check=False)
        if o:
            e.restore(ck)
        else:
            assert not e.state()["status"].any()
            ts.append(e.state()["t"][0]); xs.append(e.solution())
    return np.array(ts), np.array(xs), e

def at_times(t, v, tq, corners=()):
    """v(tq) from the accepted points (t, v): cubic through the four nearest points of the same corner-free segment (see the module's
    docstring); a query on a corner belongs to the segment that ends there (x is continuous across a corner)"""
    cs = np.array(sorted(corners), dtype=float)
    out = np.empty(len(tq))
    for i, x in enumerate(tq):
        s = int(np.searchsorted(cs, x, side="left"))
        lo_t = cs[s - 1] if s > 0 else -np.inf
        hi_t = cs[s] if s < len(cs) else np.inf
        idx = np.where((t >= (lo_t if np.isinf(lo_t) else lo_t - EPS4 * abs(lo_t))) & (t <= (hi_t if np.isinf(hi_t) else hi_t + EPS4 * abs(hi_t))))[0]
        k = int(np.searchsorted(t[idx], x))
        sel = idx[max(0, min(len(idx) - 4, k - 2)):][:4]
        tt, vv = t[sel], v[sel]
        acc = 0.0
        for a in range(len(sel)):
            w = 1.0
            for b in range(len(sel)):
                if a != b:
                    w *= (x - tt[b]) / (tt[a] - tt[b])
            acc += w * vv[a]
        out[i] = acc
    return out
''' % (ROOT, ROOT)


def run(lib, body, **env):
    e = dict(os.environ, PE_HIP_LIB=lib, **env)
    r = subprocess.run([sys.executable, "-c", PRE + body], env=e, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    return r.stdout


# ---- 1. a pinned controller is the fixed step, bit for bit
PINNED = r'''
knobs = %r
meta, _, tt_deck = golden("pn_tt_tr")
m5, ov5 = mesh5()
MEAS = [("min", 0), ("max", 1), ("avg", 1), ("rms", 0), ("integ", 1), ("cross", 0, 0.5, 0, 1)]
for name, deck, batch, ov, gmin, dt0, n in (("rc_step", D.rc_step(), 1, None, 0.0, 1e-8, 25), ("pn_tt_tr", tt_deck, 1, None, 0.0, 1e-8, 6),
                                            ("bridge", D.bridge_rectifier(), 1, None, 1e-12, 1e-5, 60), ("mesh5", m5, 5, ov5, 0.0, 2e-10, 12)):
    res = []
    for adaptive in (False, True):
        e = engine(deck, batch, ov, gmin, knobs)
        e.set_probes(list(range(deck.rows))[:8], n + 1, 1, MEAS)
        e.arm_probes()
        if adaptive:
            st = e.analyze_tr_adaptive(1.0, dt0, dt_min=dt0, dt_max=dt0, lte_reltol=-1.0, max_steps=n)
            assert st["n_accepted"] == n and st["n_rejected_lte"] == st["n_rejected_newton"] == 0 and st["t_end"] < 1.0, (name, st)
            dt, oc = e.tr_step_log()
            assert np.all(dt == dt0) and not oc.any() and len(dt) == n
            run_stats = st["run"]
        else:
            run_stats = e.analyze_tr(dt0, n)
        s = e.state()
        res.append((e.solution(), s["t"], s["steps"], s["iters"], s["status"], e.newton_trace(), *e.probe_samples(), e.measures(),
                    np.array([run_stats["steps"], run_stats["newton_iters"], run_stats["n_failed"]])))
        e.close()
    for k, (a, b) in enumerate(zip(*res)):
        assert np.array_equal(a, b, equal_nan=True), (name, k, a, b)
print("ok")
'''


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_pinned_controller_equals_fixed_step_bitwise(emu, knobs):
    assert "ok" in run(emu, PINNED % knobs)


# ---- 2. + 3. + 6. replay with today's calls, and the decisions recomputed from the samples
REPLAY_BRIDGE = r'''
knobs = %r
deck = D.bridge_rectifier()
mk = lambda: engine(deck, 1, None, 1e-12, knobs, max_newton=5)
e = mk()
e.set_probes(list(range(deck.rows)), 4096, 1)
e.arm_probes()
st = e.analyze_tr_adaptive(0.04, 1e-4)
assert st["rc"] == 0 and st["n_rejected_lte"] > 0 and st["n_rejected_newton"] > 0, st
assert st["newton_iters_rejected"] > 0 and st["run"]["steps"] == st["n_accepted"] and st["dt_smallest"] < 1e-4 <= st["dt_largest"]
t, x = samples(e)
dt, oc = e.tr_step_log()
assert len(e.newton_trace()) == st["n_accepted"], "the Newton trace holds accepted steps only"
assert dt.min() == st["dt_smallest"] and dt.max() == st["dt_largest"]
tested = check_decisions(e, st, t, x, deck.n_nodes, 0.0, 0.04, 1e-4, 1e-13, 0.04 / 50, dict(lte_reltol=1e-3, lte_abstol_v=1e-6, lte_abstol_i=1e-9, trtol=7.0))
assert tested > 100, tested
tr, xr, f = replay(mk, dt, oc)
assert np.array_equal(tr, t) and np.array_equal(xr, x), "a rejected step leaves nothing behind: every accepted point is reproduced bit for bit"
sa, sb = e.state(), f.state()
assert np.array_equal(e.solution(), f.solution()) and all(np.array_equal(sa[k], sb[k]) for k in sa), (sa, sb)
# the states are the same state: both continue identically
e.analyze_tr(1e-5, 5); f.analyze_tr(1e-5, 5)
assert np.array_equal(e.solution(), f.solution())
print("ok", st["n_accepted"], st["n_rejected_lte"], st["n_rejected_newton"])
'''


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_replay_with_fixed_step_calls_reproduces_every_accepted_point(emu, knobs):
    assert "ok" in run(emu, REPLAY_BRIDGE % knobs)


BATCH = r'''
knobs = %r
deck, ov = mesh5()
mk = lambda: engine(deck, 5, ov, 0.0, knobs)
e = mk()
e.set_probes(list(range(deck.rows)), 4096, 1)
e.arm_probes()
T = 4e-8
st = e.analyze_tr_adaptive(T, 2e-11, lte_reltol=1e-4)
assert st["rc"] == 0 and st["run"]["steps"] == 5 * st["n_accepted"], st
t, x = samples(e)
tol = dict(lte_reltol=1e-4, lte_abstol_v=1e-6, lte_abstol_i=1e-9, trtol=7.0)
tested = check_decisions(e, st, t, x, deck.n_nodes, 0.0, T, 2e-11, 2e-20, T / 50, tol)   # (the batch's q = the worst instance's: it gives the next dt)
assert tested > 20, tested
# every instance meets the tolerance on every tested step, and they differ (the worst one decided)
worst = set()
for a in range(3, len(t) - 1):
    qs = q_of(t[a - 2:a + 2], x[a - 2:a + 2], t[a + 1] - t[a], deck.n_nodes, **tol)
    assert np.all(qs <= 1 + 1e-9), (a, qs)
    worst.add(int(np.argmax(qs)))
dt, oc = e.tr_step_log()
tr, xr, f = replay(mk, dt, oc)
assert np.array_equal(tr, t) and np.array_equal(xr, x) and np.array_equal(e.solution(), f.solution())
sa, sb = e.state(), f.state()
assert all(np.array_equal(sa[k], sb[k]) for k in sa)
print("ok", st["n_accepted"], st["n_rejected_lte"], sorted(worst))
'''


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_batch_has_one_sequence_decided_by_the_worst_instance(emu, knobs):
    assert "ok" in run(emu, BATCH % knobs)


# ---- 4. accuracy and economy against references that are not the code under test
ACCURACY = r'''
knobs = %r
# (a) RC step against 1 - exp(-t / tau)
deck, tau = D.rc_step(), 1e-6
e = engine(deck, knobs=knobs)
e.set_probes(list(range(deck.rows)), 4096, 1); e.arm_probes()
st = e.analyze_tr_adaptive(10 * tau, tau / 1000, dt_max=tau, **TOL)
t, x = samples(e)
err = float(np.max(np.abs(x[:, 0, 1] - (1 - np.exp(-t / tau)))))
n_att = len(e.tr_step_log()[0])
print("rc_step: attempted", n_att, "max error", err)
assert st["t_end"] == t[-1] and abs(t[-1] - 10 * tau) <= EPS4 * 10 * tau
assert err <= 2 * 8.2e-4 and n_att <= 2 * (36 + 2), (err, n_att)
check_decisions(e, st, t, x, deck.n_nodes, 0.0, 10 * tau, tau / 1000, tau / 1000 * 1e-9, tau, TOL)
e.close()
# (b) bridge rectifier against the reference's dt = 1e-6 run
meta, gx, deck = golden("bridge_fine_tr")
tg = np.array(meta["snap_steps"]) * meta["dt"]
e = engine(deck, gmin=1e-12, knobs=knobs)
e.set_probes(list(range(deck.rows)), 8192, 1); e.arm_probes()
st = e.analyze_tr_adaptive(0.04, 1e-6, dt_max=0.04 / 50, **TOL)
t, x = samples(e)
err = float(np.max(np.abs(at_times(t, x[:, 0, 2], tg) - gx[:, 2])))
n_att = len(e.tr_step_log()[0])
print("bridge: attempted", n_att, "max error of v(3)", err)
assert err <= 2 * 3.8e-4 and n_att <= 2 * (507 + 174) < 4000, (err, n_att)
check_decisions(e, st, t, x, deck.n_nodes, 0.0, 0.04, 1e-6, 1e-15, 0.04 / 50, TOL)
e.close()
# (c) pulse -> RC against the reference's dt = 1e-7 run, the generator's corners as breakpoints
meta, gx, deck = golden("pulse_rc_fine_tr")
tg = np.array(meta["snap_steps"]) * meta["dt"]
corners = [k * 1e-3 + c for k in range(3) for c in (0.0, 1e-6, 0.5e-3 - 1e-6, 0.5e-3)]
e = engine(deck, gmin=1e-12, knobs=knobs)
e.set_probes(list(range(deck.rows)), 8192, 1); e.arm_probes()
st = e.analyze_tr_adaptive(2e-3, 1e-7, dt_max=2e-3 / 20, source_breakpoints=True, **TOL)
t, x = samples(e)
err = float(np.max(np.abs(at_times(t, x[:, 0, 1], tg, corners) - gx[:, 1])))
n_att = len(e.tr_step_log()[0])
print("pulse_rc: attempted", n_att, "max error of v(2)", err)
assert err <= 2 * 4.3e-3 and n_att <= 2 * (262 + 26), (err, n_att)
check_decisions(e, st, t, x, deck.n_nodes, 0.0, 2e-3, 1e-7, 1e-16, 2e-3 / 20, TOL, bps=corners)
# explicit breakpoints, any order, give the same sequence as the generator's own corners
f = engine(deck, gmin=1e-12, knobs=knobs)
st2 = f.analyze_tr_adaptive(2e-3, 1e-7, dt_max=2e-3 / 20, breakpoints=corners[::-1] + [5.0, -1.0], **TOL)
assert np.allclose(f.tr_step_log()[0], e.tr_step_log()[0], rtol=1e-6) and np.allclose(f.solution(), e.solution(), rtol=1e-6, atol=1e-9)
print("ok")
'''


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_accuracy_and_economy_against_analytic_and_reference_runs(emu, knobs):
    out = run(emu, ACCURACY % knobs)
    print(out)
    assert "ok" in out


# ---- 5. step cutting rescues a run that the fixed step loses
RESCUE = r'''
knobs = %r
deck = D.bridge_rectifier()
e = engine(deck, gmin=1e-12, knobs=knobs, max_newton=5)
r = e.analyze_tr(1e-4, 400, check=False)
assert r["rc"] == F.ERR_NO_CONVERGENCE and e.state()["steps"][0] == 4, (r, e.state())
e.close()
e = engine(deck, gmin=1e-12, knobs=knobs, max_newton=5)
st = e.analyze_tr_adaptive(0.04, 1e-4, dt_max=1e-4, check=False)
assert st["rc"] == 0 and st["n_rejected_newton"] > 0 and abs(st["t_end"] - 0.04) <= EPS4 * 0.04 and e.state()["t"][0] == st["t_end"], st
assert not e.state()["status"].any()
e.close()
e = engine(deck, gmin=1e-12, knobs=knobs, max_newton=5)
x0 = None
st = e.analyze_tr_adaptive(0.04, 1e-4, dt_min=1e-4, dt_max=1e-4, check=False)
s = e.state()
assert st["rc"] == F.ERR_NO_CONVERGENCE and s["status"][0] == F.ERR_NO_CONVERGENCE and s["steps"][0] == 4 and st["n_accepted"] == 4, (st, s)
assert s["t"][0] == st["t_end"] and abs(s["t"][0] - 4e-4) < 1e-12, "t rolled back to the last accepted point"
# ... and that point is the state the four accepted steps left: the failed step was rolled back completely
f = engine(deck, gmin=1e-12, knobs=knobs, max_newton=5)
f.analyze_tr(1e-4, 4)
assert np.array_equal(f.solution(), e.solution()) and np.array_equal(f.state()["iters"], s["iters"])
f.analyze_tr(1e-5, 3); e.analyze_tr(1e-5, 3)
assert np.array_equal(f.solution(), e.solution())
print("ok")
'''


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_step_cutting_rescues_a_failing_run(emu, knobs):
    assert "ok" in run(emu, RESCUE % knobs)


# ---- 7. window rules and arguments
RULES = r'''
knobs = %r
deck = D.bridge_rectifier()
lib = F.lib()
def first_dts(e, t_stop):
    st = e.analyze_tr_adaptive(t_stop, 1e-6, max_steps=6)
    return e.tr_step_log()[0], st
# an empty history: the first three steps are untested, the step stays dt_init until the fourth has been judged
for prepare in ("fresh", "analyze_dc", "reset", "set_solution", "checkpoint_load", "analyze_tr", "set_time"):
    e = engine(deck, gmin=1e-12, knobs=knobs)
    t0 = 0.0
    if prepare != "fresh":
        e.analyze_tr_adaptive(2e-4, 1e-6)                      # fills the history
        if prepare == "analyze_dc": e.analyze_dc(F.MODE_TROP)
        elif prepare == "reset": e.reset()
        elif prepare == "set_solution": e.set_solution(e.solution())
        elif prepare == "checkpoint_load": e.restore(e.checkpoint())
        elif prepare == "analyze_tr": e.analyze_tr(1e-6, 1)
        else: assert lib.pe_hip_set_time(e._h, C.c_double(2e-4), C.c_double(1e-6)) == 0
        t0 = e.state()["t"][0]
    dt, st = first_dts(e, t0 + 1e-2)
    assert np.all(dt[:4] == 1e-6) and dt[4] != 1e-6 and st["n_accepted"] == 6, (prepare, dt)
    e.close()
# a second adaptive call continues the history of the first: its first step is tested and the step moves at once
e = engine(deck, gmin=1e-12, knobs=knobs)
e.analyze_tr_adaptive(2e-4, 1e-6)
dt, st = first_dts(e, 1e-2)
assert dt[0] == 1e-6 and dt[1] != 1e-6, dt
e.close()
# probes armed before the call record accepted steps only
e = engine(deck, gmin=1e-12, knobs=knobs, max_newton=5)
e.set_probes([2], 50, 3)
e.arm_probes()
st = e.analyze_tr_adaptive(0.04, 1e-4)
t, v, n, drop = e.probe_samples()
assert st["n_rejected_lte"] + st["n_rejected_newton"] > 0 and st["n_accepted"] // 3 + 1 > 50
assert n[0] == 50 and drop[0] == st["n_accepted"] // 3 + 1 - 50, (n, drop, st)
e.close()
e = engine(deck, gmin=1e-12, knobs=knobs, max_newton=5)
e.set_probes([2], 4096, 3)
e.arm_probes()
st = e.analyze_tr_adaptive(0.04, 1e-4)
assert e.probe_samples()[2][0] == st["n_accepted"] // 3 + 1
# refusals leave the engine as it was and usable
ref = (e.solution(), e.state()["t"].copy(), e.tr_step_log()[0])
good = dict(t_stop=0.05, dt_init=1e-5)
nan, inf = float("nan"), float("inf")
for bad in (dict(dt_init=0.0), dict(dt_init=-1e-6), dict(dt_min=1e-3, dt_max=1e-4), dict(dt_min=1e-3), dict(t_stop=0.04), dict(t_stop=0.01), dict(t_stop=nan),
            dict(t_stop=inf), dict(dt_init=nan), dict(dt_max=inf), dict(lte_reltol=nan), dict(trtol=inf), dict(lte_abstol_v=nan), dict(lte_abstol_i=nan),
            dict(breakpoints=[0.045, nan])):
    a = dict(good, **bad)
    try:
        e.analyze_tr_adaptive(**a); raise AssertionError(f"accepted: {bad}")
    except F.PeHipError as err:
        assert err.code == F.ERR_ARG, (bad, err)
    assert np.array_equal(e.solution(), ref[0]) and np.array_equal(e.state()["t"], ref[1]) and np.array_equal(e.tr_step_log()[0], ref[2]), bad
assert lib.pe_hip_analyze_tr_adaptive(e._h, C.c_double(0.05), None, None) == F.ERR_ARG
st = e.analyze_tr_adaptive(0.041, 1e-5)
assert st["rc"] == 0 and st["n_accepted"] > 0
e.close()
# no circuit
f = F.Engine()
ctl = F.TrControl(1e-6, 0, 0, 0, 0, 0, 0, 0, 0, 0, None)
assert lib.pe_hip_analyze_tr_adaptive(f._h, C.c_double(1.0), C.byref(ctl), None) == F.ERR_ARG
n = C.c_longlong(-1)
assert lib.pe_hip_get_tr_step_log(f._h, 0, 0, None, None, C.byref(n)) == 0 and n.value == 0
f.close()
# instances at different time points
deck5, ov = mesh5()
e = engine(deck5, 5, ov, knobs=knobs)
e.analyze_tr(1e-10, 1)
# (a checkpoint blob holds t_now of the five instances side by side: one of them edited puts the batch at two time points, which is
#  what a failed and rolled-back instance leaves behind)
blob2 = bytearray(e.checkpoint())
tpos = bytes(blob2).find(np.full(5, e.state()["t"][0]).tobytes())
assert tpos > 0
blob2[tpos + 16:tpos + 24] = np.array([3e-10]).tobytes()
e.restore(bytes(blob2))
assert len(set(e.state()["t"].tolist())) == 2
try:
    e.analyze_tr_adaptive(1e-8, 1e-11); raise AssertionError("accepted instances at different t")
except F.PeHipError as err:
    assert err.code == F.ERR_ARG
e.analyze_tr(1e-10, 1)   # still usable
e.close()
# a host-stamp overlay is refused
OV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
def cb(user, event, mode, t, dt, x, a, b):
    if event == 1:
        a[0] = 1e-3
        b[0] = 0.0
    return 0
fn = OV(cb)
e = F.Engine(); e.set_options(g_min=0.0)
lib.pe_hip_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_int, OV, C.c_void_p]
rows = np.array([1], dtype=np.int32); cols = np.array([1], dtype=np.int32); rr = np.array([1], dtype=np.int32)
assert lib.pe_hip_set_overlay(e._h, 1, F._ip(rows), F._ip(cols), None, 1, F._ip(rr), 0, fn, None) == 0
e.load_deck(D.rc_step(), 1); e.reset()
try:
    e.analyze_tr_adaptive(1e-6, 1e-9); raise AssertionError("accepted a host-stamp overlay")
except F.PeHipError as err:
    assert err.code == F.ERR_ARG
e.analyze_tr(1e-8, 2)
e.close()
print("ok")
'''


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_window_rules_and_refused_arguments(emu, knobs):
    assert "ok" in run(emu, RULES % knobs)


# ---- breakpoints from the generators: every kind's corners, a phase shift, and the rule that per-instance parameters give none
SOURCE_BP = r'''
knobs = %r
import math
d = D.Deck(); d.n_nodes = 6
d.add("SQR", (1, 0), 3.0, 0.5, 2e3, 0.3, 1.0)       # Vh, Vl, freq, duty, phase
d.add("SAW", (2, 0), 5.0, -1.0, 1e3, 0.0)
d.add("TRI", (3, 0), 2.0, -2.0, 4e3, 2.5)
for n in (1, 2, 3):
    d.add("R", (n, n + 3), 1000.0); d.add("C", (n + 3, 0), 1e-7)
T_STOP = 1.2e-3
def corners(freq, cs, phase):
    T, shift = 1.0 / freq, phase / (2.0 * math.pi) / freq
    return [k * T + c - shift for k in range(-1, int(T_STOP * freq) + 2) for c in cs if 0 < k * T + c - shift < T_STOP]
sqr, saw, tri = corners(2e3, (0.0, 0.3 / 2e3), 1.0), corners(1e3, (0.0,), 0.0), corners(4e3, (0.0, 0.5 / 4e3), 2.5)
assert len(sqr) >= 4 and len(saw) == 1 and len(tri) >= 8
hits = lambda t, bs: [b for b in bs if np.min(np.abs(t - b)) <= EPS4 * abs(b)]
def go(batch=1, ov=None, sb=True):
    e = engine(d, batch, ov, knobs=knobs)
    e.set_probes(list(range(d.rows)), 8192, 1); e.arm_probes()
    st = e.analyze_tr_adaptive(T_STOP, 1e-7, source_breakpoints=sb, **TOL)
    return e, st, *samples(e)
e, st, t, x = go()
assert hits(t, sqr) == sqr and hits(t, saw) == saw and hits(t, tri) == tri, "every corner of every generator is a point of the run"
check_decisions(e, st, t, x, d.n_nodes, 0.0, T_STOP, 1e-7, 1e-16, T_STOP / 50, TOL, bps=sqr + saw + tri)   # dt_init after each of them
e, st, t, x = go(sb=False)
assert not hits(t, sqr + saw + tri), "without the flag no step is aimed at a corner"
check_decisions(e, st, t, x, d.n_nodes, 0.0, T_STOP, 1e-7, 1e-16, T_STOP / 50, TOL)
# two instances whose square waves differ in frequency: that generator gives no breakpoints, the shared ones still do
par = [p for k, _, _, p, _ in F.deck_tables(d, 1)[2] if k == F.VGEN][0]
par = np.repeat(par[None], 2, 0).copy()
par[1, 0, 3] = 2.1e3
e, st, t, x = go(2, {"VGEN": par})
assert not hits(t, sqr) and not hits(t, corners(2.1e3, (0.0, 0.3 / 2.1e3), 1.0)) and hits(t, saw) == saw and hits(t, tri) == tri
check_decisions(e, st, t, x, d.n_nodes, 0.0, T_STOP, 1e-7, 1e-16, T_STOP / 50, TOL, bps=saw + tri)
print("ok")
'''


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_source_breakpoints_of_every_generator_kind(emu, knobs):
    assert "ok" in run(emu, SOURCE_BP % knobs)


# ---- 8. a NaN cannot pass, through the controller: one instance of a batch holds a NaN when the call starts
NAN_STATE = r'''
knobs = %r
deck, ov = mesh5()
e = engine(deck, 5, ov, knobs=knobs)
e.analyze_tr_adaptive(2e-9, 2e-11)
x = e.solution()
x[2, 3] = np.nan
e.set_solution(x)                     # (restarts the history: the LTE test is off, the status / finiteness part of the test alone decides)
t0 = e.state()["t"][0]
e.set_probes([0, 3], 64, 1); e.arm_probes()
st = e.analyze_tr_adaptive(t0 + 1e-9, 2e-11, dt_min=2e-12, check=False)
dt, oc = e.tr_step_log()
assert st["rc"] != 0 and st["n_accepted"] == 0 and st["n_rejected_newton"] == len(oc) == 3 and np.all(oc == 2), (st, dt, oc)
assert dt[0] == 2e-11 and dt[1] == 2e-11 / 8 and dt[2] == 2e-12, dt     # h / 8, then dt_min, where the call ends
s = e.state()
assert s["status"][2] == st["rc"] and np.all(s["t"] == t0) and st["t_end"] == t0, (s, st)
assert np.array_equal(e.solution(), x, equal_nan=True), "every attempt was rolled back to the state of the call's start"
assert list(e.probe_samples()[2]) == [1] * 5, "nothing was recorded"
print("ok")
'''


@pytest.mark.parametrize("knobs", SCHEDULES, ids=IDS)
def test_a_nan_in_the_state_is_never_accepted(emu, knobs):
    assert "ok" in run(emu, NAN_STATE % knobs)


# ---- 8. a NaN cannot pass: the reduction text of pe_lte.hpp with a one-thread team
LTE_UNIT = r'''
#include "pe_lte.hpp"
#include <cstdio>
#include <limits>
#include <vector>
struct Team { int tid() const { return 0; } int size() const { return 1; } };
int main()
{
    int const B = 3, R = 5;
    std::vector<double> x(B * R), hist(3 * B * R);
    double const t[4] = {0.0, 1.0, 2.5, 3.0};
    auto f = [](double tt, int b, int r) { return (1.0 + b) * tt * tt * tt + r * tt + 0.25; };  // cubic: DD3 = 1 + b exactly representable
    for(int b = 0; b < B; ++b)
        for(int r = 0; r < R; ++r)
        {
            for(int k = 0; k < 3; ++k) hist[(static_cast<size_t>((k + 1) % 3) * B + b) * R + r] = f(t[k], b, r);
            x[b * R + r] = f(t[3], b, r);
        }
    pe::DevView V{};
    V.rows = R; V.n_nodes = 3; V.batch = B; V.x = x.data();
    pe::LteView L{};
    L.hist = hist.data(); L.s0 = 1; L.s1 = 2; L.s2 = 0;
    L.t0 = t[0]; L.t1 = t[1]; L.t2 = t[2]; L.tn = t[3]; L.h = 0.5;
    L.reltol = 0.0; L.abstol_v = 1.0; L.abstol_i = 0.5; L.trtol = 1.0; L.test = 1;
    int bad = 0;
    auto q_of = [&](int b, int& nonfinite) { nonfinite = 0; return pe::lte_value(pe::lte_partial(Team{}, V, L, b, nonfinite)); };
    int nf = 0;
    for(int b = 0; b < B; ++b)
    {
        double const q = q_of(b, nf), want = 0.5 * 0.125 * (1.0 + b) / 0.5;   // the branch rows (abstol 0.5) are the worst
        if(!(std::fabs(q - want) <= 1e-12 * want) || nf) { std::printf("instance %d: q %.17g, expected %.17g\n", b, q, want); ++bad; }
    }
    double const nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // a NaN in a HISTORY row: q is a NaN -- not the maximum of the other rows, which fmax would have returned -- and never passes
    double& planted = hist[(static_cast<size_t>(2) * B + 1) * R + 0];
    double const keep = planted;
    for(double v: {nan, -nan})
    {
        planted = v;
        double const q = q_of(1, nf);
        if(q == q || pe::lte_passes(q) || nf) { std::printf("NaN in the history gave q = %g\n", q); ++bad; }
        if(!(q_of(2, nf) == q_of(2, nf))) { std::printf("NaN leaked into another instance\n"); ++bad; }
    }
    planted = keep;
    // a non-finite CANDIDATE raises the flag whether or not the test runs, and its q never passes
    for(double v: {nan, inf, -inf})
        for(int test = 0; test < 2; ++test)
        {
            x[2 * R + 4] = v;
            L.test = test;
            double const q = q_of(2, nf);
            if(!nf || (test && pe::lte_passes(q))) { std::printf("candidate %g, test %d: flag %d q %g\n", v, test, nf, q); ++bad; }
            q_of(0, nf);
            if(nf) { std::printf("flag raised for a finite instance\n"); ++bad; }
        }
    // the image orders like the value and keeps the NaN on top
    if(!(pe::lte_image(0.5) < pe::lte_image(2.0) && pe::lte_image(2.0) < pe::lte_image(inf) && pe::lte_image(inf) < pe::lte_image(nan) && pe::lte_image(-3.0) == pe::lte_image(3.0))) ++bad;
    if(pe::lte_passes(nan) || pe::lte_passes(1.0000001) || !pe::lte_passes(1.0) || !pe::lte_passes(0.0)) ++bad;
    std::printf(bad ? "FAILED %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
'''


def test_a_nan_cannot_pass_the_lte_reduction(tmp_path):
    src = tmp_path / "lte_unit.cpp"
    src.write_text(LTE_UNIT)
    exe = tmp_path / "lte_unit"
    cc = subprocess.run(["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "tests", "emu", "hip_shim"), "-I", os.path.join(ROOT, "phy-engine_amd", "csrc"),
                         "-o", str(exe), str(src)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr)
