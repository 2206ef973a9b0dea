"""Transient probes and measurements (pe_hip_set_probes / _arm_probes / _get_probe_samples / _get_measures, include/pe_hip.h) on the
CPU: the engine's host logic and the team-generic recording code (pe_probe.hpp) through the host emulation library (tests/emu: test
infrastructure), one child process per case."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")


@pytest.fixture(scope="module")
def emu():
    make("-C", os.path.join(ROOT, "tests", "emu"))
    return EMU


# shared by every child: a nonlinear RC mesh with per-instance parameters, probes on node and branch rows, every measure kind, and
# the measures recomputed with numpy from stride-1 samples (the definitions of include/pe_hip.h)
PRE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import ctypes as C
import numpy as np
import pe_load
pe = pe_load.load()
F = pe.ffi
B, W, N, DT = 5, 6, 24, 2e-10
deck, r, c = pe.deck.rc_mesh_params(W, W, list(range(1, B + 1)), True)
OV = {"R": r[:, :, None], "C": c[:, :, None]}
NN = W * W + 1
ROWS = [0, 7, 7, W * W - 1, W * W, NN]          # mesh nodes (one twice), the source node, the source's branch current
MEAS = [("min", 0), ("max", 0), ("avg", 1), ("rms", 3), ("integ", 5), ("cross", 0, 0.5, 1, 1), ("cross", 0, 0.5, -1, 1),
        ("cross", 0, 0.3, 0, 2), ("cross", 4, -0.5, 0, 1), ("max", 5), ("min", 4), ("cross", 2, 5.0, 0, 1)]
KIND = F._MEAS_NAMES

def engine(knobs=None, batch=B):
    e = F.Engine()
    e.set_options(g_min=0.0)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, {k: v[:batch] for k, v in OV.items()})
    e.reset()
    return e

def stepwise(knobs=None, n=N):
    """solution and t after each of n calls of analyze_tr(DT, 1), starting with the point before them"""
    e = engine(knobs)
    xs, ts = [e.solution()], [e.state()["t"]]
    for _ in range(n):
        e.analyze_tr(DT, 1)
        xs.append(e.solution())
        ts.append(e.state()["t"])
    e.close()
    return np.stack(xs, 1), np.stack(ts, 1)   # [B][n+1][rows], [B][n+1]

def ref_measures(t, v, meas=MEAS):
    """[n_meas][2] of one instance from its stride-1 samples t [n], v [n][P]"""
    out = []
    T = t[-1] - t[0]
    for m in meas:
        kind, p = KIND[m[0]], m[1]
        y = v[:, p]
        if kind in (F.MEAS_MIN, F.MEAS_MAX):
            best, when = y[0], t[0]
            for k in range(1, len(y)):
                if (y[k] < best) if kind == F.MEAS_MIN else (y[k] > best):
                    best, when = y[k], t[k]
            out.append((best, when))
        elif kind in (F.MEAS_INTEG, F.MEAS_AVG, F.MEAS_RMS):
            s = 0.0
            for k in range(1, len(y)):
                s += (t[k] - t[k - 1]) * ((y[k - 1] + y[k]) if kind != F.MEAS_RMS else (y[k - 1] ** 2 + y[k] ** 2)) * 0.5
            val = s if kind == F.MEAS_INTEG else (np.nan if T == 0 else (s / T if kind == F.MEAS_AVG else np.sqrt(s / T)))
            out.append((val, T))
        else:
            level, edge, occ = m[2], m[3], m[4]
            n, when = 0, np.nan
            for k in range(1, len(y)):
                v0, v1 = y[k - 1], y[k]
                rise, fall = v0 < level <= v1, v0 > level >= v1
                if (rise if edge > 0 else (fall if edge < 0 else (rise or fall))):
                    n += 1
                    if n == occ:
                        when = t[k - 1] + (level - v0) * (t[k] - t[k - 1]) / (v1 - v0)
            out.append((when, float(n)))
    return np.array(out)

def check_measures(got, t, v, n_rec):
    """got [B][M][2] against numpy on the stride-1 samples: counts and MIN / MAX exact, times and integrals to rel 1e-12"""
    for b in range(got.shape[0]):
        ref = ref_measures(t[b, :n_rec[b]], v[b, :n_rec[b]])
        for k, m in enumerate(MEAS):
            kind = KIND[m[0]]
            g, e = got[b, k], ref[k]
            if kind in (F.MEAS_MIN, F.MEAS_MAX):
                assert g[0] == e[0] and g[1] == e[1], (b, m, g, e)
            elif kind == F.MEAS_CROSS:
                assert g[1] == e[1], (b, m, g, e)
                assert (np.isnan(g[0]) and np.isnan(e[0])) or abs(g[0] - e[0]) <= 1e-12 * abs(e[0]), (b, m, g, e)
            else:
                assert g[1] == e[1], (b, m, g, e)
                assert abs(g[0] - e[0]) <= 1e-12 * abs(e[0]) + 1e-300, (b, m, g, e)
''' % (ROOT, ROOT)


def run(emu, body, **env):
    e = dict(os.environ, PE_HIP_LIB=emu, **env)
    r = subprocess.run([sys.executable, "-c", PRE + body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.mark.parametrize("knobs", [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}], ids=["resident", "split", "split_graph"])
def test_samples_match_stepwise_runs_and_measures_match_numpy(emu, knobs):
    out = run(emu, r'''
knobs = %r
xs, ts = stepwise(knobs)
e = engine(knobs)
e.set_probes(ROWS, N + 1, 1, MEAS)
e.arm_probes()
e.analyze_tr(DT, N)
t, v, n_rec, n_drop = e.probe_samples()
assert list(n_rec) == [N + 1] * B and list(n_drop) == [0] * B, (n_rec, n_drop)
assert np.array_equal(t, ts), "sample times are the state's t after every step"
assert np.array_equal(v, xs[:, :, ROWS]), "samples are bit-identical to the stepwise solutions"
assert np.array_equal(e.solution(), xs[:, -1]), "recording leaves the solution as it was"
got = e.measures()
check_measures(got, t, v, n_rec)
# the wave has crossed the levels: the CROSS paths were exercised
assert np.all(got[:, 5, 1] >= 1) and np.all(got[:, 6, 1] >= 1) and np.all(got[:, 11, 1] == 0) and np.all(np.isnan(got[:, 11, 0]))
print("ok")
''' % knobs)
    assert "ok" in out


def test_stride_and_capacity(emu):
    run(emu, r'''
for knobs in ({"SPLIT": 0}, {"SPLIT": 1}):
    e = engine(knobs)
    e.set_probes(ROWS, N + 1, 1, MEAS)
    e.arm_probes(); e.analyze_tr(DT, N)
    t1, v1, _, _ = e.probe_samples(); m1 = e.measures()
    e.close()
    e = engine(knobs)
    e.set_probes(ROWS, N + 1, 3, MEAS)
    e.arm_probes(); e.analyze_tr(DT, N)
    t3, v3, n3, d3 = e.probe_samples(); m3 = e.measures()
    k = N // 3 + 1
    assert list(n3) == [k] * B and list(d3) == [0] * B
    assert np.array_equal(t3[:, :k], t1[:, ::3]) and np.array_equal(v3[:, :k], v1[:, ::3])
    assert np.all(np.isnan(t3[:, k:])) and np.all(np.isnan(v3[:, k:]))
    assert np.array_equal(m3, m1, equal_nan=True), "the stride thins the samples, never the measures"
    e.close()
    cap = 7
    e = engine(knobs)
    e.set_probes(ROWS, cap, 1, MEAS)
    e.arm_probes(); e.analyze_tr(DT, N)
    tc, vc, nc, dc = e.probe_samples(); mc = e.measures()
    assert list(nc) == [cap] * B and list(dc) == [N + 1 - cap] * B, (nc, dc)
    assert np.array_equal(tc, t1[:, :cap]) and np.array_equal(vc, v1[:, :cap])
    assert np.array_equal(mc, m1, equal_nan=True), "samples past capacity are dropped, the measures still see them"
    e.close()
''')


def test_failing_instances_record_accepted_steps_only(emu):
    """bridge_gmin0_fail: g_min = 0 makes the bridge singular once all four diodes are off; with per-instance load capacitors the
    instances fail at different steps.  A retry with g_min raised then solves groups of instances at different t (run_m2_tr)."""
    run(emu, r'''
from parity_common import golden
meta, gx, bdeck = golden("bridge_gmin0_fail")
BB = 4
cs = np.array([1e-4, 3e-6, 1e-5, 1e-4])[:, None, None]
for knobs in ({"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}):
    e = F.Engine(); e.set_options(g_min=0.0)
    for k, v in knobs.items(): e.set_knob(k, v)
    e.load_deck(bdeck, BB, {"C": cs}); e.reset()
    e.set_probes([0, 1, 2, 3], 400, 1, [("max", 2), ("integ", 3), ("cross", 2, 1.0, 0, 1)])
    e.arm_probes()
    st = e.analyze_tr(meta["dt"], 120, check=False)
    s = e.state()
    assert st["rc"] != 0 and np.any(s["status"] != 0), s
    e.set_options(g_min=1e-12)
    e.analyze_tr(meta["dt"], 30, check=False)   # failed instances resume from their own (rolled-back) time
    s = e.state()
    t, v, n_rec, n_drop = e.probe_samples()
    assert len(set(s["t"].tolist())) > 1, "the instances sit at different time points"
    for b in range(BB):
        assert n_rec[b] - 1 == s["steps"][b], (b, n_rec[b], s["steps"][b])
        tb = t[b, :n_rec[b]]
        assert np.all(np.diff(tb) > 0) and tb[-1] == s["t"][b]
        assert np.array_equal(v[b, n_rec[b] - 1], e.solution()[b])
    m = e.measures()
    assert np.all(m[:, 1, 1] == s["t"]), "T is the last accepted time - t_arm"
    e.close()
''')


def test_inaccurate_retry_on_the_split_schedule_keeps_the_order(emu):
    """A deliberately inexact LU (PE_EMU_PIVOT_ERROR) with refinement disabled on the resident kernel trips the residual check: the
    engine leaves the resident kernel for the split schedule and repeats the rolled-back steps there -- the samples stay in order."""
    run(emu, r'''
e = engine({"SPLIT": 0})
e.set_options(g_min=0.0, residual_tol=1e-13)
e.set_probes(ROWS, N + 1, 1, MEAS)
e.arm_probes()
e.analyze_tr(DT, N, check=False)
s = e.state()
assert e.safety_net()["careful"], "the safety net moved the engine to the split schedule"
t, v, n_rec, _ = e.probe_samples()
for b in range(B):
    assert n_rec[b] - 1 == s["steps"][b]
    assert np.all(np.diff(t[b, :n_rec[b]]) > 0) and t[b, n_rec[b] - 1] == s["t"][b]
    assert np.array_equal(v[b, n_rec[b] - 1], e.solution()[b][ROWS])
check_measures(e.measures(), t, v, n_rec)
''', PE_EMU_PIVOT_ERROR="1e-9")


def test_window_rules(emu):
    run(emu, r'''
def armed(knobs=None):
    e = engine(knobs)
    e.set_probes(ROWS, 64, 1, MEAS)
    e.arm_probes()
    e.analyze_tr(DT, 3)
    return e, e.probe_samples(), e.measures()

# arm writes sample 0 = the current solution and t, and initialises the measures there
e = engine()
e.analyze_tr(DT, 4)
e.set_probes(ROWS, 64, 1, MEAS)
t, v, n_rec, _ = e.probe_samples()
assert list(n_rec) == [0] * B and np.all(np.isnan(t)) and np.all(np.isnan(e.measures())), "nothing before the first arm"
e.arm_probes()
t, v, n_rec, n_drop = e.probe_samples()
x, s = e.solution(), e.state()
assert list(n_rec) == [1] * B and list(n_drop) == [0] * B
assert np.array_equal(t[:, 0], s["t"]) and np.array_equal(v[:, 0], x[:, ROWS]) and np.all(np.isnan(t[:, 1:]))
m = e.measures()
assert np.array_equal(m[:, 0, 0], x[:, ROWS[0]]) and np.array_equal(m[:, 0, 1], s["t"])       # MIN
assert np.all(np.isnan(m[:, 2, 0])) and np.all(m[:, 2, 1] == 0) and np.all(m[:, 4] == 0)     # AVG (T = 0), INTEG
assert np.all(np.isnan(m[:, 5, 0])) and np.all(m[:, 5, 1] == 0)                              # CROSS
e.close()

# every call that moves x or t other than analyze_tr disarms; what was recorded stays readable
blob = None
for name in ("analyze_dc", "reset", "set_solution", "set_time", "checkpoint_load"):
    e, (t0, v0, n0, d0), m0 = armed()
    if name == "analyze_dc": e.analyze_dc(F.MODE_DC)
    elif name == "reset": e.reset()
    elif name == "set_solution": e.set_solution(e.solution())
    elif name == "set_time": assert F.lib().pe_hip_set_time(e._h, C.c_double(1e-9), C.c_double(DT)) == 0
    else: e.restore(e.checkpoint())
    e.analyze_tr(DT, 2)
    t1, v1, n1, d1 = e.probe_samples()
    assert list(n1) == [4] * B, (name, n1)
    assert np.array_equal(t1, t0, equal_nan=True) and np.array_equal(v1, v0, equal_nan=True) and np.array_equal(d1, d0), name
    assert np.array_equal(e.measures(), m0, equal_nan=True), name
    e.arm_probes()                                     # a new window starts at the current point
    e.analyze_tr(DT, 1)
    assert list(e.probe_samples()[2]) == [2] * B, name
    e.close()

# load_circuit drops the configuration
e, _, _ = armed()
e.load_deck(deck, B, OV)
for call in (lambda: e.probe_samples(), lambda: e.measures(), lambda: e.arm_probes()):
    try:
        call(); raise AssertionError("accepted without a configuration")
    except F.PeHipError as err:
        assert err.code == F.ERR_ARG
e.reset(); e.analyze_tr(DT, 2)
# n_probes = n_measures = 0 removes it
e.set_probes(ROWS, 8, 1, MEAS); e.arm_probes(); e.analyze_tr(DT, 1)
e.set_probes([], 0, 0, ())
try:
    e.probe_samples(); raise AssertionError("configuration not removed")
except F.PeHipError as err:
    assert err.code == F.ERR_ARG
e.close()
''')


def test_bad_arguments_are_refused_and_the_engine_stays_usable(emu):
    run(emu, r'''
e = engine()
e.set_probes(ROWS, 16, 1, MEAS)
e.arm_probes(); e.analyze_tr(DT, 2)
ref = e.probe_samples()
lib = F.lib()
R = len(ROWS) and NN + 1
bad = [
    dict(rows=[0, R], capacity=8, stride=1, measures=()),                 # row out of range
    dict(rows=[-1], capacity=8, stride=1, measures=()),
    dict(rows=[0], capacity=0, stride=1, measures=()),                    # capacity < 1
    dict(rows=[0], capacity=8, stride=0, measures=()),                    # stride < 1
    dict(rows=[0], capacity=8, stride=1, measures=[(0, 0)]),              # unknown kind
    dict(rows=[0], capacity=8, stride=1, measures=[(7, 0)]),
    dict(rows=[0], capacity=8, stride=1, measures=[("max", 1)]),          # measure of a probe out of range
    dict(rows=[0], capacity=8, stride=1, measures=[("min", -1)]),
    dict(rows=[], capacity=8, stride=1, measures=[("min", 0)]),
    dict(rows=[0], capacity=8, stride=1, measures=[("cross", 0, 0.5, 1, 0)]),   # occurrence < 1
    dict(rows=[0], capacity=8, stride=1, measures=[("cross", 0, 0.5, 2, 1)]),   # edge outside {-1, 0, 1}
    dict(rows=[0], capacity=8, stride=1, measures=[("cross", 0, 0.5, -2, 1)]),
]
for a in bad:
    try:
        e.set_probes(**a); raise AssertionError(f"accepted: {a}")
    except F.PeHipError as err:
        assert err.code == F.ERR_ARG, (a, err)
# batch x capacity x (n_probes + 1) overflowing 64 bits (refused before the rows are read)
rows1 = np.zeros(1, dtype=np.int32)
n_m, arr = F._measures(())
rc = lib.pe_hip_set_probes(e._h, 2**31 - 1, F._ip(rows1), 2**31 - 1, 1, 0, arr)
assert rc == F.ERR_ARG, rc
# the engine and its configuration are as they were
assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(e.probe_samples(), ref))
e.analyze_tr(DT, 2)
assert list(e.probe_samples()[2]) == [5] * B
# without a circuit
f = F.Engine()
assert lib.pe_hip_set_probes(f._h, 1, F._ip(rows1), 8, 1, 0, arr) == F.ERR_ARG
assert lib.pe_hip_arm_probes(f._h) == F.ERR_ARG
f.close()
e.close()
''')


def test_sweep_over_two_emulated_devices_matches_one_and_the_engine(emu):
    run(emu, r'''
res = {}
for mask in (1, 3):
    s = F.Sweep(mask)
    s.set_options(g_min=0.0)
    s.load_deck(deck, B, OV)
    s.reset()
    s.set_probes(ROWS, N + 1, 2, MEAS)
    s.arm_probes()
    s.run(DT, N)
    res[mask] = (s.probe_samples(), s.measures(), s.probe_samples(1, 3), s.measures(2, 2))
    assert len(s.shards()) == (1 if mask == 1 else 2)
    s.close()
e = engine()
e.set_probes(ROWS, N + 1, 2, MEAS)
e.arm_probes()
e.analyze_tr(DT, N)
eng = (e.probe_samples(), e.measures())
for a, b, c in zip(res[1][0], res[3][0], eng[0]):
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
assert np.array_equal(res[1][1], res[3][1], equal_nan=True) and np.array_equal(res[1][1], eng[1], equal_nan=True)
for a, b in zip(res[3][2], eng[0]):
    assert np.array_equal(a, b[1:4], equal_nan=True)
assert np.array_equal(res[3][3], eng[1][2:4], equal_nan=True)
''', PE_EMU_DEVICES="2")


@pytest.mark.parametrize("knobs", [{"SPLIT": 0}, {"SPLIT": 1}], ids=["resident", "split"])
def test_configured_but_disarmed_probes_change_nothing(emu, knobs):
    run(emu, r'''
knobs = %r
a = engine(knobs)
a.analyze_tr(DT, 6)
b = engine(knobs)
b.set_probes(ROWS, 4, 1, MEAS)
b.analyze_tr(DT, 3)
b.arm_probes(); b.reset()                      # armed, then disarmed again
b.analyze_tr(DT, 6)
assert np.array_equal(a.solution(), b.solution())
assert list(b.probe_samples()[2]) == [1] * B
''' % knobs)
