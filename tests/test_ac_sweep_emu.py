"""Frequency-batched small-signal AC (pe_hip_set_ac_sweep_rows / pe_hip_analyze_ac_sweep / pe_hip_get_ac_sweep, include/pe_hip.h) on the
CPU: the engine's host logic and the team-generic kernel text (pe_ac_sweep.hpp) through the host emulation library (tests/emu: test
infrastructure), one child process per case.  No case but the overlay one and the one about failing points may lean on the single-point
fallback: each asserts n_fallback_points == 0."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def emu():
    make("-C", os.path.join(ROOT, "tests", "emu"))
    return EMU


PRE = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import ctypes as C
import numpy as np
import pe_load
pe = pe_load.load()
F = pe.ffi
from parity_common import golden, golden_complex

def within(a, b):
    """the project's AC tolerance (tests/test_gpu_parity.py test_ac_golden_parity)"""
    return bool(np.all(np.abs(a - b) <= 1e-9 + 1e-6 * np.abs(b)))

def bands(omegas):
    """number of frequency bands of include/pe_hip.h: ascending, omega == 0 on its own, a band takes omega <= 10 x its first"""
    w = np.sort(np.asarray(omegas, dtype=float))
    n, i = 0, 0
    while i < len(w):
        j = i + 1
        while j < len(w) and (w[j] == 0.0 if w[i] == 0.0 else w[j] <= 10.0 * w[i]):
            j += 1
        n, i = n + 1, j
    return n

def passes(omegas, P):
    w = np.sort(np.asarray(omegas, dtype=float))
    n, i = 0, 0
    while i < len(w):
        j = i + 1
        while j < len(w) and (w[j] == 0.0 if w[i] == 0.0 else w[j] <= 10.0 * w[i]):
            j += 1
        n, i = n + -(-(j - i) // P), j
    return n

MESH = pe.deck.rc_mesh(12, 12, 1, True)
MESH_W = np.logspace(7.0, 11.5, 46)          # 4.5 decades; every point solves on the single-point path of the parent commit

def mesh_engine(knobs=None, deck=MESH, batch=1, overrides=None):
    e = F.Engine()
    e.set_options(g_min=0.0)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    e.analyze_dc(F.MODE_OP)
    return e

def loop(e, omegas):
    out = []
    for w in omegas:
        x, rc = e.analyze_ac(w)
        assert rc == 0
        out.append(x)
    return np.array(out)           # [n_points][batch][rows]
''' % (ROOT, ROOT)


def run(emu, body, **env):
    e = dict(os.environ, PE_HIP_LIB=emu, **env)
    e.pop("PHY_ENGINE_HIP_AC_SWEEP_POINTS", None)
    r = subprocess.run([sys.executable, "-c", PRE + body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


@pytest.mark.parametrize("name", ["ac_rc_lowpass", "ac_linear_mix", "ac_nmos_amp", "ac_rlc_diode_acop", "ac_controlled_rest_acop", "ac_transistors_acop", "ac_transistors_hf_acop"])
def test_reference_goldens_in_one_sweep(emu, name):
    run(emu, r'''
meta, gx, deck = golden(%r)
e = F.Engine()
e.set_options(g_min=meta["gmin"], r_open=meta.get("r_open", 0.0))
e.load_deck(deck)
e.reset()
if meta["analysis"] == "ACOP" or deck.has_nonlinear():
    e.analyze_dc(F.MODE_OP)
x, status, st = e.analyze_ac_sweep(meta["omegas"])
g = golden_complex(meta, gx)
assert x.shape == (len(g), 1, g.shape[1]) and list(status) == [0] * len(g)
assert within(x[:, 0, :], g), np.max(np.abs(x[:, 0, :] - g))
assert st["n_fallback_points"] == 0 and st["n_points"] == len(g) and st["n_analyses"] == bands(meta["omegas"]), st
''' % name)


def test_shuffled_sweep_matches_the_single_point_path(emu):
    run(emu, r'''
rng = np.random.default_rng(3)
idx = rng.permutation(len(MESH_W))
idx = np.concatenate([idx, idx[5:6]])              # one duplicate
w = MESH_W[idx]
ref = loop(mesh_engine(), MESH_W)[idx]
e = mesh_engine()
x, status, st = e.analyze_ac_sweep(w)
assert x.shape == ref.shape and list(status) == [0] * len(w)
assert within(x, ref), "results in the caller's order, within the AC tolerance of the single-point path"
assert np.array_equal(x[-1], x[5]), "the duplicate point"
assert st["n_analyses"] == bands(w) == 5, st
assert st["n_passes"] == passes(w, st["points_per_pass"]) and st["points_per_pass"] > 1, st
assert st["n_fallback_points"] == 0, st
# the single-point path of an engine that has swept (automatic pass size: sized on the single-point engine) is the fresh engine's, bit for bit
assert np.array_equal(loop(e, MESH_W[:12:3]), loop(mesh_engine(), MESH_W[:12:3]))
''')


def test_one_point_per_pass_is_bit_identical_to_the_single_point_loop(emu):
    """batch 1, AC_SWEEP_POINTS = 1, ascending points: same bands, same pivot orders, same values, same refinement decisions as the loop
    of pe_hip_analyze_ac on a fresh engine -- pins the device-made value vector and the per-instance refinement to the host's arithmetic
    (omega = 0 and an inductor included: the ACOP fixture)."""
    run(emu, r'''
ref = loop(mesh_engine(), MESH_W)
x, status, st = mesh_engine({"AC_SWEEP_POINTS": 1}).analyze_ac_sweep(MESH_W)
assert np.array_equal(x, ref)
assert st["n_passes"] == len(MESH_W) and st["points_per_pass"] == 1 and st["n_fallback_points"] == 0, st
meta, gx, deck = golden("ac_rlc_diode_acop")
assert meta["omegas"][0] == 0.0
res = []
for sweep in (False, True):
    e = F.Engine()
    e.set_options(g_min=meta["gmin"], r_open=meta.get("r_open", 0.0))
    e.set_knob("AC_SWEEP_POINTS", 1)
    e.load_deck(deck)
    e.reset()
    e.analyze_dc(F.MODE_OP)
    if sweep:
        x, _, st = e.analyze_ac_sweep(meta["omegas"])
        assert st["n_fallback_points"] == 0, st
        res.append(x)
    else:
        res.append(loop(e, meta["omegas"]))
assert np.array_equal(res[0], res[1]) and np.array_equal(np.signbit(res[0].real), np.signbit(res[1].real))
''')


def test_pass_size_does_not_matter(emu):
    run(emu, r'''
res = {}
for P in (1, 3, 0):
    x, status, st = mesh_engine({"AC_SWEEP_POINTS": P}).analyze_ac_sweep(MESH_W)
    assert st["n_fallback_points"] == 0 and list(status) == [0] * len(MESH_W), st
    want = passes(MESH_W, P) if P else bands(MESH_W)      # automatic: the emulation's budget holds every band of this circuit whole
    assert st["n_passes"] == want and st["n_analyses"] == bands(MESH_W), (P, st)
    assert (st["points_per_pass"] == P) if P else (st["points_per_pass"] >= 2), (P, st)
    res[P] = x
assert within(res[1], res[0]) and within(res[3], res[0]) and within(res[3], res[1])
# the knob is read at every sweep: set after the first one, it takes effect at the next
e = mesh_engine()
_, _, st0 = e.analyze_ac_sweep(MESH_W)
e.set_knob("AC_SWEEP_POINTS", 2)
x2, _, st2 = e.analyze_ac_sweep(MESH_W)
assert st0["points_per_pass"] > 2 and st2["points_per_pass"] == 2 and st2["n_passes"] == passes(MESH_W, 2), (st0, st2)
assert within(x2, res[0])

# a batch of four instances with their own C: |v_out| = 2^-1/2 at omega = 1 / (R C_b)
d = pe.deck.ac_rc_lowpass()
caps = np.array([1e-6, 2e-6, 5e-7, 1e-7])
w = 1.0 / (1000.0 * caps)
for P in (1, 3, 0):
    e = F.Engine()
    e.set_options(g_min=0.0)
    e.set_knob("AC_SWEEP_POINTS", P)
    e.load_deck(d, batch=4, overrides={"C": caps[:, None, None]})
    e.reset()
    x, status, st = e.analyze_ac_sweep(w)
    assert st["n_fallback_points"] == 0 and x.shape == (4, 4, e.rows), st
    for b in range(4):
        assert abs(abs(x[b, b, 1]) - 2.0 ** -0.5) < 1e-12, (P, b, abs(x[b, b, 1]))
    e2 = F.Engine()
    e2.set_options(g_min=0.0)
    e2.load_deck(d, batch=4, overrides={"C": caps[:, None, None]})
    e2.reset()
    assert within(x, loop(e2, w))
''')


def test_row_selection(emu):
    run(emu, r'''
e = mesh_engine()
full, _, st = e.analyze_ac_sweep(MESH_W)
rows = [0, 17, 17, 143, e.rows - 1, 144]          # mesh nodes (one twice), the last branch row, the source node
e.set_ac_sweep_rows(rows)
re = np.empty((1, 1, len(rows))); im = np.empty_like(re)   # a stored sweep has the layout of its rows: unreadable once they change
assert F.lib().pe_hip_get_ac_sweep(e._h, 0, 1, 0, 1, F._dp(re), F._dp(im)) == F.ERR_ARG
x, status, st = e.analyze_ac_sweep(MESH_W)
assert x.shape == (len(MESH_W), 1, len(rows)) and st["n_fallback_points"] == 0
assert np.array_equal(x, full[:, :, rows]), "kept rows equal the same rows of the all-rows sweep bit for bit"
# a slice of points through the C ABI
re = np.empty((3, 1, len(rows))); im = np.empty_like(re)
assert F.lib().pe_hip_get_ac_sweep(e._h, 4, 3, 0, 1, F._dp(re), F._dp(im)) == 0
assert np.array_equal(re + 1j * im, x[4:7])
# a bad row is refused and changes nothing
for bad in ([0, e.rows], [-1]):
    try:
        e.set_ac_sweep_rows(bad); raise AssertionError("accepted")
    except F.PeHipError as err:
        assert err.code == F.ERR_ARG
assert F.lib().pe_hip_get_ac_sweep(e._h, 4, 3, 0, 1, F._dp(re), F._dp(im)) == 0 and np.array_equal(re + 1j * im, x[4:7])
x2, _, _ = e.analyze_ac_sweep(MESH_W)
assert np.array_equal(x2, x)
e.set_ac_sweep_rows(None)
x3, _, _ = e.analyze_ac_sweep(MESH_W)
assert np.array_equal(x3, full)
''')


def test_invalidation_and_arguments(emu):
    run(emu, r'''
lib = F.lib()
e = mesh_engine()
n = e.rows
re = np.empty((2, 1, n)); im = np.empty_like(re)
get = lambda: lib.pe_hip_get_ac_sweep(e._h, 0, 2, 0, 1, F._dp(re), F._dp(im))
assert get() == F.ERR_ARG and b"no AC sweep yet" in lib.pe_hip_last_error(e._h), "before any sweep"
w = MESH_W[:6]
for name in ("analyze_dc", "analyze_tr", "reset", "set_solution", "checkpoint_load", "update_param", "load_deck"):
    e.analyze_ac_sweep(w)
    assert get() == 0, name
    if name == "analyze_dc": e.analyze_dc(F.MODE_OP)
    elif name == "analyze_tr": e.analyze_tr(1e-10, 1)
    elif name == "reset": e.reset()
    elif name == "set_solution": e.set_solution(e.solution())
    elif name == "checkpoint_load": e.restore(e.checkpoint())
    elif name == "update_param": e.update_param(F.R, 0, 0, 1234.0)
    else: e.load_deck(MESH, 1)
    assert get() == F.ERR_ARG and b"no AC sweep yet" in lib.pe_hip_last_error(e._h), name
    if name in ("reset", "load_deck"):
        e.reset(); e.analyze_dc(F.MODE_OP)
# out-of-range reads
e.analyze_ac_sweep(w)
assert lib.pe_hip_get_ac_sweep(e._h, 5, 2, 0, 1, F._dp(re), F._dp(im)) == F.ERR_ARG
assert lib.pe_hip_get_ac_sweep(e._h, 0, 2, 1, 1, F._dp(re), F._dp(im)) == F.ERR_ARG
assert get() == 0
# bad sweeps
st = F.AcSweepStats()
one = np.array([1e8, 1e9])
assert lib.pe_hip_analyze_ac_sweep(e._h, 0, F._dp(one), None, C.byref(st)) == F.ERR_ARG
assert lib.pe_hip_analyze_ac_sweep(e._h, 2, None, None, C.byref(st)) == F.ERR_ARG
for bad in (-1.0, float("nan"), float("inf")):
    ws = np.array([1e8, bad])
    assert lib.pe_hip_analyze_ac_sweep(e._h, 2, F._dp(ws), None, None) == F.ERR_ARG, bad
x, status, st = e.analyze_ac_sweep(w)              # the engine is still usable
assert list(status) == [0] * len(w) and st["n_fallback_points"] == 0
# without a circuit
f = F.Engine()
assert lib.pe_hip_analyze_ac_sweep(f._h, 2, F._dp(one), None, None) == F.ERR_ARG
assert lib.pe_hip_set_ac_sweep_rows(f._h, 0, None) == F.ERR_ARG
f.close()
''')


def test_points_that_fail_in_their_batch(emu):
    """VAC - R - C - C: the node between the capacitors is held by nothing at omega = 0, so the band of the omega = 0 points cannot even be
    analysed -- it must fail into the single-point path point by point (PE_HIP_ERR_SINGULAR there), while the other bands solve and stay
    readable, whatever the pass size (the automatic one sizes itself on a band that can be analysed).  Then a batch whose second instance
    is singular at every omega (both capacitors 0: a floating node), found by the factorisation of that instance, not by the analysis."""
    run(emu, r'''
d = pe.deck.Deck()
d.n_nodes = 3
d.add("VAC", (1, 0), 1.0, 1000.0, 0.0)
d.add("R", (1, 2), 1000.0)
d.add("C", (2, 3), 1e-6)
d.add("C", (3, 0), 2e-6)
w = np.array([0.0, 1e3, 0.0, 2e3, 1e5])
def engine(P=0, batch=1, ov=None):
    e = F.Engine()
    e.set_options(g_min=0.0)
    e.set_knob("AC_SWEEP_POINTS", P)
    e.load_deck(d, batch, ov)
    e.reset()
    return e
ref = engine()
want_rc = [ref.analyze_ac(x, check=False)[1] for x in w]
assert want_rc == [F.ERR_SINGULAR, 0, F.ERR_SINGULAR, 0, 0], want_rc
good = [1, 3, 4]
want = loop(engine(), w[good])
for P in (4, 0, 1):
    e = engine(P)
    status = np.full(len(w), 77, dtype=np.int32)
    st = F.AcSweepStats()
    rc = F.lib().pe_hip_analyze_ac_sweep(e._h, len(w), F._dp(w), F._ip(status), C.byref(st))
    assert rc == F.ERR_SINGULAR, (P, rc)                       # the first failing point's status
    assert list(status) == want_rc, (P, status)
    assert st.n_fallback_points == 2 and st.n_points == 5 and st.n_analyses == 3, (P, st.asdict())
    re = np.empty((len(w), 1, e.rows)); im = np.empty_like(re)
    assert F.lib().pe_hip_get_ac_sweep(e._h, 0, len(w), 0, 1, F._dp(re), F._dp(im)) == 0, "the points that solved stay readable"
    x = re + 1j * im
    assert np.all(np.isnan(re[[0, 2]])) and np.all(np.isnan(im[[0, 2]])), "a failed point reads NaN"
    assert within(x[good], want) and abs(x[1, 0, 0] - 1.0) < 1e-12, P
    x2, status2, st2 = e.analyze_ac_sweep(w, check=False)     # the binding returns what solved instead of raising
    assert st2["rc"] == F.ERR_SINGULAR and list(status2) == want_rc and np.array_equal(x2[good], x[good])
    x3, status3, st3 = e.analyze_ac_sweep(w[good])            # and the engine goes on
    assert list(status3) == [0, 0, 0] and st3["n_fallback_points"] == 0 and np.array_equal(x3, x[good])

# an instance that is singular in the factorisation: every point has a failing instance, goes to the single-point path and fails there too
ov = {"C": np.array([[1e-6, 2e-6], [0.0, 0.0]])[:, :, None]}
wb = np.array([1e3, 2e3, 1e5])
assert [engine(0, 2, ov).analyze_ac(x, check=False)[1] for x in wb] == [F.ERR_SINGULAR] * 3
for P in (2, 0):
    e = engine(P, 2, ov)
    x, status, st = e.analyze_ac_sweep(wb, check=False)
    assert st["rc"] == F.ERR_SINGULAR and list(status) == [F.ERR_SINGULAR] * 3 and st["n_fallback_points"] == 3 and st["n_passes"] >= 1, (P, st)
    assert np.all(np.isnan(x.real)) and np.all(np.isnan(x.imag))
''')


def test_host_stamp_overlay_takes_the_single_point_path(emu):
    """the circuit of tests/cpp/overlay_batch.cpp (cubic conductor + capacitor as host hooks on node 2, an AC current source), two
    instances: the values of the overlay come from callbacks per omega, so every point is a fallback point"""
    run(emu, r'''
FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
K, G, CAP = [2e-4, 8e-4], 1e-3, 2e-9
state = {"i": 0, "ac": 0}
def hook(user, event, mode, t, dt, x, a, b):
    if event == 4:                                 # PE_HIP_OVERLAY_INSTANCE
        state["i"] = mode
        return 0
    k = K[state["i"]]
    if event == 1:                                 # ITERATE: i = (g + 3 k v^2) v' - 2 k v^3
        v = x[1]
        a[0] = G + 3.0 * k * v * v
        b[0] = 2.0 * k * v * v * v
    elif event == 3:                               # AC: g + 3 k v_op^2 + j omega C
        v = x[1]
        a[0] = G + 3.0 * k * v * v
        a[1] = t * CAP
        b[0] = b[1] = 0.0
        state["ac"] += 1
    return 0
cb = FN(hook)
lib = F.lib()
lib.pe_hip_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_int, FN, C.c_void_p]
one = np.array([1], dtype=np.int32)
rep = np.array([1e-3])
def engine():
    e = F.Engine()
    assert lib.pe_hip_set_overlay(e._h, 1, F._ip(one), F._ip(one), F._dp(rep), 1, F._ip(one), 1, cb, None) == 0
    e.set_options(g_min=1e-12)
    tables = [(F.VDC, np.array([[1, 0]], dtype=np.int32), np.array([0], dtype=np.int32), np.array([[3.0]]), 0),
              (F.R, np.array([[1, 2]], dtype=np.int32), None, np.array([[[1500.0]], [[700.0]]]), 1),
              (F.IAC, np.array([[0, 2]], dtype=np.int32), None, np.array([[1e-3, 2e5, 0.0]]), 0)]
    e.load(2, 1, tables, batch=2)
    e.analyze_dc(F.MODE_DC)
    return e
w = np.array([2e5, 3e3, 7e6, 2e5])
ref = loop(engine(), w)
state["ac"] = 0
x, status, st = engine().analyze_ac_sweep(w)
assert st["n_fallback_points"] == len(w) and st["n_passes"] == 0 and list(status) == [0] * len(w), st
assert state["ac"] == 2 * len(w)
assert np.array_equal(x, ref)
assert x[0, 0, 1] != x[0, 1, 1] and x[0, 0, 1] != x[1, 0, 1]
''')


def test_plugin_api_sweeps_under_host_emulation(emu):
    """tests/cpp/ac_sweep.cpp: run_ac_analysis of the plug-in API makes one batched sweep (log over six decades, linear) of an R-L-C
    network with a closed form; the last point stays in the nodes"""
    make("-C", CPP, "_build_emu/ac_sweep")
    out = subprocess.run([os.path.join(CPP, "_build_emu", "ac_sweep")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"ac_sweep exited {out.returncode}: {out.stderr}"
