"""Small-signal noise analysis (pe_hip_analyze_noise / pe_hip_get_noise*, include/pe_hip.h) on the CPU: the engine's host logic and the
team-generic kernel text (pe_noise.hpp) through the host emulation library (tests/emu: test infrastructure), one child process per case.
Reference and tolerance: tests/noise_common.py (the unchanged CPU oracle, direct method and transposed solve; the project's AC tolerance
propagated to a contribution).  No case but the one about failing points may lean on a retried point: each asserts n_retried_points == 0."""
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
O = pe_load.load_oracle()
import noise_common as NC

def oracle(deck, warm=None, op=None):
    """prepared oracle at its operating point (OP when the circuit is non-linear), optionally warm-started; returns (oracle, Newton iterations)"""
    o = O.Oracle(deck, g_min=0.0)
    o.prepare()
    if warm is not None:
        o.x = np.array(warm, dtype=float)
    it = o.solve("OP") if (o.nonlinear if op is None else op) else 0
    return o, it

def engine(deck, warm=None, batch=1, overrides=None, knobs=None, op=None):
    e = F.Engine()
    e.set_options(g_min=0.0)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    if warm is not None:
        e.set_solution(np.array([warm] * batch, dtype=float))
    if deck.has_nonlinear() if op is None else op:
        e.analyze_dc(F.MODE_OP)
    return e

def parity(deck, out_pos, out_neg, w, warm=None, bjt=None, what=""):
    o, it = oracle(deck, warm)
    assert it >= 0, it
    src = NC.sources(o, bjt_currents=bjt(o) if bjt else ())
    ref = NC.reference(o, w, out_pos, out_neg, src)
    e = engine(deck, warm)
    psd, c, status, st = e.analyze_noise(w, out_pos, out_neg, contributions=True)
    assert list(status) == [0] * len(w) and st["n_retried_points"] == 0 and st["n_sources"] == len(src[2]), st
    assert st["n_analyses"] == NC.bands(w) and st["n_points"] == len(w), st
    assert np.all(np.abs(e.noise_source_density()[0] - src[2]) <= 1e-6 * src[2]), "densities"
    NC.check(psd[:, 0], c[:, 0, :], ref, what)
    return e, o, psd, c

def mesh(seed):
    d = pe.deck.rc_mesh(12, 12, seed, True)
    d.add("IDC", (0, 79), 4e-4)                       # biases the junctions around the centre node: shot noise that is not zero
    return d
MESH_W = np.logspace(7.0, 11.5, 10)
''' % (ROOT, ROOT)


def run(emu, body, **env):
    e = dict(os.environ, PE_HIP_LIB=emu, **env)
    e.pop("PHY_ENGINE_HIP_AC_SWEEP_POINTS", None)
    r = subprocess.run([sys.executable, "-c", PRE + body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_closed_forms(emu):
    """R - C low pass: 4 k T R / (1 + (omega R C)^2) at the capacitor; its integral against k T / C with the quadrature error of these
    points computed here; a resistive divider: 4 k T (R1 || R2)"""
    run(emu, r'''
d = pe.deck.ac_rc_lowpass()
R, Cap, T = 1000.0, 1e-6, NC.T_DEFAULT
w = np.logspace(0.0, 7.0, 141)
e, o, psd, c = parity(d, 1, -1, w, what="lowpass")
cf = 4.0 * NC.K_B * T * R / (1.0 + (w * R * Cap) ** 2)
# the bound of the parity test, on the closed form: one source between rows 0 and 1, y_1 - y_0 = R / (1 + j omega R C)
y1 = 1.0 / (1.0 / R + 1j * w * Cap)
d_abs = R / np.sqrt(1.0 + (w * R * Cap) ** 2)
bound = 4.0 * NC.K_B * T / R * ((d_abs + (1e-9 + 1e-6 * np.abs(y1)) + 1e-9) ** 2 - d_abs ** 2) + 1e-6 * cf
print("closed form: worst |d| / bound =", float(np.max(np.abs(psd[:, 0] - cf) / bound)))
assert np.all(np.abs(psd[:, 0] - cf) <= bound)
f = w / (2.0 * np.pi)
trap = getattr(np, "trapezoid", None) or np.trapz
integ = e.noise_integrated()
assert integ.shape == (1,) and abs(integ[0] - trap(psd[:, 0], f)) <= 1e-14 * integ[0], (integ, trap(psd[:, 0], f))
ktc = NC.K_B * T / Cap
quad = trap(cf, f) / ktc                              # the trapezoid of the closed form over these points, in units of kT/C
print("trapezoid of the closed form / (kT/C) =", quad, " integral / (kT/C) =", integ[0] / ktc)
assert abs(quad - 1.0015) < 1e-4, quad
# against kT/C: the quadrature error of these points + the integral of the per-point bound
assert abs(integ[0] - ktc) <= abs(quad - 1.0) * ktc + trap(bound, f), (integ[0], ktc)
assert abs(integ[0] - trap(cf, f)) <= trap(bound, f)
# another temperature scales a thermal circuit linearly
psd2, _, _, _ = e.analyze_noise(w, 1, -1, temp_k=2.0 * T)
assert np.all(np.abs(psd2 - 2.0 * psd) <= 1e-15 * psd2)

dv = pe.deck.Deck()
dv.n_nodes = 2
dv.add("VDC", (1, 0), 1.0)
dv.add("R", (1, 2), 3000.0)
dv.add("R", (2, 0), 1500.0)
e2 = engine(dv)
psd, _, status, st = e2.analyze_noise([0.0, 1e3, 1e6], 1, -1)
want = 4.0 * NC.K_B * T * 1000.0                      # 3k || 1.5k
# both sources see y_1 = 1000 against a row that reads 0 (the source node, ground): relative bound 2 (e_1 + e_0) / y_1 + 1e-6
tol = 2.0 * ((1e-9 + 1e-6 * 1000.0) + 1e-9) / 1000.0 + 1e-6 + 1e-12
print("divider: worst relative error", float(np.max(np.abs(psd[:, 0] - want) / want)), "bound", tol)
assert list(status) == [0, 0, 0] and np.all(np.abs(psd[:, 0] - want) <= tol * want), (psd, want)
''')


@pytest.mark.parametrize("case", ["ac_rlc_diode", "ac_nmos_amp", "ac_linear_mix", "ac_linear_mix_branch", "ac_linear_mix_differential",
                                  "bjt_common_emitter_npn", "bjt_common_emitter_pnp", "bjt_amp_tr"])
def test_parity_with_contributions(emu, case):
    body = {
        "ac_rlc_diode": 'parity(pe.deck.ac_rlc_diode(), 1, -1, np.logspace(2.0, 7.0, 26), what="rlc_diode")',
        "ac_nmos_amp": 'parity(pe.deck.ac_nmos_amp(), 4, -1, np.logspace(1.0, 8.0, 29), what="nmos_amp")',
        "ac_linear_mix": 'parity(pe.deck.ac_linear_mix(), 7, -1, np.logspace(2.0, 7.0, 21), what="linear_mix")',
        # row 8 + 4: the branch of the transformer's secondary (branches: KL 0 1, VCVS 2, XFMR 3 4, SW 5, SW 6) -- a current output
        "ac_linear_mix_branch": 'parity(pe.deck.ac_linear_mix(), 8 + 4, -1, np.logspace(2.0, 7.0, 21), what="linear_mix branch row")',
        "ac_linear_mix_differential": 'parity(pe.deck.ac_linear_mix(), 6, 2, np.logspace(2.0, 7.0, 21), what="linear_mix differential")',
        "bjt_common_emitter_npn": 'parity(pe.deck.bjt_common_emitter(False), 2, -1, np.logspace(2.0, 7.0, 11), warm=[5.0, 0.69, 0.7, 0.0], '
                                  'bjt=lambda o: [((o.x[0] - o.x[1]) / 1e5, (o.x[0] - o.x[2]) / 1e3)], what="npn")',
        "bjt_common_emitter_pnp": 'parity(pe.deck.bjt_common_emitter(True), 2, -1, np.logspace(2.0, 7.0, 11), warm=[-5.0, -0.69, -0.7, 0.0], '
                                  'bjt=lambda o: [((o.x[0] - o.x[1]) / 1e5, (o.x[0] - o.x[2]) / 1e3)], what="pnp")',
        # base fed by 470 k, collector by 2.2 k (the capacitors carry no current at the operating point)
        "bjt_amp_tr": 'd = pe.deck.bjt_amp_tr()\n'
                      'parity(d, 4, -1, np.logspace(2.0, 7.0, 11), warm=[9.0, 0.68, 4.0] + [0.0] * (O.Oracle(d).rows - 3), '
                      'bjt=lambda o: [((o.x[0] - o.x[1]) / 4.7e5, (o.x[0] - o.x[2]) / 2.2e3)], what="bjt_amp")',
    }[case]
    run(emu, body + "\n")


def test_bjt_cold_start_carries_the_failure(emu):
    """the cold-start operating point of the BJT decks fails like the reference's (the project pins that): a noise call on that state is
    refused or carries the failure -- it does not return numbers"""
    run(emu, r'''
d = pe.deck.bjt_common_emitter(False)
e = F.Engine()
e.set_options(g_min=0.0)
e.load_deck(d)
e.reset()
st = e.analyze_dc(F.MODE_OP, check=False)
assert st["rc"] != 0, "the cold start is expected to fail"
psd, c, status, ns = e.analyze_noise(np.logspace(2.0, 7.0, 6), 2, -1, check=False)
print(ns, list(status))
assert ns["rc"] == st["rc"] and list(status) == [st["rc"]] * 6 and np.all(np.isnan(psd)), (ns, psd)
# no densities were formed either: the getter reads NaN, not memory of an earlier call (or none)
S = e.noise_source_density()
assert S.shape == (1, ns["n_sources"]) and ns["n_sources"] == 4 and np.all(np.isnan(S)), S
''')


def test_biased_mesh_batch_of_three(emu):
    """12 x 12 diode mesh with a bias current into its centre: 282 sources (no multiple of 64), three instances with their own R and C,
    each against its own oracle"""
    run(emu, r'''
seeds = [1, 2, 3]
base, r, c = pe.deck.rc_mesh_params(12, 12, seeds, True)
e = engine(mesh(1), batch=3, overrides={"R": r[:, :, None], "C": c[:, :, None]})
psd, con, status, st = e.analyze_noise(MESH_W, 77, 5, contributions=True)
assert list(status) == [0] * len(MESH_W) and st["n_retried_points"] == 0 and st["n_sources"] == 282, st
assert st["n_analyses"] == NC.bands(MESH_W), st
S = e.noise_source_density()
for b, s in enumerate(seeds):
    o, it = oracle(mesh(s))
    cur = o.dio.geq * o._dio_vd() + o.dio.Ieq
    assert it > 0 and int(np.sum(np.abs(cur) > 1e-7)) >= 10, (it, cur)       # the shot-noise path cannot pass vacuously
    src = NC.sources(o)
    assert np.all(np.abs(S[b] - src[2]) <= 1e-6 * src[2])
    NC.check(psd[:, b], con[:, b, :], NC.reference(o, MESH_W, 77, 5, src), "mesh seed %d" % s)
assert not np.array_equal(psd[:, 0], psd[:, 1])
''')


def test_after_a_transient(emu):
    """the last stamp of a transient folds the diffusion-capacitance companion into the junction's slots: only the conduction current of
    the oracle's geq / Ieq after the same steps is a shot-noise current"""
    run(emu, r'''
d = pe.deck.ac_rlc_diode()
o = O.Oracle(d, g_min=0.0)
o.analyze_tr(1e-6, 5)                                 # from the zero state: the junction is still charging after five steps
e = engine(d, op=False)
e.analyze_tr(1e-6, 5)
src = NC.sources(o)
w = np.logspace(2.0, 7.0, 11)
psd, c, status, st = e.analyze_noise(w, 1, -1, contributions=True)
assert list(status) == [0] * len(w) and st["n_retried_points"] == 0, st
S = e.noise_source_density()[0]
print("densities", S, src[2])
assert np.all(np.abs(S - src[2]) <= 1e-6 * src[2])
# the companion is there, and not small: with it left in, the junction's current would be off by more than the tolerance
cur = o.dio.geq * o._dio_vd() + o.dio.Ieq
assert o.dio.tr_prev_g[0] > 0.0 and abs(o.dio.tr_prev_g[0] * o._dio_vd()[0] + o.dio.tr_hist[0]) > 1e-3 * abs(cur[0]), (o.dio.tr_prev_g, o.dio.tr_hist, cur)
NC.check(psd[:, 0], c[:, 0, :], NC.reference(o, w, 1, -1, src), "after a transient")
''')


def test_structure(emu):
    run(emu, r'''
rng = np.random.default_rng(5)
idx = rng.permutation(len(MESH_W))
idx = np.concatenate([idx, idx[3:4]])                 # one duplicate
w = MESH_W[idx]
res = {}
for P in (1, 4, 0):
    e = engine(mesh(1), knobs={"AC_SWEEP_POINTS": P})
    psd, con, status, st = e.analyze_noise(w, 77, 5, contributions=True)
    assert list(status) == [0] * len(w) and st["n_retried_points"] == 0 and st["n_analyses"] == NC.bands(w), (P, st)
    assert (st["points_per_pass"] == P and st["n_passes"] > st["n_analyses"]) if P == 1 else st["points_per_pass"] > 1, (P, st)
    res[P] = (psd, con, e.noise_integrated())
    psd0, none, _, st0 = e.analyze_noise(w, 77, 5)
    assert none is None and np.array_equal(psd0, psd), "the totals do not depend on whether the contributions are kept"
for P in (1, 4):
    for a, b in zip(res[P], res[0]):
        assert np.array_equal(a, b), "pass size %d: bit-identical densities, contributions and integral" % P
psd, con, integ = res[0]
assert np.array_equal(psd[-1], psd[3]) and np.array_equal(con[-1], con[3]), "the duplicate point reads the same bits"
assert np.all(np.abs(con.sum(axis=2) - psd) <= 1e-13 * psd), float(np.max(np.abs(con.sum(axis=2) - psd) / psd))
# the caller's order: the sorted call gives the same bits per point, and the same integral
e = engine(mesh(1))
ps, cs, _, _ = e.analyze_noise(MESH_W, 77, 5, contributions=True)
assert np.array_equal(ps[idx], psd) and np.array_equal(cs[idx], con) and np.array_equal(e.noise_integrated(), integ)
# two instances of the same circuit in one batch read the same bits as one
e = engine(mesh(1), batch=2)
p2, c2, _, _ = e.analyze_noise(MESH_W, 77, 5, contributions=True)
assert np.array_equal(p2[:, 0], ps[:, 0]) and np.array_equal(p2[:, 1], ps[:, 0]) and np.array_equal(c2[:, 1], cs[:, 0])
# a slice through the C ABI
lib = F.lib()
out = np.empty((3, 1)); oc = np.empty((3, 1, 282))
assert lib.pe_hip_get_noise(e._h, 2, 3, 1, 1, F._dp(out), F._dp(oc)) == 0
assert np.array_equal(out, p2[2:5, 1:2]) and np.array_equal(oc, c2[2:5, 1:2])
assert lib.pe_hip_get_noise(e._h, 8, 3, 0, 1, F._dp(out), None) == F.ERR_ARG
''')


def test_points_that_fail(emu):
    """VAC - R - C - C (the deck of test_ac_sweep_emu.test_points_that_fail_in_their_batch), output = the node between the capacitors:
    singular at omega = 0 -- those points are retried alone, carry PE_HIP_ERR_SINGULAR and read NaN, the others agree with the oracle,
    the integral is NaN"""
    run(emu, r'''
d = pe.deck.Deck()
d.n_nodes = 3
d.add("VAC", (1, 0), 1.0, 1000.0, 0.0)
d.add("R", (1, 2), 1000.0)
d.add("C", (2, 3), 1e-6)
d.add("C", (3, 0), 2e-6)
w = np.array([0.0, 1e3, 0.0, 2e3, 1e5])
good = [1, 3, 4]
o, _ = oracle(d)
src = NC.sources(o)
ref = NC.reference(o, w[good], 2, -1, src)
for P in (4, 0, 1):
    e = engine(d, knobs={"AC_SWEEP_POINTS": P})
    psd, c, status, st = e.analyze_noise(w, 2, -1, contributions=True, check=False)
    assert st["rc"] == F.ERR_SINGULAR and list(status) == [F.ERR_SINGULAR, 0, F.ERR_SINGULAR, 0, 0], (P, st, status)
    assert st["n_retried_points"] == 2, (P, st)
    assert np.all(np.isnan(psd[[0, 2]])) and np.all(np.isnan(c[[0, 2]])), "a failed point reads NaN"
    NC.check(psd[good, 0], c[good, 0, :], ref, "P = %d" % P)
    assert np.all(np.isnan(e.noise_integrated()))
    psd2, _, status2, st2 = e.analyze_noise(w[good], 2, -1)          # and the engine goes on
    assert list(status2) == [0, 0, 0] and st2["n_retried_points"] == 0 and np.array_equal(psd2, psd[good])
    assert np.all(np.isfinite(e.noise_integrated()))
''')


def test_refusals_invalidation_and_the_forward_sweep(emu):
    run(emu, r'''
lib = F.lib()
e = engine(mesh(1))
w = MESH_W[:6]
# a stored forward sweep reads the same bits after a noise call
e.set_ac_sweep_rows([0, 77, 144])
x, _, _ = e.analyze_ac_sweep(w)
psd, _, status, st = e.analyze_noise(w, 77, 5)
re = np.empty((len(w), 1, 3)); im = np.empty_like(re)
assert lib.pe_hip_get_ac_sweep(e._h, 0, len(w), 0, 1, F._dp(re), F._dp(im)) == 0
assert np.array_equal(re + 1j * im, x), "the forward sweep's stored result"
x2, _, _ = e.analyze_ac_sweep(w)
assert np.array_equal(x2, x), "... and the forward sweep itself"
out = np.empty((len(w), 1))
assert lib.pe_hip_get_noise(e._h, 0, len(w), 0, 1, F._dp(out), None) == 0 and np.array_equal(out, psd), "and the other way round"
# bad arguments: refused, and a following call returns what it returned before
stn = F.NoiseStats()
def call(ws, pos, neg, ctl=True):
    ws = np.ascontiguousarray(ws, dtype=float)
    c = F.NoiseControl(pos, neg, 0.0, 0)
    return lib.pe_hip_analyze_noise(e._h, len(ws), F._dp(ws), C.byref(c) if ctl else None, None, C.byref(stn))
n = e.rows
for pos, neg in ((n, -1), (-2, 0), (0, n), (3, 3), (-1, -1)):
    assert call(w, pos, neg) == F.ERR_ARG, (pos, neg)
for bad in (-1.0, float("nan"), float("inf")):
    assert call([1e8, bad], 77, 5) == F.ERR_ARG, bad
assert call(w, 77, 5, ctl=False) == F.ERR_ARG
assert lib.pe_hip_analyze_noise(e._h, 0, F._dp(w), C.byref(F.NoiseControl(77, 5, 0.0, 0)), None, None) == F.ERR_ARG
assert lib.pe_hip_analyze_noise(e._h, 2, None, C.byref(F.NoiseControl(77, 5, 0.0, 0)), None, None) == F.ERR_ARG
assert lib.pe_hip_get_noise(e._h, 0, len(w), 0, 1, F._dp(out), None) == 0 and np.array_equal(out, psd), "the stored result survives a refused call"
psd2, _, _, _ = e.analyze_noise(w, 77, 5)
assert np.array_equal(psd2, psd)
# another output pair on the same engine: only the right-hand side changes; and back
o, _ = oracle(mesh(1))
src = NC.sources(o)
psd3, c3, _, st3 = e.analyze_noise(w, 20, -1, contributions=True)
NC.check(psd3[:, 0], c3[:, 0, :], NC.reference(o, w, 20, -1, src), "second output pair")
psd4, _, _, _ = e.analyze_noise(w, 77, 5)
assert np.array_equal(psd4, psd)
# what makes a stored AC sweep unreadable makes the noise result unreadable
get = lambda: lib.pe_hip_get_noise(e._h, 0, len(w), 0, 1, F._dp(out), None)
for name in ("analyze_dc", "analyze_tr", "reset", "set_solution", "checkpoint_load", "update_param", "load_deck"):
    e.analyze_noise(w, 77, 5)
    assert get() == 0, name
    if name == "analyze_dc": e.analyze_dc(F.MODE_OP)
    elif name == "analyze_tr": e.analyze_tr(1e-10, 1)
    elif name == "reset": e.reset()
    elif name == "set_solution": e.set_solution(e.solution())
    elif name == "checkpoint_load": e.restore(e.checkpoint())
    elif name == "update_param": e.update_param(F.R, 0, 0, 1234.0)
    else: e.load_deck(mesh(1), 1)
    assert get() == F.ERR_ARG and b"no noise analysis yet" in lib.pe_hip_last_error(e._h), name
    v = np.empty(1)
    assert lib.pe_hip_get_noise_integrated(e._h, 0, 1, F._dp(v)) == F.ERR_ARG, name
    if name in ("reset", "load_deck"):
        e.reset(); e.analyze_dc(F.MODE_OP)
# update_param is seen by the next call: the first resistor's density follows its new value
e.update_param(F.R, 0, 0, 500.0)
e.analyze_dc(F.MODE_OP)
e.analyze_noise(w, 77, 5)
assert abs(e.noise_source_density()[0, 0] - 4.0 * NC.K_B * NC.T_DEFAULT / 500.0) <= 1e-15 * 4.0 * NC.K_B * NC.T_DEFAULT / 500.0
# without a circuit
f = F.Engine()
assert lib.pe_hip_analyze_noise(f._h, len(w), F._dp(w), C.byref(F.NoiseControl(0, -1, 0.0, 0)), None, None) == F.ERR_ARG
f.close()

# a circuit with a host-stamp overlay has no noise description
FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
def hook(user, event, mode, t, dt, x, a, b):
    if event == 1:
        a[0] = 1e-3; b[0] = 0.0
    elif event == 3:
        a[0] = 1e-3; a[1] = 0.0; b[0] = b[1] = 0.0
    return 0
cb = FN(hook)
lib.pe_hip_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_int, FN, C.c_void_p]
one = np.array([1], dtype=np.int32); rep = np.array([1e-3])
g = F.Engine()
assert lib.pe_hip_set_overlay(g._h, 1, F._ip(one), F._ip(one), F._dp(rep), 1, F._ip(one), 0, cb, None) == 0
g.set_options(g_min=1e-12)
g.load(2, 1, [(F.VDC, np.array([[1, 0]], dtype=np.int32), np.array([0], dtype=np.int32), np.array([[3.0]]), 0),
              (F.R, np.array([[1, 2]], dtype=np.int32), None, np.array([[1500.0]]), 0)])
g.analyze_dc(F.MODE_DC)
assert lib.pe_hip_analyze_noise(g._h, len(w), F._dp(w), C.byref(F.NoiseControl(1, -1, 0.0, 0)), None, None) == F.ERR_ARG
assert b"overlay" in lib.pe_hip_last_error(g._h)
''')


def test_source_table(emu):
    """definition order for a deck with R, D, FBR, NMOS, NPN: resistors, junctions (the rectifier's four in place), three-pin devices;
    a device with an unconnected pin (resistor, MOSFET, BJT) is enumerated with no rows and contributes nothing"""
    run(emu, r'''
d = pe.deck.Deck()
d.n_nodes = 7
d.add("VDC", (1, 0), 5.0)
d.add("NPN", (4, 5, 0), 1e-16, 1.0, 100.0, 27.0, 1.0)
d.add("R", (1, 2), 1e3)
d.add("D", (2, 3))
d.add("FBR", (3, 0, 6, 7))
d.add("R", (6, 7), 2e3)
d.add("NMOS", (5, 3, 0), 2e-3, 0.02, 1.0)
d.add("R", (1, 4), 1e5)
d.add("R", (1, 5), 1e3)
d.add("D", (7, 0))
d.add("R", (3, 0), 1e4)
e = F.Engine()
e.set_options(g_min=1e-12)
e.load_deck(d)
t = e.noise_sources()
kinds = [F.R] * 5 + [F.DIODE] * 6 + [F.NMOS, F.BJT_NPN, F.BJT_NPN]
assert list(t["kind"]) == kinds, t
assert list(t["index"]) == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 0, 0, 0], t
assert list(t["part"]) == [0] * 13 + [1], t
rows = list(zip(t["row_a"].tolist(), t["row_b"].tolist()))
assert rows[:5] == [(0, 1), (5, 6), (0, 3), (0, 4), (2, -1)], rows
assert rows[5:11] == [(1, 2), (2, 5), (-1, 5), (6, 2), (6, -1), (6, -1)], rows      # D; FBR: A->+, B->+, - ->A, - ->B; D
assert rows[11:] == [(4, -1), (3, -1), (4, -1)], rows                                # NMOS D-S; NPN B-E, C-E
# an unconnected pin: enumerated, no rows, S = 0
d2 = pe.deck.ac_rc_lowpass()
d2.add("R", (2, -1), 100.0)
e2 = engine(d2)
t2 = e2.noise_sources()
assert list(t2["kind"]) == [F.R, F.R] and list(t2["index"]) == [0, 1] and (t2["row_a"][1], t2["row_b"][1]) == (-1, -1), t2
psd, c, _, _ = e2.analyze_noise([1e3], 1, -1, contributions=True)
assert e2.noise_source_density()[0, 1] == 0.0 and c[0, 0, 1] == 0.0 and psd[0, 0] == c[0, 0, 0]
# three-pin devices with an unconnected pin keep their place in their table: a MOSFET one entry, a BJT two, no rows, S = 0
d3 = pe.deck.ac_nmos_amp()
n_before = len(engine(d3).noise_sources()["kind"])
d3.add("NMOS", (1, -1, 0), 2e-3, 0.02, 1.0)
d3.add("NPN", (-1, 1, 0), 1e-16, 1.0, 100.0, 27.0, 1.0)
d3.add("NPN", (1, 2, -1), 1e-16, 1.0, 100.0, 27.0, 1.0)
e3 = engine(d3)
t3 = e3.noise_sources()
assert len(t3["kind"]) == n_before + 5, t3
assert list(t3["kind"][-6:]) == [F.NMOS, F.NMOS] + [F.BJT_NPN] * 4 and list(t3["index"][-6:]) == [0, 1, 0, 0, 1, 1], t3
assert list(t3["part"][-6:]) == [0, 0, 0, 1, 0, 1], t3
assert all((a, b) == (-1, -1) for a, b in zip(t3["row_a"][-5:].tolist(), t3["row_b"][-5:].tolist())), t3
w3 = np.logspace(1.0, 8.0, 8)
psd3, c3, _, _ = e3.analyze_noise(w3, 4, -1, contributions=True)
psd0, c0, _, _ = engine(pe.deck.ac_nmos_amp()).analyze_noise(w3, 4, -1, contributions=True)
assert np.all(e3.noise_source_density()[0, -5:] == 0.0) and np.all(c3[:, :, -5:] == 0.0)
assert np.array_equal(psd3, psd0) and np.array_equal(c3[:, :, :-5], c0), "devices that stamp nothing change nothing"
''')


def test_plugin_api_under_host_emulation(emu):
    """tests/cpp/noise_rc.cpp: circult::analyze_noise of the plug-in API on an R - C low pass: closed form per point and kT/C"""
    make("-C", CPP, "_build_emu/noise_rc")
    out = subprocess.run([os.path.join(CPP, "_build_emu", "noise_rc")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"noise_rc exited {out.returncode}: {out.stderr}"
