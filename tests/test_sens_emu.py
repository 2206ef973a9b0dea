"""DC sensitivity analysis (pe_hip_analyze_sens / pe_hip_get_sens*, include/pe_hip.h) on the CPU: the engine's host logic and the
team-generic kernel text (pe_sens.hpp) through the host emulation library (tests/emu: test infrastructure), one child process per case.
Reference, tolerance and the case list: tests/sens_common.py (the unchanged CPU oracle set to the engine's own solution, direct method and
transposed solve; the project's AC tolerance propagated through d f / d p).  No case but the one about failing outputs may lean on a
retried output: each asserts n_retried_outputs == 0."""
import os
import subprocess
import sys

import pytest

from parity_common import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpe_hip_emu.so")
CPP = os.path.join(ROOT, "tests", "cpp")

CASES = ["diode_op", "diode_recombination", "diode_breakdown", "diode_linear_arm", "nmos_cutoff", "pmos_cutoff", "nmos_saturation", "pmos_saturation",
         "nmos_triode", "pmos_triode", "bjt_npn", "bjt_pnp", "controlled_mix_op", "controlled_mix_trop", "controlled_mix_biased", "ac_controlled_rest",
         "ccvs_dc", "cccs_dc", "vccs_dc", "vcvs_gain", "op_amp_follower", "transformer_ratio", "center_tap_ratio", "bridge_rectifier", "op_amp_low_gain",
         "unconnected_pins", "mesh12"]


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
import sens_common as SC
TEAM = 1                                              # the builds without HIP run the kernel text with a one-thread team
''' % (ROOT, ROOT)


def run(emu, body, **env):
    e = dict(os.environ, PE_HIP_LIB=emu, **env)
    e.pop("PHY_ENGINE_HIP_SENS_OUTPUTS", None)
    e.pop("PHY_ENGINE_HIP_AC_SWEEP_POINTS", None)
    r = subprocess.run([sys.executable, "-c", PRE + body], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_case_list_matches_the_reference_module():
    sys.path.insert(0, ROOT)
    import pe_load
    import sens_common as SC
    assert list(SC.cases(pe_load.load())) == CASES


@pytest.mark.parametrize("case", CASES)
def test_parity_with_every_sensitivity_kept(emu, case):
    run(emu, "SC.run_case(pe, O, %r)\n" % case)


def test_every_column_is_exercised_and_restated_derivatives_hold(emu):
    """(a) every (kind, column) of the table has, in at least one parity case, an output with |s_k| >= 1000 bound_k (at the oracle's own
    converged solution: no engine involved); (b) on the small decks every column of the restated d f / d p is compared with central
    differences of fully re-converged oracle solves (SC.fd_check), and every (kind, column) is checked by one of them.
    Two arms of the models stamp a conductance that is not the slope of the current they stamp (SC.slope_correction): a PMOS (gds and gm
    with the opposite sign) and a junction on the linear continuation of the limited exponential.  The analysis is defined on the stamped
    matrix, so there it does not give the derivative of the converged output -- measured on pmos_saturation: d v_D / d R_load 1.1018e-3
    against the difference quotient's 1.0170e-3, d v_D / d V_gate +4.068 against -4.068; on diode_linear_arm d v / d R -2.54e-5 against
    -6.21e-5.  On those two decks the difference quotients (of solves iterated until the linearly converging iteration stands) are
    compared with the reference on the slope-corrected matrix: that checks the restated d f / d p of the PMOS columns and of the linear
    arm, and pins the cause.  pmos_triode has no difference quotient: Newton's iteration moves away from that fixed point."""
    run(emu, r'''
ex = set()
for name, (deck, warm, mode) in SC.cases(pe).items():
    warm = warm() if callable(warm) else warm
    x = SC.oracle_solution(O, deck, mode, warm)
    ex |= SC.exercised(SC.reference(F, O, deck, x, mode, SC.outputs_of(deck)))
assert ex == SC.all_pairs(F), sorted(SC.all_pairs(F) - ex)
checked = set()
for name in ("diode_op", "diode_recombination", "diode_breakdown", "nmos_saturation", "nmos_triode", "bjt_npn", "bjt_pnp", "controlled_mix_biased",
             "ccvs_dc", "cccs_dc", "vccs_dc", "vcvs_gain", "transformer_ratio", "op_amp_low_gain", "center_tap_ratio"):
    deck, warm, mode = SC.cases(pe)[name]
    warm = warm() if callable(warm) else warm
    got, _ = SC.fd_check(F, O, deck, mode, SC.outputs_of(deck), warm, what=name)
    checked |= got
assert checked == SC.all_pairs(F) - {(F.PMOS, c) for c in range(3)}, sorted(SC.all_pairs(F) - checked)
for name, polish, need in (("pmos_saturation", 40, {(F.PMOS, c) for c in range(3)}), ("diode_linear_arm", 150, {(F.DIODE, c) for c in (0, 1, 4, 8)})):
    deck, warm, mode = SC.cases(pe)[name]
    warm = warm() if callable(warm) else warm
    got, ref = SC.fd_check(F, O, deck, mode, SC.outputs_of(deck), warm, what=name + " (slope-corrected matrix)", slopes=True, polish=polish)
    assert need <= got, (name, sorted(got))
    assert ("D linear" in ref["arms"]) == (name == "diode_linear_arm")
    checked |= got
print("not checked by a difference quotient:", sorted(SC.all_pairs(F) - checked))
assert checked == SC.all_pairs(F), sorted(SC.all_pairs(F) - checked)
''')


def test_several_outputs_in_one_call(emu):
    """5 outputs with SENS_OUTPUTS 1, 2 and automatic: s and rss bit-identical across the three, each output equal to its single-output
    call bit for bit, n_passes as expected, one analysis"""
    run(emu, r'''
deck = SC.mesh(pe, 12, 1)
outs = [(77, -1), (5, 77), (144, -1), (20, 100), (-1, 3)]
pos, neg = [p for p, _ in outs], [n for _, n in outs]
w = 1.0 + 0.01 * np.arange(402)
res = {}
for P, passes in ((1, 5), (2, 3), (0, 1)):
    e = SC.engine(pe, deck, knobs={"SENS_OUTPUTS": P})
    s, rss, status, st = e.analyze_sens(pos, neg, weight=w)
    assert list(status) == [0] * 5 and st["n_retried_outputs"] == 0 and st["n_analyses"] == 1 and st["n_params"] == 402, (P, st)
    assert st["n_passes"] == passes and st["outputs_per_pass"] == (P if P else 5), (P, st)
    res[P] = (s, rss)
    if P == 2:
        for o in range(5):
            s1, r1, _, st1 = e.analyze_sens([pos[o]], [neg[o]], weight=w)
            assert st1["n_passes"] == 1 and np.array_equal(s1[0], s[o]) and np.array_equal(r1[0], rss[o]), o
for P in (1, 2):
    assert np.array_equal(res[P][0], res[0][0]) and np.array_equal(res[P][1], res[0][1]), P
# a slice through the C ABI
lib = F.lib()
s, rss = res[0]
out = np.empty((2, 1, 402)); orss = np.empty((2, 1))
assert lib.pe_hip_get_sens(e._h, 1, 2, 0, 1, F._dp(out), F._dp(orss)) == 0
assert np.array_equal(out, s[1:3]) and np.array_equal(orss, rss[1:3])
assert lib.pe_hip_get_sens(e._h, 4, 2, 0, 1, F._dp(out), None) == F.ERR_ARG and lib.pe_hip_get_sens(e._h, 0, 1, 1, 1, F._dp(out), None) == F.ERR_ARG
''')


def test_batch_of_three_equals_its_single_runs(emu):
    """batch 3 of the 12 x 12 mesh with per-instance R and C: each instance against its own reference, and equal to its batch-1 run bit for
    bit"""
    run(emu, r'''
seeds = [1, 2, 3]
base, r, c = pe.deck.rc_mesh_params(12, 12, seeds, True)
outs = [(77, -1), (5, 77)]
e = SC.engine(pe, SC.mesh(pe, 12, 1), batch=3, overrides={"R": r[:, :, None], "C": c[:, :, None]})
s, _, status, st = e.analyze_sens([77, 5], [-1, 77])
assert list(status) == [0, 0] and st["n_retried_outputs"] == 0 and st["n_analyses"] == 1, st
x = e.solution()
for b, seed in enumerate(seeds):
    SC.check(s[:, b, :], SC.reference(F, O, SC.mesh(pe, 12, seed), x[b], "OP", outs), "mesh seed %d" % seed)
    e1 = SC.engine(pe, SC.mesh(pe, 12, seed))
    s1, _, _, _ = e1.analyze_sens([77, 5], [-1, 77])
    assert np.array_equal(e1.solution()[0], x[b]), "the operating point of the single run"
    assert np.array_equal(s1[:, 0, :], s[:, b, :]), "instance %d equals its batch-1 run" % b
assert not np.array_equal(s[:, 0], s[:, 1])
''')


def test_more_than_one_reduction_chunk(emu):
    """rc_mesh(32, 32, nonlinear) with the bias current: 3 010 parameters against the 2 048 of a reduction chunk -- two chunks, the second
    with a ragged tail (962 = 3 x 256 + 194).  Batch 2, one output, against the reference; rss against the sum in the documented order"""
    run(emu, r'''
seeds = [1, 2]
base, r, c = pe.deck.rc_mesh_params(32, 32, seeds, True)
e = SC.engine(pe, SC.mesh(pe, 32, 1), batch=2, overrides={"R": r[:, :, None], "C": c[:, :, None]})
n = len(e.sens_params()["kind"])
assert n == 3010, n
w = 1.0 + (np.arange(n) % 7)
s, rss, status, st = e.analyze_sens([500], [-1], weight=w)
assert list(status) == [0] and st["n_retried_outputs"] == 0 and st["n_params"] == n, st
x = e.solution()
for b, seed in enumerate(seeds):
    r_, b_ = SC.check(s[:, b, :], SC.reference(F, O, SC.mesh(pe, 32, seed), x[b], "OP", [(500, -1)]), "mesh32 seed %d" % seed)
    want, bound = SC.rss_reference(r_, b_, w)
    assert abs(rss[0, b] - want[0]) <= bound[0], (rss[0, b], want, bound)
    assert rss[0, b] == SC.rss_in_order(s[0, b], w, TEAM), (rss[0, b], SC.rss_in_order(s[0, b], w, TEAM))
_, rss0, _, _ = e.analyze_sens([500], [-1], weight=w, keep=False)
assert np.array_equal(rss0, rss)
''')


def test_normalized_weight_and_rss_only(emu):
    """normalized = 1 multiplies by the parameter (a zero-valued one reads 0: Isr of the default junction); rss is the same bits with and
    without keeping, equals the sum in the documented order, and agrees with the reference within the propagated bound"""
    run(emu, r'''
deck, warm, mode = SC.cases(pe)["diode_op"]
outs = SC.outputs_of(deck)
pos, neg = [p for p, _ in outs], [n for _, n in outs]
e = SC.engine(pe, deck)
ref = SC.reference(F, O, deck, e.solution()[0], "OP", outs)
s, none, _, _ = e.analyze_sens(pos, neg)
sn, none2, _, _ = e.analyze_sens(pos, neg, normalized=True)
assert none is None and none2 is None
r_, b_ = SC.check(sn[:, 0, :], ref, "normalized", normalized=True)
k_isr = [k for k, t in enumerate(ref["table"]) if t["name"] == "D" and t["column"] == 2][0]
assert ref["p"][k_isr] == 0.0 and np.all(s[:, 0, k_isr] != 0.0) and np.all(sn[:, 0, k_isr] == 0.0)
p = ref["p"].copy(); p[0] = 1.0 / (1.0 / p[0])       # (a resistor's p is the reciprocal of its resident conductance)
assert np.array_equal(sn[:, 0, :], np.where(p == 0.0, 0.0, p * s[:, 0, :]))
w = np.array([0.01, 0.05, 0.1, 0.0, 2.0, 0.3, 0.01, 1.0, 1.0, 0.02])
for norm, (rr, bb) in ((False, (ref["s"], ref["bound"])), (True, (r_, b_))):
    sk, rss, _, st = e.analyze_sens(pos, neg, normalized=norm, weight=w)
    nk, rss2, _, _ = e.analyze_sens(pos, neg, normalized=norm, weight=w, keep=False)
    assert nk is None and np.array_equal(rss, rss2), "the sum does not depend on whether the sensitivities are kept"
    want, bound = SC.rss_reference(rr, bb, w)
    assert np.all(np.abs(rss[:, 0] - want) <= bound), (rss, want, bound)
    for o in range(len(outs)):
        assert rss[o, 0] == SC.rss_in_order(sk[o, 0], w, TEAM), o
lib = F.lib()
out = np.empty((len(outs), 1, 10))
assert lib.pe_hip_get_sens(e._h, 0, len(outs), 0, 1, F._dp(out), None) == F.ERR_ARG and b"not kept" in lib.pe_hip_last_error(e._h)
e.analyze_sens(pos, neg)
assert lib.pe_hip_get_sens(e._h, 0, len(outs), 0, 1, None, F._dp(out)) == F.ERR_ARG and b"no weighted sum" in lib.pe_hip_last_error(e._h)
''')


def test_parameter_table(emu):
    """order and content against the deck (R, VDC, IDC, junctions with the rectifier's four in place, then the generic tables in the order
    they were passed), readable before any analysis, capacity-0-first"""
    run(emu, r'''
d = pe.deck.Deck()
d.n_nodes = 9
d.add("VDC", (1, 0), 5.0)
d.add("NPN", (4, 5, 0), 1e-16, 1.0, 100.0, 27.0, 1.0)
d.add("R", (1, 2), 1e3)
d.add("D", (2, 3))
d.add("FBR", (3, 0, 6, 7))
d.add("R", (6, 7), 2e3)
d.add("NMOS", (5, 3, 0), 2e-3, 0.02, 1.0)
d.add("R", (1, -1), 1e5)
d.add("IDC", (0, 5), 1e-3)
d.add("D", (7, -1))
d.add("XCT", (1, 0, 8, 0, 9), 2.0)
d.add("VCCS", (8, 0, 9, 0), 1e-3)
d.add("PMOS", (5, -1, 1), 2e-3, 0.02, 1.0)
d.add("C", (8, 0), 1e-9)
e = F.Engine()
e.set_options(g_min=1e-12)
e.load_deck(d)
lib = F.lib()
n = C.c_int()
assert lib.pe_hip_get_sens_params(e._h, 0, None, None, None, C.byref(n)) == 0 and n.value == 3 + 1 + 1 + 6 * 8 + 1 + 3 + 3 + 5 + 1, n.value
kind = np.full(4, -7, dtype=np.int32)
assert lib.pe_hip_get_sens_params(e._h, 3, F._ip(kind), None, None, C.byref(n)) == 0 and list(kind) == [F.R, F.R, F.R, -7]
got = SC.table_of(e)
want = [(F.R, 0, 0), (F.R, 1, 0), (F.R, 2, 0), (F.VDC, 0, 0), (F.IDC, 0, 0)]
want += [(F.DIODE, i, c) for i in range(6) for c in SC.DIODE_COLS]
want += [(F.VCCS, 0, 0)] + [(F.NMOS, 0, c) for c in range(3)] + [(F.PMOS, 0, c) for c in range(3)] + [(F.BJT_NPN, 0, c) for c in range(5)] + [(F.XFMR_CT, 0, 0)]
assert got == want, got
assert got == [(t["kind"], t["index"], t["column"]) for t in SC.parameter_table(F, d)]
f = F.Engine()
assert lib.pe_hip_get_sens_params(f._h, 0, None, None, None, C.byref(n)) == F.ERR_ARG
''')


def test_against_the_update_param_loop_on_the_engine_itself(emu):
    """end to end: central differences of update_param -> analyze_dc -> solution on the engine at h and h / 2 for every parameter of
    diode_op, nmos_common_source and bjt_common_emitter; allowance 2 |FD(h) - FD(h/2)| + bound_k, asserted where it is below 1e-3 |s_k|"""
    run(emu, r'''
# need: the parameters the outputs depend on -- diode_op: R, V, Is, N, Temp, Area (Isr is 0 there: Nr has no effect, and the junction is not
# in breakdown: Ibv, Bv have none); nmos: R, both V, Kp, lambda, Vth; bjt: V, both R, Is, N, BetaF, Temp, Area
for name, need in (("diode_op", 6), ("nmos_saturation", 6), ("bjt_npn", 8)):
    deck, warm, mode = SC.cases(pe)[name]
    outs = SC.outputs_of(deck)
    e, ref, s = SC.parity(pe, O, deck, outs, warm, mode, name)
    x0 = e.solution()
    def out_at(kind, index, column, value):
        e.update_param(kind, index, column, value)
        e.set_solution(x0)
        if e.analyze_dc(F.MODE_OP, check=False)["rc"] != 0:
            return None                               # (a zero saturation current stepped by -1e-6: no operating point, column not checked)
        e.analyze_dc(F.MODE_OP)
        x = e.solution()[0]
        return np.array([(x[p] if p >= 0 else 0.0) - (x[n] if n >= 0 else 0.0) for p, n in outs])
    checked, worst = 0, 0.0
    for k, t in enumerate(ref["table"]):
        fd = []
        for h in (1e-4, 5e-5):
            step = h * abs(t["value"]) if t["value"] != 0.0 else 1e-6 * (h / 1e-4)
            up, dn = out_at(t["kind"], t["index"], t["column"], t["value"] + step), out_at(t["kind"], t["index"], t["column"], t["value"] - step)
            if up is None or dn is None:
                break
            fd.append((up - dn) / (2.0 * step))
        e.update_param(t["kind"], t["index"], t["column"], t["value"])
        hit = False
        for o in range(len(outs) if len(fd) == 2 else 0):
            allow = 2.0 * abs(fd[0][o] - fd[1][o]) + ref["bound"][o][k]
            if allow < 1e-3 * abs(s[o, 0, k]):
                hit = True
                worst = max(worst, abs(s[o, 0, k] - fd[1][o]) / allow)
                assert abs(s[o, 0, k] - fd[1][o]) <= allow, (name, t, o, s[o, 0, k], fd[0][o], fd[1][o], allow)
        checked += hit
    print(name, "columns checked against the engine's own loop:", checked, "of", len(ref["table"]), "worst |d| / allowance =", worst)
    assert checked >= need, (name, checked)
''')


def test_operating_point_semantics(emu):
    """after a TR step of ac_rlc_diode (a junction with a transit time) the diffusion-capacitance companion is taken out: the result is
    that of the oracle's conduction geq at the engine's x; a failed operating point (the cold-start BJT deck) gives its status and NaN"""
    run(emu, r'''
d = pe.deck.ac_rlc_diode()
e = F.Engine(); e.set_options(g_min=0.0, **SC.TIGHT); e.load_deck(d); e.reset()
e.analyze_tr(1e-6, 5)
o = O.Oracle(d, g_min=0.0)
o.analyze_tr(1e-6, 5)
assert o.dio.tr_prev_g[0] > 0.0, "the companion is there"
outs = [(1, -1), (d.n_nodes, -1)]
s, _, status, st = e.analyze_sens([p for p, _ in outs], [n for _, n in outs])
assert list(status) == [0, 0] and st["n_retried_outputs"] == 0, st
# the reference at the engine's x, DC stamp (capacitors open, inductors shorted, conduction geq only); the last linearisation of a
# transient step is one Newton step behind x, which is first order in that step: the step is at the tight tolerance here
ref = SC.reference(F, O, d, e.solution()[0], "OP", outs)
SC.check(s[:, 0, :], ref, "after a transient")
big = np.abs(ref["s"]) >= 1000.0 * ref["bound"]
assert big[:, [k for k, t in enumerate(ref["table"]) if t["name"] == "D"]].any(), "the junction takes part"

d = pe.deck.bjt_common_emitter(False)
e = F.Engine(); e.set_options(g_min=0.0); e.load_deck(d); e.reset()
st = e.analyze_dc(F.MODE_OP, check=False)
assert st["rc"] != 0, "the cold start is expected to fail"
s, rss, status, ss = e.analyze_sens([2, 1], [-1, -1], weight=np.ones(8), check=False)
assert ss["rc"] == st["rc"] and list(status) == [st["rc"]] * 2 and np.all(np.isnan(s)) and np.all(np.isnan(rss)) and ss["n_params"] == 8, (ss, s)
''')


def test_refusals_invalidation_and_the_other_analyses(emu):
    run(emu, r'''
lib = F.lib()
deck = SC.mesh(pe, 12, 1)
e = SC.engine(pe, deck)
w = np.logspace(7.0, 11.5, 6)
pos = np.array([77, 5], dtype=np.int32); neg = np.array([-1, 77], dtype=np.int32)
# stored AC sweep, noise result and DC sweep read the same bits after a sensitivity call, and the other way round
e.set_ac_sweep_rows([0, 77, 144])
xa, _, _ = e.analyze_ac_sweep(w)
psd, _, _, _ = e.analyze_noise(w, 77, 5)
xd, _, _ = e.analyze_dc_sweep([1e-4, 2e-4, 4e-4], F.IDC, 0)
s, rss, status, st = e.analyze_sens(pos, neg, weight=np.ones(402))
re = np.empty((len(w), 1, 3)); im = np.empty_like(re); out = np.empty((len(w), 1)); xo = np.empty_like(xd)
assert lib.pe_hip_get_ac_sweep(e._h, 0, len(w), 0, 1, F._dp(re), F._dp(im)) == 0 and np.array_equal(re + 1j * im, xa)
assert lib.pe_hip_get_noise(e._h, 0, len(w), 0, 1, F._dp(out), None) == 0 and np.array_equal(out, psd)
assert lib.pe_hip_get_dc_sweep(e._h, 0, 3, 0, 1, F._dp(xo)) == 0 and np.array_equal(xo, xd)
xa2, _, _ = e.analyze_ac_sweep(w); psd2, _, _, _ = e.analyze_noise(w, 77, 5); xd2, _, _ = e.analyze_dc_sweep([1e-4, 2e-4, 4e-4], F.IDC, 0)
assert np.array_equal(xa2, xa) and np.array_equal(psd2, psd) and np.array_equal(xd2, xd)
so = np.empty_like(s); ro = np.empty_like(rss)
get = lambda: lib.pe_hip_get_sens(e._h, 0, 2, 0, 1, F._dp(so), F._dp(ro))
assert get() == 0 and np.array_equal(so, s) and np.array_equal(ro, rss), "and the other way round"
s2, rss2, _, _ = e.analyze_sens(pos, neg, weight=np.ones(402))
assert np.array_equal(s2, s) and np.array_equal(rss2, rss)
# the system that was really solved: the transpose of the main engine's matrix in the real block, zeros off it, the slot's selector
rp, ci, va, _ = e.matrix()
N = e.rows
import scipy.sparse as sp
J = sp.csr_matrix((va, ci, rp), shape=(N, N)).toarray()
for q, (p_, n_) in enumerate(zip(pos, neg)):
    rp2, ci2, va2, rhs = e.matrix_ac(4, q)
    A = sp.csr_matrix((va2, ci2, rp2), shape=(2 * N, 2 * N)).toarray()
    assert np.array_equal(A[:N, :N], J.T) and np.array_equal(A[N:, N:], J.T), q
    assert not A[:N, N:].any() and not A[N:, :N].any(), q
    want = np.zeros(2 * N); want[p_] += 1.0
    if n_ >= 0: want[n_] -= 1.0
    assert np.array_equal(rhs, want), q
# refusals: the engine is unchanged and the stored result stays readable
sst = F.SensStats()
wgt = np.ones(402)
def call(n, p, ng, keep=1, weight=None, ctl=True):
    p = None if p is None else np.ascontiguousarray(p, dtype=np.int32); ng = None if ng is None else np.ascontiguousarray(ng, dtype=np.int32)
    c = F.SensControl(n, None if p is None else F._ip(p), None if ng is None else F._ip(ng), 0, keep, None if weight is None else F._dp(weight))
    return lib.pe_hip_analyze_sens(e._h, C.byref(c) if ctl else None, None, C.byref(sst))
assert call(0, [1], [-1]) == F.ERR_ARG and call(-1, [1], [-1]) == F.ERR_ARG
assert call(1, None, [-1]) == F.ERR_ARG and call(1, [1], None) == F.ERR_ARG and call(1, [1], [-1], ctl=False) == F.ERR_ARG
for p_, n_ in ((N, -1), (-2, 0), (0, N), (3, 3), (-1, -1)):
    assert call(2, [1, p_], [-1, n_]) == F.ERR_ARG, (p_, n_)
for bad in (float("nan"), float("inf")):
    wb = wgt.copy(); wb[7] = bad
    assert call(1, [1], [-1], weight=wb) == F.ERR_ARG, bad
assert call(1, [1], [-1], keep=0) == F.ERR_ARG, "nothing asked for"
assert get() == 0 and np.array_equal(so, s) and np.array_equal(ro, rss), "the stored result survives a refused call"
s3, rss3, _, _ = e.analyze_sens(pos, neg, weight=wgt)
assert np.array_equal(s3, s) and np.array_equal(rss3, rss)
# what makes the stored noise result unreadable makes this one unreadable too
for name in ("analyze_dc", "analyze_tr", "reset", "set_solution", "checkpoint_load", "update_param", "load_deck"):
    e.analyze_sens(pos, neg, weight=wgt)
    assert get() == 0, name
    if name == "analyze_dc": e.analyze_dc(F.MODE_OP)
    elif name == "analyze_tr": e.analyze_tr(1e-10, 1)
    elif name == "reset": e.reset()
    elif name == "set_solution": e.set_solution(e.solution())
    elif name == "checkpoint_load": e.restore(e.checkpoint())
    elif name == "update_param": e.update_param(F.R, 0, 0, 1234.0)
    else: e.load_deck(deck, 1)
    assert get() == F.ERR_ARG and b"no sensitivity analysis yet" in lib.pe_hip_last_error(e._h), name
    if name in ("reset", "load_deck"):
        e.reset(); e.analyze_dc(F.MODE_OP)
# update_param is seen by the next call
e.update_param(F.R, 0, 0, 500.0)
e.analyze_dc(F.MODE_OP); e.analyze_dc(F.MODE_OP)
d2 = SC.perturbed(deck, SC.parameter_table(F, deck)[0], 500.0)
s4, _, _, _ = e.analyze_sens(pos, neg)
SC.check(s4[:, 0, :], SC.reference(F, O, d2, e.solution()[0], "OP", list(zip(pos.tolist(), neg.tolist()))), "after update_param")
# without a circuit
f = F.Engine()
one = np.array([0], dtype=np.int32); m1 = np.array([-1], dtype=np.int32)
assert lib.pe_hip_analyze_sens(f._h, C.byref(F.SensControl(1, F._ip(one), F._ip(m1), 0, 1, None)), None, None) == F.ERR_ARG
f.close()
# a circuit with a host-stamp overlay
FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))
def hook(user, event, mode, t, dt, x, a, b):
    if event == 1:
        a[0] = 1e-3; b[0] = 0.0
    return 0
cb = FN(hook)
lib.pe_hip_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_int, FN, C.c_void_p]
o1 = np.array([1], dtype=np.int32); rep = np.array([1e-3])
g = F.Engine()
assert lib.pe_hip_set_overlay(g._h, 1, F._ip(o1), F._ip(o1), F._dp(rep), 1, F._ip(o1), 0, cb, None) == 0
g.set_options(g_min=1e-12)
g.load(2, 1, [(F.VDC, np.array([[1, 0]], dtype=np.int32), np.array([0], dtype=np.int32), np.array([[3.0]]), 0),
              (F.R, np.array([[1, 2]], dtype=np.int32), None, np.array([[1500.0]]), 0)])
g.analyze_dc(F.MODE_DC)
assert lib.pe_hip_analyze_sens(g._h, C.byref(F.SensControl(1, F._ip(one), F._ip(m1), 0, 1, None)), None, None) == F.ERR_ARG
assert b"overlay" in lib.pe_hip_last_error(g._h)
''')


def test_outputs_that_fail(emu):
    """VDC - R - C - C after transient steps: the resident point is fine, but at omega = 0 the node between the capacitors floats and the
    adjoint system is singular.  All outputs of a call share that matrix, so every output is retried alone, carries PE_HIP_ERR_SINGULAR
    and reads NaN ("the other outputs stay readable" cannot occur within one call: one matrix).  The engine goes on: the same handle
    with another circuit gives the reference's numbers"""
    run(emu, r'''
d = pe.deck.Deck()
d.n_nodes = 3
d.add("VDC", (1, 0), 1.0)
d.add("R", (1, 2), 1000.0)
d.add("C", (2, 3), 1e-6)
d.add("C", (3, 0), 2e-6)
for P in (2, 0, 1):
    e = F.Engine(); e.set_options(g_min=0.0); e.set_knob("SENS_OUTPUTS", P); e.load_deck(d); e.reset()
    e.analyze_tr(1e-5, 3)
    s, rss, status, st = e.analyze_sens([1, 2, 0], [-1, -1, 1], weight=[1.0, 1.0], check=False)
    assert st["rc"] == F.ERR_SINGULAR and list(status) == [F.ERR_SINGULAR] * 3, (P, st, status)
    assert st["n_retried_outputs"] == 3 and np.all(np.isnan(s)) and np.all(np.isnan(rss)), (P, st)
    # and the engine goes on: the same handle with a circuit whose operating point exists
    deck, warm, mode = SC.cases(pe)["diode_op"]
    e.set_options(g_min=0.0, **SC.TIGHT); e.load_deck(deck); e.reset(); e.analyze_dc(F.MODE_OP); e.analyze_dc(F.MODE_OP)
    outs = SC.outputs_of(deck)
    s, _, status, st = e.analyze_sens([p for p, _ in outs], [n for _, n in outs])
    assert list(status) == [0] * len(outs) and st["n_retried_outputs"] == 0, st
    SC.check(s[:, 0, :], SC.reference(F, O, deck, e.solution()[0], "OP", outs), "after the failure, P = %d" % P)
''')


def test_plugin_api_under_host_emulation(emu):
    """tests/cpp/sens_divider.cpp: circult::analyze_sens of the plug-in API on a resistive divider behind a DC source against the closed
    form, the propagated AC tolerance"""
    make("-C", CPP, "_build_emu/sens_divider")
    out = subprocess.run([os.path.join(CPP, "_build_emu", "sens_divider")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"sens_divider exited {out.returncode}: {out.stderr}"
