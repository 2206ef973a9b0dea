"""GPU (MI355X): DC sensitivity analysis (pe_hip_analyze_sens, include/pe_hip.h) -- the adjoint system at omega = 0 solved per output as
instances of the sweep engine with the selectors of k_sens_rhs, d f / d p against the adjoint solution and the weighted sum of squares by
k_sens_accumulate / k_sens_finish -- against the CPU oracle set to the engine's own solution (tests/sens_common.py: direct method and
transposed solve, the project's AC tolerance propagated through d f / d p).  The cases of tests/test_sens_emu.py again on the device,
in-process.  No case may lean on a retried output: n_retried_outputs == 0."""
import os
import subprocess

import numpy as np
import pytest

import sens_common as SC
from parity_common import ROOT, make, pe

pytestmark = pytest.mark.gpu

F = pe.ffi
CPP = os.path.join(ROOT, "tests", "cpp")
TEAM = 256                                            # workgroup of k_sens_accumulate (pe_sens.hpp SENS_THREADS)


@pytest.mark.parametrize("name", list(SC.cases(pe)))
def test_parity_with_every_sensitivity_kept(oracle_mod, name):
    e, ref, s = SC.run_case(pe, oracle_mod, name)
    e.close()


@pytest.mark.parametrize("split", [0, 1])
def test_several_outputs_in_one_call(split):
    """5 outputs with SENS_OUTPUTS 1, 2 and automatic, the main engine on the resident (SPLIT 0) and on the split schedule (SPLIT 1): s and
    rss bit-identical across the three, each output equal to its single-output call bit for bit, n_passes as expected, one analysis"""
    deck = SC.mesh(pe, 12, 1)
    outs = [(77, -1), (5, 77), (144, -1), (20, 100), (-1, 3)]
    pos, neg = [p for p, _ in outs], [n for _, n in outs]
    w = 1.0 + 0.01 * np.arange(402)
    res = {}
    for P, passes in ((1, 5), (2, 3), (0, 1)):
        e = SC.engine(pe, deck, knobs={"SENS_OUTPUTS": P, "SPLIT": split})
        try:
            s, rss, status, st = e.analyze_sens(pos, neg, weight=w)
            assert list(status) == [0] * 5 and st["n_retried_outputs"] == 0 and st["n_analyses"] == 1 and st["n_params"] == 402, (P, st)
            assert st["n_passes"] == passes and st["outputs_per_pass"] == (P if P else 5), (P, st)
            res[P] = (s, rss)
            if P == 2:
                for o in range(5):
                    s1, r1, _, st1 = e.analyze_sens([pos[o]], [neg[o]], weight=w)
                    assert st1["n_passes"] == 1 and np.array_equal(s1[0], s[o]) and np.array_equal(r1[0], rss[o]), o
                # the system that was really solved in the last pass (one output): the slot's selector
                N = e.rows
                rhs = e.matrix_ac(4, 0)[3]
                want = np.zeros(2 * N)
                want[pos[4] if pos[4] >= 0 else neg[4]] = 1.0 if pos[4] >= 0 else -1.0
                if pos[4] >= 0 and neg[4] >= 0:
                    want[neg[4]] = -1.0
                assert np.array_equal(rhs, want)
        finally:
            e.close()
    for P in (1, 2):
        assert np.array_equal(res[P][0], res[0][0]) and np.array_equal(res[P][1], res[0][1]), P
    for o in range(5):
        assert res[0][1][o, 0] == SC.rss_in_order(res[0][0][o, 0], w, TEAM), o


def test_batch_of_three_equals_its_single_runs(oracle_mod):
    seeds = [1, 2, 3]
    base, r, c = pe.deck.rc_mesh_params(12, 12, seeds, True)
    outs = [(77, -1), (5, 77)]
    e = SC.engine(pe, SC.mesh(pe, 12, 1), batch=3, overrides={"R": r[:, :, None], "C": c[:, :, None]})
    try:
        s, _, status, st = e.analyze_sens([77, 5], [-1, 77])
        x = e.solution()
    finally:
        e.close()
    assert list(status) == [0, 0] and st["n_retried_outputs"] == 0 and st["n_analyses"] == 1, st
    for b, seed in enumerate(seeds):
        SC.check(s[:, b, :], SC.reference(F, oracle_mod, SC.mesh(pe, 12, seed), x[b], "OP", outs), "mesh seed %d" % seed)
        e1 = SC.engine(pe, SC.mesh(pe, 12, seed))
        try:
            s1, _, _, _ = e1.analyze_sens([77, 5], [-1, 77])
            assert np.array_equal(e1.solution()[0], x[b]), "the operating point of the single run"
        finally:
            e1.close()
        assert np.array_equal(s1[:, 0, :], s[:, b, :]), "instance %d equals its batch-1 run" % b


def test_more_than_one_reduction_chunk(oracle_mod):
    """rc_mesh(32, 32, nonlinear) with the bias current: 3 010 parameters against the 2 048 of a reduction chunk -- two chunks, the second
    with a ragged tail (962 = 3 x 256 + 194).  Batch 2, one output; the largest shape of this file"""
    seeds = [1, 2]
    base, r, c = pe.deck.rc_mesh_params(32, 32, seeds, True)
    e = SC.engine(pe, SC.mesh(pe, 32, 1), batch=2, overrides={"R": r[:, :, None], "C": c[:, :, None]})
    try:
        n = len(e.sens_params()["kind"])
        assert n == 3010, n
        w = 1.0 + (np.arange(n) % 7)
        s, rss, status, st = e.analyze_sens([500], [-1], weight=w)
        x = e.solution()
        _, rss0, _, _ = e.analyze_sens([500], [-1], weight=w, keep=False)
    finally:
        e.close()
    assert list(status) == [0] and st["n_retried_outputs"] == 0 and st["n_params"] == n, st
    assert np.array_equal(rss0, rss)
    for b, seed in enumerate(seeds):
        r_, b_ = SC.check(s[:, b, :], SC.reference(F, oracle_mod, SC.mesh(pe, 32, seed), x[b], "OP", [(500, -1)]), "mesh32 seed %d" % seed)
        want, bound = SC.rss_reference(r_, b_, w)
        assert abs(rss[0, b] - want[0]) <= bound[0], (rss[0, b], want, bound)
        assert rss[0, b] == SC.rss_in_order(s[0, b], w, TEAM), (rss[0, b], SC.rss_in_order(s[0, b], w, TEAM))


def test_normalized_weight_and_rss_only(oracle_mod):
    deck, warm, mode = SC.cases(pe)["diode_op"]
    outs = SC.outputs_of(deck)
    pos, neg = [p for p, _ in outs], [n for _, n in outs]
    e = SC.engine(pe, deck)
    try:
        ref = SC.reference(F, oracle_mod, deck, e.solution()[0], "OP", outs)
        s, none, _, _ = e.analyze_sens(pos, neg)
        sn, none2, _, _ = e.analyze_sens(pos, neg, normalized=True)
        assert none is None and none2 is None
        r_, b_ = SC.check(sn[:, 0, :], ref, "normalized", normalized=True)
        k_isr = [k for k, t in enumerate(ref["table"]) if t["name"] == "D" and t["column"] == 2][0]
        assert ref["p"][k_isr] == 0.0 and np.all(s[:, 0, k_isr] != 0.0) and np.all(sn[:, 0, k_isr] == 0.0)
        w = np.array([0.01, 0.05, 0.1, 0.0, 2.0, 0.3, 0.01, 1.0, 1.0, 0.02])
        for norm, (rr, bb) in ((False, (ref["s"], ref["bound"])), (True, (r_, b_))):
            sk, rss, _, st = e.analyze_sens(pos, neg, normalized=norm, weight=w)
            nk, rss2, _, _ = e.analyze_sens(pos, neg, normalized=norm, weight=w, keep=False)
            assert nk is None and np.array_equal(rss, rss2), "the sum does not depend on whether the sensitivities are kept"
            want, bound = SC.rss_reference(rr, bb, w)
            assert np.all(np.abs(rss[:, 0] - want) <= bound), (rss, want, bound)
            for o in range(len(outs)):
                assert rss[o, 0] == SC.rss_in_order(sk[o, 0], w, TEAM), o
    finally:
        e.close()


@pytest.mark.parametrize("name,need", [("diode_op", 6), ("nmos_saturation", 6), ("bjt_npn", 8)])
def test_against_the_update_param_loop_on_the_engine_itself(oracle_mod, name, need):
    """central differences of update_param -> analyze_dc -> solution on the device at h and h / 2 for every parameter; allowance
    2 |FD(h) - FD(h/2)| + bound_k, asserted where it is below 1e-3 |s_k| (need: tests/test_sens_emu.py)"""
    deck, warm, mode = SC.cases(pe)[name]
    outs = SC.outputs_of(deck)
    e, ref, s = SC.parity(pe, oracle_mod, deck, outs, warm, mode, name)
    try:
        x0 = e.solution()

        def out_at(t, value):
            e.update_param(t["kind"], t["index"], t["column"], value)
            e.set_solution(x0)
            if e.analyze_dc(F.MODE_OP, check=False)["rc"] != 0:
                return None
            e.analyze_dc(F.MODE_OP)
            x = e.solution()[0]
            return np.array([(x[p] if p >= 0 else 0.0) - (x[n] if n >= 0 else 0.0) for p, n in outs])

        checked, worst = 0, 0.0
        for k, t in enumerate(ref["table"]):
            fd = []
            for h in (1e-4, 5e-5):
                step = h * abs(t["value"]) if t["value"] != 0.0 else 1e-6 * (h / 1e-4)
                up, dn = out_at(t, t["value"] + step), out_at(t, t["value"] - step)
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
    finally:
        e.close()
    print(name, "columns checked:", checked, "of", len(ref["table"]), "worst |d| / allowance =", worst)
    assert checked >= need, (name, checked)


def test_plugin_api_sens():
    """tests/cpp/sens_divider.cpp against the product library: a resistive divider behind a DC source, closed form"""
    make("-C", CPP, "_build/sens_divider")
    out = subprocess.run([os.path.join(CPP, "_build", "sens_divider")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"sens_divider exited {out.returncode}: {out.stderr}"
