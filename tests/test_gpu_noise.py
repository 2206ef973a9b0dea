"""GPU (MI355X): small-signal noise analysis (pe_hip_analyze_noise, include/pe_hip.h) -- the adjoint system solved per frequency point as
instances of the sweep engine, densities by k_noise_sources, the reduction over the sources by k_noise_accumulate -- against the CPU
oracle (tests/noise_common.py: direct method and transposed solve, the project's AC tolerance propagated to a contribution) and a
closed form through the plug-in API.  No case may lean on a retried point: n_retried_points == 0."""
import os
import subprocess

import numpy as np
import pytest

import noise_common as NC
from parity_common import ROOT, make, pe

pytestmark = pytest.mark.gpu

F = pe.ffi
CPP = os.path.join(ROOT, "tests", "cpp")


def oracle(oracle_mod, deck, warm=None):
    o = oracle_mod.Oracle(deck, g_min=0.0)
    o.prepare()
    if warm is not None:
        o.x = np.array(warm, dtype=float)
    it = o.solve("OP") if o.nonlinear else 0
    assert it >= 0, it
    return o, it


def engine(deck, warm=None, batch=1, overrides=None, knobs=None):
    e = F.Engine(device=0)
    e.set_options(g_min=0.0)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    if warm is not None:
        e.set_solution(np.array([warm] * batch, dtype=float))
    if deck.has_nonlinear():
        e.analyze_dc(F.MODE_OP)
    return e


def mesh(W, seed, node, amps):
    d = pe.deck.rc_mesh(W, W, seed, True)
    d.add("IDC", (0, node), amps)      # biases the junctions around that node: shot noise that is not zero
    return d


CASES = {
    "ac_rlc_diode": (lambda: pe.deck.ac_rlc_diode(), 1, np.logspace(2.0, 7.0, 26), None, None),
    "ac_nmos_amp": (lambda: pe.deck.ac_nmos_amp(), 4, np.logspace(1.0, 8.0, 29), None, None),
    "bjt_common_emitter": (lambda: pe.deck.bjt_common_emitter(False), 2, np.logspace(2.0, 7.0, 11), [5.0, 0.69, 0.7, 0.0],
                           lambda o: [((o.x[0] - o.x[1]) / 1e5, (o.x[0] - o.x[2]) / 1e3)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_contributions(oracle_mod, name):
    make_deck, out, w, warm, bjt = CASES[name]
    deck = make_deck()
    o, _ = oracle(oracle_mod, deck, warm)
    src = NC.sources(o, bjt_currents=bjt(o) if bjt else ())
    ref = NC.reference(o, w, out, -1, src)
    e = engine(deck, warm)
    try:
        psd, c, status, st = e.analyze_noise(w, out, -1, contributions=True)
        S = e.noise_source_density()[0]
    finally:
        e.close()
    print(name, st)
    assert list(status) == [0] * len(w) and st["n_retried_points"] == 0 and st["n_sources"] == len(src[2]), st
    assert st["n_analyses"] == NC.bands(w), st
    assert np.all(np.abs(S - src[2]) <= 1e-6 * src[2])
    NC.check(psd[:, 0], c[:, 0, :], ref, name)


MESH_W = np.logspace(7.0, 11.5, 10)


def test_biased_mesh_batch_of_three(oracle_mod):
    """12 x 12 diode mesh, bias current into its centre, 282 sources (no multiple of 64), three instances with their own R and C"""
    seeds = [1, 2, 3]
    _, r, c = pe.deck.rc_mesh_params(12, 12, seeds, True)
    e = engine(mesh(12, 1, 79, 4e-4), batch=3, overrides={"R": r[:, :, None], "C": c[:, :, None]})
    try:
        psd, con, status, st = e.analyze_noise(MESH_W, 77, 5, contributions=True)
    finally:
        e.close()
    print(st)
    assert list(status) == [0] * len(MESH_W) and st["n_retried_points"] == 0 and st["n_sources"] == 282, st
    for b, s in enumerate(seeds):
        o, it = oracle(oracle_mod, mesh(12, s, 79, 4e-4))
        cur = o.dio.geq * o._dio_vd() + o.dio.Ieq
        assert int(np.sum(np.abs(cur) > 1e-7)) >= 10
        NC.check(psd[:, b], con[:, b, :], NC.reference(o, MESH_W, 77, 5, NC.sources(o)), "mesh seed %d" % s)


def test_pass_size_and_repetition_do_not_change_a_bit():
    rng = np.random.default_rng(5)
    idx = rng.permutation(len(MESH_W))
    w = MESH_W[np.concatenate([idx, idx[3:4]])]
    res = {}
    for P in (1, 4, 0):
        e = engine(mesh(12, 1, 79, 4e-4), knobs={"AC_SWEEP_POINTS": P})
        try:
            psd, con, status, st = e.analyze_noise(w, 77, 5, contributions=True)
            again = e.analyze_noise(w, 77, 5, contributions=True)
            total_only = e.analyze_noise(w, 77, 5)[0]
        finally:
            e.close()
        print(P, st)
        assert list(status) == [0] * len(w) and st["n_retried_points"] == 0, (P, st)
        assert st["points_per_pass"] == 1 if P == 1 else st["points_per_pass"] > 1, (P, st)
        assert np.array_equal(again[0], psd) and np.array_equal(again[1], con), "two consecutive calls"
        assert np.array_equal(total_only, psd), "with and without the contributions kept"
        res[P] = (psd, con)
    for P in (1, 4):
        assert np.array_equal(res[P][0], res[0][0]) and np.array_equal(res[P][1], res[0][1]), P
    psd, con = res[0]
    assert np.array_equal(psd[-1], psd[3]) and np.array_equal(con[-1], con[3]), "the duplicate point"
    assert np.all(np.abs(con.sum(axis=2) - psd) <= 1e-13 * psd)


def test_large_circuit_split_schedule_against_the_oracle(oracle_mod):
    """the 45 x 45 diode mesh with a bias current (4 054-row adjoint system: the engines run the split schedule; 4 213 sources: three
    chunks of the reduction), totals and contributions against the oracle's transposed solve"""
    deck = mesh(45, 1, 1013, 3e-4)
    omegas = np.array(sorted([2e8, 2e9, 2e10] + list(np.logspace(np.log10(2.6e8), np.log10(1.6e10), 9))))
    o, it = oracle(oracle_mod, deck)
    cur = o.dio.geq * o._dio_vd() + o.dio.Ieq
    print("oracle iterations", it, "junctions above 0.1 uA:", int(np.sum(np.abs(cur) > 1e-7)), "of", len(cur))
    assert int(np.sum(np.abs(cur) > 1e-7)) >= 100
    src = NC.sources(o)
    ref = NC.reference(o, omegas, 1000, 3, src, direct=False)
    e = engine(deck)
    try:
        psd, con, status, st = e.analyze_noise(omegas, 1000, 3, contributions=True)
    finally:
        e.close()
    print(st)
    assert st["n_sources"] == len(src[2]) == 4213, st
    assert list(status) == [0] * len(omegas) and st["n_retried_points"] == 0 and st["n_analyses"] == NC.bands(omegas), st
    NC.check(psd[:, 0], con[:, 0, :], ref, "45 x 45")


def test_noise_at_the_benchmark_size():
    """rc_mesh(100, 100) with diodes: about 21 000 sources, 16 points over four bands in one call; four of them -- the first point of
    each band, so that both calls match their pivot orders on the same values -- bit for bit equal to a call with only those four"""
    deck = pe.deck.rc_mesh(100, 100, 1, True)
    w = np.logspace(7.5, 10.7, 16)
    pick = [0, 5, 10, 15]
    a, b = engine(deck), engine(deck)
    try:
        psd, _, status, st = a.analyze_noise(w, 5049, -1)
        few, _, status4, st4 = b.analyze_noise(w[pick], 5049, -1)
    finally:
        a.close()
        b.close()
    print(st, st4, psd[:, 0])
    assert list(status) == [0] * len(w) and list(status4) == [0] * 4 and st["n_retried_points"] == 0, st
    assert np.all(np.isfinite(psd)) and np.all(psd > 0.0)
    assert st["n_passes"] < len(w) and st["n_analyses"] == NC.bands(w) == 4 and st4["n_analyses"] == 4, (st, st4)
    assert np.array_equal(psd[pick], few)


def test_plugin_api_noise():
    """tests/cpp/noise_rc.cpp against the product library: R - C low pass, closed form per point and kT/C"""
    make("-C", CPP, "_build/noise_rc")
    out = subprocess.run([os.path.join(CPP, "_build", "noise_rc")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"noise_rc exited {out.returncode}: {out.stderr}"
