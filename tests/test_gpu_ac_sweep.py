"""GPU (MI355X): the frequency-batched AC sweep (pe_hip_analyze_ac_sweep, include/pe_hip.h) -- the points of a sweep solved as extra
instances of the real-equivalent system, value vectors made by k_ac_sweep_fill, refinement per instance -- against the reference's
goldens, the single-point path, the CPU oracle, and a closed form through the plug-in API.  Tolerance: the project's AC tolerance
|d| <= 1e-9 + 1e-6 |want| (tests/test_gpu_parity.py).  No case may lean on the single-point fallback: n_fallback_points == 0."""
import os
import subprocess

import numpy as np
import pytest

from parity_common import ROOT, golden, golden_complex, make, pe

pytestmark = pytest.mark.gpu

F = pe.ffi
CPP = os.path.join(ROOT, "tests", "cpp")


def within(a, b):
    return bool(np.all(np.abs(a - b) <= 1e-9 + 1e-6 * np.abs(b)))


def bands(omegas):
    """frequency bands of include/pe_hip.h: ascending, omega == 0 on its own, a band takes omega <= 10 x its first"""
    w = np.sort(np.asarray(omegas, dtype=float))
    n, i = 0, 0
    while i < len(w):
        j = i + 1
        while j < len(w) and (w[j] == 0.0 if w[i] == 0.0 else w[j] <= 10.0 * w[i]):
            j += 1
        n, i = n + 1, j
    return n


def engine(deck, batch=1, op=True, g_min=0.0, r_open=0.0):
    e = F.Engine(device=0)
    e.set_options(g_min=g_min, r_open=r_open)
    e.load_deck(deck, batch)
    e.reset()
    if op:
        e.analyze_dc(F.MODE_OP)
    return e


def loop(e, omegas):
    out = []
    for w in omegas:
        x, rc = e.analyze_ac(w)
        assert rc == 0
        out.append(x)
    return np.array(out)


@pytest.mark.parametrize("name", ["ac_rc_lowpass", "ac_linear_mix", "ac_nmos_amp", "ac_rlc_diode_acop", "ac_controlled_rest_acop", "ac_transistors_acop", "ac_transistors_hf_acop"])
def test_reference_goldens_in_one_sweep(name):
    meta, gx, deck = golden(name)
    e = engine(deck, op=meta["analysis"] == "ACOP" or deck.has_nonlinear(), g_min=meta["gmin"], r_open=meta.get("r_open", 0.0))
    try:
        x, status, st = e.analyze_ac_sweep(meta["omegas"])
    finally:
        e.close()
    g = golden_complex(meta, gx)
    print(name, st, float(np.max(np.abs(x[:, 0, :] - g) / (1e-9 + 1e-6 * np.abs(g)))))
    assert x.shape == (len(g), 1, g.shape[1]) and list(status) == [0] * len(g)
    assert within(x[:, 0, :], g)
    assert st["n_fallback_points"] == 0 and st["n_analyses"] == bands(meta["omegas"]), st


def test_shuffled_sweep_matches_the_single_point_path():
    deck = pe.deck.rc_mesh(12, 12, 1, True)
    w_sorted = np.logspace(7.0, 11.5, 46)
    idx = np.random.default_rng(3).permutation(len(w_sorted))
    idx = np.concatenate([idx, idx[5:6]])
    w = w_sorted[idx]
    a, b = engine(deck), engine(deck)
    try:
        ref = loop(a, w_sorted)[idx]
        x, status, st = b.analyze_ac_sweep(w)
    finally:
        a.close()
        b.close()
    print(st, float(np.max(np.abs(x - ref) / (1e-9 + 1e-6 * np.abs(ref)))))
    assert x.shape == ref.shape and list(status) == [0] * len(w)
    assert within(x, ref)
    assert np.array_equal(x[-1], x[5])
    assert st["n_analyses"] == bands(w) == 5 and st["n_fallback_points"] == 0 and st["points_per_pass"] > 1, st


def test_row_selection():
    deck = pe.deck.rc_mesh(12, 12, 1, True)
    w = np.logspace(7.0, 11.5, 46)
    e = engine(deck)
    try:
        full, _, st0 = e.analyze_ac_sweep(w)
        rows = [0, 17, 17, 143, e.rows - 1, 144]
        e.set_ac_sweep_rows(rows)
        x, status, st = e.analyze_ac_sweep(w)
        assert st0["n_fallback_points"] == 0 and st["n_fallback_points"] == 0
        assert x.shape == (len(w), 1, len(rows))
        assert np.array_equal(x, full[:, :, rows]), "same batches, same launches: the kept rows are the same numbers"
        with pytest.raises(F.PeHipError) as err:
            e.set_ac_sweep_rows([0, e.rows])
        assert err.value.code == F.ERR_ARG
        x2, _, _ = e.analyze_ac_sweep(w)
        assert np.array_equal(x2, x), "a refused row selection leaves the engine as it was"
    finally:
        e.close()


def test_large_circuit_split_schedule_against_the_oracle(oracle_mod):
    """the 45 x 45 diode mesh of test_ac_on_large_circuit_split_schedule (4 054-row AC system: the AC engines run the split schedule),
    its three frequencies and 22 more between them, every point against the oracle's complex sparse LU"""
    deck = pe.deck.rc_mesh(45, 45, 1, True)
    omegas = sorted([2e8, 2e9, 2e10] + list(np.logspace(np.log10(2.3e8), np.log10(1.8e10), 22)))
    ref = oracle_mod.Oracle(deck).analyze_ac(omegas)
    assert ref is not None and all(r is not None for r in ref)
    e = engine(deck)
    try:
        x, status, st = e.analyze_ac_sweep(omegas)
    finally:
        e.close()
    ref = np.array(ref)
    print(st, float(np.max(np.abs(x[:, 0, :] - ref) / (1e-9 + 1e-6 * np.abs(ref)))))
    assert list(status) == [0] * len(omegas) and st["n_fallback_points"] == 0, st
    assert st["n_analyses"] == bands(omegas) and st["points_per_pass"] > 1, st
    assert within(x[:, 0, :], ref)


def test_sweep_at_the_benchmark_size():
    """rc_mesh(100, 100) with diodes, 64 points over 3.2 decades in one sweep; eight of them, spread over the bands, against the
    single-point path (solving all of them singly is what the sweep removes)"""
    deck = pe.deck.rc_mesh(100, 100, 1, True)
    w = np.logspace(7.5, 10.7, 64)
    a, b = engine(deck), engine(deck)
    try:
        x, status, st = a.analyze_ac_sweep(w)
        pick = list(range(0, 64, 9))
        ref = loop(b, w[pick])
    finally:
        a.close()
        b.close()
    print(st, float(np.max(np.abs(x[pick] - ref) / (1e-9 + 1e-6 * np.abs(ref)))))
    assert len(pick) >= 8
    assert list(status) == [0] * len(w) and st["n_fallback_points"] == 0, st
    assert np.all(np.isfinite(x.real)) and np.all(np.isfinite(x.imag))
    assert st["n_analyses"] == bands(w) and st["n_passes"] < len(w), st
    assert within(x[pick], ref)


def test_points_that_fail_in_their_batch():
    """VAC - R - C - C is singular at omega = 0 (nothing holds the node between the capacitors): those points get the single-point
    path's status and read NaN, the others solve and stay readable, with the pass size given and automatic"""
    d = pe.deck.Deck()
    d.n_nodes = 3
    d.add("VAC", (1, 0), 1.0, 1000.0, 0.0)
    d.add("R", (1, 2), 1000.0)
    d.add("C", (2, 3), 1e-6)
    d.add("C", (3, 0), 2e-6)
    w = np.array([0.0, 1e3, 0.0, 2e3, 1e5])
    good = [1, 3, 4]
    ref = engine(d, op=False)
    try:
        want_rc = [ref.analyze_ac(x, check=False)[1] for x in w]
        want = loop(ref, w[good])
    finally:
        ref.close()
    assert want_rc == [F.ERR_SINGULAR, 0, F.ERR_SINGULAR, 0, 0]
    for P in (4, 0):
        e = engine(d, op=False)
        try:
            e.set_knob("AC_SWEEP_POINTS", P)
            x, status, st = e.analyze_ac_sweep(w, check=False)
        finally:
            e.close()
        print(P, st, list(status))
        assert st["rc"] == F.ERR_SINGULAR and list(status) == want_rc and st["n_fallback_points"] == 2, (P, st)
        assert np.all(np.isnan(x[[0, 2]].real)) and np.all(np.isnan(x[[0, 2]].imag))
        assert within(x[good], want)


def test_plugin_api_sweeps():
    """tests/cpp/ac_sweep.cpp against the product library: log sweep over six decades and a linear sweep of an R-L-C network, closed form"""
    make("-C", CPP, "_build/ac_sweep")
    out = subprocess.run([os.path.join(CPP, "_build", "ac_sweep")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"ac_sweep exited {out.returncode}: {out.stderr}"
