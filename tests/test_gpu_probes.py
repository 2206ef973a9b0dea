"""Transient probes and measurements on the MI355X (pe_hip_set_probes / _arm_probes, include/pe_hip.h): samples recorded on the device
by the resident kernel's recording instantiation (k_tr_steps<MINW, true>) and by k_probe_record behind the split schedule's steps."""
import numpy as np
import pytest

from parity_common import golden, max_err, pe

F = pe.ffi
NL = (1e-6, 1e-5)
LIN = (1e-9, 1e-7)
MEAS = [("min", 0), ("max", 0), ("avg", 1), ("rms", 2), ("integ", 3), ("cross", 0, 0.5, 1, 1), ("cross", 0, 0.3, 0, 2), ("max", 3)]


def ref_measures(t, v, meas=MEAS):
    """[n_meas][2] of one instance from its stride-1 samples (the definitions of include/pe_hip.h)"""
    out = []
    T = t[-1] - t[0]
    for m in meas:
        kind, y = F._MEAS_NAMES[m[0]], v[:, m[1]]
        if kind in (F.MEAS_MIN, F.MEAS_MAX):
            k = 0
            for j in range(1, len(y)):
                if (y[j] < y[k]) if kind == F.MEAS_MIN else (y[j] > y[k]):
                    k = j
            out.append((y[k], t[k]))
        elif kind in (F.MEAS_INTEG, F.MEAS_AVG, F.MEAS_RMS):
            s = 0.0
            for j in range(1, len(y)):
                s += (t[j] - t[j - 1]) * ((y[j - 1] + y[j]) if kind != F.MEAS_RMS else (y[j - 1] ** 2 + y[j] ** 2)) * 0.5
            out.append((s if kind == F.MEAS_INTEG else (s / T if kind == F.MEAS_AVG else np.sqrt(s / T)), T))
        else:
            level, edge, occ = m[2], m[3], m[4]
            n, when = 0, np.nan
            for j in range(1, len(y)):
                v0, v1 = y[j - 1], y[j]
                rise, fall = v0 < level <= v1, v0 > level >= v1
                if rise if edge > 0 else (fall if edge < 0 else (rise or fall)):
                    n += 1
                    if n == occ:
                        when = t[j - 1] + (level - v0) * (t[j] - t[j - 1]) / (v1 - v0)
            out.append((when, float(n)))
    return np.array(out)


def assert_measures(got, t, v, n_rec):
    for b in range(got.shape[0]):
        ref = ref_measures(t[b, :n_rec[b]], v[b, :n_rec[b]])
        for k, m in enumerate(MEAS):
            g, e = got[b, k], ref[k]
            if m[0] in ("min", "max"):
                assert g[0] == e[0] and g[1] == e[1], (b, m, g, e)
            elif m[0] == "cross":
                assert g[1] == e[1] and ((np.isnan(g[0]) and np.isnan(e[0])) or abs(g[0] - e[0]) <= 1e-12 * abs(e[0])), (b, m, g, e)
            else:
                assert g[1] == e[1] and abs(g[0] - e[0]) <= 1e-12 * abs(e[0]) + 1e-300, (b, m, g, e)


def _engine(deck, knobs=None, batch=1, overrides=None, g_min=0.0):
    e = F.Engine(device=0)
    e.set_options(g_min=g_min)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    return e


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("mesh32_nl", {"SPLIT": 0}), ("mesh32_nl", {"SPLIT": 1, "GRAPH": 0}), ("mesh32_nl", {"SPLIT": 1, "GRAPH": 1}),
                                  ("mesh100_nl", {})], ids=["mesh32_resident", "mesh32_split", "mesh32_split_graph", "mesh100_default"])
def test_samples_bit_identical_to_stepwise_runs(case):
    name, knobs = case
    meta, _, deck = golden(name)
    n, dt = 12, meta["dt"]
    twin = _engine(deck, knobs)
    xs, ts = [twin.solution()[0]], [twin.state()["t"][0]]
    for _ in range(n):
        twin.analyze_tr(dt, 1)
        xs.append(twin.solution()[0])
        ts.append(twin.state()["t"][0])
    twin.close()
    rows_n = meta["nodes"]
    rows = [0, rows_n // 2, rows_n - 2, rows_n - 1, rows_n]   # mesh nodes, the source node, the source's branch current
    e = _engine(deck, knobs)
    e.set_probes(rows, n + 1, 1, MEAS)
    e.arm_probes()
    e.analyze_tr(dt, n)
    t, v, n_rec, n_drop = e.probe_samples()
    assert n_rec[0] == n + 1 and n_drop[0] == 0
    assert np.array_equal(t[0], np.array(ts))
    assert np.array_equal(v[0], np.array(xs)[:, rows])
    assert np.array_equal(e.solution()[0], xs[-1]), "the recording kernel computes what the probe-less one does"
    assert_measures(e.measures(), t, v, n_rec)
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,tol", [("rc_step", LIN), ("pn_tt_tr", NL), ("bridge_c2", NL), ("mesh100_nl", NL)])
def test_probe_samples_match_the_reference(name, tol):
    """one analyze_tr over the whole golden run with every row probed: the samples at the golden's snap_steps against the real reference"""
    meta, gx, deck = golden(name)
    e = F.Engine(device=0)
    e.set_options(g_min=meta["gmin"], r_open=meta.get("r_open", 0.0))
    e.load_deck(deck)
    e.reset()
    steps = max(meta["snap_steps"])
    e.set_probes(list(range(meta["rows"])), steps + 1, 1, ())
    e.arm_probes()
    e.analyze_tr(meta["dt"], steps)
    t, v, n_rec, _ = e.probe_samples()
    assert n_rec[0] == steps + 1
    for k, s in enumerate(meta["snap_steps"]):
        assert max_err(v[0, s][None], gx[k][None], *tol) <= 1.0, f"{name} at step {s}"
        assert abs(t[0, s] - s * meta["dt"]) <= 1e-9 * s * meta["dt"]
    e.close()


@pytest.mark.gpu
def test_c5_size_last_sample_is_the_solution_and_measures_match_numpy():
    """C5 size: 1 024 instances of the 100 x 100 diode mesh, 20 steps, 8 probes"""
    B, W, steps, dt = 1024, 100, 20, 1e-10
    deck, r, c = pe.deck.rc_mesh_params(W, W, list(range(1, B + 1)), True)
    e = _engine(deck, None, B, {"R": r[:, :, None], "C": c[:, :, None]})
    nn = W * W + 1
    rows = [0, 1, W, 2 * W + 3, nn // 2, nn - 2, nn - 1, nn]
    e.set_probes(rows, steps + 1, 1, MEAS)
    e.arm_probes()
    e.analyze_tr(dt, steps)
    t, v, n_rec, n_drop = e.probe_samples()
    x = e.solution()
    st = e.state()
    assert np.all(n_rec == steps + 1) and np.all(n_drop == 0)
    assert np.array_equal(v[:, steps], x[:, rows]) and np.array_equal(t[:, steps], st["t"])
    assert np.all(np.diff(t, axis=1) > 0)
    assert_measures(e.measures(), t, v, n_rec)
    e.close()
