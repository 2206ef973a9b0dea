"""Reference of the noise tests (tests/test_noise_emu.py, tests/test_gpu_noise.py): numpy / scipy over the unchanged CPU oracle
(oracle/pe_oracle.py), by the definitions of include/pe_hip.h.

Sources: resistors from the deck (4 k T / R), junctions from the oracle's last linearisation evaluated at its solution
(2 q |geq V_d(x) + Ieq|), MOSFET gm from the oracle's n3_state ((8/3) k T |gm|), BJT base / collector currents passed in by the caller
(KCL over the resistors that feed base and collector in the oracle's solution: exactly g V + Ieq, because x solves the linearised
system).  Order: resistors, junctions (D and the four of an FBR, deck order), then NMOS, PMOS, NPN, PNP.

Per omega the oracle's complex AC stamp is solved twice: DIRECT (one unit current per source, rhs[a] -= 1, rhs[b] += 1, all columns of
one splu solve; c_k = S_k |x[out_pos] - x[out_neg]|^2) and TRANSPOSED (A^T y = e_out; c_k = S_k |y_b - y_a|^2).

Tolerance: every adjoint phasor may be off by e_r = 1e-9 + 1e-6 |y_r| (the project's AC tolerance, tests/test_gpu_parity.py
test_ac_golden_parity); a contribution may therefore differ by S_k ((|D_k| + e_a + e_b)^2 - |D_k|^2) + 1e-6 S_k |D_k|^2 (the last term:
the bias-dependent density), the total by the sum of those bounds."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

K_B = 1.380650524e-23
Q_E = 1.6021765314e-19
T_DEFAULT = 300.15


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


def sources(o, temp_k=T_DEFAULT, bjt_currents=()):
    """(row_a, row_b, S) arrays of the oracle's circuit at its current state; bjt_currents: (I_b, I_c) per BJT, NPN then PNP"""
    a, b, s = [], [], []
    row = lambda n: n - 1 if n > 0 else -1
    for kind, nodes, par in o.deck.devices:
        if kind == "R":
            a.append(row(nodes[0])); b.append(row(nodes[1])); s.append(4.0 * K_B * temp_k * abs(1.0 / par[0]))
    if o.dio is not None:
        cur = o.dio.geq * o._dio_vd() + o.dio.Ieq
        for da, dc, i in zip(o.dio.a, o.dio.c, cur):
            a.append(int(da)); b.append(int(dc)); s.append(2.0 * Q_E * abs(i))
    bj = list(bjt_currents)
    for want in ("NMOS", "PMOS", "NPN", "PNP"):
        idx = 0
        for kind, nodes, par in o.deck.devices:
            if kind != want:
                continue
            if kind in ("NMOS", "PMOS"):
                gds, gm = o.n3_state[(kind, idx)]
                a.append(row(nodes[0])); b.append(row(nodes[2])); s.append(8.0 / 3.0 * K_B * temp_k * abs(gm))
            else:
                ib, ic = bj.pop(0)
                a.append(row(nodes[0])); b.append(row(nodes[2])); s.append(2.0 * Q_E * abs(ib))
                a.append(row(nodes[1])); b.append(row(nodes[2])); s.append(2.0 * Q_E * abs(ic))
            idx += 1
    return np.array(a, dtype=int), np.array(b, dtype=int), np.array(s, dtype=float)


def _matrix(o, omega):
    A, _ = o.stamp_ac(omega)
    keys = list(A.keys())
    return sp.csc_matrix((np.array([A[k] for k in keys], dtype=complex), (np.array([k[0] for k in keys]), np.array([k[1] for k in keys]))),
                         shape=(o.rows, o.rows))


def _at(v, r):
    """v[r] with ground (-1) reading 0; v [rows] or [rows][k], r scalar or array"""
    r = np.asarray(r)
    g = v[np.maximum(r, 0)]
    return np.where((r >= 0).reshape(r.shape + (1,) * (g.ndim - r.ndim)), g, 0.0)


def reference(o, omegas, out_pos, out_neg, src, direct=True):
    """per omega: contributions by the transposed solve, their bound, and (direct=True) the contributions by the direct method.
    Returns dict: contrib [n][k], total [n], bound [n][k], direct [n][k] or None."""
    ra, rb, S = src
    adj, bound, dire = [], [], []
    for w in omegas:
        M = _matrix(o, w)
        e = np.zeros(o.rows, dtype=complex)
        if out_pos >= 0:
            e[out_pos] += 1.0
        if out_neg >= 0:
            e[out_neg] -= 1.0
        y = spla.splu(M.T.tocsc(), permc_spec="COLAMD", diag_pivot_thresh=1.0).solve(e)
        d = np.abs(_at(y, rb) - _at(y, ra))
        err = lambda r: np.where(r >= 0, 1e-9 + 1e-6 * np.abs(y[np.maximum(r, 0)]), 0.0)
        adj.append(S * d * d)
        bound.append(S * ((d + err(ra) + err(rb)) ** 2 - d * d) + 1e-6 * S * d * d)
        if direct:
            rhs = np.zeros((o.rows, len(S)), dtype=complex)
            for k in range(len(S)):
                if ra[k] >= 0:
                    rhs[ra[k], k] -= 1.0
                if rb[k] >= 0:
                    rhs[rb[k], k] += 1.0
            x = spla.splu(M, permc_spec="COLAMD", diag_pivot_thresh=1.0).solve(rhs) if len(S) else np.zeros((o.rows, 0))
            out = (x[out_pos] if out_pos >= 0 else 0.0) - (x[out_neg] if out_neg >= 0 else 0.0)
            dire.append(S * np.abs(out) ** 2)
    adj, bound = np.array(adj), np.array(bound)
    return {"contrib": adj, "total": adj.sum(axis=1), "bound": bound, "direct": np.array(dire) if direct else None}


def check(psd, contrib, ref, what=""):
    """engine densities [n] and contributions [n][k] (or None) of one instance against reference(); prints the worst figure, then asserts"""
    r = ref["direct"] if ref["direct"] is not None else ref["contrib"]
    if ref["direct"] is not None:
        # the two reference methods agree to 1e-12 relative to the total
        gap = float(np.max(np.abs(ref["direct"] - ref["contrib"]).max(axis=1) / ref["total"])) if r.size else 0.0
        print(what, "direct vs transposed reference:", gap)
        assert gap <= 1e-12, gap
    tot, tb = r.sum(axis=1), ref["bound"].sum(axis=1)
    print(what, "total: worst |d| / bound =", float(np.max(np.abs(psd - tot) / tb)) if len(tb) else 0.0)
    if contrib is not None:
        nz = ref["bound"] > 0
        print(what, "contributions: worst |d| / bound =", float(np.max(np.abs(contrib - r)[nz] / ref["bound"][nz])) if nz.any() else 0.0)
        assert np.all(np.abs(contrib - r) <= ref["bound"]), what
    assert np.all(np.abs(psd - tot) <= tb), what
