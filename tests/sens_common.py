"""Reference of the DC sensitivity tests (tests/test_sens_emu.py, tests/test_gpu_sens.py): numpy / scipy over the unchanged CPU oracle
(oracle/pe_oracle.py), by the definitions of include/pe_hip.h.

Reference point: the oracle is SET to the solution the engine holds (the engine is converged with every Newton tolerance at 1e-13 / 1e-15
and solved once more from there, so that the last linearisation point and x coincide to rounding).  J, b = assemble(mode) at that x is the
Newton Jacobian.  d_k = d f / d p_k of f = A x - b is restated analytically here, per kind and raw column, from the models' formulas and
the derivation of the derived columns, with the branch predicates as the engine writes them.  DIRECT reference: J (dx / dp) = -D for all
columns with one LU; TRANSPOSED: J^T y = e, s_k = -y . d_k.  The two agree to 1e-12 of the largest |s_k| of the output.

Tolerance of the engine against the reference: every adjoint entry may be off by e_r = 1e-9 + 1e-6 |y_r| (the project's AC tolerance,
tests/test_gpu_parity.py test_ac_golden_parity, tests/noise_common.py), propagated: bound_k = sum_r e_r |d_k,r|; rss gets the sum of the
propagated bounds of its terms, sum_k w_k^2 ((|s_k| + bound_k)^2 - s_k^2).  With normalized results both sides carry |p_k|.

The restated derivatives are themselves checked (fd_check): central differences of fully re-converged oracle solves at relative steps
h = 1e-4 and h / 2 (absolute 1e-6 where the parameter is 0); allowance 2 |FD(h) - FD(h/2)| + bound_k; a column counts as checked only
where that allowance is below 1e-3 |s_k|."""
import copy
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

K_B = 1.380650524e-23
Q_E = 1.6021765314e-19
KELVIN = -273.15
TIGHT = dict(v_abstol=1e-13, v_reltol=1e-13, i_abstol=1e-15, i_reltol=1e-13)
DIODE_COLS = (0, 1, 2, 3, 4, 5, 6, 8)
NBRANCH = {"L": 1, "VDC": 1, "VAC": 1, "VCVS": 1, "CCCS": 1, "CCVS": 2, "OPAMP": 1, "XFMR": 2, "SW": 1, "SAW": 1, "SQR": 1, "PULSE": 1, "TRI": 1, "KL": 2,
           "RELAY": 1, "XCT": 3}
FBR_DEFAULT = (1e-14, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 1.0, 1.0, 0.0)
GENERIC_ORDER = ("VCCS", "VCVS", "CCCS", "CCVS", "OPAMP", "XFMR", "NMOS", "PMOS", "NPN", "PNP", "XCT")  # the order ffi.deck_tables passes them


def codes(F):
    return {"R": F.R, "VDC": F.VDC, "IDC": F.IDC, "D": F.DIODE, "VCCS": F.VCCS, "VCVS": F.VCVS, "CCCS": F.CCCS, "CCVS": F.CCVS, "OPAMP": F.OPAMP,
            "XFMR": F.XFMR, "XCT": F.XFMR_CT, "NMOS": F.NMOS, "PMOS": F.PMOS, "NPN": F.BJT_NPN, "PNP": F.BJT_PNP}


def _limexp(z):
    """(limexp, its derivative) of pe_front.hpp: predicates on the quotient"""
    if z > 50.0:
        return math.exp(50.0) * (1.0 + (z - 50.0)), math.exp(50.0)
    if z < -50.0:
        return math.exp(-50.0), 0.0
    return math.exp(z), math.exp(z)


def diode_derivatives(par, Ud):
    """{raw column: d Id / d p} of a PN junction with the deck's ten columns at junction voltage Ud; also returns the arm"""
    Is, N, Isr, Nr, Temp, Ibv, Bv, Bv_set, Area, _tt = par
    Ut = K_B * (Temp - KELVIN) / Q_E
    ct = K_B / Q_E
    Is_eff, Isr_eff, Ute, Uter = Is * Area, Isr * Area, N * Ut, Nr * Ut
    Bv_eff = Bv - N * Ut * math.log(Ibv / Is_eff) if Bv_set != 0.0 else Bv
    if Bv_set != 0.0 and Ud < -Bv_eff:
        z = -(Bv_eff + Ud) / Ute
        E, E1 = _limexp(z)
        # Id = -Is_eff E(z)
        dUte, dBve = -Is_eff * E1 * (-z / Ute), -Is_eff * E1 * (-1.0 / Ute)
        L = math.log(Ibv / Is_eff)
        # Bv_eff = Bv - N Ut (ln Ibv - ln Is - ln Area): z = -(Bv + Ud) / Ute + ln Ibv - ln Is_eff, so d Id / d Is_eff with Bv_eff following is
        # -E + E1 -- written as that difference: below the linear continuation the breakdown current -Ibv exp(-(Bv + Ud) / Ute) does not
        # depend on Is or Area at all, and the sum of the two separately rounded terms of size E would leave noise of 1e-16 E
        dIse = E1 - E
        return {0: dIse * Area, 1: dUte * Ut + dBve * (-Ut * L), 2: 0.0, 3: 0.0,
                4: dUte * N * ct + dBve * (-N * ct * L), 5: dBve * (-N * Ut / Ibv), 6: dBve, 8: dIse * Is}, "breakdown"
    z, zr = Ud / Ute, Ud / Uter
    E, E1 = _limexp(z)
    Er, Er1 = _limexp(zr)
    # Id = Is_eff (E(z) - 1) + Isr_eff (E(zr) - 1)
    dIse, dIsre = E - 1.0, Er - 1.0
    dUte, dUter = Is_eff * E1 * (-z / Ute), Isr_eff * Er1 * (-zr / Uter)
    arm = "linear" if z > 50.0 else "forward"
    return {0: dIse * Area, 1: dUte * Ut, 2: dIsre * Area, 3: dUter * Ut, 4: dUte * N * ct + dUter * Nr * ct, 5: 0.0, 6: 0.0,
            8: dIse * Is + dIsre * Isr}, arm


def mos_derivatives(nmos, vd, vg, vs, Kp, lam, Vth):
    """{column: d (drain current as stamped: into D, out of S) / d p}, arm"""
    Vc = vg - vs if nmos else vs - vg
    Vx = vd - vs if nmos else vs - vd
    Vov = Vc - Vth
    sg = 1.0 if nmos else -1.0
    if Vov <= 0.0:
        return {0: 0.0, 1: 0.0, 2: 0.0}, "cutoff"
    if Vx < Vov:
        Bq = Vov * Vx - 0.5 * Vx * Vx
        return {0: sg * Bq * (1.0 + lam * Vx), 1: sg * Kp * Bq * Vx, 2: sg * (-Kp * Vx * (1.0 + lam * Vx))}, "triode"
    return {0: sg * 0.5 * Vov * Vov * (1.0 + lam * Vx), 1: sg * 0.5 * Kp * Vov * Vov * Vx, 2: sg * (-Kp * Vov * (1.0 + lam * Vx))}, "saturation"


def bjt_derivatives(Vj, Is, N, BetaF, Temp, Area):
    """({column: d Ij / d p}, {column: d (BetaF Ij) / d p}) of the forward-active Ebers-Moll junction current Ij = Is Area (exp(Vj / (N Ut)) - 1)"""
    Ut = K_B * (Temp - KELVIN) / Q_E
    Ute, Is_eff = N * Ut, Is * Area
    e = math.exp(Vj / Ute)
    Ij = Is_eff * (e - 1.0)
    dUte = Is_eff * e * (-Vj / (Ute * Ute))
    dj = {0: (e - 1.0) * Area, 1: dUte * Ut, 2: 0.0, 3: dUte * N * K_B / Q_E, 4: (e - 1.0) * Is}
    dc = {c: BetaF * v for c, v in dj.items()}
    dc[2] = Ij
    return dj, dc


def _row(n):
    return None if n < 0 else n - 1


def parameter_table(F, deck):
    """the table of include/pe_hip.h from the deck: list of dicts kind, index, column, dev (deck device, None for a junction of an FBR),
    pos (position in the deck's parameter tuple), value"""
    code = codes(F)
    out = []
    for want in ("R", "VDC", "IDC"):
        i = 0
        for di, (kind, nodes, par) in enumerate(deck.devices):
            if kind == want:
                out.append(dict(kind=code[want], index=i, column=0, dev=di, pos=0, value=par[0], name=want))
                i += 1
    i = 0
    for di, (kind, nodes, par) in enumerate(deck.devices):
        if kind == "D":
            for c in DIODE_COLS:
                out.append(dict(kind=code["D"], index=i, column=c, dev=di, pos=c, value=par[c], name="D"))
            i += 1
        elif kind == "FBR":
            for _ in range(4):
                for c in DIODE_COLS:
                    out.append(dict(kind=code["D"], index=i, column=c, dev=None, pos=c, value=FBR_DEFAULT[c], name="D"))
                i += 1
    for want in GENERIC_ORDER:
        i = 0
        for di, (kind, nodes, par) in enumerate(deck.devices):
            if kind != want:
                continue
            for c in range(3 if want in ("NMOS", "PMOS") else 5 if want in ("NPN", "PNP") else 1):
                out.append(dict(kind=code[want], index=i, column=c, dev=di, pos=c, value=par[c], name=want))
            i += 1
    return out


def residual_derivatives(F, deck, x):
    """(table, D [rows][n_params]) of d f / d p at x: column k holds d f / d p_k of f = A x - b; a device with an unconnected pin has a
    zero column.  arms: the set of model arms taken (returned third)."""
    N = deck.n_nodes
    tab = parameter_table(F, deck)
    rows = N + sum(NBRANCH.get(k, 0) for k, _, _ in deck.devices)
    D = np.zeros((rows, len(tab)))
    arms = set()
    v = lambda r: 0.0 if r < 0 else x[r]
    bydev = {(t["dev"], t["column"]): k for k, t in enumerate(tab) if t["dev"] is not None}
    bydiode = {(t["index"], t["column"]): k for k, t in enumerate(tab) if t["name"] == "D"}

    def put(k, r, val):
        if r >= 0:
            D[r, k] += val

    br = 0
    d_index = 0
    code = codes(F)
    for di, (kind, nodes, par) in enumerate(deck.devices):
        nb = NBRANCH.get(kind, 0)
        kb = [N + br + q for q in range(nb)]
        br += nb
        n = [_row(q) for q in nodes]
        connected = all(q is not None for q in n)
        col = lambda c, dev=di: bydev[(dev, c)]
        if kind == "FBR":
            A, Bn, P, M = n
            for (a, c) in ((A, P), (Bn, P), (M, A), (M, Bn)):
                dd, arm = diode_derivatives(FBR_DEFAULT, v(a) - v(c))
                arms.add("D " + arm)
                for cc in DIODE_COLS:
                    k = bydiode[(d_index, cc)]
                    put(k, a, dd[cc])
                    put(k, c, -dd[cc])
                d_index += 1
            continue
        if kind == "D":
            if connected:
                dd, arm = diode_derivatives(par, v(n[0]) - v(n[1]))
                arms.add("D " + arm)
                for cc in DIODE_COLS:
                    put(col(cc), n[0], dd[cc])
                    put(col(cc), n[1], -dd[cc])
            d_index += 1
            continue
        if not connected or kind not in code:
            continue
        if kind == "R":
            i_over_r = (v(n[0]) - v(n[1])) / (par[0] * par[0])
            put(col(0), n[0], -i_over_r)
            put(col(0), n[1], i_over_r)
        elif kind == "VDC":
            put(col(0), kb[0], -1.0)
        elif kind == "IDC":
            put(col(0), n[0], 1.0)
            put(col(0), n[1], -1.0)
        elif kind == "VCCS":
            put(col(0), n[0], v(n[2]) - v(n[3]))
            put(col(0), n[1], -(v(n[2]) - v(n[3])))
        elif kind == "VCVS":
            put(col(0), kb[0], -(v(n[2]) - v(n[3])))
        elif kind == "CCCS":
            put(col(0), n[0], x[kb[0]])
            put(col(0), n[1], -x[kb[0]])
        elif kind == "CCVS":
            put(col(0), kb[0], -x[kb[1]])
        elif kind == "OPAMP":
            put(col(0), kb[0], -(v(n[0]) - v(n[1])))
        elif kind == "XFMR":
            put(col(0), kb[0], -(v(n[2]) - v(n[3])))
            put(col(0), kb[1], x[kb[0]])
        elif kind == "XCT":
            if par[0] != 0.0:
                w = -1.0 / (2.0 * par[0] * par[0])   # d (1 / (2 n_total)) / d n_total
                put(col(0), kb[1], -(v(n[0]) - v(n[1])) * w)
                put(col(0), kb[2], -(v(n[0]) - v(n[1])) * w)
                put(col(0), kb[0], (x[kb[1]] + x[kb[2]]) * w)
        elif kind in ("NMOS", "PMOS"):
            dd, arm = mos_derivatives(kind == "NMOS", v(n[0]), v(n[1]), v(n[2]), *par[:3])
            arms.add(kind + " " + arm)
            for cc in range(3):
                put(col(cc), n[0], dd[cc])
                put(col(cc), n[2], -dd[cc])
        elif kind in ("NPN", "PNP"):
            npn = kind == "NPN"
            Vj = v(n[0]) - v(n[2]) if npn else v(n[2]) - v(n[0])
            dj, dc = bjt_derivatives(Vj, *par[:5])
            sg = 1.0 if npn else -1.0   # NPN: Ij into B, BetaF Ij into C, both out of E; PNP: mirrored
            for cc in range(5):
                put(col(cc), n[0], sg * dj[cc])
                put(col(cc), n[1], sg * dc[cc])
                put(col(cc), n[2], -sg * (dj[cc] + dc[cc]))
    return tab, D, arms


def set_oracle(O, deck, x, g_min=0.0):
    """an oracle prepared and SET to x (the junction limiter starts from x: it passes x through)"""
    o = O.Oracle(deck, g_min=g_min)
    o.prepare()
    o.x = np.array(x, dtype=float)
    if o.dio is not None:
        o.dio.Ud_last = o._dio_vd().copy()
    return o


def _selector(rows, pos, neg):
    e = np.zeros(rows)
    if pos >= 0:
        e[pos] += 1.0
    if neg >= 0:
        e[neg] -= 1.0
    return e


def slope_correction(deck, x):
    """What the true Jacobian of f has more than the stamped matrix, as a dense [rows][rows] array.  Two arms of the models stamp a
    conductance that is not the slope of the current they stamp: a PMOS stamps gds = -d Isd / d Vsd and +gm where the slopes of its
    drain current are +d Isd / d Vsd and -gm (the reference's pmosfet.h, mirrored by pe_front.hpp), and a junction on the linear continuation of the
    limited exponential stamps Is limexp(z) / Ute where the slope is Is exp(50) / Ute.  Newton's iteration keeps its fixed point but
    converges only linearly there (a PMOS in saturation by 2 gds R per step; in triode it moves away from the fixed point).  The analysis
    uses the stamped matrix, like every small-signal analysis of the engine (include/pe_hip.h says so); difference quotients see the
    true one, so on those arms fd_check compares them with the reference on the corrected matrix."""
    N = deck.n_nodes
    rows = N + sum(NBRANCH.get(k, 0) for k, _, _ in deck.devices)
    dJ = np.zeros((rows, rows))
    v = lambda r: 0.0 if r < 0 else x[r]

    def g4(a, c, g):
        for r, cc, sg in ((a, a, 1.0), (a, c, -1.0), (c, a, -1.0), (c, c, 1.0)):
            if r >= 0 and cc >= 0:
                dJ[r, cc] += sg * g

    for kind, nodes, par in deck.devices:
        n = [_row(q) for q in nodes]
        if any(q is None for q in n):
            continue
        if kind == "PMOS":
            Kp, lam, Vth = par[:3]
            Vc, Vx = v(n[2]) - v(n[1]), v(n[2]) - v(n[0])
            Vov = Vc - Vth
            if Vov <= 0.0:
                continue
            dI = Kp * ((Vov - Vx) * (1.0 + lam * Vx) + (Vov * Vx - 0.5 * Vx * Vx) * lam) if Vx < Vov else 0.5 * Kp * Vov * Vov * lam
            g4(n[0], n[2], 2.0 * dI)                      # stamped -dI, true +dI
            gm = Kp * (Vx if Vx < Vov else Vov) * (1.0 + lam * Vx)
            # stamped: +gm (v_S - v_G) into D, out of S; the drain current -Isd falls with v_S - v_G: true -gm
            for r, cc, sg in ((n[0], n[2], 1.0), (n[0], n[1], -1.0), (n[2], n[2], -1.0), (n[2], n[1], 1.0)):
                if r >= 0 and cc >= 0:
                    dJ[r, cc] += sg * (-2.0 * gm)
        elif kind == "D":
            Is, Nn, _, _, Temp, _, _, Bv_set, Area, _ = par
            Ute = Nn * K_B * (Temp - KELVIN) / Q_E
            z = (v(n[0]) - v(n[1])) / Ute
            if z > 50.0 and Bv_set == 0.0:
                E, E1 = _limexp(z)
                g4(n[0], n[1], Is * Area * (E1 - E) / Ute)
    return dJ


def reference(F, O, deck, x, mode, outputs, g_min=0.0, slopes=False):
    """outputs: [(pos, neg)].  Returns dict: table, p [k], s [o][k] (direct method), adj [o][k] (transposed), bound [o][k], y [o][rows], D, arms.
    slopes: on the matrix with slope_correction added (fd_check only: never what the engine is compared with)"""
    o = set_oracle(O, deck, x, g_min)
    J, _ = o.assemble(mode)
    if slopes:
        J = sp.csc_matrix(J.toarray() + slope_correction(deck, o.x))
    tab, D, arms = residual_derivatives(F, deck, o.x)
    assert D.shape[0] == o.rows
    lu = spla.splu(sp.csc_matrix(J), permc_spec="COLAMD", diag_pivot_thresh=1.0)
    dx = lu.solve(-D) if D.shape[1] else np.zeros((o.rows, 0))
    lut = spla.splu(sp.csc_matrix(J.T), permc_spec="COLAMD", diag_pivot_thresh=1.0)
    s, adj, bound, ys = [], [], [], []
    for pos, neg in outputs:
        e = _selector(o.rows, pos, neg)
        y = lut.solve(e)
        s.append(e @ dx)
        adj.append(-(y @ D))
        bound.append((1e-9 + 1e-6 * np.abs(y)) @ np.abs(D))
        ys.append(y)
    return {"table": tab, "p": np.array([t["value"] for t in tab]), "s": np.array(s), "adj": np.array(adj), "bound": np.array(bound), "y": np.array(ys),
            "D": D, "arms": arms}


def check(s, ref, what="", normalized=False):
    """engine sensitivities [n_outputs][n_params] of one instance against reference(); prints the worst figure, then asserts"""
    r, b = ref["s"], ref["bound"]
    scale = np.max(np.abs(r), axis=1) if r.shape[1] else np.zeros(len(r))
    gap = float(np.max(np.max(np.abs(r - ref["adj"]), axis=1) / np.where(scale > 0, scale, 1.0))) if r.size else 0.0
    print(what, "direct vs transposed reference:", gap)
    assert gap <= 1e-12, (what, gap)
    if normalized:
        r, b = r * ref["p"], b * np.abs(ref["p"])
    nz = b > 0
    print(what, "sensitivities: worst |d| / bound =", float(np.max(np.abs(s - r)[nz] / b[nz])) if nz.any() else 0.0)
    assert s.shape == r.shape, (s.shape, r.shape)
    assert np.all(np.abs(s - r) <= b), (what, np.argwhere(np.abs(s - r) > b)[:8], s[np.abs(s - r) > b][:8], r[np.abs(s - r) > b][:8])
    return r, b


def rss_reference(r, b, w):
    """(rss [o], its bound [o]) from (possibly normalised) reference sensitivities and bounds"""
    w2 = np.asarray(w, dtype=float) ** 2
    return (w2 * r * r).sum(axis=1), (w2 * ((np.abs(r) + b) ** 2 - r * r)).sum(axis=1)


def exercised(ref):
    """set of (kind, column) with an output where |s_k| >= 1000 bound_k"""
    big = np.any((np.abs(ref["s"]) >= 1000.0 * ref["bound"]) & (ref["bound"] > 0), axis=0)
    return {(t["kind"], t["column"]) for t, ok in zip(ref["table"], big) if ok}


def oracle_solution(O, deck, mode, warm=None, g_min=0.0, strict=True, polish=3):
    """the oracle's own solution converged to rounding (the fixed point the difference quotients are formed around)"""
    o = O.Oracle(deck, g_min=g_min)
    o.prepare()
    if warm is not None:
        o.x = np.array(warm, dtype=float)
        if o.dio is not None:
            o.dio.Ud_last = o._dio_vd().copy()
    it = o.solve(mode)
    if it <= 0 and not strict:
        return None
    assert it > 0, it
    # from the converged point Newton's steps shrink quadratically: three more leave x at rounding level (a fixed count, not a criterion that
    # rounding noise on a large deck could keep from ever being met).  polish: more of them where the iteration converges only linearly
    # (slope_correction)
    for _ in range(polish if o.nonlinear else 0):
        assert o.solve_once(mode)
    return o.x.copy()


def perturbed(deck, t, value):
    d = copy.deepcopy(deck)
    kind, nodes, par = d.devices[t["dev"]]
    par = list(par)
    par[t["pos"]] = value
    d.devices[t["dev"]] = (kind, nodes, tuple(par))
    return d


def fd_check(F, O, deck, mode, outputs, warm=None, g_min=0.0, what="", slopes=False, polish=3):
    """the restated derivatives against central differences of fully re-converged oracle solves; returns the set of (kind, column) checked.
    A column whose perturbed circuit does not converge (a zero saturation current stepped by -1e-6) is not checked here."""
    x0 = oracle_solution(O, deck, mode, warm, g_min, polish=polish)
    ref = reference(F, O, deck, x0, mode, outputs, g_min, slopes)
    checked = set()
    worst = 0.0
    for k, t in enumerate(ref["table"]):
        if t["dev"] is None:
            continue
        fd = []
        for h in (1e-4, 5e-5):
            step = h * abs(t["value"]) if t["value"] != 0.0 else 1e-6 * (h / 1e-4)
            xs = [oracle_solution(O, perturbed(deck, t, t["value"] + sg * step), mode, x0, g_min, strict=False, polish=polish) for sg in (1.0, -1.0)]
            if xs[0] is None or xs[1] is None:
                break
            fd.append(np.array([((xs[0][p] if p >= 0 else 0.0) - (xs[0][n] if n >= 0 else 0.0)) - ((xs[1][p] if p >= 0 else 0.0) - (xs[1][n] if n >= 0 else 0.0))
                                for p, n in outputs]) / (2.0 * step))
        if len(fd) < 2:
            continue
        for oi in range(len(outputs)):
            allow = 2.0 * abs(fd[0][oi] - fd[1][oi]) + ref["bound"][oi][k]
            sk = ref["s"][oi][k]
            if allow < 1e-3 * abs(sk):
                checked.add((t["kind"], t["column"]))
                worst = max(worst, abs(sk - fd[1][oi]) / allow)
                assert abs(sk - fd[1][oi]) <= allow, (what, t, oi, sk, fd[0][oi], fd[1][oi], allow)
    print(what, "restated derivatives vs central differences: worst |d| / allowance =", worst, "columns checked:", len(checked))
    return checked, ref


# ---- decks of the tests that the project's deck module does not have
def diode_recombination(pe):
    """VDC 0.6 V - R 1k - junction with Isr = 1e-9, Nr = 2, Area = 2 to ground: both exponentials carry current"""
    d = pe.deck.Deck()
    d.n_nodes = 2
    d.add("VDC", (1, 0), 0.6)
    d.add("R", (1, 2), 1000.0)
    d.add("D", (2, 0), 1e-14, 1.0, 1e-9, 2.0, 27.0, 1e-3, 40.0, 0.0, 2.0, 0.0)
    return d, [0.6, 0.45, -1e-4]


def diode_breakdown(pe):
    """VDC 10 V - R 1k - reversed junction with Bv = 5 V set: biased beyond -Bv_eff (columns Ibv, Bv, and the Bv_eff chain of Is, N, Temp, Area)"""
    d = pe.deck.Deck()
    d.n_nodes = 2
    d.add("VDC", (1, 0), 10.0)
    d.add("R", (1, 2), 1000.0)
    d.add("D", (0, 2), 1e-14, 1.0, 0.0, 2.0, 27.0, 1e-3, 5.0, 1.0, 1.0, 0.0)
    return d, [10.0, 5.04, -4.96e-3]


def diode_linear_arm(pe):
    """VDC 3 V - R 1k - junction with Is = 1e-25: Ud / (N Ut) > 50, the linear continuation of the limited exponential"""
    d = pe.deck.Deck()
    d.n_nodes = 2
    d.add("VDC", (1, 0), 3.0)
    d.add("R", (1, 2), 1000.0)
    d.add("D", (2, 0), 1e-25, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 0.0, 1.0, 0.0)
    return d, [3.0, 1.35, -1.65e-3]


def unconnected_pins(pe):
    """nmos_common_source with an R, a junction and a MOSFET that each have an unconnected pin: place kept, reads 0"""
    d = pe.deck.nmos_common_source(2.0)
    d.add("R", (1, -1), 50.0)
    d.add("D", (-1, 0))
    d.add("NMOS", (1, -1, 0), 1e-3, 0.0, 1.0)
    d.add("R", (1, 0), 5000.0)
    return d


def controlled_mix_biased(pe):
    """controlled_mix with 5 mA into its input node: at the operating point its VAC is a short, so without a bias every row is 0 and
    every sensitivity with it"""
    d = pe.deck.controlled_mix()
    d.add("IDC", (0, 2), 5e-3)
    return d


def op_amp_low_gain(pe):
    """op_amp_follower with mu = 10: d vout / d mu = Vin / (1 + mu)^2 is 1e-12 at the deck's own 1e6, far below the tolerance"""
    d = pe.deck.Deck()
    d.n_nodes = 2
    d.add("VDC", (1, 0), 1.0)
    d.add("OPAMP", (1, 2, 2, 0), 10.0)
    d.add("R", (2, 0), 1000.0)
    return d


def pe_oracle():
    import pe_load
    return pe_load.load_oracle()


def pmos_common_source(pe, vg=2.0):
    """the mirror of nmos_common_source: every source and pin voltage negated, PMOS instead of NMOS"""
    src = pe.deck.nmos_common_source(vg)
    d = pe.deck.Deck()
    d.n_nodes = src.n_nodes
    for kind, nodes, par in src.devices:
        if kind in ("VDC", "IDC"):
            d.add(kind, nodes, -par[0])
        elif kind == "NMOS":
            d.add("PMOS", nodes, *par)
        else:
            d.add(kind, nodes, *par)
    return d


# ---- the shared cases (emulation: one child process each; GPU: in-process)
MODES = {"OP": 0, "DC": 1, "TROP": 5}  # pe_hip_analysis_mode


def mesh(pe, w, seed):
    """rc_mesh(w, w, seed, True) with the 0.4 mA bias current of the noise tests into the node next to its centre"""
    d = pe.deck.rc_mesh(w, w, seed, True)
    d.add("IDC", (0, (w // 2) * w + w // 2 + 1), 4e-4)
    return d


def cases(pe):
    """name -> (deck, warm start or None, mode)"""
    D = pe.deck
    out = {"diode_op": (D.diode_op(), None, "OP")}
    for f in (diode_recombination, diode_breakdown, diode_linear_arm):
        d, w = f(pe)
        out[f.__name__] = (d, w, "OP")
    for vg, arm in ((0.5, "cutoff"), (2.0, "saturation"), (4.5, "triode")):
        out["nmos_" + arm] = (D.nmos_common_source(vg), None, "OP")
        # (mirrored start: the PMOS stage starts from the negated solution of the NMOS one)
        out["pmos_" + arm] = (pmos_common_source(pe, vg), lambda vg=vg: -oracle_solution(pe_oracle(), D.nmos_common_source(vg), "OP"), "OP")
    out["bjt_npn"] = (D.bjt_common_emitter(False), [5.0, 0.69, 0.7, 0.0], "OP")
    out["bjt_pnp"] = (D.bjt_common_emitter(True), [-5.0, -0.69, -0.7, 0.0], "OP")
    out["controlled_mix_op"] = (D.controlled_mix(), None, "OP")
    out["controlled_mix_trop"] = (D.controlled_mix(), None, "TROP")
    out["controlled_mix_biased"] = (controlled_mix_biased(pe), None, "OP")
    for name in ("ac_controlled_rest", "ccvs_dc", "cccs_dc", "vccs_dc", "vcvs_gain", "op_amp_follower", "transformer_ratio", "center_tap_ratio",
                 "bridge_rectifier"):
        out[name] = (getattr(D, name)(), None, "OP")
    out["op_amp_low_gain"] = (op_amp_low_gain(pe), None, "OP")
    out["unconnected_pins"] = (unconnected_pins(pe), None, "OP")
    out["mesh12"] = (mesh(pe, 12, 1), None, "OP")
    return out


def outputs_of(deck):
    """a node row, a branch row (when there is one) and a difference of two rows"""
    N = deck.n_nodes
    out = [(N - 1, -1)]
    if deck.n_branches:
        out.append((N, -1))
    if N >= 2:
        out.append((0, N - 1))
    return out


def engine(pe, deck, warm=None, mode="OP", batch=1, overrides=None, knobs=None, g_min=0.0, settle=True):
    """an engine converged with the tight tolerances and solved once more from the converged point"""
    F = pe.ffi
    e = F.Engine()
    e.set_options(g_min=g_min, **TIGHT)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    if warm is not None:
        e.set_solution(np.array([warm] * batch, dtype=float))
    e.analyze_dc(MODES[mode])
    if settle:
        e.analyze_dc(MODES[mode])
    return e


def table_of(e):
    t = e.sens_params()
    return list(zip(t["kind"].tolist(), t["index"].tolist(), t["column"].tolist()))


def parity(pe, O, deck, outputs, warm=None, mode="OP", what="", knobs=None):
    """one call with every sensitivity kept against the reference at the engine's own solution; returns (engine, reference, s)"""
    F = pe.ffi
    if callable(warm):
        warm = warm()
    e = engine(pe, deck, warm, mode, knobs=knobs)
    ref = reference(F, O, deck, e.solution()[0], mode, outputs)
    assert [(t["kind"], t["index"], t["column"]) for t in ref["table"]] == table_of(e), what
    s, rss, status, st = e.analyze_sens([p for p, _ in outputs], [n for _, n in outputs])
    assert rss is None and list(status) == [0] * len(outputs), (what, status)
    assert st["n_retried_outputs"] == 0 and st["n_analyses"] == 1 and st["n_params"] == len(ref["table"]) and st["n_outputs"] == len(outputs), (what, st)
    check(s[:, 0, :], ref, what)
    return e, ref, s


def run_case(pe, O, name):
    deck, warm, mode = cases(pe)[name]
    e, ref, s = parity(pe, O, deck, outputs_of(deck), warm, mode, name)
    if name == "unconnected_pins":
        tab = ref["table"]
        dead = [k for k, t in enumerate(tab) if (t["name"], t["index"]) in (("R", 1), ("D", 0), ("NMOS", 1))]
        assert len(dead) == 1 + 8 + 3 and np.all(s[:, 0, dead] == 0.0), s[:, 0, dead]
        live = [k for k, t in enumerate(tab) if (t["name"], t["index"]) == ("R", 2)]
        assert np.any(s[:, 0, live] != 0.0)
    return e, ref, s


def all_pairs(F):
    """every (kind, column) the table can hold"""
    c = codes(F)
    out = {(c[k], 0) for k in ("R", "VDC", "IDC", "VCCS", "VCVS", "CCCS", "CCVS", "OPAMP", "XFMR", "XCT")}
    out |= {(c["D"], col) for col in DIODE_COLS}
    out |= {(c[k], col) for k in ("NMOS", "PMOS") for col in range(3)}
    out |= {(c[k], col) for k in ("NPN", "PNP") for col in range(5)}
    return out


def _fma(a, b, c):
    """correctly rounded a b + c (exact rational arithmetic, one rounding)"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def rss_in_order(s, w, team, chunk=2048):
    """sum_k (w_k s_k)^2 in the order of include/pe_hip.h / pe_sens.hpp for a workgroup of `team` threads (1: the builds without HIP; 256:
    the device): per chunk of `chunk` parameters every thread forms acc = fma(t, t, acc) over its strided ascending subsequence, the 64
    lanes of a wavefront combine by the shuffle-down tree (offsets 32 .. 1), the wavefronts in order, then the chunks in order"""
    t = np.asarray(w, dtype=float) * np.asarray(s, dtype=float)
    total, first = 0.0, True
    n_chunks = max(1, -(-len(t) // chunk))
    for c in range(n_chunks):
        lo, hi = c * chunk, min((c + 1) * chunk, len(t))
        acc = np.zeros(max(team, 64))
        for th in range(team):
            a = 0.0
            for k in range(lo + th, hi, team):
                a = _fma(t[k], t[k], a)
            acc[th] = a
        waves = []
        for w0 in range(0, max(team, 64), 64):
            lane = acc[w0:w0 + 64].copy()
            for o in (32, 16, 8, 4, 2, 1):
                lane[:64 - o] = lane[:64 - o] + lane[o:]      # (lanes past 64 - o keep their own value: they never reach lane 0)
            waves.append(lane[0])
        if team == 1:
            waves = [acc[0]]
        part = waves[0]
        for v in waves[1:]:
            part = part + v
        if n_chunks == 1:
            return part
        total = part if first else total + part
        first = False
    return total
