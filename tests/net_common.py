"""Reference, tolerances and cases of the network-analysis tests (tests/test_net_emu.py on the host emulation, tests/test_gpu_net.py on the
device): numpy / scipy over the unchanged CPU oracle (oracle/pe_oracle.py), by the definitions of include/pe_hip.h.

Reference.  Per omega the oracle's complex AC stamp (tests/noise_common.py builds it into a scipy matrix) is factored once and solved for
all selector columns E (e_j: +1 at pos_j, -1 at neg_j); Z[i][j] = X[pos_i][j] - X[neg_i][j]; Y = Z^-1 and
S = D^-1 (Z - Z0) (Z + Z0)^-1 D in numpy complex128.

Tolerances are derived, not chosen.  The project's AC tolerance bounds every phasor: e_r = 1e-9 + 1e-6 |x_r| (tests/test_gpu_parity.py
test_ac_golden_parity), so Z_ij may be off by E_ij = e_pos + e_neg (column j's phasors; a ground terminal adds nothing).  To first order,
with entrywise moduli and the factor 2 that covers the higher-order terms while |Y| E and |W| E stay below 1/2:
    |dY| <= 2 |Y| E |Y|
    |dS| <= 2 |D^-1| (E |W| + |Z - Z0| |W| E |W|) |D|,   W = (Z + Z0)^-1.

Conversion alone (pe_hip_convert_net): reference mpmath at 50 digits; an inverse X of M computed by Gaussian elimination with partial
pivoting in binary64 is allowed 8 (n + 2)^2 2^-52 kappa_inf(M) max(1, max |X|) per entry.  S = I - 2 D W D inherits the bound of W times
2 sqrt(z0_i z0_j), plus four roundings of forming it.

Every case is a function of (pe, O, knobs): the emulation test runs it in a child process, the GPU test in its own."""
import numpy as np
import scipy.sparse.linalg as spla

import noise_common as NC

EPS = 2.0 ** -52


def split_ports(ports):
    p = np.asarray(ports, dtype=int).reshape(-1, 2)
    return p[:, 0], p[:, 1]


def convert(Z, z0):
    """numpy complex128: (Y or None when Z is singular to numpy, S, W)"""
    z0 = np.asarray(z0, dtype=float)
    Z0, D, Di = np.diag(z0), np.diag(np.sqrt(z0)), np.diag(1.0 / np.sqrt(z0))
    W = np.linalg.inv(Z + Z0)
    S = Di @ (Z - Z0) @ W @ D
    try:
        Y = np.linalg.inv(Z)
    except np.linalg.LinAlgError:
        Y = None
    return Y, S, W


def reference(o, omegas, ports, z0, with_y=True):
    """dict of arrays over the points: Z, EZ, S, ES and (with_y) Y, EY -- the E* are the entrywise bounds"""
    pos, neg = split_ports(ports)
    n = len(pos)
    z0 = np.broadcast_to(np.asarray(50.0 if z0 is None else z0, dtype=float), (n,))
    out = {k: [] for k in ("Z", "EZ", "Y", "EY", "S", "ES")}
    for w in omegas:
        M = NC._matrix(o, w)
        E = np.zeros((o.rows, n), dtype=complex)
        for j in range(n):
            if pos[j] >= 0:
                E[pos[j], j] += 1.0
            if neg[j] >= 0:
                E[neg[j], j] -= 1.0
        X = spla.splu(M, permc_spec="COLAMD", diag_pivot_thresh=1.0).solve(E)
        err = 1e-9 + 1e-6 * np.abs(X)
        Z = NC._at(X, pos) - NC._at(X, neg)
        EZ = np.where((pos >= 0)[:, None], err[np.maximum(pos, 0)], 0.0) + np.where((neg >= 0)[:, None], err[np.maximum(neg, 0)], 0.0)
        Y, S, W = convert(Z, z0)
        D, Di = np.diag(np.sqrt(z0)), np.diag(1.0 / np.sqrt(z0))
        aW = np.abs(W)
        ES = 2.0 * Di @ (EZ @ aW + np.abs(Z - np.diag(z0)) @ aW @ EZ @ aW) @ D
        out["Z"].append(Z); out["EZ"].append(EZ); out["S"].append(S); out["ES"].append(ES)
        if with_y:
            out["Y"].append(Y); out["EY"].append(2.0 * np.abs(Y) @ EZ @ np.abs(Y))
    return {k: np.array(v) for k, v in out.items() if len(v)}


def check(Z, Y, S, ref, what="", with_y=True):
    """one instance's matrices [n_points][n][n] against reference(): prints the worst |d| / bound of each kind, then asserts"""
    worst = {}
    for name, got, want, bound in (("Z", Z, ref["Z"], ref["EZ"]), ("S", S, ref["S"], ref["ES"])) + ((("Y", Y, ref["Y"], ref["EY"]),) if with_y else ()):
        worst[name] = float(np.max(np.abs(got - want) / bound))
    print(what, "worst |d| / bound:", worst)
    for name, v in worst.items():
        assert v <= 1.0, (what, name, v)      # (a NaN fails too)
    return worst


# ---- engines

def oracle(O, deck, warm=None):
    o = O.Oracle(deck, g_min=0.0)
    o.prepare()
    if warm is not None:
        o.x = np.array(warm, dtype=float)
    it = o.solve("OP") if o.nonlinear else 0
    assert it >= 0, it
    return o


def engine(pe, deck, batch=1, overrides=None, knobs=None, op=None):
    F = pe.ffi
    e = F.Engine()
    e.set_options(g_min=0.0)
    for k, v in (knobs or {}).items():
        if v is not None:
            e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    if deck.has_nonlinear() if op is None else op:
        e.analyze_dc(F.MODE_OP)
    return e


def counts_ok(st, n_ports):
    """the point of the feature: one factorisation per pass, the other ports on kept factors"""
    assert st["n_factorisations"] == st["n_passes"], st
    assert st["n_solves"] >= (n_ports - 1) * st["n_passes"], st


# ---- parity

W5 = [0.0, 1e2, 1e4, 1e6, 1e8]
MESH6_PORTS = [(1, -1), (5, -1), (20, -1), (30, 17)]
MESH6_Z0 = [50.0, 50.0, 50.0, 100.0]
MESH6_W = [0.0, 1e7, 1e9, 1e11]
MESH16_PORTS = [(0, -1), (37, -1), (75, -1), (110, -1), (148, -1), (187, -1), (222, -1), (255, -1)]
MESH16_W = list(np.logspace(9.0, 9.9, 6))
PARITY = ("ac_linear_mix", "ac_nmos_amp", "mesh6_batch3", "mesh16_ports8")


def parity(pe, O, name, knobs=None):
    if name == "ac_linear_mix":       # non-reciprocal: a transposed result fails
        deck, ports, z0, w, seeds = pe.deck.ac_linear_mix(), [(0, -1), (6, -1), (7, 0)], [50.0, 75.0, 600.0], W5, None
    elif name == "ac_nmos_amp":       # active and non-reciprocal
        deck, ports, z0, w, seeds = pe.deck.ac_nmos_amp(), [(2, -1), (4, -1)], None, W5, None
    elif name == "mesh6_batch3":
        deck, ports, z0, w, seeds = None, MESH6_PORTS, MESH6_Z0, MESH6_W, ([1, 2, 3], 6)
    elif name == "mesh16_ports8":     # the maximum number of ports, one band, front classes the small mesh does not reach
        deck, ports, z0, w, seeds = None, MESH16_PORTS, None, MESH16_W, ([1, 2], 16)
    else:
        raise KeyError(name)
    if seeds is None:
        e = engine(pe, deck, knobs=knobs)
        decks = [deck]
    else:
        sd, side = seeds
        base, r, c = pe.deck.rc_mesh_params(side, side, sd, True)
        e = engine(pe, pe.deck.rc_mesh(side, side, sd[0], True), batch=len(sd), overrides={"R": r[:, :, None], "C": c[:, :, None]}, knobs=knobs)
        decks = [pe.deck.rc_mesh(side, side, s, True) for s in sd]
    try:
        Z, Y, S, ys, ss, ps, st = e.analyze_net(w, ports, z0)
    finally:
        e.close()
    print(name, knobs, st)
    n = len(ports)
    assert list(ps) == [0] * len(w) and st["n_retried_points"] == 0 and st["n_points"] == len(w) and st["n_ports"] == n, (ps, st)
    assert st["n_analyses"] == NC.bands(w), st
    assert not ys.any() and not ss.any(), (ys, ss)
    counts_ok(st, n)
    if knobs and knobs.get("NET_POINTS"):
        assert st["points_per_pass"] <= knobs["NET_POINTS"], st
    for b, d in enumerate(decks):
        ref = reference(oracle(O, d), w, ports, z0)
        check(Z[:, b], Y[:, b], S[:, b], ref, "%s instance %d" % (name, b))
    if name == "ac_linear_mix":
        assert np.max(np.abs(Z[2, 0] - Z[2, 0].T)) > 1e3 * np.max(reference(oracle(O, decks[0]), w[2:3], ports, z0)["EZ"]), "the case must be able to tell a transpose"
    if len(decks) > 1:
        assert not np.array_equal(Z[:, 0], Z[:, 1]), "the instances differ"
    return st


# ---- known answers

def known_answers(pe, O, knobs=None):
    F = pe.ffi
    R, Cap = 1000.0, 1e-6
    d = pe.deck.ac_rc_lowpass()
    o = oracle(O, d)
    w = [0.0, 1e3, 1e5]
    e = engine(pe, d, knobs=knobs)
    try:
        # one port at the capacitor: Z = R / (1 + j omega R C); 500 - 500j at omega = 1000
        Z, Y, S, ys, ss, ps, st = e.analyze_net(w, [(1, -1)])
        ref = reference(o, w, [(1, -1)], None)
        check(Z[:, 0], Y[:, 0], S[:, 0], ref, "lowpass one-port")
        cf = R / (1.0 + 1j * np.array(w) * R * Cap)
        assert np.all(np.abs(Z[:, 0, 0, 0] - cf) <= ref["EZ"][:, 0, 0]) and abs(cf[1] - (500 - 500j)) < 1e-9, (Z, cf)
        s11 = (cf - 50.0) / (cf + 50.0)
        assert np.all(np.abs(S[:, 0, 0, 0] - s11) <= ref["ES"][:, 0, 0]), (S, s11)
        assert list(ps) == [0, 0, 0] and not ys.any() and not ss.any()
        counts_ok(st, 1)
        # ports (row 0, gnd), (row 1, gnd): row 0 is held by the source -- Z has a zero row, Y does not exist, S does
        ports = [(0, -1), (1, -1)]
        Z, Y, S, ys, ss, ps, st = e.analyze_net(w, ports)
        ref = reference(o, w, ports, None, with_y=False)
        print("held node: Z[1] =", Z[1, 0].tolist(), "y_status", ys.T.tolist(), "s_status", ss.T.tolist())
        assert list(ps) == [0, 0, 0] and np.all(ys == F.ERR_SINGULAR) and not ss.any(), (ps, ys, ss)
        assert np.all(np.isnan(Y)) and np.all(np.isfinite(Z)) and np.all(np.isfinite(S))
        check(Z[:, 0], None, S[:, 0], ref, "lowpass held node", with_y=False)
        assert np.all(np.abs(Z[:, 0, 0, :]) <= ref["EZ"][:, 0, :]), "the zero row"
        counts_ok(st, 2)
    finally:
        e.close()
    # a single resistor R = z0 to ground as a one-port: matched
    dr = pe.deck.Deck()
    dr.n_nodes = 1
    dr.add("R", (1, 0), 75.0)
    e = engine(pe, dr, knobs=knobs)
    try:
        Z, Y, S, ys, ss, ps, st = e.analyze_net([0.0, 1e6], [(0, -1)], [75.0])
    finally:
        e.close()
    ref = reference(oracle(O, dr), [0.0, 1e6], [(0, -1)], [75.0])
    print("matched resistor: |S11| =", np.abs(S[:, 0, 0, 0]).tolist(), "bound", ref["ES"][:, 0, 0].tolist())
    assert np.all(np.abs(S[:, 0, 0, 0]) <= ref["ES"][:, 0, 0]) and np.all(np.abs(Z[:, 0, 0, 0] - 75.0) <= ref["EZ"][:, 0, 0])


# ---- properties

def properties(pe, O, knobs=None):
    knobs = dict(knobs or {})
    w = [0.0, 1e7, 3e7, 1e9, 2e9, 5e9, 1e11]
    deck = pe.deck.rc_mesh(6, 6, 1, True)
    o = oracle(O, deck)
    ref = reference(o, w, MESH6_PORTS, MESH6_Z0)
    assert np.max(np.abs(ref["Z"] - ref["Z"].transpose(0, 2, 1)) / np.abs(ref["Z"]).max()) <= 2e-15, "the reference is reciprocal there"
    res = {}
    for P in (1, 4, None):
        e = engine(pe, deck, knobs=dict(knobs, NET_POINTS=P))
        try:
            res[P] = e.analyze_net(w, MESH6_PORTS, MESH6_Z0)
        finally:
            e.close()
        st = res[P][6]
        assert list(res[P][5]) == [0] * len(w) and st["n_retried_points"] == 0, st
        counts_ok(st, 4)
        assert (st["points_per_pass"] == 1) if P == 1 else (st["points_per_pass"] <= 4 if P else st["points_per_pass"] > 1), (P, st)
    Z, Y, S = res[None][:3]
    # reciprocity of the diode-RC mesh within the propagated bound
    rec = np.abs(Z[:, 0] - Z[:, 0].transpose(0, 2, 1)) / (ref["EZ"] + ref["EZ"].transpose(0, 2, 1))
    print("reciprocity: worst |Z - Z^T| / bound =", float(rec.max()))
    assert rec.max() <= 1.0
    # bit-identical across the pass size
    for P in (1, 4):
        for a, b in zip(res[P][:5], res[None][:5]):
            assert np.array_equal(a, b, equal_nan=True), "pass size %d" % P
    # ... across batch positions
    e = engine(pe, deck, batch=3, knobs=knobs)
    try:
        Z3, Y3, S3 = e.analyze_net(w, MESH6_PORTS, MESH6_Z0)[:3]
    finally:
        e.close()
    for b in range(3):
        assert np.array_equal(Z3[:, b], Z[:, 0]) and np.array_equal(Y3[:, b], Y[:, 0]) and np.array_equal(S3[:, b], S[:, 0]), "batch position %d" % b
    # ... and with the ports permuted: rows and columns of Z permute exactly
    perm = [2, 0, 3, 1]
    e = engine(pe, deck, knobs=knobs)
    try:
        Zp = e.analyze_net(w, [MESH6_PORTS[k] for k in perm], [MESH6_Z0[k] for k in perm])[0]
    finally:
        e.close()
    assert np.array_equal(Zp[:, 0], Z[:, 0][:, perm][:, :, perm]), "permuted ports"
    # passivity of the linear RC decks: the largest singular value of S is at most 1 + bound
    for what, d, ports, z0, ws in (("lowpass", pe.deck.ac_rc_lowpass(), [(0, -1), (1, -1)], [50.0, 50.0], [0.0, 1e3, 1e5]),
                                   ("linear mesh", pe.deck.rc_mesh(6, 6, 1, False), MESH6_PORTS, MESH6_Z0, MESH6_W)):
        e = engine(pe, d, knobs=knobs)
        try:
            Sl = e.analyze_net(ws, ports, z0)[2][:, 0]
        finally:
            e.close()
        r = reference(oracle(O, d), ws, ports, z0, with_y=False)
        sv = np.array([np.linalg.svd(m, compute_uv=False)[0] for m in Sl])
        bound = np.array([np.linalg.norm(m, 2) for m in r["ES"]])     # ||dS||_2 <= || |dS| ||_2 <= ||ES||_2
        print("passivity", what, "sigma_max - 1 =", (sv - 1.0).tolist(), "bound", bound.tolist())
        assert np.all(sv <= 1.0 + bound), what


# ---- the conversion at its edges

def mp_convert(Z, z0):
    """mpmath at 50 digits: Y (None: singular), S (None: singular), kappa_inf and max |X| of both inversions"""
    import mpmath as mp
    mp.mp.dps = 50
    n = Z.shape[0]
    M = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            M[i, j] = mp.mpc(float(Z[i, j].real), float(Z[i, j].imag))
    out = []
    for which in (0, 1):
        A = M.copy()
        if which:
            for i in range(n):
                A[i, i] += mp.mpf(float(z0[i]))
        try:
            X = mp.inverse(A)
        except ZeroDivisionError:
            out.append(None)
            continue
        kappa = float(mp.mnorm(A, "inf") * mp.mnorm(X, "inf"))
        Xn = np.array([[complex(X[i, j]) for j in range(n)] for i in range(n)])
        if which:
            sq = [mp.sqrt(mp.mpf(float(v))) for v in z0]
            Sn = np.array([[complex((1 if i == j else 0) - 2 * sq[i] * X[i, j] * sq[j]) for j in range(n)] for i in range(n)])
            out.append((Sn, kappa, float(np.abs(Xn).max())))
        else:
            out.append((Xn, kappa, float(np.abs(Xn).max())))
    return out


def conversion_edges(pe):
    F = pe.ffi
    rng = np.random.default_rng(11)
    e = F.Engine()                                   # no circuit
    worst = 0.0
    try:
        def run(Zs, z0, what):
            nonlocal worst
            Zs = np.asarray(Zs, dtype=complex)
            n = Zs.shape[-1]
            Y, S, ys, ss = e.convert_net(Zs, z0)
            ref0 = np.broadcast_to(np.asarray(50.0 if z0 is None else z0, dtype=float), (n,))
            for m in range(Zs.shape[0]):
                (ry, rs) = mp_convert(Zs[m], ref0)
                for kind, got, stat, r in (("Y", Y[m], ys[m], ry), ("S", S[m], ss[m], rs)):
                    assert r is not None, (what, m, kind, "the reference is singular: use expect_singular")
                    X, kappa, mx = r
                    b = 8.0 * (n + 2) ** 2 * EPS * kappa * max(1.0, mx)
                    if kind == "S":
                        b = 2.0 * ref0.max() * b + 4.0 * EPS * max(1.0, float(np.abs(X).max()))
                    ratio = float(np.max(np.abs(got - X)) / b)
                    worst = max(worst, ratio)
                    assert stat == 0 and ratio <= 1.0, (what, m, kind, stat, ratio)
            return Y, S, ys, ss
        # n = 1, 2, 3, 8: random complex matrices with rows scaled over four decades; 1, 65 and 8 (two full workgroups) matrices
        for n in (1, 2, 3, 8):
            for n_mats in (1, 65, 8):
                Zs = (rng.normal(size=(n_mats, n, n)) + 1j * rng.normal(size=(n_mats, n, n))) * (10.0 ** rng.uniform(-1.0, 3.0, size=(n_mats, n, 1)))
                run(Zs, 50.0 if n != 3 else [50.0, 75.0, 600.0], "random n=%d mats=%d" % (n, n_mats))
        # Z[0][0] = 0, nonsingular: needs the row exchange
        run([[[0.0, 2.0 + 1j], [3.0 - 1j, 4.0]]], None, "zero leading entry")
        run([[[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [4.0, -3.0, 0.0]]], [50.0, 75.0, 600.0], "zero diagonal")
        # [[0, 50], [50, 0]]: Z inverts, Z + Z0 = [[50, 50], [50, 50]] does not
        Y, S, ys, ss = e.convert_net([[[0.0, 50.0], [50.0, 0.0]]], None)
        assert ys[0] == 0 and np.allclose(Y[0], [[0.0, 0.02], [0.02, 0.0]], rtol=0, atol=1e-17) and ss[0] == F.ERR_SINGULAR and np.all(np.isnan(S)), (Y, S, ys, ss)
        # exactly singular
        Y, S, ys, ss = e.convert_net([[[1.0, 2.0], [2.0, 4.0]], [[2.0, 0.0], [0.0, 2.0]]], None)
        assert ys[0] == F.ERR_SINGULAR and np.all(np.isnan(Y[0])) and ss[0] == 0 and np.all(np.isfinite(S[0])), (Y, S, ys, ss)
        assert ys[1] == 0 and np.array_equal(Y[1], [[0.5, 0.0], [0.0, 0.5]])
        # one NaN entry: status and NaN, and a finite neighbour in the same launch
        Zs = np.array([np.eye(3) * 10.0, np.eye(3) * 10.0, np.eye(3) * 20.0], dtype=complex)
        Zs[1, 0, 2] = np.nan
        Y, S, ys, ss = e.convert_net(Zs, None)
        assert list(ys) == [0, F.ERR_SINGULAR, 0] and list(ss) == [0, F.ERR_SINGULAR, 0], (ys, ss)
        assert np.all(np.isnan(Y[1])) and np.all(np.isnan(S[1])) and np.all(np.isfinite(Y[[0, 2]])) and np.all(np.isfinite(S[[0, 2]]))
        assert np.array_equal(Y[0], np.eye(3) * 0.1)
        # refusals
        lib = F.lib()
        z = np.zeros(4)
        for n, m, zr, zi, z0 in ((0, 1, z, z, None), (9, 1, z, z, None), (2, 0, z, z, None), (2, 1, None, z, None), (2, 1, z, None, None),
                                 (2, 1, z, z, np.array([50.0, 0.0])), (2, 1, z, z, np.array([50.0, np.inf])), (2, 1, z, z, np.array([-1.0, 50.0]))):
            rc = lib.pe_hip_convert_net(e._h, n, m, F._dp(zr) if zr is not None else None, F._dp(zi) if zi is not None else None,
                                        F._dp(z0) if z0 is not None else None, None, None, None, None, None, None)
            assert rc == F.ERR_ARG, (n, m, z0)
    finally:
        e.close()
    print("conversion: worst |d| / bound against mpmath =", worst)
    return worst


# ---- refusals, state and failures

def refusals_state_failures(pe, O, knobs=None):
    import ctypes as C
    F = pe.ffi
    lib = F.lib()
    deck = pe.deck.rc_mesh(6, 6, 1, True)
    e = engine(pe, deck, knobs=knobs)
    w = np.array(MESH6_W[1:])
    e.set_ac_sweep_rows([0, 17, 30])
    x, _, _ = e.analyze_ac_sweep(w)
    psd, _, _, _ = e.analyze_noise(w, 20, 5)
    Z, Y, S, ys, ss, ps, st = e.analyze_net(w, MESH6_PORTS, MESH6_Z0)
    # a stored forward sweep and a stored noise result read the same bits after a network call
    re = np.empty((len(w), 1, 3)); im = np.empty_like(re); out = np.empty((len(w), 1))
    assert lib.pe_hip_get_ac_sweep(e._h, 0, len(w), 0, 1, F._dp(re), F._dp(im)) == 0 and np.array_equal(re + 1j * im, x)
    assert lib.pe_hip_get_noise(e._h, 0, len(w), 0, 1, F._dp(out), None) == 0 and np.array_equal(out, psd)
    assert np.array_equal(e.analyze_ac_sweep(w)[0], x) and np.array_equal(e.analyze_noise(w, 20, 5)[0], psd)

    def stored():
        zr = np.empty((len(w), 1, 4, 4)); zi = np.empty_like(zr)
        rc = lib.pe_hip_get_net(e._h, F.NET_Z, 0, len(w), 0, 1, F._dp(zr), F._dp(zi))
        return rc, zr + 1j * zi
    assert stored()[0] == 0 and np.array_equal(stored()[1], Z)
    # every refusal leaves the engine unchanged
    n = e.rows
    stn = F.NetStats()

    def call(ws, ports, z0=None, ctl=True, n_ports=None, nullrows=False):
        ws = np.ascontiguousarray(ws, dtype=float)
        pos, neg = [np.ascontiguousarray(v, dtype=np.int32) for v in split_ports(ports)]
        ref = None if z0 is None else np.ascontiguousarray(z0, dtype=float)
        c = F.NetControl(len(pos) if n_ports is None else n_ports, None if nullrows else F._ip(pos), F._ip(neg), F._dp(ref) if ref is not None else None)
        return lib.pe_hip_analyze_net(e._h, len(ws), F._dp(ws), C.byref(c) if ctl else None, None, C.byref(stn))
    P = MESH6_PORTS
    bad = [dict(ws=[1e8, -1.0], ports=P), dict(ws=[float("nan")], ports=P), dict(ws=[float("inf")], ports=P), dict(ws=w, ports=P, ctl=False),
           dict(ws=w, ports=P, n_ports=0), dict(ws=w, ports=[(k, -1) for k in range(9)]), dict(ws=w, ports=P, nullrows=True),
           dict(ws=w, ports=[(n, -1)]), dict(ws=w, ports=[(0, n)]), dict(ws=w, ports=[(-2, 0)]), dict(ws=w, ports=[(3, 3)]), dict(ws=w, ports=[(-1, -1)]),
           dict(ws=w, ports=[(1, -1), (5, 2), (1, -1)]), dict(ws=w, ports=P, z0=[50.0, 0.0, 50.0, 50.0]), dict(ws=w, ports=P, z0=[50.0, -1.0, 50.0, 50.0]),
           dict(ws=w, ports=P, z0=[50.0, float("nan"), 50.0, 50.0]), dict(ws=w, ports=P, z0=[50.0, float("inf"), 50.0, 50.0])]
    for kw in bad:
        assert call(**kw) == F.ERR_ARG, kw
    pos, neg = [np.ascontiguousarray(v, dtype=np.int32) for v in split_ports(P)]
    ctl = F.NetControl(4, F._ip(pos), F._ip(neg), None)
    assert lib.pe_hip_analyze_net(e._h, 0, F._dp(w), C.byref(ctl), None, None) == F.ERR_ARG
    assert lib.pe_hip_analyze_net(e._h, 2, None, C.byref(ctl), None, None) == F.ERR_ARG
    assert stored()[0] == 0 and np.array_equal(stored()[1], Z), "the stored result survives the refused calls"
    assert np.array_equal(e.analyze_net(w, MESH6_PORTS, MESH6_Z0)[0], Z), "and a following call returns what it returned before"
    # what makes a stored noise result unreadable makes this one unreadable
    for name in ("analyze_dc", "update_param", "load_deck"):
        e.analyze_net(w, MESH6_PORTS, MESH6_Z0)
        assert stored()[0] == 0, name
        if name == "analyze_dc":
            e.analyze_dc(F.MODE_OP)
        elif name == "update_param":
            e.update_param(F.R, 0, 0, 1234.0)
        else:
            e.load_deck(deck, 1)
        assert stored()[0] == F.ERR_ARG and b"no network analysis yet" in lib.pe_hip_last_error(e._h), name
        yy = np.empty((len(w), 1), dtype=np.int32)
        assert lib.pe_hip_get_net_status(e._h, 0, len(w), 0, 1, F._ip(yy), None) == F.ERR_ARG, name
    e.close()
    # without a circuit
    f = F.Engine()
    assert lib.pe_hip_analyze_net(f._h, len(w), F._dp(w), C.byref(ctl), None, None) == F.ERR_ARG
    f.close()

    # failed operating point: the cold-start BJT deck of the noise tests
    e = F.Engine()
    e.set_options(g_min=0.0)
    e.load_deck(pe.deck.bjt_common_emitter(False))
    e.reset()
    op = e.analyze_dc(F.MODE_OP, check=False)
    assert op["rc"] != 0, "the cold start is expected to fail"
    Z, Y, S, ys, ss, ps, st = e.analyze_net(np.logspace(2.0, 7.0, 6), [(2, -1), (1, -1)], check=False)
    assert st["rc"] == op["rc"] and list(ps) == [op["rc"]] * 6 and np.all(ys == op["rc"]) and np.all(ss == op["rc"]), (st, ps)
    assert np.all(np.isnan(Z)) and np.all(np.isnan(Y)) and np.all(np.isnan(S))
    e.close()

    # a failing point: VAC - R - C - C, a port at the node between the capacitors -- the omega = 0 band is singular
    d = pe.deck.Deck()
    d.n_nodes = 3
    d.add("VAC", (1, 0), 1.0, 1000.0, 0.0)
    d.add("R", (1, 2), 1000.0)
    d.add("C", (2, 3), 1e-6)
    d.add("C", (3, 0), 2e-6)
    wf = np.array([0.0, 1e3, 0.0, 2e3, 1e5])
    good = [1, 3, 4]
    ports = [(2, -1), (1, -1)]
    ref = reference(oracle(O, d), wf[good], ports, None)
    for P in (4, None, 1):
        e = engine(pe, d, knobs=dict(knobs or {}, NET_POINTS=P))
        Z, Y, S, ys, ss, ps, st = e.analyze_net(wf, ports, check=False)
        assert st["rc"] == F.ERR_SINGULAR and list(ps) == [F.ERR_SINGULAR, 0, F.ERR_SINGULAR, 0, 0] and st["n_retried_points"] == 2, (P, st, ps)
        assert np.all(np.isnan(Z[[0, 2]])) and np.all(np.isnan(Y[[0, 2]])) and np.all(np.isnan(S[[0, 2]])), "a failed point reads NaN"
        assert np.all(ys[[0, 2]] == F.ERR_SINGULAR) and np.all(ss[[0, 2]] == F.ERR_SINGULAR) and not ys[good].any() and not ss[good].any()
        check(Z[good, 0], Y[good, 0], S[good, 0], ref, "failing points, P = %s" % P)
        Z2, _, _, _, _, ps2, st2 = e.analyze_net(wf[good], ports)            # and the engine goes on
        assert list(ps2) == [0, 0, 0] and st2["n_retried_points"] == 0 and np.array_equal(Z2, Z[good])
        e.close()

    # an overlay circuit is refused
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
    p1, n1 = np.array([1], dtype=np.int32), np.array([-1], dtype=np.int32)
    assert lib.pe_hip_analyze_net(g._h, len(w), F._dp(w), C.byref(F.NetControl(1, F._ip(p1), F._ip(n1), None)), None, None) == F.ERR_ARG
    assert b"overlay" in lib.pe_hip_last_error(g._h)
    g.close()


# ---- calls of different shapes on one engine

def shapes_on_one_engine(pe, O, knobs=None):
    """Two calls on one engine whose result planes have the same size (n_points x batch x n^2) and whose status arrays (n_points x batch)
    do not: the buffers of the first call must not be taken for those of the second.  8 ports x 1 point, then 1 port x 64 points; 2 ports
    x 1 point, then 1 port x 4 points; and back.  Every call reads what a fresh engine reads for it, bit for bit, with its statuses."""
    deck = pe.deck.rc_mesh(6, 6, 1, True)
    eight = [(k, -1) for k in (0, 4, 9, 13, 18, 22, 27, 35)]
    calls = [(eight, [1e9]), ([(20, -1)], list(np.logspace(9.0, 9.9, 64))), ([(1, -1), (30, 17)], [1e9]), ([(5, -1)], list(np.logspace(9.0, 9.9, 4))),
             (eight, [1e9])]

    def one(e, ports, w):
        Z, Y, S, ys, ss, ps, st = e.analyze_net(w, ports)
        assert list(ps) == [0] * len(w) and ys.shape == (len(w), 1) and not ys.any() and not ss.any(), (ps, ys, ss)
        return Z, Y, S
    e = engine(pe, deck, knobs=knobs)
    try:
        got = [one(e, ports, w) for ports, w in calls]
    finally:
        e.close()
    for (ports, w), g in zip(calls, got):
        f = engine(pe, deck, knobs=knobs)
        try:
            want = one(f, ports, w)
        finally:
            f.close()
        for a, b in zip(g, want):
            assert np.array_equal(a, b), (len(ports), len(w))
    ref = reference(oracle(O, deck), calls[1][1], calls[1][0], None)
    check(got[1][0][:, 0], got[1][1][:, 0], got[1][2][:, 0], ref, "1 port x 64 points after 8 ports x 1 point")


# ---- Touchstone

def touchstone_round_trip(pe, tmpdir):
    import os
    F = pe.ffi
    rng = np.random.default_rng(3)
    f = np.logspace(6.0, 9.0, 7)
    for n in (1, 2, 3, 5):
        S = rng.normal(size=(len(f), n, n)) + 1j * rng.normal(size=(len(f), n, n))
        path = os.path.join(tmpdir, "sweep.s%dp" % n)
        F.write_touchstone(path, f, S, [75.0] * n)
        nums, opt = [], None
        for line in open(path):
            line = line.split("!")[0].strip()
            if not line:
                continue
            if line.startswith("#"):
                opt = line[1:].split()
                continue
            nums += [float(t) for t in line.split()]
        assert [t.upper() for t in opt[:4]] == ["HZ", "S", "RI", "R"] and float(opt[4]) == 75.0, opt
        rec = np.array(nums).reshape(len(f), 1 + 2 * n * n)
        assert np.array_equal(rec[:, 0], f)                       # (repr prints round-trip precision: the comparison is exact)
        M = (rec[:, 1::2] + 1j * rec[:, 2::2]).reshape(len(f), n, n)
        if n == 2:
            M = M.transpose(0, 2, 1)                              # a 2-port file lists S11 S21 S12 S22
        assert np.array_equal(M, S), n
    for bad in ([50.0, 75.0], [50.0, float("nan")]):
        try:
            F.write_touchstone(os.path.join(tmpdir, "bad.s2p"), f, np.zeros((len(f), 2, 2)), bad)
        except ValueError:
            continue
        raise AssertionError("unequal reference resistances must raise ValueError")
