"""Reference, bounds and cases of the pole-zero tests (tests/test_pz_emu.py on the host emulation, tests/test_gpu_pz.py on the device), by the
definitions of include/pe_hip.h.

Truth.  G = Re A(j 1), B = Im A(j 1) from the unchanged CPU oracle's stamp_ac(1) (pencil() first asserts that stamp_ac(2) has the same
real part and exactly twice the imaginary part: the matrix is affine in omega).  The poles are s = s0 - omega0 / theta over the eigenvalues
theta of M' = A0^-1 (omega0 B), A0 = G + j omega0 B, computed by mpmath at 50 digits; the zeros the same on the bordered pencil
[[A(s), b], [c^T, 0]].  Eigenvalues with |theta| <= 1e-12 max |theta| are the infinite ones and are dropped (the definition of the
header).  The eigenvalues are computed a second time at 100 digits and a value is kept only if it is there again to 20 digits with a
condition number of at most KAPPA_CAP: a defective infinite eigenvalue shows up as a ring of values that moves with the working precision
(truth()), and those are no poles or zeros.  scipy's QZ on the pencil is NOT the truth: it is off by 4e-5 in the dominant pole of ac_linear_mix.

Bound per value.  |s - s_true| <= |s_true - s0| kappa_i (err_est_i + E): the first-order perturbation bound of a simple eigenvalue with
the Ritz residual as the backward error; kappa_i = |y_i| |x_i| / |y_i^H x_i| from mpmath's left and right eigenvectors of M'.  E is the
rounding of the operator (refined solve, block product, orthogonalisation).  It is measured, not derived: the worst
|s - s_true| / (kappa_i |s_true - s0|) over the converged poles of the parity cases of restate() -- a float64 numpy restatement of the same
iteration (LU with partial pivoting and one refinement round, classical Gram-Schmidt twice, LAPACK's eigenvalues of the Hessenberg matrix)
-- is E_MEASURED; the tests allow E = 16 E_MEASURED, because the kernels sum in another order and solve with the static-pivot LU.
measure_e() prints the figure again (scripts/pz_make_golden.py runs it).

The dense solver alone (pe_hip_eig_hessenberg): truth mpmath, bound kappa_i c m 2^-52 |H|_F, c = 8 x the worst ratio numpy.linalg.eigvals
(LAPACK) shows on the same matrices (C_LAPACK, measured by eig_cases(None)); last components are compared on simple eigenvalues only.

Worst |d| / bound seen: see WORST below and DESIGN.md.

Every case is a function of (pe, O, knobs): the emulation test runs it in a child process, the GPU test in its own."""
import ctypes as C
import hashlib
import json
import os

import mpmath as mp
import numpy as np
import scipy.linalg as sl

import net_common as N
import noise_common as NC

EPS = 2.0 ** -52
FLOOR = 1e-12
TOL = 1e-10
E_MEASURED = 8.8e-15     # measure_e(): worst |s - s_true| / (kappa |s_true - s0|) of restate() over the parity cases' converged poles
E = 16.0 * E_MEASURED
C_LAPACK_MEASURED = 0.85  # eig_cases(None): worst |theta - theta_true| / (kappa m 2^-52 |H|_F) of numpy.linalg.eigvals on the matrices of eig_cases
C_EIG = 8.0 * C_LAPACK_MEASURED
# worst |d| / bound seen (poles and zeros of every case; the dense solver alone)
WORST = {"emulation": {"pz": 0.085, "eig": 0.69}, "MI355X": {"pz": 0.099, "eig": 0.65}}   # (eig: of C_EIG = 6.8 allowed)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pz_mesh16_poles.json")
GOLDEN_EIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pz_eig_truth.json")
MESH16_W0 = 1e8
MESH16_SEEDS = [1, 2]
MESH6_PORTS = ((1, -1), (30, 17))
MESH6_W0 = 1e9


# ---- truth

def pencil(o):
    """(G, B) dense, after checking that the oracle's matrix is affine in omega"""
    A1, A2 = NC._matrix(o, 1.0).toarray(), NC._matrix(o, 2.0).toarray()
    assert np.array_equal(A1.real, A2.real) and np.array_equal(2.0 * A1.imag, A2.imag), "stamp_ac is not G + j omega B"
    return A1.real.copy(), A1.imag.copy()


def selectors(n, ports):
    (ip, ineg), (op, on) = ports
    b, c = np.zeros(n), np.zeros(n)
    for v, r, s in ((b, ip, 1.0), (b, ineg, -1.0), (c, op, 1.0), (c, on, -1.0)):
        if r >= 0:
            v[r] += s
    return b, c


def bordered(G, B, ports):
    n = len(G)
    b, c = selectors(n, ports)
    Gb = np.block([[G, b[:, None]], [c[None, :], np.zeros((1, 1))]])
    Bb = np.block([[B, np.zeros((n, 1))], [np.zeros((1, n + 1))]])
    return Gb, Bb


def _mpm(M):
    return mp.matrix([[mp.mpf(float(v)) for v in row] for row in M])


KAPPA_CAP = 1e12   # 2^-52 x this is 2e-4: beyond it binary64 determines less than four digits of the value


def truth(G, B, w0, ports=None, kappa=True, dps=50, stable=True):
    """finite poles (ports None) or zeros, sorted by |s - s0| (ties: larger imaginary part first), with their condition numbers.
    stable: the eigenvalues are computed a second time at twice the digits, and a value is kept only if it is there again to 20 digits and
    (kappa) its condition number is below KAPPA_CAP.  What this removes is a DEFECTIVE infinite eigenvalue: a Jordan block of size p at
    theta = 0 (the bordered pencil of rc_mesh(6, 6) has one of size 7) shows up at |theta| ~ (10^-digits)^(1/p) -- a ring of p values 360/p
    degrees apart with condition numbers ~1e48 that moves with the working precision, above any relative floor."""
    if ports is not None:
        G, B = bordered(G, B, ports)
    old = mp.mp.dps
    mp.mp.dps = dps
    try:
        Bw = _mpm(B) * mp.mpf(w0)
        M = mp.inverse(_mpm(G) + mp.mpc(0, 1) * Bw) * Bw
        if kappa:
            ev, EL, ER = mp.eig(M, left=True, right=True)
        else:
            ev = mp.eig(M, left=False, right=False)
        n = len(ev)
        big = max(abs(t) for t in ev)
        again = None
        if stable:
            mp.mp.dps = 2 * dps
            Bw2 = _mpm(B) * mp.mpf(w0)
            again = mp.eig(mp.inverse(_mpm(G) + mp.mpc(0, 1) * Bw2) * Bw2, left=False, right=False)
            mp.mp.dps = dps
        out = []
        for i in range(n):
            if not abs(ev[i]) > FLOOR * big:
                continue
            if again is not None and not min(abs(t - ev[i]) for t in again) <= mp.mpf(10) ** -20 * abs(ev[i]):
                continue
            s = mp.mpc(0, w0) - mp.mpf(w0) / ev[i]
            k = float("inf")
            if kappa:
                yx = sum(EL[i, r] * ER[r, i] for r in range(n))
                ny = mp.sqrt(sum(abs(EL[i, r]) ** 2 for r in range(n)))
                nx = mp.sqrt(sum(abs(ER[r, i]) ** 2 for r in range(n)))
                k = float(ny * nx / abs(yx)) if yx != 0 else float("inf")
                if stable and not k <= KAPPA_CAP:
                    continue
            out.append((complex(s), k))
    finally:
        mp.mp.dps = old
    out.sort(key=lambda t: (abs(t[0] - 1j * w0), -t[0].imag))
    return np.array([t[0] for t in out], dtype=complex), np.array([t[1] for t in out], dtype=float)


def kappa_float64(G, B, w0, s):
    """condition numbers of the eigenvalues of M' that map to the values s, from scipy's left and right eigenvectors in binary64 (two
    digits of a condition number are all a bound needs; used where mpmath's eigenvectors of a 258-row matrix take too long)"""
    th, VL, VR = sl.eig(np.linalg.solve(G + 1j * w0 * B, w0 * B), left=True, right=True)
    sm = 1j * w0 - w0 / np.where(th == 0.0, 1e-300, th)
    out = []
    for v in s:
        i = int(np.argmin(np.abs(sm - v)))
        out.append(np.linalg.norm(VL[:, i]) * np.linalg.norm(VR[:, i]) / abs(np.vdot(VL[:, i], VR[:, i])))
    return np.array(out)


GOLDEN_TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pz_mesh6_truth.json")


def truth_key(G, B, w0, ports):
    h = hashlib.sha256(np.ascontiguousarray(G, dtype=np.float64).tobytes() + np.ascontiguousarray(B, dtype=np.float64).tobytes())
    h.update(repr((float(w0), ports)).encode())
    return h.hexdigest()[:24]


def truth_stored(G, B, w0, ports=None):
    """truth() from the fixture (scripts/pz_make_golden.py) when it holds these very matrices, shift and ports, else computed here"""
    if os.path.exists(GOLDEN_TRUTH):
        with open(GOLDEN_TRUTH) as f:
            g = json.load(f).get(truth_key(G, B, w0, ports))
        if g is not None:
            return np.array([complex(a, b) for a, b in g["s"]]), np.array(g["kappa"])
    return truth(G, B, w0, ports)


# ---- the float64 restatement of the iteration (E is measured on it; it also says what the Arnoldi process can reach in m steps)

def start_vector(n):
    i = np.arange(n)
    return (1.0 + ((i * 7 + 3) % 11) * 0.0625) + 1j * (((i * 5 + 1) % 13) * 0.0625)


def restate(G, B, w0, m, ports=None, tol=TOL, floor=FLOOR, btol=2.0 ** -40):
    """(s sorted, err_est, n_converged, complete) by the definitions of the header, in numpy"""
    n = len(G)
    A0, Bw = G + 1j * w0 * B, w0 * B
    lu = sl.lu_factor(A0)

    def solve(r):
        x = sl.lu_solve(lu, r)
        return x + sl.lu_solve(lu, r - A0 @ x)
    if ports is not None:
        b, c = selectors(n, ports)
        z = solve(b.astype(complex))
        g = c @ z

    def op(v):
        w = solve(Bw @ v)
        return w - z * (c @ w) / g if ports is not None else w
    V = np.zeros((m + 1, n), dtype=complex)
    H = np.zeros((m + 1, m), dtype=complex)
    w = op(start_vector(n))
    k, complete, beta = 0, False, 0.0
    nw = np.linalg.norm(w)
    if nw == 0.0:
        complete = True
    else:
        V[0] = w / nw
    while not complete and k < m:
        w = op(V[k])
        nw = np.linalg.norm(w)
        for _ in range(2):
            h = V[:k + 1].conj() @ w
            w = w - V[:k + 1].T @ h
            H[:k + 1, k] += h
        hk = np.linalg.norm(w)
        H[k + 1, k] = hk
        k += 1
        if hk <= btol * nw:
            complete = True
            break
        V[k] = w / hk
        beta = hk
    if k == 0:
        return np.zeros(0, complex), np.zeros(0), 0, complete
    th, Y = np.linalg.eig(H[:k, :k])
    last = np.abs(Y[-1, :]) / np.linalg.norm(Y, axis=0)
    keep = np.abs(th) > floor * np.abs(th).max()
    th, last = th[keep], last[keep]
    s = 1j * w0 - w0 / th
    err = np.zeros(len(th)) if complete else beta * last / np.abs(th)
    order = sorted(range(len(s)), key=lambda i: (abs(s[i] - 1j * w0), -s[i].imag))
    s, err = s[order], err[order]
    run = 0
    while run < len(s) and err[run] <= tol:
        run += 1
    return s, err, run, complete


# ---- comparison

def check(got, err, ref, kap, w0, what, count=None):
    """the first `count` (default: all) values of `got` against the truth, each matched to the nearest truth value not yet taken; prints the
    worst |d| / bound, then asserts.  Returns it."""
    count = len(got) if count is None else count
    taken, worst = set(), 0.0
    for i in range(count):
        j = min((j for j in range(len(ref)) if j not in taken), key=lambda j: abs(ref[j] - got[i]))
        taken.add(j)
        bound = abs(ref[j] - 1j * w0) * kap[j] * (err[i] + E)
        worst = max(worst, abs(got[i] - ref[j]) / bound)
    print(what, "values", count, "worst |d| / bound:", worst)
    assert worst <= 1.0, (what, worst)   # (a NaN fails too)
    return worst


def run_pz(pe, e, w0, what, n_wanted=1, max_krylov=32, ports=None, check_rc=True):
    F = pe.ffi
    st, stats = e.analyze_pz(w0, what, n_wanted, max_krylov, ports, check=check_rc)
    out = {"status": st, "stats": stats}
    for which, name in ((F.PZ_POLES, "poles"), (F.PZ_ZEROS, "zeros")):
        if what & which and stats["rc"] not in (F.ERR_ARG, F.ERR_NO_DEVICE, F.ERR_INTERNAL):
            out[name] = e.pz(which, max_krylov)
    return out


def counts_ok(st):
    """the point of the method: one factorisation, every step a kept-factor solve"""
    assert st["n_factorisations"] == 1 and st["n_solves"] >= st["n_steps"], st


# ---- 1. known answers

def known_answers(pe, O, knobs=None):
    F = pe.ffi
    # one pole at -1 / (R C), complete after one step
    d = pe.deck.ac_rc_lowpass()
    e = N.engine(pe, d, knobs=knobs)
    try:
        r = run_pz(pe, e, 1e3, F.PZ_POLES)
    finally:
        e.close()
    s, err, nf, nc, cp = r["poles"]
    ref, kap = truth(*pencil(N.oracle(O, d)), 1e3)
    print("lowpass", s[0, :nf[0]], r["stats"])
    assert list(nf) == [1] and list(cp) == [1] and list(nc) == [1] and len(ref) == 1 and abs(ref[0] + 1000.0) < 1e-9
    check(s[0, :1], err[0, :1], ref, kap, 1e3, "lowpass")
    assert abs(s[0, 0] + 1000.0) <= 1000.0 * np.sqrt(2.0) * kap[0] * E
    counts_ok(r["stats"])
    # series R L C: s = (-R +- sqrt(R^2 - 4 L / C)) / (2 L); R = 100: two real poles, R = 20: a complex pair
    for R in (100.0, 20.0):
        d = pe.deck.rlc_series_vl()
        d.devices = [(k, n, (R,) + p[1:]) if k == "R" else (k, n, p) for k, n, p in d.devices]
        L, Cap, w0 = 1e-3, 1e-6, 1e4
        root = np.sqrt(complex(R * R - 4.0 * L / Cap))
        cf = np.array([(-R + root) / (2.0 * L), (-R - root) / (2.0 * L)])
        cf = np.array(sorted(cf, key=lambda v: (abs(v - 1j * w0), -v.imag)))
        e = N.engine(pe, d, knobs=knobs)
        try:
            r = run_pz(pe, e, w0, F.PZ_POLES)
        finally:
            e.close()
        s, err, nf, nc, cp = r["poles"]
        ref, kap = truth(*pencil(N.oracle(O, d)), w0)
        print("series RLC R =", R, s[0, :nf[0]], cf)
        assert list(nf) == [2] and list(cp) == [1] and len(ref) == 2
        assert np.all(np.abs(ref - cf) <= 1e-9 * np.abs(cf)), (ref, cf)
        check(s[0, :2], err[0, :2], ref, kap, w0, "series RLC")
        for i in range(2):   # in order against the closed form
            assert abs(s[0, i] - cf[i]) <= abs(cf[i] - 1j * w0) * kap[i] * (err[0, i] + E), (i, s[0, i], cf[i])
        if R == 20.0:
            assert s[0, 0].imag > 0.0 > s[0, 1].imag and abs(s[0, 0].real - s[0, 1].real) < 1e-6 * abs(s[0, 0]), "both conjugates, the nearer first"
    # the lead network's closed-form zero (the order rule at an exact tie -- equal |s - s0|, the larger imaginary part first -- needs a Hessenberg
    # matrix made by hand: scripts/pz_kernel_host.cpp, which tests/test_pz_emu.py runs)
    R1, C1, R2, w0 = 1e3, 1e-7, 250.0, 2e4
    d = pe.deck.Deck()
    d.n_nodes = 2
    d.add("VAC", (1, 0), 1.0, 1e3, 0.0)
    d.add("R", (1, 2), R1)
    d.add("C", (1, 2), C1)
    d.add("R", (2, 0), R2)
    ports = ((2, -1), (1, -1))   # the source's branch row: a voltage excitation; the output node
    e = N.engine(pe, d, knobs=knobs)
    try:
        r = run_pz(pe, e, w0, F.PZ_BOTH, ports=ports)
        gain = e.pz_gain()
    finally:
        e.close()
    G, B = pencil(N.oracle(O, d))
    z, ez, nfz, ncz, cpz = r["zeros"]
    p, ep, nfp, ncp, cpp = r["poles"]
    zr, zk = truth(G, B, w0, ports)
    pr, pk = truth(G, B, w0)
    print("lead network zeros", z[0, :nfz[0]], "poles", p[0, :nfp[0]], "H(s0)", gain)
    assert list(nfz) == [1] and list(nfp) == [1] and len(zr) == 1 and len(pr) == 1
    assert abs(zr[0] + 1.0 / (R1 * C1)) < 1e-6 and abs(pr[0] + (R1 + R2) / (R1 * R2 * C1)) < 1e-6
    check(z[0, :1], ez[0, :1], zr, zk, w0, "lead zero")
    check(p[0, :1], ep[0, :1], pr, pk, w0, "lead pole")
    # a unit into the source's branch row is its branch equation v(1) = 1: H(s0) = +R2 (1 + s R1 C1) / (R1 + R2 + s R1 R2 C1) = (9 + 8j) / 29
    s0 = 1j * w0
    h = R2 * (1.0 + s0 * R1 * C1) / (R1 + R2 + s0 * R1 * R2 * C1)
    assert abs(h - (9.0 + 8.0j) / 29.0) < 1e-15 and abs(gain[0] - h) <= 1e-9 + 1e-6 * abs(h), (gain, h)


# ---- 2. parity of poles

PARITY = {"ac_linear_mix": 1e4, "ac_rlc_diode": 1e5, "ac_nmos_amp": 1e5, "ac_controlled_rest": 1e4, "ac_transistors": 1e5}


def parity(pe, O, name, knobs=None):
    F = pe.ffi
    d, w0 = getattr(pe.deck, name)(), PARITY[name]
    e = N.engine(pe, d, knobs=knobs)
    try:
        r = run_pz(pe, e, w0, F.PZ_POLES)
    finally:
        e.close()
    s, err, nf, nc, cp = r["poles"]
    ref, kap = truth(*pencil(N.oracle(O, d)), w0)
    print(name, knobs, r["stats"], "found", nf, "reference", len(ref))
    assert list(r["status"]) == [0] and list(cp) == [1] and r["stats"]["n_complete"] == 1
    assert nf[0] == len(ref) and nc[0] == nf[0], (nf, nc, len(ref))
    assert np.all(np.isnan(s[0, nf[0]:])) and np.all(err[0, :nf[0]] == 0.0)
    counts_ok(r["stats"])
    return check(s[0, :nf[0]], err[0, :nf[0]], ref, kap, w0, name)


def measure_e(pe, O):
    """E_MEASURED again: restate() on the parity cases"""
    worst = 0.0
    for name, w0 in PARITY.items():
        G, B = pencil(N.oracle(O, getattr(pe.deck, name)()))
        ref, kap = truth(G, B, w0)
        s, err, run, complete = restate(G, B, w0, 32)
        assert complete and len(s) == len(ref), name
        for i in range(run):
            j = int(np.argmin(np.abs(ref - s[i])))
            worst = max(worst, abs(s[i] - ref[j]) / (kap[j] * abs(ref[j] - 1j * w0)))
    print("E_MEASURED =", worst)
    return worst


# ---- 3. instances that finish at different steps

def mix_batch(pe):
    """ac_linear_mix at batch 3 with per-instance R and C; instance 0's second capacitor is 0: one pole fewer.  (Instance 0, because the
    static pivot order of a batch is matched on instance 0's values: alone at batch 1 the same instance then factors in the same order, and
    its results can be compared bit for bit.)"""
    base = pe.deck.ac_linear_mix()
    nR, nC = base.count("R"), base.count("C")
    r = np.array([[p[0] for k, _, p in base.devices if k == "R"]] * 3) * np.array([[1.0], [1.25], [0.8]])
    c = np.array([[p[0] for k, _, p in base.devices if k == "C"]] * 3) * np.array([[1.0], [0.5], [2.0]])
    c[0, 1] = 0.0
    decks = []
    for b in range(3):
        d, ir, ic = pe.deck.ac_linear_mix(), 0, 0
        dev = []
        for k, n, p in d.devices:
            if k == "R":
                p, ir = (float(r[b, ir]),) + p[1:], ir + 1
            elif k == "C":
                p, ic = (float(c[b, ic]),) + p[1:], ic + 1
            dev.append((k, n, p))
        d.devices = dev
        decks.append(d)
    assert (nR, nC) == (r.shape[1], c.shape[1])
    return base, {"R": r[:, :, None], "C": c[:, :, None]}, decks


def different_steps(pe, O, knobs=None):
    F = pe.ffi
    base, ov, decks = mix_batch(pe)
    w0 = 1e4
    refs = [truth(*pencil(N.oracle(O, d)), w0) for d in decks]
    assert len(refs[0][0]) == len(refs[1][0]) - 1 == len(refs[2][0]) - 1, [len(t[0]) for t in refs]
    e = N.engine(pe, base, batch=3, overrides=ov, knobs=knobs)
    try:
        r = run_pz(pe, e, w0, F.PZ_POLES)
    finally:
        e.close()
    s, err, nf, nc, cp = r["poles"]
    print("different steps: found", nf, r["stats"])
    assert list(cp) == [1, 1, 1] and list(nf) == [len(t[0]) for t in refs]
    for b in range(3):
        check(s[b, :nf[b]], err[b, :nf[b]], refs[b][0], refs[b][1], w0, "instance %d" % b)
    counts_ok(r["stats"])
    # the instance that was parked first, alone at batch 1: the same bits
    e = N.engine(pe, decks[0], knobs=knobs)
    try:
        a = run_pz(pe, e, w0, F.PZ_POLES)["poles"]
    finally:
        e.close()
    assert np.array_equal(a[0][0], s[0], equal_nan=True) and np.array_equal(a[1][0], err[0], equal_nan=True) and a[2][0] == nf[0]


# ---- 4. the 6 x 6 mesh: poles, zeros, H(s0)

def mesh_engine(pe, side, seeds, knobs=None):
    base, r, c = pe.deck.rc_mesh_params(side, side, seeds, True)
    e = N.engine(pe, pe.deck.rc_mesh(side, side, seeds[0], True), batch=len(seeds), overrides={"R": r[:, :, None], "C": c[:, :, None]}, knobs=knobs)
    return e, [pe.deck.rc_mesh(side, side, s, True) for s in seeds]


def mesh6(pe, O, knobs=None):
    F = pe.ffi
    w0 = MESH6_W0
    e, decks = mesh_engine(pe, 6, [1, 2, 3], knobs)
    try:
        r = run_pz(pe, e, w0, F.PZ_BOTH, 8, 64, MESH6_PORTS)
        gain = e.pz_gain()
        Z = e.analyze_net([w0], [MESH6_PORTS[0], MESH6_PORTS[1]])[0]
    finally:
        e.close()
    p, ep, nfp, ncp, cpp = r["poles"]
    z, ez, nfz, ncz, cpz = r["zeros"]
    print("mesh6", r["stats"], "poles", nfp, "zeros", nfz)
    assert list(r["status"]) == [0, 0, 0] and list(cpp) == [1, 1, 1] and list(cpz) == [1, 1, 1]
    assert r["stats"]["n_factorisations"] == 1 and r["stats"]["n_solves"] >= 2 * 64
    worst = 0.0
    for b, d in enumerate(decks):
        o = N.oracle(O, d)
        G, B = pencil(o)
        pr, pk = truth_stored(G, B, w0)
        zr, zk = truth_stored(G, B, w0, MESH6_PORTS)
        assert 2 * o.rows == 76 and nfp[b] == len(pr) == 36 and len(zr) == 29 and ncz[b] == nfz[b] >= 29, (2 * o.rows, nfp[b], len(pr), nfz[b], len(zr))
        worst = max(worst, check(p[b, :nfp[b]], ep[b, :nfp[b]], pr, pk, w0, "mesh6 poles %d" % b))
        # The bordered pencil has a DEFECTIVE infinite eigenvalue here (a Jordan block of size 7 at theta' = 0: truth()).  In binary64 it lands
        # at |theta'| ~ (2^-52)^(1/7) max |theta'|, far above the relative floor, so the call returns it as up to seven more values
        # (include/pe_hip.h says so).  What is asserted: the 29 zeros that exist come first, in order, each within its bound; whatever
        # follows lies outside every one of them -- the ring, not a zero moved or doubled.
        worst = max(worst, check(z[b, :29], ez[b, :29], zr, zk, w0, "mesh6 zeros %d" % b))
        far = np.abs(z[b, 29:nfz[b]] - 1j * w0)
        print("   surplus values of the defective infinite eigenvalue:", nfz[b] - 29, "nearest at |s - s0| =", far.min() if len(far) else None)
        assert nfz[b] - 29 <= 7 and np.all(far > np.abs(zr - 1j * w0).max()), (nfz[b], far)
        # H(s0) is Z[out][in] of the network analysis at omega0, within that analysis' own bound on Z
        ref = N.reference(o, [w0], [MESH6_PORTS[0], MESH6_PORTS[1]], None)
        assert abs(gain[b] - ref["Z"][0, 1, 0]) <= ref["EZ"][0, 1, 0] and abs(gain[b] - Z[0, b, 1, 0]) <= 2.0 * ref["EZ"][0, 1, 0], (gain[b], Z[0, b, 1, 0])
    assert not np.array_equal(p[0], p[1]), "the instances differ"
    return worst


# ---- 5. the 16 x 16 mesh: not complete, the nearest poles in order with none skipped

def mesh16(pe, O, knobs=None):
    F = pe.ffi
    w0 = MESH16_W0
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["omega0"] == w0 and gold["seeds"] == MESH16_SEEDS
    e, decks = mesh_engine(pe, 16, MESH16_SEEDS, knobs)
    worst = 0.0
    try:
        assert e.rows == 258
        for m, reach in ((32, 8), (64, 22)):
            r = run_pz(pe, e, w0, F.PZ_POLES, 8, m)
            s, err, nf, nc, cp = r["poles"]
            print("mesh16 m =", m, r["stats"], "found", nf, "converged", nc)
            assert list(r["status"]) == [0, 0] and list(cp) == [0, 0] and r["stats"]["n_complete"] == 0
            counts_ok(r["stats"])
            for b in range(2):
                ref = np.array([complex(a, c) for a, c in gold["poles"][b]])
                kap = np.array(gold["kappa"][b])
                assert 8 <= nc[b] <= len(ref), (m, b, nc)
                # in order, none skipped: the i-th converged value is the i-th nearest true pole
                for i in range(nc[b]):
                    bound = abs(ref[i] - 1j * w0) * kap[i] * (err[b, i] + E)
                    worst = max(worst, abs(s[b, i] - ref[i]) / bound)
                    assert abs(s[b, i] - ref[i]) <= bound, (m, b, i, s[b, i], ref[i], bound)
                print("   instance", b, "leading converged run", nc[b], "(the restatement reaches", reach, ")")
    finally:
        e.close()
    print("mesh16 worst |d| / bound:", worst)
    return worst


# ---- 6. determinism

def determinism(pe, O, knobs=None):
    F = pe.ffi
    w0 = MESH6_W0
    e, decks = mesh_engine(pe, 6, [1, 2, 3], knobs)
    try:
        a = run_pz(pe, e, w0, F.PZ_BOTH, 4, 48, MESH6_PORTS)
        b = run_pz(pe, e, w0, F.PZ_BOTH, 4, 48, MESH6_PORTS)
        run_pz(pe, e, w0, F.PZ_POLES, 4, 16)                    # a call of another shape in between
        c = run_pz(pe, e, w0, F.PZ_BOTH, 4, 48, MESH6_PORTS)
    finally:
        e.close()

    def same(x, y, bx=slice(None), by=slice(None)):
        return all(np.array_equal(x[k][i][bx], y[k][i][by], equal_nan=True) for k in ("poles", "zeros") for i in range(5))
    assert same(a, b), "two calls on one engine"
    assert same(a, c), "after a call of another shape"
    # other batch sizes and positions: instances (3, 2) as a batch of two, instance 2 alone
    e, _ = mesh_engine(pe, 6, [3, 2], knobs)
    try:
        d = run_pz(pe, e, w0, F.PZ_BOTH, 4, 48, MESH6_PORTS)
    finally:
        e.close()
    assert same(a, d, slice(2, 3), slice(0, 1)) and same(a, d, slice(1, 2), slice(1, 2)), "batch positions"
    e, _ = mesh_engine(pe, 6, [2], knobs)
    try:
        f = run_pz(pe, e, w0, F.PZ_BOTH, 4, 48, MESH6_PORTS)
    finally:
        e.close()
    assert same(a, f, slice(1, 2), slice(0, 1)), "batch sizes; a fresh engine reads what a used one reads"


# ---- 7. the dense solver alone

def eig_matrices():
    """name -> complex [n][m][m] upper Hessenberg"""
    rng = np.random.default_rng(20240607)

    def rnd(n, m):
        return np.triu(rng.standard_normal((n, m, m)) + 1j * rng.standard_normal((n, m, m)), -1)
    out = {}
    for m, n in ((1, 1), (2, 5), (3, 5), (31, 5), (32, 5), (33, 5), (64, 1)):
        out["random m=%d" % m] = rnd(n, m)
    out["random m=16 x65"] = rnd(65, 16)
    H = rnd(1, 8)
    H[0, 4, 3] = 0.0
    out["deflated"] = H
    out["jordan"] = np.array([[[2.0, 1.0, 0.0], [0.0, 2.0, 1.0], [0.0, 0.0, 2.0]]], dtype=complex)
    H = rnd(1, 6)
    H[0] = np.triu(H[0])
    H[0, 2, 2] = H[0, 4, 4] = 1.5 - 0.5j
    H[0, 1, 0] = 0.3
    out["repeated"] = H
    H = rnd(1, 9)
    H[0] *= (10.0 ** np.linspace(-4.0, 4.0, 9))[:, None]
    out["rows over eight decades"] = H
    return out


def eig_key(H):
    return hashlib.sha256(np.ascontiguousarray(H, dtype=np.complex128).tobytes()).hexdigest()[:24]


def eig_checked(n, i):
    """of 65 matrices in one launch every one is solved and every thirteenth is compared with mpmath"""
    return n <= 5 or i % 13 == 0


def eig_truth(H, gold):
    """mpmath's eigenvalues, condition numbers and last components of H: from the fixture (scripts/pz_make_golden.py) when it holds this very
    matrix, else computed here"""
    g = gold.get(eig_key(H))
    if g is None:
        return _eig_truth(H)
    return np.array([complex(a, b) for a, b in g["theta"]]), np.array(g["kappa"]), np.array(g["last"])


def _eig_truth(H, dps=50):
    old = mp.mp.dps
    mp.mp.dps = dps
    try:
        m = len(H)
        M = mp.matrix([[mp.mpc(complex(v)) for v in row] for row in H])
        ev, EL, ER = mp.eig(M, left=True, right=True)
        th, kap, last = [], [], []
        for i in range(m):
            yx = sum(EL[i, r] * ER[r, i] for r in range(m))
            ny = mp.sqrt(sum(abs(EL[i, r]) ** 2 for r in range(m)))
            nx = mp.sqrt(sum(abs(ER[r, i]) ** 2 for r in range(m)))
            th.append(complex(ev[i]))
            kap.append(float(ny * nx / abs(yx)) if yx != 0 else float("inf"))
            last.append(float(abs(ER[m - 1, i]) / nx))
    finally:
        mp.mp.dps = old
    return np.array(th), np.array(kap), np.array(last)


def eig_cases(pe, knobs=None):
    """pe None: measures numpy.linalg.eigvals on the same matrices (C_LAPACK_MEASURED) instead of the engine"""
    e = pe.ffi.Engine() if pe is not None else None
    worst, worst_last = 0.0, 0.0
    gold = {}
    if os.path.exists(GOLDEN_EIG):
        with open(GOLDEN_EIG) as f:
            gold = json.load(f)
    try:
        for name, Hs in eig_matrices().items():
            if e is not None:
                th, last, st = e.eig_hessenberg(Hs)
                assert not st.any(), (name, st)
            else:
                th = np.array([np.linalg.eigvals(H) for H in Hs])
                last = None
            m = Hs.shape[-1]
            for i, H in enumerate(Hs):
                if not eig_checked(len(Hs), i):
                    assert np.all(np.isfinite(th[i]))
                    continue
                ref, kap, rl = eig_truth(H, gold)
                unit = m * EPS * np.linalg.norm(H)
                taken = set()
                for k in range(m):
                    j = min((j for j in range(m) if j not in taken), key=lambda j: abs(ref[j] - th[i, k]))
                    taken.add(j)
                    ratio = abs(th[i, k] - ref[j]) / (kap[j] * unit)
                    worst = max(worst, ratio)
                    gap = min([abs(ref[j] - ref[l]) for l in range(m) if l != j] or [np.inf])
                    if last is not None and m > 1 and gap > 1e-3 * np.linalg.norm(H) and kap[j] < 1e6:   # simple eigenvalues only
                        # the eigenvector's own condition: kappa |H| / gap roundings
                        bl = C_EIG * m * EPS * kap[j] * np.linalg.norm(H) / gap
                        worst_last = max(worst_last, abs(abs(last[i, k]) - rl[j]) / bl)
            print(name, "worst ratio so far:", worst, "last components:", worst_last)
        if e is not None:
            assert worst <= C_EIG and worst_last <= 1.0, (worst, worst_last)
            # the Jordan block: three times 2, whatever the perturbation does to them stays inside kappa = inf; checked plainly
            th, last, st = e.eig_hessenberg(eig_matrices()["jordan"])
            assert np.all(np.abs(th - 2.0) <= 1e-4), th
            # a NaN entry beside finite neighbours: its matrix carries a status, the others are what they are alone
            H = eig_matrices()["random m=3"][:3].copy()
            alone = e.eig_hessenberg(H[[0, 2]])
            H[1, 1, 2] = np.nan
            th, last, st = e.eig_hessenberg(H)
            assert list(st) == [0, pe.ffi.ERR_SINGULAR, 0] and np.all(np.isnan(th[1])) and np.all(np.isnan(last[1]))
            assert np.array_equal(th[[0, 2]], alone[0]) and np.array_equal(last[[0, 2]], alone[1])
            # refusals
            lib = pe.ffi.lib()
            z = np.zeros(65 * 65)
            i1 = np.zeros(1, dtype=np.int32)
            for m, n in ((0, 1), (65, 1), (3, 0)):
                assert lib.pe_hip_eig_hessenberg(e._h, m, n, *[pe.ffi._dp(z)] * 6, pe.ffi._ip(i1)) == pe.ffi.ERR_ARG
            assert lib.pe_hip_eig_hessenberg(e._h, 3, 1, None, *[pe.ffi._dp(z)] * 5, pe.ffi._ip(i1)) == pe.ffi.ERR_ARG
    finally:
        if e is not None:
            e.close()
    print("eig worst |d| / (kappa m eps |H|):", worst, "(allowed", C_EIG, ")")
    return worst


# ---- 8. refusals and statuses

def refusals_and_statuses(pe, O, knobs=None):
    F = pe.ffi
    lib = F.lib()
    w0 = MESH6_W0
    e, decks = mesh_engine(pe, 6, [1, 2, 3], knobs)
    try:
        # before any call
        assert lib.pe_hip_get_pz(e._h, F.PZ_POLES, 0, 3, 4, None, None, None, None, None, None) == F.ERR_ARG
        wsw = np.array([1e7, 1e9])
        e.set_ac_sweep_rows([0, 17, 30])
        x, _, _ = e.analyze_ac_sweep(wsw)
        psd, _, _, _ = e.analyze_noise(wsw, 20, 5)
        net0 = e.analyze_net(wsw, [(1, -1), (30, 17)])
        good = run_pz(pe, e, w0, F.PZ_BOTH, 4, 40, MESH6_PORTS)

        def ctl(**kw):
            a = dict(what=F.PZ_BOTH, omega0=w0, n_wanted=4, max_krylov=40, tol=0.0, theta_floor=0.0, breakdown_tol=0.0, in_pos=1, in_neg=-1, out_pos=30, out_neg=17)
            a.update(kw)
            return F.PzControl(*[a[k] for k, _ in F.PzControl._fields_])
        bad = [dict(what=0), dict(what=4), dict(omega0=0.0), dict(omega0=-1.0), dict(omega0=float("inf")), dict(omega0=float("nan")), dict(n_wanted=0),
               dict(n_wanted=65), dict(max_krylov=-1), dict(max_krylov=65), dict(n_wanted=41), dict(in_pos=76), dict(out_neg=-2), dict(in_pos=-1),
               dict(out_pos=17), dict(tol=-1.0), dict(tol=float("nan")), dict(theta_floor=-1e-3), dict(theta_floor=float("inf")), dict(breakdown_tol=-1.0),
               dict(breakdown_tol=float("nan"))]
        for kw in bad:
            assert lib.pe_hip_analyze_pz(e._h, C.byref(ctl(**kw)), None, None) == F.ERR_ARG, kw
            for which, name in ((F.PZ_POLES, "poles"), (F.PZ_ZEROS, "zeros")):
                got = e.pz(which, 40)
                assert all(np.array_equal(got[i], good[name][i], equal_nan=True) for i in range(5)), ("the stored result after a refusal", kw)
        assert lib.pe_hip_analyze_pz(e._h, None, None, None) == F.ERR_ARG
        # rows are not read for poles alone
        assert lib.pe_hip_analyze_pz(e._h, C.byref(ctl(what=F.PZ_POLES, in_pos=999, out_pos=17)), None, None) == F.OK
        assert lib.pe_hip_get_pz(e._h, F.PZ_ZEROS, 0, 3, 4, None, None, None, None, None, None) == F.ERR_ARG, "zeros were not asked for"
        # the stored forward sweep, noise and network results read the same bits after the calls
        re = np.empty((2, 3, 3)); im = np.empty_like(re); out = np.empty((2, 3))
        assert lib.pe_hip_get_ac_sweep(e._h, 0, 2, 0, 3, F._dp(re), F._dp(im)) == 0 and np.array_equal(re + 1j * im, x)
        assert lib.pe_hip_get_noise(e._h, 0, 2, 0, 3, F._dp(out), None) == 0 and np.array_equal(out, psd)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(net0[:5], _net_again(pe, e, 2, 2))), "stored network result"
    finally:
        e.close()
    # no circuit
    e = F.Engine()
    try:
        c0 = F.PzControl(F.PZ_POLES, w0, 1, 32, 0.0, 0.0, 0.0, -1, -1, -1, -1)
        assert lib.pe_hip_analyze_pz(e._h, C.byref(c0), None, None) == F.ERR_ARG
    finally:
        e.close()
    # a NaN capacitance in one instance of three: that instance carries a status and reads NaN, the others are what they are without it
    base, ov, mix = mix_batch(pe)
    ov["C"] = ov["C"].copy()
    ov["C"][2, 0, 0] = float("nan")
    e = N.engine(pe, base, batch=3, overrides=ov, knobs=knobs)
    try:
        r = run_pz(pe, e, 1e4, F.PZ_POLES, check_rc=False)
    finally:
        e.close()
    s, err, nf, nc, cp = r["poles"]
    print("NaN capacitance: statuses", r["status"], "rc", r["stats"]["rc"], "found", nf)
    assert r["status"][0] == 0 and r["status"][1] == 0 and r["status"][2] != 0 and r["stats"]["rc"] == r["status"][2]
    assert np.all(np.isnan(s[2])) and nf[2] == 0
    for b in range(2):
        ref, kap = truth(*pencil(N.oracle(O, mix[b])), 1e4)
        assert nf[b] == len(ref)
        check(s[b, :nf[b]], err[b, :nf[b]], ref, kap, 1e4, "beside the NaN instance %d" % b)
    # zeros with an output the input cannot reach: two separate R C sections
    d = pe.deck.Deck()
    d.n_nodes = 2
    d.add("R", (1, 0), 1e3)
    d.add("C", (1, 0), 1e-6)
    d.add("R", (2, 0), 2e3)
    d.add("C", (2, 0), 1e-6)
    e = N.engine(pe, d, knobs=knobs)
    try:
        r = run_pz(pe, e, 1e3, F.PZ_BOTH, ports=((0, -1), (1, -1)), check_rc=False)
        zs = lib.pe_hip_get_pz(e._h, F.PZ_ZEROS, 0, 1, 4, None, None, None, None, None, None)
    finally:
        e.close()
    p, ep, nfp, ncp, cpp = r["poles"]
    overlay_refused(pe)
    print("unreachable output: rc", r["stats"]["rc"], "status", r["status"], "poles", p[0, :nfp[0]])
    assert r["stats"]["rc"] == F.ERR_SINGULAR and list(r["status"]) == [F.ERR_SINGULAR] and zs == F.OK
    assert nfp[0] == 2 and np.all(np.isnan(r["zeros"][0])) and r["zeros"][2][0] == 0
    ref, kap = truth(*pencil(N.oracle(O, d)), 1e3)
    check(p[0, :2], ep[0, :2], ref, kap, 1e3, "poles beside singular zeros")


def _net_again(pe, e, npt, n):
    """the stored network result, read again without a new analysis"""
    F = pe.ffi
    out = []
    for which in (F.NET_Z, F.NET_Y, F.NET_S):
        re, im = np.empty((npt, e.batch, n, n)), np.empty((npt, e.batch, n, n))
        e._chk(F.lib().pe_hip_get_net(e._h, which, 0, npt, 0, e.batch, F._dp(re), F._dp(im)))
        out.append(re + 1j * im)
    ys, ss = np.zeros((npt, e.batch), dtype=np.int32), np.zeros((npt, e.batch), dtype=np.int32)
    e._chk(F.lib().pe_hip_get_net_status(e._h, 0, npt, 0, e.batch, F._ip(ys), F._ip(ss)))
    return out + [ys, ss]


def overlay_refused(pe):
    """a circuit with a host-stamp overlay: PE_HIP_ERR_ARG (the circuit of the network tests' refusal)"""
    F = pe.ffi
    lib = F.lib()
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
    try:
        assert lib.pe_hip_set_overlay(g._h, 1, F._ip(one), F._ip(one), F._dp(rep), 1, F._ip(one), 0, cb, None) == 0
        g.set_options(g_min=1e-12)
        g.load(2, 1, [(F.VDC, np.array([[1, 0]], dtype=np.int32), np.array([0], dtype=np.int32), np.array([[3.0]]), 0),
                      (F.R, np.array([[1, 2]], dtype=np.int32), None, np.array([[1500.0]]), 0)])
        g.analyze_dc(F.MODE_DC)
        c0 = F.PzControl(F.PZ_POLES, 1e3, 1, 32, 0.0, 0.0, 0.0, -1, -1, -1, -1)
        assert lib.pe_hip_analyze_pz(g._h, C.byref(c0), None, None) == F.ERR_ARG and b"overlay" in lib.pe_hip_last_error(g._h)
    finally:
        g.close()
