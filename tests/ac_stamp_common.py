"""Shared by tests/test_ac_stamp_emu.py and tests/test_gpu_ac_stamp.py: the small-signal systems of pe_hip_analyze_ac, pe_hip_analyze_ac_sweep
and pe_hip_analyze_noise -- what build_ac_circuit / fill_ac_values (csrc/pe_ac.cpp) and ac_sweep_fill (csrc/pe_ac_sweep.hpp) put into the
2N real-equivalent matrix and its right-hand side, read back with Engine.matrix_ac() -- against a restatement of every model's iterate_ac
in mpmath complex arithmetic (256 bits), cell by cell; then the returned phasors against an mpmath solve of the matrix as read.

The reference (ref_stamp).  The complex N x N matrix and right-hand side of circult::solve_once with iterate_ac (circuit.h:1042-1060): the
digital drives (circuit.h:1015-1022), every model in deck order through its iterate_ac_define, or its iterate_dc_define where it has none
(model_refs/base.h:216-232), then g_min on the node diagonal (circuit.h:1107-1110).  Written from the model headers, the same lines
csrc/pe_ac.cpp and oracle/pe_oracle.py::stamp_ac cite:
  resistance.h:82-96 (1 / r)           capacitor.h:84-100 (j omega C)              inductor.h:103-130 (-j omega L; short when L == 0 or omega == 0)
  VDC.h:101 (E untouched)              VAC.h:117-118,144-156 (E = Vp cos + j Vp sin) IAC.h:116-117,133-143
  PN_junction.h:406-436 (geq, j omega tt geq under omega != 0, tt > 0, geq > 0, cd > 0; no Ieq)
  VCCS.h:80-95  VCVS.h:81-102  CCCS.h:81-100  CCVS.h:80-106  op_amp.h:64-83  transformer.h:67-99  transformer_center_tap.h:79-133
  switch.h:85-103  relay.h:75-105 (contact from the engaged state)  coupled_inductors.h:119-156
  sawtooth.h:121 / square.h:124 / pulse.h:155 / triangle.h:126 (an AC short)
  nmosfet.h:145-168  pmosfet.h:143-166  BJT_NPN.h:163-183  BJT_PNP.h:163-183
A '=' of the headers replaces the complex cell (both parts), a '+=' adds to it.  The real-equivalent form [Ar -Ai; Ai Ar] and its transpose
(the adjoint system of the noise analysis) are derived from that complex system here, by definition; nothing of pe_ac.cpp's emission lists
is used.  oracle/pe_oracle.py::stamp_ac (float64) runs through the same checks as a second implementation (OracleAc).

Values.  One rounded operation of inputs (1 / r, omega C, omega L, omega L1, omega L2, gains, 1 / (2 n), r_open, g_min, +-1) is compared
BITWISE with the correctly rounded mpmath value.  gds / gm / geq of the non-linear devices are read from cells of the main engine's own
matrix(b) that hold them alone (already pinned to mpmath by tests/device_eval_common.py) and compared bitwise.  M = k sqrt(L1 L2) then
omega M, tt geq omega and Vp cos(phase) / Vp sin(phase) carry the running rounding bound of device_eval_common.E (u = 2^-53 per operation,
2 u per libm call on the host).  A cell of k contributions gets its contributions' bounds plus (k - 1) u sum |v| for the additions.

Solution (check_solution).  x as returned against the mpmath solution of the system AS READ: the componentwise backward error
max_r |b - A x|_r / (|A| |x| + |b|)_r computed here, and the forward error against the Skeel bound omega_b |A^-1| (|A| |x| + |b|) with
omega_b = 4e-16 + (k + 2) u, k the longest row (4e-16: the refinement's threshold; (k + 2) u: the rounding of the residual that decides it)."""
import math

import mpmath as mp
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from device_eval_common import E, U, OracleEngine, Worst, f_sqrt
from parity_common import instance_devices, pe      # (instance_devices: the deck's devices with instance b's overridden parameters)

F = pe.ffi
Deck = pe.deck.Deck
R_OPEN = 1e12
GMIN = 2.0 ** -40
OMEGA_B0 = mp.mpf("4e-16")


def f_cos(a):
    v = mp.cos(a.v)
    return E(math.cos(a.d), v, a.e + 2 * U * abs(v))


def f_sin(a):
    v = mp.sin(a.v)
    return E(math.sin(a.d), v, a.e + 2 * U * abs(v))


def one(v):
    """a value that is one rounded operation of inputs: the correctly rounded double, demanded bitwise"""
    return E(float(v))


# ---- the reference: complex cells as lists of signed contributions -----------------------------------------------------------------------------
class RefSystem:
    def __init__(self, n):
        self.n = n
        self.A = {}      # (r, c) -> [re contributions, im contributions]
        self.b = {}      # r -> [re contributions, im contributions]
        self.was_set = set()      # cells a complex '=' wrote

    def add(self, r, c, re=None, im=None):
        if r < 0 or c < 0:
            return
        cell = self.A.setdefault((r, c), [[], []])
        if re is not None:
            cell[0].append(re)
        if im is not None:
            cell[1].append(im)

    def setv(self, r, c, re=None, im=None):
        if r < 0 or c < 0:
            return
        self.A[(r, c)] = [[], []]
        self.was_set.add((r, c))
        self.add(r, c, re, im)

    def badd(self, r, re=None, im=None):
        if r < 0:
            return
        cell = self.b.setdefault(r, [[], []])
        if re is not None:
            cell[0].append(re)
        if im is not None:
            cell[1].append(im)

    def bset(self, r, re=None, im=None):
        if r < 0:
            return
        self.b[r] = [[], []]
        self.badd(r, re, im)

    @staticmethod
    def part(lst):
        """(value, bound, k) of one part of a cell"""
        v = sum((t.v for t in lst), mp.mpf(0))
        bound = sum((t.e for t in lst), mp.mpf(0))
        if len(lst) > 1:
            bound += (len(lst) - 1) * U * sum(abs(t.v) for t in lst)
        return v, bound, len(lst)

    def G4(self, a, b, re=None, im=None):
        neg = lambda t: None if t is None else -t
        self.add(a, a, re, im)
        self.add(a, b, neg(re), neg(im))
        self.add(b, a, neg(re), neg(im))
        self.add(b, b, re, im)

    def incidence(self, a, b, k):
        self.setv(a, k, E(1.0))
        self.setv(b, k, E(-1.0))
        self.setv(k, a, E(1.0))
        self.setv(k, b, E(-1.0))


def ref_stamp(devices, n_nodes, drives, omega, g_min, r_open, nl, arms):
    """devices: [(kind, nodes, par)] of ONE instance in deck order; drives: [(node id, volt)]; nl: {device index: values of its last
    linearisation / state} -- (geq,) diode, (gds, gm) MOSFET, (geq, gm) BJT, (engaged,) relay.  Returns the RefSystem."""
    N = n_nodes
    nb = len(drives) + sum(pe.deck.NBRANCH[k] for k, _, _ in devices)
    S = RefSystem(N + nb)
    w = float(omega)
    if w == 0.0:
        arms.add("omega = 0")
    for k, (node, volt) in enumerate(drives):      # circuit.h:1015-1022
        S.setv(node - 1, N + k, E(1.0))
        S.setv(N + k, node - 1, E(1.0))
        S.bset(N + k, E(volt))
        arms.add("digital drive")
    kb = N + len(drives)
    for i, (kind, nodes, par) in enumerate(devices):
        n = [q - 1 for q in nodes]      # row of every pin, -1: ground
        if any(q < 0 for q in nodes):
            raise AssertionError("the decks of this module leave no pin unconnected")
        br = list(range(kb, kb + pe.deck.NBRANCH[kind]))
        kb += len(br)
        if any(q == 0 for q in nodes) and kind in ("IAC", "VAC"):
            arms.add(f"{kind}: a pin on ground")
        if kind == "R":
            S.G4(n[0], n[1], re=one(1 / mp.mpf(par[0])))
        elif kind == "C":
            S.G4(n[0], n[1], im=one(mp.mpf(par[0]) * mp.mpf(w)))
        elif kind == "L":
            S.incidence(n[0], n[1], br[0])
            if par[0] == 0.0 or w == 0.0:
                arms.add("L: short (L = 0)" if par[0] == 0.0 else "L: short (omega = 0)")
            else:
                arms.add("L: -j omega L")
                S.setv(br[0], br[0], im=one(-mp.mpf(w) * mp.mpf(par[0])))
        elif kind == "VDC":
            S.incidence(n[0], n[1], br[0])
        elif kind == "VAC":
            S.incidence(n[0], n[1], br[0])
            S.bset(br[0], E(par[0]) * f_cos(E(par[2])), E(par[0]) * f_sin(E(par[2])))
        elif kind == "IDC":
            pass
        elif kind == "IAC":
            re, im = E(par[0]) * f_cos(E(par[2])), E(par[0]) * f_sin(E(par[2]))
            S.badd(n[0], -re, -im)
            S.badd(n[1], re, im)
        elif kind == "D":
            geq = E(nl[i][0])
            tt = par[9]
            S.G4(n[0], n[1], re=geq)
            if w == 0.0 or not tt > 0.0 or not geq.d > 0.0:
                arms.add("D: no diffusion term (" + ("omega = 0" if w == 0.0 else ("tt = 0" if not tt > 0.0 else "geq <= 0")) + ")")
            else:
                cd = E(tt) * geq
                if cd.d > 0.0:
                    arms.add("D: j omega tt geq")
                    S.G4(n[0], n[1], im=cd * w)
                else:
                    arms.add("D: tt geq underflows to 0")
        elif kind == "VCCS":
            g = E(par[0])
            S.add(n[0], n[2], g)
            S.add(n[0], n[3], -g)
            S.add(n[1], n[2], -g)
            S.add(n[1], n[3], g)
        elif kind == "VCVS":
            k = br[0]
            S.setv(n[0], k, E(1.0))
            S.setv(n[1], k, E(-1.0))
            S.setv(k, n[0], E(1.0))
            S.setv(k, n[1], E(-1.0))
            S.setv(k, n[2], E(-par[0]))
            S.setv(k, n[3], E(par[0]))
        elif kind == "CCCS":
            c = br[0]
            S.setv(n[0], c, E(par[0]))
            S.setv(n[1], c, E(-par[0]))
            S.setv(n[2], c, E(1.0))
            S.setv(n[3], c, E(-1.0))
            S.setv(c, n[2], E(1.0))
            S.setv(c, n[3], E(-1.0))
        elif kind == "CCVS":
            k, c = br
            S.setv(n[0], k, E(1.0))
            S.setv(n[1], k, E(-1.0))
            S.setv(n[2], c, E(1.0))
            S.setv(n[3], c, E(-1.0))
            S.setv(k, n[0], E(1.0))
            S.setv(k, n[1], E(-1.0))
            S.setv(c, n[2], E(1.0))
            S.setv(c, n[3], E(-1.0))
            S.setv(k, c, E(-par[0]))
        elif kind == "OPAMP":
            k = br[0]
            S.setv(n[2], k, E(1.0))
            S.setv(n[3], k, E(-1.0))
            S.setv(k, n[2], E(1.0))
            S.setv(k, n[3], E(-1.0))
            S.add(k, n[0], E(-par[0]))
            S.add(k, n[1], E(par[0]))
        elif kind == "XFMR":
            kP, kS = br
            S.setv(n[0], kP, E(1.0))
            S.setv(n[1], kP, E(-1.0))
            S.setv(kP, n[0], E(1.0))
            S.setv(kP, n[1], E(-1.0))
            S.setv(n[2], kS, E(1.0))
            S.setv(n[3], kS, E(-1.0))
            S.add(kP, n[2], E(-par[0]))
            S.add(kP, n[3], E(par[0]))
            S.setv(kS, kS, E(1.0))
            S.setv(kS, kP, E(par[0]))
        elif kind == "SW":
            arms.add("SW: closed" if par[0] != 0.0 else "SW: open")
            S.incidence(n[0], n[1], br[0])
            S.setv(br[0], br[0], E(-(0.0 if par[0] != 0.0 else r_open)))
        elif kind == "RELAY":
            engaged = bool(nl[i][0])
            arms.add("RELAY: engaged" if engaged else "RELAY: not engaged")
            S.incidence(n[2], n[3], br[0])
            S.setv(br[0], br[0], E(-(0.0 if engaged else r_open)))
        elif kind in pe.deck.VGEN_LAYOUT:
            arms.add("time generator: AC short")
            S.incidence(n[0], n[1], br[0])
        elif kind == "XCT":
            kP, k1, k2 = br
            P, Q, S1, CT, S2 = n
            S.setv(P, kP, E(1.0))
            S.setv(Q, kP, E(-1.0))
            S.setv(S1, k1, E(1.0))
            S.setv(CT, k1, E(-1.0))
            S.setv(CT, k2, E(1.0))
            S.setv(S2, k2, E(-1.0))
            nh = 2.0 * par[0]      # n_half (exact)
            inv = one(1 / mp.mpf(nh)) if nh != 0.0 else None
            arms.add("XCT: n != 0" if nh != 0.0 else "XCT: n = 0")
            S.setv(k1, S1, E(1.0))
            S.setv(k1, CT, E(-1.0))
            if inv is not None:
                S.add(k1, P, -inv)
                S.add(k1, Q, inv)
            S.setv(k2, CT, E(1.0))
            S.setv(k2, S2, E(-1.0))
            if inv is not None:
                S.add(k2, P, -inv)
                S.add(k2, Q, inv)
                S.setv(kP, kP, E(1.0))
                S.setv(kP, k1, inv)
                S.setv(kP, k2, inv)
        elif kind == "KL":
            k1, k2 = br
            S.setv(n[0], k1, E(1.0))
            S.setv(n[1], k1, E(-1.0))
            S.setv(n[2], k2, E(1.0))
            S.setv(n[3], k2, E(-1.0))
            S.setv(k1, n[0], E(1.0))
            S.setv(k1, n[1], E(-1.0))
            S.setv(k2, n[2], E(1.0))
            S.setv(k2, n[3], E(-1.0))
            M = E(par[2]) * f_sqrt(E(par[0]) * E(par[1]))
            S.setv(k1, k1, im=one(-mp.mpf(w) * mp.mpf(par[0])))
            S.setv(k1, k2, im=-(M * w))
            S.setv(k2, k1, im=-(M * w))
            S.setv(k2, k2, im=one(-mp.mpf(w) * mp.mpf(par[1])))
        elif kind in ("NMOS", "PMOS"):
            gds, gm = E(nl[i][0]), E(nl[i][1])
            D, G, Sn = n
            S.G4(D, Sn, re=gds)
            if kind == "NMOS":
                S.add(D, G, gm)
                S.add(D, Sn, -gm)
                S.add(Sn, G, -gm)
                S.add(Sn, Sn, gm)
            else:
                S.add(D, Sn, gm)
                S.add(D, G, -gm)
                S.add(Sn, Sn, -gm)
                S.add(Sn, G, gm)
        elif kind in ("NPN", "PNP"):
            geq, gm = E(nl[i][0]), E(nl[i][1])
            B, Cn, En = n
            S.G4(B, En, re=geq)
            if kind == "NPN":
                S.add(Cn, B, gm)
                S.add(Cn, En, -gm)
                S.add(En, B, -gm)
                S.add(En, En, gm)
            else:
                S.add(En, En, gm)
                S.add(En, B, -gm)
                S.add(Cn, En, -gm)
                S.add(Cn, B, gm)
        else:
            raise AssertionError(f"no AC restatement of {kind}")
    if g_min != 0.0:
        arms.add("g_min != 0")
        for r in range(N):
            S.add(r, r, E(g_min))
    return S


# ---- engines ------------------------------------------------------------------------------------------------------------------------------------
class OracleAc(OracleEngine):
    """oracle/pe_oracle.py behind the Engine methods this module uses: stamp_ac as the float64 second implementation"""

    def __init__(self, mod, deck, batch, overrides, g_min, r_open, drives):
        super().__init__(mod, deck, batch, overrides, 0)
        self.o = [mod.Oracle(o.deck, g_min, drives, r_open) for o in self.o]
        for o in self.o:
            o.prepare()
        self.rows = self.o[0].rows
        self._ac = [None] * batch

    def analyze_ac(self, omega, check=True):
        x = np.full((self.batch, self.rows), np.nan, dtype=complex)
        rc = 0
        for b, o in enumerate(self.o):
            A, rhs = o.stamp_ac(omega)
            n = self.rows
            ii, jj, vv = [], [], []
            for (r, c), v in A.items():
                v = complex(v)
                ii += [r, r, r + n, r + n]
                jj += [c, c + n, c, c + n]
                vv += [v.real, -v.imag, v.imag, v.real]
            M = sp.csr_matrix(sp.coo_matrix((vv, (ii, jj)), shape=(2 * n, 2 * n)))
            M.sort_indices()
            self._ac[b] = (M, np.concatenate([rhs.real, rhs.imag]))
            xs = o.solve_ac(omega)
            if xs is None:
                rc = F.ERR_SINGULAR
            else:
                x[b] = xs
        return x, rc

    def matrix_ac(self, which=0, instance=0, rhs=True):
        M, b = self._ac[instance]
        return M.indptr, M.indices, M.data, (b if rhs else None)


def ac_engine(deck, batch=1, knobs=None, overrides=None, g_min=0.0, drives=()):
    knobs = knobs or {}
    if "ORACLE" in knobs:
        return OracleAc(knobs["ORACLE"], deck, batch, overrides, g_min, R_OPEN, list(drives))
    e = F.Engine()
    e.set_options(g_min=g_min, r_open=R_OPEN)
    for k, v in knobs.items():
        e.set_knob(k, v)
    if drives:
        e.set_digital_drives([d[0] for d in drives], [d[1] for d in drives])
    e.load_deck(deck, batch, overrides, n_drives=len(drives))
    e.reset()
    return e


def cells_of(rp, ci, va):
    return {(r, int(ci[s])): float(va[s]) for r in range(len(rp) - 1) for s in range(rp[r], rp[r + 1])}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- the cell-by-cell comparison ----------------------------------------------------------------------------------------------------------------
def check_system(W, name, got, rhs, S, what, transposed=False):
    """got: {(r, c): value} of the 2N real-equivalent system as read; S: the reference.  Every complex cell (r, c): the four real cells hold
    (Re, -Im; Im, Re) -- of the transpose, with `transposed` --; cells the reference leaves empty are absent or exactly 0.0."""
    n = S.n
    seen = set()
    for (r, c), (re_l, im_l) in S.A.items():
        re, bre, kre = RefSystem.part(re_l)
        im, bim, kim = RefSystem.part(im_l)
        quad = (((r, c), re, bre), ((r, c + n), -im, bim), ((r + n, c), im, bim), ((r + n, c + n), re, bre))
        for (rr, cc), v, bound in quad:
            key = (cc, rr) if transposed else (rr, cc)
            seen.add(key)
            if (r, c) in S.was_set and "ORACLE_PATTERN" not in what:
                # a complex '=' clears both parts of the cell: the part it does not write is an explicit zero of the pattern
                assert key in got, f"{name} {what}: cell {key} of complex ({r}, {c}), written by '=', is not in the pattern"
            g = got.get(key, 0.0)
            W.check(name, g, E(0, v), f"{what}, cell {key} of complex ({r}, {c})", bound)
    for key, g in got.items():
        if key not in seen:
            assert g == 0.0, f"{name} {what}: cell {key} holds {g!r} where the reference stamps nothing"
    if rhs is None:
        return
    for r in range(n):
        re_l, im_l = S.b.get(r, ([], []))
        for row, lst in ((r, re_l), (r + n, im_l)):
            v, bound, _ = RefSystem.part(lst)
            W.check(name + " rhs", rhs[row], E(0, v), f"{what}, right-hand side row {row}", bound)


def longest_row(rp):
    return int(np.max(np.diff(rp)))


# ---- the solve chain: mpmath solution of the system as read -----------------------------------------------------------------------------------
def mp_solve(M, cols):
    """solutions of M y = col for every column (lists of mpf), to the working precision: float64 LU as the preconditioner of an iterative
    refinement whose residuals are exact sums in mpmath.  Returns None when M is singular in float64."""
    M = sp.csc_matrix(M)
    n = M.shape[0]
    coo = M.tocoo()
    ent = [(int(r), int(c), mp.mpf(float(v))) for r, c, v in zip(coo.row, coo.col, coo.data)]
    try:
        lu = spla.splu(M, permc_spec="COLAMD", diag_pivot_thresh=1.0)
    except RuntimeError:
        return None
    out = []
    for col in cols:
        y = [mp.mpf(0)] * n
        for _ in range(80):
            res = list(col)
            for r, c, v in ent:
                res[r] -= v * y[c]
            scale = max([abs(t) for t in col] + [abs(t) for t in y])
            worst = max(abs(t) for t in res)
            if worst == 0 or worst <= scale * mp.mpf(2) ** -200:
                break
            d = lu.solve(np.array([float(t / worst) for t in res]))
            if not np.all(np.isfinite(d)):
                return None
            y = [a + mp.mpf(float(t)) * worst for a, t in zip(y, d)]
        else:
            return None
        out.append(y)
    return out


def check_solution(W, name, rp, ci, va, rhs, x, what, skeel=True, cache=None):
    """x: the returned phasors [N] complex of this instance; (rp, ci, va, rhs): its system as read; cache: {system: (exact, inverse)}.
    The oracle (name None) is not put through it: Oracle.solve_ac is SuperLU without refinement, which leaves 1e-34 where a decoupled row's
    exact solution is 0 -- a componentwise backward error of 1 on that row; the oracle's part is the stamp."""
    if name is None:
        return
    n2 = len(rp) - 1
    xr = np.concatenate([x.real, x.imag])
    assert np.all(np.isfinite(xr)), f"{name} {what}: phasors not finite"
    M = sp.csr_matrix((va, ci, rp), shape=(n2, n2))
    xm = [mp.mpf(float(t)) for t in xr]
    bm = [mp.mpf(float(t)) for t in rhs]
    res, mag = list(bm), [abs(t) for t in bm]
    for r in range(n2):
        for s in range(rp[r], rp[r + 1]):
            t = mp.mpf(float(va[s])) * xm[ci[s]]
            res[r] -= t
            mag[r] += abs(t)
    omega_b = OMEGA_B0 + (longest_row(rp) + 2) * U
    berr = max((abs(a) / m for a, m in zip(res, mag) if m > 0), default=mp.mpf(0))
    assert all(a == 0 for a, m in zip(res, mag) if m == 0), f"{name} {what}: a residual on an empty row"
    W.ratio[name + " backward error"] = max(W.ratio.get(name + " backward error", 0.0), float(berr / omega_b))
    assert berr <= omega_b, f"{name} {what}: componentwise backward error {float(berr):.3g} above {float(omega_b):.3g}"
    if not skeel:
        return
    key = (bits(va).tobytes(), bits(rhs).tobytes(), np.asarray(ci).tobytes())
    if cache is not None and key in cache:
        exact, inv = cache[key]
    else:
        sol = mp_solve(M, [bm])
        assert sol is not None, f"{name} {what}: the system as read is singular"
        exact = sol[0]
        unit = []
        for j in range(n2):
            e = [mp.mpf(0)] * n2
            e[j] = mp.mpf(1)
            unit.append(e)
        inv = mp_solve(M, unit)      # columns of the inverse
        if cache is not None:
            cache[key] = (exact, inv)
    worst = 0.0
    # the reference's own error: mp_solve stops at a residual of 2^-200 relative; with the conditioning of these systems (below 2^50) its
    # solutions are good to 2^-150 of their largest entry
    ref_tol = mp.mpf(2) ** -150 * max(abs(t) for t in exact)
    for r in range(n2):
        bound = omega_b * sum(abs(inv[j][r]) * mag[j] for j in range(n2)) + ref_tol
        err = abs(xm[r] - exact[r])
        if bound == 0:
            assert err == 0, f"{name} {what}: row {r} is {float(xm[r])!r}, exactly {mp.nstr(exact[r], 20)} expected"
            continue
        worst = max(worst, float(err / bound))
        assert err <= bound, f"{name} {what}: row {r} forward error {float(err):.3g} above the Skeel bound {float(bound):.3g}"
    W.ratio[name + " forward / Skeel"] = max(W.ratio.get(name + " forward / Skeel", 0.0), worst)


# ---- (a) one device per deck, every pin on a node of its own --------------------------------------------------------------------------------------
class Case:
    """one device under test; pins: 'r' a node with a resistor to ground, 'v' a node held by a VDC (bias), 0 ground"""

    def __init__(self, name, kind, pins, par, batch_par=None, bias=None, omegas=(1000.0,), drives=False):
        self.name, self.kind, self.omegas = name, kind, omegas
        d = Deck()
        nodes, self.vdc = [], []
        for p in pins:
            if p == 0:
                nodes.append(0)
                continue
            node = d.new_node()
            nodes.append(node)
            if p == "r":
                d.add("R", (node, 0), 100.0 * node)
            else:
                self.vdc.append(d.count("VDC"))
                d.add("VDC", (node, 0), 0.0)
        self.dev = len(d.devices)
        d.add(kind, nodes, *par)
        if kind not in ("IAC", "VAC"):      # a stimulus, so that the phasors of check (e) are not all zero: right-hand side only
            d.add("IAC", (0, next(q for q in nodes if q)), 1e-3, 50.0, 0.7)
        self.nodes = nodes
        self.deck = d
        self.drives = [(nodes[0], 1.5)] if drives else []
        self.overrides = {}
        self.batch = 1
        if batch_par is not None:
            self.batch = len(batch_par)
            rows = [[list(batch_par[b]) if i == self.dev else list(p) for i, (k, _, p) in enumerate(d.devices) if k == kind] for b in range(self.batch)]
            self.overrides[kind] = np.array(rows, dtype=float)      # (the pin resistors of the case "R" keep their values)
        if bias is not None:      # [B][number of 'v' pins]
            self.batch = len(bias)
            self.overrides["VDC"] = np.array(bias, dtype=float).reshape(self.batch, len(self.vdc), 1)


D_TT = (1e-14, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 1.0, 1.0, 1e-8)
D_TT0 = D_TT[:9] + (0.0,)
D_TINY = D_TT[:9] + (1e-300,)
MOS = (2e-3, 0.02, 1.0)
BJT = (1e-16, 1.0, 100.0, 27.0, 1.0)
W0 = 1000.0


def single_cases():
    sg = -1.0
    return [
        Case("R", "R", "rr", (330.0,), [[330.0], [1e-3], [7e9]]),
        Case("C", "C", "rr", (1e-6,), [[1e-6], [3.3e-12], [-2e-6]], omegas=(W0, 0.0, 1e9)),
        Case("L", "L", "rr", (1e-3,), [[1e-3], [0.0], [-4e-3]], omegas=(W0, 0.0)),
        Case("VDC", "VDC", "rr", (5.0,)),
        Case("VAC", "VAC", "rr", (2.0, 50.0, 0.3), [[2.0, 50.0, 0.3], [1e-3, 50.0, 4.0], [5.0, 50.0, 0.0]], omegas=(W0, 0.0)),
        Case("VAC on ground", "VAC", ("r", 0), (2.0, 50.0, 1.1)),
        Case("IDC", "IDC", "rr", (1.0,)),
        Case("IAC", "IAC", "rr", (1e-3, 50.0, 0.4), [[1e-3, 50.0, 0.4], [2.0, 50.0, -2.5]]),
        Case("IAC on ground", "IAC", (0, "r"), (1e-3, 50.0, 0.4)),
        Case("IAC into ground", "IAC", ("r", 0), (1e-3, 50.0, 2.0)),
        Case("D tt", "D", "vv", D_TT, bias=[[0.6, 0.0], [0.0, 0.55], [0.3, 0.9]], omegas=(W0, 0.0)),
        Case("D tt = 0", "D", "vv", D_TT0, bias=[[0.6, 0.0]]),
        Case("D tt geq underflow", "D", "vv", D_TINY, bias=[[0.0, 2.0], [0.6, 0.0]]),
        Case("VCCS", "VCCS", "rrrr", (2e-3,), [[2e-3], [-0.7]]),
        Case("VCVS", "VCVS", "rrrr", (3.0,), [[3.0], [-0.25]]),
        Case("CCCS", "CCCS", "rrrr", (2.0,), [[2.0], [-5.5]]),
        Case("CCVS", "CCVS", "rrrr", (500.0,), [[500.0], [-1e-2]]),
        Case("OPAMP", "OPAMP", "rrrr", (1e5,), [[1e5], [3.0]]),
        Case("XFMR", "XFMR", "rrrr", (2.0,), [[2.0], [-0.5]]),
        Case("SW", "SW", "rr", (0.0,), [[0.0], [1.0]]),
        Case("RELAY", "RELAY", "vvrr", (5.0, 3.0), bias=[[6.0, 0.0], [1.0, 0.0], [0.0, -7.0]]),
        Case("SAW", "SAW", "rr", (5.0, 0.0, 1e3, 0.0)),
        Case("SQR", "SQR", "rr", (5.0, 0.0, 1e3, 0.5, 0.0)),
        Case("PULSE", "PULSE", "rr", (5.0, 0.0, 1e3, 0.5, 0.0, 1e-6, 1e-6)),
        Case("TRI", "TRI", "rr", (5.0, 0.0, 1e3, 0.0)),
        Case("KL", "KL", "rrrr", (1e-3, 4e-3, 0.8), [[1e-3, 4e-3, 0.8], [2e-6, 3e-3, -0.5], [1e-3, 1e-3, 0.0]], omegas=(W0, 0.0)),
        Case("XCT", "XCT", "rrrrr", (2.0,), [[2.0], [-3.0]]),
        Case("XCT n = 0", "XCT", "rrrrr", (2.0,), [[2.0], [0.0]]),
        # (Vd, Vg, Vs): saturation, triode, and drain and source swapped (Vds < 0)
        Case("NMOS", "NMOS", "vvv", MOS, bias=[[3.0, 2.25, 0.25], [0.75, 2.25, 0.25], [0.25, 3.5, 1.0], [0.0, 2.0, 0.5]]),
        Case("PMOS", "PMOS", "vvv", MOS, bias=[[sg * 3.0, sg * 2.25, sg * 0.25], [sg * 0.75, sg * 2.25, sg * 0.25], [sg * 0.25, sg * 3.5, sg * 1.0],
                                               [0.0, -2.0, -0.5]]),
        # (Vb, Vc, Ve): forward active, and collector and emitter swapped
        Case("NPN", "NPN", "vvv", BJT, bias=[[0.9, 2.0, 0.25], [0.9, 0.1, 0.25], [0.6, 0.1, 0.0]]),
        Case("PNP", "PNP", "vvv", BJT, bias=[[-0.9, -2.0, -0.25], [-0.9, -0.1, -0.25], [-0.6, -0.1, 0.0]]),
        Case("digital drive", "R", "rr", (1e3,), drives=True),
    ]


SINGLE_ARMS = ["omega = 0", "L: short (L = 0)", "L: short (omega = 0)", "L: -j omega L", "D: j omega tt geq", "D: no diffusion term (omega = 0)",
               "D: no diffusion term (tt = 0)", "D: tt geq underflows to 0", "SW: open", "SW: closed", "RELAY: engaged", "RELAY: not engaged",
               "XCT: n = 0", "XCT: n != 0", "IAC: a pin on ground", "VAC: a pin on ground", "g_min != 0", "time generator: AC short", "digital drive",
               "NMOS: Vds > 0", "NMOS: Vds < 0", "PMOS: Vds > 0", "PMOS: Vds < 0", "NPN: Vce > 0", "NPN: Vce < 0", "PNP: Vce > 0", "PNP: Vce < 0"]


def nl_values(e, deck, b):
    """{device index: values} of instance b's last linearisation, read from cells of the main engine's matrix(b) that hold them alone (the
    decks of this module put no other device across D-S / D-G of a MOSFET, B-E / C-B of a BJT, anode-cathode of a diode); the relay's state
    from its contact cell"""
    kinds = {k for k, _, _ in deck.devices}
    if not kinds & {"D", "NMOS", "PMOS", "NPN", "PNP", "RELAY"}:
        return {}
    rp, ci, va, _ = e.matrix(b)
    A = sp.csr_matrix((va, ci, rp), shape=(len(rp) - 1, len(rp) - 1))
    out = {}
    kb = deck.n_nodes
    for i, (kind, nodes, par) in enumerate(deck.devices):
        n = [q - 1 for q in nodes]
        if kind == "D":
            out[i] = (-float(A[n[0], n[1]]),)
        elif kind in ("NMOS", "PMOS"):
            out[i] = (-float(A[n[2], n[0]]), float(A[n[0], n[1]]) * (1.0 if kind == "NMOS" else -1.0))
        elif kind in ("NPN", "PNP"):
            out[i] = (-float(A[n[0], n[2]]), float(A[n[1], n[0]]))
        elif kind == "RELAY":
            out[i] = (float(A[kb, kb]) == 0.0,)
        kb += pe.deck.NBRANCH[kind]
    return out


def check_single(knobs, label="", g_min=0.0, sweep=True, only=None):
    """(a), and for every case (c): the sweep's systems bit-identical to the single-point ones, and (e): the phasors of both paths"""
    W = Worst()
    for case in single_cases():
        if only and case.name not in only:
            continue
        B = case.batch
        e = ac_engine(case.deck, B, knobs, case.overrides, g_min, case.drives)
        nonlinear = case.deck.has_nonlinear()
        if nonlinear:
            st = e.analyze_dc(F.MODE_OP, check=False)
            assert all(s == 0 for s in e.state()["status"]), f"{case.name}: operating point {st}"
        devs = [instance_devices(case.deck, case.overrides, b) for b in range(B)]
        nl = [nl_values(e, case.deck, b) for b in range(B)]
        dev_i = case.dev
        for b in range(B):      # arms of the bias sets, asserted on the values the devices hold
            if case.kind in ("NMOS", "PMOS", "NPN", "PNP"):
                v = {n: (case.overrides["VDC"][b, j, 0]) for j, n in zip(range(len(case.vdc)), case.nodes)}
                first, last = v[case.nodes[0]], v[case.nodes[2]]
                if case.kind in ("NMOS", "PMOS"):
                    vds = (first - last) * (1.0 if case.kind == "NMOS" else -1.0)
                    W.arms.add(f"{case.kind}: Vds " + ("> 0" if vds > 0 else "< 0"))
                    assert nl[b][dev_i][0] != 0.0 and nl[b][dev_i][1] != 0.0 and nl[b][dev_i][0] != nl[b][dev_i][1], (case.name, b, nl[b])
                else:
                    vce = (v[case.nodes[1]] - last) * (1.0 if case.kind == "NPN" else -1.0)
                    W.arms.add(f"{case.kind}: Vce " + ("> 0" if vce > 0 else "< 0"))
                    assert nl[b][dev_i][0] > 0.0 and nl[b][dev_i][1] > 0.0 and nl[b][dev_i][0] != nl[b][dev_i][1], (case.name, b, nl[b])
        singular = {b for b in range(B) if case.kind == "XCT" and devs[b][dev_i][2][0] == 0.0}      # (the reference's row kP is empty)
        single = {}
        for w in case.omegas:
            x, rc = e.analyze_ac(w, check=False)
            assert rc == (F.ERR_SINGULAR if singular else 0), f"{case.name} at omega {w}: analyze_ac returned {rc}"
            if singular:
                # the reference leaves the ampere-turns row kP empty under n_half == 0 (transformer_center_tap.h:124-130): its system is
                # singular and so is this one -- there is no assembled system to read, the status is the check (and the arm)
                for b in singular:
                    ref_stamp(devs[b], case.deck.n_nodes, case.drives, w, g_min, R_OPEN, nl[b], W.arms)
                continue
            for b in range(B):
                what = f"{label} {case.name}, instance {b}, omega {w}, g_min {g_min}"
                rp, ci, va, rhs = e.matrix_ac(0, b, rhs=not singular)
                S = ref_stamp(devs[b], case.deck.n_nodes, case.drives, w, g_min, R_OPEN, nl[b], W.arms)
                check_system(W, case.kind, cells_of(rp, ci, va), rhs, S, what)
                single[w, b] = (rp.copy(), ci.copy(), va.copy(), None if rhs is None else rhs.copy())
                if not singular:
                    check_solution(W, None if "ORACLE" in knobs else "single-point", rp, ci, va, rhs, x[b], what)
        if sweep and not singular and "ORACLE" not in knobs:
            ws = list(case.omegas)
            sweeps = [(2, [w, w, w]) for w in ws] + [(1, ws[::-1])] + ([(0, ws[1:] + ws[:1])] if len(ws) > 1 else [])
            check_sweep_identity(case.deck, B, knobs, case.overrides, g_min, case.drives, sweeps, single, W, f"{label} {case.name}")
        e.close()
    if not only:
        W.need(SINGLE_ARMS if g_min != 0.0 else [a for a in SINGLE_ARMS if a != "g_min != 0"], "single-device decks")
    W.report(f"AC stamp, one device per deck, g_min {g_min} {label}")
    return W


def pass_layout(omegas, P):
    """the passes of pe_hip_analyze_ac_sweep as include/pe_hip.h defines them: points ascending (ties in the caller's order), omega == 0 a
    band of its own, a band takes every point with omega <= 10 w0, ceil(points / P) passes per band; unused points repeat the last one.
    Returns the list of passes, each a list of P omegas."""
    order = sorted(range(len(omegas)), key=lambda i: omegas[i])
    passes, i = [], 0
    while i < len(order):
        w0 = omegas[order[i]]
        j = i + 1
        while j < len(order) and (omegas[order[j]] == 0.0 if w0 == 0.0 else omegas[order[j]] <= 10.0 * w0):
            j += 1
        for first in range(i, j, P):
            pts = [omegas[order[k]] for k in range(first, min(first + P, j))]
            passes.append(pts + [pts[-1]] * (P - len(pts)))
        i = j
    return passes


def check_sweep_identity(deck, B, knobs, overrides, g_min, drives, sweeps, single, W, what):
    """(c): on a fresh engine, for every (AC_SWEEP_POINTS knob, omegas in the caller's order) of `sweeps`: every instance q = b P + p of the
    sweep's last pass, matrix and stamped right-hand side, bit-identical to the single-point engine's at that omega (`single`:
    {(omega, b): system}, from an engine that ran single points only); and (e) on the sweep's phasors of every point"""
    e = ac_engine(deck, B, knobs, overrides, g_min, drives)
    if deck.has_nonlinear():
        e.analyze_dc(F.MODE_OP)
    for knob, ws in sweeps:
        e.set_knob("AC_SWEEP_POINTS", knob)
        x, status, stats = e.analyze_ac_sweep(ws, check=False)
        # (a point may fall back to the single-point path -- an instance whose zero pattern differs from instance 0's can meet a bad static
        # pivot --: the pass was filled all the same)
        assert stats["rc"] == 0 and not status.any(), f"{what}: sweep {stats} {status}"
        P = e.ac_pass_size(1)
        assert P >= 1 and (knob == 0 or P <= knob), (knob, P)
        passes = pass_layout(ws, P)
        assert stats["n_passes"] == len(passes), (stats, passes)
        last = passes[-1]
        W.arms.add("sweep: P = 1" if P == 1 else "sweep: P > 1")
        if len(ws) % P and sum(len(set(p)) < P for p in passes):
            W.arms.add("sweep: last pass partly unused")
        if 0.0 in ws and any(w != 0.0 for w in ws):
            W.arms.add("sweep: omega = 0 next to nonzero points in one call")
        for b in range(B):
            for p, w in enumerate(last):
                rp, ci, va, rhs = e.matrix_ac(1, b * P + p)
                srp, sci, sva, srhs = single[w, b]
                assert np.array_equal(rp, srp) and np.array_equal(ci, sci), f"{what}: pattern of sweep instance {b * P + p}"
                bad = np.nonzero(bits(va) != bits(sva))[0]
                assert len(bad) == 0, (f"{what}: sweep instance {b * P + p} (instance {b}, omega {w}) value slots {bad[:5]}: {va[bad[:5]]} "
                                       f"against the single-point {sva[bad[:5]]}")
                bad = np.nonzero(bits(rhs) != bits(srhs))[0]
                assert len(bad) == 0, f"{what}: sweep instance {b * P + p} right-hand side rows {bad[:5]}: {rhs[bad[:5]]} against {srhs[bad[:5]]}"
        W.ratio.setdefault("sweep fill bit-identical", 0.0)
        for i, w in enumerate(ws):
            for b in range(B):
                rp, ci, va, rhs = single[w, b]
                check_solution(W, "sweep", rp, ci, va, rhs, x[i, b], f"{what}, sweep point {i} (omega {w}), instance {b}", skeel=len(rp) <= 60)
    e.close()


def check_inf_inductor(knobs, label=""):
    """the AC_OMEGA_ZERO rule: the host writes +0.0 for omega L at omega == 0 whatever L is.  A sign of zero cannot be seen behind the gather
    (0.0 + -0.0 and 0.0 - -0.0 are both +0.0), an infinite L can: base x omega would be inf x 0 = NaN, the rule gives the short"""
    d = Deck()
    a, b = d.new_node(), d.new_node()
    d.add("R", (a, 0), 100.0)
    d.add("R", (b, 0), 200.0)
    d.add("L", (a, b), math.inf)
    d.add("IAC", (0, a), 1e-3, 50.0, 0.4)
    W = Worst()
    e = ac_engine(d, 1, knobs)
    x, rc = e.analyze_ac(0.0, check=False)
    assert rc == 0, rc
    rp, ci, va, rhs = e.matrix_ac(0, 0)
    S = ref_stamp(d.devices, 2, [], 0.0, 0.0, R_OPEN, {}, W.arms)
    check_system(W, "L = inf at omega = 0", cells_of(rp, ci, va), rhs, S, label)
    e2 = ac_engine(d, 1, knobs)
    xs, status, stats = e2.analyze_ac_sweep([0.0, 0.0], check=False)
    assert stats["rc"] == 0 and stats["n_fallback_points"] == 0, (stats, status)
    P = e2.ac_pass_size(1)
    for q in range(P):
        rp2, ci2, va2, rhs2 = e2.matrix_ac(1, q)
        assert np.array_equal(bits(va2), bits(va)) and np.array_equal(bits(rhs2), bits(rhs)), (va2, va)
    assert np.array_equal(bits(xs[0, 0].real), bits(x[0].real)) and np.array_equal(bits(xs[0, 0].imag), bits(x[0].imag))
    W.report(f"AC stamp, infinite inductor at omega = 0 {label}")
    return W


# ---- (b) a mixed deck with shared nodes ---------------------------------------------------------------------------------------------------------
def mixed_block(d, pad_r=0):
    """one block: every linear kind at least once, a diode with tt, a PMOS, an NPN and a PNP on shared nodes; '=' and '+=' stamps meet on the
    cells (k, T = P) of the op-amp and (kP, P = T) of the transformer, '=' over '=' on (k, S = P) of the VCVS; pad_r more parallel resistors"""
    n = [0] + [d.new_node() for _ in range(31)]
    add = d.add
    add("VAC", (n[1], 0), 1.0, 50.0, 0.3)
    add("R", (n[1], n[2]), 1000.0)
    add("C", (n[2], 0), 1e-7)
    add("L", (n[2], n[3]), 1e-3)
    add("R", (n[3], 0), 200.0)
    add("IDC", (0, n[3]), 1e-3)
    add("KL", (n[3], 0, n[4], 0), 1e-3, 4e-3, 0.8)
    add("R", (n[4], 0), 300.0)
    add("VCVS", (n[5], 0, n[5], n[4]), 2.5)
    add("R", (n[5], 0), 1e3)
    add("VCCS", (n[6], 0, n[5], 0), 1e-3)
    add("R", (n[6], 0), 1e3)
    add("C", (n[6], n[5]), 2e-8)
    add("CCCS", (n[7], 0, n[6], n[8]), 2.0)
    add("R", (n[8], 0), 300.0)
    add("R", (n[7], 0), 150.0)
    add("CCVS", (n[9], 0, n[7], n[10]), 500.0)
    add("R", (n[10], 0), 1e3)
    add("R", (n[9], 0), 1e3)
    add("OPAMP", (n[9], n[11], n[11], 0), 1e3)
    add("R", (n[11], 0), 1e3)
    add("XFMR", (n[11], 0, n[12], n[11]), 2.0)
    add("R", (n[12], 0), 120.0)
    add("SW", (n[12], n[13]), 1.0)
    add("R", (n[13], 0), 75.0)
    add("C", (n[13], 0), 2e-7)
    add("SW", (n[13], n[14]), 0.0)      # r_open = 1e12 next to j omega C (the hard case of the refinement)
    add("R", (n[14], 0), 1e4)
    add("C", (n[14], 0), 1e-9)
    add("XCT", (n[13], 0, n[15], 0, n[16]), 2.0)
    add("R", (n[15], 0), 100.0)
    add("R", (n[16], 0), 100.0)
    add("VDC", (n[17], 0), 6.0)
    add("RELAY", (n[17], 0, n[15], n[18]), 5.0, 3.0)
    add("R", (n[18], 0), 1e3)
    add("SAW", (n[19], 0), 5.0, 0.0, 1e3, 0.0)
    add("R", (n[19], n[20]), 1e3)
    add("IAC", (0, n[20]), 1e-3, 50.0, 0.4)
    add("C", (n[20], 0), 1e-7)
    add("VDC", (n[21], 0), 5.0)
    add("R", (n[21], n[22]), 1e3)
    add("D", (n[22], n[23]), *D_TT)
    add("R", (n[23], 0), 100.0)
    add("C", (n[22], 0), 1e-8)
    add("PMOS", (n[24], n[25], n[21]), 1e-3, 0.05, 1.0)
    add("R", (n[24], 0), 500.0)      # (small enough that no resistance of the batch takes the drain past the source: Newton diverges there)
    add("R", (n[21], n[25]), 1e5)
    add("R", (n[25], 0), 1e5)
    add("C", (n[25], n[20]), 1e-7)
    add("VDC", (n[26], 0), 0.85)      # (the BJT models have no junction limiting: a resistor-biased junction does not converge from x = 0
    add("R", (n[21], n[27]), 2.2e3)
    add("NPN", (n[26], n[27], n[28]), 1e-15, 1.0, 150.0, 27.0, 1.0)
    add("VDC", (n[28], 0), 0.25)      #  for every resistance of the batch: base and emitter are held, on nodes that resistors and capacitors share)
    add("R", (n[28], n[20]), 1e4)
    add("C", (n[26], n[2]), 1e-6)
    add("VDC", (n[31], 0), 4.75)
    add("R", (n[31], n[19]), 1e4)
    add("PNP", (n[29], n[30], n[31]), 1e-15, 1.0, 150.0, 27.0, 1.0)
    add("VDC", (n[29], 0), 4.15)
    add("R", (n[29], n[2]), 1e5)
    add("R", (n[30], 0), 2.2e3)
    add("C", (n[30], n[27]), 1e-9)
    for k in range(pad_r):      # parallel resistors and capacitors on nodes that already carry some: more contributions per cell, more value slots
        a = n[2 + (7 * k) % 19]
        if k % 3 == 2:
            add("C", (a, 0), 1e-9 * (1 + k))
        else:
            add("R", (a, 0), 1e4 * (1 + k))


def mixed_deck(blocks=5, pad_r=45, tail=2):
    d = Deck()
    for _ in range(blocks):
        mixed_block(d, pad_r)
    prev = 1
    for _ in range(tail):      # a few rows more
        node = d.new_node()
        d.add("R", (prev, node), 50.0)
        d.add("C", (node, 0), 1e-8)
        prev = node
    return d


def mixed_overrides(deck, B=3):
    """per-instance resistances and capacitances (the nonlinear devices' isolated cells stay isolated: topology is shared)"""
    nR, nC = deck.count("R"), deck.count("C")
    r0 = np.array([p[0] for k, _, p in deck.devices if k == "R"])
    c0 = np.array([p[0] for k, _, p in deck.devices if k == "C"])
    u = pe.deck.uniform01(7, B * (nR + nC)).reshape(B, nR + nC)
    ov = {"R": (r0[None, :] * (0.8 + 0.4 * u[:, :nR]))[:, :, None], "C": (c0[None, :] * (0.5 + u[:, nR:]))[:, :, None]}
    ov["R"][0, :, 0], ov["C"][0, :, 0] = r0, c0
    return ov


MIXED_OMEGAS = [2.0e4, 0.0, 3.0e3, 2.9e4, 3.0e4, 5.0e5]      # shuffled; bands {0}, {3e3 .. 3e4}, {5e5}


def run_mixed(knobs, label, blocks, pad_r, tail, omegas, g_min, skeel_on):
    deck = mixed_deck(blocks, pad_r, tail)
    B = 3
    ov = mixed_overrides(deck, B)
    W = Worst()
    e = ac_engine(deck, B, knobs, ov, g_min)
    st = e.analyze_dc(F.MODE_OP, check=False)
    assert all(s == 0 for s in e.state()["status"]), f"mixed deck: operating point {st}"
    devs = [instance_devices(deck, ov, b) for b in range(B)]
    nl = [nl_values(e, deck, b) for b in range(B)]
    single, shape = {}, None
    for w in omegas:
        x, rc = e.analyze_ac(w, check=False)
        assert rc == 0, f"mixed deck at omega {w}: {rc}"
        for b in range(B):
            what = f"{label} mixed deck ({blocks} blocks), instance {b}, omega {w}"
            rp, ci, va, rhs = e.matrix_ac(0, b)
            S = ref_stamp(devs[b], deck.n_nodes, [], w, g_min, R_OPEN, nl[b], W.arms)
            check_system(W, "mixed deck", cells_of(rp, ci, va), rhs, S, what)
            single[w, b] = (rp.copy(), ci.copy(), va.copy(), rhs.copy())
            check_solution(W, None if "ORACLE" in knobs else "single-point", rp, ci, va, rhs, x[b], what, skeel=skeel_on and b == 1 and w == omegas[0])
            shape = (len(rp) - 1, len(ci))
    return e, deck, ov, W, single, shape, devs, nl


def check_mixed(knobs, label="", big=True):
    """(b), with (c) and (e) on the same deck.  big: 5 blocks padded so that the system has a few rows more than 512 and both the value part
    and the right-hand-side part of the value vector cross workgroup boundaries of k_ac_sweep_fill; else one block (Skeel bound evaluated)"""
    blocks, pad_r, tail = (5, 45, 2) if big else (1, 4, 1)
    e, deck, ov, W, single, shape, devs, nl = run_mixed(knobs, label, blocks, pad_r, tail, MIXED_OMEGAS, GMIN, not big)
    W.need(["omega = 0", "L: short (omega = 0)", "L: -j omega L", "D: j omega tt geq", "D: no diffusion term (omega = 0)", "SW: open", "SW: closed",
            "RELAY: engaged", "XCT: n != 0", "g_min != 0", "time generator: AC short", "IAC: a pin on ground", "VAC: a pin on ground"], "mixed deck")
    if big and "ORACLE" not in knobs:
        rows2 = shape[0]
        assert 512 < rows2 <= 560, rows2
        dv_len = e_dv_len(deck)
        assert dv_len[0] > 512 and dv_len[0] // 256 < (dv_len[0] + rows2) // 256, (dv_len, rows2)
    if "ORACLE" not in knobs:
        mid = [2.0e4, 3.0e3, 2.9e4, 3.0e4, 2.0e4]      # one band, 3.0e4 on its edge 10 w0: with P = 3 the last pass is [2.9e4, 3.0e4, unused]
        sweeps = [(4, MIXED_OMEGAS + [2.0e4]), (3, mid), (0, [0.0, 0.0]), (1, [2.0e4, 3.0e3])]
        check_sweep_identity(deck, 3, knobs, ov, GMIN, [], sweeps if not big else sweeps[:3], single, W, f"{label} mixed deck")
        W.need(["sweep: P > 1", "sweep: last pass partly unused", "sweep: omega = 0 next to nonzero points in one call"] + ([] if big else ["sweep: P = 1"]),
               "mixed deck sweep")
    e.close()
    W.report(f"AC stamp, mixed deck ({blocks} blocks) {label}")
    return W


def e_dv_len(deck):
    """(value slots, i.e. first right-hand-side slot) of the AC value vector: 2 fixed slots + one per value of pe_ac.hpp's AcSlot list"""
    per = {"R": 1, "C": 1, "L": 1, "VAC": 2, "D": 2, "IAC": 2, "VCCS": 1, "VCVS": 1, "CCCS": 1, "CCVS": 1, "OPAMP": 1, "XFMR": 1, "SW": 1, "RELAY": 1,
           "XCT": 2, "KL": 3, "NMOS": 2, "PMOS": 2, "NPN": 2, "PNP": 2}
    return (2 + sum(per.get(k, 0) for k, _, _ in deck.devices),)


# ---- (d) the adjoint system of the noise analysis ---------------------------------------------------------------------------------------------
def check_adjoint(knobs, label=""):
    """matrix_ac(3) after analyze_noise: the exact transpose of the forward real-equivalent matrix at that omega, cell for cell (and the
    reference's transpose within the bounds); the right-hand side the selector alone.  Output pairs: a node against ground (out_neg = -1),
    two nodes, a branch row."""
    W = Worst()
    deck = mixed_deck(1, 4, 1)
    B = 2
    ov = mixed_overrides(deck, B)
    omegas = [3.0e4, 2.0e4]
    branch_row = deck.n_nodes + 1      # the inductor's current (VAC holds the first branch)
    for out_pos, out_neg in ((12, -1), (5, 13), (branch_row, 2)):
        e = ac_engine(deck, B, knobs, ov, GMIN)
        e.analyze_dc(F.MODE_OP)
        devs = [instance_devices(deck, ov, b) for b in range(B)]
        nl = [nl_values(e, deck, b) for b in range(B)]
        e.set_knob("AC_SWEEP_POINTS", 2)      # (a knob drops the main engine's symbolic analysis, not its operating point)
        psd, _, status, stats = e.analyze_noise(omegas, out_pos, out_neg, check=False)
        assert stats["rc"] == 0 and not status.any() and stats["n_retried_points"] == 0, (stats, status)
        P = e.ac_pass_size(3)
        assert P == 2
        last = pass_layout(omegas, P)[-1]
        adj = {(b, p): e.matrix_ac(3, b * P + p) for b in range(B) for p in range(P)}
        for (b, p), (rp, ci, va, rhs) in adj.items():
            w = last[p]
            what = f"{label} adjoint of the mixed block, output ({out_pos}, {out_neg}), instance {b}, omega {w}"
            x, rc = e.analyze_ac(w)
            frp, fci, fva, _ = e.matrix_ac(0, b)
            fwd = sp.csr_matrix((fva, fci, frp), shape=(len(frp) - 1,) * 2)
            T = sp.csr_matrix(fwd.T)
            T.sort_indices()
            assert np.array_equal(T.indptr, rp) and np.array_equal(T.indices, ci), f"{what}: pattern is not the transposed pattern"
            bad = np.nonzero(bits(T.data) != bits(va))[0]
            assert len(bad) == 0, f"{what}: slots {bad[:5]} hold {va[bad[:5]]}, the forward matrix transposed {T.data[bad[:5]]}"
            S = ref_stamp(devs[b], deck.n_nodes, [], w, GMIN, R_OPEN, nl[b], W.arms)
            check_system(W, "adjoint", cells_of(rp, ci, va), None, S, what, transposed=True)
            want = np.zeros(len(rp) - 1)
            want[out_pos] = 1.0
            if out_neg >= 0:
                want[out_neg] = -1.0
            assert np.array_equal(bits(rhs), bits(want)), f"{what}: right-hand side {rhs[np.nonzero(rhs != want)[0][:5]]} is not the selector"
        try:
            e.matrix_ac(2, 0)
            raise AssertionError("the noise analysis' single-point engine never assembles: its values cannot be read")
        except F.PeHipError as ex:
            assert ex.code == F.ERR_ARG
        e.close()
    W.ratio.setdefault("adjoint is the exact transpose", 0.0)
    W.report(f"AC stamp, adjoint {label}")
    return W


# ---- (e) a NaN parameter in a batch of three ----------------------------------------------------------------------------------------------------
def check_nan_instance(knobs, label=""):
    """a NaN parameter in instance 1 of a batch of three, on both paths: a NaN capacitance (a matrix entry) and a NaN source amplitude (the
    right-hand side only: the matrix is sound, the solution is not).  Neither comes back as PE_HIP_OK -- the solve refuses a non-finite pivot
    or solution (PE_HIP_ERR_SINGULAR, DESIGN.md known difference 5), and what passed it would meet the refinement's non-finite test
    (PE_HIP_ERR_INACCURATE) --, the two paths report the same status (a status is per call / per point, over the instances), and the same
    batch with the healthy value solves on both."""
    deck = mixed_deck(1, 4, 1)
    B = 3
    w = 2.0e4
    rcs = {}
    for what, kind, row in (("capacitance", "C", 3), ("IAC amplitude", "IAC", 0)):
        ov = mixed_overrides(deck, B)
        if kind not in ov:
            ov[kind] = np.array([[list(p) for k, _, p in deck.devices if k == kind]] * B, dtype=float)
        good = {k: v.copy() for k, v in ov.items()}
        ov[kind][1, row, 0] = math.nan
        for path in ("single", "sweep"):
            e = ac_engine(deck, B, knobs, ov, GMIN)
            e.analyze_dc(F.MODE_OP)
            if path == "single":
                x, rc = e.analyze_ac(w, check=False)
            else:
                xs, status, stats = e.analyze_ac_sweep([w, 2.5e4], check=False)
                rc = int(status[0])
                assert stats["rc"] == rc and status[1] == rc, (stats, status)
                assert np.all(np.isnan(xs.real)) and np.all(np.isnan(xs.imag)), "a failed point reads NaN"
            assert rc in (F.ERR_SINGULAR, F.ERR_INACCURATE), f"{label} {path}: a NaN {what} came back with status {rc}"
            rcs[what, path] = rc
            e.close()
        assert rcs[what, "single"] == rcs[what, "sweep"], rcs
        e = ac_engine(deck, B, knobs, good, GMIN)
        e.analyze_dc(F.MODE_OP)
        x, rc = e.analyze_ac(w)
        xs, status, stats = e.analyze_ac_sweep([w, 2.5e4])
        assert np.all(np.isfinite(x.real)) and np.all(np.isfinite(xs.real)) and not status.any()
        e.close()
    print(f"RATIOS NaN instance {label}: " + ", ".join(f"{k[0]} ({k[1]}) {v}" for k, v in rcs.items()))
    return rcs


# ---- (f) the band edge of the single-point path -----------------------------------------------------------------------------------------------
def check_band_edge(knobs, label=""):
    """single-point runs at w0, 10 w0, nextafter(10 w0), 0.1 w0, its lower neighbour and 0 -> nonzero -> 0 on ONE engine: each returns phasors
    within the bound of check_solution of the system a fresh engine assembles at that omega (bit-identical to this engine's), so a
    re-analysis or its absence does not show"""
    W = Worst()
    deck = mixed_deck(1, 4, 1)
    B = 2
    ov = mixed_overrides(deck, B)
    w0 = 3.0e3
    seq = [w0, 10.0 * w0, float(np.nextafter(10.0 * w0, math.inf)), w0, 0.1 * w0, w0, float(np.nextafter(0.1 * w0, 0.0)), 0.0, w0, 0.0]
    e = ac_engine(deck, B, knobs, ov, GMIN)
    e.analyze_dc(F.MODE_OP)
    cache = {}
    sym = -1.0
    for step, w in enumerate(seq):
        x, rc = e.analyze_ac(w)
        # the rule of include/pe_hip.h: matched again when there is no order yet, across omega == 0, or more than a decade away
        if sym < 0.0 or (w == 0.0) != (sym == 0.0) or (w != 0.0 and (w > 10.0 * sym or w < 0.1 * sym)):
            sym = w
            W.arms.add("band edge: analysed again")
        else:
            W.arms.add("band edge: order kept" + (" on the edge" if w in (10.0 * sym, 0.1 * sym) else ""))
        assert e.ac_analysis_omega() == sym, f"{label} band edge, step {step} (omega {w!r}): the pivot order is that of {e.ac_analysis_omega()!r}, the rule says {sym!r}"
        f = ac_engine(deck, B, knobs, ov, GMIN)
        f.analyze_dc(F.MODE_OP)
        xf, _ = f.analyze_ac(w)
        for b in range(B):
            what = f"{label} band edge, step {step} (omega {w!r}), instance {b}"
            rp, ci, va, rhs = e.matrix_ac(0, b)
            frp, fci, fva, frhs = f.matrix_ac(0, b)
            assert np.array_equal(ci, fci) and np.array_equal(bits(va), bits(fva)) and np.array_equal(bits(rhs), bits(frhs)), what
            check_solution(W, "band edge", rp, ci, va, rhs, x[b], what, skeel=b == 0, cache=cache)
            check_solution(W, "band edge (fresh engine)", rp, ci, va, rhs, xf[b], what, skeel=b == 0, cache=cache)
        f.close()
    e.close()
    W.need(["band edge: analysed again", "band edge: order kept", "band edge: order kept on the edge"], "band edge")
    W.report(f"AC band edge {label}")
    return W


def check_oracle_within_bound(mod, which):
    """the float64 oracle through the same checks: the bounds are conditions the inputs can meet"""
    knobs = {"ORACLE": mod}
    if which == "single":
        check_single(knobs, "oracle", 0.0, sweep=False)
    elif which == "single_gmin":
        check_single(knobs, "oracle", GMIN, sweep=False)
    else:
        check_mixed(knobs, "oracle", big=False)
