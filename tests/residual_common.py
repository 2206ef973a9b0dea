"""Shared by tests/test_residual_emu.py and tests/test_gpu_residual.py: the residual safety net of the static-pivot LU
-- residual_norms and backward_error of pe_front.hpp, the in-kernel check of the resident kernels with its team_max4 reduction,
k_m2_residual / k_m2_refine_apply / k_m2_clear_eta / k_m2_retest / launch_m2_refine of the split schedule, and the host loop
m2_check_residuals / prepare_inaccurate_retry of pe_engine_newton.cpp -- against a restatement of eta over the engine's own A, b and x,
on solves that really are inaccurate.  Written against the Engine calls only: the same text runs on the host emulation and on the device.

The cell.  IDC (0 -> node) - R (node -> 0) - SW (node -> 0, open), g_min = 0, r_open = 1: rows  v / r + i = I  and  v - r_open i = 0.
The pivot order is matched on instance 0, where r < 1 lets the diagonal 1 / r win; an instance with a large r then pivots on its tiny
1 / r, and the cancellation (I - i) / g destroys v.  eta runs from 1e-14 (r = 1e3) to 0.33 (r >= 1e16): no emulation-only knob.

Reading eta.  The decision is eta <= residual_tol, so the engine's eta is the double t at which a solve is accepted under
residual_tol = t and flagged under nextafter(t, 0).  "Flagged" is read from safety_net(): any counter moved (one instance of
interest), or refined + (instances left as ERR_INACCURATE) (a count over the batch).  Every probe is a fresh engine (the resident
schedule leaves itself for good once the net has tripped).

The reference.  A (CSR, original order) and b come from matrix(b), x from solution() of a run with the check off (residual_tol = -1);
an accepted x is not altered by the check (asserted bitwise wherever an instance is not flagged).  restate() is the kernel's text in
plain double: per row acc = b_i, then acc -= a * x over the row's entries in CSR order, rowsum += |a|; the four maxima
mr = max |acc|, ma = max rowsum, mx = max |x|, mb = max |b| (non-finite counts as +inf); den = ma * mx + mb; eta = mr / den, or
(mr > 0 ? inf : 0) where den is 0.  Twice: every multiply-add unfused (two roundings), and every one fused (exact in fractions, rounded
once) -- the device compiler is free to contract them, a host compiler without an FMA target is not.  The engine must be one of the
two, bit for bit.

The interval (derived from the row lengths, u = 2^-53, gamma_n = n u / (1 - n u), no underflow: asserted on the products).  Row i has
k_i entries.  acc_i = fl(acc - fl(a x)) repeated k_i times gives  acc_i = b_i prod(1 + e_l) - sum_j a_j x_j (1 + d_j) prod_{l >= j}(1 + e_l):
b_i carries k_i roundings and term j at most k_i + 1, so |acc_i - r_i| <= gamma_(k_i + 1) (|b_i| + sum_j |a_j x_j|) =: E_i (a fused
step drops d_j: covered), and |mr - max |r_i|| <= E := max_i E_i.  rowsum_i is a sum of k_i non-negative terms from 0 (k_i - 1
roundings that matter): within gamma_(K - 1) relative, K = max k_i; mx and mb are exact.  den = fl(fl(ma mx) + mb) adds one rounding
on the product and one on the sum of non-negative terms: den within gamma_(K + 1) relative of its exact value D.  The quotient adds
one rounding.  Hence every double evaluation of eta lies in
    [ max(0, R - E) / (D (1 + gamma_(K+1))) (1 - u),  (R + E) / (D (1 - gamma_(K+1))) (1 + u) ],   R = max |r_i| exact,
and eta_exact = R / D.  exact() evaluates this in mpmath at 256 bits; the end points are rounded outwards to doubles.

Forward error.  x* - x = A^-1 (b - A x) exactly, so  |x - x*|_inf <= |A^-1|_inf |r|_inf = cond_inf(A) eta |x|_inf (1 + |b| / (|A| |x|)):
both factors from mpmath (the inverse of the cell's 2 x 2 block), times 1 + 2^-40 for rounding the bound itself.  A repaired instance
must satisfy it with eta_after restated from its final x; the same instance's x with the net off must lie OUTSIDE that bound."""
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

from device_eval_common import F, PE_THREADS
from newton_common import same_bits
from parity_common import pe

mp.mp.prec = 256
U = mp.mpf(2) ** -53
INACC = F.ERR_INACCURATE
NO_CONV = F.ERR_NO_CONVERGENCE
TINY = 5e-324                     # the smallest positive double
DEFAULT_TOL = 1e-10               # apply_options of pe_engine.cpp: residual_tol = 0 means this
M2_RESIDUAL_THREADS = 256         # __launch_bounds__ of k_m2_residual
N_WRAP = 515                      # cells of the wrap deck: 1030 rows, above PE_THREADS and above the k_m2_residual workgroup
SILENT = {"refined": 0, "rematched": 0, "careful": False}
assert 2 * N_WRAP > 2 * PE_THREADS and PE_THREADS >= M2_RESIDUAL_THREADS


def below(t):
    return float(np.nextafter(t, 0.0))


def report(label, what, **figures):
    print(f"RESIDUAL {label} {what}: " + ", ".join(f"{k} {v}" for k, v in figures.items()))


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def _fabs(v):
    return abs(v) if abs(v) <= 1.7976931348623157e308 else math.inf      # finite_abs of pe_front.hpp (NaN -> inf)


def _fms(acc, a, x):
    """fl(acc - a * x) with one rounding"""
    if not (math.isfinite(acc) and math.isfinite(a) and math.isfinite(x)):
        return acc - a * x
    return float(Fraction(acc) - Fraction(a) * Fraction(x))


def _fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


class Restated:
    pass


def restate(A, x, fused, drop=None, row_range=None):
    """the four maxima, their rows and eta of one instance; drop: a row left out (self-checks only)"""
    rp, ci, va, rhs = A
    rows = len(rhs)
    n4, at = [0.0, 0.0, 0.0, 0.0], [-1, -1, -1, -1]
    acc_all = np.zeros(rows)
    for r in (range(rows) if row_range is None else row_range):
        if r == drop:
            continue
        acc, rowsum = float(rhs[r]), 0.0
        for e in range(rp[r], rp[r + 1]):
            a, xv = float(va[e]), float(x[ci[e]])
            acc = _fms(acc, a, xv) if fused else acc - a * xv
            rowsum += abs(a)
        acc_all[r] = acc
        for k, v in enumerate((_fabs(acc), _fabs(rowsum), _fabs(float(x[r])), _fabs(float(rhs[r])))):
            if v > n4[k]:      # (fmax keeps the first of equal values: the row of a tie is the first one)
                n4[k], at[k] = v, r
    den = _fma(n4[1], n4[2], n4[3]) if fused else n4[1] * n4[2] + n4[3]
    out = Restated()
    out.n4, out.rows_at, out.den, out.acc = n4, at, den, acc_all
    out.eta = n4[0] / den if den > 0.0 else (math.inf if n4[0] > 0.0 else 0.0)
    return out


def gamma(n):
    return n * U / (1 - n * U)


def exact(A, x):
    """(eta_exact, lo, hi, R, D) in mpmath / doubles rounded outwards: the interval of the module's docstring"""
    rp, ci, va, rhs = A
    rows = len(rhs)
    R = E = ma = mx = mb = mp.mpf(0)
    K = int(np.max(np.diff(rp)))
    for r in range(rows):
        res, mag, rs = mp.mpf(float(rhs[r])), abs(mp.mpf(float(rhs[r]))), mp.mpf(0)
        for e in range(rp[r], rp[r + 1]):
            t = mp.mpf(float(va[e])) * mp.mpf(float(x[ci[e]]))
            assert t == 0 or abs(t) > mp.mpf(2) ** -960, "a product near the underflow threshold: the interval does not cover it"
            res -= t
            mag += abs(t)
            rs += abs(mp.mpf(float(va[e])))
        k = int(rp[r + 1] - rp[r])
        R, E = max(R, abs(res)), max(E, gamma(k + 1) * mag)
        ma, mx, mb = max(ma, rs), max(mx, abs(mp.mpf(float(x[r])))), max(mb, abs(mp.mpf(float(rhs[r]))))
    D = ma * mx + mb
    if D == 0:
        return 0.0, 0.0, 0.0, R, D
    g = gamma(K + 1)
    lo = max(mp.mpf(0), R - E) / (D * (1 + g)) * (1 - U)
    hi = (R + E) / (D * (1 - g)) * (1 + U)
    lo_d, hi_d = float(lo), float(hi)
    if mp.mpf(lo_d) > lo:
        lo_d = below(lo_d)
    if mp.mpf(hi_d) < hi:
        hi_d = float(np.nextafter(hi_d, math.inf))
    return R / D, lo_d, hi_d, R, D


def dense(A):
    rp, ci, va, rhs = A
    n = len(rhs)
    M = mp.zeros(n, n)
    for r in range(n):
        for e in range(rp[r], rp[r + 1]):
            M[r, int(ci[e])] += mp.mpf(float(va[e]))
    return M, mp.matrix([mp.mpf(float(v)) for v in rhs])


def forward(A, x):
    """(x* of A x = b in mpmath, the bound |A^-1|_inf |b - A x|_inf (1 + 2^-40), |A^-1|_inf) -- small systems only"""
    M, b = dense(A)
    n = len(b)
    Mi = mp.inverse(M)
    xs = Mi * b
    xm = mp.matrix([mp.mpf(float(v)) for v in x])
    r = b - M * xm
    ninv = max(sum(abs(Mi[i, j]) for j in range(n)) for i in range(n))
    rn = max(abs(r[i]) for i in range(n))
    return xs, ninv * rn * (1 + mp.mpf(2) ** -40), ninv


def error_to(xs, x):
    return max(abs(mp.mpf(float(x[i])) - xs[i]) for i in range(len(x)))


# ---- decks ----------------------------------------------------------------------------------------------------------------------------------
class Cells:
    """N cells IDC - R - SW (- D) (- C): cell c has node row c and branch row N + c (read back from the stamp by check_rows)"""

    def __init__(self, N=1, diode=False, cap=0.0):
        d = pe.deck.Deck()
        nodes = [d.new_node() for _ in range(N)]
        for n in nodes:
            d.add("IDC", (0, n), 1.0)
            d.add("R", (n, 0), 1e-3)
            d.add("SW", (n, 0), 0.0)
            if diode:
                d.add("D", (0, n))      # reverse biased by the cell's positive node voltage: g_d of the order of Is / Ut leaves the pivot bad
            if cap > 0.0:
                d.add("C", (n, 0), cap)
        self.N, self.deck, self.cap = N, d, cap
        assert d.n_nodes == N and d.rows == 2 * N

    def overrides(self, r, idc=None, sw=None):
        """r [B][N] (and IDC, SW tables [B][N])"""
        ov = {"R": np.asarray(r, dtype=float)[:, :, None]}
        if idc is not None:
            ov["IDC"] = np.asarray(idc, dtype=float)[:, :, None]
        if sw is not None:
            ov["SW"] = np.asarray(sw, dtype=float)[:, :, None]
        return ov


def check_rows(A, N, cells):
    rp, ci, va, rhs = A
    for c in cells:
        node, br = ci[rp[c]:rp[c + 1]].tolist(), ci[rp[N + c]:rp[N + c + 1]].tolist()
        assert sorted(node) == [c, N + c] and sorted(br) == [c, N + c], f"cell {c}: node row columns {node}, branch row columns {br}"


class Run:
    pass


def engine(deck, batch, overrides, knobs, tol, tols=None, max_newton=0):
    e = F.Engine()
    e.set_options(g_min=0.0, r_open=1.0, residual_tol=tol, max_newton=max_newton, **(tols or {}))
    for k, v in knobs.items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    return e


def solve(deck, batch, overrides, knobs, tol, ana=("DC",), tols=None, max_newton=0, matrices=False, probes=None, keep=False):
    """a fresh engine under residual_tol = tol; ana: ("DC",) / ("OP",) or ("TR", dt, steps)"""
    e = engine(deck, batch, overrides, knobs, tol, tols, max_newton)
    if probes:
        e.set_probes(probes, capacity=8)
        e.arm_probes()
    out = analyse(e, ana, matrices)
    if probes:
        out.probe = e.probe_samples()
    if keep:
        out.engine = e
    else:
        e.close()
    return out


def analyse(e, ana, matrices=False):
    out = Run()
    if ana[0] == "TR":
        out.rc = e.analyze_tr(ana[1], ana[2], check=False)["rc"]
    else:
        out.rc = e.analyze_dc(F.MODE_OP if ana[0] == "OP" else F.MODE_DC, check=False)["rc"]
    st = e.state()
    out.x, out.status, out.iters, out.steps, out.t = e.solution(), st["status"].copy(), st["iters"].copy(), st["steps"].copy(), st["t"].copy()
    out.trace, out.net, out.info = e.newton_trace().tolist(), e.safety_net(), e.info()
    out.fired = out.net != SILENT
    out.flagged = out.net["refined"] + int(np.sum(out.status == INACC))
    out.A = [e.matrix(b) for b in range(e.batch)] if matrices else None
    return out


def forms(off):
    """{"unfused": [Restated per instance], "fused": [...]} of a net-off run (with matrices), and whether the two give the same eta bits"""
    f = {name: [restate(off.A[b], off.x[b], fused) for b in range(len(off.x))] for name, fused in (("unfused", False), ("fused", True))}
    same = all(same_bits(a.eta, b.eta) for a, b in zip(f["unfused"], f["fused"]))
    return f, same


def intervals(off, f, label, what):
    """every restated eta inside the derived interval of its exact value; returns the per-instance (eta_exact, lo, hi)"""
    out = []
    for b in range(len(off.x)):
        ex, lo, hi, _, _ = exact(off.A[b], off.x[b])
        for name in f:
            assert lo <= f[name][b].eta <= hi, f"{label} {what}, instance {b}: the {name} restatement {f[name][b].eta!r} is outside [{lo!r}, {hi!r}] (exact {mp.nstr(ex, 20)})"
        out.append((ex, lo, hi))
    return out


def bisect_eta(probe, lo=TINY, hi=1.0):
    """diagnostic only: the engine's eta as the smallest tolerance that does not flag (probe(t) -> flagged?)"""
    if probe(hi):
        return math.inf
    while below(hi) > lo:
        mid = lo + (hi - lo) / 2.0 if hi / max(lo, TINY) < 4.0 else math.sqrt(lo) * math.sqrt(hi)
        if not (lo < mid < hi):
            break
        if probe(mid):
            lo = mid
        else:
            hi = mid
    return hi


def match_form(f, same, probe_counts, label, what, iv=None):
    """the two-probe assertion over a batch.  probe_counts(t) -> number of flagged instances under residual_tol = t.  For a form's etas
    and each distinct value v > 0 among them: #{eta > v} instances are flagged at v and #{eta >= v} at nextafter(v, 0).  The engine must
    match one form at every value; returns its name ("both" if the restatements coincide)."""
    cache = {}

    def count(t):
        if t not in cache:
            cache[t] = probe_counts(t)
        return cache[t]

    failures, matched = {}, []
    for name in (("unfused",) if same else ("unfused", "fused")):
        etas = [r.eta for r in f[name]]
        bad = []
        for v in sorted({e for e in etas if 0.0 < e < math.inf}):
            want_at, want_below = sum(1 for e in etas if e > v), sum(1 for e in etas if e >= v)
            got_at, got_below = count(v), count(below(v))
            if (got_at, got_below) != (want_at, want_below):
                bad.append(f"eta {v!r}: flagged {got_at} at it (restated {want_at}), {got_below} just below (restated {want_below})")
        if bad:
            failures[name] = bad
        else:
            matched.append(name)
    if matched:
        return "both" if same else matched[0]      # (two restatements that differ cannot both match: their edges differ)
    diag = ""
    if len(f["unfused"]) <= 2:
        diag = f"; bisection over the batch's largest eta gives {bisect_eta(lambda t: count(t) > 0)!r}"
    raise AssertionError(f"{label} {what}: the engine's eta matches neither restatement: {failures}; intervals (exact, lo, hi) {iv}{diag}")


def worst_ratio(f, iv, name):
    """max over instances of |eta_restated - eta_exact| / (its bound), the form the engine matched"""
    w = mp.mpf(0)
    for r, (ex, lo, hi) in zip(f["unfused" if name == "both" else name], iv):
        bound = max(mp.mpf(hi) - ex, ex - mp.mpf(lo))
        if bound > 0:
            w = max(w, abs(mp.mpf(r.eta) - ex) / bound)
    return float(w)


# ---- 1. the inclusive edge across magnitudes ------------------------------------------------------------------------------------------------
EDGE_R = (1e3, 1e8, 1e10, 1e12, 1e13, 1e16)


def check_edges(knobs, label=""):
    """one cell at batch 2 (instance 0: r = 1e-3, the pivot order's), r of instance 1 over EDGE_R; then divider_dc.  The instance of
    interest carries the batch's largest eta, so "any counter moved" reads it."""
    cd = Cells(1)
    got, worst = {}, 0.0
    for r in EDGE_R:
        ov = cd.overrides([[1e-3], [r]])
        off = solve(cd.deck, 2, ov, knobs, -1.0, matrices=True)
        assert off.rc == 0 and not off.fired, (off.rc, off.net)
        check_rows(off.A[1], 1, [0])
        f, same = forms(off)
        iv = intervals(off, f, label, f"edge r = {r:g}")
        assert all(f[n][1].eta > 64.0 * f[n][0].eta for n in f), "instance 1 does not carry the largest eta"

        def flagged(t, ov=ov, off=off):
            on = solve(cd.deck, 2, ov, knobs, t)
            assert on.rc == 0 and same_bits(on.x[0], off.x[0]) and (on.fired or same_bits(on.x, off.x)), f"{label} r = {r:g}, tolerance {t!r}: an accepted x was altered"
            return int(on.fired)
        only1 = {n: [v[1]] for n, v in f.items()}
        name = match_form(only1, same_bits(f["unfused"][1].eta, f["fused"][1].eta), flagged, label, f"edge r = {r:g}", iv)
        got[r] = (f["unfused"][1].eta, name)
        worst = max(worst, worst_ratio(only1, iv[1:], name))
        on = solve(cd.deck, 2, ov, knobs, 0.0)      # the default tolerance
        want = f["unfused"][1].eta > DEFAULT_TOL
        assert all((f[n][1].eta > DEFAULT_TOL) == want for n in f)
        assert on.rc == 0 and on.net["refined"] == int(want) and on.net["rematched"] == 0, (r, on.net)
    d = pe.deck.divider_dc()
    off = solve(d, 1, None, knobs, -1.0, matrices=True)
    f, same = forms(off)
    iv = intervals(off, f, label, "divider_dc")

    def flagged(t):
        on = solve(d, 1, None, knobs, t)
        assert on.fired or (on.rc == 0 and same_bits(on.x, off.x))
        return int(on.fired)
    eta0 = f["unfused"][0].eta
    name = match_form(f, same, flagged, label, "divider_dc", iv) if eta0 > 0.0 else "zero"
    on = solve(d, 1, None, knobs, 0.0)
    assert on.rc == 0 and not on.fired and same_bits(on.x, off.x) and eta0 < 1e-15, (on.net, eta0)
    report(label, "edges", **{f"r={r:g}": f"{e!r} ({n})" for r, (e, n) in got.items()}, divider_dc=f"{eta0!r} ({name})", worst_over_bound=f"{worst:.3g}")
    return got


# ---- 2. every reduction at every thread position ----------------------------------------------------------------------------------------------
def wrap_positions(N):
    node = sorted({0, 63, 64, 255, 256, PE_THREADS - 1, PE_THREADS, N - 1})
    branch = sorted({N, 767, 768, 2 * N - 1})
    return [p for p in node if p < N], [p for p in branch if N <= p < 2 * N]


# the four cells that carry the four maxima by their own parameters, and the cell each one sits in while another one is being moved
MOVERS = {
    "max |r|": dict(home=300, r=1e12, idc=1.0, sw=0.0, cls="branch"),      # the bad cell: its residual sits on its branch row
    "max |x|": dict(home=301, r=1e-3, idc=20.0, sw=1.0, cls="branch"),     # switch closed: v = 0, i = I on the branch row
    "max |b|": dict(home=302, r=1e-3, idc=100.0, sw=0.0, cls="node"),      # the source's entry of b sits on the node row
    "max row sum": dict(home=303, r=2.0 ** -20, idc=1.0, sw=0.0, cls="node"),      # 1 / r + 1 on the node row
}


def check_positions(knobs, label=""):
    """N_WRAP cells; instance 0 all healthy (r = 1e-3: the pivot order's), every other instance holds the four cells of MOVERS, one of
    them placed so that its maximum sits on a wanted row, the other three at home.  Where a maximum can sit is the cell's: the residual
    of the bad cell and the switch current on branch rows (N ..), the source's b and the row sum 1 / r + r_open on node rows (.. N - 1);
    together the four visit row 0, 63 / 64, 255 / 256, 511 / 512, 767 / 768, N - 1 / N and the last row, and all four maxima go through the
    same loop and the same reduction at every position.  The parameters do not depend on the position, so every placement must come to
    one and the same eta, bit for bit -- a row that a stride, an offset or a reduction loses changes that instance's eta alone."""
    N = N_WRAP
    node_rows, branch_rows = wrap_positions(N)
    cd = Cells(N)
    place = [(m, p) for m, s in MOVERS.items() for p in (node_rows if s["cls"] == "node" else branch_rows)]
    B = 1 + len(place)
    r, idc, sw = np.full((B, N), 1e-3), np.ones((B, N)), np.zeros((B, N))
    homes = {s["home"] for s in MOVERS.values()}
    for b, (m, p) in enumerate(place, start=1):
        c = p if p < N else p - N
        assert c not in homes
        for m2, s in MOVERS.items():
            at = c if m2 == m else s["home"]
            r[b, at], idc[b, at], sw[b, at] = s["r"], s["idc"], s["sw"]
    ov = cd.overrides(r, idc, sw)
    off = solve(cd.deck, B, ov, knobs, -1.0, matrices=True)
    assert off.rc == 0 and not off.fired
    check_rows(off.A[1], N, [0, N // 2, N - 1])
    f, same = forms(off)
    iv = intervals(off, f, label, "positions")
    for b, (m, p) in enumerate(place, start=1):      # the self-checks: this placement can fail
        for name, fused in (("unfused", False), ("fused", True)):
            R = f[name][b]
            assert len(set(R.rows_at)) == 4, f"{label} {m} on row {p}: the four maxima sit on rows {R.rows_at}"
            k = {"max |r|": 0, "max row sum": 1, "max |x|": 2, "max |b|": 3}[m]      # the order of residual_norms' out4
            assert R.rows_at[k] == p, f"{label} {m} on row {p}: that maximum sits on row {R.rows_at[k]}"
            assert not same_bits(restate(off.A[b], off.x[b], fused, drop=p).eta, R.eta), f"{label} {m} on row {p}: dropping the row leaves eta unchanged"
    for name in f:
        assert len({r_.eta for r_ in f[name][1:]}) == 1, f"{label}: the {name} restatement differs between placements"

    def counts(t):
        on = solve(cd.deck, B, ov, knobs, t)
        assert on.rc == 0 and on.net["rematched"] == 0 and not on.status.any(), (t, on.net, on.status)
        changed = [b for b in range(B) if not same_bits(on.x[b], off.x[b])]
        assert len(changed) <= on.flagged, f"{label} positions, tolerance {t!r}: {len(changed)} instances changed, {on.flagged} were flagged"
        return on.flagged
    etas = {n: v[1:] for n, v in f.items()}      # instance 0 (eta about 1e-17) is read alone: a batch of one below
    name = match_form(etas, all(same_bits(a.eta, b_.eta) for a, b_ in zip(etas["unfused"], etas["fused"])), counts, label, "positions", iv[1:2])
    one = solve(cd.deck, 1, cd.overrides(r[:1], idc[:1], sw[:1]), knobs, -1.0, matrices=True)
    assert same_bits(one.x[0], off.x[0])
    f1, same1 = forms(one)

    def alone(t):
        return int(solve(cd.deck, 1, cd.overrides(r[:1], idc[:1], sw[:1]), knobs, t).fired)
    name0 = match_form(f1, same1, alone, label, "positions, instance 0 alone", iv[:1])
    info = off.info
    report(label, "positions", instances=B, eta=repr(f["unfused"][1].eta), form=name, eta0=repr(f1["unfused"][0].eta), form0=name0,
           rows="/".join(str(p) for p in node_rows + branch_rows), ew_grid=info["ew_grid"], worst_over_bound=f"{worst_ratio(f, iv, name):.3g}")
    return name, info


# ---- 3. refinement really repairs, per instance ---------------------------------------------------------------------------------------------
MIX_R = (1e12, 1e10, 1e3, 1e16, 1e8, 1e-3, 1e13, 3e14, 1e5)
EDGE_OF_MIX = 1e10


def check_repair(knobs, B, label=""):
    """one cell, batch B: instance 0 r = 1e-3, instance b r = MIX_R[(b - 1) % 9] (b / 7 added to the mantissa from the second turn on);
    the tolerance is the restated eta of the first instance with r = 1e10 -- that instance sits exactly on the edge and is not
    flagged; under the next double below it is"""
    cd = Cells(1)
    r = np.array([1e-3] + [MIX_R[(b - 1) % len(MIX_R)] * (1.0 + ((b - 1) // len(MIX_R)) / 7.0) for b in range(1, B)])
    r = r[:B]
    ov = cd.overrides(r[:, None])
    off = solve(cd.deck, B, ov, knobs, -1.0, matrices=True)
    assert off.rc == 0 and not off.fired
    f, same = forms(off)
    intervals(off, f, label, f"repair batch {B}")
    edge = next(b for b in range(B) if r[b] == EDGE_OF_MIX)
    problems, passed = {}, []
    for name in (("unfused",) if same else ("unfused", "fused")):
        etas = np.array([v.eta for v in f[name]])
        try:
            for tol, edge_flagged in ((float(etas[edge]), False), (below(float(etas[edge])), True)):
                want = etas > tol
                assert bool(want[edge]) == edge_flagged and want.any() and not want.all()
                on = solve(cd.deck, B, ov, knobs, tol, matrices=True)
                w = f"{label} repair batch {B} ({name}), tolerance {tol!r}"
                assert on.rc == 0 and not on.status.any(), f"{w}: rc {on.rc}, status {on.status}"
                assert on.net["refined"] == int(want.sum()) and on.net["rematched"] == 0, f"{w}: {on.net}, the restatement flags {int(want.sum())}"
                assert on.net["careful"] == (knobs["SPLIT"] == 0), f"{w}: careful {on.net['careful']}"
                n_out = 0
                for b in range(B):
                    if not want[b]:
                        assert same_bits(on.x[b], off.x[b]), f"{w}: instance {b} (eta {etas[b]!r}) was not flagged but changed"
                        continue
                    after = [restate(on.A[b], on.x[b], fu).eta for fu in (False, True)]
                    assert max(after) <= tol, f"{w}: instance {b} repaired to eta {after} above the tolerance"
                    xs, bound, ninv = forward(on.A[b], on.x[b])
                    assert same_bits(on.A[b][2], off.A[b][2]) and same_bits(on.A[b][3], off.A[b][3])
                    err_on, err_off = error_to(xs, on.x[b]), error_to(xs, off.x[b])
                    assert err_on <= bound, f"{w}: instance {b}: |x - x*| = {mp.nstr(err_on, 5)} above cond * eta_after bound {mp.nstr(bound, 5)}"
                    assert err_off > bound, f"{w}: instance {b}: the net-off x is inside the bound of the repaired one ({mp.nstr(err_off, 5)} <= {mp.nstr(bound, 5)}): nothing was repaired"
                    n_out += 1
                assert n_out == int(want.sum())
            passed.append(name)
        except AssertionError as exc:
            problems[name] = str(exc)
    assert passed, f"{label} repair batch {B}: neither restatement predicts the engine: {problems}"
    # (where the two restatements differ only in instances away from the edge, both predict the same sets and both pass)
    form = "both (coincide)" if same else " and ".join(passed)
    report(label, f"repair batch {B}", form=form, tolerance=repr(float(etas[edge])), flagged=int((etas > float(etas[edge])).sum()), edge_instance=edge,
           distinct_eta=len(set(etas.tolist())))
    return form


# ---- 4. non-linear: k_m2_retest -----------------------------------------------------------------------------------------------------------------
def newton_tols(scale):
    """absolute tolerances only, node and branch alike: the step of the refinement's correction decides"""
    return dict(v_abstol=scale, i_abstol=scale, v_reltol=1e-300, i_reltol=1e-300)


def check_retest(knobs, label=""):
    """the cell with a diode across it (instance 0 healthy, instance 1 r = 1e12).  With the net off the accepted iterate of instance 1
    is off by c = |x_off - x*| (x*: the mpmath solution of its last linearisation).  The refinement moves x by about c after the
    Newton test has passed, and k_m2_retest judges the moved x against xprev: under Newton tolerances of c / 100 it violates, the solve
    takes exactly one more iteration than with the net off and converges; under 100 c it does not, and the count stays.
    On the resident schedule the flagged instance's solve fails inside the kernel and is repeated from its own (failed) iterate on the
    host-driven schedule; iters counts accepted solves only, so the repeated solve's count is what is reported."""
    cd = Cells(1, diode=True)
    ov = cd.overrides([[1e-3], [1e12]])
    probe = solve(cd.deck, 2, ov, knobs, -1.0, ana=("OP",), matrices=True)
    assert probe.rc == 0, (probe.rc, probe.status)
    xs, _, _ = forward(probe.A[1], probe.x[1])
    c = float(error_to(xs, probe.x[1]))
    assert 1e-9 < c < 1e-2, c
    out = {}
    for which, scale in (("small", c / 100.0), ("large", c * 100.0)):
        tols = newton_tols(scale)
        off = solve(cd.deck, 2, ov, knobs, -1.0, ana=("OP",), tols=tols, matrices=True)
        assert off.rc == 0 and not off.status.any() and off.trace == [int(off.iters[0])], (off.rc, off.status, off.trace, off.iters)
        f, same = forms(off)
        assert all(v[1].eta > DEFAULT_TOL and v[0].eta <= DEFAULT_TOL for v in f.values()), [(v[0].eta, v[1].eta) for v in f.values()]
        on = solve(cd.deck, 2, ov, knobs, 0.0, ana=("OP",), tols=tols, matrices=True)
        w = f"{label} retest, {which} Newton tolerances ({scale:.3g})"
        assert on.rc == 0 and not on.status.any(), f"{w}: rc {on.rc}, status {on.status}"
        assert on.net["rematched"] == 0 and on.net["refined"] >= 1 and on.net["careful"] == (knobs["SPLIT"] == 0), f"{w}: {on.net}"
        assert same_bits(on.x[0], off.x[0]) and on.iters[0] == off.iters[0] and on.trace == off.trace, f"{w}: the healthy instance changed"
        extra = 1 if which == "small" else 0
        if knobs["SPLIT"]:
            want = int(off.iters[1]) + extra
        else:
            # the repeated solve starts on the failed (converged, inaccurate) iterate: one iteration reproduces it and passes the Newton
            # test at once; then the refinement, and one more iteration where the corrected x violates
            want = 1 + extra
        assert on.iters[1] == want, f"{w}: iters {on.iters.tolist()} (net off {off.iters.tolist()}), expected {want} for the flagged instance"
        after = [restate(on.A[1], on.x[1], fu).eta for fu in (False, True)]
        assert max(after) <= DEFAULT_TOL, f"{w}: eta after {after}"
        xs_on, bound, _ = forward(on.A[1], on.x[1])
        assert error_to(xs_on, on.x[1]) <= bound
        assert error_to(xs_on, off.x[1]) > bound, f"{w}: the net-off x lies inside the repaired bound"
        out[which] = (off.iters.tolist(), on.iters.tolist(), on.net["refined"])
    report(label, "retest", correction=f"{c:.3g}", **{k: f"off {a} on {b} refined {n}" for k, (a, b, n) in out.items()})
    return out


# ---- 5. transient ---------------------------------------------------------------------------------------------------------------------------
TR_DT = 2.0 ** -20
TR_CAP = 2.0 ** -70      # 2 C / dt = 2^-49 = 1.8e-15: far below 1 / r = 1e-12, the pivot stays bad


def trapezoid(r, cap, dt, steps, idc=1.0):
    """the cell in mpmath from the all-zero state: (1 / r + 1 + 2 C / dt) v' = I + (2 C / dt) v + i_C,  i_C' = (2 C / dt) (v' - v) - i_C"""
    g = 2 * mp.mpf(cap) / mp.mpf(dt)
    v = ic = mp.mpf(0)
    for _ in range(steps):
        vn = (mp.mpf(idc) + g * v + ic) / (1 / mp.mpf(r) + 1 + g)
        ic = g * (vn - v) - ic
        v = vn
    return mp.matrix([v, v])      # (r_open = 1: the switch current equals v)


def check_transient(knobs, label=""):
    """the cell with a capacitor, batch 3 (r = 1e-3, 1e12, 1e3), three steps of TR_DT from reset().  Step by step: an engine with the net
    on takes one step at a time; before each, its checkpoint goes to a net-off engine that takes the same step and shows the x the check
    sees -- restated, it says which instances the step flags.  Then one uninterrupted analyze_tr(dt, 3), and once more with probes."""
    cd = Cells(1, cap=TR_CAP)
    rr = [1e-3, 1e12, 1e3]
    B = len(rr)
    ov = cd.overrides([[v] for v in rr])
    E = engine(cd.deck, B, ov, knobs, 0.0)      # (SPLIT = 0 keeps every call's first attempt on the resident kernel, careful or not)
    flagged_pairs, bounds = 0, [mp.mpf(0)] * B
    first_flagged = None
    for s in range(3):
        blob = E.checkpoint()
        o = engine(cd.deck, B, ov, knobs, -1.0)
        o.restore(blob)
        off = analyse(o, ("TR", TR_DT, 1), matrices=True)
        o.close()
        assert off.rc == 0 and not off.fired
        f, same = forms(off)
        intervals(off, f, label, f"transient step {s}")
        want = np.array([v.eta > DEFAULT_TOL for v in f["unfused"]])
        assert want.tolist() == [v.eta > DEFAULT_TOL for v in f["fused"]] and want[1] and not want[0], (s, [v.eta for v in f["unfused"]])
        before = E.safety_net()["refined"]
        on = analyse(E, ("TR", TR_DT, 1), matrices=True)
        assert on.rc == 0 and not on.status.any() and np.all(on.steps == s + 1), (on.rc, on.status, on.steps)
        assert on.net["refined"] - before == int(want.sum()) and on.net["rematched"] == 0, f"{label} TR step {s}: {on.net}, was {before}, flags {want.tolist()}"
        for b in range(B):
            if not want[b]:
                assert same_bits(on.x[b], off.x[b])
                xs, bnd, ninv = forward(off.A[b], off.x[b])
            else:
                assert max(restate(on.A[b], on.x[b], fu).eta for fu in (False, True)) <= DEFAULT_TOL
                xs, bnd, ninv = forward(on.A[b], on.x[b])
                assert error_to(xs, off.x[b]) > bnd, f"{label} TR step {s}, instance {b}: the net-off x lies inside the repaired bound"
            g = 2.0 * TR_CAP / TR_DT
            assert 16.0 * g * float(ninv) <= 2.0 ** -20      # what a step's error adds to the next step's b: below 2^-20 of itself
            bmax = max(abs(mp.mpf(float(v))) for v in on.A[b][3])
            bounds[b] += bnd + ninv * 8 * U * bmax      # (the engine's b is the rounded companion history)
        if want.any() and first_flagged is None:
            first_flagged = s
        flagged_pairs += int(want.sum())
    x_steps, net_steps = E.solution(), E.safety_net()
    E.close()
    assert first_flagged == 0 and flagged_pairs >= 3
    for b in range(B):
        err = error_to(trapezoid(rr[b], TR_CAP, TR_DT, 3), x_steps[b])
        assert err <= bounds[b] * (1 + mp.mpf(2) ** -20), f"{label} TR: instance {b} is {mp.nstr(err, 5)} from the 256-bit trapezoid, bound {mp.nstr(bounds[b], 5)}"
    off3 = solve(cd.deck, B, ov, knobs, -1.0, ana=("TR", TR_DT, 3))
    assert error_to(trapezoid(rr[1], TR_CAP, TR_DT, 3), off3.x[1]) > bounds[1] * (1 + mp.mpf(2) ** -20), "the net-off transient lies inside the bound"
    for probes in (None, [0, 1]):
        on = solve(cd.deck, B, ov, knobs, 0.0, ana=("TR", TR_DT, 3), probes=probes)
        w = f"{label} TR uninterrupted" + (" with probes" if probes else "")
        assert on.rc == 0 and not on.status.any() and np.all(on.steps == 3) and np.all(on.t == 3 * TR_DT), f"{w}: rc {on.rc}, {on.status}, {on.steps}"
        assert on.net["refined"] == flagged_pairs and on.net["rematched"] == 0, f"{w}: {on.net}, the restatement flags {flagged_pairs} (instance, step) pairs"
        assert on.net["careful"] == (knobs["SPLIT"] == 0), f"{w}: {on.net}"
        assert same_bits(on.x, x_steps), f"{w}: not the step-by-step solution"
        if probes:
            t, val, n_rec, n_drop = on.probe
            assert n_rec.tolist() == [4] * B and not n_drop.any(), (n_rec, n_drop)      # the armed state, then three accepted steps: none twice, none lost
            assert same_bits(val[:, 3, :], on.x[:, probes]) and np.all(t[:, 3] == on.t)
    report(label, "transient", flagged_pairs=flagged_pairs, refined=net_steps["refined"])
    return flagged_pairs


# ---- 6. degenerate norms ----------------------------------------------------------------------------------------------------------------------
def check_degenerate(knobs, label=""):
    cd = Cells(1)
    # all sources zero: eta = 0, accepted under the smallest positive tolerance
    ov = cd.overrides([[1e-3], [1e12]], idc=[[0.0], [0.0]])
    for tol in (-1.0, TINY, 0.0):
        z = solve(cd.deck, 2, ov, knobs, tol, matrices=True)
        assert z.rc == 0 and not z.fired and not z.x.any() and not z.status.any(), (tol, z.net, z.x)
        assert restate(z.A[1], z.x[1], False).eta == 0.0
    # residual_tol = 0 is 1e-10: a scan of r finds the instance just at or below 1e-10 and the one just above
    B = 129
    r = np.array([1e-3] + [10.0 ** (6.0 + 3.0 * k / (B - 2)) for k in range(B - 1)])
    scan = solve(cd.deck, B, cd.overrides(r[:, None]), knobs, -1.0, matrices=True)
    f, same = forms(scan)
    etas = {n: np.array([v.eta for v in f[n]]) for n in f}
    agree = [b for b in range(1, B) if (etas["unfused"][b] > DEFAULT_TOL) == (etas["fused"][b] > DEFAULT_TOL)]
    lo = max((b for b in agree if etas["unfused"][b] <= DEFAULT_TOL), key=lambda b: etas["unfused"][b])
    hi = min((b for b in agree if etas["unfused"][b] > DEFAULT_TOL), key=lambda b: etas["unfused"][b])
    assert 0.25 * DEFAULT_TOL < etas["unfused"][lo] <= DEFAULT_TOL < etas["unfused"][hi] < 4.0 * DEFAULT_TOL, (etas["unfused"][lo], etas["unfused"][hi])
    for b, fires in ((lo, False), (hi, True)):
        ov2 = cd.overrides([[1e-3], [r[b]]])
        off = solve(cd.deck, 2, ov2, knobs, -1.0)
        assert same_bits(off.x[1], scan.x[b]), "the scan's instance alone is not the same solve"
        for tol in (0.0, DEFAULT_TOL):
            on = solve(cd.deck, 2, ov2, knobs, tol)
            assert on.rc == 0 and on.fired == fires and on.net["refined"] == int(fires), f"{label} degenerate: r {r[b]!r} eta {etas['unfused'][b]!r} under residual_tol {tol!r}: {on.net}"
            assert fires or same_bits(on.x, off.x)
    # negative tolerances switch the check off, however bad the solve
    ov3 = cd.overrides([[1e-3], [1e16]])
    ref = solve(cd.deck, 2, ov3, knobs, -1.0, matrices=True)
    assert restate(ref.A[1], ref.x[1], False).eta > 0.1
    for tol in (-TINY, -1e-300, -1e300, -math.inf):
        n = solve(cd.deck, 2, ov3, knobs, tol)
        assert n.rc == 0 and not n.fired and not n.status.any() and same_bits(n.x, ref.x), (tol, n.net)
    report(label, "degenerate", below=f"r {r[lo]!r} eta {etas['unfused'][lo]!r}", above=f"r {r[hi]!r} eta {etas['unfused'][hi]!r}", eta_r1e16=repr(restate(ref.A[1], ref.x[1], False).eta))
    return r[lo], r[hi]


# ---- 7. failure stays clean ---------------------------------------------------------------------------------------------------------------------
def check_failure(knobs, label=""):
    """an unreachable tolerance (1e-30) on a batch whose instances 0 and 2 have no source (x = 0, eta = 0) and whose other instances have
    eta > 0: bad cells (r = 1e12, 1e3, 2.9e5), which a refinement of this 2 x 2 block takes to a residual of exactly 0, and healthy
    ones (r = 1e-3, 3e-3, 0.7) at 1e-17, which neither refinement nor a re-match improves.  One DC point, then one TR step."""
    cd = Cells(1, cap=TR_CAP)
    r, idc = [[0.5], [1e12], [1.0], [1e3], [1e-3], [3e-3], [0.7], [2.9e5]], [[0.0], [1.0], [0.0], [1.0], [1.0], [0.3], [1.1], [0.9]]
    B, exact_ones, others = len(r), [0, 2], [1, 3, 4, 5, 6, 7]
    ov = cd.overrides(r, idc)
    out = {}
    for ana in (("DC",), ("TR", TR_DT, 1)):
        off = solve(cd.deck, B, ov, knobs, -1.0, ana=ana, matrices=True)
        assert off.rc == 0
        f, _ = forms(off)
        etas = {n: [v.eta for v in f[n]] for n in f}
        assert all(all(e[b] == 0.0 for b in exact_ones) and all(e[b] > 1e-30 for b in others) for e in etas.values()), etas
        on = solve(cd.deck, B, ov, knobs, 1e-30, ana=ana, matrices=True, keep=True)
        e = on.engine
        w = f"{label} failure {ana[0]}"
        assert not on.status[exact_ones].any() and same_bits(on.x[exact_ones], off.x[exact_ones]), f"{w}: the exact instances: status {on.status}"
        for b in others:      # flagged: left as inaccurate, or (after the re-match on its own values) solved to eta <= 1e-30
            assert on.status[b] == INACC or (on.status[b] == 0 and max(restate(on.A[b], on.x[b], fu).eta for fu in (False, True)) <= 1e-30), f"{w}: instance {b}: status {on.status[b]}"
        assert (on.status == INACC).any() and on.rc == INACC, f"{w}: rc {on.rc}, status {on.status}"
        assert on.net["careful"] and on.net["rematched"] >= 1, f"{w}: {on.net}"
        if ana[0] == "TR":      # rolled back: a failed instance stays at t = 0 with no step counted, the others moved on
            for b in range(B):
                ok = on.status[b] == 0
                assert on.steps[b] == int(ok) and on.t[b] == (TR_DT if ok else 0.0), f"{w}: instance {b}: steps {on.steps[b]}, t {on.t[b]}"
        assert np.array_equal(on.iters[on.status == INACC], np.zeros(int((on.status == INACC).sum()), dtype=np.int64)), f"{w}: iters {on.iters}"
        # not sticky: the same engine under the default tolerance goes on
        e.set_options(g_min=0.0, r_open=1.0, residual_tol=0.0)
        again = analyse(e, ana, matrices=True)
        e.close()
        assert again.rc == 0 and not again.status.any(), f"{w}: after the failure: rc {again.rc}, status {again.status}"
        for b in range(B):
            assert max(restate(again.A[b], again.x[b], fu).eta for fu in (False, True)) <= DEFAULT_TOL, f"{w}: instance {b} after the failure"
        out[ana[0]] = (on.status.tolist(), on.net)
    report(label, "failure", **{k: f"status {s} net {n}" for k, (s, n) in out.items()})
    return out
