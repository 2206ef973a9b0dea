"""Shared bodies of the tests of the backward-Euler and Gear-2 integration rules of the transient (pe_hip_set_tr_method /
pe_hip_get_tr_history / pe_hip_sweep_set_tr_method, include/pe_hip.h): tests/test_integ_emu.py runs them on the host emulation, one
child process per case, tests/test_gpu_integ.py on the device -- there the 512-thread team of the resident kernels (the barrier between
the reads of h_p and its commit), the grid-wide team of the split schedule with the commit as a launch of its own, and the captured
launch sequences are what is added.

The reference is never the engine under test: Ref is a dense numpy integrator of the descriptor form E x' + G x = b(t) of the MNA system,
built here from the deck.  A step solves (G + a0 E) x_{n+1} = b(t_{n+1}) - E (a1 x_n + a2 x_{n-1}) with numpy.linalg.solve and the
coefficient table of the header, the BE start and the fallback at rho > 1 + sqrt 2 included; for linear circuits that is algebraically the
per-element companion form.  Tolerance: the project's LIN = (1e-9, 1e-7) through max_err.  A junction adds its current and the diffusion
capacitance cd = tt geq, frozen at the last linearisation of the previous step as the engine freezes it; Newton runs to 1e-13; tolerance
NL = (1e-6, 1e-5).  The controller cases restate the bodies of tests/test_tr_adaptive_emu.py with the estimates and exponents of the two
rules."""
import math

import numpy as np

from parity_common import max_err, pe

F, D = pe.ffi, pe.deck
LIN = (1e-9, 1e-7)
NL = (1e-6, 1e-5)
TRAP, BE, GEAR2 = 0, 1, 2
RHO_MAX = 1.0 + math.sqrt(2.0)
EPS4 = 4 * np.finfo(float).eps
H = 1e-7
W = 2.0 * math.pi * 2e5
TT = 1e-7


# ---------------------------------------------------------------------------------------------------------------- decks
def c_only():
    d = D.Deck()
    d.n_nodes = 3
    d.add("VAC", (1, 0), 2.0, W, 0.0)
    d.add("R", (1, 2), 100.0)
    d.add("C", (2, 0), 1e-8)
    d.add("R", (2, 3), 200.0)
    d.add("C", (3, 0), 5e-9)
    d.add("C", (1, 3), 2e-9)
    return d


def l_only():
    d = D.Deck()
    d.n_nodes = 3
    d.add("VAC", (1, 0), 2.0, W, 0.0)
    d.add("R", (1, 2), 100.0)
    d.add("L", (2, 3), 1e-4)
    d.add("R", (3, 0), 50.0)
    d.add("L", (2, 0), 3e-4)
    return d


def kl_only():
    d = D.Deck()
    d.n_nodes = 4
    d.add("VAC", (1, 0), 2.0, W, 0.0)
    d.add("R", (1, 2), 100.0)
    d.add("KL", (2, 0, 3, 0), 1e-4, 4e-4, 0.9)
    d.add("R", (3, 0), 300.0)
    d.add("KL", (3, 0, 4, 0), 2e-4, 1e-4, 0.5)
    d.add("R", (4, 0), 100.0)
    return d


def d_only():
    d = D.Deck()
    d.n_nodes = 3
    d.add("VAC", (1, 0), 2.0, W, 0.0)
    d.add("R", (1, 2), 100.0)
    d.add("D", (2, 3), 1e-14, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 1.0, 1.0, TT)
    d.add("R", (3, 0), 100.0)
    d.add("D", (2, 0), 1e-13, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 1.0, 1.0, 3 * TT)
    return d


def mixed():
    d = D.Deck()
    d.n_nodes = 6
    d.add("VAC", (1, 0), 2.0, W, 0.0)
    d.add("R", (1, 2), 100.0)
    d.add("C", (2, 0), 1e-8)
    d.add("L", (2, 3), 1e-4)
    d.add("R", (3, 0), 150.0)
    d.add("D", (3, 4), 1e-14, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 1.0, 1.0, TT)
    d.add("C", (4, 0), 4e-9)
    d.add("R", (4, 0), 200.0)
    d.add("KL", (3, 0, 5, 0), 1e-4, 2e-4, 0.8)
    d.add("R", (5, 6), 100.0)
    d.add("L", (6, 0), 2e-4)
    d.add("D", (5, 0), 1e-13, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 1.0, 1.0, 2 * TT)
    d.add("C", (5, 6), 1e-9)
    return d


def rl_edge():
    """series R = 1 Ohm, L = 1 nH behind a square source that falls from 1 V to 0 at t = 250 ns (between steps 2 and 3 at h = 100 ns):
    from its operating point (i = 1 A) the inductor current decays from 1 A, so that the inductor voltage -R i keeps its relative accuracy
    all the way down (a rising edge would leave V - R i, which cancels to the rounding floor after eight steps)"""
    d = D.Deck()
    d.n_nodes = 2
    d.add("SQR", (1, 0), 1.0, 0.0, 1e5, 0.025, 0.0)
    d.add("R", (1, 2), 1.0)
    d.add("L", (2, 0), 1e-9)
    return d


def rlc():
    """series R = 10 Ohm, L = 1 mH, C = 1 uF driven by a 2 kHz unit sine"""
    d = D.Deck()
    d.n_nodes = 3
    d.add("VAC", (1, 0), 1.0, 2.0 * math.pi * 2e3, 0.0)
    d.add("R", (1, 2), 10.0)
    d.add("L", (2, 3), 1e-3)
    d.add("C", (3, 0), 1e-6)
    return d


DECKS = {"c_only": c_only, "l_only": l_only, "kl_only": kl_only, "d_only": d_only, "mixed": mixed}


def overrides(deck, batch):
    """per-instance R and C values: instance b scales every R by 1 + 0.3 b / batch and every C by 1 - 0.2 b / batch"""
    ov = {}
    for kind, f in (("R", 0.3), ("C", -0.2)):
        vals = [p[0] for k, _, p in deck.devices if k == kind]
        if vals:
            ov[kind] = np.array([[[v * (1.0 + f * b / batch)] for v in vals] for b in range(batch)])
    return ov


def engine(deck, knobs=None, batch=1, ov=None, method=None, gmin=0.0, **opt):
    e = F.Engine()
    e.set_options(g_min=gmin, **opt)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    if method is not None:
        e.set_tr_method(method)
    e.load_deck(deck, batch, ov)
    e.reset()
    return e


def set_time(e, t, last_step):
    import ctypes as C
    fn = F.lib().pe_hip_set_time
    fn.argtypes = [C.c_void_p, C.c_double, C.c_double]
    e._chk(fn(e._h, float(t), float(last_step)))


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


# ---------------------------------------------------------------------------------------------------------------- the restatement
def coef(method, h, hp, fallback=True):
    if method == GEAR2 and hp > 0.0 and (not fallback or not (h / hp > RHO_MAX)):
        rho = h / hp
        return (1 + 2 * rho) / (h * (1 + rho)), -(1 + rho) / h, rho * rho / (h * (1 + rho))
    return 1.0 / h, -1.0 / h, 0.0


class Ref:
    """descriptor form of one instance of a deck: rows as the engine numbers them (nodes in creation order, then branches in model order)"""

    def __init__(self, deck, b=0, batch=1, ov=None):
        n, N = deck.n_nodes, deck.rows
        self.N, self.n_nodes = N, n
        self.E, self.G = np.zeros((N, N)), np.zeros((N, N))
        self.src, self.diodes = [], []
        par = {kind: iter(ov[kind][b, :, 0]) for kind in (ov or {})}
        k = n

        def g4(M, a, c, v):
            for (r, s, sg) in ((a, a, 1), (a, c, -1), (c, a, -1), (c, c, 1)):
                if r > 0 and s > 0:
                    M[r - 1, s - 1] += sg * v

        def inc(a, c, kk):
            for node, sg in ((a, 1.0), (c, -1.0)):
                if node > 0:
                    self.G[node - 1, kk] += sg
                    self.G[kk, node - 1] += sg

        for kind, nodes, p in deck.devices:
            v0 = next(par[kind]) if kind in par else p[0]
            if kind == "R":
                g4(self.G, nodes[0], nodes[1], 1.0 / v0)
            elif kind == "C":
                g4(self.E, nodes[0], nodes[1], v0)
            elif kind == "L":
                inc(nodes[0], nodes[1], k)
                self.E[k, k] -= p[0]
                k += 1
            elif kind in ("VAC", "SQR", "VDC"):
                inc(nodes[0], nodes[1], k)
                self.src.append((k, kind, p))
                k += 1
            elif kind == "KL":
                inc(nodes[0], nodes[1], k)
                inc(nodes[2], nodes[3], k + 1)
                m = p[2] * math.sqrt(p[0] * p[1])
                self.E[k, k] -= p[0]
                self.E[k, k + 1] -= m
                self.E[k + 1, k] -= m
                self.E[k + 1, k + 1] -= p[1]
                k += 2
            elif kind == "D":
                ut = 1.380650524e-23 * (p[4] + 273.15) / 1.6021765314e-19
                self.diodes.append({"a": nodes[0] - 1, "c": nodes[1] - 1, "is": p[0] * p[8], "ute": p[1] * ut, "tt": p[9], "geq": 0.0})
            else:
                raise ValueError(kind)
        assert k == N
        self.restart(np.zeros(N), 0.0)

    def restart(self, x, t):
        self.x, self.t, self.xm, self.hp = np.array(x, dtype=float), float(t), None, 0.0

    def b(self, t):
        out = np.zeros(self.N)
        for k, kind, p in self.src:
            if kind == "VAC":
                out[k] = p[0] * math.sin(p[1] * t + p[2])
            elif kind == "VDC":
                out[k] = p[0]
            else:  # SQR: Vh Vl freq duty phase
                T = 1.0 / p[2]
                out[k] = p[0] if math.fmod(t + p[4] / (2.0 * math.pi) / p[2], T) < p[3] * T else p[1]
        return out

    def vd(self, d, x):
        return (x[d["a"]] if d["a"] >= 0 else 0.0) - (x[d["c"]] if d["c"] >= 0 else 0.0)

    def dc(self, t=0.0):
        """operating point of a linear deck: E out"""
        assert not self.diodes
        self.restart(np.linalg.solve(self.G, self.b(t)), t)
        return self.x

    def peek(self, method, h, fallback=True):
        """the step of size h from the current point under `method`, not taken"""
        a0, a1, a2 = coef(method, h, self.hp, fallback)
        xm = self.xm if self.xm is not None else np.zeros(self.N)
        A = self.G + a0 * self.E
        rhs = self.b(self.t + h) - self.E @ (a1 * self.x + a2 * xm)
        if not self.diodes:
            return np.linalg.solve(A, rhs), []
        cds = [d["tt"] * d["geq"] if d["tt"] > 0.0 and d["geq"] > 0.0 else 0.0 for d in self.diodes]
        x = self.x.copy()
        for it in range(400):
            J, r = A.copy(), A @ x - rhs
            geqs = []
            for d, cd in zip(self.diodes, cds):
                v = self.vd(d, x)
                e = math.exp(min(v / d["ute"], 200.0))
                i = d["is"] * (e - 1.0) + cd * (a0 * v + a1 * self.vd(d, self.x) + a2 * self.vd(d, xm))
                g = d["is"] * e / d["ute"]
                geqs.append(g)
                for node, sg in ((d["a"], 1.0), (d["c"], -1.0)):
                    if node >= 0:
                        r[node] += sg * i
                        for n2, s2 in ((d["a"], 1.0), (d["c"], -1.0)):
                            if n2 >= 0:
                                J[node, n2] += sg * s2 * (g + cd * a0)
            dx = np.linalg.solve(J, -r)
            lim = max(1.0, max(abs(self.vd(d, dx)) for d in self.diodes) / 0.05)  # (damped: no junction moves by more than 50 mV)
            x = x + dx / lim
            if lim == 1.0 and np.max(np.abs(dx)) <= 1e-13 * max(1.0, np.max(np.abs(x))):
                return x, geqs
        raise AssertionError("the restatement's Newton did not converge")

    def step(self, method, h, fallback=True):
        x, geqs = self.peek(method, h, fallback)
        for d, g in zip(self.diodes, geqs):
            d["geq"] = g
        self.xm, self.x, self.t, self.hp = self.x, x, self.t + h, h
        return x


def ref_run(deck, method, hs, batch=1, ov=None):
    """x [len(hs)][batch][rows] of the restatement"""
    out = np.empty((len(hs), batch, deck.rows))
    for b in range(batch):
        r = Ref(deck, b, batch, ov)
        for s, h in enumerate(hs):
            out[s, b] = r.step(method, h)
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. every device kind
def check_devices(name, method, batch, knobs, where):
    deck = DECKS[name]()
    ov = overrides(deck, batch) if batch > 1 else None
    tol = NL if deck.has_nonlinear() else LIN
    # (junctions: cd = tt geq is frozen at the engine's LAST LINEARISATION, one Newton step before the accepted iterate; with the default
    #  Newton tolerance that point is 1e-6 V from the solution and geq moves by 4e-5 of itself -- the engine's Newton is run as far as the
    #  restatement's so that both freeze the same cd)
    tight = dict(v_abstol=1e-12, v_reltol=1e-12, i_abstol=1e-12, i_reltol=1e-12, max_newton=200) if deck.has_nonlinear() else {}
    e = engine(deck, knobs, batch, ov, method, gmin=1e-12 if deck.has_nonlinear() else 0.0, **tight)
    want = ref_run(deck, method, [H] * 12, batch, ov) if not deck.has_nonlinear() else None
    if want is None:  # (the junctions' reference sees the g_min the engine stamps)
        want = np.empty((12, batch, deck.rows))
        for b in range(batch):
            r = Ref(deck, b, batch, ov)
            r.G[np.arange(deck.n_nodes), np.arange(deck.n_nodes)] += 1e-12
            for s in range(12):
                want[s, b] = r.step(method, H)
    worst = 0.0
    for s in range(12):
        e.analyze_tr(H, 1)
        worst = max(worst, max_err(e.solution(), want[s], *tol))
    assert np.all(e.tr_history() == H) and e.tr_method == method
    print(f"INTEG {where} devices {name} method {method} batch {batch}: worst err/tol {worst:.3g}")
    assert worst <= 1.0, worst
    assert np.max(np.abs(want[-1])) > 1e-3, "the case has a signal"
    e.close()


# ---------------------------------------------------------------------------------------------------------------- 2. variable ratios
def pattern(n_triples, T):
    u = T / (3.0 * n_triples)
    return [1.5 * u, 0.75 * u, 0.75 * u] * n_triples


def check_ratios(knobs, where):
    deck = rlc()
    hs = pattern(8, 1e-4)
    e = engine(deck, knobs, 1, None, GEAR2)
    r = Ref(deck)
    worst = 0.0
    for h in hs:
        e.analyze_tr(h, 1)
        worst = max(worst, max_err(e.solution()[0], r.step(GEAR2, h), *LIN))
        assert e.tr_history()[0] == h
    assert worst <= 1.0, worst
    # one step of ratio 3: the BE coefficients, and the restatement alone shows that they are not the GEAR2 ones
    h3 = 3.0 * hs[-1]
    be, _ = r.peek(GEAR2, h3)
    assert same_bits(be, r.peek(BE, h3)[0])
    g2, _ = r.peek(GEAR2, h3, fallback=False)
    gap = max_err(be, g2, *LIN)
    assert gap > 100.0, gap
    e.analyze_tr(h3, 1)
    x = e.solution()[0]
    err_be, err_g2 = max_err(x, be, *LIN), max_err(x, g2, *LIN)
    print(f"INTEG {where} ratios: pattern err/LIN {worst:.3g}; ratio 3: to BE {err_be:.3g}, to GEAR2 {err_g2:.3g} (restatement's gap {gap:.3g})")
    assert err_be <= 1.0 and err_g2 > 100.0 and e.tr_history()[0] == h3
    e.close()


def check_factor_reuse(knobs, where):
    """a linear circuit with refactor_every_solve = 0: what the host reuses is keyed on a0, not on dt -- a GEAR2 step after a restart has
    a0 = 1 / h, the following ones 3 / (2 h) at the same dt, a BE fallback step 1 / h again"""
    deck = rlc()
    h = 2e-6
    for m in (BE, GEAR2):
        e = engine(deck, knobs, 3, None, m, refactor_every_solve=0)
        r = Ref(deck)
        worst = 0.0
        plan = [(h, 4), (h, 3), (2 * h, 2), (h, 1), (3 * h, 2), (h, 3), "reset", (h, 3), (h, 1), "dc", (h, 2)]
        for item in plan:
            if item == "reset":
                e.reset()
                r.restart(np.zeros(deck.rows), 0.0)
                continue
            if item == "dc":
                e.analyze_dc(F.MODE_TROP)
                r.restart(e.solution()[0], e.state()["t"][0])
                continue
            dt, n = item
            e.analyze_tr(dt, n)
            for _ in range(n):
                want = r.step(m, dt)
            for b in range(3):
                worst = max(worst, max_err(e.solution()[b], want, *LIN))
        net = e.safety_net()
        print(f"INTEG {where} factor reuse method {m}: worst err/LIN {worst:.3g}, safety net {net}")
        assert worst <= 1.0, (m, worst)
        # (factors of another a0 are close enough for the residual safety net to repair by refinement: it must not have been needed)
        assert net["refined"] == 0 and net["rematched"] == 0 and not net["careful"], net
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 3. L-stability
def ringing(e_or_ref, method, is_ref):
    """inductor voltage at the ten steps after the edge (steps 3 .. 12), from the operating point"""
    v = []
    for s in range(12):
        x = e_or_ref.step(method, H) if is_ref else (e_or_ref.analyze_tr(H, 1), e_or_ref.solution()[0])[1]
        v.append(x[1])
    return np.array(v[2:])


def check_l_stability(knobs, where):
    deck = rl_edge()
    got = {}
    for m in (TRAP, BE, GEAR2):
        e = engine(deck, knobs, 1, None, m)
        e.analyze_dc(F.MODE_TROP)
        got[m] = ringing(e, m, False)
        e.close()
        if m != TRAP:
            r = Ref(deck)
            r.dc(0.0)
            want = ringing(r, m, True)
            err = np.max(np.abs(got[m] - want) / (LIN[0] * 1e-9 + LIN[1] * np.abs(want)))  # (relative: the values fall through twenty decades)
            assert max_err(got[m], want, *LIN) <= 1.0 and err <= 1.0, (m, got[m], want)
    t, b, g = np.abs(got[TRAP]), np.abs(got[BE]), np.abs(got[GEAR2])
    print(f"INTEG {where} ringing: TRAP |v10/v1| {t[9] / t[0]:.3g}; BE |v6/v1| {b[5] / b[0]:.3g}; GEAR2 |v6/v1| {g[5] / g[0]:.3g}")
    assert np.all(got[TRAP][1:] * got[TRAP][:-1] < 0.0) and t[9] > 0.5 * t[0], got[TRAP]
    assert np.all(np.diff(b) < 0.0), b
    assert b[5] < 1e-4 * b[0] and g[5] < 1e-4 * g[0]


# ---------------------------------------------------------------------------------------------------------------- 4. order
REF_1MS = {}


def ref_value():
    if "v" not in REF_1MS:
        r = Ref(rlc())
        for _ in range(200000):
            r.step(GEAR2, 1e-3 / 200000)
        REF_1MS["v"] = r.x[2]
    return REF_1MS["v"]


def order_ratios(errs):
    return [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]


BRACKET = {BE: (1.9, 2.1), GEAR2: (3.8, 4.2)}
ORDER_CASES = [(BE, False), (GEAR2, False), (GEAR2, True)]


def order_steps(n, pat):
    return pattern(n // 3, 1e-3) if pat else [1e-3 / n] * n


def check_order_restatement():
    """the restatement alone is inside every bracket"""
    deck = rlc()
    for m, pat in ORDER_CASES:
        errs = []
        for n in ((399, 798, 1596) if pat else (400, 800, 1600)):
            r = Ref(deck)
            for h in order_steps(n, pat):
                r.step(m, h)
            errs.append(abs(r.x[2] - ref_value()))
        rr = order_ratios(errs)
        print(f"INTEG restatement order method {m} pattern {pat}: {rr}")
        assert all(BRACKET[m][0] <= q <= BRACKET[m][1] for q in rr), (m, pat, rr)


def check_order(knobs, where):
    deck = rlc()
    for m, pat in ORDER_CASES:
        errs = []
        for n in ((399, 798, 1596) if pat else (400, 800, 1600)):
            e = engine(deck, knobs, 1, None, m)
            if pat:
                for h in order_steps(n, pat):
                    e.analyze_tr(h, 1)
            else:
                e.analyze_tr(1e-3 / n, n)
            errs.append(abs(e.solution()[0][2] - ref_value()))
            e.close()
        rr = order_ratios(errs)
        print(f"INTEG {where} order method {m} pattern {pat}: {rr}")
        assert all(BRACKET[m][0] <= q <= BRACKET[m][1] for q in rr), (m, pat, rr)


# ---------------------------------------------------------------------------------------------------------------- 5. history across launches
def check_launches(knobs, where):
    deck = mixed()
    ov = overrides(deck, 3)
    mk = lambda m: engine(deck, knobs, 3, ov, m, gmin=1e-12)
    sizes = {}
    for m in (TRAP, BE, GEAR2):
        a, b, c = mk(m), mk(m), mk(m)
        a.analyze_tr(H, 12)
        for _ in range(12):
            b.analyze_tr(H, 1)
        assert same_bits(a.solution(), b.solution()), m
        c.analyze_tr(H, 6)
        ck = c.checkpoint()
        sizes[m] = len(ck)
        f = mk(m)
        f.restore(ck)
        assert same_bits(f.tr_history(), c.tr_history())
        f.analyze_tr(H, 6)
        assert same_bits(a.solution(), f.solution()), m
        sa, sf = a.state(), f.state()
        assert all(np.array_equal(sa[k], sf[k]) for k in sa)
        assert ck[:8] == (b"PEHIPCK2" if m == TRAP else b"PEHIPCK3")
        if m == TRAP:
            trap_blob = ck
        else:
            # across methods: refused, engine unchanged and usable
            for other in (TRAP, BE, GEAR2):
                if other == m:
                    continue
                g = mk(other)
                g.analyze_tr(H, 2)
                before = g.solution()
                try:
                    g.restore(ck)
                    raise AssertionError("a checkpoint with history loaded under another method")
                except F.PeHipError as err:
                    assert err.code == F.ERR_ARG and "method" in str(err), str(err)
                assert same_bits(before, g.solution()) and g.tr_method == other
                g.analyze_tr(H, 1)
                g.close()
            # a blob without history is accepted and restarts the history
            g = mk(m)
            g.analyze_tr(H, 3)
            assert np.all(g.tr_history() == H)
            g.restore(trap_blob)
            assert np.all(g.tr_history() == 0.0)
            g.analyze_tr(H, 1)
            g.close()
        for q in (a, b, c, f):
            q.close()
    stride = deck.count("C") + deck.count("L") + 2 * deck.count("KL") + deck.count("D") + 1
    assert sizes[BE] == sizes[GEAR2] == sizes[TRAP] + 8 + 3 * stride * 8, sizes
    print(f"INTEG {where} launches ok, blob sizes {sizes}")


# ---------------------------------------------------------------------------------------------------------------- 6. restart rules
def check_restarts(knobs, where):
    deck = rlc()
    ov = None
    h = 2e-6

    def fresh():
        e = engine(deck, knobs, 2, ov, GEAR2)
        e.analyze_tr(h, 5)
        assert np.all(e.tr_history() == h)
        return e

    trap_blob = {}
    t0 = engine(deck, knobs, 2, ov, TRAP)
    t0.analyze_tr(h, 3)
    trap_blob["ck"] = t0.checkpoint()
    t0.close()
    calls = {
        "load_circuit": lambda e: (e.load_deck(deck, 2, ov), e.set_solution(np.tile([0.3, 0.2, 0.1, 1e-3, -1e-3][:deck.rows], (2, 1)))),
        "reset": lambda e: e.reset(),
        "analyze_dc": lambda e: e.analyze_dc(F.MODE_TROP),
        "analyze_op_stepping": lambda e: e.analyze_op_stepping(F.MODE_TROP),
        "set_solution": lambda e: e.set_solution(0.5 * e.solution()),
        "set_time": lambda e: set_time(e, 3e-5, h),
        "checkpoint_load": lambda e: e.restore(trap_blob["ck"]),
        "method_change": lambda e: (e.set_tr_method(BE), e.set_tr_method(GEAR2)),
    }
    for name, call in calls.items():
        e = fresh()
        call(e)
        assert np.all(e.tr_history() == 0.0), name
        x0, t = e.solution(), e.state()["t"]
        e.analyze_tr(h, 1)
        for b in range(2):
            r = Ref(deck)
            r.restart(x0[b], t[b])
            be = r.peek(BE, h)[0]
            r.xm, r.hp = x0[b] * 0.0, h  # (any second point: a GEAR2 step from here differs)
            assert max_err(e.solution()[b], be, *LIN) <= 1.0, (name, b)
        assert np.all(e.tr_history() == h)
        e.close()
    # analyze_tr does not restart: the next GEAR2 step is the two-step formula, not the BE step
    e = fresh()
    r = Ref(deck)
    for _ in range(5):
        r.step(GEAR2, h)
    be, g2 = r.peek(BE, h)[0], r.peek(GEAR2, h)[0]
    e.analyze_tr(h, 1)
    x = e.solution()[0]
    assert max_err(x, g2, *LIN) <= 1.0 and max_err(x, be, *LIN) > 100.0, (max_err(x, g2, *LIN), max_err(x, be, *LIN))
    e.close()
    print(f"INTEG {where} restarts ok")


# ---------------------------------------------------------------------------------------------------------------- 7. default untouched
def check_default(knobs, where):
    deck = mixed()
    ov = overrides(deck, 3)
    runs = []
    for setting in ("none", "trap", "gear_then_trap"):
        e = engine(deck, knobs, 3, ov, None, gmin=1e-12)
        if setting == "trap":
            e.set_tr_method(TRAP)
        elif setting == "gear_then_trap":
            e.set_tr_method(GEAR2)
            e.set_tr_method(TRAP)
        info = e.info()["bytes_per_instance"]
        e.analyze_tr(H, 12)
        ck = e.checkpoint()
        runs.append((e.solution(), info, ck))
        assert np.all(e.tr_history() == 0.0) and e.tr_method == TRAP
        e.close()
    for x, info, ck in runs[1:]:
        assert same_bits(x, runs[0][0]) and info == runs[0][1] and ck == runs[0][2]
    # AC, noise and sensitivity at a transient operating point do not depend on the method
    out = []
    for m in (TRAP, BE, GEAR2):
        e = engine(deck, knobs, 3, ov, m, gmin=1e-12)
        e.update_param(F.VAC, 0, 2, [0.7] * 3)  # (a phase: the TROP point is not the zero solution)
        e.analyze_dc(F.MODE_TROP)
        ac, _ = e.analyze_ac(2.0 * math.pi * 1e5)
        psd, _, _, _ = e.analyze_noise([1e3, 1e5, 1e7], 3)
        s, _, _, _ = e.analyze_sens([3, 4])
        out.append((ac.real, ac.imag, psd, s))
        e.close()
    for o in out[1:]:
        assert all(same_bits(a, b) for a, b in zip(o, out[0]))
    assert np.max(np.abs(out[0][0])) > 0 and np.all(np.isfinite(out[0][2]))
    print(f"INTEG {where} default ok")


# ---------------------------------------------------------------------------------------------------------------- 8. controller
def samples(e):
    t, v, n, drop = e.probe_samples()
    assert len(set(n.tolist())) == 1 and not drop.any(), (n, drop)
    return t[0, :n[0]].copy(), np.transpose(v[:, :n[0]], (1, 0, 2)).copy()


def q_of(method, tt, xx, h, n_nodes, lte_reltol, lte_abstol_v, lte_abstol_i, trtol):
    """per-instance q of the candidate xx[3] at tt[3] against the three points before it, with the estimate of `method` (include/pe_hip.h)"""
    d10, d21, dn2 = (xx[1] - xx[0]) / (tt[1] - tt[0]), (xx[2] - xx[1]) / (tt[2] - tt[1]), (xx[3] - xx[2]) / (tt[3] - tt[2])
    e0, e1 = (d21 - d10) / (tt[2] - tt[0]), (dn2 - d21) / (tt[3] - tt[1])
    if method == BE:
        dd, scale = e1, h * h
    else:
        dd = (e1 - e0) / (tt[3] - tt[0])
        rho = h / (tt[2] - tt[1])
        scale = h * h * h * ((1.0 + rho) * (1.0 + rho)) / (rho * (1.0 + 2.0 * rho))
    abstol = np.where(np.arange(xx.shape[2]) < n_nodes, lte_abstol_v, lte_abstol_i)
    tol = trtol * (lte_reltol * np.maximum(np.abs(xx[3]), np.abs(xx[2])) + abstol)
    return np.max(scale * np.abs(dd) / tol, axis=1)


def check_decisions(method, e, st, t, x, n_nodes, t0, t_stop, dt_init, dt_min, dt_max, tol, bps=()):
    """every entry of the step log against the rule of include/pe_hip.h, from the recorded accepted points alone (check_decisions of
    tests/test_tr_adaptive_emu.py with the constants and the exponent of `method`)"""
    ex = -0.5 if method == BE else -1.0 / 3.0
    dt, oc = e.tr_step_log()
    assert st["n_accepted"] + st["n_rejected_lte"] + st["n_rejected_newton"] == len(dt) == len(oc)
    assert (oc == 0).sum() == st["n_accepted"] == len(t) - 1 and (oc == 1).sum() == st["n_rejected_lte"] and (oc == 2).sum() == st["n_rejected_newton"]
    bps = sorted([b for b in bps if t0 < b < t_stop]) + [t_stop]
    reached = lambda at, bp: at >= bp or abs(at - bp) <= EPS4 * abs(bp)
    now, a, expect, tested, n_pts, prev_h = t0, 0, dt_init, 0, 0, None
    for k in range(len(dt)):
        bp = next(b for b in bps if not reached(now, b))
        h = dt[k]
        lands = h == bp - now
        assert h <= dt_max * (1 + 1e-12) and (h >= dt_min or lands), (k, h)
        if expect is not None:
            want = min(max(expect, dt_min), dt_max, bp - now)
            assert abs(h - want) <= 1e-9 * want, (k, h, want)
        else:
            assert 0.1 * prev_h * (1 - 1e-9) <= h <= max(0.9 * prev_h, dt_min) * (1 + 1e-9) or lands, (k, h, prev_h)
        if oc[k] == 2:
            expect = h / 8
        elif oc[k] == 1:
            assert n_pts >= 3 and h > dt_min
            expect, prev_h = None, h
        else:
            assert t[a + 1] == now + h
            q = None
            if n_pts >= 3 and tol["lte_reltol"] > 0:
                q = float(np.max(q_of(method, t[a - 2:a + 2], x[a - 2:a + 2], h, n_nodes, **tol)))
                assert q <= 1 + 1e-9 or h <= dt_min, (k, q, h)
                tested += 1
            now, a = t[a + 1], a + 1
            at_bp = bp != t_stop and reached(now, bp)
            n_pts = 1 if at_bp else min(n_pts + 1, 4)
            expect = dt_init if at_bp else (h if q is None else h * (min(2.0, 0.9 * q ** ex) if q > 0 else 2.0))
    assert st["t_end"] == now
    return tested


def replay(make_engine, dt, oc, restart_at=()):
    """checkpoint, analyze_tr(dt_k, 1), restore where the log says rejected -> accepted t [n], x [n][B][rows], engine"""
    e = make_engine()
    ts, xs = [e.state()["t"][0]], [e.solution()]
    for h, o in zip(dt, oc):
        ck = e.checkpoint()
        e.analyze_tr(h, 1, check=False)
        if o:
            e.restore(ck)
        else:
            assert not e.state()["status"].any()
            ts.append(e.state()["t"][0])
            xs.append(e.solution())
    return np.array(ts), np.array(xs), e


def check_controller_pinned(method, knobs, where):
    deck = mixed()
    ov = overrides(deck, 3)
    res = []
    for adaptive in (False, True):
        e = engine(deck, knobs, 3, ov, method, gmin=1e-12)
        if adaptive:
            st = e.analyze_tr_adaptive(1.0, H, dt_min=H, dt_max=H, lte_reltol=-1.0, max_steps=12)
            assert st["n_accepted"] == 12 and st["n_rejected_lte"] == st["n_rejected_newton"] == 0, st
        else:
            e.analyze_tr(H, 12)
        s = e.state()
        res.append((e.solution(), s["t"], s["steps"], s["iters"], e.tr_history()))
        e.close()
    for a, b in zip(*res):
        assert np.array_equal(a, b), (a, b)
    print(f"INTEG {where} pinned controller method {method} ok")


def check_controller_replay(method, knobs, where):
    """a run with LTE and Newton rejections, replayed as fixed-step calls on a fresh engine: every accepted point bit for bit (the history
    array is part of the roll-back snapshot), and every decision re-derived from the recorded samples"""
    deck = D.bridge_rectifier()
    mk = lambda: engine(deck, knobs, 1, None, method, gmin=1e-12, max_newton=5)
    e = mk()
    e.set_probes(list(range(deck.rows)), 8192, 1)
    e.arm_probes()
    T, dt0 = 0.02, 1e-4
    st = e.analyze_tr_adaptive(T, dt0)
    assert st["rc"] == 0 and st["n_rejected_lte"] > 0 and st["n_rejected_newton"] > 0, st
    t, x = samples(e)
    dt, oc = e.tr_step_log()
    tested = check_decisions(method, e, st, t, x, deck.n_nodes, 0.0, T, dt0, dt0 * 1e-9, T / 50, dict(lte_reltol=1e-3, lte_abstol_v=1e-6, lte_abstol_i=1e-9, trtol=7.0))
    assert tested > 50, tested
    tr, xr, f = replay(mk, dt, oc)
    assert np.array_equal(tr, t) and np.array_equal(xr, x), "a rejected step leaves nothing behind"
    assert same_bits(e.tr_history(), f.tr_history())
    e.analyze_tr(1e-5, 5)
    f.analyze_tr(1e-5, 5)
    assert np.array_equal(e.solution(), f.solution())
    print(f"INTEG {where} controller method {method}: accepted {st['n_accepted']} lte {st['n_rejected_lte']} newton {st['n_rejected_newton']} tested {tested}")
    e.close()
    f.close()


def check_controller_breakpoint(knobs, where):
    """after a source breakpoint the first step is a BE step"""
    deck = D.Deck()
    deck.n_nodes = 2
    deck.add("SQR", (1, 0), 1.0, 0.0, 1e5, 0.5, 0.0)   # corner at 5 us
    deck.add("R", (1, 2), 100.0)
    deck.add("C", (2, 0), 1e-8)
    e = engine(deck, knobs, 1, None, GEAR2)
    e.set_probes(list(range(deck.rows)), 4096, 1)
    e.arm_probes()
    st = e.analyze_tr_adaptive(8e-6, 1e-7, source_breakpoints=True)
    assert st["rc"] == 0
    t, x = samples(e)
    k = int(np.argmin(np.abs(t - 5e-6)))
    assert abs(t[k] - 5e-6) <= EPS4 * 5e-6 and k + 2 < len(t) and k >= 3
    r = Ref(deck)
    r.restart(x[k, 0], t[k])
    h = t[k + 1] - t[k]
    be = r.peek(BE, h)[0]
    r.xm, r.hp = x[k - 1, 0], t[k] - t[k - 1]
    g2 = r.peek(GEAR2, h, fallback=False)[0]
    eb, eg = max_err(x[k + 1, 0], be, *LIN), max_err(x[k + 1, 0], g2, *LIN)
    print(f"INTEG {where} breakpoint: first step after the corner to BE {eb:.3g}, to GEAR2 across it {eg:.3g}")
    assert eb <= 1.0 and eg > 100.0
    # ... and the one after it is a two-step formula again
    r.restart(x[k + 1, 0], t[k + 1])
    r.xm, r.hp = x[k, 0], h
    assert max_err(x[k + 2, 0], r.peek(GEAR2, t[k + 2] - t[k + 1])[0], *LIN) <= 1.0
    e.close()


def check_controller_nan(method, knobs, where):
    """a NaN planted in the history array (through a checkpoint blob) is never accepted"""
    deck = c_only()
    e = engine(deck, knobs, 2, None, method)
    e.analyze_tr(H, 4)
    ck = bytearray(e.checkpoint())
    stride = deck.count("C") + 1
    hist = np.frombuffer(bytes(ck[-2 * stride * 8:]), dtype=np.float64).copy()
    assert np.all(hist[[stride - 1, 2 * stride - 1]] == H)
    hist[stride + 1] = np.nan   # second capacitor of instance 1
    ck[-2 * stride * 8:] = hist.tobytes()
    e.restore(bytes(ck))
    x0, t0 = e.solution(), e.state()["t"].copy()
    st = e.analyze_tr_adaptive(t0[0] + 20 * H, H, check=False)
    dt, oc = e.tr_step_log()
    if method == GEAR2:
        assert st["rc"] != 0 and st["n_accepted"] == 0 and len(oc) > 0 and np.all(oc == 2), (st, oc)
        assert same_bits(e.solution(), x0) and np.array_equal(e.state()["t"], t0), "every attempt was rolled back"
    else:
        # (BE reads no second point: a2 = 0 multiplies it -- 0 x NaN is a NaN all the same)
        assert st["rc"] != 0 and st["n_accepted"] == 0 and np.all(oc == 2), (st, oc)
    print(f"INTEG {where} nan method {method}: {len(oc)} attempts, none accepted")
    e.close()


# ---------------------------------------------------------------------------------------------------------------- 9. refusals
def check_refusals(knobs, where):
    import ctypes as C
    deck = rlc()
    e = engine(deck, knobs, 2, None, GEAR2)
    e.analyze_tr(2e-6, 3)
    x, hp = e.solution(), e.tr_history()
    for bad in (-1, 3, 99):
        try:
            e.set_tr_method(bad)
            raise AssertionError("an unknown method was accepted")
        except F.PeHipError as err:
            assert err.code == F.ERR_ARG
        assert e.tr_method == GEAR2 and same_bits(e.tr_history(), hp) and same_bits(e.solution(), x)
    lib = F.lib()
    m = C.c_int(7)
    assert lib.pe_hip_set_tr_method(None, BE) == F.ERR_ARG and lib.pe_hip_get_tr_method(None, C.byref(m)) == F.ERR_ARG and m.value == 7
    assert lib.pe_hip_get_tr_method(e._h, None) == F.ERR_ARG
    buf = np.zeros(2)
    assert lib.pe_hip_get_tr_history(None, 0, 2, F._dp(buf)) == F.ERR_ARG
    assert lib.pe_hip_get_tr_history(e._h, 0, 3, F._dp(buf)) == F.ERR_ARG and lib.pe_hip_get_tr_history(e._h, 0, 2, None) == F.ERR_ARG
    assert lib.pe_hip_sweep_set_tr_method(None, BE) == F.ERR_ARG
    e.analyze_tr(2e-6, 1)   # usable, and the history went on
    assert np.all(e.tr_history() == 2e-6)
    e.close()
    # a setting of the engine: allowed without a circuit, survives the load
    e = F.Engine()
    e.set_tr_method(BE)
    e.load_deck(deck, 1)
    e.reset()
    assert e.tr_method == BE
    e.analyze_tr(2e-6, 2)
    assert e.tr_history()[0] == 2e-6
    e.close()
    check_overlay_refusal(knobs)
    print(f"INTEG {where} refusals ok")


def check_overlay_refusal(knobs):
    """a circuit with a host-stamp overlay integrates in its own hooks: TR under BE / GEAR2 is refused, engine unchanged and usable"""
    import ctypes as C
    deck = D.rc_step()
    CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))

    def cb(user, event, mode, t, dt, x, a, b):
        if event == 1:
            a[0] = 1e-3
            b[0] = 0.0
        return 0

    fn = CB(cb)
    e = F.Engine()
    e.set_options(g_min=0.0)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    lib = F.lib()
    lib.pe_hip_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_int, CB, C.c_void_p]
    rows, cols, rr = np.array([1], dtype=np.int32), np.array([1], dtype=np.int32), np.array([1], dtype=np.int32)
    assert lib.pe_hip_set_overlay(e._h, 1, F._ip(rows), F._ip(cols), None, 1, F._ip(rr), 0, fn, None) == 0
    e.load_deck(deck, 1)
    e.reset()
    e.analyze_tr(1e-8, 2)
    x = e.solution()
    for m in (BE, GEAR2):
        e.set_tr_method(m)
        st = e.analyze_tr(1e-8, 1, check=False)
        assert st["rc"] == F.ERR_ARG and same_bits(e.solution(), x) and e.state()["steps"][0] == 2
    e.set_tr_method(TRAP)
    e.analyze_tr(1e-8, 1)
    assert e.state()["steps"][0] == 3
    e.close()


# ---------------------------------------------------------------------------------------------------------------- 10. sweep twin
def check_sweep(knobs, where):
    deck = mixed()
    ov = overrides(deck, 3)
    for m in (BE, GEAR2):
        e = engine(deck, None, 3, ov, m, gmin=1e-12)
        e.analyze_tr(H, 8)
        s = F.Sweep(1)
        s.set_options(g_min=1e-12)
        s.set_tr_method(m)
        s.load_deck(deck, 3, ov)
        s.reset()
        s.run(H, 8)
        assert same_bits(s.solution(), e.solution()), m
        try:
            s.set_tr_method(5)
            raise AssertionError("an unknown method was accepted")
        except F.PeHipError as err:
            assert err.code == F.ERR_ARG
        s.close()
        e.close()
    print(f"INTEG {where} sweep ok")
