"""Shared by tests/test_param_emu.py and tests/test_gpu_param.py: instance b of a batch reads ITS parameters for every device of every kind
on every path, and pe_hip_update_param changes exactly one (device, column, instance)  ("Per-instance parameters").

The formulas behind the stamps are pinned to mpmath by device_eval_common.py and ac_stamp_common.py; what is checked here is WHICH
parameters reach them.  The bar is therefore bit identity between two routes to the same numbers:
  1. a batch loaded with per-instance tables for every kind and column  ==  one engine of batch 1 per instance, loaded from a plain deck
     that carries that instance's values (the unbatched-table path device_eval_common validates), at the same iterate, DC1 and TR1;
     and the static cells against values stated here from the instance's parameters, the non-linear ones through the references of
     device_eval_common with the instance's parameters -- with a deliberately wrong instance's parameters these must FAIL for every kind;
  2. the small-signal systems of the same batch against ac_stamp_common.ref_stamp of the instance's devices;
  3. a batch loaded at the deck's values and brought to the tables by update_param, column by column  ==  the batch of 1.;
  4. an analysis after update_param  ==  the same analysis on a fresh engine loaded with the new value (nothing stale);
  5. a sweep sharded over two devices  ==  one device  ==  one engine.
The same kernel text runs on the same inputs on both sides of every comparison and the gather order of a cell does not depend on the batch:
any differing bit is a parameter that went to the wrong place.

Spreads.  Instance 0 holds the deck's values; every other value is deck value x (1 + s u), u = uniform01, one u per (kind, device, column,
instance); a deck value of 0 takes a u instead (x the absolute scale of the column).  SPREAD gives s per column.  The spreads of the
non-linear and bias-setting columns are chosen so that the float64 oracle (oracle/pe_oracle.py through OracleEngine, one plain deck per
instance) converges from x = 0 at the operating point for all B = 5 instances: check_reference_converges asserts exactly that on the
CPU.  The BJT junctions and the MOSFET gates stay held by sources / dividers as in ac_stamp_common.mixed_block."""
import numpy as np
import scipy.sparse as sp

import ac_stamp_common as AC
import device_eval_common as DE
from device_eval_common import DT, E, SCHEDULES, Worst  # noqa: F401  (SCHEDULES: re-exported for the two test modules)
from parity_common import instance_deck, instance_devices, pe

F = pe.ffi
Deck = pe.deck.Deck
VGEN_LAYOUT = pe.deck.VGEN_LAYOUT
R_OPEN = AC.R_OPEN
B_MAX = 5

# ---- spreads: s per column (see the module text); "alt": the column alternates 0 / 1 per instance; "keep": the deck's value in every
# instance; (s, a): relative spread s, absolute scale a where the deck's value is 0.  The reference converges from x = 0 at OP for all
# B_MAX instances with these (check_reference_converges).
SPREAD = {
    "R": [0.2], "C": [0.3], "L": [0.3],
    "VDC": [0.02],                                        # bias-setting: the held junctions move by a fraction of N Ut
    "VAC": [0.2, 0.2, (0.3, 1.0)], "IDC": [0.3],
    # Is N Isr Nr Temp Ibv Bv Bv_set Area tt tt_in_tr
    "D": [0.3, 0.05, (0.3, 1e-12), 0.05, 0.5, 0.3, 0.2, "alt", 0.3, 0.5, 0.5],
    "IAC": [0.3, 0.2, (0.3, 1.0)],
    "VCCS": [0.1], "VCVS": [0.1], "CCCS": [0.1], "CCVS": [0.1], "OPAMP": [0.2], "XFMR": [0.1],
    "SW": ["alt"],
    # type Vh Vl freq duty phase tr tf (the type is fixed at load time)
    "VGEN": ["keep", 0.2, (0.2, 0.5), 0.2, 0.2, (0.3, 1.0), (0.5, 1e-6), (0.5, 1e-6)],
    "KL": [0.3, 0.3, 0.1],
    "NMOS": [0.2, 0.3, 0.1], "PMOS": [0.2, 0.3, 0.1],
    # Is N BetaF Temp Area ("temp": 0 .. 60 degrees C)
    "NPN": [0.3, 0.02, 0.2, "temp", 0.2], "PNP": [0.3, 0.02, 0.2, "temp", 0.2],
    # Von Voff ("von": the coil source's voltage x 1.15 / 0.85 in odd / even instances, so the coil sits on either side; Von > Voff)
    "RELAY": ["von", 0.2],
    "XCT": [0.1],
}
RELAY_COIL = 6.0      # the coil sources of mixed_block


# ---- the deck -----------------------------------------------------------------------------------------------------------------------------
def param_block(d):
    """one mixed_block (every kind once, the held-junction structure kept) + two NMOS cells biased like its PMOS cell (divider on the gate,
    drain resistor from the 5 V rail; a source resistor so that no other device lies across D-S) + SQR, PULSE and TRI generators next to
    the SAW and the IAC"""
    base = d.n_nodes
    AC.mixed_block(d, 0)
    n = [0] + [base + i for i in range(1, 32)]
    add = d.add
    for rd, rs, par in ((500.0, 100.0, (2e-3, 0.02, 1.0)), (470.0, 120.0, (1.5e-3, 0.03, 0.9))):
        dn, g, s = d.new_node(), d.new_node(), d.new_node()
        add("R", (n[21], dn), rd)
        add("R", (n[21], g), 1e5)
        add("R", (g, 0), 1e5)
        add("NMOS", (dn, g, s), *par)
        add("R", (s, 0), rs)
        add("C", (g, n[20]), 1e-8)
    for kind, par in (("SQR", (3.0, 0.5, 2e3, 0.3, 1.0)), ("PULSE", (4.0, 0.25, 3e3, 0.5, 0.2, 2e-5, 3e-5)), ("TRI", (2.0, -2.0, 4e3, 2.0))):
        p = d.new_node()
        add(kind, (p, 0), *par)
        add("R", (p, n[20]), 2e3)
    return n


def param_deck():
    """two blocks; between them one R, C, D and NMOS with an unconnected pin (node id -1): from there on the index in the table and the
    index among the resident devices differ.  Under 150 rows."""
    d = Deck()
    n1 = param_block(d)
    d.add("R", (n1[2], -1), 777.0)
    d.add("C", (-1, n1[2]), 3e-8)
    d.add("D", (n1[22], -1), *AC.D_TT)
    d.add("NMOS", (n1[24], -1, n1[21]), 2e-3, 0.02, 1.0)
    param_block(d)
    assert d.rows < 150, d.rows
    return d


def table_name(kind):
    return "VGEN" if kind in VGEN_LAYOUT else kind


def deck_rows(deck):
    """{table name: [[ncol values] per device in deck order]} as ffi.deck_tables lays the tables out, + which (device, column) the deck line
    does not carry (a generator's absent columns; they hold the defaults of deck_tables)"""
    rows, absent = {}, {}
    dflt = (5.0, 0.0, 1e3, 0.5, 0.0, 0.0, 0.0)
    for kind, _, par in deck.devices:
        name = table_name(kind)
        if name == "VGEN":
            ty, pos = VGEN_LAYOUT[kind]
            row = [float(ty)] + [par[q] if q >= 0 else dflt[j] for j, q in enumerate(pos)]
            miss = [0] + [1 + j for j, q in enumerate(pos) if q < 0]
        else:
            row = list(par) + ([1.0] if kind == "D" else [])
            miss = []
        absent.setdefault(name, []).append(miss)
        rows.setdefault(name, []).append(row)
    return rows, absent


def all_overrides(deck, B):
    """a table [B][count][ncol] for EVERY kind of the deck and EVERY column (module text).  Asserted here: outside the columns that
    alternate or are kept, no two instances and no two devices of a kind share a value in any column."""
    rows, absent = deck_rows(deck)
    ov = {}
    for t, name in enumerate(sorted(rows)):
        base = np.array(rows[name], dtype=float)
        cnt, ncol = base.shape
        assert ncol == F.NCOL[name] == len(SPREAD[name]), (name, ncol)
        u = pe.deck.uniform01(1000 + t, B * cnt * ncol).reshape(B, cnt, ncol)
        tab = np.repeat(base[None], B, axis=0)
        for c, s in enumerate(SPREAD[name]):
            for b in range(1, B):
                for j in range(cnt):
                    v0 = base[j, c]
                    if s == "keep" or c in absent[name][j]:
                        v = v0
                    elif s == "alt":
                        v = float((int(v0 != 0.0) + b) % 2)
                    elif s == "temp":
                        v = 60.0 * u[b, j, c]
                    elif s == "von":
                        v = RELAY_COIL * (1.15 if b % 2 else 0.85) * (1.0 + 0.02 * u[b, j, c])
                    else:
                        rel, scale = s if isinstance(s, tuple) else (s, None)
                        v = v0 * (1.0 + rel * u[b, j, c]) if v0 != 0.0 else scale * u[b, j, c]
                    tab[b, j, c] = v
        for c, s in enumerate(SPREAD[name]):
            if s in ("keep", "alt"):
                continue
            vals = [tab[b, j, c] for b in range(B) for j in range(cnt) if c not in absent[name][j]]
            # (devices of one kind may share a DECK value -- the two blocks are copies --: instance 0 is left out of the device comparison)
            per_dev = [tab[b, j, c] for b in range(1, B) for j in range(cnt) if c not in absent[name][j]]
            assert len(set(per_dev)) == len(per_dev), f"{name} column {c}: two devices or instances share a value"
            for j in range(cnt):
                if c not in absent[name][j]:
                    col = [tab[b, j, c] for b in range(B)]
                    assert len(set(col)) == B, f"{name} device {j} column {c}: two instances share a value: {col}"
            assert all(np.isfinite(vals)), (name, c)
        if name == "RELAY":
            assert np.all(tab[:, :, 0] > tab[:, :, 1]), "RELAY: Von <= Voff"
            eng = tab[:, :, 0] <= RELAY_COIL * 0.98      # (the coil source moves by 2 percent at the most)
            off = tab[:, :, 0] >= RELAY_COIL * 1.02
            assert np.all(eng | off) and np.all(eng.any(axis=0) & off.any(axis=0)), "RELAY: the coil is not on either side of Von in some instance"
        ov[name] = tab
    return ov


def check_coverage(deck, ov, B):
    """every kind of ffi's table of column counts, and every column of it, is in a per-instance table whose instances differ there
    (the generator type apart, which is fixed at load time); fails by name"""
    missing = []
    for name, ncol in F.NCOL.items():
        if name not in ov:
            missing.append(f"{name}: no table")
            continue
        tab = np.asarray(ov[name])
        if tab.shape[0] != B or tab.shape[1] != sum(1 for k, _, _ in deck.devices if table_name(k) == name) or tab.shape[2] != ncol:
            missing.append(f"{name}: table of shape {tab.shape}")
            continue
        for c in range(ncol):
            if (name, c) == ("VGEN", 0):
                continue
            if not any(len(set(tab[:, j, c].tolist())) > 1 for j in range(tab.shape[1])):
                missing.append(f"{name} column {c}: the same in every instance")
    assert not missing, "per-instance tables do not cover: " + "; ".join(missing)
    assert set(SPREAD) == set(F.NCOL), sorted(set(SPREAD) ^ set(F.NCOL))


_CASE = {}


def case(B=3):
    """(deck, overrides [B], iterate [B][rows]) -- computed once per process and left unchanged"""
    if B not in _CASE:
        deck = param_deck()
        ov = all_overrides(deck, B)
        check_coverage(deck, ov, B)
        _CASE[B] = (deck, ov, iterate(deck, B))
    return _CASE[B]


def check_reference_converges(oracle_mod, B=B_MAX):
    """the condition the spreads are chosen under: the float64 oracle on every instance's own deck converges from x = 0 at the operating point"""
    deck, ov, _ = case(B)
    o = DE.OracleEngine(oracle_mod, deck, B, ov, 0)
    o.analyze_dc(F.MODE_OP)
    assert not o.status.any(), f"the reference does not converge for instances {np.nonzero(o.status)[0].tolist()}: iterations {o.trace}"
    return o


# ---- the iterate --------------------------------------------------------------------------------------------------------------------------
def checked_nonlinear(deck):
    """[(kind, device index, nodes)] of the first diode, PMOS, NMOS, NPN and PNP of each block (all pins connected)"""
    out, per_kind = [], {}
    for i, (kind, nodes, par) in enumerate(deck.devices):
        if kind in ("D", "PMOS", "NMOS", "NPN", "PNP") and all(q > 0 for q in nodes):
            k = per_kind.get(kind, 0)
            per_kind[kind] = k + 1
            if kind != "NMOS" or k % 2 == 0:      # (two NMOS cells per block: the first of each)
                out.append((kind, i, nodes))
    assert sorted(k for k, _, _ in out) == sorted(["D", "PMOS", "NMOS", "NPN", "PNP"] * 2), out
    return out


def iterate(deck, B):
    """[B][rows]: node voltages from uniform01 inside the ranges device_eval_common uses (MOS_BIAS, BJT_VJ, its diode points: -1 .. 3.5 V),
    branch currents of a few mA; the pins of the checked non-linear devices on biases that conduct, moved a little per instance; the relay
    coils on the coil sources' 6 V (between the Von of the instances)"""
    u = pe.deck.uniform01(99, B * deck.rows).reshape(B, deck.rows)
    x = np.empty((B, deck.rows))
    x[:, :deck.n_nodes] = -1.0 + 4.5 * u[:, :deck.n_nodes]
    x[:, deck.n_nodes:] = 4e-3 * (u[:, deck.n_nodes:] - 0.5)
    for b in range(B):
        for kind, i, n in checked_nonlinear(deck):
            if kind == "D":
                v = (0.9 + 0.02 * b, 0.3)
            elif kind == "PMOS":
                v = (0.5, 0.75 + 0.1 * b, 3.0)
            elif kind == "NMOS":
                v = (2.5, 2.25 + 0.1 * b, 0.25)
            elif kind == "NPN":
                v = (0.85 + 0.01 * b, 2.0, 0.25)
            else:
                v = (1.4 - 0.01 * b, 0.5, 2.0)
            for node, val in zip(n, v):
                x[b, node - 1] = val
        for kind, nodes, par in deck.devices:
            if kind == "RELAY":
                x[b, nodes[0] - 1] = RELAY_COIL
    return x


# ---- engines ------------------------------------------------------------------------------------------------------------------------------
def engine(deck, batch, knobs, overrides=None, max_newton=0, g_min=0.0, residual_tol=-1.0):
    """(residual safety net off in the one-iteration forms: a retry would stamp again)"""
    e = F.Engine()
    e.set_options(g_min=g_min, max_newton=max_newton, residual_tol=residual_tol, r_open=R_OPEN)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    return e


def one_iteration(e, x, form):
    """DC1 / TR1 of device_eval_common: one Newton iteration at the set iterate; TR1 lands on t = DT > 0 (every time source off its zero)"""
    e.reset()
    e.set_solution(x)
    if form == "DC1":
        e.analyze_dc(F.MODE_DC, check=False)
    else:
        e.analyze_tr(DT, 1, check=False)
    DE.statuses_ok(e, form)


def stamps(e):
    return [tuple(np.array(a, copy=True) for a in e.matrix(b)) for b in range(e.batch)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_stamp(got, want, what):
    """bit for bit: pattern, values, right-hand side"""
    rp, ci, va, rhs = got
    wrp, wci, wva, wrhs = want
    assert np.array_equal(rp, wrp) and np.array_equal(ci, wci), f"{what}: patterns differ"
    bad = np.nonzero(bits(va) != bits(wva))[0]
    if len(bad):
        rows = np.searchsorted(rp, bad, side="right") - 1
        cells = [(int(r), int(ci[s])) for r, s in zip(rows[:5], bad[:5])]
        raise AssertionError(f"{what}: {len(bad)} matrix values differ, first at cells {cells}: {va[bad[:5]]} against {wva[bad[:5]]}")
    bad = np.nonzero(bits(rhs) != bits(wrhs))[0]
    assert len(bad) == 0, f"{what}: right-hand side rows {bad[:5]} differ: {rhs[bad[:5]]} against {wrhs[bad[:5]]}"


def differing(got, want):
    """(cells, right-hand-side rows) where two stamps of one pattern differ"""
    rp, ci, va, rhs = got
    bad = np.nonzero(bits(va) != bits(want[2]))[0]
    rows = np.searchsorted(rp, bad, side="right") - 1
    return {(int(r), int(ci[s])) for r, s in zip(rows, bad)}, set(np.nonzero(bits(rhs) != bits(want[3]))[0].tolist())


FORMS = ("DC1", "TR1")
_BATCH_STAMPS = {}


def batch_stamps(knobs, B=3):
    """{form: stamps of every instance} of engine A: batch B loaded with all_overrides (computed once per schedule and process)"""
    key = (tuple(sorted((knobs or {}).items())), B)
    if key not in _BATCH_STAMPS:
        deck, ov, x = case(B)
        e = engine(deck, B, knobs, ov, max_newton=1)
        out = {}
        for form in FORMS:
            one_iteration(e, x, form)
            out[form] = stamps(e)
        e.close()
        _BATCH_STAMPS[key] = out
    return _BATCH_STAMPS[key]


# ---- 1. load-time tables --------------------------------------------------------------------------------------------------------------------
def check_load_bitwise(knobs, label=""):
    """matrix(b) of the batch == matrix(0) of a batch-1 engine loaded from instance b's plain deck, DC1 and TR1"""
    deck, ov, x = case(3)
    A = batch_stamps(knobs)
    for b in range(3):
        e = engine(instance_deck(deck, ov, b), 1, knobs, None, max_newton=1)
        for form in FORMS:
            one_iteration(e, x[b], form)
            same_stamp(A[form][b], stamps(e)[0], f"{label} {form}, instance {b} of the batch against its own deck")
        e.close()
    # the instances do differ: a batch that gave every instance the same table would pass the loop above only through E_b
    for form in FORMS:
        cells, rows = differing(A[form][0], A[form][1])
        assert len(cells) > 50 and len(rows) > 10, (form, len(cells), len(rows))


STATIC_KINDS = ("R", "VDC", "IDC", "VCCS", "VCVS", "CCCS", "CCVS", "OPAMP", "XFMR", "XCT", "SW", "RELAY")
NL_KINDS = ("D", "PMOS", "NMOS", "NPN", "PNP")
ENGINE_KINDS = ("C", "L", "KL", "VAC", "IAC", "VGEN")      # companion and time-source stamps: the independent statement is instance b's own deck


def relay_engaged(devs, xb):
    """relay.h: engaged from released when the coil voltage reaches Von (the state after reset is released)"""
    return {i: (xb[n[0] - 1] - (xb[n[1] - 1] if n[1] else 0.0)) >= par[0] for i, (kind, n, par) in enumerate(devs) if kind == "RELAY"}


def connected(devs):
    """ref_stamp's view: devices with an unconnected pin stamp nothing (none of them has a branch row)"""
    out = []
    for kind, nodes, par in devs:
        if any(q < 0 for q in nodes):
            assert pe.deck.NBRANCH[kind] == 0
            continue
        out.append((kind, nodes, par))
    return out


def check_static_cells(stamp, deck, devs, xb, W, what, only=None):
    """the DC1 stamp of one instance: every matrix cell that holds ONE contribution, of a static kind, bitwise against the value stated
    from devs' parameters (ac_stamp_common.ref_stamp at omega = 0 restates exactly those: an input or one rounded operation; in DC a
    capacitor stamps nothing and an inductor is a short, as there); the right-hand side of every VDC row and of every node that carries an
    IDC alone.  only: restrict to cells / rows of that kind.  Returns the number of values compared per kind."""
    rp, ci, va, rhs = stamp
    got = AC.cells_of(rp, ci, va)
    devs = connected(devs)
    N = deck.n_nodes
    eng = relay_engaged(devs, xb)
    nl = {}
    for i, (kind, n, par) in enumerate(devs):
        nl[i] = {"D": (1.0,), "NMOS": (1.0, 1.0), "PMOS": (1.0, 1.0), "NPN": (1.0, 1.0), "PNP": (1.0, 1.0), "RELAY": (eng.get(i, False),)}.get(kind)
    owner = {}      # cell -> kinds of the devices that contribute to its real part
    kb = N
    counts = {}
    for i, dev in enumerate(devs):
        kind = dev[0]
        # one device at a time: which cells it writes.  kb - N stand-in drives put its branch rows where the deck has them
        S1 = AC.ref_stamp([dev], N, [(1, 0.0)] * (kb - N), 0.0, 0.0, R_OPEN, {0: nl[i]}, set())
        for (r, c), (re_l, im_l) in S1.A.items():
            if N <= r < kb or N <= c < kb:
                continue      # (cells of the stand-in rows)
            if re_l or (r, c) in S1.was_set:
                owner.setdefault((r, c), []).append((kind, re_l))
        kb += pe.deck.NBRANCH[kind]
    for (r, c), lst in owner.items():
        if len(lst) != 1 or lst[0][0] not in STATIC_KINDS or (only and lst[0][0] != only):
            continue
        kind, re_l = lst[0]
        if len(re_l) != 1:
            continue
        W.check(kind, got.get((r, c), 0.0), re_l[0], f"{what}, cell ({r}, {c})", 0)
        counts[kind] = counts.get(kind, 0) + 1
    # right-hand side: VDC rows hold V; a node with one IDC and no other source of right-hand side in DC holds -+I (IDC.h:84-95)
    kb = N
    rhs_users = {}
    for kind, n, par in devs:
        for r in ([q - 1 for q in n] if kind in ("IDC", "IAC", "D", "NMOS", "PMOS", "NPN", "PNP") else []):
            rhs_users.setdefault(r, []).append(kind)
    for kind, n, par in devs:
        if kind == "VDC" and only in (None, "VDC"):
            W.check("VDC", rhs[kb], E(par[0]), f"{what}, right-hand side row {kb}", 0)
            counts["VDC"] = counts.get("VDC", 0) + 1
        if kind == "IDC" and only in (None, "IDC"):
            for q, sign in ((n[0], -1.0), (n[1], 1.0)):
                if q > 0 and rhs_users[q - 1] == ["IDC"]:
                    W.check("IDC", rhs[q - 1], E(sign * par[0]), f"{what}, right-hand side row {q - 1}", 0)
                    counts["IDC"] = counts.get("IDC", 0) + 1
        kb += pe.deck.NBRANCH[kind]
    return counts


def check_nl_cells(stamp_dc, stamp_tr, deck, devs, xb, W, what, only=None):
    """the cells that hold one non-linear device alone (off the diagonal: (a, c) of a diode, (S, D) and (D, G) of a MOSFET, (B, E) and (C, B)
    of a BJT -- no other device lies across those pins) through DiodeRef / ref_mos / ref_bjt with devs' parameters, at their bounds"""
    for form, stamp in (("DC1", stamp_dc), ("TR1", stamp_tr)):
        rp, ci, va, rhs = stamp
        A = sp.csr_matrix((va, ci, rp), shape=(len(rp) - 1,) * 2)
        for kind, i, n in checked_nonlinear(deck):
            if only and kind != only:
                continue
            par = devs[i][2]
            v = [xb[q - 1] for q in n]
            w = f"{what} {form}, {kind} (device {i})"
            if kind == "D":
                ref = DE.DiodeRef(DE.diode_prepared(par))
                vd = v[0] - v[1]
                if form == "TR1":
                    ref.companion(vd, DT)
                g, ie, bg, bi = ref.eval(vd, form == "TR1", W.arms)
                W.check("diode geq", -DE.cell(A, n[0], n[1]), E(0, g), w, bg)
            elif kind in ("NMOS", "PMOS"):
                gds, gm, ieq = DE.ref_mos(kind == "NMOS", v[0], v[1], v[2], *par, W.arms)
                assert gm.d != 0.0 and gds.d != 0.0, f"{w}: the bias does not conduct"
                W.check(f"{kind} gds", -DE.cell(A, n[2], n[0]), gds, w)
                W.check(f"{kind} gm", DE.cell(A, n[0], n[1]) * (1.0 if kind == "NMOS" else -1.0), gm, w)
            else:
                geq, i1, gm, i2 = DE.ref_bjt(kind == "NPN", v[0], v[2], *DE.bjt_prepared(par), W.arms)
                W.check(f"{kind} geq", -DE.cell(A, n[0], n[2]), geq, w)
                W.check(f"{kind} gm", DE.cell(A, n[1], n[0]), gm, w)


def swapped(deck, ov, b, B, name):
    """instance b's devices with the parameters of table `name` taken from instance (b + 1) % B: the deliberately wrong reference"""
    wrong = dict(ov)
    wrong[name] = np.roll(np.asarray(ov[name]), -1, axis=0)
    assert wrong[name].shape[0] == B
    return wrong


def check_load_references(knobs, label="", wrong=False):
    """the stamps of the batch, per instance, against the independent statements (check_static_cells, check_nl_cells); wrong: then with one
    kind's parameters taken from the next instance -- the statement must FAIL, for every kind (ENGINE_KINDS: through that kind's stamps of
    a batch-1 engine loaded with the wrong values)"""
    deck, ov, x = case(3)
    A = batch_stamps(knobs)
    W = Worst()
    total = {}
    for b in range(3):
        devs = instance_devices(deck, ov, b)
        for k, v in check_static_cells(A["DC1"][b], deck, devs, x[b], W, f"{label} instance {b}").items():
            total[k] = total.get(k, 0) + v
        check_nl_cells(A["DC1"][b], A["TR1"][b], deck, devs, x[b], W, f"{label} instance {b}")
    lacking = [k for k in STATIC_KINDS if total.get(k, 0) < 3 * 2]
    assert not lacking, f"static kinds without a cell of their own in every instance and block: {lacking} ({total})"
    W.report(f"per-instance parameters, load-time tables {label}")
    if not wrong:
        return W
    caught = {}
    kinds = {table_name(k) for k, _, _ in deck.devices}
    assert kinds == set(F.NCOL), sorted(kinds ^ set(F.NCOL))
    for name in sorted(kinds):
        caught[name] = 0
        for b in range(3):
            bad = swapped(deck, ov, b, 3, name)
            devs = instance_devices(deck, bad, b)
            try:
                if name in STATIC_KINDS:
                    check_static_cells(A["DC1"][b], deck, devs, x[b], Worst(), "wrong reference", only=name)
                elif name in NL_KINDS:
                    check_nl_cells(A["DC1"][b], A["TR1"][b], deck, devs, x[b], Worst(), "wrong reference", only=name)
                else:
                    assert name in ENGINE_KINDS, name
                    e = engine(instance_deck(deck, bad, b), 1, knobs, None, max_newton=1)
                    try:
                        one_iteration(e, x[b], "TR1")
                        same_stamp(A["TR1"][b], stamps(e)[0], "wrong reference")
                    finally:
                        e.close()
            except AssertionError:
                caught[name] += 1
    # SW alternates 0 / 1 and the relays are engaged in the even instances: instance 2 stamps what instance 0's values give, the swap is
    # invisible there
    missed = [k for k, v in caught.items() if v < (2 if k in ("SW", "RELAY") else 3)]
    assert not missed, f"a reference with the next instance's parameters passes for {missed}: {caught}"
    print(f"WRONG REFERENCE {label}: failures per kind (of 3 instances) {caught}")
    return W


# ---- 3. update_param == a fresh load ---------------------------------------------------------------------------------------------------------
def loaded_stamps(deck, B, knobs, table, x):
    e = engine(deck, B, knobs, table, max_newton=1)
    out = {}
    for form in FORMS:
        one_iteration(e, x, form)
        out[form] = stamps(e)
    e.close()
    return out


def current_stamps(e, x):
    out = {}
    for form in FORMS:
        one_iteration(e, x, form)
        out[form] = stamps(e)
    return out


def same_stamps(got, want, what):
    for form in FORMS:
        for b, (g, w) in enumerate(zip(got[form], want[form])):
            same_stamp(g, w, f"{what}, {form}, instance {b}")


def update_pass(e, now, target, scalar_of, first_scalar):
    """one update_param call per (kind, index in the table, column) that brings the engine from the table `now` to `target`, alternating
    the scalar form (instance scalar_of's value for all) and the batched form from call to call.  Returns the table the engine then holds
    and the set of (name, j, c) that took the scalar form."""
    held = {k: np.array(v, copy=True) for k, v in now.items()}
    scalar, call = set(), 0 if first_scalar else 1
    for name in sorted(target):
        tab = np.asarray(target[name])
        for j in range(tab.shape[1]):
            for c in range(tab.shape[2]):
                if (name, c) == ("VGEN", 0):
                    continue
                if call % 2 == 0:
                    e.update_param(F.KIND_CODE[name], j, c, float(tab[scalar_of, j, c]))
                    held[name][:, j, c] = tab[scalar_of, j, c]
                    scalar.add((name, j, c))
                else:
                    e.update_param(F.KIND_CODE[name], j, c, tab[:, j, c])
                    held[name][:, j, c] = tab[:, j, c]
                call += 1
    return held, scalar


def check_update_equals_load(knobs, label=""):
    """engine U: batch 3 loaded from the plain deck, brought to all_overrides by update_param.  Pass 1 alternates scalar / batched calls,
    pass 2 alternates the other way round (so every column has taken both forms), pass 3 gives the batched form to what pass 2 left scalar:
    after each pass the stamps equal those of an engine LOADED with the table the calls describe; after pass 3 that is engine A of case 1.
    Then the host mirror: diode Temp then Is, BJT Area then Temp, one raw column per call -- equal to a load with both changed (the raw
    columns are kept, not re-derived from stale ones)."""
    B = 3
    deck, ov, x = case(B)
    A = batch_stamps(knobs)
    rows, _ = deck_rows(deck)
    plain = {k: np.repeat(np.array(v, dtype=float)[None], B, axis=0) for k, v in rows.items()}
    U = engine(deck, B, knobs, None, max_newton=1)
    same_stamps(current_stamps(U, x), loaded_stamps(deck, B, knobs, plain, x), f"{label} batched load of the deck's own values")
    held, s1 = update_pass(U, plain, ov, 1, True)
    same_stamps(current_stamps(U, x), loaded_stamps(deck, B, knobs, held, x), f"{label} pass 1")
    held, s2 = update_pass(U, held, ov, 2, False)
    assert not s1 & s2 and len(s1 | s2) == sum(np.asarray(t).shape[1] * np.asarray(t).shape[2] for t in ov.values()) - len(ov["VGEN"][0])
    same_stamps(current_stamps(U, x), loaded_stamps(deck, B, knobs, held, x), f"{label} pass 2")
    for name, j, c in sorted(s2):
        U.update_param(F.KIND_CODE[name], j, c, np.asarray(ov[name])[:, j, c])
    same_stamps(current_stamps(U, x), A, f"{label} pass 3 against the batch loaded with the tables")
    # -- the host mirror keeps the raw columns
    both = {k: np.array(v, copy=True) for k, v in ov.items()}
    for name, cols in (("D", (4, 0)), ("NPN", (4, 3)), ("PNP", (4, 3))):
        tab = both[name]
        for c in cols:
            for j in range(tab.shape[1]):
                u = pe.deck.uniform01(500 + 10 * c + j, B)
                tab[:, j, c] = tab[:, j, c] * (1.0 + 0.1 * u) + (5.0 * u if name != "D" and c == 3 else 0.0)
                U.update_param(F.KIND_CODE[name], j, c, tab[:, j, c])
    same_stamps(current_stamps(U, x), loaded_stamps(deck, B, knobs, both, x), f"{label} two raw columns of a derived kind, one call each")
    U.close()


VISIBLE_LAST = ("R", "C", "L", "VDC", "VAC", "IDC", "IAC", "VCCS", "VCVS", "CCCS", "CCVS", "OPAMP", "XFMR", "SW", "KL", "NMOS", "PMOS", "NPN", "PNP", "XCT")


def device_rows(deck, name, j):
    """rows (= columns) of the j-th device of table `name`: its pins and its branches; None when it has an unconnected pin"""
    kb, seen = deck.n_nodes, 0
    for kind, nodes, par in deck.devices:
        nb = pe.deck.NBRANCH[kind]
        if table_name(kind) == name:
            if seen == j:
                if any(q < 0 for q in nodes):
                    return None
                return {q - 1 for q in nodes if q > 0} | set(range(kb, kb + nb))
            seen += 1
        kb += nb
    raise AssertionError((name, j))


def check_update_locality(knobs, label=""):
    """one call per kind -- the last device of the table, its last column, the batched form with instance 1 alone changed --: only cells
    and right-hand-side rows of that device in that instance change; refusals and the unconnected device change nothing"""
    B = 3
    deck, ov, x = case(B)
    U = engine(deck, B, knobs, ov, max_newton=1)
    before = current_stamps(U, x)
    changed_kinds = set()
    for name in sorted(ov):
        tab = np.asarray(ov[name])
        j, c = tab.shape[1] - (2 if name == "NMOS" else 1), tab.shape[2] - 1      # (NMOS: the first cell of the block, whose iterate conducts)
        col = tab[:, j, c].copy()
        col[1] = float(col[1] == 0.0) if SPREAD[name][c] == "alt" else col[1] * 1.0625 + (0.25 if col[1] == 0.0 else 0.0)
        U.update_param(F.KIND_CODE[name], j, c, col)
        after = current_stamps(U, x)
        own = device_rows(deck, name, j)
        assert own is not None
        for form in FORMS:
            for b in range(B):
                cells, rows = differing(after[form][b], before[form][b])
                if b != 1:
                    assert not cells and not rows, f"{label} {name} {form}: a change of instance 1 moved instance {b}: cells {sorted(cells)[:5]}, rows {sorted(rows)[:5]}"
                    continue
                stray = {q for q in cells if q[0] not in own or q[1] not in own}
                assert not stray and rows <= own, f"{label} {name} {form}: cells {sorted(stray)[:5]} / rows {sorted(rows - own)[:5]} are not of device {j} (rows {sorted(own)})"
                if cells or rows:
                    changed_kinds.add(name)
        before = after
    assert set(VISIBLE_LAST) <= changed_kinds, f"{label}: the change does not show for {sorted(set(VISIBLE_LAST) - changed_kinds)}"
    # -- refusals: PE_HIP_ERR_ARG, nothing moves
    counts = {name: np.asarray(t).shape[1] for name, t in ov.items()}
    refused = [(F.KIND_CODE[name], 0, F.NCOL[name]) for name in ov] + [(F.KIND_CODE[name], counts[name], 0) for name in ov]
    refused += [(F.VGEN, 0, 0), (0, 0, 0), (99, 0, 0), (F.R, -1, 0), (F.R, 0, -1)]
    for kind, j, c in refused:
        for val in (1.25, np.full(B, 1.25)):
            try:
                U.update_param(kind, j, c, val)
            except F.PeHipError as ex:
                assert ex.code == F.ERR_ARG, (kind, j, c, ex)
            else:
                raise AssertionError(f"{label}: update_param(kind {kind}, index {j}, column {c}) was accepted")
    same_stamps(current_stamps(U, x), before, f"{label} after the refused calls")
    # -- the unconnected devices: accepted, nothing resident changes; the index after them is the next connected device
    for name in ("R", "C", "D", "NMOS"):
        j = next(k for k in range(counts[name]) if device_rows(deck, name, k) is None)
        for c in range(F.NCOL[name]):
            U.update_param(F.KIND_CODE[name], j, c, np.asarray(ov[name])[:, j, c] * 1.5 + 0.125)
    same_stamps(current_stamps(U, x), before, f"{label} after update_param on the unconnected devices")
    j = next(k for k in range(counts["R"]) if device_rows(deck, "R", k) is None) + 1
    col = np.asarray(ov["R"])[:, j, 0] * 2.0
    U.update_param(F.R, j, 0, col)
    after = current_stamps(U, x)
    own = device_rows(deck, "R", j)
    a, b_ = sorted(own) if len(own) == 2 else (min(own), min(own))
    for b in range(B):
        cells, rows = differing(after["DC1"][b], before["DC1"][b])
        assert cells and all(q[0] in own and q[1] in own for q in cells) and not rows, f"{label}: R index {j} (after the unconnected one) moved cells {sorted(cells)[:6]}"
        got = AC.cells_of(*after["DC1"][b][:3])
        if a != b_:
            assert got[(a, b_)] == -(1.0 / col[b]), (got[(a, b_)], col[b])
    U.close()


# ---- 5. shards -------------------------------------------------------------------------------------------------------------------------------
def check_shards(label=""):
    """batch 5 over two devices (shards [0, 3) and [3, 5) read every multi-column table from an offset) == one device == one engine"""
    B = 5
    deck, ov, _ = case(B)
    out = {}
    for mask in (3, 1):
        s = F.Sweep(mask)
        s.set_options(g_min=0.0)
        s.load_deck(deck, B, ov)
        if mask == 3:
            assert [(f, c) for _, f, c in s.shards()] == [(0, 3), (3, 2)], s.shards()
        s.reset()
        s.operating_point(F.MODE_TROP)      # (no instance of this deck, the deck's own values included, takes a first transient step from x = 0)
        st = s.run(DT, 3)
        assert st["n_failed"] == 0, st
        out[mask] = s.solution()
        s.close()
    e = F.Engine()
    e.set_options(g_min=0.0)
    e.load_deck(deck, B, ov)
    e.reset()
    e.analyze_dc(F.MODE_TROP)
    e.analyze_tr(DT, 3)
    x = e.solution()
    e.close()
    for b in range(B):
        assert np.array_equal(bits(out[3][b]), bits(out[1][b])), f"{label} instance {b}: two shards against one: {np.nonzero(out[3][b] != out[1][b])[0][:5]}"
        assert np.array_equal(bits(out[1][b]), bits(x[b])), f"{label} instance {b}: the sweep against one engine"
    assert len({out[1][b].tobytes() for b in range(B)}) == B, "two instances have the same solution"


# ---- 6. the column counts ------------------------------------------------------------------------------------------------------------------
PIN_DT = 2.0 ** -20


def count_case(name):
    """a deck with ONE device of table `name` (pins on nodes that carry a resistor to ground and a current source each) and a table
    [2][1][ncol] whose second instance differs in the LAST column only, by a change that shows in three transient steps after the operating point"""
    d = Deck()
    npin = {"VGEN": 2}.get(name) or pe.deck.NPINS[name]
    p = [d.new_node() for _ in range(max(npin, 4))]
    for i, node in enumerate(p):
        d.add("R", (node, 0), 1e3 * (i + 1))
        d.add("IDC", (0, node), 1e-3 * (i + 1))      # 1, 4, 9, 16 V on the free pins
    d.add("IAC", (0, p[0]), 2e-4, 2e5, 0.3)          # ... which move from step to step, so that C, L and k show
    T = 8.0 * PIN_DT
    kind, nodes, par, last = {
        "D": ("D", (p[0], 0), AC.D_TT, 0.0),                                              # tt_in_tr: the diffusion companion from step 2 on
        "NMOS": ("NMOS", (p[2], p[1], p[0]), (2e-4, 0.02, 1.0), 1.25), "PMOS": ("PMOS", (p[0], p[1], p[2]), (2e-4, 0.02, 0.5), 0.625),
        "NPN": ("NPN", (p[1], p[2], p[0]), (1e-15, 1.0, 150.0, 27.0, 1.0), 1.5), "PNP": ("PNP", (p[0], p[2], p[1]), (1e-15, 1.0, 150.0, 27.0, 1.0), 1.5),
        # coil on a pulse: 6 V at t = DT (engages), 3.5 V from 2 DT on: Voff = 3 stays engaged, Voff = 4 releases
        "RELAY": ("RELAY", (p[0], p[1], p[2], p[3]), (5.0, 3.0), 4.0),
        # tf: at t = 3 DT the pulse (Ton = 4 DT) is on its falling edge when tf is 2 DT, still high when it is DT / 2
        "VGEN": ("PULSE", (p[0], p[1]), (5.0, 0.0, 1.0 / T, 0.5, 0.0, 0.0, 2.0 * PIN_DT), 0.5 * PIN_DT),
        "SW": ("SW", (p[0], p[1]), (0.0,), 1.0),
        "VAC": ("VAC", (p[0], p[1]), (2.0, 1e5, 0.3), 0.9), "IAC": ("IAC", (p[0], p[1]), (1e-3, 1e5, 0.3), 0.9),
        "KL": ("KL", tuple(p[:4]), (1e-3, 4e-3, 0.8), 0.5),
    }.get(name, (name, tuple(p[:npin]), tuple(1.5 * v for v in pe.deck.DEFAULTS.get(name, (1.0,))), None))
    if name in ("NPN", "PNP"):
        d.add("VDC", (p[1], p[0]), 0.6)      # the junction held (the BJT models have no junction limiting)
    if name == "PMOS":
        d.add("VDC", (p[2], 0), 5.0)         # the source on a rail one volt above the gate (a free source node does not converge, in the reference either)
    if name == "RELAY":
        d.add("PULSE", (p[0], p[1]), 6.0, 3.5, 1.0 / T, 0.25, 0.0, 0.0, 0.0)
    d.add(kind, nodes, *par)
    rows, _ = deck_rows(d)
    row = rows[name][-1]
    tab = np.array([[row], [row]], dtype=float)
    tab[1, 0, -1] = last if last is not None else 2.0 * row[-1]
    assert tab.shape == (2, 1, F.NCOL[name]) and tab[1, 0, -1] != tab[0, 0, -1]      # (one device per kind: [2][1][ncol])
    if tab.shape[2] > 1:
        assert np.array_equal(tab[0, 0, :-1], tab[1, 0, :-1])
    if name in ("R", "IDC", "IAC", "VDC"):      # (the pin resistors, the pin sources and the junction source are devices of these tables too)
        full = np.repeat(np.array(rows[name], dtype=float)[None], 2, axis=0)
        full[1, -1] = tab[1, 0]
        tab = full
    return d, {name: tab}


def check_column_counts(two_devices):
    """ffi.NCOL against the library's three copies: per kind, batch 2 on the one-device deck of count_case.  Instance 1 of the batch ==
    the same batch loaded from the plain deck with the last column set by update_param, instance 0 == its plain deck, bit for bit (a loader or gen_ncol count that differs from ffi's puts instance 1's row at
    another offset), the last column's change shows, and with two_devices a sweep over two devices, one instance each, gives the same
    (param_columns slices the table for the second shard)."""
    for name in F.NCOL:
        deck, ov = count_case(name)
        sol = []
        # (the third: the same batch from the plain deck, the last column put there by update_param -- which writes by the engine's own
        #  layout, not by a table's stride; the same instance 0, so the same pivot order and the same rounding)
        for d_, b_, o_ in ((deck, 2, ov), (instance_deck(deck, ov, 0), 1, None), (deck, 2, None)):
            e = F.Engine()
            e.set_options(g_min=0.0, r_open=R_OPEN)
            e.load_deck(d_, b_, o_)
            if b_ == 2 and o_ is None:
                tab = np.asarray(ov[name])
                e.update_param(F.KIND_CODE[name], tab.shape[1] - 1, tab.shape[2] - 1, tab[:, -1, -1])
            e.reset()
            e.analyze_dc(F.MODE_TROP)
            e.analyze_tr(PIN_DT, 3)
            sol.append(e.solution())
            e.close()
        assert np.array_equal(bits(sol[0][0]), bits(sol[1][0])), f"{name}: instance 0 of the batch against its own deck"
        assert np.array_equal(bits(sol[0]), bits(sol[2])), f"{name}: the batch loaded with the table against the batch brought there by update_param: {np.nonzero(sol[0] != sol[2])}"
        assert not np.array_equal(sol[0][0], sol[0][1]), f"{name}: the change of the last column does not show in the solution"
        if two_devices:
            s = F.Sweep(3)
            s.set_options(g_min=0.0)
            s.load_deck(deck, 2, ov)
            assert [(f, c) for _, f, c in s.shards()] == [(0, 1), (1, 1)], s.shards()
            s.reset()
            s.operating_point(F.MODE_TROP)
            s.run(PIN_DT, 3)
            xs = s.solution()
            s.close()
            assert np.array_equal(bits(xs), bits(sol[0])), f"{name}: two shards of one instance each against one engine: {np.nonzero(xs != sol[0])}"


def check_short_table_refused():
    """a [B][n][10] diode table (the deck's ten values without tt_in_tr) is refused in Python, as is any other last dimension"""
    deck, ov, _ = case(3)
    for name in F.NCOL:
        for ncol in (F.NCOL[name] - 1, F.NCOL[name] + 1):
            bad = dict(ov)
            good = np.asarray(ov[name])
            bad[name] = np.zeros(good.shape[:2] + (ncol,))
            try:
                F.deck_tables(deck, 3, bad)
            except ValueError as ex:
                assert name in str(ex), ex
            else:
                raise AssertionError(f"deck_tables accepted a {name} table with {ncol} columns")
    F.deck_tables(deck, 3, ov)


# ---- 2. load-time tables, AC side ------------------------------------------------------------------------------------------------------------
AC_OMEGAS = [0.0, 2.0e4]
AC_SWEEPS = [[2.0e4, 0.0, 3.0e3],         # bands {0} and {3e3, 2e4}: with P = 2 the pass of omega = 0 is partly unused, the last pass full
             [2.0e4, 3.0e3, 2.5e4]]       # one band: the last pass is [2.5e4, unused]
# the two-node output pair of ac_stamp_common.check_adjoint (nothing drives it at DC: its sensitivities are all 0), and the first NPN's
# collector against the first PMOS's drain
OUTPUTS = [(5, 13), (26, 23)]


def connected_deck(deck):
    """the deck without its devices with an unconnected pin (they stamp nothing and have no branch: every row keeps its number)"""
    out = Deck()
    out.n_nodes = deck.n_nodes
    out.devices = connected(deck.devices)
    assert out.rows == deck.rows
    return out


def selector(n2, pos, neg):
    want = np.zeros(n2)
    want[pos] = 1.0
    if neg >= 0:
        want[neg] = -1.0
    return want


def check_adjoint_system(W, e, which, q, fwd, S, out, what):
    """matrix_ac(which, q): the exact transpose of the forward system `fwd` (as read at that omega), the reference's transpose within its
    bounds, the right-hand side the selector of `out` alone (ac_stamp_common.check_adjoint)"""
    rp, ci, va, rhs = e.matrix_ac(which, q)
    frp, fci, fva, _ = fwd
    T = sp.csr_matrix(sp.csr_matrix((fva, fci, frp), shape=(len(frp) - 1,) * 2).T)
    T.sort_indices()
    assert np.array_equal(T.indptr, rp) and np.array_equal(T.indices, ci), f"{what}: pattern is not the transposed pattern"
    bad = np.nonzero(bits(T.data) != bits(va))[0]
    assert len(bad) == 0, f"{what}: slots {bad[:5]} hold {va[bad[:5]]}, the forward matrix transposed {T.data[bad[:5]]}"
    AC.check_system(W, "adjoint", AC.cells_of(rp, ci, va), None, S, what, transposed=True)
    want = selector(len(rp) - 1, *out)
    assert np.array_equal(bits(rhs), bits(want)), f"{what}: right-hand side {rhs[np.nonzero(rhs != want)[0][:5]]} is not the selector"


def check_ac(knobs, label=""):
    """the deck and tables of case 1 at the operating point: the systems of analyze_ac, of the last pass of analyze_ac_sweep (instance
    q = b P + p), of the adjoint engines of analyze_noise and analyze_sens, against ref_stamp of INSTANCE b's devices, cell by cell at
    the bounds of ac_stamp_common"""
    B = 3
    deck, ov, _ = case(B)
    cdeck = connected_deck(deck)
    W = Worst()
    e = AC.ac_engine(deck, B, knobs, ov, AC.GMIN)
    st = e.analyze_dc(F.MODE_OP, check=False)
    assert all(s == 0 for s in e.state()["status"]), f"{label}: operating point {st} {e.state()['status']}"
    devs = [connected(instance_devices(deck, ov, b)) for b in range(B)]
    nl = [AC.nl_values(e, cdeck, b) for b in range(B)]
    engaged = [sorted(v[0] for i, v in nl[b].items() if cdeck.devices[i][0] == "RELAY") for b in range(B)]
    assert engaged[0] == [True, True] and engaged[1] == [False, False], f"{label}: relay states {engaged}"      # the coil on either side of Von
    ref = lambda b, w: AC.ref_stamp(devs[b], deck.n_nodes, [], w, AC.GMIN, R_OPEN, nl[b], W.arms)
    single = {}
    for w in AC_OMEGAS + [3.0e3, 2.5e4, 3.0e4]:
        x, rc = e.analyze_ac(w, check=False)
        assert rc == 0, f"{label}: analyze_ac({w}) returned {rc}"
        for b in range(B):
            rp, ci, va, rhs = e.matrix_ac(0, b)
            if w in AC_OMEGAS:
                AC.check_system(W, "single point", AC.cells_of(rp, ci, va), rhs, ref(b, w), f"{label} instance {b}, omega {w}")
            single[w, b] = (rp.copy(), ci.copy(), va.copy(), rhs.copy())
    e.set_knob("AC_SWEEP_POINTS", 2)      # (a knob drops the main engine's symbolic analysis, not its operating point)
    for ws in AC_SWEEPS:
        x, status, stats = e.analyze_ac_sweep(ws, check=False)
        assert stats["rc"] == 0 and not status.any(), f"{label}: sweep {stats} {status}"
        P = e.ac_pass_size(1)
        assert P == 2, P
        passes = AC.pass_layout(ws, P)
        assert stats["n_passes"] == len(passes) and any(len(set(p)) < P for p in passes), (stats, passes)
        for b in range(B):
            for p, w in enumerate(passes[-1]):
                q = b * P + p
                rp, ci, va, rhs = e.matrix_ac(1, q)
                AC.check_system(W, "sweep", AC.cells_of(rp, ci, va), rhs, ref(b, w), f"{label} sweep {ws}, instance {q} = ({b}, {p}), omega {w}")
                srp, sci, sva, srhs = single[w, b]
                assert np.array_equal(ci, sci) and np.array_equal(bits(va), bits(sva)) and np.array_equal(bits(rhs), bits(srhs)), \
                    f"{label} sweep {ws}: instance {q} is not bit-identical to the single-point system of instance {b} at omega {w}"
    # -- the adjoint engines: noise at two frequencies of one band (P = 2), sens with two outputs (P = 2) at omega = 0
    omegas = [3.0e4, 2.0e4]
    psd, _, status, stats = e.analyze_noise(omegas, *OUTPUTS[0], check=False)
    assert stats["rc"] == 0 and not status.any(), (stats, status)
    P = e.ac_pass_size(3)
    assert P == 2, P
    last = AC.pass_layout(omegas, P)[-1]
    for b in range(B):
        for p, w in enumerate(last):
            check_adjoint_system(W, e, 3, b * P + p, single[w, b], ref(b, w), OUTPUTS[0], f"{label} noise adjoint, instance ({b}, {p}), omega {w}")
    s, _, status, stats = e.analyze_sens([o[0] for o in OUTPUTS], [o[1] for o in OUTPUTS], check=False)
    assert stats["rc"] == 0 and not status.any() and stats["outputs_per_pass"] == 2, (stats, status)
    for b in range(B):
        for p, out in enumerate(OUTPUTS):
            check_adjoint_system(W, e, 4, b * 2 + p, single[0.0, b], ref(b, 0.0), out, f"{label} sens adjoint, instance ({b}, output {p})")
    # the sensitivities read instance b's parameters: two instances never share a row of them
    assert np.all(np.isfinite(s)) and np.count_nonzero(s[1, 0]) > 10, s[1, 0]
    assert len({s[1, b].tobytes() for b in range(B)}) == B, "two instances have the same sensitivities"
    e.close()
    W.need(["omega = 0", "SW: open", "SW: closed", "RELAY: engaged", "RELAY: not engaged", "D: j omega tt geq"], "per-instance AC")
    W.report(f"per-instance parameters, AC side {label}")
    return W


# ---- 4. nothing stale after update_param ---------------------------------------------------------------------------------------------------
# (table, index in the table, column): one parameter per kind group whose change shows in the results below.  Indices are those of the
# first block (see param_block / mixed_block for the order of the devices of a kind).
STALE_GROUPS = [("R", 22, 0), ("C", 0, 0), ("L", 0, 0), ("KL", 0, 2), ("VDC", 3, 0), ("IDC", 0, 0), ("VAC", 0, 0), ("IAC", 0, 0), ("VGEN", 3, 1),
                ("D", 0, 0), ("NMOS", 0, 2), ("NPN", 0, 2), ("SW", 1, 0), ("RELAY", 0, 0), ("VCVS", 0, 0)]
STALE_DT = 2.0 ** -17
STALE_OMEGAS = [2.0e4, 3.0e3, 2.5e4]
STALE_PORTS = [(1, -1), (5, 13)]


def stale_value(ov, name, j, c):
    """the new column: instance 0 keeps its value (the static pivot order of a batch is matched on instance 0: the engine that takes the
    change and the engine loaded with it then factor in the same order, and bit identity is a fair demand), the others move.  SW: the
    second switch of the block is open in instance 0 and closed in instance 1 -- instance 2 closes too.  RELAY: instance 1's Von falls
    below the coil voltage, its contact closes (an engaged relay would stay engaged above Voff whatever Von becomes)."""
    col = np.array(np.asarray(ov[name])[:, j, c], copy=True)
    if name == "SW":
        assert col[0] == 0.0 and col[1] == 1.0 and col[2] == 0.0, col
        col[2] = 1.0
    elif name == "RELAY":
        assert col[1] > RELAY_COIL, col
        col[1] = RELAY_COIL * 0.9
    else:
        col[1:] = col[1:] * 1.125 + (0.125 if name == "VAC" else 0.0)
    return col


def _tr(e):
    st = e.analyze_tr(STALE_DT, 4, check=False)
    return [np.array([st["rc"], st["newton_iters"], st["steps"]])]


def _op(e):
    st = e.analyze_dc(F.MODE_OP, check=False)
    return [np.array([st["rc"], st["newton_iters"]])]


def _ac(e):
    x, rc = e.analyze_ac(2.0e4, check=False)
    return [np.array([rc]), x.real, x.imag]


def _ac_sweep(e):
    x, status, stats = e.analyze_ac_sweep(STALE_OMEGAS, check=False)
    return [np.array([stats["rc"], stats["n_fallback_points"]]), status, x.real, x.imag]


def _noise(e):
    out = []
    for pair in OUTPUTS[::-1]:      # (the bias part of the deck and the chain the VAC drives meet only on nodes that sources hold: one output in each)
        psd, contrib, status, stats = e.analyze_noise(STALE_OMEGAS, *pair, contributions=True, check=False)
        out += [np.array([stats["rc"]]), status, psd, contrib]
    return out


def _sens(e):
    s, _, status, stats = e.analyze_sens([o[0] for o in OUTPUTS], [o[1] for o in OUTPUTS], check=False)
    return [np.array([stats["rc"]]), status, s]


def _net(e):
    Z, Y, S, ys, ss, status, stats = e.analyze_net(STALE_OMEGAS, STALE_PORTS, check=False)
    return [np.array([stats["rc"], stats["n_factorisations"]]), status, ys, ss, Z.real, Z.imag, Y.real, Y.imag, S.real, S.imag]


def _pz(e):
    status, stats = e.analyze_pz(2.0e4, what=F.PZ_BOTH, n_wanted=2, max_krylov=16, ports=((1, -1), OUTPUTS[0]), check=False)
    out = [np.array([stats["rc"], stats["n_steps"]]), status]
    for which in (F.PZ_POLES, F.PZ_ZEROS):
        s, err, nf, nc, cp = e.pz(which, 16)
        out += [s.real, s.imag, err, nf, nc, cp]
    return out


def _dc_sweep(e):
    # the 5 V rail of the first block (TRACE: a relay's state depends on history, the parallel order is refused on this deck)
    x, status, stats = e.analyze_dc_sweep([4.9, 5.1, 5.0], F.VDC, 1, order=F.DC_SWEEP_TRACE, check=False)
    return [np.array([stats["rc"], stats["newton_iters"], stats["n_failed"]]), status, x] + list(e.dc_sweep_status())


def _dc_sweep_parallel(e):
    x, status, stats = e.analyze_dc_sweep([4.9, 5.1, 5.0], F.VDC, 1, order=F.DC_SWEEP_PARALLEL, check=False)
    assert stats["rc"] != 0 or stats["points_per_pass"] > 1, stats      # instance q = b P + p of the sweep engine carries b's values
    return [np.array([stats["rc"], stats["newton_iters"], stats["n_failed"]]), status, x] + list(e.dc_sweep_status())


def without_relays(deck, ov):
    """the parallel order of the DC sweep refuses a deck with a relay (its state depends on history): the same deck and tables without them"""
    d = Deck()
    d.n_nodes = deck.n_nodes
    d.devices = [dev for dev in deck.devices if dev[0] != "RELAY"]
    return d, {k: v for k, v in ov.items() if k != "RELAY"}


# analysis -> (the call, whether the operating point is taken again before it -- the small-signal analyses read its linearisation)
STALE_ANALYSES = {"tr": (_tr, False), "ac": (_ac, True), "ac_sweep": (_ac_sweep, True), "noise": (_noise, True), "sens": (_sens, True),
                  "net": (_net, True), "pz": (_pz, True), "dc_sweep": (_dc_sweep, True), "dc_sweep_parallel": (_dc_sweep_parallel, True)}


# What a change cannot show in -- neither in the analysis nor in the operating point taken before it --, by the physics of the deck: C, L,
# the coupling and the AC sources stamp nothing at DC, and the chain the VAC drives (switches, relay contact, VCVS) carries no DC signal at all, so the DC
# analyses see none of them; noise, network parameters and poles do not depend on the AC sources.  Everywhere else the change must show
# against an engine loaded with the table before the change (what a stale value would give).
_AC_SRC, _NO_DC = {"VAC", "IAC"}, {"C", "L", "KL", "VAC", "IAC", "SW", "RELAY", "VCVS"}
STALE_INVISIBLE = {"tr": set(), "ac": set(), "ac_sweep": set(), "noise": _AC_SRC, "net": _AC_SRC, "pz": _AC_SRC,
                   "sens": _NO_DC, "dc_sweep": _NO_DC, "dc_sweep_parallel": _NO_DC}


def full_state(e):
    st = e.state()
    return [e.solution(), st["status"], st["iters"], st["steps"], st["t"]]


def same_results(a, b, what):
    assert len(a) == len(b), what
    for k, (p, q) in enumerate(zip(a, b)):
        if p is None or q is None:
            assert p is None and q is None, what
            continue
        p, q = np.asarray(p), np.asarray(q)
        assert p.shape == q.shape and p.dtype == q.dtype, f"{what}: result {k}: {p.shape} {p.dtype} against {q.shape} {q.dtype}"
        same = np.array_equal(p.view(np.int64), q.view(np.int64)) if p.dtype == np.float64 else np.array_equal(p, q)
        if not same:
            bad = np.argwhere(p != q)[:4]
            raise AssertionError(f"{what}: result {k} differs at {bad.tolist()}: {p[tuple(bad.T)]} against {q[tuple(bad.T)]}")


def stale_engine(deck, B, knobs, table):
    e = F.Engine()
    e.set_options(g_min=AC.GMIN, r_open=R_OPEN)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.set_knob("AC_SWEEP_POINTS", 2)
    e.load_deck(deck, B, table)
    e.reset()
    return e


def check_nothing_stale(knobs, analysis, label=""):
    """the analysis twice on one engine with a parameter changed in between, for every group of STALE_GROUPS in turn (the engine keeps the
    earlier changes): the second call's results, and the engine's solution, statuses, iteration and step counts after it, are those of a
    fresh engine loaded with the changed table and brought to the same state by restore(checkpoint()), bit for bit -- and not those of
    a fresh engine loaded with the table before the change, wherever the analysis can see the parameter (STALE_INVISIBLE)."""
    call, with_op = STALE_ANALYSES[analysis]
    B = 3
    deck, ov, _ = case(B)
    if analysis == "dc_sweep_parallel":
        deck, ov = without_relays(deck, ov)
    table = {k: np.array(v, copy=True) for k, v in ov.items()}
    e = stale_engine(deck, B, knobs, table)
    st = e.analyze_dc(F.MODE_TROP if analysis == "tr" else F.MODE_OP, check=False)
    assert st["rc"] == 0, st

    def run(eng):
        pre = _op(eng) if with_op else []
        return pre + call(eng) + full_state(eng)

    odd = []
    first = run(e)
    assert first[0][0] == 0 and first[1 if with_op else 0][0] == 0, f"{label} {analysis}: the first call failed: {first[0]} {first[1]}"
    for name, j, c in STALE_GROUPS:
        if name not in table:
            continue
        blob = e.checkpoint()
        col = stale_value(table, name, j, c)
        assert not np.array_equal(col, table[name][:, j, c])
        old = {k: np.array(v, copy=True) for k, v in table.items()}
        table[name][:, j, c] = col
        e.update_param(F.KIND_CODE[name], j, c, col)
        got = run(e)
        want = []
        for tab in (table, old):      # (the engine loaded with the table before the change: what a stale value would give)
            f = stale_engine(deck, B, knobs, tab)
            f.restore(blob)
            want.append(run(f))
            f.close()
        assert want[0][0][0] == 0, f"{label} {analysis} after update_param({name}, {j}, {c}): {want[0][0]}"
        same_results(got, want[0], f"{label} {analysis} after update_param({name}, {j}, {c})")
        shows = any(not np.array_equal(np.asarray(p), np.asarray(q), equal_nan=True) for p, q in zip(*want) if p is not None)
        if shows != (name not in STALE_INVISIBLE[analysis]):
            odd.append((name, j, c, shows))
    e.close()
    assert not odd, f"{label} {analysis}: (table, index, column, shows) against STALE_INVISIBLE: {odd}"


def check_nothing_stale_mesh(label=""):
    """the same at batch 5 on the 56 x 56 diode mesh of static_skip_common -- the smallest circuit where the lane-group kernel and its static
    fronts exist --: analyze_tr(dt, 4) twice at one dt with an R, a C and a D changed in between (the factors of the static fronts, kept
    across the Newton iterations of a point, and the static part stamped once per dt must not outlive the change)"""
    import static_skip_common as SK
    deck, ov = SK.case(True)
    B = SK.BATCH
    rows, _ = deck_rows(deck)
    table = {"R": np.array(ov["R"], copy=True), "C": np.array(ov["C"], copy=True), "D": np.repeat(np.array(rows["D"], dtype=float)[None], B, axis=0)}

    def fresh():
        e = F.Engine()
        e.set_options(g_min=0.0)
        e.set_knob("GEOMETRY_BATCH", 1024)
        e.set_knob("STATIC_SKIP", 1)
        e.load_deck(deck, B, table)
        e.reset()
        return e

    def run(eng):
        st = eng.analyze_tr(SK.DT, 4, check=False)
        return [np.array([st["rc"], st["newton_iters"], st["steps"]])] + full_state(eng)

    e = fresh()
    first = run(e)
    assert first[0][0] == 0 and e.static_skip_stats()["skipped_launches"] > 0, (first[0], e.static_skip_stats())
    nR, nC, nD = (table[k].shape[1] for k in ("R", "C", "D"))
    for name, j, c, factor in (("R", nR // 2, 0, 0.5), ("C", nC // 3, 0, 3.0), ("D", nD // 2, 0, 50.0), ("R", nR - 1, 0, 2.0)):
        blob = e.checkpoint()
        col = table[name][:, j, c].copy()
        col[1:] *= factor      # (instance 0 keeps its value: the pivot order of both engines is matched on it)
        table[name][:, j, c] = col
        e.update_param(F.KIND_CODE[name], j, c, col)
        got = run(e)
        f = fresh()
        f.restore(blob)
        want = run(f)
        f.close()
        same_results(got, want, f"{label} mesh after update_param({name}, {j}, {c})")
        assert not np.array_equal(got[1][1:], first[1][1:])
        first = got
    assert e.static_skip_stats()["skipped_launches"] > 0
    e.close()
