"""Shared bodies of the tests of the stepped operating point (pe_hip_analyze_op_stepping / pe_hip_get_op_step_state / pe_hip_get_op_step_log,
include/pe_hip.h): tests/test_op_step_emu.py runs them on the host emulation, one child process per case, tests/test_gpu_op_step.py on the
device -- there the 256-thread workgroup of k_op_step_control, its ballot and its strided copies are what is added.

The reference is never the engine under test: restate() is the controller of the header in plain Python doubles (+, *, min, comparisons),
driving one fresh Oracle (oracle/pe_oracle.py, unchanged) per level -- x, the junction state, the relay contacts and the three-pin devices'
state are carried, the VDC / IDC values of a copy of the deck are scaled by one rounded multiply, g_min is passed per level.  A level is
accepted when the oracle converges within the Newton cap to a finite solution.  Tolerance: the project's NL through max_err."""
import copy

import numpy as np

from dc_sweep_common import NL, diode_chain, engine, oracle_mod
from newton_common import CellDeck
from parity_common import MODES, golden, max_err, pe

F = pe.ffi
GMIN, SOURCE, AUTO = F.STEP_GMIN, F.STEP_SOURCE, F.STEP_AUTO
DEFAULTS = dict(dl_init=0.125, grow=2.0, shrink=0.25, dl_min=2.0 ** -20, g_start=1e-2, max_levels=200)
MODE_NAME = {v: k for k, v in MODES.items()}
GOLDENS = ["bjt_npn_ce_dc_fail", "bjt_pnp_ce_op_fail", "bjt_amp_trop_fail"]


# ---------------------------------------------------------------------------------------------------------------- the oracle, one level
def scaled(deck, lam):
    """a copy of the deck whose independent static sources hold lam * value (one rounded multiply)"""
    d = copy.deepcopy(deck)
    for i, (k, n, p) in enumerate(d.devices):
        if k in ("VDC", "IDC"):
            d.devices[i] = (k, n, (float(lam * p[0]),) + tuple(p[1:]))
    return d


def state_of(o):
    s = {"x": o.x.copy(), "relay": list(o.relay_engaged), "n3": copy.deepcopy(o.n3_state)}
    if o.dio is not None:
        s["dio"] = (o.dio.Ud_last.copy(), o.dio.geq.copy(), o.dio.Ieq.copy())
    return s


def oracle_level(deck, mode, g_min, state, cap):
    """one fresh Oracle at one level, from the zero state or from a copy of `state`; -> (oracle, iterations, accepted)"""
    o = oracle_mod().Oracle(deck, g_min=g_min)
    o.prepare()
    if state is not None:
        o.x = state["x"].copy()
        o.relay_engaged = list(state["relay"])
        o.n3_state = copy.deepcopy(state["n3"])
        if o.dio is not None:
            o.dio.Ud_last, o.dio.geq, o.dio.Ieq = (a.copy() for a in state["dio"])
    with np.errstate(all="ignore"):
        it = o.solve(mode)
    return o, it, bool(0 < it <= cap and np.all(np.isfinite(o.x)))


class Outcome:
    pass


def restate(deck, mode, method, g_min=0.0, cap_direct=64, cap_step=None, logged_values=None, **ctl):
    """the whole call on the oracle: -> Outcome with solved_in (0 direct, 1 gmin, 2 source, -1 failed), x (solved: the solution; failed: the
    last accepted level of the last phase, zeros if none), lam, levels, rejected, log [(phase, lambda, value, accepted, iterations)].
    logged_values: the values an engine logged -- the gmin levels then run at exactly those (they come from a libm call there), after they
    have been compared with the restated g_start * (g_end / g_start)^lambda to a relative 1e-14."""
    c = dict(DEFAULTS, **{k: v for k, v in ctl.items() if v > 0})
    cap_step = cap_direct if cap_step is None else cap_step
    mode = MODE_NAME.get(mode, mode)
    out = Outcome()
    out.log, out.levels, out.rejected = [], 0, 0
    o, it, ok = oracle_level(deck, mode, g_min, None, cap_direct)
    out.direct_iters = it
    if ok:
        out.solved_in, out.x, out.lam = 0, o.x, 1.0
        return out
    g_end = max(g_min, 1e-13)
    rows = len(o.x)
    for ph in ([GMIN] if method == GMIN else [SOURCE] if method == SOURCE else [GMIN, SOURCE]):
        state = shadow = None
        lam, delta, t, first = 0.0, c["dl_init"], 0.0, True
        while True:
            if ph == GMIN:
                val = c["g_start"] * (g_end / c["g_start"]) ** t if t < 1.0 else g_min
                if logged_values is not None and len(out.log) < len(logged_values):
                    got = float(logged_values[len(out.log)])
                    assert abs(got - val) <= 1e-14 * abs(val), f"level {len(out.log)}: logged gmin {got!r}, restated {val!r}"
                    val = got
                dk, g = deck, val
            else:
                val, dk, g = t, scaled(deck, t), g_min
            o, it, ok = oracle_level(dk, mode, g, state, cap_step)
            out.levels += 1
            out.log.append((ph, t, val, ok, it if ok else 0))
            failed = False
            if ok:
                shadow = state = state_of(o)
                lam = t
                if first:
                    first = False
                else:
                    delta = delta * c["grow"]
                if t >= 1.0:
                    out.solved_in, out.x, out.lam = ph, o.x, 1.0
                    return out
            else:
                out.rejected += 1
                if first:
                    failed = True
                else:
                    delta = delta * c["shrink"]
                    failed = delta < c["dl_min"]
                    state = shadow
            if out.levels >= c["max_levels"] or (failed and not (ph == GMIN and method == AUTO)):
                out.solved_in, out.lam = -1, lam
                out.x = shadow["x"] if shadow is not None else np.zeros(rows)
                return out
            if failed:
                break
            t = min(1.0, lam + delta)
    raise AssertionError("unreachable")


def instance_deck(deck, volts):
    """the deck of one instance of a batch whose VDC table is `volts` [nVdc]"""
    d = copy.deepcopy(deck)
    j = 0
    for i, (k, n, p) in enumerate(d.devices):
        if k == "VDC":
            d.devices[i] = (k, n, (float(volts[j]),) + tuple(p[1:]))
            j += 1
    return d


# ---------------------------------------------------------------------------------------------------------------- comparisons
def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


def compare_log(e, b, ref, what):
    """the device's log of instance b against the restated run: lambda bit for bit, values (gmin: relative 1e-14, checked inside restate;
    source: lambda itself), outcomes, Newton counts of the accepted levels; the per-instance state beside it"""
    lg = e.op_step_log(b)
    assert lg["n_total"] == len(ref.log) == len(lg["lambda"]), (what, lg["n_total"], len(ref.log))
    for i, (ph, t, val, ok, it) in enumerate(ref.log):
        assert lg["phase"][i] == ph, (what, i, lg["phase"][i], ph)
        assert same_bits(lg["lambda"][i], t), (what, i, float(lg["lambda"][i]).hex(), float(t).hex())
        if ph == SOURCE:
            assert same_bits(lg["value"][i], t), (what, i)
        else:
            assert abs(lg["value"][i] - val) <= 1e-14 * abs(val), (what, i, lg["value"][i], val)
        assert bool(lg["outcome"][i]) == ok, f"{what}: level {i} (phase {ph}, lambda {t}) outcome {lg['outcome'][i]}, oracle {ok}"
        if ok:
            assert lg["iters"][i] == it, f"{what}: level {i} took {lg['iters'][i]} iterations, the oracle {it}"
    s = e.op_step_state()
    assert s["phase_solved_in"][b] == ref.solved_in and s["levels"][b] == ref.levels and s["rejected"][b] == ref.rejected, (what, {k: v[b] for k, v in s.items()}, ref.solved_in, ref.levels, ref.rejected)
    assert same_bits(s["lambda_reached"][b], ref.lam), (what, s["lambda_reached"][b], ref.lam)


def restate_like(e, b, deck, mode, method, g_min, cap_direct, cap_step, **ctl):
    """restate() at the gmin values instance b of the engine logged"""
    lg = e.op_step_log(b)
    return restate(deck, mode, method, g_min, cap_direct, cap_step, logged_values=[v for p, v in zip(lg["phase"], lg["value"]) if p == GMIN] if method != SOURCE else None, **ctl)


# ================================================================================================================ the cases
def check_golden(name, knobs, label=""):
    """1 + 2. a golden that pe_hip_analyze_dc fails on: still fails there; GMIN, SOURCE and AUTO solve it; log and solution against the
    restated oracle run; a following pe_hip_analyze_dc from that state converges and stays within NL"""
    meta, _, deck = golden(name)
    mode = MODES[meta["analysis"]]
    for method in (GMIN, SOURCE, AUTO):
        e = engine(deck, knobs=knobs, g_min=meta["gmin"], r_open=meta.get("r_open", 0.0))
        assert e.analyze_dc(mode, check=False)["rc"] in (F.ERR_NO_CONVERGENCE, F.ERR_SINGULAR), "the direct solve must keep failing"
        e.reset()
        st = e.analyze_op_stepping(mode, method, log_capacity=64)
        ref = restate_like(e, 0, deck, mode, method, meta["gmin"], 64, 64)
        assert ref.solved_in == (SOURCE if method == SOURCE else GMIN), ref.solved_in
        compare_log(e, 0, ref, f"{label} {name} method {method}")
        x = e.solution()[0]
        err = max_err(x, ref.x, *NL)
        print(f"OPSTEP {label} {name} method {method}: levels {st['n_levels']} rejected {st['n_rejected']} iters {st['newton_iters']} err/NL {err:.3g}")
        assert err <= 1.0, err
        assert st["n_failed"] == 0 and st["n_direct"] == 0 and st["n_levels"] == ref.levels and st["n_rejected"] == ref.rejected, st
        assert st["n_solves"] == ref.levels + 1 and st["n_launches"] == ref.levels + 2, st
        assert e.state()["status"][0] == 0
        assert e.analyze_dc(mode, check=False)["rc"] == 0
        assert max_err(e.solution()[0], ref.x, *NL) <= 1.0
        e.close()
    if "ce_" in name:
        assert abs(abs(ref.x[1]) - 0.692889) < 1e-6, ref.x[1]


CHAIN_V = [0.5, 2.0, 5.0, 10.0]


def chain_engine(knobs, volts, cap=6):
    d = diode_chain(1)
    return d, engine(d, batch=len(volts), overrides={"VDC": np.asarray(volts, dtype=float)[:, None, None]}, knobs=knobs, g_min=0.0, max_newton=cap)


def check_mixed(knobs, label=""):
    """3. diode_chain(1) at 0.5 / 2 / 5 / 10 V, Newton cap 6, AUTO: every outcome in one batch"""
    refs = [restate(instance_deck(diode_chain(1), [v]), "OP", AUTO, 0.0, 6, 6) for v in CHAIN_V]
    # the condition on the inputs, on the oracle alone
    assert refs[0].solved_in == 0
    assert any(r.solved_in == GMIN and r.rejected > 0 for r in refs)
    assert any(r.solved_in == SOURCE and any(p == GMIN for p, *_ in r.log) for r in refs)
    d, e = chain_engine(knobs, CHAIN_V)
    st = e.analyze_op_stepping(F.MODE_OP, AUTO, step_max_newton=6, log_capacity=64)
    x = e.solution()
    s = e.op_step_state()
    print(f"OPSTEP {label} mixed: solved_in {s['phase_solved_in'].tolist()} levels {s['levels'].tolist()} rejected {s['rejected'].tolist()} stats {st}")
    for b, v in enumerate(CHAIN_V):
        ref = restate_like(e, b, instance_deck(d, [v]), "OP", AUTO, 0.0, 6, 6)
        compare_log(e, b, ref, f"{label} mixed instance {b}")
        assert max_err(x[b], ref.x, *NL) <= 1.0, b
    assert st["n_direct"] == 1 and st["n_failed"] == 0 and st["n_gmin"] + st["n_source"] == 3 and st["n_source"] >= 1, st
    assert st["n_levels"] == sum(r.levels for r in refs) and st["n_rejected"] == sum(r.rejected for r in refs), st
    assert st["n_solves"] == 1 + max(r.levels for r in refs), st
    assert not e.state()["status"].any()
    # the directly converged instance: what pe_hip_analyze_dc leaves, bit for bit
    _, e1 = chain_engine(knobs, CHAIN_V)
    e1.analyze_dc(F.MODE_OP, check=False)
    assert same_bits(e1.solution()[0], x[0])
    e1.close()
    # every stepped instance: its own batch-1 run of the same call, bit for bit
    for b in range(1, 4):
        _, eb = chain_engine(knobs, CHAIN_V[b:b + 1])
        eb.analyze_op_stepping(F.MODE_OP, AUTO, step_max_newton=6, log_capacity=64)
        assert same_bits(eb.solution()[0], x[b]), f"instance {b} differs from its batch-1 run"
        # (a finished instance is parked: the later levels of the others add nothing to its counters)
        assert eb.state()["iters"][0] == e.state()["iters"][b], (b, eb.state()["iters"], e.state()["iters"])
        eb.close()
    e.close()


def check_wrap(knobs, n=258, B=3, label=""):
    """4. loops that wrap: n cells (sources, diodes and rows beyond the 256-thread team), drive levels permuted over the instances, a Newton
    cap that forces stepping; every instance equals its batch-1 run bit for bit and the oracle under NL"""
    cd = CellDeck(n)
    levels = np.array([0.4, 3.0, 7.0])
    volts = np.array([[levels[(i + b) % 3] for i in range(n)] for b in range(B)])
    cap = 6
    ctl = dict(step_max_newton=cap, log_capacity=64)
    e = engine(cd.deck, batch=B, overrides=cd.overrides(volts), knobs=knobs, g_min=0.0, max_newton=cap)
    st = e.analyze_op_stepping(F.MODE_OP, AUTO, check=False, **ctl)
    x = e.solution()
    s = e.op_step_state()
    assert st["rc"] == 0 and st["n_direct"] == 0 and st["n_failed"] == 0, st
    print(f"OPSTEP {label} wrap n {n} B {B}: levels {st['n_levels']} rejected {st['n_rejected']} solves {st['n_solves']} gpu_ms {st['gpu_ms']:.2f}")
    refs = {}
    for b in sorted(set(range(min(B, 3))) | {B - 1}):
        key = b % 3
        if key not in refs:
            refs[key] = restate_like(e, b, instance_deck(cd.deck, volts[b]), "OP", AUTO, 0.0, cap, cap)
            assert refs[key].rejected > 0 or refs[key].levels > 2
        compare_log(e, b, refs[key], f"{label} wrap instance {b}")
        assert max_err(x[b], refs[key].x, *NL) <= 1.0, b
        eb = engine(cd.deck, batch=1, overrides=cd.overrides(volts[b:b + 1]), knobs=knobs, g_min=0.0, max_newton=cap)
        eb.analyze_op_stepping(F.MODE_OP, AUTO, **ctl)
        assert same_bits(eb.solution()[0], x[b]), f"instance {b} differs from its batch-1 run"
        eb.close()
    for b in range(B):   # (instances with the same drive levels in the same places are the same problem)
        assert same_bits(x[b], x[b % 3]) and s["levels"][b] == s["levels"][b % 3], b
    e.close()


def check_failure(knobs, label=""):
    """5. the failure path: dl_min 0.1 and max_levels 3 on the 10 V chain, beside instances that solve"""
    d = diode_chain(1)
    volts = [0.5, 10.0, 2.0]
    for ctl in (dict(dl_min=0.1), dict(max_levels=3)):
        for method in (GMIN, SOURCE):
            refs = [restate(instance_deck(d, [v]), "OP", method, 0.0, 6, 6, **ctl) for v in volts]
            assert refs[1].solved_in == -1 and refs[0].solved_in == 0, [r.solved_in for r in refs]
            _, e = chain_engine(knobs, volts)
            st = e.analyze_op_stepping(F.MODE_OP, method, check=False, step_max_newton=6, log_capacity=64, **ctl)
            s, status, x = e.op_step_state(), e.state()["status"], e.solution()
            print(f"OPSTEP {label} failure {ctl} method {method}: rc {st['rc']} solved_in {s['phase_solved_in'].tolist()} lambda {s['lambda_reached'].tolist()}")
            for b, v in enumerate(volts):
                ref = restate_like(e, b, instance_deck(d, [v]), "OP", method, 0.0, 6, 6, **ctl)
                compare_log(e, b, ref, f"{label} failure instance {b}")
                assert max_err(x[b], ref.x, *NL) <= 1.0, (b, x[b], ref.x)     # (failed: the last accepted level's solution)
                assert (status[b] == 0) == (ref.solved_in >= 0), (b, status)
            n_failed = sum(r.solved_in < 0 for r in refs)
            assert status[1] in (F.ERR_NO_CONVERGENCE, F.ERR_SINGULAR) and st["rc"] == status[1] and st["n_failed"] == n_failed, (st, status)
            # the other instances: their batch-1 run, bit for bit
            for b in (0, 2):
                _, eb = chain_engine(knobs, volts[b:b + 1])
                eb.analyze_op_stepping(F.MODE_OP, method, check=False, step_max_newton=6, log_capacity=64, **ctl)
                assert same_bits(eb.solution()[0], x[b]), b
                eb.close()
            # a following pe_hip_analyze_dc: exactly what an engine that never stepped does from the same state (handed over as a
            # checkpoint) -- full source values and the engine's g_min in the system it stamps
            _, f = chain_engine(knobs, volts)
            f.restore(e.checkpoint())      # (a restore re-applies the load-time values of the engine it lands in)
            rc_f = f.analyze_dc(F.MODE_OP, check=False)["rc"]
            rc_e = e.analyze_dc(F.MODE_OP, check=False)["rc"]
            assert rc_e == rc_f and same_bits(e.solution(), f.solution()) and np.array_equal(e.state()["status"], f.state()["status"]), (rc_e, rc_f)
            for b in range(3):
                (_, _, va, rhs), (_, _, vf, rf) = e.matrix(b), f.matrix(b)
                assert same_bits(va, vf) and same_bits(rhs, rf) and volts[b] in rhs.tolist(), (b, rhs)
            e.close()
            f.close()


def check_relay(knobs, label=""):
    """6a. a deck with a relay: its contact state is part of the state that is zeroed, saved and restored.  The coil sits on the stepped
    source, so the contact closes at some level of source stepping and stays closed (hysteresis) as the oracle says."""
    d = pe.deck.Deck()
    d.n_nodes = 3
    d.add("VDC", (1, 0), 8.0)
    d.add("RELAY", (1, 0, 1, 2), 5.0, 3.0)
    d.add("R", (2, 3), 100.0)
    d.add("D", (3, 0))
    d.add("R", (1, 0), 1e4)
    cap = 6
    for method in (SOURCE, GMIN):
        e = engine(d, knobs=knobs, g_min=0.0, max_newton=cap)
        st = e.analyze_op_stepping(F.MODE_OP, method, check=False, step_max_newton=cap, log_capacity=64)
        ref = restate_like(e, 0, d, "OP", method, 0.0, cap, cap)
        print(f"OPSTEP {label} relay method {method}: rc {st['rc']} solved_in {ref.solved_in} levels {ref.levels} rejected {ref.rejected}")
        assert ref.solved_in == method and (ref.rejected > 0 or method == GMIN), (ref.solved_in, ref.rejected)
        compare_log(e, 0, ref, f"{label} relay")
        assert st["rc"] == 0 and max_err(e.solution()[0], ref.x, *NL) <= 1.0
        assert abs(e.solution()[0][1] - 8.0) < 1e-6, "the contact must be closed at the solution"
        e.close()


def check_switch_generator(knobs, label=""):
    """6b. a generator and a switch beside a stepped source: the switch's resistance is never scaled and the generator keeps its value -- read
    from the system of an intermediate level (max_levels cuts the call short; pe_hip_get_matrix shows the last stamp)"""
    d = pe.deck.Deck()
    d.n_nodes = 4
    d.add("VDC", (1, 0), 10.0)
    d.add("SW", (1, 2), 0.0)          # open: -r_open on its branch diagonal
    d.add("R", (1, 2), 100.0)
    d.add("D", (2, 0))
    d.add("SQR", (3, 0), 5.0, 1.0, 1e3, 0.25, 0.0)
    d.add("R", (3, 4), 1e3)
    d.add("R", (4, 0), 1e3)
    d.add("IDC", (0, 4), 1e-3)
    e = engine(d, knobs=knobs, g_min=0.0, max_newton=6)
    st = e.analyze_op_stepping(F.MODE_OP, SOURCE, check=False, step_max_newton=6, max_levels=2, log_capacity=8)
    cut = restate(d, "OP", SOURCE, 0.0, 6, 6, max_levels=2)
    compare_log(e, 0, cut, f"{label} switch + generator, two levels")
    assert st["rc"] != 0 and [t for _, t, *_ in cut.log] == [0.0, 0.125], (st, cut.log)
    rp, ci, va, rhs = e.matrix(0)
    A, b = oracle_level(scaled(d, 0.125), "OP", 0.0, None, 64)[0].assemble("OP")
    A = A.toarray()
    dense = np.zeros_like(A)
    for r in range(len(rp) - 1):
        dense[r, ci[rp[r]:rp[r + 1]]] = va[rp[r]:rp[r + 1]]
    k_vdc, k_sw, k_gen = d.n_nodes, d.n_nodes + 1, d.n_nodes + 2               # branch rows in model order: VDC, SW, SQR
    print(f"OPSTEP {label} switch: branch diagonal {dense[k_sw, k_sw]!r} rhs {rhs.tolist()}")
    assert dense[k_sw, k_sw] == -1e12 == A[k_sw, k_sw], "the switch's resistance must not be scaled"
    assert same_bits(rhs[k_vdc], 0.125 * 10.0) and same_bits(rhs[3], 0.125 * 1e-3), rhs      # VDC and IDC at lambda = 1/8
    assert rhs[k_gen] == b[k_gen] != 0.0, (rhs[k_gen], b[k_gen])                            # the generator at its t = 0 value, unscaled
    assert max_err(e.solution()[0], cut.x, *NL) <= 1.0
    # ... and the full call: the real values are back, the solution is the oracle's
    st = e.analyze_op_stepping(F.MODE_OP, SOURCE, step_max_newton=6, log_capacity=64)
    full = restate(d, "OP", SOURCE, 0.0, 6, 6)
    compare_log(e, 0, full, f"{label} switch + generator")
    assert max_err(e.solution()[0], full.x, *NL) <= 1.0
    rhs = e.matrix(0)[3]
    assert rhs[d.n_nodes] == 10.0 and rhs[3] == 1e-3, rhs
    e.close()


def check_refusals(knobs, label=""):
    """7a. PE_HIP_ERR_ARG: modes, methods, negative fields, NULL control; state reads before a call; nothing fails costs one launch"""
    d, e = chain_engine(knobs, [0.5, 0.3])
    lib = F.lib()
    null = F.C.POINTER(F.OpStepControl)()
    assert lib.pe_hip_get_op_step_state(e._h, 0, 2, None, None, None, None, None) == F.ERR_ARG and b"no stepping call yet" in lib.pe_hip_last_error(e._h)
    assert lib.pe_hip_get_op_step_log(e._h, 0, 0, None, None, None, None, None, None) == F.ERR_ARG
    assert lib.pe_hip_analyze_op_stepping(e._h, F.MODE_OP, null, None) == F.ERR_ARG
    for mode in (F.MODE_TR, 2, -1):
        assert e.analyze_op_stepping(mode, AUTO, check=False)["rc"] == F.ERR_ARG, mode
    for method in (0, 4, -1):
        assert e.analyze_op_stepping(F.MODE_OP, method, check=False)["rc"] == F.ERR_ARG, method
    for bad in (dict(max_levels=-1), dict(step_max_newton=-1), dict(log_capacity=-1), dict(dl_init=-0.5), dict(grow=-2.0), dict(shrink=-1.0),
                dict(dl_min=-1e-3), dict(g_start=-1.0), dict(grow=float("nan"))):
        assert e.analyze_op_stepping(F.MODE_OP, AUTO, check=False, **bad)["rc"] == F.ERR_ARG, bad
    before = e.solution().copy()
    assert same_bits(before, np.zeros_like(before)), "a refused call must not have solved anything"
    for mode in (F.MODE_OP, F.MODE_DC, F.MODE_TROP):
        e.reset()
        st = e.analyze_op_stepping(mode, AUTO, log_capacity=0)
        assert st["n_direct"] == 2 and st["n_levels"] == 0 and st["n_launches"] == 1 and st["n_solves"] == 1, st
        _, f = chain_engine(knobs, [0.5, 0.3])
        f.analyze_dc(mode)
        assert same_bits(e.solution(), f.solution()) and f.checkpoint() == e.checkpoint(), "nothing failed: the state pe_hip_analyze_dc leaves"
        assert e.op_step_state()["phase_solved_in"].tolist() == [0, 0] and e.op_step_log(1)["n_total"] == 0
        f.close()
    e.close()


def check_overlay(knobs, label=""):
    """7b. with a host-stamp overlay SOURCE is refused and AUTO runs the direct attempt and gmin stepping only"""
    d = diode_chain(1)
    d.devices[0] = ("VDC", (1, 0), (10.0,))
    e = F.Engine()
    e.set_options(g_min=0.0, max_newton=6)
    for k, v in knobs.items():
        e.set_knob(k, v)
    C = F.C
    FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))

    def hook(user, event, mode, t, dt, x, a, b):
        if event == 1:
            a[0] = 1e-12      # (a conductance far below anything NL or a Newton count can see)
            b[0] = 0.0
        return 0
    cb = FN(hook)
    F.lib().pe_hip_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_int, FN, C.c_void_p]
    one = np.array([1], dtype=np.int32)
    assert F.lib().pe_hip_set_overlay(e._h, 1, F._ip(one), F._ip(one), F._dp(np.array([1e-12])), 1, F._ip(one), 0, cb, None) == 0
    e.load_deck(d, 1)
    e.reset()
    assert e.analyze_op_stepping(F.MODE_OP, SOURCE, check=False)["rc"] == F.ERR_ARG and b"overlay" in F.lib().pe_hip_last_error(e._h)
    st = e.analyze_op_stepping(F.MODE_OP, AUTO, check=False, step_max_newton=6, log_capacity=64)
    lg = e.op_step_log(0)
    assert set(lg["phase"].tolist()) == {GMIN} and st["n_source"] == 0, (st, lg)
    ref = restate(d, "OP", GMIN, 0.0, 6, 6)
    assert ref.solved_in == -1 and st["rc"] != 0 and e.op_step_state()["phase_solved_in"][0] == -1 and lg["n_total"] == ref.levels
    e.close()


def check_sweep(label=""):
    """7c. pe_hip_sweep_operating_point_stepping: the same call per device engine -- every instance's solution is the same bits whichever
    device ran it and equals the single engine's; the statistics are summed"""
    d = pe.deck.bjt_common_emitter()
    volts = np.array([5.0, 0.4, 4.0, 6.0, 0.3, 5.5, 4.5])
    ov = {"VDC": volts[:, None, None]}
    e = engine(d, batch=len(volts), overrides=ov, g_min=0.0)
    se = e.analyze_op_stepping(F.MODE_OP, AUTO)
    assert se["n_direct"] >= 1 and se["n_gmin"] >= 1 and se["n_failed"] == 0, se
    out = {}
    for mask in (1, 3):
        s = F.Sweep(mask)
        s.set_options(g_min=0.0)
        s.load_deck(d, len(volts), ov)
        s.reset()
        st = s.operating_point_stepping(F.MODE_OP, AUTO)
        out[mask] = (s.shards(), s.solution(), st)
        s.close()
    assert len(out[1][0]) == 1 and len(out[3][0]) == 2, (out[1][0], out[3][0])
    assert same_bits(out[1][1], out[3][1]) and same_bits(out[1][1], e.solution())
    for k in ("n_levels", "n_accepted", "n_rejected", "n_direct", "n_gmin", "n_source", "n_failed", "newton_iters"):
        assert out[1][2][k] == out[3][2][k] == se[k], (k, out[1][2], out[3][2], se)
    ref = restate(instance_deck(d, volts[:1]), "OP", AUTO, 0.0, 64, 64)
    assert max_err(out[3][1][0], ref.x, *NL) <= 1.0
    e.close()
    print(f"OPSTEP {label} sweep: {out[3][2]}")
