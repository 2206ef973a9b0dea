"""Shared bodies of the DC sweep tests (pe_hip_set_dc_sweep_rows / pe_hip_analyze_dc_sweep / pe_hip_get_dc_sweep / _status, include/pe_hip.h):
tests/test_dc_sweep_emu.py runs them on the host emulation, one child process per case, tests/test_gpu_dc_sweep.py on the device.

References are never the code under test: the unchanged oracle (oracle/pe_oracle.py), one Oracle per point -- for continuation the rule is
replayed on the oracle with the seed that seed_point reports, copying x and the diode state -- and the main engine's own single-point path
(restore / update_param / analyze_dc), which the sweep does not touch.  Tolerances: the project's LIN and NL through max_err."""
import copy

import numpy as np

from parity_common import max_err, pe

F = pe.ffi
LIN = (1e-9, 1e-7)          # the project's tolerances (tests/test_gpu_parity.py)
NL = (1e-6, 1e-5)
KIND = {F.VDC: "VDC", F.IDC: "IDC", F.R: "R"}
_ORACLE = None


def oracle_mod():
    global _ORACLE
    if _ORACLE is None:
        import pe_load
        _ORACLE = pe_load.load_oracle()
    return _ORACLE


# ---------------------------------------------------------------------------------------------------------------- decks
def with_value(deck, kind, index, value):
    """a copy of the deck whose index-th device of that kind has `value` in column 0"""
    d = copy.deepcopy(deck)
    seen = -1
    for i, (k, n, p) in enumerate(d.devices):
        if k == KIND[kind]:
            seen += 1
            if seen == index:
                d.devices[i] = (k, n, (float(value),) + tuple(p[1:]))
                return d
    raise IndexError((kind, index))


def replace_source(deck, old):
    """the deck with its one `old` source (a VAC or a generator: nothing a DC sweep can step) replaced by a VDC in the same place"""
    d = copy.deepcopy(deck)
    (i,) = [i for i, (k, _, _) in enumerate(d.devices) if k == old]
    d.devices[i] = ("VDC", d.devices[i][1][:2], (1.0,))
    return d


def diode_chain(n):
    """VDC - 100 Ohm - n default diodes in series to ground"""
    d = pe.deck.Deck()
    d.n_nodes = 1 + n
    d.add("VDC", (1, 0), 0.0)
    d.add("R", (1, 2), 100.0)
    for k in range(n):
        d.add("D", (2 + k, 3 + k if k < n - 1 else 0))
    return d


def divider_with_idc():
    """divider_dc + a current source into its middle node (the deck has no IDC of its own)"""
    d = pe.deck.divider_dc()
    d.add("IDC", (0, 1), 0.01)
    return d


def controlled_mix_dc():
    """controlled_mix + what a DC sweep can step: its VAC is 0 V at DC, so a VDC behind 200 Ohm and an IDC feed node 2"""
    d = pe.deck.controlled_mix()
    d.n_nodes = 11
    d.add("VDC", (11, 0), 1.0)
    d.add("R", (11, 2), 200.0)
    d.add("IDC", (0, 2), 1e-3)
    return d


def mesh_dc(w=12, h=12):
    return replace_source(pe.deck.rc_mesh(w, h, 1, True), "VAC")


def relay_dc():
    return replace_source(pe.deck.relay_ramp(), "TRI")


# ---------------------------------------------------------------------------------------------------------------- engines
def engine(deck, batch=1, overrides=None, knobs=None, **opts):
    e = F.Engine()
    e.set_options(**opts)
    for k, v in (knobs or {}).items():
        e.set_knob(k, v)
    e.load_deck(deck, batch, overrides)
    e.reset()
    return e


def single_point_loop(e, values, kind, index, mode=F.MODE_OP, warm=False):
    """the main engine's own path, one point at a time: from the state the engine is in (warm: from the last converged point instead).
    Returns (x [n][batch][rows] with NaN where the solve failed, rc [n], Newton iterations of instance 0 [n])."""
    blob = e.checkpoint()
    xs, rcs, its = [], [], []
    for v in values:
        if not warm:
            e.restore(blob)
        n0 = len(e.newton_trace())
        e.update_param(kind, index, 0, v)
        rc = e.analyze_dc(mode, check=False)["rc"]
        tr = e.newton_trace()
        x = e.solution()
        if rc != 0:
            x = np.full_like(x, np.nan)
            e.restore(blob)
        elif warm:
            blob = e.checkpoint()
        xs.append(x)
        rcs.append(rc)
        its.append(int(tr[n0]) if len(tr) > n0 else 0)
    if not warm:
        e.restore(blob)
    return np.array(xs), np.array(rcs), np.array(its)


# ---------------------------------------------------------------------------------------------------------------- oracle
def oracle_at(deck, kind, index, value, g_min=0.0, seed=None, mode="OP"):
    """one Oracle at one point, from the zero state or from a copy of `seed`'s x and diode state; returns it after its solve with .iters"""
    o = oracle_mod().Oracle(with_value(deck, kind, index, value), g_min=g_min)
    o.prepare()
    if seed is not None:
        o.x = seed.x.copy()
        if o.dio is not None:
            o.dio.Ud_last = seed.dio.Ud_last.copy()
            o.dio.geq = seed.dio.geq.copy()
            o.dio.Ieq = seed.dio.Ieq.copy()
    o.iters = o.solve(mode)
    return o


def oracle_sweep(deck, kind, index, values, g_min=0.0):
    return np.array([oracle_at(deck, kind, index, v, g_min).x for v in values])


def converged(o, cap):
    return 0 < o.iters <= cap and bool(np.all(np.isfinite(o.x)))


def nearest_converged(values, ok):
    """The rule, restated: for every failing point the converged point nearest in sorted-value position, where equal values share a
    position; ties go to the lower position.  values, ok in the caller's order; returns the caller's index of the seed, -1: none / not failing."""
    values = np.asarray(values, dtype=float)
    order = np.argsort(values, kind="stable")
    pos = np.empty(len(values), dtype=int)
    pos[order] = np.arange(len(values))
    rank = np.searchsorted(np.unique(values), values)
    seed = np.full(len(values), -1)
    good = [i for i in range(len(values)) if ok[i]]
    for i in range(len(values)):
        if ok[i] or not good:
            continue
        seed[i] = min(good, key=lambda s: (abs(rank[s] - rank[i]), pos[s]))
    return seed


def oracle_continuation(deck, kind, index, values, cap, max_rounds=0, g_min=0.0):
    """the whole continuation of one pass on the oracle: returns (oracles per point, ok per point, history of ok per round, seeds used)"""
    n = len(values)
    os_ = [oracle_at(deck, kind, index, v, g_min) for v in values]
    ok = np.array([converged(o, cap) for o in os_])
    hist = [ok.copy()]
    used = np.full(n, -1)
    rounds = 0
    while not ok.all() and ok.any() and rounds < (max_rounds if max_rounds > 0 else n):
        seed = nearest_converged(values, ok)
        new = ok.copy()
        for i in np.nonzero(~ok)[0]:
            os_[i] = oracle_at(deck, kind, index, values[i], g_min, seed=os_[seed[i]])
            used[i] = seed[i]
            new[i] = converged(os_[i], cap)
        rounds += 1
        progress = new.sum() > ok.sum()
        ok = new
        hist.append(ok.copy())
        if not progress:
            break
    return os_, ok, hist, used


def snapshot(e, with_ac=False):
    """what a DC sweep must leave alone, as bits"""
    st = e.state()
    out = [e.solution().tobytes(), e.checkpoint(), e.newton_trace().tobytes()] + [np.asarray(st[k]).tobytes() for k in sorted(st)]
    if with_ac:
        re = np.empty((2, e.batch, e.rows))
        im = np.empty_like(re)
        assert F.lib().pe_hip_get_ac_sweep(e._h, 0, 2, 0, e.batch, F._dp(re), F._dp(im)) == 0
        out += [re.tobytes(), im.tobytes()]
    return out


# ================================================================================================================ the cases
def check_linear():
    """1. VDC, IDC and R (six decades) on divider_dc and controlled_mix against the oracle under LIN; unsorted values with a duplicate and a
    negative one; results in the caller's order.  (A negative resistance in series with controlled_mix's junction has no unique operating
    point: the negative R value is swept on the divider only.)"""
    lists = {F.VDC: [3.0, -1.5, 0.5, 3.0, 7.0, 0.0], F.IDC: [1e-3, -2e-3, 5e-4, 1e-3, 0.0, 2e-2],
             F.R: [1e3, 1.0, 1e6, 1e3, 10.0, 1e5, 1e2, 1e4]}
    for deck, targets in ((divider_with_idc(), {F.VDC: 0, F.IDC: 0, F.R: 1}), (controlled_mix_dc(), {F.VDC: 0, F.IDC: 0, F.R: 1})):
        e = engine(deck)
        for kind, index in targets.items():
            vals = list(lists[kind])
            if kind == F.R and not deck.has_nonlinear():
                vals.insert(3, -47.0)
            x, status, st = e.analyze_dc_sweep(vals, kind, index)
            ref = oracle_sweep(deck, kind, index, vals)
            assert x.shape == (len(vals), 1, e.rows) and list(status) == [0] * len(vals), (status, st)
            err = max_err(x[:, 0, :], ref, *LIN)
            print("linear", KIND[kind], deck.rows, "err/tol", err)
            assert err <= 1.0, (KIND[kind], err)
            dup = [i for i, v in enumerate(vals) if vals.index(v) != i][0]
            assert np.array_equal(x[dup], x[vals.index(vals[dup])]), "the duplicate point"
            assert st["n_failed"] == 0 and st["n_rounds"] == 0 and st["n_points"] == len(vals), st
        e.close()


def check_nonlinear_no_continuation(name):
    """2. continuation off: every point equals the main engine's single-point path from the same state (NL) and the oracle (NL);
    n_rounds == 0; pass sizes 1, 4 and automatic agree (NL); on the mesh also on the split schedule"""
    deck, kind, index, vals, knob_sets = {
        "diode_op": (pe.deck.diode_op(), F.VDC, 0, [1.0, 0.2, -3.0, 0.75, 5.0, 0.2, 2.5, 0.6, 12.0], [{}]),
        "nmos": (pe.deck.nmos_common_source(), F.VDC, 1, [2.0, 0.0, 0.9, 1.1, 3.5, 1.5, 5.0, 2.0, 2.6], [{}]),
        "mesh": (mesh_dc(), F.VDC, 0, [2.0, 0.3, -1.0, 0.9, 4.0, 0.6, 1.4, 0.3, 3.0], [{}, {"SPLIT": 1}]),
    }[name]
    ref_o = oracle_sweep(deck, kind, index, vals)
    for knobs in knob_sets:
        ref_e, rcs, _ = single_point_loop(engine(deck, knobs=knobs), vals, kind, index)
        assert not rcs.any(), rcs
        res = {}
        for P in (1, 4, 0):
            e = engine(deck, knobs=dict(knobs, DC_SWEEP_POINTS=P))
            x, status, st = e.analyze_dc_sweep(vals, kind, index, continuation=0)
            assert list(status) == [0] * len(vals) and st["n_rounds"] == 0 and st["n_failed_cold"] == 0, st
            assert st["points_per_pass"] == (P if P else len(vals)) and st["n_passes"] == (-(-len(vals) // P) if P else 1), st
            ee, eo = max_err(x, ref_e, *NL), max_err(x[:, 0, :], ref_o, *NL)
            print("nonlinear", name, knobs, "P", P, "err/tol vs engine", ee, "vs oracle", eo)
            assert ee <= 1.0 and eo <= 1.0, (name, P, ee, eo)
            res[P] = x
            e.close()
        assert max_err(res[1], res[0], *NL) <= 1.0 and max_err(res[4], res[0], *NL) <= 1.0 and max_err(res[4], res[1], *NL) <= 1.0


def check_mapping():
    """3. batch 3 with per-instance parameters, 41 points at P = 8 (six passes, the last partial): instance b at point p is the
    single-instance run of instance b's parameters; a kept-rows subset with a branch row; set_dc_sweep_rows(None)"""
    deck = pe.deck.diode_op()
    r = np.array([1000.0, 330.0, 4700.0])
    vals = np.linspace(-1.0, 3.0, 41)[np.random.default_rng(7).permutation(41)]
    e = engine(deck, 3, {"R": r[:, None, None]}, {"DC_SWEEP_POINTS": 8})
    full, status, st = e.analyze_dc_sweep(vals, F.VDC, 0, continuation=0)
    assert full.shape == (41, 3, e.rows) and st["n_passes"] == 6 and st["points_per_pass"] == 8 and not status.any(), st
    for b in range(3):
        one = engine(with_value(deck, F.R, 0, r[b]))
        ref, rcs, _ = single_point_loop(one, vals, F.VDC, 0)
        err = max_err(full[:, b, :], ref[:, 0, :], *NL)
        print("mapping instance", b, "err/tol", err)
        assert not rcs.any() and err <= 1.0, (b, err)
        assert max_err(full[:, b, :], oracle_sweep(with_value(deck, F.R, 0, r[b]), F.VDC, 0, vals), *NL) <= 1.0
        one.close()
    rows = [2, 0, 2]                                   # the source's branch current (twice) and its node
    e.set_dc_sweep_rows(rows)
    buf = np.empty((1, 1, 3))
    assert F.lib().pe_hip_get_dc_sweep(e._h, 0, 1, 0, 1, F._dp(buf)) == F.ERR_ARG, "a stored sweep has the layout of its rows"
    x, _, _ = e.analyze_dc_sweep(vals, F.VDC, 0, continuation=0)
    assert x.shape == (41, 3, 3) and np.array_equal(x, full[:, :, rows])
    part = np.empty((5, 2, 3))                         # a slice of points and instances through the C ABI
    assert F.lib().pe_hip_get_dc_sweep(e._h, 30, 5, 1, 2, F._dp(part)) == 0 and np.array_equal(part, x[30:35, 1:3])
    for bad in ([0, e.rows], [-1]):
        try:
            e.set_dc_sweep_rows(bad)
            raise AssertionError("accepted")
        except F.PeHipError as err:
            assert err.code == F.ERR_ARG
    e.set_dc_sweep_rows(None)
    x, _, _ = e.analyze_dc_sweep(vals, F.VDC, 0, continuation=0)
    assert np.array_equal(x, full)
    e.close()


CHAIN_V = np.linspace(0.0, 10.0, 41)


def check_continuation():
    """4. the three-diode chain at max_newton = 6: the cold failures are the main engine's own, one or more rounds converge every point,
    values and Newton counts match the seed-matched oracle replay, no seed had failed when it was used; with continuation off the cold
    failures read NaN with PE_HIP_ERR_NO_CONVERGENCE"""
    deck, cap = diode_chain(3), 6
    _, cold_rc, cold_it = single_point_loop(engine(deck, max_newton=cap), CHAIN_V, F.VDC, 0)
    n_cold = int((cold_rc != 0).sum())
    e = engine(deck, max_newton=cap)
    max_rounds = 4
    x, status, st = e.analyze_dc_sweep(CHAIN_V, F.VDC, 0, continuation=1, max_rounds=max_rounds)
    s, it, seed = e.dc_sweep_status()
    print("continuation", st, "cold failures of the main engine", n_cold)
    assert st["n_failed_cold"] == n_cold > 0, (st, n_cold)
    assert not status.any() and not s.any() and st["n_failed"] == 0 and 1 <= st["n_rounds"] <= max_rounds, st
    assert st["n_reseeded"] >= n_cold
    cold_ok = cold_rc == 0
    assert np.array_equal(seed[:, 0] == -1, cold_ok), "exactly the cold failures were reseeded"
    # the replay: every point from the seed the engine reports
    os_ = {}

    def replay(i):
        if i not in os_:
            os_[i] = oracle_at(deck, F.VDC, 0, CHAIN_V[i], seed=None if seed[i, 0] < 0 else replay(int(seed[i, 0])))
        return os_[i]
    ref = np.array([replay(i).x for i in range(len(CHAIN_V))])
    err = max_err(x[:, 0, :], ref, *NL)
    print("continuation err/tol", err, "iterations", it[:, 0])
    assert err <= 1.0, err
    assert all(converged(os_[i], cap) for i in os_)
    assert np.array_equal(it[:, 0], [os_[i].iters for i in range(len(CHAIN_V))]), "the Newton count of the single successful attempt"
    assert np.array_equal(it[cold_ok, 0], cold_it[cold_ok])
    # no seed had failed when it was used: with one round, every seed converged cold; in general, the statuses after k rounds
    ok = cold_ok.copy()
    for k in range(1, st["n_rounds"] + 1):
        _, _, stk = e.analyze_dc_sweep(CHAIN_V, F.VDC, 0, continuation=1, max_rounds=k, check=False)
        sk, _, seedk = e.dc_sweep_status()
        tried = ~ok
        assert ok[seedk[tried, 0]].all(), k
        assert np.array_equal(seedk[tried, 0], nearest_converged(CHAIN_V, ok)[tried]), k
        ok = sk[:, 0] == 0
    # the oracle's own continuation agrees on who converges when
    _, ok_o, hist, _ = oracle_continuation(deck, F.VDC, 0, CHAIN_V, cap)
    assert np.array_equal(hist[0], cold_ok) and ok_o.all()
    # continuation off: exactly the cold failures, as NaN
    x0, status0, st0 = e.analyze_dc_sweep(CHAIN_V, F.VDC, 0, continuation=0, check=False)
    s0, _, _ = e.dc_sweep_status()
    assert st0["rc"] == F.ERR_NO_CONVERGENCE and st0["n_rounds"] == 0 and st0["n_failed"] == n_cold, st0
    assert np.array_equal(np.isnan(x0[:, 0, :]).all(axis=1), ~cold_ok) and np.array_equal(np.isnan(x0[:, 0, :]).any(axis=1), ~cold_ok)
    assert np.array_equal(s0[:, 0], np.where(cold_ok, 0, F.ERR_NO_CONVERGENCE)) and np.array_equal(status0, s0[:, 0])
    assert max_err(x0[cold_ok, 0, :], ref[cold_ok], *NL) <= 1.0
    e.close()


def check_no_progress():
    """5. the one-diode chain at max_newton = 6: the oracle's replay of the rule stalls with a point left (checked first: 38 -> 30 -> 1
    failing, then a round that converges nothing), and so does the engine -- n_failed > 0 after at most n_points rounds, the failing point
    NaN, the others right"""
    deck, cap = diode_chain(1), 6
    os_, ok_o, hist, used = oracle_continuation(deck, F.VDC, 0, CHAIN_V, cap)
    fails = [int((~h).sum()) for h in hist]
    print("oracle replay, failing per round", fails)
    assert not ok_o.all() and fails[-1] == fails[-2] > 0, "the oracle replay must stall at this cap"
    e = engine(deck, max_newton=cap)
    x, status, st = e.analyze_dc_sweep(CHAIN_V, F.VDC, 0, continuation=1, check=False)
    s, it, seed = e.dc_sweep_status()
    print("no progress", st)
    assert st["rc"] != 0 and 0 < st["n_failed"] == int((~ok_o).sum()) and st["n_rounds"] <= len(CHAIN_V) and st["n_rounds"] == len(hist) - 1, st
    assert np.array_equal(s[:, 0] == 0, ok_o) and np.array_equal(status != 0, ~ok_o)
    assert np.isnan(x[~ok_o]).all() and not np.isnan(x[ok_o]).any()
    assert np.array_equal(seed[ok_o, 0], used[ok_o])
    ref = np.array([o.x for o in os_])
    err = max_err(x[ok_o, 0, :], ref[ok_o], *NL)
    print("no progress err/tol", err)
    assert err <= 1.0
    e.close()


def check_classify_edges(n):
    """6. diode_op, three rows, n points in ONE pass from a converged state in the middle of the range, with a Newton cap that leaves
    failures at both ends: after every round seed_point equals the restated rule on the statuses of the round before"""
    deck, cap = pe.deck.diode_op(), 3
    e = engine(deck, max_newton=cap, knobs={"DC_SWEEP_POINTS": n})
    e.set_options(max_newton=64)
    e.update_param(F.VDC, 0, 0, 5.0)
    e.analyze_dc(F.MODE_OP)                               # the state every point starts from: the operating point at 5 V
    e.set_options(max_newton=cap)
    vals = np.linspace(-30.0, 40.0, n) if n > 1 else np.array([40.0])
    if n > 8:
        vals[5], vals[n - 3], vals[n // 2 + 1] = vals[4], vals[n - 4], vals[n // 2]     # duplicates: at a failing end and in the middle
        vals = vals[np.random.default_rng(n).permutation(n)]
    e.set_dc_sweep_rows([0, 1, 2])
    _, _, st = e.analyze_dc_sweep(vals, F.VDC, 0, continuation=0, check=False)
    assert st["n_passes"] == 1 and st["points_per_pass"] == n, st
    ok = e.dc_sweep_status()[0][:, 0] == 0
    order = np.argsort(vals, kind="stable")
    print("classify", n, "cold failures", int((~ok).sum()), "first / last sorted point ok", ok[order[0]], ok[order[-1]])
    assert not ok[order[-1]] and (n == 1 or (not ok[order[0]] and ok.any())), "failures at both ends of the range, converged points between"
    prev_seed = np.full(n, -1)
    for k in range(1, 8):
        x, _, st = e.analyze_dc_sweep(vals, F.VDC, 0, continuation=1, max_rounds=k, check=False)
        s, _, seed = e.dc_sweep_status()
        want = nearest_converged(vals, ok)
        ran = st["n_rounds"] == k
        if ran:
            assert np.array_equal(seed[~ok, 0], want[~ok]), (n, k)
        assert np.array_equal(seed[ok, 0], prev_seed[ok]), "a converged pair is never solved again"
        assert np.array_equal(np.isnan(x[:, 0, :]).any(axis=1), s[:, 0] != 0)
        new_ok = s[:, 0] == 0
        assert (new_ok | ~ok).all()
        if not ran or new_ok.all() or new_ok.sum() == ok.sum():
            break
        ok, prev_seed = new_ok, seed[:, 0].copy()
    if n == 1:
        assert st["n_failed"] == 1 and st["n_rounds"] == 0 and seed[0, 0] == -1, st
    e.close()


def check_trace():
    """7. TRACE: the relay's hysteresis loop over an up-down list against the oracle stepped in the same order; PARALLEL refuses a relay;
    TRACE on the diode chain equals the main engine's warm-started loop"""
    deck = relay_dc()
    up = np.arange(0.0, 8.25, 0.5)
    vals = np.concatenate([up, up[::-1][1:]])
    e = engine(deck)
    x, status, st = e.analyze_dc_sweep(vals, F.VDC, 1, order=F.DC_SWEEP_TRACE)
    assert not status.any() and st["n_passes"] == len(vals) and st["points_per_pass"] == 1, st
    closed = x[:, 0, 1] > 0.5                              # node 2: 1 V through the closed contact onto 100 Ohm
    want, state = [], False
    for v in vals:
        state = (v >= 5.0) if not state else not (v <= 3.0)
        want.append(state)
    assert np.array_equal(closed, want), (closed, want)
    assert closed[list(vals).index(4.5)] != closed[len(vals) - 1 - list(vals[::-1]).index(4.5)], "4.5 V: open going up, closed going down"
    o = oracle_mod().Oracle(deck)
    ref = []
    for v in vals:
        o.kinds["VDC"]["p"][1] = (float(v),)
        assert o.analyze_dc("OP")
        ref.append(o.x.copy())
    err = max_err(x[:, 0, :], np.array(ref), *NL)
    print("trace relay err/tol", err)
    assert err <= 1.0
    _, _, seed = e.dc_sweep_status()
    assert list(seed[:, 0]) == [-1] + list(range(len(vals) - 1)), "every point starts from the one before"
    rc = F.lib().pe_hip_analyze_dc_sweep(e._h, len(vals), F._dp(vals), F.C.byref(F.DcSweepControl(F.VDC, 1, 0, F.MODE_OP, F.DC_SWEEP_PARALLEL, 1, 0)), None, None)
    assert rc == F.ERR_ARG and b"TRACE" in F.lib().pe_hip_last_error(e._h)
    e.close()
    # the diode chain: the classical warm-started loop, a failing point skipped
    for n, cap in ((3, 6), (1, 6)):
        deck = diode_chain(n)
        ref, rcs, its = single_point_loop(engine(deck, max_newton=cap), CHAIN_V, F.VDC, 0, warm=True)
        e = engine(deck, max_newton=cap)
        x, status, st = e.analyze_dc_sweep(CHAIN_V, F.VDC, 0, order=F.DC_SWEEP_TRACE, check=False)
        s, it, seed = e.dc_sweep_status()
        good = rcs == 0
        print("trace chain", n, "failed points", int((~good).sum()), "iterations", it[:, 0])
        assert np.array_equal(status == 0, good) and st["n_failed"] == int((~good).sum()) and np.array_equal(status, rcs), (status, rcs)
        assert np.isnan(x[~good]).all() and max_err(x[good], ref[good], *NL) <= 1.0
        assert np.array_equal(it[good, 0], its[good]) and it[:, 0].max() <= 5 + (n == 1)
        last, want_seed = -1, []
        for i in range(len(CHAIN_V)):
            want_seed.append(last)
            last = i if good[i] else last
        assert list(seed[:, 0]) == want_seed
        e.close()


def check_isolation_and_refusals():
    """8. the main engine is read, never written; an update_param between two sweeps changes the second; every refusal is PE_HIP_ERR_ARG
    and leaves the same bits; get_dc_sweep before any sweep is PE_HIP_ERR_ARG"""
    lib = F.lib()
    deck = pe.deck.Deck()                             # a junction state to leave alone, an AC source for a stored AC sweep
    deck.n_nodes = 4
    deck.add("VDC", (1, 0), 0.8)
    deck.add("R", (1, 2), 470.0)
    deck.add("D", (2, 3))
    deck.add("R", (3, 0), 100.0)
    deck.add("C", (2, 0), 1e-9)
    deck.add("VAC", (4, 0), 1.0, 1e4, 0.0)
    deck.add("R", (4, 2), 1e3)
    r = np.array([470.0, 100.0, 1e3])
    e = engine(deck, 2, {"R": (r[None, :] * np.array([1.0, 1.5])[:, None])[:, :, None]})
    buf = np.empty((1, 2, e.rows))
    assert lib.pe_hip_get_dc_sweep(e._h, 0, 1, 0, 2, F._dp(buf)) == F.ERR_ARG and b"no DC sweep yet" in lib.pe_hip_last_error(e._h)
    assert lib.pe_hip_get_dc_sweep_status(e._h, 0, 1, 0, 2, None, None, None) == F.ERR_ARG
    e.analyze_dc(F.MODE_OP)
    e.analyze_tr(1e-7, 3)
    e.analyze_dc(F.MODE_OP)
    e.analyze_ac_sweep([1e3, 1e5])
    n_vdc = deck.count("VDC")
    before = snapshot(e, True)
    vals = [0.2, 1.5, -0.4, 0.9]
    x1, status, st = e.analyze_dc_sweep(vals, F.VDC, n_vdc - 1)
    assert not status.any() and snapshot(e, True) == before, "PARALLEL left the main engine alone"
    xt, _, _ = e.analyze_dc_sweep(vals, F.VDC, n_vdc - 1, order=F.DC_SWEEP_TRACE)
    assert snapshot(e, True) == before, "TRACE left the main engine alone"
    assert max_err(xt, x1, *NL) <= 1.0
    # the sweep is the single-point path from the engine's state, instance by instance
    ref, rcs, _ = single_point_loop(e, vals, F.VDC, n_vdc - 1)
    e.update_param(F.VDC, n_vdc - 1, 0, 0.8)
    assert not rcs.any() and max_err(x1, ref, *NL) <= 1.0
    # an update_param between two sweeps changes the second
    e.update_param(F.R, 0, 0, 10.0)
    x2, _, st2 = e.analyze_dc_sweep(vals, F.VDC, n_vdc - 1)
    assert st2["n_analyses"] >= 1 and not np.allclose(x2, x1, rtol=1e-6, atol=0.0)
    x3, _, st3 = e.analyze_dc_sweep(vals, F.VDC, n_vdc - 1)
    assert np.array_equal(x3, x2) and st3["n_analyses"] == 0, "nothing changed: the sweep engine and its analysis are reused"
    ref2, _, _ = single_point_loop(e, vals, F.VDC, n_vdc - 1)
    e.update_param(F.VDC, n_vdc - 1, 0, 0.8)
    assert max_err(x2, ref2, *NL) <= 1.0
    # refusals: PE_HIP_ERR_ARG, the same bits, the stored sweep still readable
    before = snapshot(e)
    v = np.array(vals)

    def refused(values, n=None, **kw):
        c = dict(kind=F.VDC, index=n_vdc - 1, column=0, mode=F.MODE_OP, order=F.DC_SWEEP_PARALLEL, continuation=1, max_rounds=0)
        c.update(kw)
        ctl = F.DcSweepControl(c["kind"], c["index"], c["column"], c["mode"], c["order"], c["continuation"], c["max_rounds"])
        vv = None if values is None else np.ascontiguousarray(values, dtype=float)
        rc = lib.pe_hip_analyze_dc_sweep(e._h, len(vv) if n is None else n, None if vv is None else F._dp(vv), F.C.byref(ctl), None, None)
        assert rc == F.ERR_ARG, (rc, kw)
        assert snapshot(e) == before
        got = np.empty_like(x3)
        assert lib.pe_hip_get_dc_sweep(e._h, 0, len(vals), 0, 2, F._dp(got)) == 0 and np.array_equal(got, x3)
    refused(v, n=0)
    refused(None, n=2)
    refused([0.1, float("nan")])
    refused([0.1, float("inf")])
    refused([100.0, 0.0], kind=F.R, index=0)
    refused(v, mode=F.MODE_TR)
    refused(v, mode=F.MODE_TROP)
    refused(v, order=2)
    refused(v, kind=F.CAP, index=0)
    refused(v, kind=F.VAC, index=0)
    refused(v, column=1)
    refused(v, index=n_vdc)
    refused(v, index=-1)
    assert lib.pe_hip_analyze_dc_sweep(e._h, 4, F._dp(v), None, None, None) == F.ERR_ARG and snapshot(e) == before
    e.close()
    f = F.Engine()                                     # no circuit
    ctl = F.DcSweepControl(F.VDC, 0, 0, F.MODE_OP, 0, 1, 0)
    assert lib.pe_hip_analyze_dc_sweep(f._h, 4, F._dp(v), F.C.byref(ctl), None, None) == F.ERR_ARG
    assert lib.pe_hip_set_dc_sweep_rows(f._h, 0, None) == F.ERR_ARG
    f.close()
    # a device with an unconnected pin sweeps nothing: every point is the same solve
    d = pe.deck.diode_op()
    d.add("R", (-1, 2), 50.0)
    e = engine(d)
    x, status, _ = e.analyze_dc_sweep([10.0, 3.0, -2.0], F.R, 1)
    assert not status.any() and np.array_equal(x[0], x[1]) and np.array_equal(x[0], x[2])
    assert max_err(x[0, 0], oracle_mod_x(d), *NL) <= 1.0
    e.close()


def oracle_mod_x(deck):
    o = oracle_mod().Oracle(deck)
    assert o.analyze_dc("OP")
    return o.x


def check_overlay_refused():
    """8. (continued) a circuit with a host-stamp overlay is refused"""
    C = F.C
    FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double))

    def hook(user, event, mode, t, dt, x, a, b):
        if event == 1:
            a[0] = 1e-3
            b[0] = 0.0
        return 0
    cb = FN(hook)
    lib = F.lib()
    lib.pe_hip_set_overlay.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.c_int, FN, C.c_void_p]
    one = np.array([1], dtype=np.int32)
    rep = np.array([1e-3])
    e = F.Engine()
    assert lib.pe_hip_set_overlay(e._h, 1, F._ip(one), F._ip(one), F._dp(rep), 1, F._ip(one), 0, cb, None) == 0
    e.load_deck(pe.deck.divider_dc())
    e.analyze_dc(F.MODE_DC)
    before = snapshot(e)
    v = np.array([1.0, 2.0])
    for order in (F.DC_SWEEP_PARALLEL, F.DC_SWEEP_TRACE):
        ctl = F.DcSweepControl(F.VDC, 0, 0, F.MODE_OP, order, 1, 0)
        assert lib.pe_hip_analyze_dc_sweep(e._h, 2, F._dp(v), C.byref(ctl), None, None) == F.ERR_ARG
        assert b"overlay" in lib.pe_hip_last_error(e._h) and snapshot(e) == before
    e.close()
