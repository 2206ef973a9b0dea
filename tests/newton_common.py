"""Shared by tests/test_newton_emu.py and tests/test_gpu_newton.py: the decision of when a Newton iterate is accepted -- the row test
|x - xprev| <= atol + rtol * max(|x|, |xprev|) of newton_violations (pe_front.hpp: the resident kernels), k_m2_finish (pe_kernels.hip: the
split schedule, through the col_src permutation, reduced by atomicOr over the workgroups) and their serial twins in
tests/emu/pe_kernels_emu.cpp, its reduction over the rows, and the host loop m2_point that retires the instances one by one -- at its
edges, against a restatement in plain double over the engine's own iterates.  Written against the Engine calls only: the same text runs on
the host emulation and on the device.

The recorder.  After a solve that ends with ERR_NO_CONVERGENCE at max_newton = k, solution() holds the k-th iterate (OP, DC, TROP; in TR
only t and the counters roll back).  record() runs a fresh engine per k = 1, 2, ... with every tolerance at 1e-300 (normal, not
subnormal; absorbed by any other term; 0 would mean "default") and the residual safety net off (a retry would stamp again), until every
instance returns 0: a step of exactly 0, which every tolerance accepts (or until K caps, where some cell of a busy circuit alternates
between two neighbouring doubles for ever).  An instance that stopped repeats its last iterate.  A TR step
starts from a checkpoint() blob restored before every capped run.  The runs must be reproducible: an instance that stopped at cap k
returns the same bits at every later cap, and the first and the last cap are run twice.  Sequences are recorded per schedule and per
platform; nothing compares an emulation sequence with a device sequence.

The reference.  predict() takes the iterates x_0 .. x_K of one instance, n_nodes and the four tolerances and returns the first k >= 1 at
which no row violates, with the violating rows of every earlier k.  The predicate is evaluated in double exactly as written:
not (abs(x - xp) <= tol), with max(|x|, |xp|) and r < n_nodes, so that a NaN on either side is a violation.  tol is formed twice:
unfused, fl(atol + fl(rtol * m)), and fused, atol + rtol * m exactly (fractions) rounded once -- the device compiler is free to contract
it.  The two differ by less than 2 ulp(tol), so the exact form is only computed for the rows whose |x - xp| lies within 4 ulp of the
unfused tol; everywhere else the decisions are equal by that bound.  A tolerance set may be used by a check only if both forms give the
same decision at every row and iteration of the recorded sequence: admitted() says so, and every generator asserts it (the one
admissible reduction: of the five sets of the busy-circuit check a rejected one is left out and reported)."""
import math
from fractions import Fraction

import numpy as np

from device_eval_common import F, NO_CONV, PE_THREADS, WRAP_CELLS, branch_rows
from parity_common import pe

TINY = 1e-300
OFF = dict(v_abstol=TINY, v_reltol=TINY, i_abstol=TINY, i_reltol=TINY)
SINGULAR = F.ERR_SINGULAR
MODES = {"OP": F.MODE_OP, "DC": F.MODE_DC, "TROP": F.MODE_TROP}


def effective(tols):
    """apply_options of pe_engine.cpp: 0 means the default, i_reltol = 0 follows v_reltol"""
    t = {k: float((tols or {}).get(k, 0.0)) for k in ("v_abstol", "v_reltol", "i_abstol", "i_reltol")}
    out = {"v_abstol": t["v_abstol"] if t["v_abstol"] > 0.0 else 1e-6, "v_reltol": t["v_reltol"] if t["v_reltol"] > 0.0 else 1e-3,
           "i_abstol": t["i_abstol"] if t["i_abstol"] > 0.0 else 1e-12}
    out["i_reltol"] = t["i_reltol"] if t["i_reltol"] > 0.0 else out["v_reltol"]
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def same_bits(a, b):
    return bits(a) == bits(b)


# ---- the reference --------------------------------------------------------------------------------------------------------------------------
def _violations(x, xp, n_nodes, tols, fused, pick=np.maximum, which="max"):
    """bool [rows]: rows that violate; `pick` / `which` restate the predicate with a planted fault (generator conditions only)"""
    t = effective(tols)
    rows = len(x)
    node = np.arange(rows) < n_nodes
    atol = np.where(node, t["v_abstol"], t["i_abstol"])
    rtol = np.where(node, t["v_reltol"], t["i_reltol"])
    with np.errstate(invalid="ignore"):
        m = np.abs(x) if which == "x" else pick(np.abs(x), np.abs(xp))
        d = np.abs(x - xp)
        tol = atol + rtol * m                      # unfused: two roundings
        bad = ~(d <= tol)
        if fused:
            near = np.abs(d - tol) <= 4.0 * np.spacing(tol)
            for r in np.nonzero(near)[0]:
                exact = Fraction(float(atol[r])) + Fraction(float(rtol[r])) * Fraction(float(m[r]))
                bad[r] = not (float(d[r]) <= float(exact))      # float(Fraction) rounds once, to nearest
    return bad


def predict(seq, n_nodes, tols, fused=False, **fault):
    """seq [K + 1][rows] -> (k, violating rows of every earlier iteration [k - 1 arrays]); k is None if every recorded iteration violates"""
    earlier = []
    for k in range(1, len(seq)):
        bad = _violations(seq[k], seq[k - 1], n_nodes, tols, fused, **fault)
        if not bad.any():
            return k, earlier
        earlier.append(np.nonzero(bad)[0])
    return None, earlier


def admitted(seqs, n_nodes, tols):
    """both forms of tol give the same decision at every row and iteration of every instance's sequence"""
    for seq in seqs:
        for k in range(1, len(seq)):
            if not np.array_equal(_violations(seq[k], seq[k - 1], n_nodes, tols, False), _violations(seq[k], seq[k - 1], n_nodes, tols, True)):
                return False
    return True


def predict_all(rec, tols, cap=64):
    """per instance: (status, iterations taken, index of the iterate held) under `tols` and max_newton = cap, from the recording"""
    assert admitted(rec.seq, rec.n_nodes, tols), f"tolerance set {tols} is not admitted: fused and unfused tol decide differently"
    out = []
    for b, seq in enumerate(rec.seq):
        if rec.singular[b]:
            out.append((SINGULAR, 0, None))
            continue
        k, _ = predict(seq, rec.n_nodes, tols)
        assert k is not None, f"instance {b}: no recorded iteration is accepted under {tols}"
        out.append((0, k, k) if k <= cap else (NO_CONV, 0, cap))
    return out


# ---- the recorder ---------------------------------------------------------------------------------------------------------------------------
def factory(deck, batch, knobs, overrides=None):
    """-> make(max_newton, tols, residual_tol): a fresh engine, loaded and reset"""
    def make(max_newton=0, tols=None, residual_tol=-1.0):
        e = F.Engine()
        e.set_options(g_min=0.0, max_newton=max_newton, residual_tol=residual_tol, **(tols or {}))
        for k, v in knobs.items():
            e.set_knob(k, v)
        e.load_deck(deck, batch, overrides)
        e.reset()
        return e
    make.n_nodes, make.rows, make.batch = deck.n_nodes, deck.rows, batch
    return make


class Analysis:
    """one solve point: OP / DC / TROP, or one TR step of dt; from reset(), from a checkpoint blob, from a set iterate"""

    def __init__(self, kind, dt=None, blob=None, start=None):
        self.kind, self.dt, self.blob, self.start = kind, dt, blob, start

    def prepare(self, e):
        if self.blob is not None:
            e.restore(self.blob)
        if self.start is not None:
            e.set_solution(self.start)

    def run(self, e):
        if self.kind == "TR":
            return e.analyze_tr(self.dt, 1, check=False)["rc"]
        return e.analyze_dc(MODES[self.kind], check=False)["rc"]


class Recording:
    pass


def record(make, ana, K=24):
    B = make.batch

    def capped(k):
        e = make(max_newton=k, tols=OFF)
        ana.prepare(e)
        x0 = e.solution()
        ana.run(e)
        x, st = e.solution(), e.state()["status"].copy()
        e.close()
        return x0, x, st

    xs, done_at = [], [None] * B
    sing = np.zeros(B, dtype=bool)
    for k in range(1, K + 1):
        x0, x, st = capped(k)
        if k == 1:
            xs.append(x0)
            assert same_bits(capped(1)[1], x), "record: the cap-1 run is not reproducible"
        assert all(s in (0, NO_CONV, SINGULAR) for s in st), f"record: statuses {sorted(set(st.tolist()))} at cap {k}"
        for b in range(B):
            if done_at[b] is not None:      # x_k of a run with a larger cap, where it can be observed: the instance stopped at done_at[b]
                assert st[b] == (SINGULAR if sing[b] else 0) and same_bits(x[b], xs[done_at[b]][b]), f"record: instance {b} stopped at cap {done_at[b]}, differs at cap {k}"
            elif st[b] != NO_CONV:
                done_at[b] = k
                sing[b] = st[b] == SINGULAR
        xs.append(x)
        if all(d is not None for d in done_at):
            assert same_bits(capped(k)[1], x), f"record: the cap-{k} run is not reproducible"
            break
    else:
        # (a circuit of many cells need not come to a step of exactly 0 everywhere: some cell may alternate between two neighbouring
        #  doubles for ever.  The recording then ends at K, and predict_all refuses a tolerance set that accepts nothing up to there.)
        assert same_bits(capped(K)[1], x), f"record: the cap-{K} run is not reproducible"
    rec = Recording()
    rec.seq = np.array(xs).transpose(1, 0, 2).copy()      # [B][K + 1][rows]
    rec.singular, rec.n_nodes, rec.K = sing, make.n_nodes, len(xs) - 1
    for b in range(B):
        if not sing[b] and done_at[b] is not None:
            assert same_bits(rec.seq[b, -1], rec.seq[b, done_at[b]]) and same_bits(rec.seq[b, done_at[b]], rec.seq[b, done_at[b] - 1]), f"record: instance {b} did not stop on a zero step"
    return rec


# ---- decks ----------------------------------------------------------------------------------------------------------------------------------
class CellDeck:
    """N independent cells VDC - R (1 kOhm) - D (the diode of deck.diode_op()); cap > 0: a capacitor across each diode.  Cell i takes the
    node rows 2 i and 2 i + 1 -- the diode's node first if i is in diode_first, else the source's node first -- and branch row 2 N + i."""

    def __init__(self, N, cap=0.0, diode_first=()):
        d = pe.deck.Deck()
        self.N, self.node_row, self.src_row = N, [], []
        for i in range(N):
            n1, n2 = d.new_node(), d.new_node()
            a, dn = (n2, n1) if i in diode_first else (n1, n2)
            d.add("VDC", (a, 0), 0.0)
            d.add("R", (a, dn), 1000.0)
            d.add("D", (dn, 0))
            if cap > 0.0:
                d.add("C", (dn, 0), cap)
            self.node_row.append(dn - 1)
            self.src_row.append(a - 1)
        br = branch_rows(d)
        self.branch_row = [br[i] for i, (kind, _, _) in enumerate(d.devices) if kind == "VDC"]
        assert d.rows == 3 * N and self.branch_row == list(range(2 * N, 3 * N))
        self.deck = d

    def overrides(self, volts, r=None):
        """volts [B][N] -> the VDC table (and the R table if r [B][N] is given)"""
        ov = {"VDC": np.asarray(volts, dtype=float)[:, :, None]}
        if r is not None:
            ov["R"] = np.asarray(r, dtype=float)[:, :, None]
        return ov


def check_rows_from_matrix(e, cd):
    """the row numbering the checks rely on, read back from the stamp: a source's branch row holds its incidence entry in its node's column"""
    rp, ci, va, rhs = e.matrix(0)
    for i in (0, cd.N // 2, cd.N - 1):
        k = cd.branch_row[i]
        cols = ci[rp[k]:rp[k + 1]].tolist()
        assert cd.src_row[i] in cols, f"cell {i}: branch row {k} has columns {cols}, its source node is row {cd.src_row[i]}"
        cols = ci[rp[cd.node_row[i]]:rp[cd.node_row[i] + 1]].tolist()
        assert cd.src_row[i] in cols and cd.node_row[i] in cols, f"cell {i}: diode row {cd.node_row[i]} has columns {cols}"


# ---- running the engine under a tolerance set and comparing it with the prediction ---------------------------------------------------------
def run_and_compare(make, ana, rec, tols, cap=0, what="", residual_tol=-1.0, iters_before=None):
    """a fresh engine under `tols` (and max_newton = cap): status, iters and solution of every instance against predict over rec; the
    trace entry is instance 0's; the return code the first failing instance's status.  Returns the per-instance counts."""
    want = predict_all(rec, tols, cap or 64)
    e = make(max_newton=cap, tols=tols, residual_tol=residual_tol)
    ana.prepare(e)
    rc = ana.run(e)
    st = e.state()
    x = e.solution()
    tr = e.newton_trace()
    net = e.safety_net()
    e.close()
    first_fail = next((s for s, _, _ in want if s != 0), 0)
    assert rc == first_fail, f"{what}: return code {rc}, the first failing instance's status is {first_fail}"
    for b, (s, k, hold) in enumerate(want):
        w = f"{what}, instance {b}"
        assert st["status"][b] == s, f"{w}: status {st['status'][b]}, predicted {s}"
        assert st["iters"][b] == k + (0 if iters_before is None else iters_before[b]), f"{w}: iters {st['iters'][b]}, predicted {k}"
        if hold is not None:
            assert same_bits(x[b], rec.seq[b, hold]), f"{w}: the solution is not bitwise the recorded iterate {hold} (max |diff| {np.nanmax(np.abs(x[b] - rec.seq[b, hold])):.3g})"
    s0, k0, _ = want[0]
    assert len(tr) == 1 and tr[0] == (k0 if s0 == 0 else s0), f"{what}: newton_trace {tr.tolist()}, predicted {(k0 if s0 == 0 else s0)}"
    if residual_tol >= 0.0:
        assert net == {"refined": 0, "rematched": 0, "careful": False}, f"{what}: safety net {net}"
    return [k if s == 0 else s for s, k, _ in want]


def report(label, what, **figures):
    print(f"NEWTON {label} {what}: " + ", ".join(f"{k} {v}" for k, v in figures.items()))


# ---- 1. the inclusive edge, per row class ----------------------------------------------------------------------------------------------------
def pinned(cls, atol):
    """the tolerance set that lets only the absolute term of one class decide: the other class's atol is 1.0 (no step of these decks
    exceeds it), both rtol are 1e-300"""
    return dict(v_abstol=atol if cls == "node" else 1.0, i_abstol=atol if cls == "branch" else 1.0, v_reltol=TINY, i_reltol=TINY)


def edge_pairs(rec, b, row, cls):
    """pairs (j, j2, delta): predict gives j with atol = delta = |x_j - x_(j-1)| of `row` and a later j2 with nextafter(delta, 0); at the
    lower value `row` is the only violating row of iteration j.  The steps are not monotone: searched."""
    seq, out = rec.seq[b], []
    for j in range(1, rec.K + 1):
        delta = abs(float(seq[j, row]) - float(seq[j - 1, row]))
        if not delta > 0.0:
            continue
        lower = float(np.nextafter(delta, 0.0))
        k_hi, _ = predict(seq, rec.n_nodes, pinned(cls, delta))
        k_lo, earlier = predict(seq, rec.n_nodes, pinned(cls, lower))
        if k_hi == j and k_lo is not None and k_lo > j and earlier[j - 1].tolist() == [row]:
            out.append((j, k_lo, delta))
    return out


def check_edges(knobs, label=""):
    """one driven cell (1.0 V) among WRAP_CELLS at 0 V; a warm start on x_6 of the cold sequence adds a decreasing tail"""
    n = WRAP_CELLS
    cd = CellDeck(n)
    c = n // 2
    v = np.zeros((1, n))
    v[0, c] = 1.0
    make = factory(cd.deck, 1, knobs, cd.overrides(v))
    e = make(max_newton=1)
    e.analyze_dc(F.MODE_OP, check=False)
    check_rows_from_matrix(e, cd)
    e.close()
    cold = record(make, Analysis("OP"))
    others = np.delete(cold.seq[0], [cd.node_row[c], cd.branch_row[c], cd.src_row[c]], axis=1)
    assert not others.any(), "the rows of the cells at 0 V move"
    runs = [("cold", Analysis("OP"), cold)]
    if cold.K >= 7:
        warm = Analysis("OP", start=cold.seq[:, 6])
        runs.append(("warm", warm, record(make, warm)))
    count = {}
    for cls, row in (("node", cd.node_row[c]), ("branch", cd.branch_row[c])):
        js = set()
        for name, ana, rec in runs:
            for j, j2, delta in edge_pairs(rec, 0, row, cls):
                for atol, want in ((delta, j), (float(np.nextafter(delta, 0.0)), j2)):
                    got = run_and_compare(make, ana, rec, pinned(cls, atol), what=f"{label} edge {cls} {name} j = {j}, atol {atol!r}")
                    assert got == [want], (got, want)
                js.add((name, j))
        assert len({j for _, j in js}) >= 2, f"{label}: fewer than two different pinned iterations for the {cls} rows: {sorted(js)}"
        count[cls] = len(js)
    report(label, "edges", node=count["node"], branch=count["branch"], iterations=cold.K)
    return count


# ---- 2. every thread position decides -------------------------------------------------------------------------------------------------------
def wanted_rows(n):
    nn = 2 * n
    node = sorted({0, 63, 64, PE_THREADS - 1, PE_THREADS, 255, 256, 767, 768, nn - 1})
    return [p for p in node if p < nn], [nn, 3 * n - 1]


def check_positions(knobs, label="", every_cell=False):
    """instance b drives cell c_b alone: under the node pin its deciding row is that cell's diode node, under the branch pin its source's
    branch row.  The cells are chosen (and their two nodes ordered) so that the deciding rows are row 0, the last row, n_nodes - 1 and
    n_nodes, 63 / 64, PE_THREADS - 1 / PE_THREADS, 255 / 256 and 767 / 768.  every_cell: one instance per cell, so that every row decides
    for some instance -- k_m2_finish takes row col_src[k] at thread position k, and the permutation is not visible through the API: with
    every row deciding, every thread position does, whatever the permutation."""
    n = WRAP_CELLS
    node_rows, branch_rows_ = wanted_rows(n)
    cd = CellDeck(n, diode_first={p // 2 for p in node_rows if p % 2 == 0})
    cells = list(range(n)) if every_cell else sorted({p // 2 for p in node_rows} | {k - 2 * n for k in branch_rows_})
    for p in node_rows:
        assert cd.node_row[p // 2] == p, f"row {p} is not the diode node of cell {p // 2}"
    for k in branch_rows_:
        assert cd.branch_row[k - 2 * n] == k and (k - 2 * n) in cells
    B = len(cells)
    v = np.zeros((B, n))
    v[np.arange(B), cells] = 1.0
    make = factory(cd.deck, B, knobs, cd.overrides(v))
    e = make(max_newton=1)
    e.analyze_dc(F.MODE_OP, check=False)
    check_rows_from_matrix(e, cd)
    info = e.info()
    e.close()
    ana = Analysis("OP")
    rec = record(make, ana)
    reached = {}
    for cls, rows in (("node", cd.node_row), ("branch", cd.branch_row)):
        pairs = edge_pairs(rec, 0, rows[cells[0]], cls)
        assert pairs, f"{label}: no pinned pair for the {cls} rows"
        j, j2, delta = pairs[0]
        for b, c in enumerate(cells):      # one tolerance pins every instance: the cells are equal, their steps must be (bitwise)
            mine = [p for p in edge_pairs(rec, b, rows[c], cls) if p[0] == j]
            assert mine and mine[0] == (j, j2, delta), f"{label}: instance {b} (cell {c}) has the pair {mine}, instance 0 {(j, j2, delta)}"
        for atol, want in ((delta, j), (float(np.nextafter(delta, 0.0)), j2)):
            got = run_and_compare(make, ana, rec, pinned(cls, atol), what=f"{label} positions {cls} atol {atol!r}")
            assert got == [want] * B, (got, want)
        reached[cls] = sorted(rows[c] for c in cells)
    for p in node_rows:
        assert p in reached["node"]
    for k in branch_rows_:
        assert k in reached["branch"]
    report(label, "positions", instances=B, node_rows=len(reached["node"]), branch_rows=len(reached["branch"]),
           wanted="/".join(str(p) for p in node_rows + branch_rows_), ew_grid=info["ew_grid"], n_wavefronts=info["n_wavefronts"])
    return reached, info


# ---- 3. the relative term -------------------------------------------------------------------------------------------------------------------
def _flip(seq, n_nodes, tols_of, j, lo, hi):
    """the smallest double rtol in (lo, hi] at which predict gives j (the decision of the deciding row is monotone in rtol)"""
    assert predict(seq, n_nodes, tols_of(hi))[0] == j and predict(seq, n_nodes, tols_of(lo))[0] != j
    while float(np.nextafter(lo, math.inf)) < hi:
        mid = lo + (hi - lo) / 2.0
        if predict(seq, n_nodes, tols_of(mid))[0] == j:
            hi = mid
        else:
            lo = mid
    return lo, hi


def check_relative(knobs, label=""):
    """atol = 1e-300, rtol pinned by bisection on predict to the double at which the decision flips, at an iteration where |x| and |xprev| of
    the deciding row differ by more than 10 %: a min for the max, or |x| alone, predicts another iteration there (asserted).  In the cold
    sequence of the 1.0 V cell the 0.31 V step sits behind smaller relative steps, which a relative tolerance of its size accepts first; so
    the cell is driven with 0.3 V and started above its operating point (diode node on 0.56 .. 0.62 V, below the limiter's threshold):
    the first iteration then takes the node down by more than a tenth, and it is that iteration the pinned rtol decides.  Searched, not
    assumed."""
    n = 8
    cd = CellDeck(n)
    c = 3
    v = np.zeros((1, n))
    v[0, c] = 0.3
    make = factory(cd.deck, 1, knobs, cd.overrides(v))
    starts = [None]
    for vd in (0.6, 0.58, 0.56, 0.62):
        x0 = np.zeros((1, cd.deck.rows))
        x0[0, cd.node_row[c]], x0[0, cd.src_row[c]], x0[0, cd.branch_row[c]] = vd, 0.3, 0.5 * (vd - 0.3) / 1000.0
        starts.append(x0)
    done = {}
    for cls, row in (("node", cd.node_row[c]), ("branch", cd.branch_row[c])):
        def tols_of(rt, cls=cls):
            if cls == "node":
                return dict(v_abstol=TINY, v_reltol=rt, i_abstol=1.0, i_reltol=TINY)
            return dict(v_abstol=1.0, v_reltol=TINY, i_abstol=TINY, i_reltol=rt)
        found = None
        for s, x0 in enumerate(starts):
            ana = Analysis("OP", start=x0)
            rec = record(make, ana)
            seq = rec.seq[0]
            for j in range(1, rec.K + 1):
                a, b = abs(float(seq[j, row])), abs(float(seq[j - 1, row]))
                d = abs(float(seq[j, row]) - float(seq[j - 1, row]))
                if not (d > 0.0 and min(a, b) < 0.9 * max(a, b) and min(a, b) > 0.0):
                    continue
                q = d / max(a, b)
                if predict(seq, rec.n_nodes, tols_of(2.0 * q))[0] != j or predict(seq, rec.n_nodes, tols_of(0.5 * q))[0] in (j, None):
                    continue
                lo, hi = _flip(seq, rec.n_nodes, tols_of, j, 0.5 * q, 2.0 * q)
                if predict(seq, rec.n_nodes, tols_of(hi), pick=np.minimum)[0] == j or predict(seq, rec.n_nodes, tols_of(hi), which="x")[0] == j:
                    continue      # (|x| alone differs from the max only where |xprev| is the larger one)
                found = (s, ana, rec, j, lo, hi)
                break
            if found:
                break
        assert found, f"{label}: no iteration with a relative step of more than 10 % decides for the {cls} rows"
        s, ana, rec, j, lo, hi = found
        seq = rec.seq[0]
        # a planted min, or |x| alone, predicts another iteration than the max at the accepting value
        assert predict(seq, rec.n_nodes, tols_of(hi), pick=np.minimum)[0] != j and predict(seq, rec.n_nodes, tols_of(hi), which="x")[0] != j
        for rt, accept in ((hi, True), (lo, False)):
            got = run_and_compare(make, ana, rec, tols_of(rt), what=f"{label} relative {cls} rtol {rt!r}")
            assert (got == [j]) == accept, (got, j, accept)
        if cls == "branch":
            # i_reltol = 0 follows v_reltol: the branch rows must follow the pinned v_reltol (v_abstol = 1.0 lets every node row pass)
            for rt, accept in ((hi, True), (lo, False)):
                follow = dict(v_abstol=1.0, v_reltol=rt, i_abstol=TINY, i_reltol=0.0)
                if accept:
                    assert predict(seq, rec.n_nodes, dict(follow, i_reltol=1e-3))[0] != j, "an i_reltol defaulting to 1e-3 would predict the same iteration"
                got = run_and_compare(make, ana, rec, follow, what=f"{label} relative: i_reltol follows v_reltol {rt!r}")
                assert (got == [j]) == accept, (got, j, accept)
        done[cls] = (s, j, hi)
    report(label, "relative", **{k: f"start {s} iteration {j} rtol {hi!r}" for k, (s, j, hi) in done.items()})
    return done


# ---- 4. mixed tolerances on a busy circuit (and 6, 10) ---------------------------------------------------------------------------------------
TOL_SETS = {
    "defaults": {},
    "loose absolute": dict(v_abstol=1e-3, v_reltol=TINY, i_abstol=1e-6, i_reltol=TINY),
    "tight relative": dict(v_abstol=TINY, v_reltol=1e-9, i_abstol=TINY, i_reltol=1e-6),
    "mixed": dict(v_abstol=1e-9, v_reltol=1e-2, i_abstol=1e-15, i_reltol=1e-5),
    "very loose": dict(v_abstol=1e-2, v_reltol=0.25, i_abstol=1e-4, i_reltol=0.25),
}


def busy(n, B, seed=5, lo=0.2, hi=1.2):
    """every cell driven: VDC spread over lo .. hi, a different permutation per instance"""
    base = lo + (hi - lo) * pe.deck.uniform01(seed, n)
    v = np.zeros((B, n))
    for b in range(B):
        v[b] = base[np.argsort(pe.deck.uniform01(seed + 100 + b, n))]
    return v


def check_busy(knobs, label="", modes=("OP", "DC", "TROP"), residual_tol=-1.0):
    n, B = WRAP_CELLS, 3
    cd = CellDeck(n)
    make = factory(cd.deck, B, knobs, cd.overrides(busy(n, B)))
    counts, n_admitted = set(), {}
    for mode in modes:
        ana = Analysis(mode)
        rec = record(make, ana)
        ok = [name for name, tols in TOL_SETS.items() if admitted(rec.seq, rec.n_nodes, tols)]
        n_admitted[mode] = len(ok)
        assert "defaults" in ok and len(ok) >= 4, f"{label} {mode}: only {ok} are admitted by the fused / unfused rule"
        for name in ok:
            counts |= set(run_and_compare(make, ana, rec, TOL_SETS[name], what=f"{label} busy {mode} {name}", residual_tol=residual_tol))
    assert len(counts) >= 3, f"{label}: accepted iteration counts {sorted(counts)}: fewer than three distinct ones"
    report(label, "busy" + (" with the residual check" if residual_tol >= 0.0 else ""), counts="/".join(map(str, sorted(counts))),
           admitted="/".join(f"{m} {k} of {len(TOL_SETS)}" for m, k in n_admitted.items()))
    return counts, n_admitted


# ---- 6. max_newton edges ----------------------------------------------------------------------------------------------------------------------
def linear_deck_one_iteration(knobs, label, start=None):
    d = pe.deck.divider_dc()
    make = factory(d, 1, knobs)
    e = make(max_newton=1, tols=OFF)
    if start is not None:
        e.set_solution(start)
    rc = e.analyze_dc(F.MODE_DC, check=False)["rc"]
    st, x, tr = e.state(), e.solution(), e.newton_trace()
    e.close()
    assert rc == 0 and st["status"][0] == 0 and st["iters"][0] == 1 and tr.tolist() == [1], f"{label}: linear deck: rc {rc}, state {st}, trace {tr}"
    return x


def check_cap(knobs, label=""):
    n = WRAP_CELLS
    cd = CellDeck(n)
    make = factory(cd.deck, 1, knobs, cd.overrides(busy(n, 1)))
    ana = Analysis("OP")
    rec = record(make, ana)
    k = predict_all(rec, {})[0][1]
    assert k >= 3
    assert run_and_compare(make, ana, rec, {}, cap=k, what=f"{label} cap = count") == [k]
    assert run_and_compare(make, ana, rec, {}, cap=k - 1, what=f"{label} cap = count - 1") == [NO_CONV]
    # the failed solve leaves iters where they were: the same engine converges first (iters = k), then fails from that state
    e = make(max_newton=k)
    assert ana.run(e) == 0
    it0 = e.state()["iters"].copy()
    e.set_options(g_min=0.0, max_newton=1, residual_tol=-1.0, **OFF)
    e.set_solution(rec.seq[:, 0])
    assert ana.run(e) == NO_CONV
    st = e.state()
    e.close()
    assert st["status"][0] == NO_CONV and np.array_equal(st["iters"], it0) and it0[0] == k, (st, it0)
    x = linear_deck_one_iteration(knobs, label)
    assert np.allclose(x[0], [2.0, 3.0, -0.1], rtol=1e-12, atol=0.0), x      # 3 V over 10 + 20 Ohm
    report(label, "cap", count=k)
    return k


# ---- 7. NaN is a violation, not a pass --------------------------------------------------------------------------------------------------------
def check_nan(knobs, label=""):
    n = WRAP_CELLS
    cd = CellDeck(n, diode_first={n - 1})      # row 0 and the last node row are sources' nodes: no device reads them
    assert cd.src_row[0] == 0 and cd.src_row[n - 1] == 2 * n - 1
    make = factory(cd.deck, 1, knobs, cd.overrides(np.full((1, n), 0.3)))
    tols = dict(v_abstol=1e3, i_abstol=1e3, v_reltol=TINY, i_reltol=TINY)
    clean = record(make, Analysis("OP"))
    assert run_and_compare(make, Analysis("OP"), clean, tols, what=f"{label} NaN: clean start") == [1]
    for row in (0, 2 * n - 1):
        x0 = np.zeros((1, cd.deck.rows))
        x0[0, row] = np.nan
        ana = Analysis("OP", start=x0)
        rec = record(make, ana)
        assert np.isnan(rec.seq[0, 0, row]) and np.isfinite(rec.seq[0, 1:]).all()
        assert same_bits(rec.seq[0, 1:clean.K + 1], clean.seq[0, 1:]), "the NaN start changed the iterates"
        assert run_and_compare(make, ana, rec, tols, what=f"{label} NaN at row {row}") == [2]
    x = linear_deck_one_iteration(knobs, label)
    xn = linear_deck_one_iteration(knobs, label, start=np.full((1, 3), np.nan))
    assert same_bits(x, xn) and np.isfinite(x).all(), (x, xn)
    report(label, "NaN", rows=f"0/{2 * n - 1}")


# ---- 5. instances retire independently ------------------------------------------------------------------------------------------------------
def spread(n, B, seed=9):
    """every cell driven, instance b up to a voltage of its own (0.3 .. 1.2 V): the instances need different iteration counts"""
    top = 0.3 + 0.9 * pe.deck.uniform01(seed, B)
    v = busy(n, B, seed + 1, 0.0, 1.0)
    return 0.2 + (top[:, None] - 0.2) * v


def check_retire(knobs, label="", n=64, B=65, singular=20, solo=True):
    """max_newton on the median predicted count: some instances converge, the others end as ERR_NO_CONVERGENCE on their cap-th iterate;
    one instance has a series resistor of 0 Ohm (a non-finite entry: ERR_SINGULAR).  Every converged instance against its solo run."""
    cd = CellDeck(n)
    v = spread(n, B)
    r = np.full((B, n), 1000.0)
    if singular is not None:
        r[singular, 5] = 0.0
    make = factory(cd.deck, B, knobs, cd.overrides(v, r))
    ana = Analysis("OP")
    rec = record(make, ana)
    assert rec.singular.tolist() == [b == singular for b in range(B)], np.nonzero(rec.singular)[0]
    counts = [k for s, k, _ in predict_all(rec, {}) if s == 0]
    cap = int(np.median(counts))
    assert min(counts) <= cap < max(counts), (min(counts), cap, max(counts))
    got = run_and_compare(make, ana, rec, {}, cap=cap, what=f"{label} retire batch {B}")
    n_conv = sum(1 for g in got if g > 0)
    assert n_conv and NO_CONV in got and len({g for g in got if g > 0}) >= 2, got
    if solo:
        for b, g in enumerate(got):
            if g <= 0:
                continue
            m1 = factory(cd.deck, 1, knobs, cd.overrides(v[b:b + 1], r[b:b + 1]))
            e = m1(max_newton=cap)
            rc = ana.run(e)
            x, it = e.solution(), e.state()["iters"]
            e.close()
            assert rc == 0 and it[0] == g and same_bits(x[0], rec.seq[b, g]), f"{label}: instance {b} alone: rc {rc}, {it[0]} iterations (batch: {g}), bitwise {same_bits(x[0], rec.seq[b, g])}"
    report(label, f"retire batch {B}", cap=cap, converged=n_conv, no_convergence=got.count(NO_CONV), singular=got.count(SINGULAR),
           counts="/".join(map(str, sorted({g for g in got if g > 0}))))
    return got


# ---- 8. transient ---------------------------------------------------------------------------------------------------------------------------
TR_DT = 2.0 ** -20


def check_transient(knobs, label="", residual_tol=-1.0):
    """cells with a capacitor (1 nF: R C = 1 us beside the step of 2^-20 s), batch 3, three steps from reset() without TROP.  Each step's
    sequence is recorded from the checkpoint before it (taken from an engine that steps under the tolerance set of the check), then one
    uninterrupted analyze_tr(dt, 3), and once more with probes armed (the PROBES instantiation of the resident kernel)."""
    n, B = WRAP_CELLS, 3
    cd = CellDeck(n, cap=1e-9)
    make = factory(cd.deck, B, knobs, cd.overrides(busy(n, B, seed=13)))
    tols = TOL_SETS["mixed"]
    E = make(tols=tols, residual_tol=residual_tol)
    ks, rec = [], None
    for s in range(3):
        ana = Analysis("TR", dt=TR_DT, blob=E.checkpoint())
        rec = record(make, ana)
        want = predict_all(rec, tols)
        assert all(st == 0 for st, _, _ in want)
        ks.append([k for _, k, _ in want])
        assert E.analyze_tr(TR_DT, 1, check=False)["rc"] == 0
        x = E.solution()
        for b in range(B):
            assert same_bits(x[b], rec.seq[b, ks[-1][b]]), f"{label} TR step {s}, instance {b}: not the predicted iterate {ks[-1][b]}"
    assert E.newton_trace().tolist() == [k[0] for k in ks], (E.newton_trace(), ks)
    E.close()
    ks = np.array(ks)
    last = np.array([rec.seq[b, ks[2][b]] for b in range(B)])
    probe_rows = [cd.node_row[0], cd.node_row[n - 1], cd.branch_row[n // 2]]
    for probes in (False, True):
        e = make(tols=tols, residual_tol=residual_tol)
        if probes:
            e.set_probes(probe_rows, capacity=4)
            e.arm_probes()
        rc = e.analyze_tr(TR_DT, 3, check=False)["rc"]
        st, x, tr, net = e.state(), e.solution(), e.newton_trace(), e.safety_net()
        w = f"{label} TR uninterrupted" + (" with probes" if probes else "")
        assert rc == 0 and not st["status"].any() and np.all(st["steps"] == 3), f"{w}: rc {rc}, {st}"
        assert tr.tolist() == ks[:, 0].tolist(), f"{w}: trace {tr.tolist()}, predicted {ks[:, 0].tolist()}"
        assert st["iters"].tolist() == ks.sum(axis=0).tolist(), f"{w}: iters {st['iters'].tolist()}, predicted {ks.sum(axis=0).tolist()}"
        assert same_bits(x, last), f"{w}: the solution is not the predicted iterate of step 3"
        if probes:
            t, val, n_rec, n_drop = e.probe_samples()
            assert n_rec.tolist() == [4] * B and not n_drop.any(), (n_rec, n_drop)      # the armed state, then the three accepted steps
            assert same_bits(val[:, 3, :], x[:, probe_rows]) and np.all(t[:, 3] == st["t"]), f"{w}: the last sample is not the solution"
        if residual_tol >= 0.0:
            assert net == {"refined": 0, "rematched": 0, "careful": False}, f"{w}: safety net {net}"
        e.close()
    report(label, "transient" + (" with the residual check" if residual_tol >= 0.0 else ""), counts="/".join(map(str, sorted(set(ks.ravel().tolist())))),
           per_step=" ".join(",".join(map(str, k)) for k in ks.tolist()))
    return ks


# ---- 9. derived engines inherit the options ---------------------------------------------------------------------------------------------------
def check_sweep(knobs, label=""):
    n = 8
    cd = CellDeck(n)
    base = np.full((1, n), 0.2)      # (the other cells stay low, so that the swept cell sets the count)
    values = [0.25, 0.45, 0.65, 0.85, 1.05, 1.2]
    recs = []
    for val in values:
        v = base.copy()
        v[0, 0] = val
        make = factory(cd.deck, 1, knobs, cd.overrides(v))
        recs.append((make, record(make, Analysis("OP"))))
    per_set = {}
    for name in ("defaults", "very loose"):
        tols = TOL_SETS[name]
        single = [run_and_compare(make, Analysis("OP"), rec, tols, what=f"{label} sweep point {p} alone, {name}")[0] for p, (make, rec) in enumerate(recs)]
        e = factory(cd.deck, 1, knobs, cd.overrides(base))(tols=tols)
        x, status, stats = e.analyze_dc_sweep(values, F.VDC, 0, mode=F.MODE_OP, order=F.DC_SWEEP_PARALLEL, continuation=0, check=False)
        st, iters, seed = e.dc_sweep_status()
        e.close()
        assert stats["rc"] == 0 and not status.any() and not st.any(), (stats, status, st)
        assert iters[:, 0].tolist() == single, f"{label} sweep under {name}: iterations {iters[:, 0].tolist()}, single points (= predict) {single}"
        per_set[name] = single
    assert per_set["defaults"] != per_set["very loose"], per_set
    report(label, "sweep", **{k.replace(" ", "_"): "/".join(map(str, v)) for k, v in per_set.items()})
    return per_set


# ---- 10. no false alarm -----------------------------------------------------------------------------------------------------------------------
def check_no_false_alarm(knobs, label=""):
    """checks 4 and 8 once more with residual_tol at its default: the recordings (made with the check off) predict the same counts and
    bits, and no counter of the safety net moves"""
    check_busy(knobs, label, residual_tol=0.0)
    check_transient(knobs, label, residual_tol=0.0)


def check_batch_384(knobs, label=""):
    """cells(8) at batch 384 (the resident kernels' 128-VGPR build): instance order only"""
    return check_retire(knobs, label, n=8, B=384, singular=None, solo=False)
