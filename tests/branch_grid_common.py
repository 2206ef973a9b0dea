"""Shared by tests/test_gpu_branch_grid.py and tests/test_branch_grid_emu.py: the multifrontal LU on BRANCH-HEAVY circuits.

Every other circuit the suite factors at scale is a node-voltage matrix: symmetric pattern, dominant diagonal, a handful of branch rows,
a row matching (pe_symbolic.cpp match_rows) that is the identity but for two rows.  branch_grid(W) is a W x W grid in which half the
horizontal links are inductors, with VCVS / VCCS / CCCS / CCVS / transformers / op-amp followers sprinkled over it: about 35 % of the
rows are branch rows, the pattern is unsymmetric, at DC (inductors are shorts: a zero diagonal in every inductor row) the matching moves
70 % of the rows, and in a transient step every node row holds a conductance of 1e-3 beside branch-current entries of 1.  The matrices
are healthy -- cond_1 about 6e7, plain SciPy LU without refinement 1e-8 tolerance units from the refined reference, both asserted of
every stamp used (assert_healthy) -- so whatever the product loses on them it loses by its own static choice of pivots.

Two sizes: W = 24 (993 rows: the resident kernels and, under SPLIT = 1, the split schedule) and W = 44 (3 379 rows: the smallest the
policy itself puts on the split schedule with lane-group fronts).

What every run asserts of every instance it solves (judge): (f) NO SILENT ERROR -- a status of OK comes with a solution within tolerance,
a solution outside it with ERR_INACCURATE, ERR_SINGULAR or ERR_NO_CONVERGENCE -- and, these systems being what plain LU solves, that the
instance IS solved: status OK, within tolerance.  Errors are in the project's tolerance units |x - x_ref| / (atol + rtol |x_ref|), LIN for
linear decks against reference_solve (front_shapes_common: SciPy LU + long-double refinement) of the engine's own stamp, NL for decks
with diodes against oracle/pe_oracle.py.

Where the matching is asserted to move at least half of the rows: on the DC stamp, which every run starts from.  A transient stamp has a
usable diagonal (-2 L / dt) in every inductor row; the matching keeps those, moves 14 % of the rows there, all onto pivots that are large
in the scaling of the maximum-product matching, and the runs say so in their output (the greedy augmenting paths this family was found
with moved 51 % and lost nine digits on them)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import front_shapes_common as F
from parity_common import pe

LIN = F.LIN                 # the project's linear tolerance (tests/test_gpu_parity.py)
NL = (1e-6, 1e-5)           # ... and the one for decks with diodes
SEEDS = {24: (1, 2, 3), 44: (1, 2)}
DTS = (1e-9, 1e-10)
FAILED = (pe.ffi.ERR_INACCURATE, pe.ffi.ERR_SINGULAR, pe.ffi.ERR_NO_CONVERGENCE)
SCHEDULES_24 = [{"SPLIT": 0}, {"SPLIT": 1, "GRAPH": 0}, {"SPLIT": 1, "GRAPH": 1}]
IDS_24 = ["resident", "split", "split_graph"]
# W = 44: the default, the wave fronts on the per-instance path (with the two amalgamation knobs of front_shapes_common.check_launch_variants,
# so that the tree stays the one of the lane-group launch geometry) and their backward pass on it
VARIANTS_44 = [{}, {"QUAD": 0, "ABSORB_M": 32, "RELAX_SMALL": 4}, {"QUAD_BACK": 0}]
IDS_44 = ["default", "quad0", "quad_back0"]
# The followers' gain.  At 1e5 the DC stamps have cond_1 = 2.8e9 (W = 24) and 4.1e9 (W = 44): the gain is the largest entry of the matrix
# and carries |A|_1 (row-equilibrated the same matrices are at 1e5) -- above the 1e9 this module requires of its inputs.  At 1e4 they are at
# 2.8e8 and 4.1e8, the transient stamps at 6e7 as before, and the greedy matching loses as many digits as it did at 1e5.
OPAMP_GAIN = 1e4
# what the DC analysis of W = 44 reaches under the default knobs, both seeds (names of front_shapes_common)
CLASSES_44 = ["quad, one row set (m <= 16)", "quad, m = 16", "quad, m = 17", "quad, m = 32", "quad, p = 16", "quad, >= 4 children", "wave, m = 33",
              "wave, m in 36..45", "cooperative, mode 0", "cooperative, mode 1", "cooperative, mode 2", "top fronts"]


def branch_grid(W, seed=1, nonlinear=False):
    def node(i, j):
        return i * W + j + 1

    d = pe.deck.Deck()
    d.n_nodes = W * W
    u = pe.deck.uniform01(seed, 8 * W * W)
    k = 0
    for i in range(W):
        for j in range(W):
            if j + 1 < W:
                if (i + j) % 2 == 0:
                    d.add("L", (node(i, j), node(i, j + 1)), 1e-6 * (1 + u[k]))
                else:
                    d.add("R", (node(i, j), node(i, j + 1)), 1000.0 * (1 + u[k]))
            k += 1
            if i + 1 < W:
                d.add("R", (node(i, j), node(i + 1, j)), 1000.0 * (1 + u[k]))
            k += 1
            d.add("C", (node(i, j), 0), 1e-12 * (1 + u[k]))
            k += 1
            d.add("R", (node(i, j), 0), 1e5 * (1 + u[k]))
            k += 1
            c = i * W + j
            if c % 37 == 5 and i + 2 < W and j + 2 < W:
                a = d.new_node()
                d.add("VCVS", (a, 0, node(i, j), node(i + 2, j + 2)), 0.5)
                d.add("R", (a, node(i + 1, j)), 2000.0)
            if c % 41 == 7 and i + 3 < W and j + 1 < W:
                d.add("VCCS", (node(i + 3, j), 0, node(i, j), node(i, j + 1)), 1e-4)
            if c % 43 == 9 and i + 2 < W and j + 2 < W:
                a = d.new_node()
                d.add("CCCS", (node(i + 2, j + 2), 0, node(i, j), a), 0.3)
                d.add("R", (a, 0), 700.0)
            if c % 47 == 11 and i + 2 < W and j + 2 < W:
                a = d.new_node()
                b = d.new_node()
                d.add("CCVS", (a, 0, node(i, j), b), 50.0)
                d.add("R", (b, 0), 900.0)
                d.add("R", (a, node(i + 2, j + 1)), 1500.0)
            if c % 53 == 13 and i + 2 < W and j + 2 < W:
                a = d.new_node()
                d.add("XFMR", (node(i, j), 0, a, 0), 2.0)
                d.add("R", (a, node(i + 2, j + 2)), 800.0)
            if c % 59 == 17 and i + 2 < W:
                a = d.new_node()
                d.add("OPAMP", (a, 0, node(i, j), a), OPAMP_GAIN)
                d.add("R", (a, node(i + 2, j)), 1200.0)
            if nonlinear and (i + j) % 8 == 0:
                d.add("D", (node(i, j), 0))
    s = d.new_node()
    d.add("VDC", (s, 0), 1.0)
    d.add("R", (s, node(0, 0)), 50.0)
    d.add("IDC", (node(W - 1, W - 1), 0), 1e-3)
    return d


_DECKS = {}


def deck_of(W, seed, nonlinear=False):
    key = (W, seed, nonlinear)
    if key not in _DECKS:
        _DECKS[key] = branch_grid(W, seed, nonlinear)
    return _DECKS[key]


def value_tables(deck, seed, batch):
    """overrides {"R": [batch][nR][1], "L": [batch][nL][1]}: every resistor and inductor of instance b times a factor in [1, 1.3] of its
    own, drawn like front_shapes_common.resistor_table.  The pivot order is matched on instance 0: the others run on pivots chosen for
    other values."""
    out = {}
    for kind, salt in (("R", 0), ("L", 500)):
        base = np.array([p[0] for k, _, p in deck.devices if k == kind])
        t = np.empty((batch, len(base), 1))
        for b in range(batch):
            t[b, :, 0] = base * (1.0 + 0.3 * pe.deck.uniform01(1000 * seed + salt + b, len(base)))
        out[kind] = t
    return out


def instance_deck(deck, tables, b):
    """the deck of instance b: `deck` with its resistors and inductors at the values of tables (in deck order)"""
    out = pe.deck.Deck()
    out.n_nodes = deck.n_nodes
    it = {k: iter(v[b, :, 0]) for k, v in tables.items()}
    for kind, nodes, par in deck.devices:
        out.add(kind, nodes, *((float(next(it[kind])),) + tuple(par[1:]) if kind in it else par))
    return out


def new_engine(knobs=None, device=0):
    return F.new_engine(knobs, device)


def reached(table):
    """the front classes of front_shapes_common a front table holds, with their counts"""
    return {k: v for k, v in F.class_counts(table).items() if v}


def units(x, x_ref, tol):
    return float(np.max(np.abs(x - x_ref) / (tol[0] + tol[1] * np.abs(x_ref))))


# ---- what a run asserts about its inputs ---------------------------------------------------------------------------------------------
def assert_healthy(A, b, x_ref, what):
    """the input is healthy with the reference alone: plain SciPy LU, no refinement, within 1e-6 tolerance units of reference_solve; a
    1-norm condition estimate (Higham's estimator on SciPy's factors) below 1e9"""
    lu = spla.splu(A.tocsc())
    plain = units(lu.solve(np.asarray(b, dtype=np.float64)), x_ref, LIN)
    inv = spla.LinearOperator(A.shape, matvec=lambda v: lu.solve(np.asarray(v, dtype=np.float64).ravel()),
                              rmatvec=lambda v: lu.solve(np.asarray(v, dtype=np.float64).ravel(), "T"))
    cond = float(abs(A).sum(axis=0).max() * spla.onenormest(inv))
    print(f"{what}: input: plain LU {plain:.3g} tolerance units from the reference, cond_1 estimate {cond:.3g}")
    assert plain <= 1e-6, f"{what}: the input is not healthy: plain LU is {plain} tolerance units from the refined reference"
    assert cond < 1e9, f"{what}: the input is not healthy: cond_1 estimate {cond}"
    return plain, cond


def assert_dc_input(eng, W, what):
    """after the DC analysis: the matching moved at least half of the rows; at W = 24 at least 300 rows of the stamp have a structurally
    zero diagonal; the pattern is not symmetric; at W = 44 the policy chose the split schedule with lane-group fronts and the front table
    holds lane-group, wave, cooperative and top fronts (by name: CLASSES_44)"""
    info = eng.info()
    assert info["n_row_swaps"] >= info["rows"] / 2, f"{what}: the matching moved {info['n_row_swaps']} of {info['rows']} rows"
    A, _ = F.stamped_system(eng, 0)
    P = sp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    has_diag = P.diagonal() != 0
    n_zero = int(np.count_nonzero(~has_diag | (A.diagonal() == 0.0)))
    assert W != 24 or n_zero >= 300, f"{what}: {n_zero} rows with a zero diagonal"
    assert (P != P.T).nnz > 0, f"{what}: the pattern is symmetric"
    counts = reached(eng.front_table())
    if W == 44 and eng.get_knob("QUAD") != 0:
        assert info["n_parts"] > 1 and info["n_quad_fronts"] > 0, info
        F.assert_classes(eng.front_table(), CLASSES_44)
    elif W == 44:
        assert info["n_parts"] > 1 and info["n_quad_fronts"] == 0, info
    print(f"{what}: rows {info['rows']}, row swaps {info['n_row_swaps']}, zero diagonals {n_zero}, parts {info['n_parts']}, "
          f"lane-group fronts {info['n_quad_fronts']}, classes {counts}")
    return info


# ---- the verdict on one instance -----------------------------------------------------------------------------------------------------
def judge(status, err, what):
    """(f) no silent error, then the required outcome: the instance is solved"""
    assert err <= 1.0 or status in FAILED, f"{what}: SILENT ERROR: status {status} with a solution {err:.3g} tolerance units off"
    assert status == 0, f"{what}: given up (status {status}) on a system plain LU solves; the solution left is {err:.3g} tolerance units off"
    assert err <= 1.0, f"{what}: {err:.3g} tolerance units off"


def judge_linear(eng, what):
    """every instance of the engine's last (linear) solve against reference_solve of its own stamp at LIN; returns the worst error"""
    x, status = eng.solution(), eng.state()["status"]
    worst = 0.0
    verdicts = []
    for b in range(eng.batch):
        A, rhs = F.stamped_system(eng, b)
        xr = F.reference_solve(A, rhs)
        assert_healthy(A, rhs, xr, f"{what}, instance {b}")
        err = units(x[b], xr, LIN)
        worst = max(worst, err)
        verdicts.append((int(status[b]), err, f"{what}, instance {b}"))
    print(f"{what}: worst error {worst:.3g} tolerance units, status {status.tolist()}, safety net {eng.safety_net()}")
    for v in verdicts:
        judge(*v)
    return worst


def load(eng, W, seed, batch, nonlinear=False):
    deck = deck_of(W, seed, nonlinear)
    tables = value_tables(deck, seed, batch) if batch > 1 else None
    eng.load_deck(deck, batch=batch, overrides=tables)
    eng.reset()
    return deck, tables


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def check_dc(knobs, W, seed, where=""):
    """(a) DC solve, batches 1 and 5 (R and L of every instance its own): every instance against reference_solve of its own stamp"""
    for batch in (1, 5):
        eng = new_engine(knobs)
        try:
            load(eng, W, seed, batch)
            st = eng.analyze_dc(pe.ffi.MODE_DC, check=False)
            what = f"{where} DC W={W} seed={seed} batch={batch}"
            assert_dc_input(eng, W, what)
            judge_linear(eng, what)
            assert st["rc"] == 0, st
        finally:
            eng.close()


def check_first_step(knobs, W, seed, where=""):
    """(b) one transient step from the DC point at dt = 1e-9 and 1e-10, linear deck: the step's solution against reference_solve of the
    step's own stamp"""
    for dt in DTS:
        eng = new_engine(knobs)
        try:
            load(eng, W, seed, 1)
            eng.analyze_dc(pe.ffi.MODE_DC, check=False)
            what = f"{where} first step W={W} seed={seed} dt={dt:g}"
            assert_dc_input(eng, W, what)
            judge_linear(eng, what + " (DC point)")
            st = eng.analyze_tr(dt, 1, check=False)
            print(f"{what}: rc {st['rc']}, row swaps of the transient analysis {eng.info()['n_row_swaps']}, classes {reached(eng.front_table())}")
            judge_linear(eng, what)
            assert st["rc"] == 0, st
        finally:
            eng.close()


def oracle_run(oracle_mod, deck, dt, steps):
    o = oracle_mod.Oracle(deck)
    assert o.analyze_dc("DC")
    o.analyze_tr(dt, steps)
    return o


def check_four_steps(knobs, W, seed, nonlinear, oracle_mod, batch=1, dt=1e-9, where=""):
    """(c) four transient steps after the DC point against oracle/pe_oracle.py on the same deck (per-instance decks for a batch): LIN for
    the linear deck, NL for the deck with diodes, fail_step == -1 on both sides; the Newton counts of instance 0 beside the oracle's"""
    tol = NL if nonlinear else LIN
    eng = new_engine(knobs)
    try:
        deck, tables = load(eng, W, seed, batch, nonlinear)
        what = f"{where} four steps W={W} seed={seed} batch={batch} {'diodes' if nonlinear else 'linear'}"
        st0 = eng.analyze_dc(pe.ffi.MODE_DC, check=False)
        assert_dc_input(eng, W, what)
        st = eng.analyze_tr(dt, 4, check=False)
        x, status, trace = eng.solution(), eng.state()["status"], eng.newton_trace().tolist()
        worst, verdicts = 0.0, []
        for b in range(batch):
            o = oracle_run(oracle_mod, deck if tables is None else instance_deck(deck, tables, b), dt, 4)
            assert o.fail_step == -1, f"{what}: the oracle fails at step {o.fail_step}"
            err = units(x[b], o.x, tol)
            worst = max(worst, err)
            verdicts.append((int(status[b]), err, f"{what}, instance {b}"))
            if b == 0:
                print(f"{what}: Newton counts {trace}, the oracle's {list(o.newton_iters)}")
        print(f"{what}: worst error {worst:.3g} tolerance units, rc {st0['rc']} / {st['rc']}, status {status.tolist()}, safety net {eng.safety_net()}, "
              f"classes {reached(eng.front_table())}")
        for v in verdicts:
            judge(*v)
        assert st0["rc"] == 0 and st["rc"] == 0, (st0, st)      # (fail_step == -1 on the engine's side)
        return x
    finally:
        eng.close()


def check_static_skip(W, seed, oracle_mod, where=""):
    """(d) STATIC_SKIP 1 against 0 on the deck with diodes, bit for bit: the static-skip row tables (row_keep, row_dyn, wy) are indexed
    through a row permutation that is far from the identity here"""
    out = {}
    for skip in (1, 0):
        eng = new_engine({"STATIC_SKIP": skip})
        try:
            load(eng, W, seed, 5, True)
            eng.analyze_dc(pe.ffi.MODE_DC, check=False)
            rc = eng.analyze_tr(1e-9, 4, check=False)["rc"]
            out[skip] = (eng.solution(), eng.newton_trace().tolist(), eng.state()["status"].tolist(), eng.state()["iters"].tolist(), rc, eng.static_skip_stats())
        finally:
            eng.close()
    print(f"{where} static skip W={W} seed={seed}: {out[1][5]} against {out[0][5]}, Newton counts {out[1][1]}")
    assert out[1][5]["skipped_launches"] > 0 and out[0][5]["skipped_launches"] == 0, (out[1][5], out[0][5])
    assert out[1][1:5] == out[0][1:5], (out[1][1:5], out[0][1:5])
    assert np.array_equal(out[1][0], out[0][0]), f"{np.count_nonzero(out[1][0] != out[0][0])} unknowns differ"
    assert out[1][4] == 0 and not any(out[1][2])
    print("BRANCH GRID OK")


def stamps(W, seed, dt=1e-9):
    """(DC stamp, TR stamp of the first step) of the linear deck as read back from matrix(0): [(A csr, b)]"""
    eng = new_engine()
    try:
        load(eng, W, seed, 1)
        eng.analyze_dc(pe.ffi.MODE_DC, check=False)
        dc = F.stamped_system(eng, 0)
        eng.analyze_tr(dt, 1, check=False)
        tr = F.stamped_system(eng, 0)
    finally:
        eng.close()
    return [dc, tr]


def judge_seam(call, A, b, what):
    """one call of a solver seam: (f) a return of OK comes with the figures of front_shapes_common.check_seam_solution, and it is OK"""
    try:
        x, _ = call()
    except pe.ffi.PeHipError as e:
        assert e.code in FAILED, e
        raise AssertionError(f"{what}: given up ({e}) on a system plain LU solves")
    F.check_seam_solution(A, b, x, what)


def check_seams(W, seed, where=""):
    """(e) the DC stamp and the TR stamp through pe_hip_solve_csr_real (copy_pattern = True, then the cached pattern with the values of
    another seed) and through pe_hip_solve_csr_complex with a random phase on every entry"""
    other = SEEDS[W][(SEEDS[W].index(seed) + 1) % len(SEEDS[W])]
    mine, theirs = stamps(W, seed), stamps(W, other)
    eng = pe.ffi.Engine(device=0)
    try:
        for name, (A, b), (A2, b2) in zip(("DC stamp", "TR stamp"), mine, theirs):
            what = f"{where} seam W={W} seed={seed} {name}"
            assert np.array_equal(A.indptr, A2.indptr) and np.array_equal(A.indices, A2.indices)
            n = A.shape[0]
            assert_healthy(A, b, F.reference_solve(A, b), what)
            judge_seam(lambda: eng.solve_csr(n, A.indptr, A.indices, A.data, b, copy_pattern=True), A, b, what + ", real")
            swaps = pe.ffi.analyze_pattern(n, A.indptr, A.indices, A.data)["n_row_swaps"]
            print(f"{what}: row swaps {swaps}, classes {reached(eng.front_table(1))}")
            judge_seam(lambda: eng.solve_csr(n, A2.indptr, A2.indices, A2.data, b2, copy_pattern=False), A2, b2, what + f", real, cached pattern with the values of seed {other}")
            rng = np.random.default_rng(7)
            Z = sp.csr_matrix((A.data * np.exp(2j * np.pi * rng.uniform(size=A.nnz)), A.indices, A.indptr), shape=A.shape)
            bz = b * np.exp(2j * np.pi * rng.uniform(size=n))
            judge_seam(lambda: eng.solve_csr_complex(n, Z.indptr, Z.indices, Z.data, bz, copy_pattern=True), Z, bz, what + ", complex")
            print(f"{what}, complex: classes {reached(eng.front_table(2))}")
        # A cached pivot order that does not fit the values of the call.  The transient stamp keeps the diagonal -2 L / dt of the inductor
        # rows as their pivots; with the order cached from it, the DC stamp (the same pattern, those diagonals exactly zero) meets zero
        # pivots, and the DC stamp with 1e-13 in their place -- as healthy a matrix -- meets pivots of 1e-13 that no status word reports:
        # without the residual check of the real seam that solution comes back as it is, with a return of OK.
        (Ad, bd), (At, bt) = mine
        n = Ad.shape[0]
        assert np.array_equal(Ad.indptr, At.indptr) and np.array_equal(Ad.indices, At.indices)
        rows = np.repeat(np.arange(n), np.diff(Ad.indptr))
        tiny = Ad.copy()
        tiny.data[(rows == Ad.indices) & (Ad.data == 0.0) & (At.data != 0.0)] = 1e-13
        assert np.count_nonzero(tiny.data != Ad.data) >= n // 4
        for name, M in (("zero", Ad), ("1e-13", tiny)):
            what = f"{where} seam W={W} seed={seed} pivot order of the TR stamp, DC stamp with {name} diagonals"
            assert_healthy(M, bd, F.reference_solve(M, bd), what)
            judge_seam(lambda: eng.solve_csr(n, At.indptr, At.indices, At.data, bt, copy_pattern=True), At, bt, what + " (the TR stamp)")
            judge_seam(lambda: eng.solve_csr(n, M.indptr, M.indices, M.data, bd, copy_pattern=False), M, bd, what)
    finally:
        eng.close()
    print("BRANCH GRID OK")


# ---- circuits' own AC stamps through the complex seam ---------------------------------------------------------------------------------
AC_GOLDENS = ("ac_rc_lowpass", "ac_linear_mix", "ac_nmos_amp", "ac_controlled_rest_acop", "ac_rlc_diode_acop", "ac_transistors_acop", "ac_transistors_hf_acop")
AC_OMEGAS = (0.0,) + tuple(float(w) for w in np.logspace(0.0, 9.0, 28))
AC = (1e-9, 1e-6)           # the tolerance of the AC goldens (tests/test_gpu_parity.py)


def check_ac_stamps(name, oracle_mod, where=""):
    """The complex seam on what the reference hands it: the oracle's AC stamp (stamp_ac, after the operating point where the golden has
    one) of an AC golden's circuit at omega = 0 and 28 frequencies from 1 to 1e9 rad/s, as stamped -- no phases added: the real and
    imaginary parts of a circuit's entries are conductances and susceptances, and blocks of either cancel exactly (two nodes joined by a
    capacitor alone), which a pivot order chosen on the real-equivalent magnitudes row by row runs into.  Every point SciPy's complex LU
    solves has to be solved, within the goldens' tolerance of reference_solve; the others have to be refused."""
    from parity_common import golden
    meta, _, deck = golden(name)
    o = oracle_mod.Oracle(deck, g_min=meta["gmin"], r_open=meta.get("r_open", 0.0))
    assert o.analyze_ac([1.0], acop=meta["analysis"] == "ACOP") is not None
    eng = pe.ffi.Engine(device=0)
    worst, solved = 0.0, 0
    try:
        for w in AC_OMEGAS:
            A, b = o.stamp_ac(w)
            keys = sorted(A)
            Z = sp.csr_matrix((np.array([A[k] for k in keys], dtype=complex), (np.array([k[0] for k in keys]), np.array([k[1] for k in keys]))), shape=(o.rows, o.rows))
            Z.sort_indices()
            what = f"{where} AC stamp of {name} at omega {w:g}"
            try:
                xr = spla.splu(Z.tocsc()).solve(b)
                healthy = bool(np.all(np.isfinite(xr)))
            except RuntimeError:
                healthy = False
            try:
                x, _ = eng.solve_csr_complex(o.rows, Z.indptr, Z.indices, Z.data, b, copy_pattern=True)
            except pe.ffi.PeHipError as e:
                assert e.code in FAILED, e
                assert not healthy, f"{what}: given up ({e}) on a system SciPy's LU solves"
                continue
            if not healthy:      # (accepted by the seam's own residual check: it has to be a solution)
                xr = x
                assert float(np.max(np.abs(Z @ x - b))) <= 1e-9 * max(1.0, float(np.max(np.abs(b)))), what
            err = units(x, F.reference_solve(Z, b) if healthy else xr, AC)
            worst, solved = max(worst, err), solved + 1
            assert err <= 1.0, f"{what}: SILENT ERROR: {err:.3g} tolerance units off with a return of OK"
    finally:
        eng.close()
    print(f"{where} AC stamps of {name}: {solved} of {len(AC_OMEGAS)} points solved, worst error {worst:.3g} tolerance units")
    assert solved >= len(AC_OMEGAS) - 1      # (omega = 0 may be singular: a node held by capacitors alone)
    print("BRANCH GRID OK")


def check_all(knobs, W, seed, oracle_mod, where=""):
    """(a), (b), (c) under one set of knobs"""
    check_dc(knobs, W, seed, where)
    check_first_step(knobs, W, seed, where)
    check_four_steps(knobs, W, seed, False, oracle_mod, batch=3, where=where)
    check_four_steps(knobs, W, seed, True, oracle_mod, batch=1, where=where)
    print("BRANCH GRID OK")
