"""Shared by tests/test_gpu_front_shapes.py and tests/test_front_shapes_emu.py: circuits and matrices whose assembly trees sit ON the
integer limits of the front classes (pe_symbolic.cpp fits_quad: order 32, 16 pivots, 255 own entries, 16 children; the wave slot: order
35 / 45; max_pivots), a high-precision reference, and the check that a run really reached the classes it was written for.

Gadgets.  A CLIQUE of k new nodes (every pair joined by a resistor) tied to one mesh node by one resistor is eliminated as one front of
order k with k - 1 pivots and k * k - 1 own entries of A (k = 16: 16x15 with 255 entries, the last lane-group front; k = 17: 17x16 with
288, the first that is not); a clique of more than wave_p / max_pivots nodes is cut into a chain of links.  A HUB is a 6-node clique with
n 4-node cliques (three new nodes and, round robin, one node of the hub): with absorption and last-child merging limited (knobs
ABSORB_M=8, RELAX_SMALL=1, RELAX_X100=0) its front keeps n children.  A FAN is n rim nodes, not joined to one another, and n / 3 + 2
three-node cliques (blades) each joined to every rim node: a blade node has fewer neighbours than a rim node, so the blades are
eliminated first and leave the rim a clique made of fill alone -- 16 pivots with few own entries, which a clique of A cannot have
(16 x 16 = 256).  The PENDANT is a pair of nodes joined by a resistor and tied to the mesh by one resistor and nothing else: with that
resistor at inf the pair floats and the instance's matrix is singular ([[g, -g], [-g, g]]).  Every clique, hub and fan carries a current
source and a resistor to ground, so that its unknowns are not just copies of the mesh node's.

Where a gadget hangs on the mesh decides how the nested dissection cuts around it, and with that whether its fronts end up inside a
wave subtree (a 16-node clique under a cooperative parent is still 16x15, one cut through it is not): the sites below (origin, step)
were chosen so that every class of DEFAULT_CLASSES and KNOB_CLASSES is reached, and assert_classes() fails the tests by name of the
missing class if a change of the analysis moves them.  The pendant's site is chosen the same way: its far node is a leaf front of its
own (1 pivot, 1 update row, 3 own entries, no child -- no other front looks like that) and the node whose pivot becomes zero is a pivot
of that leaf's parent; pendant_fronts() finds both and the tests require both to be lane-group fronts."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import parity_common
from parity_common import pe

LIN = (1e-9, 1e-7)          # the project's linear tolerance (tests/test_gpu_parity.py)
MESH = 56                   # 56 x 56 nodes + source node + source branch = 3 138 rows: the split schedule (rows >= 3 000)
CLIQUES = (15, 16, 17, 31, 32, 33)
CHAIN_CLIQUE = 104          # links 104x25 (panels + pull), 79x7 and 72x32 (chain links: order > 69, the largest whole front in the
                            # 4 952-double LDS share of the sweep geometry), 40x16 ... (whole); 70 nodes give layouts 1 and 0 only
HUBS = (16, 15, 17, 18)
FANS = (16,)
PENDANT_SITE = (47, 30)     # mesh (row, column) the pendant hangs on: both of its fronts are lane-group fronts there (pendant_fronts)
KNOBS_MANY_CHILDREN = {"ABSORB_M": 8, "RELAX_SMALL": 1, "RELAX_X100": 0}
SEED_SEAM = 1


def _clique(d, nodes, r=1000.0):
    for i, a in enumerate(nodes):
        for b in nodes[i + 1:]:
            d.add("R", (a, b), r)


def _feed(d, nodes):
    """a current into the first node, a path to ground from the last: the gadget's unknowns differ from one another"""
    d.add("IDC", (nodes[0], 0), 1e-3)
    d.add("R", (nodes[-1], 0), 2000.0)


def gadget_mesh(seed=1, cliques=CLIQUES, chain=CHAIN_CLIQUE, hubs=HUBS, fans=FANS, pendant=True, mesh=MESH, origin=(3, 4), step=9, pendant_site=PENDANT_SITE):
    """(deck, index of the pendant's tie resistor among the deck's resistors -- the row of an overrides["R"] table)"""
    d = pe.deck.rc_mesh(mesh, mesh, seed, False)
    # every gadget on a mesh node of its own, spread over the grid (away from the borders and from one another)
    per_row = (mesh - origin[1] + step - 1) // step
    sites = [(origin[0] + step * (k // per_row)) * mesh + (origin[1] + step * (k % per_row)) + 1 for k in range(len(cliques) + len(hubs) + len(fans) + 2)]
    assert max(sites) <= mesh * mesh
    site = iter(sites)

    def new(n):
        return [d.new_node() for _ in range(n)]

    for k in tuple(cliques) + ((chain,) if chain else ()):
        nodes = new(k)
        _clique(d, nodes)
        d.add("R", (nodes[0], next(site)), 1000.0)
        _feed(d, nodes[1:])
    for n_children in hubs:
        hub = new(6)
        _clique(d, hub)
        d.add("R", (hub[0], next(site)), 1000.0)
        _feed(d, hub[1:])
        for c in range(n_children):
            child = [hub[1 + c % 5]] + new(3)
            _clique(d, child)
            d.add("R", (child[3], 0), 5000.0)
    for n_rim in fans:
        rim = new(n_rim)
        for _ in range(n_rim // 3 + 2):
            blade = new(3)
            _clique(d, blade)
            for a in rim:
                for c in blade:
                    d.add("R", (a, c), 1000.0)
        d.add("R", (rim[0], next(site)), 1000.0)
        _feed(d, rim[1:])
    tie = -1
    if pendant:
        a, b = new(2)
        d.add("R", (a, b), 1000.0)
        d.add("R", (a, pendant_site[0] * mesh + pendant_site[1] + 1 if pendant_site else next(site)), 1000.0)
        tie = d.count("R") - 1
    return d, tie


def resistor_table(deck, seed, batch, repeat=None):
    """overrides["R"] [batch][nR][1]: every resistor of instance b times a factor in [1, 1.3] drawn from (seed, b); repeat = {b: b0}
    gives instance b the values of instance b0"""
    base = np.array([p[0] for k, _, p in deck.devices if k == "R"])
    r = np.empty((batch, len(base), 1))
    for b in range(batch):
        r[b, :, 0] = base * (1.0 + 0.3 * pe.deck.uniform01(1000 * seed + b, len(base)))
    for b, b0 in (repeat or {}).items():
        r[b] = r[b0]
    return r


def instance_deck(deck, r_values):
    """the deck of one instance: `deck` with its resistors at r_values (in deck order)"""
    return parity_common.instance_deck(deck, {"R": np.asarray(r_values, dtype=float).reshape(1, -1, 1)}, 0)


# ---- reference ------------------------------------------------------------------------------------------------------------------------
LD = np.longdouble
_SPLIT = LD(2) ** ((np.finfo(LD).nmant + 2) // 2) + LD(1)   # Veltkamp's constant for the long-double mantissa (2^32 + 1 on x86)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker), in long double"""
    p = a * b
    ca, cb = _SPLIT * a, _SPLIT * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _real_equivalent(A, *vectors):
    """[[Ar, -Ai], [Ai, Ar]] and [re; im] of every vector: a complex system as a real one of twice the order"""
    A = A.tocsr()
    out = [sp.bmat([[A.real, -A.imag], [A.imag, A.real]], format="csr")]
    for v in vectors:
        v = np.asarray(v)
        out.append(np.concatenate([v.real, v.imag]))
    return out


def _residual_real(A, b, x, x_lo=None):
    """b - A (x + x_lo) of a real CSR system in long double.  SciPy has no long-double matvec: an explicit pass over the CSR arrays, one
    step per position inside a row for all rows at once, every product a x split exactly into two long doubles and every row sum
    carried with its rounding error (a compensated sum) -- the result is good to far below one long-double ulp of the largest term,
    which the refinement needs: it is A^-1 times this error that the corrections cannot go below.  Measured on the gadget mesh
    (|x|_inf = 1.88, so the stopping rule of reference_solve is 1.9e-17): with plain long-double products and row sums the corrections
    of rounds 2 .. 8 wander between 1.6e-17 and 9.3e-17 and the rule is met by chance or not at all; with this pass they fall below
    it in the third round.  Do not simplify it away."""
    A = A.tocsr()
    n = A.shape[0]
    a, xj = A.data.astype(LD), np.asarray(x).astype(LD)[A.indices]
    xl = None if x_lo is None else np.asarray(x_lo).astype(LD)[A.indices]
    acc, comp = np.asarray(b).astype(LD).copy(), np.zeros(n, dtype=LD)
    length = np.diff(A.indptr)
    for k in range(int(length.max()) if n else 0):
        rows = np.flatnonzero(length > k)
        e = A.indptr[rows] + k
        p, pe_ = _two_prod(a[e], xj[e])
        s, se = _two_sum(acc[rows], -p)
        acc[rows] = s
        comp[rows] += se - pe_
        if xl is not None:
            comp[rows] -= a[e] * xl[e]
    return acc + comp


def residual_ld(A, x, b):
    """b - A x in long double (complex systems: in real-equivalent form, returned complex)"""
    if any(np.iscomplexobj(v) for v in (A.data, x, b)):
        A2, x2, b2 = _real_equivalent(A, x, b)
        r = _residual_real(A2, b2, x2)
        return r[:A.shape[0]] + 1j * r[A.shape[0]:]
    return _residual_real(A, b, x)


def reference_solve(A, b, rounds=5):
    """SciPy's sparse LU + iterative refinement: residuals in long double (above), the solution carried as an unevaluated sum of two
    long doubles, until a correction is below 1e-17 |x|_inf -- asserted to happen within `rounds` rounds.  Returns x in long double
    (complex long double for a complex system, which is solved in real-equivalent form).  Raises RuntimeError (SciPy's) for an exactly
    singular matrix."""
    n = A.shape[0]
    cplx = np.iscomplexobj(A.data) or np.iscomplexobj(b)
    if cplx:
        A, b = _real_equivalent(A, b)
    A = A.tocsr()
    lu = spla.splu(A.tocsc())
    x, x_lo = lu.solve(np.asarray(b, dtype=np.float64)).astype(LD), np.zeros(A.shape[0], dtype=LD)
    converged = False
    for _ in range(rounds):
        dx = lu.solve(_residual_real(A, b, x, x_lo).astype(np.float64)).astype(LD)
        x, x_lo = _two_sum(x, x_lo + dx)
        if np.max(np.abs(dx)) <= 1e-17 * np.max(np.abs(x)):
            converged = True
            break
    assert converged, f"reference_solve: refinement still corrects by {float(np.max(np.abs(dx))):.3g} after {rounds} rounds"
    return x[:n] + 1j * x[n:] if cplx else x


def check_solution(A, b, x, x_ref=None, tol=LIN, what=""):
    """x against the reference at abs tol[0] + rel tol[1], and |A x - b|_inf <= 1e-12 max(1, |b|_inf) in long double
    (the bound of test_full_size_properties); returns (error in tolerance units, residual)"""
    x_ref = reference_solve(A, b) if x_ref is None else x_ref
    err = float(np.max(np.abs(x - x_ref) / (tol[0] + tol[1] * np.abs(x_ref))))
    res = float(np.max(np.abs(residual_ld(A, x, b))))
    print(f"{what}: error {err:.3g} tolerance units, residual {res:.3g}")
    assert err <= 1.0, f"{what}: {err} tolerance units from the reference"
    assert res <= 1e-12 * max(1.0, float(np.max(np.abs(b)))), f"{what}: residual {res}"
    return err, res


def stamped_system(eng, b):
    rp, ci, va, rhs = eng.matrix(b)
    return sp.csr_matrix((va, ci, rp), shape=(eng.rows, eng.rows)), rhs


# ---- classes --------------------------------------------------------------------------------------------------------------------------
def _classes(t):
    m = t["p"] + t["u"]
    quad, wave = t["quad"] == 1, (t["kind"] == 0) & (t["quad"] == 0)
    coop = t["kind"] == 1
    return {
        "quad, one row set (m <= 16)": quad & (m <= 16),
        "quad, m = 16": quad & (m == 16),
        "quad, m = 17": quad & (m == 17),
        "quad, m = 32": quad & (m == 32),
        "quad, p = 16": quad & (t["p"] == 16),
        "quad, 255 own entries": quad & (t["n_own"] == 255),
        "quad, >= 4 children": quad & (t["n_children"] >= 4),
        "quad, 16 children": quad & (t["n_children"] == 16),
        "wave, > 255 own entries with m <= 32": wave & (t["n_own"] > 255) & (m <= 32),
        "wave, m = 33": wave & (m == 33),
        "wave, m in 36..45": wave & (m >= 36) & (m <= 45),
        "wave, >= 17 children": wave & (t["n_children"] >= 17),
        "wave, p = 20": wave & (t["p"] == 20),
        "cooperative, p > 20": coop & (t["p"] > 20),
        "cooperative, mode 0": coop & (t["mode"] == 0),
        "cooperative, mode 1": coop & (t["mode"] == 1),
        "cooperative, mode 2": coop & (t["mode"] == 2),
        "top fronts": t["kind"] == 2,
        # reported, never required
        "mode 3 (chain link continued in LDS)": t["mode"] == 3,
        "top, mode 0": (t["kind"] == 2) & (t["mode"] == 0),
        "top, mode 1": (t["kind"] == 2) & (t["mode"] == 1),
        "top, mode 2": (t["kind"] == 2) & (t["mode"] == 2),
    }


DEFAULT_CLASSES = ["quad, one row set (m <= 16)", "quad, m = 16", "quad, m = 17", "quad, m = 32", "quad, p = 16", "quad, 255 own entries",
                   "quad, >= 4 children", "wave, > 255 own entries with m <= 32", "wave, m = 33", "wave, m in 36..45", "cooperative, mode 0",
                   "cooperative, mode 1", "cooperative, mode 2", "top fronts"]
KNOB_CLASSES = ["quad, 16 children", "wave, >= 17 children"]
SEAM_CLASSES = ["wave, p = 20", "cooperative, p > 20", "cooperative, mode 0", "cooperative, mode 1", "cooperative, mode 2"]


def pendant_fronts(table):
    """(leaf, parent): the front that eliminates the pendant's far node -- the only childless front with 1 pivot, 1 update row and 3
    own entries (the node's diagonal and its two couplings) -- and its parent, which by the definition of the assembly tree holds that
    update row, the pendant's near node, as a pivot: the pivot that is exactly zero when the tie resistor is inf"""
    leaf = np.flatnonzero((table["n_children"] == 0) & (table["p"] == 1) & (table["u"] == 1) & (table["n_own"] == 3))
    assert len(leaf) == 1, f"the pendant's leaf front is not unique in the front table: {leaf}"
    parent = int(table["parent"][leaf[0]])
    assert parent >= 0
    return int(leaf[0]), parent


def assert_pendant_in_quad(table):
    """the bad pivot of test (e) sits in a front of the lane-group kernel (and so does the leaf below it)"""
    leaf, parent = pendant_fronts(table)
    m = table["p"] + table["u"]
    assert table["quad"][leaf] == 1 and table["quad"][parent] == 1, (
        f"the pendant's fronts are not lane-group fronts: leaf {leaf} quad {table['quad'][leaf]}, parent {parent} "
        f"({m[parent]}x{table['p'][parent]}, kind {table['kind'][parent]}, quad {table['quad'][parent]})")
    return leaf, parent


def assert_no_wave_front_above(table, wave_p):
    """every front with more than wave_p pivots sits outside the wave class"""
    bad = np.flatnonzero((table["kind"] == 0) & (table["p"] > wave_p))
    assert len(bad) == 0, f"wave fronts with more than {wave_p} pivots: {[(int(s), int(table['p'][s])) for s in bad]}"


def class_counts(table):
    return {k: int(np.count_nonzero(v)) for k, v in _classes(table).items()}


def assert_classes(table, required):
    """fails with the list of the required classes the front table does not contain (and the counts of all of them)"""
    counts = class_counts(table)
    missing = [k for k in required if counts[k] == 0]
    assert not missing, f"front classes not reached: {missing}; reached: {counts}"
    return counts


# ---- matrices for the solver seams (resident kernel: wave_m 56, wave_p 20, max_pivots 48) -------------------------------------------------
SEAM_SIZES = {"chain200": (20, 21, 22, 48, 49, 50, 56, 57, 58, 200), "chain100": (20, 21, 22, 48, 49, 50, 56, 57, 58, 100)}
# Real seam: chain200 is the run that is there for the layouts (all classes).  chain100 on the real seam is there for the pivot limits and
# the copy_pattern=False solve on a second pattern, not for the layouts: all of its fronts fit the LDS whole (modes 1 and 2 are required
# of chain200 on the real seam and of chain100 on the complex seam, whose real-equivalent system has twice the order).
SEAM_REQUIRED = {"chain200": SEAM_CLASSES, "chain100": SEAM_CLASSES[:3]}
SEAM_WAVE_P = 20
_SEAM = None


def seam_patterns(seed=SEED_SEAM):
    """{name: (A csr real, b)}: dense diagonal blocks (cliques) chained by single couplings, sized around wave_p (20 / 21), wave_m
    (56 / 57) and max_pivots (48 / 49), one block large enough for a chain of links whose first ones no longer fit the LDS whole -- order
    200 for the real seam, 100 for the complex one (its real-equivalent system has twice the order) --, and six rows with a structurally
    zero diagonal coupled pairwise to rows of the first block (the pattern of voltage-source branches: the row matching has to move
    them).  Values: every off-diagonal drawn on its own (unsymmetric), the diagonal >= the row's absolute sum except in those rows."""
    global _SEAM
    if _SEAM is not None and seed == SEED_SEAM:
        return _SEAM
    out = {}
    for name, sizes in SEAM_SIZES.items():
        rng = np.random.default_rng(100 * seed + len(out))
        n_zero = 6
        n = sum(sizes) + n_zero
        M = np.zeros((n, n))
        pat = np.zeros((n, n), dtype=bool)
        o, prev = 0, -1
        for k in sizes:
            pat[o:o + k, o:o + k] = True
            if prev >= 0:
                pat[prev, o] = pat[o, prev] = True
            prev = o + k - 1
            o += k
        for z in range(n_zero):      # row o + z: like a source branch on node 3 z of the first block
            pat[o + z, 3 * z] = pat[3 * z, o + z] = True
        M[pat] = rng.uniform(-1.0, 1.0, int(pat.sum()))
        np.fill_diagonal(M, 0.0)
        dom = np.abs(M).sum(axis=1) + rng.uniform(0.1, 1.0, n)
        for i in range(o):
            M[i, i] = dom[i]
        A = sp.csr_matrix(M)
        A.sort_indices()
        assert A.nnz == int(pat.sum()) and not pat[o:, o:].any()      # (no drawn value is exactly zero; the last rows have no diagonal entry)
        out[name] = (A, rng.standard_normal(n))
    if seed == SEED_SEAM:
        _SEAM = out
    return out


def check_seam_solution(A, b, x, what):
    """the figures of test_solve_csr_real_seam / test_solve_csr_complex_seam: |x - x_ref|_inf <= 1e-9 max(1, |x_ref|_inf), residual <= 1e-12 max(1, |b|_inf)"""
    xr = reference_solve(A, b)
    err, res = float(np.max(np.abs(x - xr))), float(np.max(np.abs(residual_ld(A, x, b))))
    print(f"{what}: error {err:.3g} (|x_ref| {float(np.max(np.abs(xr))):.3g}), residual {res:.3g} (|b| {float(np.max(np.abs(b))):.3g})")
    assert err <= 1e-9 * max(1.0, float(np.max(np.abs(xr)))), f"{what}: error {err}"
    assert res <= 1e-12 * max(1.0, float(np.max(np.abs(b)))), f"{what}: residual {res}"


def check_real_seam(eng, name):
    """pe_hip_solve_csr_real on a seam pattern, then on the cached pattern with every row's values scaled by -1 / 2 alternately"""
    A, b = seam_patterns()[name]
    n = A.shape[0]
    x, _ = eng.solve_csr(n, A.indptr, A.indices, A.data, b, copy_pattern=True)
    counts = assert_classes(eng.front_table(1), SEAM_REQUIRED[name])
    assert_no_wave_front_above(eng.front_table(1), SEAM_WAVE_P)
    print(f"real seam {name}: {counts}")
    check_seam_solution(A, b, x, f"real seam {name}")
    A2 = sp.csr_matrix(sp.diags(np.where(np.arange(n) % 2 == 0, -1.0, 2.0)) @ A)
    A2.sort_indices()
    assert np.array_equal(A2.indices, A.indices) and np.array_equal(A2.indptr, A.indptr)
    x2, _ = eng.solve_csr(n, A2.indptr, A2.indices, A2.data, b, copy_pattern=False)
    check_seam_solution(A2, b, x2, f"real seam {name}, cached pattern")


def check_complex_seam(eng, name):
    """pe_hip_solve_csr_complex on the same pattern with a random phase on every entry"""
    A, b = seam_patterns()[name]
    rng = np.random.default_rng(7)
    Z = sp.csr_matrix((A.data * np.exp(2j * np.pi * rng.uniform(size=A.nnz)), A.indices, A.indptr), shape=A.shape)
    bz = b * np.exp(2j * np.pi * rng.uniform(size=len(b)))
    x, _ = eng.solve_csr_complex(Z.shape[0], Z.indptr, Z.indices, Z.data, bz, copy_pattern=True)
    counts = assert_classes(eng.front_table(2), SEAM_CLASSES)
    assert_no_wave_front_above(eng.front_table(2), SEAM_WAVE_P)
    print(f"complex seam {name}: {counts}")
    check_seam_solution(Z, bz, x, f"complex seam {name}")
    try:
        eng.front_table(1)
        raise AssertionError("front_table(1) without an analysis of the real seam must be refused")
    except pe.ffi.PeHipError as e:
        assert e.code == pe.ffi.ERR_ARG


# ---- the checks (run on the device by tests/test_gpu_front_shapes.py, on the host emulation by tests/test_front_shapes_emu.py) ----------
SEED = 1
_DECK = None


def deck_and_tie():
    global _DECK
    if _DECK is None:
        _DECK = gadget_mesh(SEED)
    return _DECK


def new_engine(knobs=None, device=0):
    """a fresh engine under the launch geometry of the 1 024-instance sweep (split schedule, lane-group kernel), g_min = 0"""
    eng = pe.ffi.Engine(device=device)
    eng.set_options(g_min=0.0)
    eng.set_knob("GEOMETRY_BATCH", 1024)
    for k, v in (knobs or {}).items():
        eng.set_knob(k, v)
    return eng


def solve_dc(eng, r, check=True):
    """one linear DC solve of the gadget mesh with the resistor table r [batch][nR][1]: one stamp, one factorisation, one forward / backward pass"""
    deck, _ = deck_and_tie()
    eng.load_deck(deck, batch=len(r), overrides={"R": r})
    eng.reset()
    return eng.analyze_dc(pe.ffi.MODE_DC, check=check)


def check_instances(eng, instances, what):
    x = eng.solution()
    for b in instances:
        A, rhs = stamped_system(eng, b)
        check_solution(A, rhs, x[b], what=f"{what}, instance {b}")
    return x


def check_parity(eng, batch, required=DEFAULT_CLASSES, what="parity"):
    """(a) / (b): every instance of a batch with distinct values against the reference; the class table"""
    deck, _ = deck_and_tie()
    st = solve_dc(eng, resistor_table(deck, SEED, batch))
    info = eng.info()
    assert st["rc"] == 0 and info["rows"] >= 3000 and info["n_parts"] > 1 and info["n_wavefronts"] == 4 and info["n_quad_fronts"] > 0, (st, info)
    counts = assert_classes(eng.front_table(), required)
    print(f"{what}, batch {batch}: {counts}")
    check_instances(eng, range(batch), f"{what}, batch {batch}")
    return counts


def check_slot_independence(eng):
    """(c): the values of instance 0 again in instances 3 (another lane group), 4 (the next quad) and 6 (the last live slot of a partial
    quad) of a batch of 7: the four solutions are bitwise equal"""
    deck, _ = deck_and_tie()
    solve_dc(eng, resistor_table(deck, SEED, 7, repeat={3: 0, 4: 0, 6: 0}))
    assert eng.info()["n_quad_fronts"] > 0
    assert_classes(eng.front_table(), DEFAULT_CLASSES)
    x = check_instances(eng, range(7), "slot independence")
    for b in (3, 4, 6):
        assert np.array_equal(x[b], x[0]), f"instance {b} differs from instance 0 in {np.count_nonzero(x[b] != x[0])} unknowns"
    assert not np.array_equal(x[1], x[0])


def check_one_bad_instance(eng):
    """(e): the pendant's tie resistor at inf in ONE instance of a batch of 6 -- slot 1 of the first quad, slot 3 of it, slot 1 of the
    second, partial quad: that instance alone reports ERR_SINGULAR, the other five are right; then the healthy values on the same engine.
    The front whose pivot is exactly zero is asserted to be a lane-group front (assert_pendant_in_quad)."""
    deck, tie = deck_and_tie()
    healthy = resistor_table(deck, SEED, 6)
    for bad in (1, 3, 5):
        r = healthy.copy()
        r[bad, tie, 0] = np.inf
        st = solve_dc(eng, r, check=False)
        want = [pe.ffi.ERR_SINGULAR if b == bad else 0 for b in range(6)]
        assert st["rc"] != 0 and list(eng.state()["status"]) == want, (bad, st, eng.state()["status"])
        assert eng.info()["n_quad_fronts"] > 0
        assert_classes(eng.front_table(), DEFAULT_CLASSES)
        assert_pendant_in_quad(eng.front_table())      # the zero pivot is met by the lane-group kernel, in one slot of a quad
        A, _ = stamped_system(eng, bad)
        try:     # the input is what it claims: SciPy refuses that instance's matrix
            spla.splu(A.tocsc())
            raise AssertionError(f"instance {bad}: SciPy factors the matrix that should be singular")
        except RuntimeError as e:
            assert "singular" in str(e)
        check_instances(eng, [b for b in range(6) if b != bad], f"bad instance {bad}")
    st = solve_dc(eng, healthy)      # the failure is not sticky: the flag word is cleared
    assert st["rc"] == 0 and list(eng.state()["status"]) == [0] * 6
    assert_pendant_in_quad(eng.front_table())
    check_instances(eng, range(6), "healthy again")


def check_launch_variants(make_engine=new_engine):
    """(d): QUAD=0 (the wave fronts on the per-instance path) and QUAD_BACK=0 (their backward pass on it), per-engine knobs, one engine
    after the other: the solutions of a batch of 5 equal the default's bit for bit (the lane-group kernel keeps the
    operation order of the per-instance path).  With the lane-group kernel on, the launch geometry of >= 192 instances amalgamates up
    to order 32 and forces last-child merges up to 4 pivots (pe_engine_policy.cpp symbolic_options); QUAD=0 alone would fall back to
    35 / 8 and factor ANOTHER tree, so the QUAD=0 engine is given those two values: the assembly trees are asserted identical, only the
    kernel that runs the wave fronts differs."""
    deck, _ = deck_and_tie()
    r = resistor_table(deck, SEED, 5)
    out, tree = {}, {}
    for name, knobs in (("default", {}), ("QUAD=0", {"QUAD": 0, "ABSORB_M": 32, "RELAX_SMALL": 4}), ("QUAD_BACK=0", {"QUAD_BACK": 0})):
        eng = make_engine(knobs)
        try:
            st = solve_dc(eng, r)
            nq = eng.info()["n_quad_fronts"]
            assert st["rc"] == 0 and eng.info()["n_parts"] > 1
            assert (nq == 0) if name == "QUAD=0" else (nq > 0), (name, nq)
            out[name] = eng.solution().copy()
            tree[name] = eng.front_table()
        finally:
            eng.close()
    assert_classes(tree["default"], DEFAULT_CLASSES)
    for name in ("QUAD=0", "QUAD_BACK=0"):
        for k in ("p", "u", "parent", "kind", "mode", "n_children", "n_own"):
            assert np.array_equal(tree[name][k], tree["default"][k]), f"{name}: another assembly tree ({k})"
        assert np.array_equal(out[name], out["default"]), f"{name}: {np.count_nonzero(out[name] != out['default'])} unknowns differ from the default's"


def check_transient_step(eng, oracle_mod):
    """(f): two transient steps after the DC solve of a batch of 5 (a second symbolic class, new factors, the same fronts) against the
    oracle on the per-instance decks"""
    deck, _ = deck_and_tie()
    r = resistor_table(deck, SEED, 5)
    solve_dc(eng, r)
    st = eng.analyze_tr(1e-10, 2)
    assert st["rc"] == 0 and eng.info()["n_quad_fronts"] > 0
    assert_classes(eng.front_table(), DEFAULT_CLASSES)
    x = eng.solution()
    for b in range(5):
        o = oracle_mod.Oracle(instance_deck(deck, r[b]))
        assert o.analyze_dc("DC")
        o.analyze_tr(1e-10, 2)
        assert o.fail_step == -1
        err = float(np.max(np.abs(x[b] - o.x) / (LIN[0] + LIN[1] * np.abs(o.x))))
        print(f"transient step, instance {b}: error {err:.3g} tolerance units")
        assert err <= 1.0, f"instance {b}: {err} tolerance units from the oracle"
