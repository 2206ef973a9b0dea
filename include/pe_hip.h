/* pe_hip.h -- C ABI of the MI355X-native transient engine (libpe_hip.so).
 *
 * This is the drop-in boundary behind Phy-Engine's solver seam.  Plain pointers and sizes only; every
 * function returns 0 on success and a negative pe_hip_status otherwise; no exception crosses the boundary;
 * a handle is thread-compatible (one thread at a time), distinct handles are independent.
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   include/phy_engine/circuits/solver/cuda_sparse_lu.h:465-473   cuda_sparse_lu::solve_csr_real(...)
 *        -> pe_hip_solve_csr_real()             (same arguments, host pointers, caller-owned)
 *   include/phy_engine/circuits/solver/cuda_sparse_lu.h:295-312   cuda_sparse_lu::solve_csr / solve_csr_timed on std::complex<double>
 *        -> pe_hip_solve_csr_complex()          (same arguments; the complex arrays as interleaved doubles)
 *   include/phy_engine/circuits/solver/cuda_sparse_lu.h:27-34     struct timings
 *        -> pe_hip_timings
 *   include/phy_engine/circuits/circuit.h:1122-1482               the CUDA branch of circult::solve_once
 *   include/phy_engine/circuits/circuit.h:233-256,363-374,892-985 TR loop / update_tr_step / Newton loop
 *        -> pe_hip_load_circuit() + pe_hip_analyze_tr()/pe_hip_analyze_dc(): the whole per-time-step path
 *           (device stamps, g_min, LU, triangular solves, Newton test, trapezoidal companion update) stays
 *           resident on the GPU; the host only reads node voltages / branch currents back.
 *   include/phy_engine/circuits/circuit.h:63-68,115-121           cuda_solve_policy / cuda_node_threshold
 *        -> pe_hip_device_count() is what `auto_select` consults.
 */
#ifndef PE_HIP_H
#define PE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pe_hip_engine pe_hip_engine; /* opaque */

enum pe_hip_status
{
    PE_HIP_OK = 0,
    PE_HIP_ERR_ARG = -1,       /* bad argument / call order */
    PE_HIP_ERR_NO_DEVICE = -2, /* no HIP device, or the HIP runtime failed */
    PE_HIP_ERR_SINGULAR = -3,  /* zero / non-finite pivot (reference: factorizationIsOk()==false, circuit.h:1517) */
    PE_HIP_ERR_NO_CONVERGENCE = -4, /* Newton exhausted max_iter (reference: solve() returns false, circuit.h:984) */
    PE_HIP_ERR_INTERNAL = -5,
    PE_HIP_ERR_INACCURATE = -6 /* the static-pivot LU left a residual ||Ax - b|| above tolerance that refinement and re-matching could not
                                  repair (the reference pivots partially, Eigen/src/SparseLU/SparseLU.h:464-469); the step is rolled back */
};

/* device kinds of the resident path; parameter columns per device in `params` */
enum pe_hip_kind
{
    PE_HIP_R = 1,    /* nodes a,b        params: r                           (linear/resistance.h:82-110) */
    PE_HIP_C = 2,    /* nodes a,b        params: C                           (linear/capacitor.h:106-155) */
    PE_HIP_L = 3,    /* nodes a,b +branch params: L                          (linear/inductor.h:134-195) */
    PE_HIP_VDC = 4,  /* nodes a,b +branch params: V                          (linear/VDC.h:82-97) */
    PE_HIP_VAC = 5,  /* nodes a,b +branch params: Vp, omega[rad/s], phase[rad] (linear/VAC.h:162-179) */
    PE_HIP_IDC = 6,  /* nodes a,b        params: I                           (linear/IDC.h:84-95) */
    PE_HIP_DIODE = 7,/* nodes a,c        params: Is,N,Isr,Nr,Temp,Ibv,Bv,Bv_set,Area,tt, tt_in_tr
                                                                            (non-linear/PN_junction.h:296-503;
                                                                             tt_in_tr=0 for the diodes of a
                                                                             full_bridge_rectifier, which has no
                                                                             iterate_tr: base.h:248-264) */
    /* ---- the remaining linear stampers.  Four-pin kinds take nodes [count][4], kinds with two
     * branches take branch [count][2]; pins in the reference's pin order. */
    PE_HIP_IAC = 8,    /* nodes a,b           params: Ip, omega[rad/s], phase[rad]  TR/TROP only, nothing in OP/DC (linear/IAC.h:124-160) */
    PE_HIP_VCCS = 9,   /* nodes S,T,P,Q       params: g       I(S->T) = g (vP - vQ)                         (linear/VCCS.h:80-95) */
    PE_HIP_VCVS = 10,  /* nodes S,T,P,Q +1 br params: mu      vS - vT = mu (vP - vQ)                        (linear/VCVS.h:81-102) */
    PE_HIP_CCCS = 11,  /* nodes S,T,P,Q +1 br params: alpha   sense branch P->Q (a short), I(S->T) = alpha i (linear/CCCS.h:81-100) */
    PE_HIP_CCVS = 12,  /* nodes S,T,P,Q +2 br params: r       branches: output k, sense c; vS - vT = r i_c  (linear/CCVS.h:80-106) */
    PE_HIP_OPAMP = 13, /* nodes S,T,P,Q +1 br params: mu      output P,Q driven by mu (vS - vT)             (linear/op_amp.h:64-83) */
    PE_HIP_XFMR = 14,  /* nodes P,Q,S,T +2 br params: n       ideal transformer Vp = n Vs, Is = -n Ip       (linear/transformer.h:67-98) */
    PE_HIP_SWITCH = 15,/* nodes a,b     +1 br params: cut_through (0/1): D = -(cut ? 0 : r_open)            (controller/switch.h:86-103) */
    PE_HIP_VGEN = 16,  /* nodes +,-     +1 br params: type, Vh, Vl, freq[Hz], duty, phase[rad], tr, tf
                                              type 0 sawtooth, 1 square, 2 pulse, 3 triangle; OP/DC/TROP take t = 0
                                              (generator/sawtooth.h:88-107, square.h:93-110, pulse.h:107-141, triangle.h:88-112) */
    PE_HIP_COUPLED_L = 17,/* nodes p1,p2,s1,s2 +2 br params: L1, L2, k  trapezoidal 2x2 Thevenin companion in TR, two
                                              shorts otherwise (linear/coupled_inductors.h:92-115,160-246) */
    /* three-pin non-linear devices: nodes [count][3]; re-linearised every Newton iteration on the device */
    PE_HIP_NMOS = 18,     /* nodes D,G,S  params: Kp, lambda, Vth   Shichman-Hodges level 1 (non-linear/nmosfet.h:84-141) */
    PE_HIP_PMOS = 19,     /* nodes D,G,S  params: Kp, lambda, Vth                          (non-linear/pmosfet.h:84-139) */
    PE_HIP_BJT_NPN = 20,  /* nodes B,C,E  params: Is, N, BetaF, Temp, Area   forward-active Ebers-Moll (non-linear/BJT_NPN.h:100-158) */
    PE_HIP_BJT_PNP = 21,  /* nodes B,C,E  params: Is, N, BetaF, Temp, Area                  (non-linear/BJT_PNP.h:100-158) */
    PE_HIP_RELAY = 22,    /* nodes C+,C-,A,B +1 br  params: Von, Voff   contact A-B closes at v(C+)-v(C-) >= Von, opens at <= Voff (state
                             per instance, re-evaluated at every stamp; open = r_open); counts as non-linear (controller/relay.h:75-105) */
    PE_HIP_XFMR_CT = 23   /* nodes P,Q,S1,CT,S2 [count][5] +3 br (kP, kH1, kH2)  params: n_total = Vp / V(S1-S2)
                                                                                   (linear/transformer_center_tap.h:71-132) */
};
#define PE_HIP_DIODE_NPARAM 11
#define PE_HIP_VGEN_NPARAM 8
#define PE_HIP_KIND_MAX 23

/* analysis modes (phy_engine::analyze_type, circuits/analyze.h:7-16) */
enum pe_hip_mode
{
    PE_HIP_MODE_OP = 0,
    PE_HIP_MODE_DC = 1,
    PE_HIP_MODE_TR = 4,
    PE_HIP_MODE_TROP = 5
};

typedef struct pe_hip_device_table
{
    int kind;             /* pe_hip_kind */
    int count;            /* devices in this table */
    const int* nodes;     /* [count][pins] node ids: 0 = ground, 1..n_nodes, -1 = unconnected pin (pins = 2 .. 5: see pe_hip_kind) */
    const int* branch;    /* [count][branches] global branch index (0-based, after digital drives) for kinds with branch rows, else NULL */
    const double* params; /* [batch][count][ncol] when params_batched, else [count][ncol] (shared by every instance) */
    int params_batched;
} pe_hip_device_table;

/* Newton / environment knobs (phy_engine::environment, circuits/environment/environment.h:7-22; defaults of
 * circuit.h:898-903 apply where a field is <= 0) */
typedef struct pe_hip_options
{
    double v_abstol, v_reltol, i_abstol, i_reltol;
    double g_min;
    int max_newton; /* 0 -> 64 */
    int refactor_every_solve; /* 1 (default): factor on every solve_once like the reference; 0: reuse the factors of a linear circuit while dt is unchanged */
    double r_open; /* contact resistance of an open switch (environment.h r_open; <= 0 -> 1e12, circuit.h:1012) */
    double residual_tol; /* safety net of the static-pivot LU: after every linear solve eta = ||Ax - b||_inf / (||A||_inf ||x||_inf + ||b||_inf)
                            is checked per instance; above this (0 -> 1e-10, < 0 disables the check) the solve is refined with the same
                            factors' order, then re-matched on that instance's values, else PE_HIP_ERR_INACCURATE */
} pe_hip_options;

/* mirrors cuda_sparse_lu::timings (cuda_sparse_lu.h:27-34) */
typedef struct pe_hip_timings
{
    double h2d_ms, solve_ms, d2h_ms, solve_host_ms, total_host_ms, analyze_ms;
} pe_hip_timings;

typedef struct pe_hip_info
{
    int rows, n_nodes, n_branches, batch;
    int nnz_a;
    long long nnz_lu;        /* structural nnz(L)+nnz(U) of this engine's ordering (F of SURVEY.md 8d) */
    long long nnz_lu_stored; /* entries held in the dense front panels (incl. relaxation zeros) */
    int n_fronts, max_front, tree_depth, n_row_swaps;
    double factor_flops;
    long long bytes_per_instance; /* resident HBM bytes per circuit instance */
    int n_r, n_c, n_l, n_v, n_i, n_d;
    int nonlinear;
    int n_parts;      /* > 1: multi-workgroup schedule (one circuit spread over n_parts workgroups + top levels) */
    int n_top_levels; /* launches of the top of the tree in that schedule */
    int n_wavefronts; /* wavefronts per workgroup of the launch geometry chosen for this batch */
    int lds_bytes;    /* dynamic LDS per workgroup */
    long long nnz_lu_stored_top; /* part of nnz_lu_stored held by the fronts of the top levels (split schedule: k_m2_factor_top / k_m2_solve_top) */
    int n_wave_fronts;           /* fronts below the cooperative part of the tree (one wavefront each) ... */
    int n_quad_fronts;           /* ... of which the lane-group kernel k_m2_factor_quads factors (four instances per wavefront); 0: not in use */
    long long nnz_lu_stored_quad; /* part of nnz_lu_stored held by those fronts */
    int mid_top_limit, ew_grid, quad_lds_pad; /* launch-shape knobs MID_TOP / EW_GRID / QUAD_LDS in effect for THIS engine's resident circuit
                                                 (pe_hip_set_knob, else the environment, else the default; 0 = rule of the policy) */
} pe_hip_info;

typedef struct pe_hip_run_stats
{
    long long steps;        /* accepted time points, summed over instances */
    long long newton_iters; /* solve_once-equivalents, summed over instances */
    double gpu_ms;          /* HIP-event time of the kernels of this call, on the engine's stream */
    int n_launches;
    int n_failed;           /* instances that stopped early */
    double dominant_ms;     /* HIP-event time of the launches of the dominant kernel within gpu_ms: the resident kernel itself, or in the
                               split schedule k_m2_factor_parts (k_m2_solve_parts when the factors are reused) */
    int dominant_launches;
} pe_hip_run_stats;

int pe_hip_device_count(void);
int pe_hip_create(int device, pe_hip_engine** out);
void pe_hip_destroy(pe_hip_engine* h);
const char* pe_hip_last_error(pe_hip_engine* h); /* valid until the next call on h; h may be NULL (creation errors) */

/* ---- drop-in for cuda_sparse_lu::solve_csr_real (cuda_sparse_lu.h:465-473): A x = b, CSR, sorted columns.
 * copy_pattern != 0: (re)analyse the pattern; == 0: reuse the cached analysis (same n/nnz/pattern).  Every solve is followed by a
 * residual check on the device (componentwise backward error, as in the complex twin below): a healthy solution is returned as the
 * kernels left it; one above 1e-10 is refined, and a cached pivot order that fails on the values of this call (bad pivot, or still
 * inaccurate) is re-made on them once.  Returns PE_HIP_ERR_SINGULAR / PE_HIP_ERR_INACCURATE where the reference's solver returns false:
 * never PE_HIP_OK with a solution that failed the check. */
int pe_hip_solve_csr_real(pe_hip_engine* h, int n, int nnz, const int* row_ptr, const int* col_ind, const double* values,
                          const double* b, double* x, int copy_pattern, pe_hip_timings* out);

/* ---- drop-in for the complex twin cuda_sparse_lu::solve_csr_timed / solve_csr on std::complex<double> (cuda_sparse_lu.h:295-312), which
 * circult::solve_once calls when the stamped system is not all-real (circuit.h:1332: AC / ACOP).  values_re_im / b_re_im / x_re_im are
 * the arrays of std::complex<double> the reference passes, seen as interleaved (re, im) doubles: 2 nnz, 2 n and 2 n of them.  Solved in
 * real-equivalent form [Ar -Ai; Ai Ar] by the kernels of the real seam + fp64 iterative refinement on the device; copy_pattern as above
 * (a cached pattern keeps its pivot order and is re-analysed once on the current values if a solve with it fails).  Returns
 * PE_HIP_ERR_SINGULAR / PE_HIP_ERR_INACCURATE where the reference's solver returns false. */
int pe_hip_solve_csr_complex(pe_hip_engine* h, int n, int nnz, const int* row_ptr, const int* col_ind, const double* values_re_im,
                             const double* b_re_im, double* x_re_im, int copy_pattern, pe_hip_timings* out);

/* Build id of this library: 16 hex digits of a sha256 over its sources, headers and compile flags (csrc/Makefile).  bench.py prints it and
 * every profile summary under profiles/ carries it, so a figure can be tied to the library that produced it. */
const char* pe_hip_build_id(void);

/* ---- resident path */
int pe_hip_load_circuit(pe_hip_engine* h, int n_nodes, int n_branches, int batch, int n_tables, const pe_hip_device_table* tables);
int pe_hip_set_options(pe_hip_engine* h, const pe_hip_options* opt);
int pe_hip_get_info(pe_hip_engine* h, pe_hip_info* out);
/* The fronts of an analysis the engine holds, in postorder (children before parents), copied from its symbolic tables: read-only, nothing
 * is recomputed.  `which` 0: the resident circuit (after its first analysis), 1: the last analysis of pe_hip_solve_csr_real, 2: that of
 * pe_hip_solve_csr_complex (its real-equivalent 2n system); PE_HIP_ERR_ARG when that analysis does not exist.  Arrays of `capacity` ints
 * (any may be NULL), *n_fronts receives the count -- call with capacity 0 first.  Per front s: pivots[s], updates[s] (order m = pivots +
 * updates), parent[s] (-1: root), kind[s] (0 wave front, 1 cooperative front of a part, 2 top front), quad[s] (1: factored by the lane-group
 * kernel, as counted by pe_hip_info::n_quad_fronts), mode[s] (LDS layout: 0 whole front, 1 pivot panels + pulled Schur tiles, 2 chain link,
 * 3 chain link continued in LDS), n_children[s], n_own[s] (entries of A assembled into the front). */
int pe_hip_get_front_table(pe_hip_engine* h, int which, int capacity, int* pivots, int* updates, int* parent, int* kind, int* quad, int* mode,
                           int* n_children, int* n_own, int* n_fronts);
/* is_static[s] (array of `capacity` ints, same `which` and postorder as pe_hip_get_front_table): 1 = no x-dependent entry or row in the front's whole subtree. */
int pe_hip_get_static_fronts(pe_hip_engine* h, int which, int capacity, int* is_static, int* n_fronts);
/* Launches of the lane-group factor kernel since the circuit was loaded: those that skipped the static fronts (knob STATIC_SKIP, default 1) and the others. */
int pe_hip_get_static_skip_stats(pe_hip_engine* h, long long* skipped_launches, long long* full_launches);
/* Of those launches, the Newton iterations issued after a refinement round of their own solve point, and how many of them skipped (always 0: a refinement ends the skip for its point). */
int pe_hip_get_static_skip_refinement_stats(pe_hip_engine* h, long long* launches_after_refinement, long long* skipped_after_refinement);

/* Tuning knobs of ONE engine: the launch-geometry / symbolic-analysis parameters INTEGRATION.md lists as the PHY_ENGINE_HIP_* environment
 * family (the counterpart of the reference's cuda_policy / cuda_node_threshold members plus its PHY_ENGINE_CUDA_* variables,
 * circuit.h:63-68, benchmark/README.md:11-21), set per engine instead of per process: `name` with or without the PHY_ENGINE_HIP_
 * prefix ("PARTS", "ABSORB_M", "SPLIT", ...).  A knob set here wins over the environment variable of the same name, which wins over the
 * measured default; it takes effect at the next analysis of the resident circuit (the symbolic analysis is redone).  Test-only
 * variables (…_TEST_*, …_FULL_STAMP, …_DUMP_SCHEDULE, …_LDS_BYTES) stay environment-only.
 * Knob "STATIC_SKIP" (default 1): 0 = every Newton iteration factors the static fronts of the lane-group kernel again (bit-identical results). */
int pe_hip_set_knob(pe_hip_engine* h, const char* name, int value);
int pe_hip_get_knob(pe_hip_engine* h, const char* name, int* value, int* is_set); /* what is set (engine, else environment); is_set may be NULL */

/* digital_out of circult (circuit.h:102,509,1015-1022): ideal sources occupying the FIRST `count` branches.
 * Pass the drives before pe_hip_load_circuit() (they are part of the branch numbering).  On a loaded engine the same
 * drive set with new voltages updates in place; a different set invalidates the resident circuit (reload it). */
int pe_hip_set_digital_drives(pe_hip_engine* h, int count, const int* node, const double* volt);

/* ---- Host-stamp overlay: plug-in models WITHOUT a device table.
 * The reference's extension mechanism is the per-model stamp hook (iterate_{dc,tr,op,trop}_define(tag, M&, MNA&[, t]) with the
 * fallback chains of model/model_refs/base.h:216-304, called in the model loop of circult::solve_once, circuit.h:1071-1084).
 * A user model that only has those hooks is evaluated ON THE HOST, once per Newton iteration, into a fixed set of matrix
 * cells / right-hand-side rows discovered once (what mna_keep_pattern_ready does, circuit.h:993-1003); the values are uploaded
 * and ADDED to the device-side stamp.  The hooks read node voltages, so the Newton loop of such a circuit is driven from the
 * host (one callback + one small upload per iteration and instance).  In a batch every group of calls is preceded by
 * PE_HIP_OVERLAY_INSTANCE with the instance index in `mode` (see below) -- small-signal AC included (one PE_HIP_OVERLAY_AC call per instance).
 *   rows / cols / rhs_rows  absolute MNA indices, 0-based: nodes 0 .. n_nodes-1, then branches (mna.h:60-157 G/B/C/D/I/E layout)
 *   representative          |value| per cell for the static pivot matching (the discovery stamp), may be NULL
 *   nonlinear               1: the circuit needs Newton iterations even without a built-in non-linear device
 *   fn(user, event, mode, t, dt, x, a_values, b_values) -> 0 ok, else the analysis fails with PE_HIP_ERR_INTERNAL:
 *     PE_HIP_OVERLAY_STEP     start of a transient step, x = solution of the previous time point, dt = new step (the models'
 *                             step_changed_tr hooks; circult::update_tr_step, circuit.h:363-374); a_values / b_values NULL
 *     PE_HIP_OVERLAY_ITERATE  before the stamp of every Newton iteration, x = current iterate: fill a_values[n_cells] and
 *                             b_values[n_rhs] (mode = pe_hip_mode of the solve, t = time of the point being solved)
 * Call before pe_hip_load_circuit() (the cells are part of the sparsity pattern); n_cells = n_rhs = 0 with fn = NULL removes it. */
#define PE_HIP_OVERLAY_STEP 0
#define PE_HIP_OVERLAY_ITERATE 1
/*     PE_HIP_OVERLAY_CONVERGED  the iterate x has passed the engine's Newton test: the models' check_convergence hooks are consulted
 *                             as circult::solve does (circuit.h:950-963) -- return 0 to accept it, PE_HIP_OVERLAY_VETO to iterate again
 *                             (counts against max_newton like any other iteration); a_values / b_values NULL */
#define PE_HIP_OVERLAY_CONVERGED 2
#define PE_HIP_OVERLAY_VETO 100 /* a RETURN value (of the CONVERGED event only), deliberately unlike every event number and every small error code */
/* COMPATIBILITY NOTE for callbacks written against round 2 (events STEP / ITERATE only): since round 3 every callback of a non-linear
 * circuit also receives PE_HIP_OVERLAY_CONVERGED, every callback of a batch > 1 PE_HIP_OVERLAY_INSTANCE -- both with a_values / b_values
 * NULL -- and PE_HIP_OVERLAY_AC where small-signal analysis is used.  A callback must dispatch on `event` and return 0 for events it does
 * not handle; one that treats "anything but STEP" as ITERATE would write through NULL. */
/*     PE_HIP_OVERLAY_AC       one small-signal point of pe_hip_analyze_ac (the models' iterate_ac hooks, circuit.h:389-431): t carries
 *                             omega, x the operating point; a_values holds 2 n_cells doubles -- the real parts of the cells, then the
 *                             imaginary parts -- and b_values 2 n_rhs likewise */
#define PE_HIP_OVERLAY_AC 3
/*     PE_HIP_OVERLAY_INSTANCE  batch > 1 only, before each of the calls above: they concern instance `mode` of the batch (x, a_values,
 *                             b_values NULL).  Models with state of their own (a junction's last voltage, a companion history) keep one
 *                             copy per instance and switch here; a callback that cannot returns non-zero and the analysis fails. */
#define PE_HIP_OVERLAY_INSTANCE 4
typedef int (*pe_hip_overlay_fn)(void* user, int event, int mode, double t, double dt, const double* x, double* a_values, double* b_values);
int pe_hip_set_overlay(pe_hip_engine* h, int n_cells, const int* rows, const int* cols, const double* representative, int n_rhs, const int* rhs_rows,
                       int nonlinear, pe_hip_overlay_fn fn, void* user);

/* overwrite one parameter column of one device for every instance (values: [batch] if batched else [1]) */
int pe_hip_update_param(pe_hip_engine* h, int kind, int index, int column, const double* values, int batched);

/* tr_duration / last_step of every instance (circuit.h:161-162), e.g. when a netlist is re-loaded mid-simulation */
int pe_hip_set_time(pe_hip_engine* h, double t, double last_step);
int pe_hip_reset(pe_hip_engine* h); /* circult::reset(), circuit.h:446-465: t = 0, x = 0, companion state cleared */

/* one OP / DC / TROP solve (Newton inside), every instance */
int pe_hip_analyze_dc(pe_hip_engine* h, int mode, pe_hip_run_stats* stats);
/* `nsteps` fixed-dt transient steps, every instance: update_tr_step -> t += dt -> Newton(solve_once)  (a step chosen by the engine:
 * pe_hip_analyze_tr_adaptive below) */
int pe_hip_analyze_tr(pe_hip_engine* h, double dt, int nsteps, pe_hip_run_stats* stats);

/* ---- Variable-step transient: from the current time to the ABSOLUTE time t_stop (> t_now) with a step chosen from the local truncation
 * error (LTE) of the trapezoidal rule and cut when Newton fails.  One decision per attempted step, taken on the host from ONE small
 * read-back; the state of a step is snapshotted, rolled back and tested on the device.
 *   Lockstep.  The batch advances with ONE step sequence (the split schedule solves every instance at one time point per launch sequence):
 *   the step is decided by the worst instance, so every instance meets its tolerance, and an instance's result depends -- within that
 *   tolerance -- on its batch-mates.  All instances must sit at the same t (else PE_HIP_ERR_ARG).
 *   An attempted step of size h = min(dt, dt_max, t_bp - t_now), t_bp the next breakpoint or t_stop, is the ordinary step of
 *   pe_hip_analyze_tr(h, 1) (companion update, Newton, residual safety net with its retries); the new time is t_now + h as that step
 *   forms it, and a breakpoint counts as reached when |t - t_bp| <= 4 eps |t_bp|.
 *     - an instance fails, or its candidate is not finite: roll back, dt = h / 8 (outcome 2).  At h <= dt_min the call ends as
 *       pe_hip_analyze_tr does: the step rolled back, the failed instances' status kept, their status returned.
 *     - LTE test, once three accepted points are in the history: err_r = h^3 / 2 |DD3_r| (third divided difference over those points and
 *       the candidate x*), tol_r = trtol (lte_reltol max(|x*_r|, |x_n,r|) + abstol), q = max err_r / tol_r over all rows of all instances.
 *       q > 1 (or not a number) and h > dt_min: roll back, dt = h max(0.1, 0.9 q^(-1/3)) (outcome 1); at dt_min the step is accepted and
 *       counted in n_at_dt_min.  That estimate and the exponent 1/3 are the trapezoidal rule's (error h^3 / 12 times the third derivative).
 *       Under pe_hip_set_tr_method (below) they become: PE_HIP_TR_BE err_r = h^2 |DD2_r| over the last two points and the candidate, exponent
 *       1/2; PE_HIP_TR_GEAR2 err_r = h^3 (1 + rho)^2 / (rho (1 + 2 rho)) |DD3_r| with rho = h / (t2 - t1), exponent 1/3.
 *     - accepted (outcome 0): dt = h min(2, 0.9 q^(-1/3)) if the step was tested, else dt = h.  A step that reached a breakpoint other
 *       than t_stop restarts the history at that point and continues with dt = dt_init.
 *   The history (three previous solutions per instance, device memory of the engine) is empty at the first adaptive call and after
 *   everything that ends a probe window (pe_hip_analyze_dc, _reset, _set_solution, _set_time, _checkpoint_load, _load_circuit) and after
 *   pe_hip_analyze_tr; a call that finds it empty does not count its starting point (it need not lie on the trajectory): its first three
 *   steps are untested.  A second adaptive call continues the history of the first.  The history is not part of a checkpoint.
 *   Probes armed before the call record ACCEPTED steps only; pe_hip_get_newton_trace likewise.
 *   PE_HIP_ERR_ARG, engine unchanged: no circuit, c == NULL, dt_init <= 0, dt_min > dt_max, t_stop <= t_now, a non-finite value, instances at
 *   different t, a host-stamp overlay (its models keep host state that cannot be rolled back).  There is no twin on the multi-device
 *   pe_hip_sweep_* handle (each device would choose its own step sequence). */
typedef struct pe_hip_tr_control {
    double dt_init;        /* first step, and the step after every breakpoint; > 0 */
    double dt_min, dt_max; /* <= 0: dt_init * 1e-9 and (t_stop - t_now) / 50 */
    double lte_reltol, lte_abstol_v, lte_abstol_i; /* <= 0: 1e-3, 1e-6, 1e-9; a NEGATIVE lte_reltol switches the LTE test off */
    double trtol;          /* <= 0: 7 (SPICE's over-estimate factor of the divided-difference LTE) */
    long long max_steps;   /* cap on ATTEMPTED steps of this call; <= 0: none.  Reaching it ends the call with PE_HIP_OK and t_end < t_stop */
    int source_breakpoints;/* 1: corners of SQR / PULSE / SAW / TRI generators whose parameters are shared by the batch are breakpoints
                              (a generator with more than 100 000 periods before t_stop is left to the LTE test) */
    int n_breakpoints; const double* breakpoints; /* further absolute times, any order; may be NULL */
} pe_hip_tr_control;
typedef struct pe_hip_tr_adaptive_stats {
    long long n_accepted, n_rejected_lte, n_rejected_newton, n_at_dt_min; /* steps of the batch (one sequence per call) */
    long long newton_iters_rejected;  /* solve_once-equivalents spent in rejected steps, summed over instances */
    int n_analyses;                   /* symbolic (re-)analyses the dt range caused */
    double dt_smallest, dt_largest, t_end; /* over the attempted steps */
    pe_hip_run_stats run;             /* as pe_hip_analyze_tr fills it: accepted steps / their Newton iterations only */
} pe_hip_tr_adaptive_stats;
int pe_hip_analyze_tr_adaptive(pe_hip_engine* h, double t_stop, const pe_hip_tr_control* c, pe_hip_tr_adaptive_stats* stats);
/* every attempted step of the last adaptive call, from entry `first`: dt, and 0 accepted / 1 rejected by LTE / 2 rejected by Newton;
 * *n_total = entries of the log; dt / outcome may be NULL */
int pe_hip_get_tr_step_log(pe_hip_engine* h, long long first, int capacity, double* dt, int* outcome, long long* n_total);

/* Checkpoint / resume of the device-resident simulation state of every instance (solution, time, companion histories,
 * junction and relay state, counters, device values): a transient continued from a loaded checkpoint is bit-identical to an
 * uninterrupted one.  The blob does not contain the circuit: load the same circuit (same tables, same batch) first. */
int pe_hip_checkpoint_size(pe_hip_engine* h, size_t* bytes);
int pe_hip_checkpoint_save(pe_hip_engine* h, void* buffer, size_t capacity);
int pe_hip_checkpoint_load(pe_hip_engine* h, const void* buffer, size_t size);

/* Small-signal AC at angular frequency omega [rad/s] (circult::solve_once with the models' iterate_ac hooks; one call per
 * sweep point of run_ac_analysis, circuit.h:389-431).  Non-linear devices are stamped at their last linearisation: run
 * pe_hip_analyze_dc(PE_HIP_MODE_OP) first, as the reference's AC / ACOP cases do (circuit.h:192-232).  The complex system
 * is solved in real-equivalent form [Ar -Ai; Ai Ar] by the same kernels.  pe_hip_get_solution_ac returns the phasors.
 * Up to three rounds of iterative refinement while the componentwise backward error is above 4e-16 or not a number, then one closing
 * residual evaluation: PE_HIP_ERR_INACCURATE when that final backward error is not finite (the sweep below applies the same rule per
 * instance). */
int pe_hip_analyze_ac(pe_hip_engine* h, double omega, pe_hip_run_stats* stats);
int pe_hip_get_solution_ac(pe_hip_engine* h, int first_instance, int count, double* re, double* im);

/* A whole frequency sweep as one call.  The points become extra instances of the real-equivalent system on a third engine (batch =
 * instances of the circuit x points per pass), the value vectors are made on the device (every AC value is constant or omega x a
 * per-instance constant: one base vector per circuit instance is uploaded per sweep, not one vector per point), iterative refinement is
 * decided per instance, and only the kept rows come back, in one copy.
 *   Bands.  The static pivot order is matched on representative values at one frequency, exactly as pe_hip_analyze_ac does it: the
 *   points are sorted ascending, omega == 0 points form a band of their own, a band starts at its first omega w0, is analysed on instance
 *   0's values at w0 and takes every point with omega <= 10 w0.  A band is solved in ceil(points / P) passes.
 *   Points per pass P.  Knob AC_SWEEP_POINTS (pe_hip_set_knob / PHY_ENGINE_HIP_AC_SWEEP_POINTS, read at every sweep); 0 = automatic: what
 *   fits half of the device's free memory, at most 4 GiB (a fixed 256 MiB in builds without HIP), by pe_hip_info.bytes_per_instance of
 *   the AC system, never more than the largest band holds or than 65535 instances in all.  Sizing the first automatic sweep of a circuit costs one
 *   symbolic analysis on the single-point engine if pe_hip_analyze_ac has not run on it yet (not part of n_analyses).  The third engine is
 *   rebuilt only when P changes.
 *   Memory outside that budget: the result, 2 x n_points x instances x kept rows doubles, once on the device and once on the host
 *   (200 points x 8 instances x 10 002 rows: 256 MB each) -- select rows (pe_hip_set_ac_sweep_rows) where that matters.
 *   A band whose values cannot be analysed (singular at its w0, e.g. a node held by capacitors only at omega = 0) launches nothing: its
 *   points take the fallback below.  gpu_ms is the HIP-event time around the passes on the engine's stream -- fill, solves, refinement
 *   with its host round trips, gather --; the bands' symbolic analyses run on the host before them and are not in it.
 *   Fallback.  A point with an instance at PE_HIP_ERR_SINGULAR / _INACCURATE in its batch, or whose refined solution is not finite, is
 *   solved again by pe_hip_analyze_ac (which analyses on that point's own values) and counted in n_fallback_points; if that fails too its
 *   status is the point's status.  A circuit with a host-stamp overlay (pe_hip_set_overlay: the values come from callbacks per omega)
 *   takes that path for every point.  A HIP error ends the call.
 * pe_hip_analyze_ac / pe_hip_get_solution_ac are unchanged; after a sweep pe_hip_get_solution_ac holds the last fallback point, if any.
 * pe_hip_analyze_dc, _analyze_tr, _analyze_tr_adaptive, _reset, _set_solution, _checkpoint_load, _update_param and _load_circuit make the stored sweep
 * unreadable (PE_HIP_ERR_ARG, "no AC sweep yet").  There is no sweep twin on the multi-device pe_hip_sweep_* handle (it has no AC at all). */
typedef struct pe_hip_ac_sweep_stats {
    int n_points;            /* as passed */
    int n_passes;            /* batched factor+solve passes */
    int points_per_pass;     /* largest number of points put into one pass */
    int n_analyses;          /* symbolic analyses (one per frequency band) */
    int n_refine_rounds;     /* correction solves, summed over passes */
    int n_fallback_points;   /* points that were (re)solved by the single-point path */
    double gpu_ms;           /* HIP-event time of the passes */
} pe_hip_ac_sweep_stats;

/* rows of x = [node voltages ; branch currents] kept for every point of the following sweeps; n_rows = 0 / rows = NULL: all rows.
 * Needs a loaded circuit; dropped by pe_hip_load_circuit.  PE_HIP_ERR_ARG (engine unchanged) for a row out of range.  A stored sweep
 * becomes unreadable (its layout is that of the rows it was made with). */
int pe_hip_set_ac_sweep_rows(pe_hip_engine* h, int n_rows, const int* rows);

/* Small-signal AC at omegas[0..n_points) [rad/s], any order, duplicates and 0 allowed, every instance of the batch.  Same meaning per
 * point as pe_hip_analyze_ac (non-linear devices at their last linearisation: run the OP first).  point_status (may be NULL) receives a
 * pe_hip_status per point (worst over the instances).  Returns PE_HIP_OK when every point solved, else the first failing point's status;
 * the points that solved stay readable.  PE_HIP_ERR_ARG for n_points < 1, a negative or non-finite omega, omegas == NULL. */
int pe_hip_analyze_ac_sweep(pe_hip_engine* h, int n_points, const double* omegas, int* point_status, pe_hip_ac_sweep_stats* stats);

/* phasors of the last sweep, in the CALLER's point order: re / im [n_points][count][n_kept_rows]; a failed point reads NaN */
int pe_hip_get_ac_sweep(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, double* re, double* im);

/* Read-back of a small-signal system as the device last assembled it (pe_hip_get_matrix reads the main engine only): the 2N x 2N
 * real-equivalent system [Ar -Ai; Ai Ar] in CSR with sorted columns (explicit zeros included), N = rows of the circuit.
 *   which  0: the single-point engine of pe_hip_analyze_ac;  1: the batched engine of the last pass of pe_hip_analyze_ac_sweep, instance
 *          q = b * P + p (circuit instance b, point p of that pass; unused points of a pass repeat its last omega);  2 / 3: the
 *          single-point and the batched engine of pe_hip_analyze_noise (the adjoint, i.e. transposed, system).  Engine 2 only sizes the
 *          automatic pass: it never assembles values, so asking it for vals is PE_HIP_ERR_ARG.  4: the batched engine of the last pass of
 *          pe_hip_analyze_sens (the adjoint system at omega = 0), instance q = b * P + p, rhs the selector of the output in slot p.
 *   vals  the values of the last assembly (vals may be NULL).
 *   rhs    [2N] the right-hand side AS STAMPED -- the copy the refinement keeps, not the residual a refinement round leaves in the value
 *          vector (may be NULL).  PE_HIP_ERR_ARG when the last solve on that engine failed before the copy was taken.
 * Capacity-0-first like pe_hip_get_front_table: with nnz_capacity == 0 only *n_rows (2N) and *nnz are written; else nnz_capacity >= nnz,
 * row_ptr holds 2N + 1 ints, col_ind / vals nnz entries.  PE_HIP_ERR_ARG when that engine does not exist yet.  Launches nothing.
 * pe_hip_get_ac_pass_size: P of engine 1 or 3.  pe_hip_get_ac_analysis_omega: the omega whose values the pivot order of engine 0 was last
 * matched on (-1: none yet) -- pe_hip_analyze_ac matches again when there is none, when omega == 0 and that one are not both zero, or when
 * omega > 10 x or < 0.1 x that one. */
int pe_hip_get_matrix_ac(pe_hip_engine* h, int which, int instance, int nnz_capacity, int* row_ptr, int* col_ind, double* vals, double* rhs, int* n_rows,
                         int* nnz);
int pe_hip_get_ac_pass_size(pe_hip_engine* h, int which, int* points_per_pass);
int pe_hip_get_ac_analysis_omega(pe_hip_engine* h, double* omega);

/* ---- DC sweep (.DC): the operating point at every value of one swept parameter, as one call.  The points become extra instances of the
 * circuit on an engine of its own (batch = instances of the circuit x points per pass); the swept value is written on the device, the
 * kept rows come back in one copy.  THE MAIN ENGINE IS READ, NEVER WRITTEN: its solution, parameters, time, status, counters, Newton
 * trace, probes and any stored AC / noise sweep are the same bits before and after the call.
 *   Swept parameter.  kind / index / column as pe_hip_update_param names them: PE_HIP_VDC column 0, PE_HIP_IDC column 0, or PE_HIP_R column
 *   0 (the engine holds 1.0 / r, divided on the host exactly as pe_hip_update_param does).  Anything else: PE_HIP_ERR_ARG.  A device with
 *   an unconnected pin sweeps nothing -- every point is then the same solve.  values: any order, duplicates and mixed signs allowed; the
 *   same value goes to every instance of the batch.  Every call takes the main engine's CURRENT parameters, options and knobs (a
 *   pe_hip_update_param between two sweeps takes effect; the sweep engine is rebuilt after one), its time and last step.
 *   PE_HIP_DC_SWEEP_PARALLEL.  Every point starts from the main engine's current state of its instance (solution, junction state, relay
 *   contacts, device value vector) and is the solve that pe_hip_update_param with that value followed by pe_hip_analyze_dc would make from
 *   there.  Without continuation the result does not depend on the pass size but through the summation order of the launch geometry.
 *   continuation = 1 (natural-parameter continuation).  After each solve a pair (point, instance) fails when its status is not PE_HIP_OK or its
 *   solution is not finite.  Each failing pair is reseeded -- solution and junction state copied -- from the converged point of the SAME
 *   instance that is nearest in sorted-value position within the pass, where equal values share a position (distance 0); a tie goes to the
 *   lower position.  Only reseeded pairs are solved again; a converged pair is never solved twice.  The rounds of a pass end when nothing
 *   fails, when a round converges no new pair, or after max_rounds (<= 0: the points of the pass).  Neighbours are searched inside the
 *   pass only, so with continuation a point's status may depend on the pass size; it is deterministic for a given one.  The host reads one
 *   small record per round and no solution.
 *   PE_HIP_DC_SWEEP_TRACE.  The classical .DC: the points run one after another in the CALLER's order, each from the state the last
 *   converged point left (the first from the main engine's state), so an up-down list traces a relay's hysteresis loop.  A failed point
 *   reads NaN and the next one starts from the last converged state (a shadow copy per instance on the sweep engine).  continuation and
 *   max_rounds are ignored.
 *   Refusals (PE_HIP_ERR_ARG, nothing changed, a stored sweep stays readable): no circuit, n_points < 1, values or the control NULL, a
 *   non-finite value, r == 0 for PE_HIP_R, a mode other than PE_HIP_MODE_OP / PE_HIP_MODE_DC, an unknown order, an index out of range, a
 *   host-stamp overlay (pe_hip_set_overlay), PARALLEL on a circuit with a PE_HIP_RELAY (its result depends on history: use TRACE).
 *   Points per pass P.  Knob DC_SWEEP_POINTS (pe_hip_set_knob / PHY_ENGINE_HIP_DC_SWEEP_POINTS, read at every sweep); 0 = automatic: the
 *   memory budget of pe_hip_analyze_ac_sweep by pe_hip_info.bytes_per_instance of the main engine (four times its circuit arrays while it
 *   has no symbolic analysis yet), never more than the points or than 65535 instances in all.  Passes take contiguous runs of the sorted
 *   values; the unused slots of the last pass repeat its last point and are not gathered.  TRACE always runs one point at a time.
 *   One symbolic analysis serves the sweep engine, on instance 0's values at the first sorted point (TRACE: the first point); the
 *   residual safety net covers the rest as elsewhere (its re-analyses count in n_analyses).  A sweep engine that is still current -- same
 *   P, no parameter, option or knob changed since -- is reused with its analysis (n_analyses = 0).
 * The stored result stays readable until the next DC sweep, pe_hip_set_dc_sweep_rows or pe_hip_load_circuit.  There is no twin on the
 * multi-device pe_hip_sweep_* handle. */
#define PE_HIP_DC_SWEEP_PARALLEL 0
#define PE_HIP_DC_SWEEP_TRACE    1
typedef struct pe_hip_dc_sweep_control {
    int kind, index, column; /* the swept parameter, named as pe_hip_update_param names it */
    int mode;                /* PE_HIP_MODE_OP or PE_HIP_MODE_DC */
    int order;               /* PE_HIP_DC_SWEEP_PARALLEL | PE_HIP_DC_SWEEP_TRACE */
    int continuation;        /* PARALLEL only: 1 = reseed failed points (rule above) */
    int max_rounds;          /* reseeding rounds per pass; <= 0: points of the pass */
} pe_hip_dc_sweep_control;
typedef struct pe_hip_dc_sweep_stats {
    int n_points;             /* as passed */
    int n_passes;             /* PARALLEL: passes; TRACE: points */
    int points_per_pass;      /* largest number of points put into one pass */
    int n_rounds;             /* reseeding rounds of the pass that took most */
    long long n_failed_cold;  /* (point, instance) pairs not converged after round 0 (TRACE: after their one attempt) */
    long long n_reseeded;     /* seed copies made by the rounds */
    long long n_failed;       /* pairs still failing at the end */
    long long newton_iters;   /* all attempts, summed; an attempt that did not converge counts max_newton */
    int n_analyses;           /* symbolic analyses of the sweep engine during this call */
    double gpu_ms;            /* HIP-event time of the passes on the sweep engine's stream */
} pe_hip_dc_sweep_stats;

/* rows of x = [node voltages ; branch currents] kept for every point of the following DC sweeps; n_rows = 0 / rows = NULL: all rows.
 * Needs a loaded circuit; dropped by pe_hip_load_circuit.  PE_HIP_ERR_ARG (engine unchanged) for a row out of range.  A stored DC sweep
 * becomes unreadable (its layout is that of the rows it was made with). */
int pe_hip_set_dc_sweep_rows(pe_hip_engine* h, int n_rows, const int* rows);

/* The sweep described above.  point_status (may be NULL) receives a pe_hip_status per point: the first failing instance's.  Returns
 * PE_HIP_OK when every pair converged, else the first failing point's status; the pairs that converged stay readable. */
int pe_hip_analyze_dc_sweep(pe_hip_engine* h, int n_points, const double* values, const pe_hip_dc_sweep_control* c, int* point_status,
                            pe_hip_dc_sweep_stats* stats);

/* results of the last DC sweep in the CALLER's point order: x [n_points][count][n_kept_rows], NaN where the pair failed */
int pe_hip_get_dc_sweep(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, double* x);
/* per pair [n_points][count] (each may be NULL): pe_hip_status of its last attempt; Newton iterations of that attempt when it converged
 * (else 0); seed_point = the caller's index of the point its last attempt started from, -1: the main engine's own state */
int pe_hip_get_dc_sweep_status(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, int* status, int* newton_iters,
                               int* seed_point);

/* ---- Operating point with gmin and source stepping: the continuation every simulator of this kind falls back on when the bare Newton
 * iteration of pe_hip_analyze_dc does not converge.  The solves are those of pe_hip_analyze_dc, untouched; the controller around them
 * lives on the device, one (phase, lambda, Delta) per instance, and the host reads one small record per level: no solution, no status array.
 *   1. Direct attempt.  The first solve is exactly pe_hip_analyze_dc of that mode from the resident state.  An instance that converges there is
 *   finished: its state is bit for bit what pe_hip_analyze_dc leaves.  Only failing instances step; failing = status not PE_HIP_OK, or a
 *   solution that is not finite.  A batch in which nothing fails costs one extra small launch and one read-back.
 *   2. Phases.  method = PE_HIP_STEP_GMIN: gmin stepping only; PE_HIP_STEP_SOURCE: source stepping only; PE_HIP_STEP_AUTO: gmin stepping, then
 *   source stepping for what gmin stepping could not solve.  Instances of one batch may be in different phases at the same time.  A phase
 *   starts from x = 0 with the junction state and the relay contacts as pe_hip_reset leaves them; time, companion histories and counters
 *   are not touched (the Newton iterations of the levels count like any other).
 *   3. The homotopy, lambda in [0, 1].  Source stepping: every independent static source value of the instance holds lambda * its real value
 *   (one rounded multiply; at lambda = 1 the real value itself): PE_HIP_VDC, PE_HIP_IDC and the digital drives.  The other values written
 *   at load time are no sources and are never scaled: the resistance of a PE_HIP_SWITCH, the gains of the controlled sources and of the
 *   op-amp, the transformer ratios.  Sources whose value is formed at every iteration -- PE_HIP_VAC, PE_HIP_IAC, PE_HIP_VGEN -- are not
 *   scaled either: in OP / DC they contribute what they always do there, in TROP they keep their value at t = 0.  Gmin stepping: the conductance from every
 *   node to ground is g_start * (g_end / g_start)^lambda below lambda = 1 and the engine's g_min itself at lambda = 1, with
 *   g_end = max(g_min, 1e-13); sources stay at their real values.
 *   4. The controller, in plain double arithmetic (+, *, min, comparisons).  Level lambda = 0 is solved first; if it fails, the phase fails.
 *   Then the candidate is t = min(1, lambda + Delta).  Accepted (status PE_HIP_OK and a finite solution): the state goes into the instance's
 *   shadow, lambda = t, Delta *= grow (not after the level lambda = 0).  Rejected: the state comes back from the shadow, Delta *= shrink;
 *   Delta < dl_min fails the phase.  The instance fails when its last phase fails or when it has spent max_levels levels over all its phases.
 *   Fields <= 0 take their defaults: dl_init 0.125, grow 2, shrink 0.25, dl_min 2^-20, g_start 1e-2, max_levels 200.  step_max_newton <= 0:
 *   the engine's max_newton; a positive value caps the Newton iterations of the stepping levels only (the direct attempt and the
 *   options of the engine are untouched).
 *   5. What the call leaves.  A solved instance has status PE_HIP_OK and holds its solution at the real source values and the engine's g_min.
 *   A failed instance has the status of its last failed attempt (PE_HIP_ERR_NO_CONVERGENCE or PE_HIP_ERR_SINGULAR) and holds the state of the
 *   last accepted level of its last phase, zeros if that phase accepted none.  Whatever the outcome -- an error return included -- every
 *   source value and the node-to-ground conductance of every instance are the real ones again before the call returns: no later analysis
 *   runs on scaled sources.  (pe_hip_get_matrix shows the system of the last solve, as always.)  Returns the first failing instance's
 *   status, like pe_hip_analyze_dc.
 *   6. Refusals (PE_HIP_ERR_ARG): no circuit, the control NULL, an unknown method, a mode other than OP / DC / TROP, a negative control
 *   field, a non-finite one; PE_HIP_STEP_SOURCE on a circuit with a host-stamp overlay (pe_hip_set_overlay: its sources are not the
 *   engine's to scale) -- PE_HIP_STEP_AUTO then runs the direct attempt and gmin stepping only.
 * One symbolic analysis serves every level (matched on instance 0's values as elsewhere); the residual safety net covers the large-gmin
 * levels.  The shadow and the controller's arrays are allocated at the first call and freed with the circuit. */
#define PE_HIP_STEP_GMIN   1
#define PE_HIP_STEP_SOURCE 2
#define PE_HIP_STEP_AUTO   3
typedef struct pe_hip_op_step_control {
    int method;          /* PE_HIP_STEP_GMIN | PE_HIP_STEP_SOURCE | PE_HIP_STEP_AUTO */
    int max_levels;      /* levels per instance over all its phases; <= 0: 200 */
    int step_max_newton; /* Newton cap of the stepping levels; <= 0: the engine's */
    int log_capacity;    /* log entries kept per instance; 0: none */
    double dl_init, grow, shrink, dl_min; /* <= 0: 0.125, 2, 0.25, 2^-20 */
    double g_start;      /* <= 0: 1e-2 */
} pe_hip_op_step_control;
typedef struct pe_hip_op_step_stats {
    long long n_levels;      /* levels solved, summed over the instances (the direct attempt is not a level) */
    long long n_accepted, n_rejected;
    int n_direct, n_gmin, n_source; /* instances solved by the direct attempt / in the gmin phase / in the source phase */
    int n_failed;            /* instances that gave up */
    long long newton_iters;  /* all attempts, summed; an attempt that did not converge counts its cap */
    int n_solves;            /* batched solves of the call, the direct attempt included */
    int n_launches;          /* controller launches */
    double gpu_ms;           /* HIP-event time of the whole call on the engine's stream */
    double control_ms;       /* host time spent in the controller launches and their read-backs */
} pe_hip_op_step_stats;
int pe_hip_analyze_op_stepping(pe_hip_engine* h, int mode, const pe_hip_op_step_control* c, pe_hip_op_step_stats* stats);
/* outcome per instance of the last stepping call (each array may be NULL): phase_solved_in 0 direct, 1 gmin, 2 source, -1 failed;
 * lambda_reached = the last accepted lambda of its last phase (1 when solved); levels solved; levels rejected; Newton iterations of all
 * its attempts.  PE_HIP_ERR_ARG before the first call on the resident circuit. */
int pe_hip_get_op_step_state(pe_hip_engine* h, int first, int count, int* phase_solved_in, double* lambda_reached, int* levels, int* rejected,
                             long long* newton_iters);
/* the log of one instance as kept on the device, at most `capacity` entries in the order solved (each array may be NULL): phase (1 gmin,
 * 2 source), lambda of the level, value = what was written for it (the node-to-ground conductance, or lambda itself for source stepping),
 * outcome (1 accepted, 0 rejected), Newton iterations when accepted.  n_total: levels the instance solved, which may exceed log_capacity. */
int pe_hip_get_op_step_log(pe_hip_engine* h, int instance, int capacity, int* phase, double* lambda, double* value, int* outcome, int* iters,
                           int* n_total);

/* ---- Small-signal noise analysis (.NOISE): the output noise spectral density of the circuit at its operating point, the share of every
 * device in it, and the integrated noise over the swept band -- by the ADJOINT method: one solve of the transposed small-signal system per
 * frequency point, whatever the number of sources.  With A the complex small-signal matrix of pe_hip_analyze_ac at omega and e the output
 * selector, A^T y = e gives the transfer of a current injected between rows a and b to the output as y_b - y_a, so a white current source
 * of density S_k there contributes S_k |y_b - y_a|^2.  The real-equivalent system solved is the transpose of [Ar -Ai; Ai Ar], which is
 * that of A^H: A^H z = e has z = conj(y) for the real e, and |z_b - z_a| = |y_b - y_a|.
 *   Output.  x[out_pos] - x[out_neg], x the small-signal solution (rows 0-based: node n is row n - 1, branch currents after the nodes);
 *   -1 = none (ground).  out_pos == out_neg (both -1 included) is PE_HIP_ERR_ARG.  The result is a ONE-SIDED density in V^2/Hz (A^2/Hz when
 *   the output is a branch row) at f = omega / 2 pi.
 *   Temperature.  temp_k is the circuit temperature of the thermal sources; <= 0: 300.15 K, the models' default Temp of 27 C.  Constants as
 *   the models use them: k = 1.380650524e-23, q = 1.6021765314e-19.
 *   Sources.  White current sources, mutually uncorrelated, each between two rows, in this fixed order:
 *     1. every resistor, in table order: S = 4 k T |g| between its nodes, g the conductance of its AC stamp;
 *     2. every junction of the diode table, in table order (PN_junction; the four junctions of a full-bridge rectifier are four entries of
 *        that table): shot noise S = 2 q |I_d| between anode and cathode;
 *     3. every three-pin device, table by table in the order the tables were passed to pe_hip_load_circuit, each in table order: a
 *        MOSFET one source S = (8/3) k T |gm| between D and S; a BJT two, base 2 q |I_b| between B and E (part 0), then collector
 *        2 q |I_c| between C and E (part 1).
 *   The bias currents are those that flow in the SOLVED LINEARISED NETWORK -- the last linearisation evaluated at the resident solution x:
 *   I_d = geq V_d(x) + Ieq, I_b = geq V_j(x) + Ieq_be, I_c = gm V_j(x) + Ieq_c, gm that linearisation's -- not the model formula evaluated
 *   again at x (the two differ at the level of the Newton tolerance; this one satisfies KCL with x).  Of a diode only the conduction
 *   current counts: the diffusion-capacitance companion a transient stamp folds into the junction's conductance and current is taken out.
 *   A device whose AC stamp is skipped (an unconnected pin) keeps its place with S = 0 and rows -1, -1 (a BJT: both parts).  Everything else is
 *   noiseless: g_min, switch and relay contacts, controlled sources, op-amp, transformers, independent sources and generators.  There is
 *   no flicker noise (the models have no KF / AF) and no input-referred noise (divide by |H|^2 from pe_hip_analyze_ac_sweep).
 *   Operating point.  Like pe_hip_analyze_ac the call uses the last linearisation: run pe_hip_analyze_dc(PE_HIP_MODE_OP) first.  An
 *   instance whose last analysis failed (status != 0 in pe_hip_get_instance_state) has no operating point: the call returns that status,
 *   every point carries it and reads NaN.
 *   Points.  The rules of pe_hip_analyze_ac_sweep: any order, duplicates and 0 allowed, the same bands (n_analyses counts them), the same
 *   AC_SWEEP_POINTS knob and automatic pass size, gpu_ms measured the same way, results in the caller's order.  A point with a failing or
 *   non-finite instance in its batch is retried ALONE: one pass of one point, under an analysis on its own values (counted in
 *   n_retried_points, its analysis in n_analyses); if it fails again the point carries that status and reads NaN, the others stay
 *   readable.  Returns PE_HIP_OK, or the first failing point's status.
 *   Determinism.  The sum over the sources is formed on the device without floating-point atomics, in an order that depends on the number
 *   of sources only: the densities and contributions of a point do not depend on the pass size, the batch or the pass it fell into.
 *   They do depend on the other points of the call through the band: the pivot order of a band is made at its representative (first)
 *   frequency, so a point reads the same bits in two calls only where it falls into bands with the same representative in both.
 *   Integrated noise.  Trapezoidal rule in linear f over the distinct points sorted ascending, on the host from the stored densities;
 *   NaN when any point failed.
 *   The call has sweep state of its own (adjoint system, engines, buffers): a stored forward sweep stays readable, bit for bit.  The calls
 *   that make a stored AC sweep unreadable make the stored noise result unreadable too (PE_HIP_ERR_ARG, "no noise analysis yet").
 *   PE_HIP_ERR_ARG, engine unchanged: no circuit, n_points < 1, omegas or c NULL, a negative or non-finite omega, a row out of range,
 *   out_pos == out_neg, a circuit with a host-stamp overlay (its models have no noise description).  There is no twin on the multi-device
 *   pe_hip_sweep_* handle. */
typedef struct pe_hip_noise_control {
    int out_pos, out_neg;     /* rows of x; -1: ground */
    double temp_k;            /* <= 0: 300.15 */
    int keep_contributions;   /* 1: keep S_k |y_b - y_a|^2 of every source: n_points x batch x n_sources doubles, device and host */
} pe_hip_noise_control;
typedef struct pe_hip_noise_stats {
    int n_points;             /* as passed */
    int n_sources;            /* sources of the circuit */
    int n_passes;             /* batched factor+solve passes, retries included */
    int points_per_pass;      /* largest number of points put into one pass */
    int n_analyses;           /* symbolic analyses: one per frequency band + one per retried point */
    int n_refine_rounds;      /* correction solves, summed over passes */
    int n_retried_points;     /* points that failed in their batch and were solved again alone */
    double gpu_ms;            /* HIP-event time of the passes */
} pe_hip_noise_stats;
int pe_hip_analyze_noise(pe_hip_engine* h, int n_points, const double* omegas, const pe_hip_noise_control* c, int* point_status, pe_hip_noise_stats* stats);
/* densities of the last call in the CALLER's point order: psd [n_points][count]; contrib NULL or [n_points][count][n_sources] (needs
 * keep_contributions); a failed point reads NaN */
int pe_hip_get_noise(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, double* psd, double* contrib);
/* the source table of the resident circuit (no analysis needed): kind (pe_hip_kind), index of the device in its table, part (0; BJT
 * collector: 1), the two rows (-1: ground); *n_sources receives the count, at most `capacity` entries are written; any pointer may be NULL */
int pe_hip_get_noise_sources(pe_hip_engine* h, int capacity, int* kind, int* index, int* part, int* row_a, int* row_b, int* n_sources);
/* current densities S_k of the last call, [count][n_sources], A^2/Hz; NaN after a call that was refused for a failed operating point */
int pe_hip_get_noise_source_density(pe_hip_engine* h, int first_instance, int count, double* s);
/* integrated output noise of the last call over its band, [count], V^2 (A^2) */
int pe_hip_get_noise_integrated(pe_hip_engine* h, int first_instance, int count, double* v2);

/* ---- DC sensitivity analysis (.SENS): the first-order sensitivity of one or more outputs of the resident operating point to EVERY device
 * parameter of every instance, by the ADJOINT method: one solve per output, whatever the number of parameters.  With the residual
 * f(x, p) = A(x; p) x - b(x; p) of the operating point, J its Jacobian and e the output selector, J^T y = e gives
 * d out / d p_k = -y^T d f / d p_k.  J^T is the adjoint small-signal system of pe_hip_analyze_noise at omega = 0 (the AC stamp at
 * omega = 0 is the Newton Jacobian cell for cell); the outputs are the "points" of that sweep body, all in one band.
 *   Output o.  x[out_pos[o]] - x[out_neg[o]] (rows 0-based as everywhere, -1 = ground).  out_pos[o] == out_neg[o] is PE_HIP_ERR_ARG.
 *   Operating point.  The last linearisation, exactly as pe_hip_analyze_ac / _noise use it: the Jacobian is the one of the last stamp, and
 *   d f / d p is evaluated at the resident x with the arm of the model that the device evaluation takes there.  The Jacobian therefore
 *   belongs to the iterate BEFORE the accepted one: the result is exact to first order in the last Newton step.  A caller who wants it
 *   tighter runs pe_hip_analyze_dc once more from the converged point.  Whatever mode produced the resident point (OP, DC, TROP, a TR step)
 *   is taken as it is; reactive elements are at omega = 0 (capacitors open, inductors shorted), and the diffusion-capacitance companion a
 *   transient stamp folds into a junction is taken out, as in the noise analysis.  An instance whose last analysis failed has no
 *   operating point: the call returns that status, every output carries it and everything reads NaN.
 *   The Jacobian is the STAMPED matrix.  Two arms of the models stamp a conductance that is not the slope of the current they stamp: a
 *   PMOS (gds and gm carry the opposite sign, as in the reference's pmosfet.h) and a junction on the linear continuation of the limited
 *   exponential (Ud / (N Ut) > 50: Is limexp / Ute instead of Is exp(50) / Ute).  Newton's fixed point is the same, but on those arms the
 *   result is not the derivative of the converged output (figures: DESIGN.md 8).
 *   Parameters.  Named as pe_hip_update_param names them -- raw columns (kind, index in its table, column) -- in a table that is fixed per
 *   circuit and readable without an analysis (pe_hip_get_sens_params), in this order:
 *     1. PE_HIP_R column 0, in table order;  2. PE_HIP_VDC column 0;  3. PE_HIP_IDC column 0;
 *     4. every entry of the diode table, in table order, each with columns Is, N, Isr, Nr, Temp, Ibv, Bv, Area (0-6 and 8; not Bv_set, tt,
 *        tt_in_tr);
 *     5. the remaining kinds table by table in the order the tables were passed to pe_hip_load_circuit, each in table order: VCCS g, VCVS mu,
 *        CCCS alpha, CCVS r, OPAMP mu, XFMR n, XFMR_CT n_total (one column each); MOSFETs Kp, lambda, Vth; BJTs Is, N, BetaF, Temp, Area.
 *   A device with an unconnected pin keeps its place and reads 0.  Everything else is a constant of the analysis: C, L, coupled inductors,
 *   VAC / IAC, generators, switch, relay, digital drives, g_min, r_open.  The raw columns reach the device as derived ones (a junction's
 *   Is Area, N Ut, Nr Ut, Bv_eff = Bv - N Ut ln(Ibv / (Is Area)); a BJT's Is Area, N Ut): the chain rule through that derivation is part of
 *   the result, the breakdown arm and the linear continuation of the limited exponential included.  A centre-tapped transformer with
 *   n_total = 0 reads 0.
 *   Results.  s[o][b][k] = d out_o / d p_k of instance b.  normalized = 1: p_k d out_o / d p_k, and a parameter that is 0 reads 0 (a
 *   resistor's p_k is the reciprocal of its resident conductance).  weight (NULL: none; [n_params], shared by the batch, finite): the call
 *   also forms rss[o][b] = sum_k (w_k s[o][b][k])^2 over the returned (normalised when asked) values; with w_k = sigma_k this is the
 *   first-order variance of the output.  keep_sensitivities = 0 returns only rss: nothing of size n_params comes back to the host
 *   (keep_sensitivities = 0 without weights asks for nothing: PE_HIP_ERR_ARG).
 *   Passes.  P outputs x batch instances per pass.  Knob SENS_OUTPUTS (pe_hip_set_knob / PHY_ENGINE_HIP_SENS_OUTPUTS, read at every call);
 *   0 = automatic by the memory rule of pe_hip_analyze_ac_sweep.  One symbolic analysis, on the values of instance 0.  An output with a
 *   failing or non-finite instance in its pass is retried ALONE under an analysis of its own (counted in n_retried_outputs and
 *   n_analyses); if it fails again it carries that status and reads NaN, the others stay readable.  Returns PE_HIP_OK or the first failing
 *   output's status.
 *   Determinism.  No floating-point atomics; the rss sum is formed on the device in an order that depends on n_params only.  Results do not
 *   depend on P, the batch or the pass an output fell into.
 *   The main engine is read and never written.  The call has state of its own (adjoint system, engines, buffers): a stored AC sweep, noise
 *   result and DC sweep read the same bits before and after.  The calls that make the stored noise result unreadable make this one
 *   unreadable too (PE_HIP_ERR_ARG, "no sensitivity analysis yet").
 *   PE_HIP_ERR_ARG, engine unchanged: no circuit, n_outputs < 1, c or its row arrays NULL, a row out of range, equal rows, a non-finite
 *   weight, a circuit with a host-stamp overlay.  There is no twin on the multi-device pe_hip_sweep_* handle. */
typedef struct pe_hip_sens_control {
    int n_outputs;
    const int* out_pos;       /* [n_outputs] rows of x; -1: ground */
    const int* out_neg;
    int normalized;           /* 1: p_k d out / d p_k */
    int keep_sensitivities;   /* 1: keep s: n_outputs x batch x n_params doubles, device and host */
    const double* weight;     /* NULL, or [n_params] */
} pe_hip_sens_control;
typedef struct pe_hip_sens_stats {
    int n_outputs;            /* as passed */
    int n_params;             /* parameters of the circuit */
    int n_passes;             /* batched factor+solve passes, retries included */
    int outputs_per_pass;     /* largest number of outputs put into one pass */
    int n_analyses;           /* symbolic analyses: one + one per retried output */
    int n_refine_rounds;      /* correction solves, summed over passes */
    int n_retried_outputs;    /* outputs that failed in their pass and were solved again alone */
    double gpu_ms;            /* HIP-event time of the passes */
} pe_hip_sens_stats;
/* the parameter table of the resident circuit (no analysis needed): kind (pe_hip_kind), index of the device in its table, raw column;
 * *n_params receives the count, at most `capacity` entries are written; any pointer may be NULL */
int pe_hip_get_sens_params(pe_hip_engine* h, int capacity, int* kind, int* index, int* column, int* n_params);
int pe_hip_analyze_sens(pe_hip_engine* h, const pe_hip_sens_control* c, int* output_status, pe_hip_sens_stats* stats);
/* results of the last call: s NULL or [n_outputs][count][n_params] (needs keep_sensitivities); rss NULL or [n_outputs][count] (needs
 * weights); a failed output reads NaN */
int pe_hip_get_sens(pe_hip_engine* h, int first_output, int n_outputs, int first_instance, int count, double* s, double* rss);

/* ---- Multi-port network analysis (.NET / .SP / .LIN): the impedance, admittance and scattering matrices of the circuit at its operating
 * point between n chosen terminal pairs (ports), over a frequency sweep.  The matrix of a frequency point is the same for every port and
 * only the right-hand side differs: a pass of the sweep factors ONCE and solves the other ports with the factors kept.
 *   Z.  With A the complex small-signal matrix of pe_hip_analyze_ac at omega and e_j = +1 at port_pos[j], -1 at port_neg[j] (a unit current
 *   into port j's positive terminal and out of its negative one; rows 0-based as everywhere, -1: ground), A x = e_j gives column j:
 *   Z[i][j] = x[port_pos[i]] - x[port_neg[i]], the response at port i to an excitation at port j, in ohm for node rows.  Every independent
 *   AC source of the circuit is switched off: the right-hand side is the selector alone, the matrix is untouched -- a voltage source is a
 *   short, a current source is open.
 *   Y and S.  Y = Z^-1.  S = D^-1 (Z - Z0) (Z + Z0)^-1 D with Z0 = diag(z0), D = diag(sqrt z0): power waves with real reference
 *   resistances.  S is formed from (Z + Z0)^-1, not from Y: a port on a node held by a voltage source makes Z singular and leaves S well
 *   defined.  Both inverses come from complex Gaussian elimination with partial pivoting by modulus, on the device, one matrix per
 *   (point, instance).  An inverse does not exist when an entry of the matrix M to invert is not finite or, after pivoting, a pivot is not
 *   finite or has |pivot| <= n_ports 2^-52 max |M_ij|: that matrix (Y, or S) reads NaN and its status is PE_HIP_ERR_SINGULAR; Z is
 *   unaffected, and so is the other of the two.
 *   Operating point.  The rule of pe_hip_analyze_ac: the last linearisation -- run pe_hip_analyze_dc(PE_HIP_MODE_OP) first.  An instance
 *   whose last analysis failed has no operating point: the call returns that status, every point carries it and reads NaN.
 *   Points.  The rules of pe_hip_analyze_ac_sweep: any order, duplicates and 0 allowed, the same bands (n_analyses counts them), the same
 *   memory rule for the automatic pass size; the knob NET_POINTS sets the pass size; gpu_ms is measured the same way (the conversion
 *   included); results in the caller's order.  A point with a failing or non-finite instance in its pass is retried ALONE, one pass of one
 *   point under an analysis on its own values (n_retried_points); if it fails again it carries that status and reads NaN (Z, Y and S, the
 *   two matrix statuses carry it too), the other points stay readable.  Returns PE_HIP_OK, or the first failing point's status; a
 *   singular Y or S is no failure of the call.
 *   One factorisation per pass.  A pass fills the value vectors, writes port 0's selector, factors and solves, and for ports 1 .. n-1
 *   writes the next selector and solves with the factors kept; every refinement correction of this call uses the kept factors too
 *   (threshold, at most three rounds and the closing residual are those of the forward sweep).  n_factorisations counts the batched
 *   numeric factorisations launched: one per pass, plus any the residual safety net forced (a re-match on an instance's own values, in
 *   the factoring solve or in a kept-factor one, is followed by a factorisation of EVERY instance under the new pivot order, and those
 *   factors are the ones kept from then on); n_solves the batched kept-factor solves.
 *   pe_hip_options.refactor_every_solve speaks of the main engine's transient and does not apply to this call's own engine.
 *   Determinism.  The conversion of a matrix depends on that matrix alone (no atomics, no scratch), the column of a port on its own
 *   right-hand side: results do not depend on the pass size, the batch or the pass, and permuting the ports permutes rows and columns of
 *   Z exactly.  They depend on the other points of the call through the band, as in the noise analysis.
 *   State.  The call has state of its own (a forward small-signal system with selector lists, engines, buffers); the main engine is read
 *   and never written: a stored AC sweep, noise result, sensitivity result and DC sweep read the same bits before and after.  The calls
 *   that make a stored noise result unreadable make this one unreadable too (PE_HIP_ERR_ARG, "no network analysis yet").
 *   PE_HIP_ERR_ARG, engine unchanged: no circuit, n_points < 1, omegas or c NULL, a negative or non-finite omega, n_ports out of range,
 *   port_pos / port_neg NULL, a row out of range, port_pos == port_neg for a port (both -1 included), two identical ports, a non-finite
 *   or non-positive z0, a circuit with a host-stamp overlay.  There is no twin on the multi-device pe_hip_sweep_* handle. */
#define PE_HIP_NET_MAX_PORTS 8
enum { PE_HIP_NET_Z = 0, PE_HIP_NET_Y = 1, PE_HIP_NET_S = 2 };
typedef struct pe_hip_net_control {
    int n_ports;              /* 1 .. PE_HIP_NET_MAX_PORTS */
    const int* port_pos;      /* [n_ports] rows of x; -1: ground */
    const int* port_neg;
    const double* z0;         /* [n_ports] reference resistances, finite, > 0; NULL: 50 ohm each */
} pe_hip_net_control;
typedef struct pe_hip_net_stats {
    int n_points;             /* as passed */
    int n_ports;
    int n_passes;             /* passes, retries included */
    int points_per_pass;      /* largest number of points put into one pass */
    int n_analyses;           /* symbolic analyses: one per frequency band + one per retried point */
    int n_factorisations;     /* batched numeric factorisations launched (passes + retries + any the safety net forced) */
    int n_solves;             /* batched kept-factor solves: ports after the first, and every refinement correction */
    int n_refine_rounds;      /* correction solves, summed over passes and ports */
    int n_retried_points;     /* points that failed in their pass and were solved again alone */
    double gpu_ms;            /* HIP-event time of the passes and of the conversion */
} pe_hip_net_stats;
int pe_hip_analyze_net(pe_hip_engine* h, int n_points, const double* omegas, const pe_hip_net_control* c, int* point_status, pe_hip_net_stats* stats);
/* one matrix kind (PE_HIP_NET_Z / _Y / _S) of the last call in the CALLER's point order: re, im [n_points][count][n_ports][n_ports], entry
 * [i][j] the response at port i to an excitation at port j; a failed point, and a matrix without inverse, read NaN */
int pe_hip_get_net(pe_hip_engine* h, int which, int first_point, int n_points, int first_instance, int count, double* re, double* im);
/* statuses of Y and of S of the last call, [n_points][count] each: PE_HIP_OK, PE_HIP_ERR_SINGULAR, or the status of a failed point;
 * either pointer may be NULL */
int pe_hip_get_net_status(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, int* y_status, int* s_status);
/* The conversion alone, on caller-supplied impedance matrices z_re / z_im [n_mats][n_ports][n_ports]: the same device kernel, the same
 * rules.  Needs a created engine, no circuit.  z0: [n_ports] or NULL (50 ohm each).  y_* / s_*: [n_mats][n_ports][n_ports], statuses
 * [n_mats]; any output pointer may be NULL.  PE_HIP_ERR_ARG: n_ports out of range, n_mats < 1, z_re or z_im NULL, a bad z0. */
int pe_hip_convert_net(pe_hip_engine* h, int n_ports, int n_mats, const double* z_re, const double* z_im, const double* z0, double* y_re, double* y_im,
                       double* s_re, double* s_im, int* y_status, int* s_status);

/* ---- Pole-zero analysis (.PZ): the natural frequencies of the circuit at its operating point nearest to a shift the caller names, and
 * the zeros of one transfer function, by shift-invert Arnoldi on ONE factorisation.
 *   The pencil.  The small-signal matrix of pe_hip_analyze_ac is affine in omega: A(s) = G + s B with real G = Re A(j 1), B = Im A(j 1).
 *   The poles are the finite s with det A(s) = 0.  Independent sources do not matter: only the matrix is used.  The shift is
 *   s0 = j omega0, omega0 > 0 finite, chosen near the band of interest: a purely imaginary shift is what the real-equivalent engine
 *   factors anyway, A0 = A(s0).
 *   Poles.  s = s0 - omega0 / theta' over the eigenvalues theta' of M' = A0^-1 (omega0 B); omega0 B is the lower-left block of the matrix
 *   the engine has assembled at omega0, nothing is divided by omega0.  Eigenvalues with |theta'| <= theta_floor max |theta'| are the
 *   pencil's infinite eigenvalues (nodes without reactive elements) and are dropped: a definition, not a tolerance.
 *   Zeros of H(s) = c^T A(s)^-1 b, b a unit current into in_pos and out of in_neg, c reading x[out_pos] - x[out_neg] (rows as in
 *   pe_hip_analyze_net: -1 is ground, a branch row makes it a voltage excitation): the finite eigenvalues of the bordered pencil
 *   [[A(s), b], [c^T, 0]], whose shift-inverted operator is M'_z v = w - z (c^T w) / (c^T z) with w = M' v, z = A0^-1 b -- one more
 *   solve on the kept factors per call.  c^T z = H(s0) is returned (pe_hip_get_pz_gain).  H(s0) zero or not finite: that instance's
 *   zeros carry PE_HIP_ERR_SINGULAR, its poles are unaffected.  A mode that is uncontrollable or unobservable from the chosen ports
 *   appears as a coinciding pole and zero, as in SPICE.
 *   What the floor cannot remove.  Where the infinite eigenvalue is DEFECTIVE -- a Jordan block of size p at theta' = 0, which the bordered
 *   pencil of a transfer function with several zeros at infinity can have -- rounding spreads it over a ring of p values at
 *   |theta'| ~ (2^-52)^(1/p) max |theta'|, far above any relative floor (p = 7: 6e-3).  The call returns them: up to p more values, the
 *   farthest of the list, |s - s0| ~ omega0 / |theta'|, ill-determined in every digit.  err_est measures the Krylov residual only, not the
 *   conditioning of a value: on a complete instance they carry err_est 0 and count as converged like every other value.  A caller tells
 *   them by their distance (beyond the band the shift was chosen for) or by moving omega0: a zero stays where it is, the ring moves.
 *   Iteration, per instance, all instances in lock-step.  The start vector is M' r, r a fixed function of the row index (no random
 *   numbers: the same for every instance and run).  Arnoldi without restart, up to max_krylov steps, classical Gram-Schmidt applied twice
 *   against all previous vectors.  An instance is COMPLETE when h(k+1,k) <= breakdown_tol |w|, |w| taken before orthogonalisation: its
 *   Krylov space is invariant, its Ritz values are the whole finite spectrum reachable from the start vector; it is parked -- its
 *   right-hand sides are zero from then on, nothing of it is overwritten.  Ritz values are the eigenvalues of the k x k Hessenberg
 *   matrix (complex single-shift QR with Wilkinson shifts on the device, at most 30 k sweeps: beyond that the instance carries
 *   PE_HIP_ERR_NO_CONVERGENCE).  err_est = |h(k+1,k)| |e_k^T y_i| / |theta'_i|, 0 for a complete instance; a value is CONVERGED when
 *   err_est <= tol.  Results per instance are sorted by |s - s0| ascending, ties by larger imaginary part first.  Fewer than n_wanted
 *   converged leading entries is no failure of the call: the counts say so.  No restarts.
 *   Operating point.  The rule of pe_hip_analyze_net: run pe_hip_analyze_dc(PE_HIP_MODE_OP) first; an instance whose last analysis failed
 *   has no operating point: the call returns that status, every instance carries it and reads NaN.
 *   Statuses.  A singular or non-finite A0 (the shift on a pole of a lossless LC, a NaN parameter) gives that instance the engine's
 *   status: it reads NaN, the others stay readable.  Returns PE_HIP_OK or the first failing instance's status.
 *   One factorisation.  The call is one pass of one point of the sweep body: poles and zeros together are 1 + 2 (max_krylov + 1)
 *   right-hand sides on one factorisation; n_factorisations is 1 plus whatever the residual safety net forced, n_solves the batched
 *   kept-factor solves, refinement corrections included.
 *   Determinism.  The kernels of this call sum through a fixed tree per instance (no atomics) and nothing of an instance is read from
 *   another or from an earlier call: two calls return the same bits.  Across batches the same holds where the solves do -- the static pivot
 *   order of the factorisation is matched on instance 0's values, as for every analysis of these engines: an instance reads the same bits
 *   at another batch size or position when that order is the same (always, when it is instance 0 in both).
 *   State.  The call has state of its own; the main engine is read and never written: a stored AC sweep, noise, sensitivity, network
 *   and DC-sweep result read the same bits before and after.  The basis takes batch x (max_krylov + 1) x 2 rows doubles on the device,
 *   checked against the memory budget of the sweep's automatic pass size.
 *   PE_HIP_ERR_ARG, engine unchanged: no circuit, c NULL, `what` outside 1 .. 3, omega0 not finite or <= 0, n_wanted or max_krylov outside
 *   1 .. PE_HIP_PZ_MAX_KRYLOV, n_wanted > max_krylov, a non-finite or negative tol, theta_floor or breakdown_tol, when zeros are asked
 *   for a row out of range or pos == neg for a port (both -1 included), a basis that does not fit the memory budget, a circuit with a
 *   host-stamp overlay.  There is no twin on the multi-device pe_hip_sweep_* handle. */
#define PE_HIP_PZ_MAX_KRYLOV 64
enum { PE_HIP_PZ_POLES = 1, PE_HIP_PZ_ZEROS = 2 };
typedef struct pe_hip_pz_control {
    int what;                 /* PE_HIP_PZ_POLES, PE_HIP_PZ_ZEROS, or 3: both */
    double omega0;            /* the shift s0 = j omega0, rad/s, finite, > 0 */
    int n_wanted;             /* 1 .. max_krylov: how many nearest values the caller is after.  Validated only: the call always runs max_krylov
                                 steps, and the caller compares n_converged with it */
    int max_krylov;           /* Arnoldi steps, 1 .. PE_HIP_PZ_MAX_KRYLOV; 0: 32 */
    double tol;               /* err_est of a converged value; 0: 1e-10 */
    double theta_floor;       /* 0: 1e-12 */
    double breakdown_tol;     /* 0: 2^-40 */
    int in_pos, in_neg;       /* rows of b (zeros only) */
    int out_pos, out_neg;     /* rows of c (zeros only) */
} pe_hip_pz_control;
typedef struct pe_hip_pz_stats {
    int n_steps;              /* Arnoldi steps run per kind (poles, zeros): max_krylov, or 0 when no pass ran */
    int n_factorisations;     /* batched numeric factorisations launched: 1 + what the safety net forced */
    int n_solves;             /* batched kept-factor solves, refinement corrections included */
    int n_refine_rounds;      /* correction solves */
    int n_complete;           /* instances whose pole iteration is complete */
    double gpu_ms;            /* HIP-event time of the pass and of the Ritz kernel */
} pe_hip_pz_stats;
/* instance_status: NULL or [batch], the worst of what the instance's poles and zeros carry */
int pe_hip_analyze_pz(pe_hip_engine* h, const pe_hip_pz_control* c, int* instance_status, pe_hip_pz_stats* stats);
/* results of the last call, which = PE_HIP_PZ_POLES or PE_HIP_PZ_ZEROS (it must have been asked for): re, im, err_est [count][capacity]
 * padded with NaN (values past capacity are not returned); n_found, n_converged (the length of the leading converged run), complete
 * [count]; any output pointer may be NULL */
int pe_hip_get_pz(pe_hip_engine* h, int which, int first_instance, int count, int capacity, double* re, double* im, double* err_est, int* n_found,
                  int* n_converged, int* complete);
/* H(s0) = c^T A0^-1 b of the last call (it must have asked for zeros): re, im [count] */
int pe_hip_get_pz_gain(pe_hip_engine* h, int first_instance, int count, double* re, double* im);
/* The dense eigenvalue kernel alone, on caller-supplied upper Hessenberg matrices h_re / h_im [n_mats][m][m] (what lies below the
 * subdiagonal is not read), 1 <= m <= PE_HIP_PZ_MAX_KRYLOV.  Needs a created engine, no circuit.  theta_re / theta_im [n_mats][m]: the
 * eigenvalues; last_re / last_im [n_mats][m]: for each the last component of its unit eigenvector; status [n_mats]: PE_HIP_OK,
 * PE_HIP_ERR_SINGULAR (an entry is not finite: that matrix reads NaN) or PE_HIP_ERR_NO_CONVERGENCE.  PE_HIP_ERR_ARG: m out of range,
 * n_mats < 1, a NULL pointer. */
int pe_hip_eig_hessenberg(pe_hip_engine* h, int m, int n_mats, const double* h_re, const double* h_im, double* theta_re, double* theta_im, double* last_re,
                          double* last_im, int* status);

/* x = [node voltages ; branch currents], instance-major [count][rows] */
int pe_hip_get_solution(pe_hip_engine* h, int first_instance, int count, double* x);
int pe_hip_set_solution(pe_hip_engine* h, int first_instance, int count, const double* x);
/* per-instance: status (pe_hip_status), accepted steps, Newton iterations, current time */
/* Diagnostics of the residual safety net (pe_hip_options.residual_tol): solves repaired by iterative refinement, symbolic
 * re-analyses on a failing instance's own values, and whether the engine has left the resident kernel for the host-driven
 * (refining) schedule.  Any pointer may be NULL. */
int pe_hip_get_safety_net_counters(pe_hip_engine* h, long long* refined, long long* rematched, int* careful);

/* On-box achievable HBM bandwidth (SURVEY.md 8d "measure the achievable ceiling on the box with a device-to-device stream
 * kernel"): copies `bytes` (two temporary buffers of that size) `reps` times; *gbps = (read + written bytes) / HIP-event time. */
int pe_hip_measure_hbm_ceiling(pe_hip_engine* h, size_t bytes, int reps, double* gbps);

/* The sweep's one exchange step: per-row statistics of the current solution over this engine's instances,
 * computed on the device -- out[0][r] = sum_b x_b[r], out[1][r] = sum_b x_b[r]^2, out[2][r] = min_b, out[3][r] = max_b
 * (out: [4][rows] doubles, host memory).  Ranks combine them with one SUM and one MAX all-reduce (min travels as -min). */
int pe_hip_sweep_statistics(pe_hip_engine* h, double* out);

int pe_hip_get_instance_state(pe_hip_engine* h, int first_instance, int count, int* status, long long* steps, long long* iters, double* t);

/* ---- Transient probes and measurements (.probe / .measure tran), recorded ON THE DEVICE at every accepted transient step of every
 * instance; the host reads back only what was asked for.
 *   pe_hip_set_probes  rows[n_probes]: indices into x as pe_hip_get_solution returns it (node voltages, then branch currents; duplicates
 *                      allowed); room for `capacity` samples per instance; a sample every `stride`-th accepted step; n_measures streaming
 *                      measurements m[] over those probes.  Needs a loaded circuit (pe_hip_load_circuit drops the configuration);
 *                      n_probes = n_measures = 0 removes it.  PE_HIP_ERR_ARG, engine unchanged and usable, for: a row out of range;
 *                      capacity < 1 or stride < 1; an unknown kind; a measure's probe out of range; CROSS with occurrence < 1 or an edge
 *                      outside {-1, 0, 1}; batch x capacity x (n_probes + 1) overflowing 64 bits.
 *   pe_hip_arm_probes  opens a window at every instance's current point: sample 0 = (t_now, x[rows]), every measure initialised there.
 *                      Every accepted TR step of pe_hip_analyze_tr then updates the measures, and every stride-th one since arming appends
 *                      a sample (t, x[rows]); samples past `capacity` are only counted (n_dropped) -- the measures still see them.  A
 *                      rejected or rolled-back step records nothing.  Anything else that moves x or t (pe_hip_analyze_dc, _reset,
 *                      _set_solution, _set_time, _checkpoint_load, _load_circuit) disarms the window; what it recorded stays readable
 *                      until the next arm.  No AC.
 *   pe_hip_get_probe_samples  t [count][capacity], v [count][capacity][n_probes] (slots past n_recorded[b] are NaN), n_recorded [count],
 *                      n_dropped [count]; any pointer may be NULL.
 *   pe_hip_get_measures  out [count][n_measures][2], with (t0,v0) -> (t1,v1) consecutive accepted points of the window, T = t_last - t_arm:
 *                      MIN / MAX  extreme value (strict compare), time of its first occurrence
 *                      INTEG      sum (t1 - t0)(v0 + v1) / 2, T
 *                      AVG        INTEG / T (NaN if T = 0), T
 *                      RMS        sqrt(sum (t1 - t0)(v0^2 + v1^2) / 2 / T) (NaN if T = 0), T
 *                      CROSS      time of the occurrence-th selected crossing (rise: v0 < level <= v1, fall: v0 > level >= v1, at
 *                                 t0 + (level - v0)(t1 - t0)/(v1 - v0); NaN if not reached), number of selected crossings seen
 *                      An instance that was never armed since the configuration reads NaN. */
enum pe_hip_measure_kind
{
    PE_HIP_MEAS_MIN = 1,
    PE_HIP_MEAS_MAX = 2,
    PE_HIP_MEAS_AVG = 3,
    PE_HIP_MEAS_RMS = 4,
    PE_HIP_MEAS_INTEG = 5,
    PE_HIP_MEAS_CROSS = 6
};
typedef struct pe_hip_measure
{
    int kind;       /* pe_hip_measure_kind */
    int probe;      /* index into the probe list */
    int edge;       /* CROSS: +1 rise, -1 fall, 0 either */
    int occurrence; /* CROSS: k >= 1 */
    double level;   /* CROSS */
} pe_hip_measure;
int pe_hip_set_probes(pe_hip_engine* h, int n_probes, const int* rows, int capacity, int stride, int n_measures, const pe_hip_measure* m);
int pe_hip_arm_probes(pe_hip_engine* h);
int pe_hip_get_probe_samples(pe_hip_engine* h, int first_instance, int count, double* t, double* v, int* n_recorded, long long* n_dropped);
int pe_hip_get_measures(pe_hip_engine* h, int first_instance, int count, double* out);

/* ---- Fourier analysis of transient probes (.four): harmonics 0 .. H of f0 and the total harmonic distortion of configured probes,
 * accumulated ON THE DEVICE at every accepted step of an armed probe window; the host reads back (H + 1) coefficients per probe and instance.
 *   The window is [t_start, t_end], t_end = t_start + n_periods / f0, formed once on the host in double.  Tw = t_end - t_start,
 *   w0 = 2 pi f0, tau = t - t_start.  v(t) of a configured probe is the piecewise-linear interpolant through the accepted points of the
 *   armed window, the pairs (t0,v0) -> (t1,v1) the measures see.  For k = 0 .. H:
 *                      a_0 = (1 / Tw) int v dtau, b_0 = 0
 *                      a_k = (2 / Tw) int v cos(k w0 tau) dtau,  b_k = (2 / Tw) int v sin(k w0 tau) dtau      (k >= 1)
 *   over the part of the window the accepted steps covered: the exact integral of that interpolant (Filon-trapezoidal weights per
 *   segment, not a sample rule).  A segment that straddles t_start or t_end is clipped there, its end value taken by linear
 *   interpolation; segments wholly outside contribute nothing.  Each integral is a compensated sum in the order of the accepted steps;
 *   `stride` and `capacity` of the sample buffer have no influence, rejected or rolled-back steps record nothing.
 *                      amp_k = sqrt(a_k^2 + b_k^2), amp_0 = |a_0|
 *                      phase_k = atan2(-b_k, a_k) (phase_0 = 0 or pi), so that v ~ a_0 + sum amp_k cos(k w0 tau + phase_k)
 *                      thd = sqrt(sum_{k = 2 .. H} amp_k^2) / amp_1, summed in ascending k; the division is what IEEE gives
 *                      covered[b] = length of the window integrated so far (the sum of the clipped segments' tau_b - tau_a)
 *   Coefficients are always normalised by the nominal Tw: compare covered with Tw.  An instance whose covered is 0 (never armed since
 *   the configuration, or a window not yet reached) reads NaN.  Running past t_end is harmless, the last segment is clipped: with fixed
 *   steps do run a step or two past it, because t is accumulated step by step and may fall a rounding short of t_end; with
 *   pe_hip_analyze_tr_adaptive make t_end the t_stop or a breakpoint.
 *   pe_hip_set_fourier  needs a probe configuration with at least one probe; `probes` are indices into its probe list (duplicates
 *                      allowed).  NULL or n_probes = 0 removes the analysis.  pe_hip_set_probes and pe_hip_load_circuit drop it.  Like
 *                      pe_hip_set_probes, a successful call ends an armed window: arm again.  pe_hip_arm_probes zeroes the accumulators;
 *                      whatever disarms the probe window disarms this too, and what was accumulated stays readable until the next arm.
 *                      Not part of a checkpoint.  PE_HIP_ERR_ARG, engine and current configuration unchanged, for: no circuit or no
 *                      probes; f0 not finite or <= 0; t_start not finite; n_periods < 1; n_harmonics outside 1 .. 63; a probe index out
 *                      of range; n_probes < 0; a t_end that is not finite or not > t_start in double.
 *   pe_hip_get_fourier  coef [count][n_probes][H + 1][4] = a, b, amp, phase; thd [count][n_probes]; covered [count]; any pointer may be
 *                      NULL.  Normalisation, amp, phase and thd are computed on the device (k_fourier_finish) at every call. */
typedef struct pe_hip_fourier_control
{
    double f0;        /* Hz, finite, > 0 */
    double t_start;   /* absolute time, finite */
    int n_periods;    /* >= 1 */
    int n_harmonics;  /* H, 1 .. 63  (DC + H harmonics = at most one wavefront of lanes) */
    int n_probes;
    const int* probes; /* indices into the probe list of pe_hip_set_probes; duplicates allowed */
} pe_hip_fourier_control;
int pe_hip_set_fourier(pe_hip_engine* h, const pe_hip_fourier_control* c);
int pe_hip_get_fourier(pe_hip_engine* h, int first_instance, int count, double* coef, double* thd, double* covered);

/* ---- Integration rule of the transient (SPICE method=trap / gear, a backward-Euler step).  The trapezoidal rule is A-stable but not
 * L-stable: on a stiff element hit by an edge its amplification factor tends to -1 and the element's voltage or current alternates in
 * sign step after step.  Backward Euler (first order) and the variable-step second-order Gear rule (BDF2) damp such an element at once.
 *   For a step from t_n to t_n + h, with h_p the accepted step that led to t_n and rho = h / h_p, the derivative at the new point is
 *   a0 y_{n+1} + a1 y_n + a2 y_{n-1}:
 *                      BE     a0 = 1 / h                         a1 = -1 / h           a2 = 0
 *                      GEAR2  a0 = (1 + 2 rho) / (h (1 + rho))   a1 = -(1 + rho) / h   a2 = rho^2 / (h (1 + rho))
 *   A GEAR2 step takes the BE coefficients, decided per instance on the device, when the instance has no second point (h_p = 0) or when
 *   rho > 1 + sqrt 2, the zero-stability limit of variable-step BDF2.  Capacitors, inductors and coupled inductors get the companion of
 *   the rule.  The diffusion capacitance of a junction is cd = tt geq of the last linearisation, FROZEN at the start of the step as it is
 *   for the trapezoidal rule, under the same guards: companion conductance a0 cd, history cd (a1 vd_n + a2 vd_{n-1}).
 *   pe_hip_set_tr_method  an engine setting like the options: allowed without a circuit, survives pe_hip_load_circuit.  The default is
 *                      PE_HIP_TR_TRAP; an engine that never calls it, or sets TRAP, computes the bits it always computed and allocates
 *                      nothing.  An unknown value is PE_HIP_ERR_ARG, engine unchanged.  Setting the current method again changes nothing;
 *                      a different one restarts the integration history of every instance.
 *   pe_hip_get_tr_history  h_prev [count]: per instance the step h_p that its second history point belongs to; 0: the next step starts the
 *                      history (a BE step under GEAR2).  Reads 0 under TRAP.
 *   The history restarts (h_p := 0 for every instance) at pe_hip_load_circuit, _reset, _analyze_dc and _analyze_op_stepping,
 *   _set_solution, _set_time, _checkpoint_load of a blob without history, a method change, and inside pe_hip_analyze_tr_adaptive at every
 *   breakpoint other than t_stop that a step reaches (the derivative jumps at a source corner: a two-step formula must not look across
 *   it).  pe_hip_analyze_tr does NOT restart it: consecutive calls continue one trajectory, with whatever dt each call has.  An instance
 *   whose step failed restarts its own history before its next step.
 *   Variable-step controller (pe_hip_analyze_tr_adaptive).  The history rule (three accepted points before the test runs) and the
 *   decisions are those of the trapezoidal rule (err_r = h^3 / 2 |DD3_r|, exponent 1/3); estimate and exponent become
 *                      BE     err_r = h^2 |DD2_r| over the last two points and the candidate (the error is h^2 / 2 times the second
 *                             derivative, which is about 2 DD2); rejection factor max(0.1, 0.9 q^(-1/2)), growth min(2, 0.9 q^(-1/2))
 *                      GEAR2  err_r = h^3 (1 + rho)^2 / (rho (1 + 2 rho)) |DD3_r|, rho = h / (t2 - t1) (the error is
 *                             h^3 (1 + rho)^2 / (6 rho (1 + 2 rho)) times the third derivative, which is about 6 DD3: 2/9 h^3 at rho = 1);
 *                             exponent 1/3
 *   The growth cap of 2 keeps rho below 1 + sqrt 2.  q travels as the NaN-preserving integer image of the maximum, as before.
 *   Checkpoints.  Under TRAP a blob is "PEHIPCK2", byte for byte what it was.  Under BE / GEAR2 it is "PEHIPCK3": the same parts, then the
 *   method and the history; a continued run is bit-identical to an uninterrupted one.  A "PEHIPCK2" blob loads under any method and
 *   restarts the history; a "PEHIPCK3" blob loads only into an engine set to the blob's method (else PE_HIP_ERR_ARG).
 *   A circuit with a host-stamp overlay integrates in its own host hooks: pe_hip_analyze_tr under a method other than TRAP is
 *   PE_HIP_ERR_ARG, engine unchanged.  AC, noise, sensitivity, DC sweep and operating points do not depend on the method. */
enum pe_hip_tr_method { PE_HIP_TR_TRAP = 0, PE_HIP_TR_BE = 1, PE_HIP_TR_GEAR2 = 2 };
int pe_hip_set_tr_method(pe_hip_engine* h, int method);
int pe_hip_get_tr_method(pe_hip_engine* h, int* method);
int pe_hip_get_tr_history(pe_hip_engine* h, int first_instance, int count, double* h_prev);

/* ---- Monte-Carlo / parameter sweep over several GPUs of one node (csrc/pe_sweep.cpp).
 * Independent instances of ONE topology are the natural shard of this path: the symbolic analysis is replicated per device, the
 * instances are dealt out in contiguous blocks of ceil(batch / G) per device -- the chunk rule of the reference's only
 * multi-device code, src/pe_synth_cuda_u64_cones.cu:1894-1904 -- and, like that code's entry points (:1861-1872: extern "C",
 * device mask first), the device set is a bit mask.  One engine + one host thread per device while a call runs; no exchange
 * between devices except the final reduction of the per-row statistics (pe_hip_sweep_reduce: combined on the host in device
 * order, bitwise reproducible).  Tables as pe_hip_load_circuit: batched parameter blocks are [batch][count][ncol] over the
 * WHOLE sweep.  All calls return pe_hip_status; pe_hip_sweep_last_error(s) is valid until the next call on s (s may be NULL
 * after a failed create). */
typedef struct pe_hip_sweep pe_hip_sweep;
int pe_hip_sweep_create(unsigned device_mask, pe_hip_sweep** out); /* bit d = HIP device d */
void pe_hip_sweep_destroy(pe_hip_sweep* s);
const char* pe_hip_sweep_last_error(pe_hip_sweep* s);
int pe_hip_sweep_devices(pe_hip_sweep* s);
int pe_hip_sweep_shard(pe_hip_sweep* s, int index, int* device, int* first_instance, int* count); /* block of the index-th device of the mask */
int pe_hip_sweep_set_options(pe_hip_sweep* s, const pe_hip_options* opt);
int pe_hip_sweep_load_circuit(pe_hip_sweep* s, int n_nodes, int n_branches, int batch, int n_tables, const pe_hip_device_table* tables);
int pe_hip_sweep_reset(pe_hip_sweep* s);
int pe_hip_sweep_operating_point(pe_hip_sweep* s, int mode, pe_hip_run_stats* stats); /* OP / DC / TROP solve of every instance */
/* the same with gmin / source stepping, per device engine; stats: sums over the devices, times and launch counts of the slowest */
int pe_hip_sweep_operating_point_stepping(pe_hip_sweep* s, int mode, const pe_hip_op_step_control* c, pe_hip_op_step_stats* stats);
int pe_hip_sweep_run(pe_hip_sweep* s, double dt, int nsteps, pe_hip_run_stats* stats); /* transient steps of every instance; stats: sums, slowest device's times */
int pe_hip_sweep_reduce(pe_hip_sweep* s, double* out); /* [4][rows]: sum, sum of squares, min, max of the current solution over all instances */
int pe_hip_sweep_get_solution(pe_hip_sweep* s, int first_instance, int count, double* x);
int pe_hip_sweep_get_instance_state(pe_hip_sweep* s, int first_instance, int count, int* status, long long* steps, long long* iters, double* t);
/* transient probes of every instance of the sweep: the same meaning as pe_hip_set_probes / _arm_probes / _get_probe_samples / _get_measures,
 * forwarded to each device's engine; read-back in global instance order */
int pe_hip_sweep_set_probes(pe_hip_sweep* s, int n_probes, const int* rows, int capacity, int stride, int n_measures, const pe_hip_measure* m);
int pe_hip_sweep_arm_probes(pe_hip_sweep* s);
int pe_hip_sweep_get_probe_samples(pe_hip_sweep* s, int first_instance, int count, double* t, double* v, int* n_recorded, long long* n_dropped);
int pe_hip_sweep_get_measures(pe_hip_sweep* s, int first_instance, int count, double* out);
/* the Fourier analysis of every instance of the sweep: pe_hip_set_fourier on each device's engine, pe_hip_get_fourier in global instance order */
int pe_hip_sweep_set_fourier(pe_hip_sweep* s, const pe_hip_fourier_control* c);
int pe_hip_sweep_get_fourier(pe_hip_sweep* s, int first_instance, int count, double* coef, double* thd, double* covered);
/* pe_hip_set_tr_method on every device's engine (allowed before pe_hip_sweep_load_circuit) */
int pe_hip_sweep_set_tr_method(pe_hip_sweep* s, int method);
/* iteration count of every step of instance 0 since the last reset (parity with the reference's Newton counts) */
int pe_hip_get_newton_trace(pe_hip_engine* h, int capacity, int* iters, int* n_out);
/* last stamped MNA system of one instance (CSR, sorted columns; vals/rhs may be NULL) */
int pe_hip_get_matrix(pe_hip_engine* h, int instance, int* row_ptr, int* col_ind, double* vals, double* rhs);

/* in-kernel phase clocks of one instance since the last reset, 100 MHz ticks:
 * [0] device eval + MNA gather, [1] LU wave fronts (incl. the fused forward substitution), [2] LU cooperative fronts,
 * [3] cooperative part of the backward pass, [4] Newton bookkeeping, [5] backward pass (all of it; a separate forward pass of
 * the factor-reuse path is counted here too), [6] cooperative assembly, [7] cooperative block loops */
int pe_hip_get_phase_clocks(pe_hip_engine* h, int instance, long long* ticks8);
/* the same plus, from slot 8 on, six values per cooperative-front layout (0 whole front in LDS, 1 pivot panels + pulled Schur
 * tiles, 2 chain link): assembly, block loop, Schur update, factor store [ticks], fronts [count], sum of m*m; slots 48.. (split
 * schedule): for parts 0..3 of the instance, start / end tick and hardware placement of that workgroup in the last factor launch */
int pe_hip_get_phase_clocks_ex(pe_hip_engine* h, int instance, int capacity, long long* ticks, int* n_out);

/* host-only: run the symbolic analysis on a pattern and report its statistics (no GPU needed) */
int pe_hip_analyze_pattern(int n, const int* row_ptr, const int* col_ind, const double* values, pe_hip_info* out);

/* host-only: the assembly tree of that analysis.  Arrays of `capacity` ints; *n_fronts receives the count.
 * pivots[s], updates[s] (front order m = pivots + updates), parent[s] (-1 = root); fronts are in postorder. */
int pe_hip_analyze_pattern_fronts(int n, const int* row_ptr, const int* col_ind, const double* values, int capacity, int* pivots, int* updates,
                                  int* parent, int* n_fronts);

#ifdef __cplusplus
}
#endif
#endif /* PE_HIP_H */
