"""ctypes binding of libpe_hip.so (include/pe_hip.h).  Thin: plain pointers in, numpy arrays out.

The library is the product; this file only marshals.  There is no CPU fallback: if the shared library
is missing, or no HIP device is visible, `Engine()` raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PE_HIP_LIB", os.path.join(_HERE, "libpe_hip.so"))

# pe_hip_kind
R, CAP, L, VDC, VAC, IDC, DIODE = 1, 2, 3, 4, 5, 6, 7
IAC, VCCS, VCVS, CCCS, CCVS, OPAMP, XFMR, SWITCH, VGEN, COUPLED_L = 8, 9, 10, 11, 12, 13, 14, 15, 16, 17
NMOS, PMOS, BJT_NPN, BJT_PNP, RELAY, XFMR_CT = 18, 19, 20, 21, 22, 23
DIODE_NPARAM = 11
VGEN_NPARAM = 8
# parameter columns of a device table, by the kind names of deck_tables.  The library holds the same counts in the loader and gen_ncol
# (csrc/pe_circuit.cpp) and in param_columns (csrc/pe_sweep.cpp); tests/param_common.py pins this table to them.
NCOL = {"R": 1, "C": 1, "L": 1, "VDC": 1, "VAC": 3, "IDC": 1, "D": DIODE_NPARAM, "IAC": 3, "VCCS": 1, "VCVS": 1, "CCCS": 1, "CCVS": 1, "OPAMP": 1,
        "XFMR": 1, "SW": 1, "VGEN": VGEN_NPARAM, "KL": 3, "NMOS": 3, "PMOS": 3, "NPN": 5, "PNP": 5, "RELAY": 2, "XCT": 1}
KIND_CODE = {"R": R, "C": CAP, "L": L, "VDC": VDC, "VAC": VAC, "IDC": IDC, "D": DIODE, "IAC": IAC, "VCCS": VCCS, "VCVS": VCVS, "CCCS": CCCS,
             "CCVS": CCVS, "OPAMP": OPAMP, "XFMR": XFMR, "SW": SWITCH, "VGEN": VGEN, "KL": COUPLED_L, "NMOS": NMOS, "PMOS": PMOS,
             "NPN": BJT_NPN, "PNP": BJT_PNP, "RELAY": RELAY, "XCT": XFMR_CT}
MODE_OP, MODE_DC, MODE_TR, MODE_TROP = 0, 1, 4, 5
OK, ERR_ARG, ERR_NO_DEVICE, ERR_SINGULAR, ERR_NO_CONVERGENCE, ERR_INTERNAL, ERR_INACCURATE = 0, -1, -2, -3, -4, -5, -6

EXPORTS = [
    "pe_hip_device_count", "pe_hip_create", "pe_hip_destroy", "pe_hip_last_error", "pe_hip_solve_csr_real", "pe_hip_solve_csr_complex", "pe_hip_build_id",
    "pe_hip_load_circuit", "pe_hip_set_options", "pe_hip_get_info", "pe_hip_get_front_table", "pe_hip_set_digital_drives", "pe_hip_set_overlay", "pe_hip_set_knob", "pe_hip_get_knob", "pe_hip_update_param",
    "pe_hip_reset", "pe_hip_analyze_dc", "pe_hip_analyze_tr", "pe_hip_get_solution", "pe_hip_set_solution",
    "pe_hip_get_instance_state", "pe_hip_sweep_statistics", "pe_hip_measure_hbm_ceiling", "pe_hip_get_safety_net_counters", "pe_hip_get_newton_trace", "pe_hip_get_matrix", "pe_hip_analyze_pattern",
    "pe_hip_analyze_pattern_fronts", "pe_hip_get_phase_clocks", "pe_hip_get_phase_clocks_ex", "pe_hip_analyze_ac", "pe_hip_get_solution_ac", "pe_hip_set_ac_sweep_rows", "pe_hip_analyze_ac_sweep", "pe_hip_get_ac_sweep", "pe_hip_checkpoint_size", "pe_hip_checkpoint_save", "pe_hip_checkpoint_load", "pe_hip_set_time",
    "pe_hip_sweep_create", "pe_hip_sweep_destroy", "pe_hip_sweep_last_error", "pe_hip_sweep_devices", "pe_hip_sweep_shard", "pe_hip_sweep_set_options",
    "pe_hip_sweep_load_circuit", "pe_hip_sweep_reset", "pe_hip_sweep_operating_point", "pe_hip_sweep_run", "pe_hip_sweep_reduce", "pe_hip_sweep_get_solution",
    "pe_hip_sweep_get_instance_state", "pe_hip_set_probes", "pe_hip_arm_probes", "pe_hip_get_probe_samples", "pe_hip_get_measures",
    "pe_hip_sweep_set_probes", "pe_hip_sweep_arm_probes", "pe_hip_sweep_get_probe_samples", "pe_hip_sweep_get_measures",
    "pe_hip_set_fourier", "pe_hip_get_fourier", "pe_hip_sweep_set_fourier", "pe_hip_sweep_get_fourier",
    "pe_hip_analyze_tr_adaptive", "pe_hip_get_tr_step_log",
    "pe_hip_set_tr_method", "pe_hip_get_tr_method", "pe_hip_get_tr_history", "pe_hip_sweep_set_tr_method",
    "pe_hip_analyze_noise", "pe_hip_get_noise", "pe_hip_get_noise_sources", "pe_hip_get_noise_source_density", "pe_hip_get_noise_integrated",
    "pe_hip_get_sens_params", "pe_hip_analyze_sens", "pe_hip_get_sens",
    "pe_hip_analyze_net", "pe_hip_get_net", "pe_hip_get_net_status", "pe_hip_convert_net",
    "pe_hip_analyze_pz", "pe_hip_get_pz", "pe_hip_get_pz_gain", "pe_hip_eig_hessenberg",
    "pe_hip_set_dc_sweep_rows", "pe_hip_analyze_dc_sweep", "pe_hip_get_dc_sweep", "pe_hip_get_dc_sweep_status",
    "pe_hip_analyze_op_stepping", "pe_hip_get_op_step_state", "pe_hip_get_op_step_log", "pe_hip_sweep_operating_point_stepping",
    "pe_hip_get_static_fronts", "pe_hip_get_static_skip_stats", "pe_hip_get_static_skip_refinement_stats",
    "pe_hip_get_matrix_ac", "pe_hip_get_ac_pass_size", "pe_hip_get_ac_analysis_omega",
]
DC_SWEEP_PARALLEL, DC_SWEEP_TRACE = 0, 1
NET_MAX_PORTS = 8
NET_Z, NET_Y, NET_S = 0, 1, 2
PZ_MAX_KRYLOV = 64
PZ_POLES, PZ_ZEROS, PZ_BOTH = 1, 2, 3
# pe_hip_tr_method
TR_TRAP, TR_BE, TR_GEAR2 = 0, 1, 2
_TR_NAMES = {"trap": TR_TRAP, "be": TR_BE, "gear2": TR_GEAR2, "gear": TR_GEAR2}
STEP_GMIN, STEP_SOURCE, STEP_AUTO = 1, 2, 3
# pe_hip_measure_kind
MEAS_MIN, MEAS_MAX, MEAS_AVG, MEAS_RMS, MEAS_INTEG, MEAS_CROSS = 1, 2, 3, 4, 5, 6
_MEAS_NAMES = {"min": MEAS_MIN, "max": MEAS_MAX, "avg": MEAS_AVG, "rms": MEAS_RMS, "integ": MEAS_INTEG, "cross": MEAS_CROSS}


class DeviceTable(C.Structure):
    _fields_ = [("kind", C.c_int), ("count", C.c_int), ("nodes", C.POINTER(C.c_int)), ("branch", C.POINTER(C.c_int)),
                ("params", C.POINTER(C.c_double)), ("params_batched", C.c_int)]


class Options(C.Structure):
    _fields_ = [("v_abstol", C.c_double), ("v_reltol", C.c_double), ("i_abstol", C.c_double), ("i_reltol", C.c_double),
                ("g_min", C.c_double), ("max_newton", C.c_int), ("refactor_every_solve", C.c_int), ("r_open", C.c_double), ("residual_tol", C.c_double)]


class Timings(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("h2d_ms", "solve_ms", "d2h_ms", "solve_host_ms", "total_host_ms", "analyze_ms")]


class Info(C.Structure):
    _fields_ = [("rows", C.c_int), ("n_nodes", C.c_int), ("n_branches", C.c_int), ("batch", C.c_int), ("nnz_a", C.c_int),
                ("nnz_lu", C.c_longlong), ("nnz_lu_stored", C.c_longlong), ("n_fronts", C.c_int), ("max_front", C.c_int),
                ("tree_depth", C.c_int), ("n_row_swaps", C.c_int), ("factor_flops", C.c_double),
                ("bytes_per_instance", C.c_longlong), ("n_r", C.c_int), ("n_c", C.c_int), ("n_l", C.c_int), ("n_v", C.c_int),
                ("n_i", C.c_int), ("n_d", C.c_int), ("nonlinear", C.c_int), ("n_parts", C.c_int), ("n_top_levels", C.c_int),
                ("n_wavefronts", C.c_int), ("lds_bytes", C.c_int), ("nnz_lu_stored_top", C.c_longlong), ("n_wave_fronts", C.c_int),
                ("n_quad_fronts", C.c_int), ("nnz_lu_stored_quad", C.c_longlong), ("mid_top_limit", C.c_int), ("ew_grid", C.c_int),
                ("quad_lds_pad", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Measure(C.Structure):
    _fields_ = [("kind", C.c_int), ("probe", C.c_int), ("edge", C.c_int), ("occurrence", C.c_int), ("level", C.c_double)]


class FourierControl(C.Structure):
    _fields_ = [("f0", C.c_double), ("t_start", C.c_double), ("n_periods", C.c_int), ("n_harmonics", C.c_int), ("n_probes", C.c_int),
                ("probes", C.POINTER(C.c_int))]


def _measures(measures):
    """measures: (kind, probe[, level, edge, occurrence]) tuples or dicts with those keys; kind a MEAS_* value or its name ('min', 'cross', ...)."""
    ms = list(measures)
    arr = (Measure * max(1, len(ms)))()
    for i, m in enumerate(ms):
        if isinstance(m, dict):
            kind, probe = m["kind"], m["probe"]
            level, edge, occ = m.get("level", 0.0), m.get("edge", 0), m.get("occurrence", 1)
        else:
            kind, probe = m[0], m[1]
            level = m[2] if len(m) > 2 else 0.0
            edge = m[3] if len(m) > 3 else 0
            occ = m[4] if len(m) > 4 else 1
        kind = _MEAS_NAMES.get(kind, kind) if isinstance(kind, str) else kind
        arr[i] = Measure(int(kind), int(probe), int(edge), int(occ), float(level))
    return len(ms), arr


def _probe_argtypes(l, prefix):
    getattr(l, prefix + "set_probes").argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.POINTER(Measure)]
    getattr(l, prefix + "arm_probes").argtypes = [C.c_void_p]
    getattr(l, prefix + "get_probe_samples").argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                                C.POINTER(C.c_longlong)]
    getattr(l, prefix + "get_measures").argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
    getattr(l, prefix + "set_fourier").argtypes = [C.c_void_p, C.POINTER(FourierControl)]
    getattr(l, prefix + "get_fourier").argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]


class _Probes:
    """set_probes / arm_probes / probe_samples / measures, shared by Engine and Sweep (prefix pe_hip_ / pe_hip_sweep_)."""
    _prefix = "pe_hip_"
    _probe_cfg = (0, 0, 0)  # n_probes, capacity, n_measures
    _four_cfg = (0, 0)      # configured probes, harmonics

    def set_probes(self, rows, capacity, stride=1, measures=()):
        """record x[rows] of every instance at every stride-th accepted transient step of an armed window (room for `capacity` samples)
        and update `measures` on the device; rows=[] with measures=() removes the configuration"""
        r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
        n_m, arr = _measures(measures)
        self._chk(getattr(lib(), self._prefix + "set_probes")(self._h, len(r), _ip(r), int(capacity), int(stride), n_m, arr))
        self._probe_cfg = (len(r), int(capacity), n_m) if (len(r) or n_m) else (0, 0, 0)
        self._four_cfg = (0, 0)  # (a probe configuration drops the Fourier one)

    def arm_probes(self):
        self._chk(getattr(lib(), self._prefix + "arm_probes")(self._h))

    def probe_samples(self, first=0, count=None):
        """(t [count][capacity], v [count][capacity][n_probes], n_recorded [count], n_dropped [count]); slots past n_recorded are NaN"""
        count = self.batch - first if count is None else count
        n_p, cap, _ = self._probe_cfg
        t = np.empty((count, cap))
        v = np.empty((count, cap, n_p))
        n_rec = np.empty(count, dtype=np.int32)
        n_drop = np.empty(count, dtype=np.int64)
        self._chk(getattr(lib(), self._prefix + "get_probe_samples")(self._h, int(first), int(count), _dp(t), _dp(v), _ip(n_rec),
                                                            n_drop.ctypes.data_as(C.POINTER(C.c_longlong))))
        return t, v, n_rec, n_drop

    def measures(self, first=0, count=None):
        """[count][n_measures][2] (include/pe_hip.h: value, then time / T / crossings seen)"""
        count = self.batch - first if count is None else count
        out = np.empty((count, self._probe_cfg[2], 2))
        self._chk(getattr(lib(), self._prefix + "get_measures")(self._h, int(first), int(count), _dp(out)))
        return out

    def set_fourier(self, f0=None, t_start=0.0, n_periods=1, n_harmonics=9, probes=()):
        """harmonics 0 .. n_harmonics of f0 over [t_start, t_start + n_periods / f0] of the probes `probes` (indices into the probe list),
        accumulated on the device at every accepted step of an armed window (include/pe_hip.h); probes=() removes the analysis.  Ends an
        armed window like set_probes: arm again."""
        p = np.ascontiguousarray(probes, dtype=np.int32).reshape(-1)
        fn = getattr(lib(), self._prefix + "set_fourier")
        if len(p) == 0:
            self._chk(fn(self._h, None))
            self._four_cfg = (0, 0)
            return
        c = FourierControl(float(f0), float(t_start), int(n_periods), int(n_harmonics), len(p), _ip(p))
        self._chk(fn(self._h, C.byref(c)))
        self._four_cfg = (len(p), int(n_harmonics))

    def fourier(self, first=0, count=None):
        """(coef [count][n_probes][H + 1][4] = a, b, amp, phase; thd [count][n_probes]; covered [count]) -- NaN where nothing was integrated"""
        count = self.batch - first if count is None else count
        n_p, H = self._four_cfg
        coef = np.empty((count, n_p, H + 1, 4))
        thd = np.empty((count, n_p))
        cov = np.empty(count)
        self._chk(getattr(lib(), self._prefix + "get_fourier")(self._h, int(first), int(count), _dp(coef), _dp(thd), _dp(cov)))
        return coef, thd, cov


class RunStats(C.Structure):
    _fields_ = [("steps", C.c_longlong), ("newton_iters", C.c_longlong), ("gpu_ms", C.c_double), ("n_launches", C.c_int),
                ("n_failed", C.c_int), ("dominant_ms", C.c_double), ("dominant_launches", C.c_int)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TrControl(C.Structure):
    _fields_ = [("dt_init", C.c_double), ("dt_min", C.c_double), ("dt_max", C.c_double), ("lte_reltol", C.c_double), ("lte_abstol_v", C.c_double),
                ("lte_abstol_i", C.c_double), ("trtol", C.c_double), ("max_steps", C.c_longlong), ("source_breakpoints", C.c_int),
                ("n_breakpoints", C.c_int), ("breakpoints", C.POINTER(C.c_double))]


class TrAdaptiveStats(C.Structure):
    _fields_ = [("n_accepted", C.c_longlong), ("n_rejected_lte", C.c_longlong), ("n_rejected_newton", C.c_longlong), ("n_at_dt_min", C.c_longlong),
                ("newton_iters_rejected", C.c_longlong), ("n_analyses", C.c_int), ("dt_smallest", C.c_double), ("dt_largest", C.c_double),
                ("t_end", C.c_double), ("run", RunStats)]

    def asdict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "run"}
        d["run"] = self.run.asdict()
        return d


class AcSweepStats(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_passes", C.c_int), ("points_per_pass", C.c_int), ("n_analyses", C.c_int), ("n_refine_rounds", C.c_int),
                ("n_fallback_points", C.c_int), ("gpu_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DcSweepControl(C.Structure):
    _fields_ = [("kind", C.c_int), ("index", C.c_int), ("column", C.c_int), ("mode", C.c_int), ("order", C.c_int), ("continuation", C.c_int),
                ("max_rounds", C.c_int)]


class DcSweepStats(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_passes", C.c_int), ("points_per_pass", C.c_int), ("n_rounds", C.c_int), ("n_failed_cold", C.c_longlong),
                ("n_reseeded", C.c_longlong), ("n_failed", C.c_longlong), ("newton_iters", C.c_longlong), ("n_analyses", C.c_int), ("gpu_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class OpStepControl(C.Structure):
    _fields_ = [("method", C.c_int), ("max_levels", C.c_int), ("step_max_newton", C.c_int), ("log_capacity", C.c_int), ("dl_init", C.c_double),
                ("grow", C.c_double), ("shrink", C.c_double), ("dl_min", C.c_double), ("g_start", C.c_double)]


class OpStepStats(C.Structure):
    _fields_ = [("n_levels", C.c_longlong), ("n_accepted", C.c_longlong), ("n_rejected", C.c_longlong), ("n_direct", C.c_int), ("n_gmin", C.c_int),
                ("n_source", C.c_int), ("n_failed", C.c_int), ("newton_iters", C.c_longlong), ("n_solves", C.c_int), ("n_launches", C.c_int),
                ("gpu_ms", C.c_double), ("control_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def op_step_control(method=STEP_AUTO, max_levels=0, step_max_newton=0, log_capacity=256, dl_init=0.0, grow=0.0, shrink=0.0, dl_min=0.0, g_start=0.0):
    """pe_hip_op_step_control; a field left at 0 takes the default of include/pe_hip.h"""
    return OpStepControl(int(method), int(max_levels), int(step_max_newton), int(log_capacity), float(dl_init), float(grow), float(shrink),
                         float(dl_min), float(g_start))


class NoiseControl(C.Structure):
    _fields_ = [("out_pos", C.c_int), ("out_neg", C.c_int), ("temp_k", C.c_double), ("keep_contributions", C.c_int)]


class NoiseStats(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_sources", C.c_int), ("n_passes", C.c_int), ("points_per_pass", C.c_int), ("n_analyses", C.c_int),
                ("n_refine_rounds", C.c_int), ("n_retried_points", C.c_int), ("gpu_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SensControl(C.Structure):
    _fields_ = [("n_outputs", C.c_int), ("out_pos", C.POINTER(C.c_int)), ("out_neg", C.POINTER(C.c_int)), ("normalized", C.c_int),
                ("keep_sensitivities", C.c_int), ("weight", C.POINTER(C.c_double))]


class SensStats(C.Structure):
    _fields_ = [("n_outputs", C.c_int), ("n_params", C.c_int), ("n_passes", C.c_int), ("outputs_per_pass", C.c_int), ("n_analyses", C.c_int),
                ("n_refine_rounds", C.c_int), ("n_retried_outputs", C.c_int), ("gpu_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class NetControl(C.Structure):
    _fields_ = [("n_ports", C.c_int), ("port_pos", C.POINTER(C.c_int)), ("port_neg", C.POINTER(C.c_int)), ("z0", C.POINTER(C.c_double))]


class NetStats(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_ports", C.c_int), ("n_passes", C.c_int), ("points_per_pass", C.c_int), ("n_analyses", C.c_int),
                ("n_factorisations", C.c_int), ("n_solves", C.c_int), ("n_refine_rounds", C.c_int), ("n_retried_points", C.c_int),
                ("gpu_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PzControl(C.Structure):
    _fields_ = [("what", C.c_int), ("omega0", C.c_double), ("n_wanted", C.c_int), ("max_krylov", C.c_int), ("tol", C.c_double),
                ("theta_floor", C.c_double), ("breakdown_tol", C.c_double), ("in_pos", C.c_int), ("in_neg", C.c_int), ("out_pos", C.c_int),
                ("out_neg", C.c_int)]


class PzStats(C.Structure):
    _fields_ = [("n_steps", C.c_int), ("n_factorisations", C.c_int), ("n_solves", C.c_int), ("n_refine_rounds", C.c_int), ("n_complete", C.c_int),
                ("gpu_ms", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run `make -C phy-engine_amd/csrc` (or __graft_entry__.build())")
        l = C.CDLL(LIB_PATH)
        l.pe_hip_last_error.restype = C.c_char_p
        l.pe_hip_last_error.argtypes = [C.c_void_p]
        l.pe_hip_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        l.pe_hip_destroy.argtypes = [C.c_void_p]
        l.pe_hip_destroy.restype = None
        l.pe_hip_load_circuit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DeviceTable)]
        l.pe_hip_set_options.argtypes = [C.c_void_p, C.POINTER(Options)]
        l.pe_hip_get_info.argtypes = [C.c_void_p, C.POINTER(Info)]
        l.pe_hip_get_front_table.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 9
        l.pe_hip_get_static_fronts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        l.pe_hip_get_static_skip_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        l.pe_hip_get_static_skip_refinement_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        l.pe_hip_set_digital_drives.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]
        l.pe_hip_update_param.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int]
        l.pe_hip_reset.argtypes = [C.c_void_p]
        l.pe_hip_analyze_dc.argtypes = [C.c_void_p, C.c_int, C.POINTER(RunStats)]
        l.pe_hip_analyze_tr.argtypes = [C.c_void_p, C.c_double, C.c_int, C.POINTER(RunStats)]
        l.pe_hip_get_solution.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        l.pe_hip_set_solution.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        l.pe_hip_sweep_statistics.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        l.pe_hip_get_safety_net_counters.argtypes = [C.c_void_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
        l.pe_hip_measure_hbm_ceiling.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
        l.pe_hip_get_instance_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_longlong),
                                                C.POINTER(C.c_longlong), C.POINTER(C.c_double)]
        l.pe_hip_get_newton_trace.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        l.pe_hip_get_matrix.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]
        l.pe_hip_solve_csr_real.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                                            C.POINTER(Timings)]
        l.pe_hip_solve_csr_complex.argtypes = l.pe_hip_solve_csr_real.argtypes
        l.pe_hip_build_id.restype = C.c_char_p
        l.pe_hip_build_id.argtypes = []
        l.pe_hip_analyze_pattern.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(Info)]
        _probe_argtypes(l, "pe_hip_")
        _probe_argtypes(l, "pe_hip_sweep_")
        l.pe_hip_set_ac_sweep_rows.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.pe_hip_analyze_ac_sweep.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(AcSweepStats)]
        l.pe_hip_get_ac_sweep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.pe_hip_get_matrix_ac.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                           C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        l.pe_hip_get_ac_pass_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.pe_hip_analyze_noise.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(NoiseControl), C.POINTER(C.c_int), C.POINTER(NoiseStats)]
        l.pe_hip_get_noise.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.pe_hip_get_noise_sources.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 6
        l.pe_hip_get_noise_source_density.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        l.pe_hip_get_noise_integrated.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        l.pe_hip_get_sens_params.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 4
        l.pe_hip_analyze_sens.argtypes = [C.c_void_p, C.POINTER(SensControl), C.POINTER(C.c_int), C.POINTER(SensStats)]
        l.pe_hip_get_sens.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.pe_hip_analyze_net.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(NetControl), C.POINTER(C.c_int), C.POINTER(NetStats)]
        l.pe_hip_get_net.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.pe_hip_get_net_status.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        l.pe_hip_convert_net.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_double)] * 7 + [C.POINTER(C.c_int)] * 2
        l.pe_hip_analyze_pz.argtypes = [C.c_void_p, C.POINTER(PzControl), C.POINTER(C.c_int), C.POINTER(PzStats)]
        l.pe_hip_get_pz.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_double)] * 3 + [C.POINTER(C.c_int)] * 3
        l.pe_hip_get_pz_gain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        l.pe_hip_eig_hessenberg.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_double)] * 6 + [C.POINTER(C.c_int)]
        l.pe_hip_set_dc_sweep_rows.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        l.pe_hip_analyze_dc_sweep.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(DcSweepControl), C.POINTER(C.c_int), C.POINTER(DcSweepStats)]
        l.pe_hip_get_dc_sweep.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
        l.pe_hip_get_dc_sweep_status.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3
        l.pe_hip_analyze_op_stepping.argtypes = [C.c_void_p, C.c_int, C.POINTER(OpStepControl), C.POINTER(OpStepStats)]
        l.pe_hip_get_op_step_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                               C.POINTER(C.c_longlong)]
        l.pe_hip_get_op_step_log.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                             C.POINTER(C.c_int), C.POINTER(C.c_int)]
        l.pe_hip_sweep_operating_point_stepping.argtypes = [C.c_void_p, C.c_int, C.POINTER(OpStepControl), C.POINTER(OpStepStats)]
        l.pe_hip_analyze_tr_adaptive.argtypes = [C.c_void_p, C.c_double, C.POINTER(TrControl), C.POINTER(TrAdaptiveStats)]
        l.pe_hip_get_tr_step_log.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]
        l.pe_hip_set_tr_method.argtypes = [C.c_void_p, C.c_int]
        l.pe_hip_get_tr_method.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        l.pe_hip_get_tr_history.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        _lib = l
    return _lib


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class PeHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pe_hip error {code}: {msg}")
        self.code = code


def analyze_pattern(n, row_ptr, col_ind, values=None):
    """Host-only symbolic analysis statistics (no GPU needed)."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    ci = np.ascontiguousarray(col_ind, dtype=np.int32)
    info = Info()
    vals = None if values is None else np.ascontiguousarray(values, dtype=np.float64)
    rc = lib().pe_hip_analyze_pattern(int(n), _ip(rp), _ip(ci), None if vals is None else _dp(vals), C.byref(info))
    if rc != 0:
        raise PeHipError(rc, "analyze_pattern failed")
    return info.asdict()


def deck_tables(deck, batch=1, overrides=None, n_drives=0):
    """Deck -> (n_nodes, n_branches, [(kind, nodes[int32 count x 2], branch[int32]|None, params[f64], batched)]).

    Branch indices follow circult::prepare (circuit.h:509-531): digital drives first, then models in order.
    `overrides`: {kind_name: array [batch][count][ncol]} per-instance parameters (Monte-Carlo sweeps).
    FBR devices expand to their four PN junctions (full_bridge_rectifier.h:19-50) with tt_in_tr = 0.
    """
    overrides = overrides or {}
    from .deck import NBRANCH, VGEN_LAYOUT
    names = tuple(NCOL)
    unknown = sorted(set(overrides) - set(names))
    if unknown:
        raise ValueError(f"overrides for unknown kinds {unknown}: the tables are {names}")
    groups = {k: {"nodes": [], "branch": [], "par": []} for k in names}
    k = n_drives
    for kind, nodes, par in deck.devices:
        if kind == "FBR":
            A, B, P, M = nodes
            dflt = (1e-14, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 1.0, 1.0, 0.0, 0.0)
            for (a, c) in ((A, P), (B, P), (M, A), (M, B)):
                groups["D"]["nodes"].append((a, c))
                groups["D"]["par"].append(dflt)
            continue
        nb = NBRANCH[kind]
        if kind in VGEN_LAYOUT:
            ty, pos = VGEN_LAYOUT[kind]
            dflt = (5.0, 0.0, 1e3, 0.5, 0.0, 0.0, 0.0)
            par = (float(ty),) + tuple(par[q] if q >= 0 else dflt[j] for j, q in enumerate(pos))
            kind = "VGEN"
        g = groups[kind]
        g["nodes"].append(nodes)
        g["par"].append(tuple(par) + ((1.0,) if kind == "D" else ()))
        for _ in range(nb):
            g["branch"].append(k)
            k += 1
    code = KIND_CODE
    tables = []
    for name, g in groups.items():
        if not g["nodes"]:
            continue
        nodes = np.ascontiguousarray(np.array(g["nodes"], dtype=np.int32))
        branch = np.ascontiguousarray(np.array(g["branch"], dtype=np.int32)) if g["branch"] else None
        if name in overrides:
            par = np.ascontiguousarray(overrides[name], dtype=np.float64)
            if par.shape != (batch, len(nodes), NCOL[name]):
                raise ValueError(f"overrides[{name!r}] has shape {par.shape}: the {name} table of this deck and batch is "
                                 f"[{batch}][{len(nodes)}][{NCOL[name]}]")
            batched = 1
        else:
            par = np.ascontiguousarray(np.array(g["par"], dtype=np.float64))
            batched = 0
        tables.append((code[name], nodes, branch, par, batched))
    return deck.n_nodes, k, tables


def analyze_pattern_fronts(n, row_ptr, col_ind, values=None):
    """Host-only: (pivots, updates, parent) arrays of the assembly tree, fronts in postorder."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    ci = np.ascontiguousarray(col_ind, dtype=np.int32)
    vals = None if values is None else np.ascontiguousarray(values, dtype=np.float64)
    cap = max(1, int(n))
    p = np.zeros(cap, dtype=np.int32)
    u = np.zeros(cap, dtype=np.int32)
    par = np.zeros(cap, dtype=np.int32)
    nf = C.c_int()
    fn = lib().pe_hip_analyze_pattern_fronts
    fn.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                   C.POINTER(C.c_int), C.POINTER(C.c_int)]
    rc = fn(int(n), _ip(rp), _ip(ci), None if vals is None else _dp(vals), cap, _ip(p), _ip(u), _ip(par), C.byref(nf))
    if rc != 0:
        raise PeHipError(rc, "analyze_pattern_fronts failed")
    k = nf.value
    return p[:k].copy(), u[:k].copy(), par[:k].copy()


class Engine(_Probes):
    """One resident circuit (optionally a batch of parameter instances) on one GPU."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().pe_hip_create(int(device), C.byref(self._h))
        if rc != 0:
            raise PeHipError(rc, lib().pe_hip_last_error(None).decode())
        self.rows = 0
        self.batch = 1
        self._keep = []

    def close(self):
        if self._h:
            lib().pe_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, allow=()):
        if rc != 0 and rc not in allow:
            raise PeHipError(rc, lib().pe_hip_last_error(self._h).decode())
        return rc

    def set_options(self, g_min=0.0, v_abstol=0.0, v_reltol=0.0, i_abstol=0.0, i_reltol=0.0, max_newton=0, refactor_every_solve=1, r_open=0.0, residual_tol=0.0):
        o = Options(v_abstol, v_reltol, i_abstol, i_reltol, g_min, max_newton, refactor_every_solve, r_open, residual_tol)
        self._chk(lib().pe_hip_set_options(self._h, C.byref(o)))

    def set_knob(self, name, value):
        """one of the PHY_ENGINE_HIP_* tuning knobs for THIS engine; takes effect at the next analysis"""
        self._chk(lib().pe_hip_set_knob(self._h, name.encode(), int(value)))

    def get_knob(self, name):
        v, s = C.c_int(0), C.c_int(0)
        self._chk(lib().pe_hip_get_knob(self._h, name.encode(), C.byref(v), C.byref(s)))
        return v.value if s.value else None

    def set_digital_drives(self, nodes, volts):
        n = np.ascontiguousarray(nodes, dtype=np.int32)
        v = np.ascontiguousarray(volts, dtype=np.float64)
        self._chk(lib().pe_hip_set_digital_drives(self._h, len(n), _ip(n), _dp(v)))

    def load(self, n_nodes, n_branches, tables, batch=1):
        arr = (DeviceTable * max(1, len(tables)))()
        self._keep = list(tables)
        for i, (kind, nodes, branch, par, batched) in enumerate(tables):
            arr[i] = DeviceTable(kind, len(nodes), _ip(nodes), None if branch is None else _ip(branch), _dp(par), batched)
        self._chk(lib().pe_hip_load_circuit(self._h, int(n_nodes), int(n_branches), int(batch), len(tables), arr))
        self.rows = n_nodes + n_branches
        self.batch = batch
        self._probe_cfg = (0, 0, 0)  # (a load drops the probe configuration)
        self._four_cfg = (0, 0)
        self._ac_rows = None         # (... and the row selection of AC sweeps)
        self._dc_rows = None         # (... and of DC sweeps)

    def load_deck(self, deck, batch=1, overrides=None, n_drives=0):
        n_nodes, n_br, tables = deck_tables(deck, batch, overrides, n_drives)
        self.load(n_nodes, n_br, tables, batch)

    def info(self):
        i = Info()
        self._chk(lib().pe_hip_get_info(self._h, C.byref(i)))
        return i.asdict()

    def front_table(self, which=0):
        """the fronts of an analysis this engine holds, in postorder: dict of int32 arrays p, u, parent, kind (0 wave, 1 cooperative, 2 top),
        quad, mode, n_children, n_own (pe_hip_get_front_table).  which: 0 the resident circuit, 1 / 2 the last solve_csr / solve_csr_complex"""
        n = C.c_int()
        self._chk(lib().pe_hip_get_front_table(self._h, int(which), 0, *[None] * 8, C.byref(n)))
        names = ("p", "u", "parent", "kind", "quad", "mode", "n_children", "n_own")
        out = {k: np.zeros(n.value, dtype=np.int32) for k in names}
        self._chk(lib().pe_hip_get_front_table(self._h, int(which), n.value, *[_ip(out[k]) for k in names], C.byref(n)))
        return out

    def static_fronts(self, which=0):
        """int32 array in the order of front_table(which): 1 = the front's whole subtree holds no x-dependent entry or row (pe_hip_get_static_fronts)"""
        n = C.c_int()
        self._chk(lib().pe_hip_get_static_fronts(self._h, int(which), 0, None, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        self._chk(lib().pe_hip_get_static_fronts(self._h, int(which), n.value, _ip(out), C.byref(n)))
        return out

    def static_skip_stats(self):
        """lane-group factor launches since load: {'skipped_launches': without the static fronts, 'full_launches': the others}"""
        a, b = C.c_longlong(), C.c_longlong()
        self._chk(lib().pe_hip_get_static_skip_stats(self._h, C.byref(a), C.byref(b)))
        c, d = C.c_longlong(), C.c_longlong()
        self._chk(lib().pe_hip_get_static_skip_refinement_stats(self._h, C.byref(c), C.byref(d)))
        return {"skipped_launches": a.value, "full_launches": b.value, "launches_after_refinement": c.value, "skipped_after_refinement": d.value}

    def reset(self):
        self._chk(lib().pe_hip_reset(self._h))

    def analyze_tr(self, dt, nsteps, check=True):
        st = RunStats()
        rc = lib().pe_hip_analyze_tr(self._h, float(dt), int(nsteps), C.byref(st))
        if check:
            self._chk(rc)
        d = st.asdict()
        d["rc"] = rc
        return d

    def analyze_tr_adaptive(self, t_stop, dt_init, dt_min=0.0, dt_max=0.0, lte_reltol=0.0, lte_abstol_v=0.0, lte_abstol_i=0.0, trtol=0.0,
                            max_steps=0, source_breakpoints=False, breakpoints=(), check=True):
        """Variable-step transient up to the absolute time t_stop (pe_hip_analyze_tr_adaptive): the step follows the local truncation
        error and is cut when Newton fails; 0 / omitted arguments take the defaults of include/pe_hip.h, a negative lte_reltol switches
        the LTE test off.  Returns the statistics as a dict, the run statistics under 'run' and the return code under 'rc'."""
        bp = np.ascontiguousarray(breakpoints, dtype=np.float64).reshape(-1)
        c = TrControl(float(dt_init), float(dt_min), float(dt_max), float(lte_reltol), float(lte_abstol_v), float(lte_abstol_i), float(trtol),
                      int(max_steps), 1 if source_breakpoints else 0, len(bp), _dp(bp) if len(bp) else None)
        st = TrAdaptiveStats()
        rc = lib().pe_hip_analyze_tr_adaptive(self._h, float(t_stop), C.byref(c), C.byref(st))
        if check:
            self._chk(rc)
        d = st.asdict()
        d["rc"] = rc
        return d

    def tr_step_log(self):
        """(dt [n], outcome [n]) of every attempted step of the last adaptive call: 0 accepted, 1 rejected by the LTE test, 2 by Newton"""
        n = C.c_longlong(0)
        self._chk(lib().pe_hip_get_tr_step_log(self._h, 0, 0, None, None, C.byref(n)))
        dt = np.empty(n.value)
        oc = np.empty(n.value, dtype=np.int32)
        if n.value:
            self._chk(lib().pe_hip_get_tr_step_log(self._h, 0, int(n.value), _dp(dt), _ip(oc), C.byref(n)))
        return dt, oc

    def set_tr_method(self, method):
        """integration rule of the transient: TR_TRAP (default), TR_BE or TR_GEAR2, or 'trap' / 'be' / 'gear2' (pe_hip_set_tr_method); an
        engine setting that survives load_deck.  A change restarts the integration history of every instance."""
        m = _TR_NAMES[method.lower()] if isinstance(method, str) else int(method)
        self._chk(lib().pe_hip_set_tr_method(self._h, m))

    @property
    def tr_method(self):
        m = C.c_int(0)
        self._chk(lib().pe_hip_get_tr_method(self._h, C.byref(m)))
        return m.value

    def tr_history(self, first=0, count=None):
        """h_p [count]: the step the second history point of every instance belongs to; 0: its next step starts the history (always under TRAP)"""
        count = self.batch - first if count is None else count
        out = np.empty(count)
        self._chk(lib().pe_hip_get_tr_history(self._h, int(first), int(count), _dp(out)))
        return out

    def analyze_dc(self, mode=MODE_DC, check=True):
        st = RunStats()
        rc = lib().pe_hip_analyze_dc(self._h, int(mode), C.byref(st))
        if check:
            self._chk(rc)
        d = st.asdict()
        d["rc"] = rc
        return d

    def solution(self, first=0, count=None):
        count = self.batch - first if count is None else count
        x = np.empty((count, self.rows))
        self._chk(lib().pe_hip_get_solution(self._h, first, count, _dp(x)))
        return x

    def safety_net(self):
        """{'refined': solves repaired by refinement, 'rematched': symbolic re-analyses, 'careful': host-driven schedule forced}."""
        a, b, c = C.c_longlong(0), C.c_longlong(0), C.c_int(0)
        self._chk(lib().pe_hip_get_safety_net_counters(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"refined": a.value, "rematched": b.value, "careful": bool(c.value)}

    def measure_hbm_ceiling(self, nbytes=1 << 31, reps=5):
        """GB/s of a device-to-device stream copy on this engine's GPU (read + written bytes / HIP-event time)."""
        g = C.c_double(0.0)
        self._chk(lib().pe_hip_measure_hbm_ceiling(self._h, C.c_size_t(nbytes), int(reps), C.byref(g)))
        return g.value

    def sweep_statistics(self):
        """[4][rows]: sum, sum of squares, min, max of the current solution over this engine's instances (computed on the device)."""
        out = np.empty((4, self.rows))
        self._chk(lib().pe_hip_sweep_statistics(self._h, _dp(out)))
        return out

    def set_solution(self, x, first=0):
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.rows)
        self._chk(lib().pe_hip_set_solution(self._h, first, len(x), _dp(x)))

    def state(self):
        st = np.empty(self.batch, dtype=np.int32)
        steps = np.empty(self.batch, dtype=np.int64)
        iters = np.empty(self.batch, dtype=np.int64)
        t = np.empty(self.batch)
        self._chk(lib().pe_hip_get_instance_state(self._h, 0, self.batch, _ip(st), steps.ctypes.data_as(C.POINTER(C.c_longlong)),
                                                  iters.ctypes.data_as(C.POINTER(C.c_longlong)), _dp(t)))
        return {"status": st, "steps": steps, "iters": iters, "t": t}

    def newton_trace(self, capacity=1 << 16):
        buf = np.zeros(capacity, dtype=np.int32)
        n = C.c_int()
        self._chk(lib().pe_hip_get_newton_trace(self._h, capacity, _ip(buf), C.byref(n)))
        return buf[:min(n.value, capacity)].copy()

    def matrix(self, instance=0):
        info = self.info()
        rp = np.empty(self.rows + 1, dtype=np.int32)
        ci = np.empty(info["nnz_a"], dtype=np.int32)
        va = np.empty(info["nnz_a"])
        rhs = np.empty(self.rows)
        self._chk(lib().pe_hip_get_matrix(self._h, instance, _ip(rp), _ip(ci), _dp(va), _dp(rhs)))
        return rp, ci, va, rhs

    def phase_clocks(self, instance=0):
        """In-kernel phase times of one instance since reset(), in microseconds (see pe_hip_get_phase_clocks)."""
        t = np.zeros(8, dtype=np.int64)
        fn = lib().pe_hip_get_phase_clocks
        fn.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong)]
        self._chk(fn(self._h, instance, t.ctypes.data_as(C.POINTER(C.c_longlong))))
        names = ["eval_stamp", "lu_wave", "lu_coop", "backward_coop", "newton", "backward", "coop_asm", "coop_piv"]
        return {n: float(t[i]) / 100.0 for i, n in enumerate(names)}

    def checkpoint(self) -> bytes:
        """Device-resident simulation state of every instance as one blob (pe_hip_checkpoint_save)."""
        n = C.c_size_t()
        lib().pe_hip_checkpoint_size.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        self._chk(lib().pe_hip_checkpoint_size(self._h, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        lib().pe_hip_checkpoint_save.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        self._chk(lib().pe_hip_checkpoint_save(self._h, buf, n.value))
        return buf.raw

    def restore(self, blob: bytes):
        lib().pe_hip_checkpoint_load.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
        self._chk(lib().pe_hip_checkpoint_load(self._h, blob, len(blob)))

    def analyze_ac(self, omega, check=True):
        """Small-signal AC at `omega` rad/s; returns the complex solution [batch][rows]."""
        st = RunStats()
        fn = lib().pe_hip_analyze_ac
        fn.argtypes = [C.c_void_p, C.c_double, C.POINTER(RunStats)]
        rc = fn(self._h, float(omega), C.byref(st))
        if check:
            self._chk(rc)
        re = np.empty((self.batch, self.rows))
        im = np.empty((self.batch, self.rows))
        if rc == 0:
            g = lib().pe_hip_get_solution_ac
            g.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
            self._chk(g(self._h, 0, self.batch, _dp(re), _dp(im)))
        return re + 1j * im, rc

    def set_ac_sweep_rows(self, rows=None):
        """rows of x kept for every point of the following analyze_ac_sweep calls; None / empty: all rows"""
        r = np.ascontiguousarray([] if rows is None else rows, dtype=np.int32).reshape(-1)
        self._chk(lib().pe_hip_set_ac_sweep_rows(self._h, len(r), _ip(r) if len(r) else None))
        self._ac_rows = len(r) if len(r) else None

    def analyze_ac_sweep(self, omegas, check=True):
        """Small-signal AC at every omega of `omegas` (rad/s, any order) in batched passes on the device (pe_hip_analyze_ac_sweep).
        Returns (x [n_points][batch][n_kept] complex in the caller's order -- NaN where a point failed --, status [n_points], stats dict
        with the return code under 'rc')."""
        w = np.ascontiguousarray(omegas, dtype=np.float64).reshape(-1)
        n = len(w)
        status = np.zeros(max(n, 1), dtype=np.int32)
        st = AcSweepStats()
        rc = lib().pe_hip_analyze_ac_sweep(self._h, n, _dp(w), _ip(status), C.byref(st))
        if check:
            self._chk(rc)
        kept = self._ac_rows if getattr(self, "_ac_rows", None) else self.rows
        re = np.full((n, self.batch, kept), np.nan)
        im = np.full((n, self.batch, kept), np.nan)
        if rc not in (ERR_ARG, ERR_NO_DEVICE, ERR_INTERNAL) and n:
            self._chk(lib().pe_hip_get_ac_sweep(self._h, 0, n, 0, self.batch, _dp(re), _dp(im)))
        d = st.asdict()
        d["rc"] = rc
        return re + 1j * im, status[:n], d

    def matrix_ac(self, which=0, instance=0, rhs=True):
        """(row_ptr, col_ind, vals, rhs) of a small-signal system as the device last assembled it (pe_hip_get_matrix_ac): the 2N
        real-equivalent system of the single-point engine (which 0), of instance q = b * P + p of the sweep's last pass (1), of the noise
        analysis' adjoint engines (2 / 3), of the batched adjoint engine of the last analyze_sens pass (4).  rhs: as stamped, or None with rhs=False."""
        n, nz = C.c_int(), C.c_int()
        self._chk(lib().pe_hip_get_matrix_ac(self._h, int(which), int(instance), 0, None, None, None, None, C.byref(n), C.byref(nz)))
        rp = np.empty(n.value + 1, dtype=np.int32)
        ci = np.empty(nz.value, dtype=np.int32)
        va = np.empty(nz.value)
        b = np.empty(n.value) if rhs else None
        self._chk(lib().pe_hip_get_matrix_ac(self._h, int(which), int(instance), nz.value, _ip(rp), _ip(ci), _dp(va), _dp(b) if rhs else None,
                                             C.byref(n), C.byref(nz)))
        return rp, ci, va, b

    def ac_analysis_omega(self):
        """omega whose values the single-point AC engine's pivot order was last matched on (-1.0: none yet)"""
        w = C.c_double()
        fn = lib().pe_hip_get_ac_analysis_omega
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._chk(fn(self._h, C.byref(w)))
        return w.value

    def ac_pass_size(self, which=1):
        """points per pass P of the batched engine of the last analyze_ac_sweep (which 1) or analyze_noise (3)"""
        p = C.c_int()
        self._chk(lib().pe_hip_get_ac_pass_size(self._h, int(which), C.byref(p)))
        return p.value

    def analyze_op_stepping(self, mode=MODE_OP, method=STEP_AUTO, check=True, **control):
        """operating point with gmin / source stepping where the direct attempt fails (pe_hip_analyze_op_stepping); control: the fields of
        pe_hip_op_step_control (op_step_control).  Returns the statistics + "rc"."""
        st = OpStepStats()
        ctl = op_step_control(method, **control)
        rc = lib().pe_hip_analyze_op_stepping(self._h, int(mode), C.byref(ctl), C.byref(st))
        if check:
            self._chk(rc)
        return dict(st.asdict(), rc=rc)

    def op_step_state(self):
        """per instance of the last analyze_op_stepping: phase_solved_in (0 direct, 1 gmin, 2 source, -1 failed), lambda_reached, levels,
        rejected, newton_iters"""
        B = self.batch
        ph, lv, rj = (np.zeros(B, dtype=np.int32) for _ in range(3))
        lam = np.zeros(B)
        it = np.zeros(B, dtype=np.int64)
        self._chk(lib().pe_hip_get_op_step_state(self._h, 0, B, _ip(ph), _dp(lam), _ip(lv), _ip(rj), it.ctypes.data_as(C.POINTER(C.c_longlong))))
        return {"phase_solved_in": ph, "lambda_reached": lam, "levels": lv, "rejected": rj, "newton_iters": it}

    def op_step_log(self, instance):
        """the device-side log of one instance: phase, lambda, value, outcome, iters per level solved (as many as log_capacity kept) + n_total"""
        n = C.c_int()
        self._chk(lib().pe_hip_get_op_step_log(self._h, int(instance), 0, None, None, None, None, None, C.byref(n)))
        k = n.value
        ph, oc, it = (np.zeros(k, dtype=np.int32) for _ in range(3))
        lam, val = np.zeros(k), np.zeros(k)
        self._chk(lib().pe_hip_get_op_step_log(self._h, int(instance), k, _ip(ph), _dp(lam), _dp(val), _ip(oc), _ip(it), C.byref(n)))
        return {"phase": ph, "lambda": lam, "value": val, "outcome": oc, "iters": it, "n_total": n.value}

    def set_dc_sweep_rows(self, rows=None):
        """rows of x kept for every point of the following analyze_dc_sweep calls; None / empty: all rows"""
        r = np.ascontiguousarray([] if rows is None else rows, dtype=np.int32).reshape(-1)
        self._chk(lib().pe_hip_set_dc_sweep_rows(self._h, len(r), _ip(r) if len(r) else None))
        self._dc_rows = len(r) if len(r) else None

    def analyze_dc_sweep(self, values, kind, index, column=0, mode=MODE_OP, order=DC_SWEEP_PARALLEL, continuation=1, max_rounds=0, check=True):
        """The operating point at every value of `values` (any order) of parameter (kind, index, column) in batched passes on the device
        (pe_hip_analyze_dc_sweep); this engine's own state is read, never written.  Returns (x [n_points][batch][n_kept] in the caller's
        order -- NaN where a pair failed --, status [n_points], stats dict with the return code under 'rc')."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        n = len(v)
        status = np.zeros(max(n, 1), dtype=np.int32)
        st = DcSweepStats()
        ctl = DcSweepControl(int(kind), int(index), int(column), int(mode), int(order), int(continuation), int(max_rounds))
        rc = lib().pe_hip_analyze_dc_sweep(self._h, n, _dp(v), C.byref(ctl), _ip(status), C.byref(st))
        if check:
            self._chk(rc)
        kept = self._dc_rows if getattr(self, "_dc_rows", None) else self.rows
        x = np.full((n, self.batch, kept), np.nan)
        if rc not in (ERR_ARG, ERR_NO_DEVICE, ERR_INTERNAL) and n:
            self._chk(lib().pe_hip_get_dc_sweep(self._h, 0, n, 0, self.batch, _dp(x)))
            self._dc_n = n
        d = st.asdict()
        d["rc"] = rc
        return x, status[:n], d

    def dc_sweep_status(self):
        """per pair of the last DC sweep, each [n_points][batch]: status of its last attempt, Newton iterations of that attempt when it
        converged, and the caller's index of the point it was seeded from (-1: this engine's own state)"""
        n = getattr(self, "_dc_n", 0)
        out = [np.zeros((n, self.batch), dtype=np.int32) for _ in range(3)]
        if n:
            self._chk(lib().pe_hip_get_dc_sweep_status(self._h, 0, n, 0, self.batch, _ip(out[0]), _ip(out[1]), _ip(out[2])))
        return tuple(out)

    def analyze_noise(self, omegas, out_pos, out_neg=-1, temp_k=0.0, contributions=False, check=True):
        """Output noise density of x[out_pos] - x[out_neg] (rows of x, -1: ground) at every omega of `omegas` (rad/s, any order) by the
        adjoint method on the device (pe_hip_analyze_noise).  Returns (psd [n_points][batch], one-sided, V^2/Hz -- NaN where a point
        failed --, contrib [n_points][batch][n_sources] or None, status [n_points], stats dict with the return code under 'rc')."""
        w = np.ascontiguousarray(omegas, dtype=np.float64).reshape(-1)
        n = len(w)
        status = np.zeros(max(n, 1), dtype=np.int32)
        st = NoiseStats()
        ctl = NoiseControl(int(out_pos), int(out_neg), float(temp_k), 1 if contributions else 0)
        rc = lib().pe_hip_analyze_noise(self._h, n, _dp(w), C.byref(ctl), _ip(status), C.byref(st))
        if check:
            self._chk(rc)
        psd = np.full((n, self.batch), np.nan)
        contrib = np.full((n, self.batch, st.n_sources), np.nan) if contributions else None
        if rc not in (ERR_ARG, ERR_NO_DEVICE, ERR_INTERNAL) and n:
            self._chk(lib().pe_hip_get_noise(self._h, 0, n, 0, self.batch, _dp(psd), _dp(contrib) if contributions and st.n_sources else None))
        d = st.asdict()
        d["rc"] = rc
        return psd, contrib, status[:n], d

    def noise_sources(self):
        """the source table of the resident circuit: dict of int arrays kind (pe_hip_kind), index (in its table), part (BJT collector: 1),
        row_a, row_b (-1: ground), in the order of the contributions"""
        n = C.c_int()
        self._chk(lib().pe_hip_get_noise_sources(self._h, 0, None, None, None, None, None, C.byref(n)))
        out = {k: np.zeros(n.value, dtype=np.int32) for k in ("kind", "index", "part", "row_a", "row_b")}
        self._chk(lib().pe_hip_get_noise_sources(self._h, n.value, *[_ip(out[k]) for k in ("kind", "index", "part", "row_a", "row_b")], C.byref(n)))
        return out

    def noise_source_density(self):
        """current densities S_k of the last analyze_noise, [batch][n_sources], A^2/Hz"""
        n = C.c_int()
        self._chk(lib().pe_hip_get_noise_sources(self._h, 0, None, None, None, None, None, C.byref(n)))
        s = np.zeros((self.batch, n.value))
        self._chk(lib().pe_hip_get_noise_source_density(self._h, 0, self.batch, _dp(s)))
        return s

    def noise_integrated(self):
        """integrated output noise of the last analyze_noise over its band (trapezoidal rule in f), [batch], V^2"""
        v = np.zeros(self.batch)
        self._chk(lib().pe_hip_get_noise_integrated(self._h, 0, self.batch, _dp(v)))
        return v

    def sens_params(self):
        """the parameter table of the resident circuit (pe_hip_get_sens_params): dict of int arrays kind (pe_hip_kind), index (in its
        table), column (raw column as update_param names it), in the order of the sensitivities"""
        n = C.c_int()
        self._chk(lib().pe_hip_get_sens_params(self._h, 0, None, None, None, C.byref(n)))
        out = {k: np.zeros(n.value, dtype=np.int32) for k in ("kind", "index", "column")}
        self._chk(lib().pe_hip_get_sens_params(self._h, n.value, *[_ip(out[k]) for k in ("kind", "index", "column")], C.byref(n)))
        return out

    def analyze_sens(self, out_pos, out_neg=None, normalized=False, weight=None, keep=True, check=True):
        """First-order sensitivity of every output x[out_pos[o]] - x[out_neg[o]] (rows of x, -1 / None: ground) of the resident operating
        point to every parameter of sens_params() by the adjoint method on the device (pe_hip_analyze_sens).  Returns
        (s [n_outputs][batch][n_params] or None when not kept, rss [n_outputs][batch] = sum_k (weight_k s_k)^2 or None without weights,
        status [n_outputs], stats dict with the return code under 'rc'); a failed output reads NaN."""
        pos = np.ascontiguousarray(out_pos, dtype=np.int32).reshape(-1)
        neg = np.full(len(pos), -1, dtype=np.int32) if out_neg is None else np.ascontiguousarray(out_neg, dtype=np.int32).reshape(-1)
        if len(neg) != len(pos):
            raise ValueError("out_pos and out_neg differ in length")
        n = len(pos)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        n_par = C.c_int()
        self._chk(lib().pe_hip_get_sens_params(self._h, 0, None, None, None, C.byref(n_par)))
        if w is not None and len(w) != n_par.value:
            raise ValueError("weight needs one entry per parameter")
        status = np.zeros(max(n, 1), dtype=np.int32)
        st = SensStats()
        ctl = SensControl(n, _ip(pos) if n else None, _ip(neg) if n else None, 1 if normalized else 0, 1 if keep else 0,
                          _dp(w) if w is not None else None)
        rc = lib().pe_hip_analyze_sens(self._h, C.byref(ctl), _ip(status), C.byref(st))
        if check:
            self._chk(rc)
        s = np.full((n, self.batch, n_par.value), np.nan) if keep else None
        rss = np.full((n, self.batch), np.nan) if w is not None else None
        if rc not in (ERR_ARG, ERR_NO_DEVICE, ERR_INTERNAL) and n and (keep or w is not None):
            self._chk(lib().pe_hip_get_sens(self._h, 0, n, 0, self.batch, _dp(s) if keep and n_par.value else None, _dp(rss) if rss is not None else None))
        d = st.asdict()
        d["rc"] = rc
        return s, rss, status[:n], d

    def analyze_net(self, omegas, ports, z0=None, check=True):
        """Impedance, admittance and scattering matrices between the ports -- (pos, neg) pairs of rows of x, -1: ground -- at every omega of
        `omegas` (rad/s, any order) on the device (pe_hip_analyze_net); z0: reference resistance per port (None: 50 ohm each).  Returns
        (Z, Y, S complex [n_points][batch][n][n], entry [i][j] the response at port i to an excitation at port j, y_status and s_status
        [n_points][batch], point_status [n_points], stats dict with the return code under 'rc'); a failed point and a matrix without
        inverse read NaN."""
        w = np.ascontiguousarray(omegas, dtype=np.float64).reshape(-1)
        pr = np.ascontiguousarray(ports, dtype=np.int32).reshape(-1, 2)
        pos, neg = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        n, npt = len(pos), len(w)
        ref = None if z0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(z0, dtype=np.float64), (n,)))
        status = np.zeros(max(npt, 1), dtype=np.int32)
        st = NetStats()
        ctl = NetControl(n, _ip(pos) if n else None, _ip(neg) if n else None, _dp(ref) if ref is not None else None)
        rc = lib().pe_hip_analyze_net(self._h, npt, _dp(w), C.byref(ctl), _ip(status), C.byref(st))
        if check:
            self._chk(rc)
        mats = [np.full((npt, self.batch, n, n), np.nan + 0j) for _ in range(3)]
        ys = np.full((npt, self.batch), rc, dtype=np.int32)
        ss = np.full((npt, self.batch), rc, dtype=np.int32)
        if rc not in (ERR_ARG, ERR_NO_DEVICE, ERR_INTERNAL) and npt and n:
            re, im = np.empty((npt, self.batch, n, n)), np.empty((npt, self.batch, n, n))
            for which in (NET_Z, NET_Y, NET_S):
                self._chk(lib().pe_hip_get_net(self._h, which, 0, npt, 0, self.batch, _dp(re), _dp(im)))
                mats[which] = re + 1j * im
            self._chk(lib().pe_hip_get_net_status(self._h, 0, npt, 0, self.batch, _ip(ys), _ip(ss)))
        d = st.asdict()
        d["rc"] = rc
        return mats[0], mats[1], mats[2], ys, ss, status[:npt], d

    def convert_net(self, Z, z0=None):
        """Y = Z^-1 and S (power waves, real reference resistances z0, None: 50 ohm each) of caller-supplied impedance matrices
        Z complex [..., n, n] by the device kernel of analyze_net (pe_hip_convert_net; needs no circuit).  Returns (Y, S, y_status,
        s_status) shaped like Z / its leading dimensions; a matrix without inverse reads NaN with status ERR_SINGULAR."""
        Zc = np.asarray(Z, dtype=np.complex128)
        n = Zc.shape[-1]
        if Zc.ndim < 2 or Zc.shape[-2] != n:
            raise ValueError("Z must be [..., n, n]")
        lead = Zc.shape[:-2]
        m = int(np.prod(lead, dtype=np.int64))
        zr, zi = np.ascontiguousarray(Zc.real).reshape(m, n, n), np.ascontiguousarray(Zc.imag).reshape(m, n, n)
        ref = None if z0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(z0, dtype=np.float64), (n,)))
        out = [np.empty((m, n, n)) for _ in range(4)]
        ys, ss = np.zeros(max(m, 1), dtype=np.int32), np.zeros(max(m, 1), dtype=np.int32)
        self._chk(lib().pe_hip_convert_net(self._h, n, m, _dp(zr), _dp(zi), _dp(ref) if ref is not None else None, *[_dp(o) for o in out], _ip(ys), _ip(ss)))
        return ((out[0] + 1j * out[1]).reshape(Zc.shape), (out[2] + 1j * out[3]).reshape(Zc.shape), ys[:m].reshape(lead), ss[:m].reshape(lead))

    def analyze_pz(self, omega0, what=PZ_POLES, n_wanted=1, max_krylov=32, ports=None, tol=0.0, theta_floor=0.0, breakdown_tol=0.0, check=True):
        """Poles and / or zeros nearest to the shift j omega0 by shift-invert Arnoldi on one factorisation (pe_hip_analyze_pz).  ports:
        ((in_pos, in_neg), (out_pos, out_neg)) rows of x, -1: ground -- needed for zeros.  Returns (instance_status [batch], stats dict with
        the return code under 'rc'); the values come from pz() / pz_gain()."""
        (ip, ineg), (op, on) = ports if ports is not None else ((-1, -1), (-1, -1))
        ctl = PzControl(int(what), float(omega0), int(n_wanted), int(max_krylov), float(tol), float(theta_floor), float(breakdown_tol), int(ip), int(ineg),
                        int(op), int(on))
        status = np.zeros(max(self.batch, 1), dtype=np.int32)
        st = PzStats()
        rc = lib().pe_hip_analyze_pz(self._h, C.byref(ctl), _ip(status), C.byref(st))
        if check:
            self._chk(rc)
        d = st.asdict()
        d["rc"] = rc
        return status[:self.batch], d

    def pz(self, which=PZ_POLES, capacity=PZ_MAX_KRYLOV):
        """The poles (PZ_POLES) or zeros (PZ_ZEROS) of the last analyze_pz: (s complex [batch][capacity] sorted by |s - s0|, padded with NaN,
        err_est [batch][capacity], n_found, n_converged, complete [batch])."""
        B = self.batch
        re, im, err = np.empty((B, capacity)), np.empty((B, capacity)), np.empty((B, capacity))
        nf, nc, cp = (np.zeros(max(B, 1), dtype=np.int32) for _ in range(3))
        self._chk(lib().pe_hip_get_pz(self._h, int(which), 0, B, int(capacity), _dp(re), _dp(im), _dp(err), _ip(nf), _ip(nc), _ip(cp)))
        return re + 1j * im, err, nf[:B], nc[:B], cp[:B]

    def pz_gain(self):
        """H(s0) = c^T A0^-1 b of the last analyze_pz that asked for zeros, complex [batch]"""
        re, im = np.empty(max(self.batch, 1)), np.empty(max(self.batch, 1))
        self._chk(lib().pe_hip_get_pz_gain(self._h, 0, self.batch, _dp(re), _dp(im)))
        return (re + 1j * im)[:self.batch]

    def eig_hessenberg(self, H):
        """Eigenvalues of upper Hessenberg matrices H complex [..., m, m] (1 <= m <= PZ_MAX_KRYLOV) and, for each, the last component of its
        unit eigenvector, by the Ritz kernel of analyze_pz (pe_hip_eig_hessenberg; needs no circuit).  Returns (theta, last complex
        [..., m], status [...])."""
        Hc = np.asarray(H, dtype=np.complex128)
        m = Hc.shape[-1]
        if Hc.ndim < 2 or Hc.shape[-2] != m:
            raise ValueError("H must be [..., m, m]")
        lead = Hc.shape[:-2]
        n = int(np.prod(lead, dtype=np.int64))
        hr, hi = np.ascontiguousarray(Hc.real).reshape(n, m, m), np.ascontiguousarray(Hc.imag).reshape(n, m, m)
        out = [np.empty((n, m)) for _ in range(4)]
        status = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(lib().pe_hip_eig_hessenberg(self._h, m, n, _dp(hr), _dp(hi), *[_dp(o) for o in out], _ip(status)))
        return (out[0] + 1j * out[1]).reshape(lead + (m,)), (out[2] + 1j * out[3]).reshape(lead + (m,)), status[:n].reshape(lead)

    def phase_clocks_coop(self, instance=0):
        """Per-layout breakdown of the cooperative fronts (see pe_hip_get_phase_clocks_ex), microseconds / counts."""
        t = np.zeros(48, dtype=np.int64)
        n = C.c_int()
        fn = lib().pe_hip_get_phase_clocks_ex
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
        self._chk(fn(self._h, instance, 48, t.ctypes.data_as(C.POINTER(C.c_longlong)), C.byref(n)))
        out = {}
        for L, name in enumerate(("whole", "panel", "chain", "wave0")):
            q = t[8 + 6 * L: 14 + 6 * L] if L < 3 else t[32:38]
            out[name] = {"asm": q[0] / 100.0, "piv": q[1] / 100.0, "schur": q[2] / 100.0, "store": q[3] / 100.0, "fronts": int(q[4]), "sum_m2": int(q[5])}
        out["wave0"]["asm_own"] = t[38] / 100.0
        out["part_us"] = [float(v) / 100.0 for v in t[40:48]]
        out["wave_phase_us"] = [float(v) / 100.0 for v in t[26:32]]
        return out

    def update_param(self, kind, index, column, values):
        """one value for every instance, or [batch] values (pe_hip_update_param's batched form)"""
        v = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64)      # (a column sliced out of a table is strided: the library reads a dense array)
        if v.shape not in ((1,), (self.batch,)):
            raise ValueError(f"update_param takes one value or [{self.batch}] values, not an array of shape {v.shape}")
        self._chk(lib().pe_hip_update_param(self._h, kind, index, column, _dp(v), 1 if len(v) > 1 else 0))

    def solve_csr(self, n, row_ptr, col_ind, values, b, copy_pattern=True):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(col_ind, dtype=np.int32)
        va = np.ascontiguousarray(values, dtype=np.float64)
        bb = np.ascontiguousarray(b, dtype=np.float64)
        x = np.empty(n)
        tm = Timings()
        self._chk(lib().pe_hip_solve_csr_real(self._h, n, len(ci), _ip(rp), _ip(ci), _dp(va), _dp(bb), _dp(x), 1 if copy_pattern else 0,
                                              C.byref(tm)))
        return x, {k: getattr(tm, k) for k, _ in tm._fields_}

    def solve_csr_complex(self, n, row_ptr, col_ind, values, b, copy_pattern=True):
        """pe_hip_solve_csr_complex: complex128 arrays travel as the interleaved (re, im) doubles std::complex<double> is."""
        rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
        ci = np.ascontiguousarray(col_ind, dtype=np.int32)
        va = np.ascontiguousarray(values, dtype=np.complex128)
        bb = np.ascontiguousarray(b, dtype=np.complex128)
        x = np.empty(n, dtype=np.complex128)
        tm = Timings()
        self._chk(lib().pe_hip_solve_csr_complex(self._h, n, len(ci), _ip(rp), _ip(ci), va.ctypes.data_as(C.POINTER(C.c_double)),
                                                 bb.ctypes.data_as(C.POINTER(C.c_double)), x.ctypes.data_as(C.POINTER(C.c_double)),
                                                 1 if copy_pattern else 0, C.byref(tm)))
        return x, {k: getattr(tm, k) for k, _ in tm._fields_}


def build_id():
    """16 hex digits identifying the loaded library build (pe_hip_build_id)."""
    return lib().pe_hip_build_id().decode()


class Sweep(_Probes):
    """Monte-Carlo sweep over the devices of `device_mask` (pe_hip_sweep_*): contiguous instance blocks per device, one engine each."""
    _prefix = "pe_hip_sweep_"

    def __init__(self, device_mask=1):
        l = lib()
        l.pe_hip_sweep_last_error.restype = C.c_char_p
        l.pe_hip_sweep_last_error.argtypes = [C.c_void_p]
        for name in ("pe_hip_sweep_destroy", "pe_hip_sweep_devices", "pe_hip_sweep_reset"):
            getattr(l, name).argtypes = [C.c_void_p]
        l.pe_hip_sweep_destroy.restype = None
        l.pe_hip_sweep_set_options.argtypes = [C.c_void_p, C.POINTER(Options)]
        l.pe_hip_sweep_load_circuit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DeviceTable)]
        l.pe_hip_sweep_run.argtypes = [C.c_void_p, C.c_double, C.c_int, C.POINTER(RunStats)]
        l.pe_hip_sweep_set_tr_method.argtypes = [C.c_void_p, C.c_int]
        l.pe_hip_sweep_operating_point.argtypes = [C.c_void_p, C.c_int, C.POINTER(RunStats)]
        l.pe_hip_sweep_reduce.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        l.pe_hip_sweep_get_solution.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]
        l.pe_hip_sweep_shard.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self._h = C.c_void_p()
        rc = l.pe_hip_sweep_create(C.c_uint(int(device_mask)), C.byref(self._h))
        if rc != 0:
            raise PeHipError(rc, (l.pe_hip_sweep_last_error(None) or b"").decode())
        self.rows = 0
        self.batch = 0

    def close(self):
        if self._h:
            lib().pe_hip_sweep_destroy(self._h)
            self._h = C.c_void_p()

    def _chk(self, rc):
        if rc != 0:
            raise PeHipError(rc, (lib().pe_hip_sweep_last_error(self._h) or b"").decode())

    def set_options(self, g_min=0.0, refactor_every_solve=1, residual_tol=0.0):
        o = Options(0.0, 0.0, 0.0, 0.0, g_min, 0, refactor_every_solve, 0.0, residual_tol)
        self._chk(lib().pe_hip_sweep_set_options(self._h, C.byref(o)))

    def set_tr_method(self, method):
        """pe_hip_set_tr_method on every device's engine (Engine.set_tr_method)"""
        m = _TR_NAMES[method.lower()] if isinstance(method, str) else int(method)
        self._chk(lib().pe_hip_sweep_set_tr_method(self._h, m))

    def load_deck(self, deck, batch, overrides=None):
        n_nodes, n_br, tables = deck_tables(deck, batch, overrides, 0)
        arr = (DeviceTable * max(1, len(tables)))()
        self._keep = list(tables)
        for i, (kind, nodes, branch, par, batched) in enumerate(tables):
            arr[i] = DeviceTable(kind, len(nodes), _ip(nodes), None if branch is None else _ip(branch), _dp(par), batched)
        self._chk(lib().pe_hip_sweep_load_circuit(self._h, int(n_nodes), int(n_br), int(batch), len(tables), arr))
        self.rows, self.batch = n_nodes + n_br, batch
        self._probe_cfg = (0, 0, 0)
        self._four_cfg = (0, 0)

    def shards(self):
        out = []
        for i in range(lib().pe_hip_sweep_devices(self._h)):
            d, f, c = C.c_int(), C.c_int(), C.c_int()
            self._chk(lib().pe_hip_sweep_shard(self._h, i, C.byref(d), C.byref(f), C.byref(c)))
            out.append((d.value, f.value, c.value))
        return out

    def reset(self):
        self._chk(lib().pe_hip_sweep_reset(self._h))

    def run(self, dt, nsteps):
        st = RunStats()
        self._chk(lib().pe_hip_sweep_run(self._h, float(dt), int(nsteps), C.byref(st)))
        return st.asdict()

    def operating_point(self, mode=MODE_OP):
        """pe_hip_sweep_operating_point: Engine.analyze_dc on every device's engine, statistics summed"""
        st = RunStats()
        self._chk(lib().pe_hip_sweep_operating_point(self._h, int(mode), C.byref(st)))
        return st.asdict()

    def operating_point_stepping(self, mode=MODE_OP, method=STEP_AUTO, check=True, **control):
        """pe_hip_sweep_operating_point_stepping: Engine.analyze_op_stepping on every device's engine, statistics summed"""
        st = OpStepStats()
        ctl = op_step_control(method, **control)
        rc = lib().pe_hip_sweep_operating_point_stepping(self._h, int(mode), C.byref(ctl), C.byref(st))
        if check:
            self._chk(rc)
        return dict(st.asdict(), rc=rc)

    def reduce(self):
        out = np.empty((4, self.rows))
        self._chk(lib().pe_hip_sweep_reduce(self._h, _dp(out)))
        return out

    def solution(self, first=0, count=None):
        count = self.batch - first if count is None else count
        x = np.empty((count, self.rows))
        self._chk(lib().pe_hip_sweep_get_solution(self._h, int(first), int(count), _dp(x)))
        return x


def write_touchstone(path, freqs_hz, S, z0):
    """Touchstone v1 file (.sNp, `# Hz S RI R z0`) of a scattering sweep S complex [n_points][n][n] at freqs_hz; z0: the reference
    resistance per port (or one number).  Version 1 has ONE reference: ValueError unless all z0 are equal.  Data order of the format:
    a 2-port writes S11 S21 S12 S22 on one line; every other n writes the matrix row by row (at most four pairs per line for n >= 3)."""
    f = np.asarray(freqs_hz, dtype=np.float64).reshape(-1)
    Sc = np.asarray(S, dtype=np.complex128)
    if Sc.ndim != 3 or Sc.shape[0] != len(f) or Sc.shape[1] != Sc.shape[2]:
        raise ValueError("S must be [n_points][n][n] with one matrix per frequency")
    n = Sc.shape[1]
    ref = np.broadcast_to(np.asarray(z0, dtype=np.float64), (n,))
    if not np.all(ref == ref[0]) or not np.isfinite(ref[0]) or not ref[0] > 0.0:
        raise ValueError("Touchstone v1 has one reference resistance: all z0 must be equal, finite and positive")
    num = lambda v: repr(float(v))
    pair = lambda z: num(z.real) + " " + num(z.imag)
    with open(path, "w") as fh:
        fh.write("! %d-port scattering parameters, %d points\n" % (n, len(f)))
        fh.write("# Hz S RI R %s\n" % num(ref[0]))
        for k in range(len(f)):
            M = Sc[k]
            if n == 2:
                fh.write(" ".join([num(f[k]), pair(M[0, 0]), pair(M[1, 0]), pair(M[0, 1]), pair(M[1, 1])]) + "\n")
                continue
            first = True
            for i in range(n):
                for c0 in range(0, n, 4):
                    body = " ".join(pair(M[i, j]) for j in range(c0, min(n, c0 + 4)))
                    fh.write((num(f[k]) + " " if first else "  ") + body + "\n")
                    first = False
