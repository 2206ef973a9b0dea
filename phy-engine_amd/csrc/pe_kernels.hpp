// pe_kernels.hpp -- host-callable launchers of pe_kernels.hip.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

#include "pe_device.hpp"

#ifndef PE_THREADS
    #define PE_THREADS 512  // upper bound (launch bounds); a launch uses V.n_waves * 64 threads
#endif

namespace pe
{
    hipError_t launch_tr_steps(hipStream_t st, DevView const& V, double dt, int nsteps, bool reuse_factor);
    hipError_t launch_dc_point(hipStream_t st, DevView const& V, int mode);
    hipError_t launch_factor_solve(hipStream_t st, DevView const& V, bool do_factor);
    // multi-workgroup mode (V.n_parts > 1)
    hipError_t launch_m2_companion(hipStream_t st, DevView const& V, double dt);
    // stamp_mode: 0 everything; 1 not the first Newton iteration of this solve point -- only the x-dependent slots / rows are stamped again (V.dyn_a /
    // dyn_b); 2 first iteration of a transient step whose matrix holds the stamp of this dt: x-dependent matrix slots + the whole right-hand side
    // companion: first iteration of a transient step -- the companion update of that step (dt = companion_dt) runs inside the evaluation launch
    hipError_t launch_m2_iteration(hipStream_t st, DevView const& V, int mode, double t, double last_step, bool do_factor, hipEvent_t ev0 = nullptr,
                                   hipEvent_t ev1 = nullptr, int stamp_mode = 0, bool companion = false, double companion_dt = 0.0);
    // the same iteration with the static fronts of the lane-group kernel kept (sk.save) or skipped (sk.skip): pe_device.hpp StaticSkip.  Builds
    // without HIP (the emulation library): host definitions in pe_engine_newton.cpp on top of launch_m2_iteration / launch_m2_iteration_graph.
    hipError_t launch_m2_iteration_static(hipStream_t st, DevView const& V, int mode, double t, double last_step, bool do_factor, hipEvent_t ev0, hipEvent_t ev1,
                                          int stamp_mode, bool companion, double companion_dt, StaticSkip const& sk);
    // the same sequence + the publication of its results (launch_m2_publish) as ONE captured graph launch, built on first use per (mode,
    // do_factor, stamp_dynamic, companion, V) and replayed afterwards; small sweeps only (pe_engine_newton.cpp).  No HIP events around the
    // dominant launch in this path.  The cache belongs to an engine (created / destroyed with it, cleared when its view changes for good).
    struct M2GraphCache;
    M2GraphCache* m2_graphs_create();
    void m2_graphs_destroy(M2GraphCache* c);
    void m2_graphs_clear(M2GraphCache* c);
    hipError_t launch_m2_iteration_graph(hipStream_t st, M2GraphCache* cache, DevView const& V, int mode, double t, double last_step, bool do_factor, int stamp_mode,
                                         bool companion, double companion_dt, int* pub_flags, double* pub_eta, unsigned long long* pub_seq, unsigned long long seq);
    hipError_t launch_m2_iteration_graph_static(hipStream_t st, M2GraphCache* cache, DevView const& V, int mode, double t, double last_step, bool do_factor,
                                                int stamp_mode, bool companion, double companion_dt, int* pub_flags, double* pub_eta, unsigned long long* pub_seq,
                                                unsigned long long seq, StaticSkip const& sk);
    // device-to-device stream copy of `bytes` (multiple of 16): the kernel behind pe_hip_measure_hbm_ceiling
    hipError_t launch_stream_copy(hipStream_t st, void const* src, void* dst, size_t bytes);
    // one round of iterative refinement of the active instances' last solve + re-check (residual safety net, pe_front.hpp)
    hipError_t launch_m2_refine(hipStream_t st, DevView const& V);
    // flags + residual norms of the iteration just launched -> pinned host memory, then `seq` into *pub_seq (device-visible pointers)
    hipError_t launch_m2_publish(hipStream_t st, DevView const& V, int* pub_flags, double* pub_eta, unsigned long long* pub_seq, unsigned long long seq);
    // small-signal AC refinement on the device (pe_front.hpp ac_residual): r = b0 - A xacc of every instance into its right-hand-side
    // value slots dv[rhs0 ..), *worst (device, one double) = max componentwise backward error over all instances
    hipError_t launch_ac_residual(hipStream_t st, DevView const& V, double const* xacc, double const* b0, int rhs0, double* worst);
    // xacc = first ? x : xacc + x  (every instance; x = the engine's current solution);  first also keeps b0 = the stamped right-hand side
    hipError_t launch_ac_accumulate(hipStream_t st, DevView const& V, double* xacc, double* b0, bool first);
    // complex twin of the solver seam (batch 1, aval in CSR order, V.csr_rp / V.csr_ci set): V.rhs = b0 - A xacc, *worst (device, one double) = max
    // componentwise backward error
    hipError_t launch_csr_residual(hipStream_t st, DevView const& V, double const* xacc, double const* b0, double* worst);
    // per-row {sum v, sum v^2, min, max} of x over the instances (the payload of the sweep's one exchange step):
    // `partial` holds n_chunks x 4 x rows doubles, `out` 4 x rows (both device memory); deterministic (fixed chunk order)
    hipError_t launch_sweep_statistics(hipStream_t st, DevView const& V, int n_chunks, double* partial, double* out);
    // transient probes (pe_probe.hpp): open the window of every instance at its current point / record the split schedule's step at time t
    // for the instances with V.pr.accept[b] != 0.  (launch_tr_steps records when its view has probe_armed set: then it is a ProbedView.)
    // The engine's translation unit pe_engine_newton.cpp holds a serial host definition of both for builds without HIP (the emulation library).
    hipError_t launch_probe_arm(hipStream_t st, ProbedView const& V);
    hipError_t launch_probe_record(hipStream_t st, ProbedView const& V, double t);
    // Fourier analysis of probes (pe_fourier.hpp): coefficients [count][n_fp][H + 1][4] and THD [count][n_fp] of the instances from `first`
    hipError_t launch_fourier_finish(hipStream_t st, FourierView const& F, int first, int count, double* coef, double* thd);
    // frequency-batched AC sweep (pe_ac_sweep.hpp): V is the view of the sweep's AC engine, whose instance b * S.P + p is circuit instance b at
    // point p of the pass.  fill: the value vector of every instance from the base vectors and S.omega.  residual_each: r = b0 - A xacc into
    // the right-hand-side slots, S.worst[q] per instance and *S.n_above = instances above the refinement threshold (NaN counts).
    // accumulate_each: xacc (+)= x, after the first time only for the instances above the threshold.  gather: the kept rows of xacc into
    // S.res_re / S.res_im at the caller's index of each point.  Builds without HIP: serial host definitions in pe_engine_ac.cpp.
    struct AcSweepView;
    hipError_t launch_ac_sweep_fill(hipStream_t st, DevView const& V, AcSweepView const& S);
    hipError_t launch_ac_residual_each(hipStream_t st, DevView const& V, AcSweepView const& S);
    hipError_t launch_ac_accumulate_each(hipStream_t st, DevView const& V, AcSweepView const& S, bool first);
    hipError_t launch_ac_sweep_gather(hipStream_t st, DevView const& V, AcSweepView const& S);
    // noise analysis (pe_noise.hpp).  sources: V is the MAIN engine's view -- Z.S[b][k] of every circuit instance from its resident operating
    // point, and the shared row pairs Z.rows.  accumulate: V is the view of the adjoint sweep engine after refinement -- for every instance
    // b * Z.P + p with Z.point[p] >= 0 the contributions S_k |y_b - y_a|^2 (into Z.contrib when kept) and their sum into Z.psd, in a
    // summation order that depends on Z.n_src only.  Builds without HIP: serial host definitions in pe_engine_ac.cpp.
    struct NoiseView;
    hipError_t launch_noise_sources(hipStream_t st, DevView const& V, NoiseView const& Z);
    hipError_t launch_noise_accumulate(hipStream_t st, DevView const& V, NoiseView const& Z);
    // DC sensitivity analysis (pe_sens.hpp).  rhs: V is the view of the adjoint sweep engine after launch_ac_sweep_fill -- the right-hand-side
    // slots of instance b * Z.P + p become the selector of output Z.point[p] (zero for an unused slot).  accumulate: V is that view after
    // refinement, M the MAIN engine's view (operating point, read only) -- for every instance with Z.point[p] >= 0 the sensitivities of its
    // output to every parameter (into Z.s when kept) and, with weights, the sum of their weighted squares into Z.rss, in a summation order
    // that depends on Z.n_par only.  Builds without HIP: serial host definitions in pe_engine_ac.cpp.
    struct SensView;
    hipError_t launch_sens_rhs(hipStream_t st, DevView const& V, SensView const& Z);
    hipError_t launch_sens_accumulate(hipStream_t st, DevView const& V, DevView const& M, SensView const& Z);
    // multi-port network analysis (pe_net.hpp): V is the view of the sweep's engine.  rhs: port j's selector into the right-hand-side slots
    // of every instance and into Z.b0.  gather: column j of Z.z_re / Z.z_im of every instance with Z.point[p] >= 0 from Z.xacc.  convert:
    // Y, S and their statuses of n_mats matrices [n][n] (device pointers), one wavefront per matrix; any output may be null.  Builds
    // without HIP: serial host definitions in pe_engine_ac.cpp.
    struct NetView;
    hipError_t launch_net_rhs(hipStream_t st, DevView const& V, NetView const& Z, int j);
    hipError_t launch_net_gather(hipStream_t st, DevView const& V, NetView const& Z, int j);
    hipError_t launch_net_convert(hipStream_t st, int n, int n_mats, double const* z_re, double const* z_im, double const* z0, double* y_re, double* y_im,
                                  double* s_re, double* s_im, int* y_status, int* s_status);
    // pole-zero analysis (pe_pz.hpp): V is the view of the call's engine (one point per pass).  bmul: (omega0 B) x basis vector `src` (-1:
    // the start vector's pre-image) into the right-hand-side slots of every instance and into Z.b0, zeros for a parked instance.  store_z:
    // Z.zvec and Z.gain from Z.xacc.  orth: Arnoldi step k of every running instance from Z.xacc (zeros: with the rank-one correction),
    // one workgroup per instance.  ritz: the matrices of R, one wavefront per matrix with the matrix in LDS; hipErrorInvalidValue when
    // R.m is out of range or the matrix does not fit the LDS of a workgroup.  Builds without HIP: serial host definitions in pe_engine_ac.cpp.
    struct PzView;
    struct PzRitzView;
    hipError_t launch_pz_bmul(hipStream_t st, DevView const& V, PzView const& Z, int src);
    hipError_t launch_pz_store_z(hipStream_t st, DevView const& V, PzView const& Z);
    hipError_t launch_pz_orth(hipStream_t st, DevView const& V, PzView const& Z, int k, bool zeros);
    hipError_t launch_pz_ritz(hipStream_t st, PzRitzView const& R);
    // variable-step transient (pe_lte.hpp): lte: q of the candidate V.x against the history ring + failed / non-finite instances into
    // L.result (cleared first); history_push: V.x of every instance into ring slot `slot`; state_copy: every (dst, src, bytes) of the table
    // (snapshot and roll-back of a step).  Builds without HIP: serial host definitions in pe_engine_newton.cpp.
    struct LteView;
    struct StateCopy;
    hipError_t launch_tr_lte(hipStream_t st, DevView const& V, LteView const& L);
    hipError_t launch_tr_history_push(hipStream_t st, DevView const& V, double* hist, int slot);
    hipError_t launch_tr_state_copy(hipStream_t st, StateCopy const& S);
    // backward Euler / Gear-2 (pe_integ.hpp; V.tr_method, V.tr_hist).  lte_integ: launch_tr_lte with the estimate of `method`.  restart: h_p := 0
    // of every instance (only_failed: of the instances whose status is not OK).  The companion update of a step itself rides in
    // launch_tr_steps / launch_m2_companion / launch_m2_iteration*, dispatched on V.tr_method.  Builds without HIP: serial host definitions
    // in pe_engine_newton.cpp.
    hipError_t launch_tr_lte_integ(hipStream_t st, DevView const& V, LteView const& L, int method);
    hipError_t launch_integ_restart(hipStream_t st, DevView const& V, bool only_failed);
    // DC sweep (pe_dc_sweep.hpp): V is the view of the sweep engine, whose instance b * S.P + p is circuit instance b at slot p of the pass.
    // fill: the swept slot of every instance from S.value.  seed: solution and junction / relay state of every destination with
    // S.seed_of[q] >= 0 from that source -- a circuit instance of the main engine (from_main: round 0) or an instance of the sweep engine.
    // classify: one workgroup per circuit instance -- bookkeeping of the pairs solved since the last classification, nearest converged slot
    // of every failing one, S.seed_of and the statuses of the next round (reseed: else everything is parked), counts into S.rec.
    // gather: the kept rows of every valid pair into S.res at the caller's index, NaN where it failed.  Builds without HIP: serial host
    // definitions in pe_engine_newton.cpp.
    struct DcSweepView;
    hipError_t launch_dc_sweep_fill(hipStream_t st, DevView const& V, DcSweepView const& S);
    hipError_t launch_dc_sweep_seed(hipStream_t st, DevView const& V, DcSweepView const& S, bool from_main);
    hipError_t launch_dc_sweep_classify(hipStream_t st, DevView const& V, DcSweepView const& S, bool reseed);
    hipError_t launch_dc_sweep_gather(hipStream_t st, DevView const& V, DcSweepView const& S);
    // gmin / source stepping for operating points (pe_op_step.hpp): the controller of every instance after a solve -- role BEGIN classifies the
    // direct attempt and opens the first phase of the failing instances, CONTROL accepts or rejects the level just solved and writes the
    // slots of the next one, FINISH puts the real values and the final statuses back.  The host zeroes S.rec before the launch and reads it
    // after.  Builds without HIP: serial host definition in pe_engine_newton.cpp.
    struct OpStepView;
    hipError_t launch_op_step_control(hipStream_t st, DevView const& V, OpStepView const& S, int role);
}  // namespace pe
