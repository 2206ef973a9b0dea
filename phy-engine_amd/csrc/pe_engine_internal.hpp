// pe_engine_internal.hpp -- what the translation units of the engine share: the engine object behind the opaque pe_hip_engine handle of
// include/pe_hip.h, its device-memory pools, the error convention, and the helpers that cross file boundaries.  Not installed, not part
// of the C ABI.
// The owning types come first (Pool, DevBuf, KeptRows for device memory; Pinned, Event, Stream, EnginePtr, GraphsPtr for what else the
// engine holds), then the engine object -- whose declaration order IS its destruction order --, then the shared helpers.
//   pe_engine.cpp             handle life cycle (pe_hip_create, pe_hip_destroy, engine_build), options, circuit load, getters / setters, the solve_csr_real seam
//   pe_engine_policy.cpp      launch geometry by batch size, symbolic analysis + its upload (the PHY_ENGINE_HIP_* knobs live here)
//   pe_engine_newton.cpp      host-driven Newton / transient loops of the split schedule, residual safety net, pe_hip_analyze_tr / _dc
//   pe_engine_checkpoint.cpp  pe_hip_checkpoint_*
//   pe_engine_ac.cpp          pe_hip_analyze_ac / pe_hip_get_solution_ac, pe_hip_analyze_ac_sweep / pe_hip_get_ac_sweep, pe_hip_analyze_noise / pe_hip_get_noise*,
//                             pe_hip_analyze_sens / pe_hip_get_sens*, pe_hip_analyze_net / pe_hip_get_net*, pe_hip_analyze_pz / pe_hip_get_pz*; the helpers of every stored result (KeptRows, stored_window)
//   pe_engine_seam.cpp        pe_hip_solve_csr_complex (the complex twin of the solver seam)
//   pe_sweep.cpp              pe_hip_sweep_*: the multi-device handle (uses EnginePtr, engine_build and set_symbolic_reference only; everything else through the C ABI)
#pragma once
// (the helpers below are shared between the engine's translation units only: not exported from libpe_hip.so)
#define PE_ENG_HIDDEN __attribute__((visibility("hidden")))
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/pe_hip.h"
#include "pe_ac.hpp"
#include "pe_ac_sweep.hpp"
#include "pe_circuit.hpp"
#include "pe_dc_sweep.hpp"
#include "pe_device.hpp"
#include "pe_kernels.hpp"
#include "pe_integ.hpp"
#include "pe_lte.hpp"
#include "pe_net.hpp"
#include "pe_noise.hpp"
#include "pe_op_step.hpp"
#include "pe_pz.hpp"
#include "pe_sens.hpp"
#include "pe_symbolic.hpp"

#include <map>
#include <thread>
#include <utility>

namespace pe_eng  // (Pool is a member type of the engine object: default visibility, header-only)
{
    using clk = std::chrono::steady_clock;
    inline double ms_since(clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); }

    struct Pool
    {
        std::vector<void*> ptrs;
        size_t bytes{};
        Pool() = default;
        Pool(Pool&& o) noexcept : ptrs(std::move(o.ptrs)), bytes(o.bytes) { o.forget(); }
        Pool& operator=(Pool&& o) noexcept  // (what this pool held is freed: a state struct is reset by assigning a fresh one)
        {
            if(this != &o)
            {
                release();
                ptrs = std::move(o.ptrs);
                bytes = o.bytes;
                o.forget();
            }
            return *this;
        }
        ~Pool() { release(); }
        void forget()
        {
            ptrs.clear();
            bytes = 0;
        }
        void release()
        {
            for(void* p: ptrs) (void)hipFree(p);
            ptrs.clear();
            bytes = 0;
        }
        template <class T>
        hipError_t alloc(T*& out, size_t n, bool zero = true)
        {
            out = nullptr;
            size_t const b = std::max<size_t>(n, 1) * sizeof(T);
            void* p{};
            hipError_t e = hipMalloc(&p, b);
            if(e != hipSuccess) return e;
            ptrs.push_back(p);
            bytes += b;
            if(zero)
            {
                e = hipMemset(p, 0, b);
                if(e != hipSuccess) return e;
            }
            out = static_cast<T*>(p);
            return hipSuccess;
        }
        template <class T>
        hipError_t upload(T const*& out, std::vector<T> const& v)
        {
            T* p{};
            hipError_t e = alloc(p, v.size(), false);
            if(e != hipSuccess) return e;
            if(!v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
            out = p;
            return e;
        }
    };

    // a device buffer sized by the call that fills it: kept while the next call asks for the same length
    template <class T>
    struct DevBuf
    {
        Pool pool;
        T* p{};
        size_t len{};
        void release()
        {
            pool.release();
            p = nullptr;
            len = 0;
        }
        hipError_t ensure(size_t n, bool zero = true)
        {
            if(len == n && p) return hipSuccess;
            release();
            hipError_t const e = pool.alloc(p, n, zero);
            if(e == hipSuccess) len = n;
            return e;
        }
        hipError_t ensure_at_least(size_t n, bool zero = true) { return len >= n && p ? hipSuccess : ensure(n, zero); }
        hipError_t fill_nan() { return hipMemset(p, 0xff, len * sizeof(T)); }  // (all ones: a NaN -- what no pass wrote reads NaN)
    };

    // the rows of x a sweep keeps (pe_hip_set_ac_sweep_rows / pe_hip_set_dc_sweep_rows; empty: all rows) and their device copy -- a buffer of
    // its own, reused while it is large enough: a caller alternating row selections allocates nothing
    struct KeptRows
    {
        std::vector<int> rows;
        int* d_keep{};
        size_t cap{};
        bool on_device{};  // d_keep holds `rows`
        KeptRows() = default;
        KeptRows(KeptRows&& o) noexcept { *this = std::move(o); }
        KeptRows& operator=(KeptRows&& o) noexcept
        {
            if(this != &o)
            {
                if(d_keep) (void)hipFree(d_keep);
                rows = std::move(o.rows);
                d_keep = std::exchange(o.d_keep, nullptr);
                cap = std::exchange(o.cap, 0);
                on_device = std::exchange(o.on_device, false);
            }
            return *this;
        }
        ~KeptRows()
        {
            if(d_keep) (void)hipFree(d_keep);
        }
        int set(pe_hip_engine* h, char const* name, int n_rows, int const* rows_in);  // (the owner's stored result is the caller's to invalidate)
        int upload(pe_hip_engine* h, int const*& keep_out);                            // keep_out: the device copy, nullptr for all rows
    };

    // a pinned host buffer of n T, kept while it is large enough (flags: hipHostMallocCoherent | hipHostMallocMapped for memory the device
    // writes and the host polls -- device() is then the same memory as the device sees it)
    template <class T>
    struct Pinned
    {
        Pinned() = default;
        Pinned(Pinned&& o) noexcept { *this = std::move(o); }
        Pinned& operator=(Pinned&& o) noexcept
        {
            if(this != &o) release(), p = std::exchange(o.p, nullptr), dev = std::exchange(o.dev, nullptr), cap = std::exchange(o.cap, 0);
            return *this;
        }
        ~Pinned() { release(); }
        void release()
        {
            if(p) (void)hipHostFree(p);
            p = dev = nullptr;
            cap = 0;
        }
        hipError_t ensure_at_least(size_t n, unsigned flags = hipHostMallocDefault)
        {
            if(cap >= n && p) return hipSuccess;
            release();
            void* q{};
            hipError_t e = hipHostMalloc(&q, std::max<size_t>(n, 1) * sizeof(T), flags);
            if(e != hipSuccess) return e;
            p = static_cast<T*>(q);
            if(flags & hipHostMallocMapped)
            {
                if(e = hipHostGetDevicePointer(&q, p, 0); e != hipSuccess) return release(), e;
                dev = static_cast<T*>(q);
            }
            cap = n;
            return hipSuccess;
        }
        T* data() const { return p; }
        T* device() const { return dev; }
        size_t capacity() const { return cap; }

    private:
        T *p{}, *dev{};
        size_t cap{};
    };

    // an event / a stream: made by create() (a default-constructed one holds nothing), destroyed with its owner
    template <class H, hipError_t (*Destroy)(H)>
    struct Handle
    {
        H h{};
        Handle() = default;
        Handle(Handle&& o) noexcept : h(std::exchange(o.h, H{})) {}
        Handle& operator=(Handle&& o) noexcept
        {
            if(this != &o) reset(), h = std::exchange(o.h, H{});
            return *this;
        }
        ~Handle() { reset(); }
        void reset() { h = h ? ((void)Destroy(h), H{}) : H{}; }
        operator H() const { return h; }
    };
    struct Event : Handle<hipEvent_t, hipEventDestroy>
    {
        hipError_t create() { return reset(), hipEventCreate(&h); }
    };
    struct Stream : Handle<hipStream_t, hipStreamDestroy>
    {
        hipError_t create() { return reset(), hipStreamCreate(&h); }
    };

    // an engine owned by another object (the sub-engines of the analyses, the engines of a pe_hip_sweep: pe_hip_destroy synchronises its
    // stream before anything of it goes), and the captured-graph cache of an engine (pe_kernels.hpp)
    template <class T, void (*Destroy)(T*)>
    struct Deleter
    {
        void operator()(T* p) const { Destroy(p); }
    };
    using EnginePtr = std::unique_ptr<pe_hip_engine, Deleter<pe_hip_engine, pe_hip_destroy>>;
    using GraphsPtr = std::unique_ptr<pe::M2GraphCache, Deleter<pe::M2GraphCache, pe::m2_graphs_destroy>>;
}  // namespace pe_eng
using pe_eng::Pool;

// Everything the engine owns is a member that frees itself, and pe_hip_destroy is "set the device, synchronise the stream, delete".  The
// ORDER of destruction is the reverse of the declaration order below, and it matters:
//   - stream and events are declared first: they go last, after everything that was enqueued on them;
//   - the pools are declared before the captured-graph cache: the graphs go before the memory their nodes point into and before the stream;
//   - the sub-engines (ac, noise, sens, net, pz, dcs) are declared after the pools and buffers their kernels read: each goes first, and
//     synchronises its own stream in its pe_hip_destroy.
// A state struct that holds a sub-engine beside buffers of its own (Ac, Ac::Sweep, DcSweep) does not leave that to its member order: its
// destructor and its drop() reset the engine explicitly before anything else goes.  Noise, Sens, Net and Pz declare their Ac last.
struct pe_hip_engine
{
    int device{};
    pe_eng::Stream stream;
    pe_eng::Event ev0, ev1;
    pe_eng::Event evk0, evk1;   // around the dominant launch of one split-schedule iteration
    double dominant_ms{};       // accumulated over the current analyze call
    int dominant_launches{};
    std::string err;
    pe_hip_options opt{};
    int lds_limit{65536};
    std::map<std::string, int> knobs;  // pe_hip_set_knob: this engine's overrides of the PHY_ENGINE_HIP_* tuning knobs (name without the prefix)

    // resident circuit
    bool loaded{};
    pe::HostCircuit hc;
    std::vector<int> drv_node;
    std::vector<double> drv_volt;
    pe::OverlaySpec overlay;      // host-stamp overlay (pe_hip_set_overlay): part of the pattern of the next load
    pe_hip_overlay_fn overlay_fn{};
    void* overlay_user{};
    std::vector<double> ov_x, ov_a, ov_b;  // staging of the callback
    // What belongs to the resident circuit and is not a buffer: pe_hip_load_circuit resets ALL of it by assigning a fresh Resident, so a
    // field added here cannot carry one circuit's state into the next.  Reset: the class and dt of the symbolic analysis (the next analysis
    // is made again), the validity of the factors and of the static matrix stamps (the matrix is gone), what the device's `active` array
    // holds (the array is gone), the safety net's verdicts and counters and the launch counters (they speak of the circuit), the tables of
    // the static fronts and the statistics scratch (pointers into pools the load releases), and the host's view of the BE / GEAR2 history.
    // NOT here, because a load keeps them: device, lds_limit, opt, knobs, tr_method (engine settings); the overlay, its callback and the
    // digital drives (part of the pattern of the NEXT load); param_epoch, n_symbolic, analyze_ms, dominant_* (monotone or per-call
    // diagnostics); graph_mode (chosen again by the next solve point; only active_dev is cleared beside it); pub_seq and the pinned
    // buffers (sized by the largest batch so far, content per call); csr / csrz (the seam's own state).  fact_dt, a_static_dt, integ_failed,
    // refined_in_point and n_factor_launches stay as a load has always left them: read behind a flag reset here, written before use, or read as a difference.
    struct Resident
    {
        int sym_class{-1};  // 0: static (OP/DC/TROP) pattern weights, 1: TR
        double sym_dt{};    // time step whose companion values the TR analysis was matched on
        bool fact_valid{};
        // split schedule: instances whose matrix (aval) holds a FULL transient stamp at step size a_static_dt -- their next steps at that dt
        // stamp the x-dependent slots only (pe_engine_newton.cpp run_m2_tr); cleared together with fact_valid wherever a static value may
        // change (invalidate_factors)
        std::vector<char> a_static;
        std::vector<int> active_dev;  // what the device's `active` array currently holds (an unchanged mask is not uploaded again)
        bool singular_rematched{};    // the one re-match after a singular pivot has been spent for this resident circuit
        bool careful{};               // residual safety net tripped on the resident kernel: stay on the host-driven (refining) schedule
        long long n_refined{}, n_rematched{};  // solves repaired by refinement / symbolic re-analyses on an instance's own values (diagnostics)
        // static fronts of the lane-group kernel (pe_device.hpp StaticSkip): the tables of the current analysis (sym_pool; all null
        // when it has no static quad front) and the quad factor launches since the circuit was loaded, by program
        pe::StaticSkip static_skip{};
        long long quad_skipped_launches{}, quad_full_launches{};
        // iteration launches of the lane-group factor kernel issued after a refinement round of their own solve point, and those of them
        // that skipped the static fronts (must stay 0: pe_hip_get_static_skip_refinement_stats)
        long long quad_launches_after_refinement{}, quad_skipped_after_refinement{};
        double* stats_scratch{};      // pe_hip_sweep_statistics: partial sums + result (device, owned by circ_pool)
        size_t stats_doubles{};
        double integ_hp{};            // (see tr_method below)
    } resident;
    // host-driven Newton loop (split schedule): pinned staging for the per-iteration `active` upload / `flags` read-back (grown together)
    pe_eng::Pinned<int> pin_active, pin_flags;
    // results published by the last launch of an iteration straight into pinned host memory (k_m2_publish): [sequence number][flags][norms]
    pe_eng::Pinned<char> pub;
    unsigned long long pub_seq{};
    bool graph_mode{};            // the quad list behind the device's `active` mask is laid out for a captured sequence (full grid)
    pe_eng::Pinned<double> stats_pinned;  // pinned host landing buffer of the result of pe_hip_sweep_statistics
    // transient probes (pe_hip_set_probes / pe_hip_arm_probes, pe_probe.hpp): configuration and device buffers (dropped by a circuit
    // load) and the armed window.  The engine's view V never carries them; the launches that record get probe_view(h).
    struct Probes
    {
        Pool pool;
        bool configured{}, armed{};
        int n_probes{}, n_meas{}, capacity{}, stride{}, batch{};
        std::vector<int> kind;     // per measure (the host finishes AVG / RMS)
        pe::ProbeView pv{};        // device buffers
    } probe;
    pe_eng::Pinned<int> pin_accept;  // pinned staging of the split schedule's accepted set of the probes (kept across loads)
    // Fourier analysis of probes (pe_hip_set_fourier, pe_fourier.hpp): rides on the probe configuration and its armed window; dropped with it
    struct Fourier
    {
        Pool pool;
        bool configured{};
        int n_fp{}, H{};
        pe::FourierView fv{};      // device buffers (the host's copy: k_fourier_finish takes it by value)
        pe::FourierView const* dev{};  // the same in device memory: what probe_view hands to the recording launches
        double* out_coef{};        // [batch][n_fp][H + 1][4] result of k_fourier_finish
        double* out_thd{};         // [batch][n_fp]
    } fourier;
    // variable-step transient (pe_hip_analyze_tr_adaptive, pe_lte.hpp): the shadow copy of the state of a step, the history ring and the
    // result slots (allocated at the first adaptive call, dropped by a circuit load), the history's host side, and the step log of the last call
    struct TrAdaptive
    {
        Pool pool;
        bool allocated{};
        pe::StateCopy save{}, restore{};   // state -> shadow, shadow -> state (the arrays of tr_state_parts + the trace cursor)
        long long* shadow_iters{};         // the shadow of n_iters (what a rejected step spent is read against it)
        double* hist{};                    // [3][batch][rows]
        unsigned long long* q_each{};      // [batch]
        pe::LteResult* result{};
        int n_pts{};                       // accepted points in the history (0: restarted; the ring holds the last three)
        int head{};                        // ring slot of the newest point
        double t_pts[3]{};                 // time of the point in each ring slot
        std::vector<double> log_dt;
        std::vector<int> log_outcome;
    } tra;
    // integration rule of the transient (pe_hip_set_tr_method, pe_integ.hpp): an engine setting like the options -- it survives a circuit
    // load.  The history array V.tr_hist lives in a pool of its own, allocated once a rule other than the trapezoidal one is in effect for a
    // resident circuit (a trapezoidal user's memory is what it was).  integ_hp: the h_p that EVERY instance holds as far as the host can
    // show (0 after a restart, the step after steps that every instance took); NaN when it cannot -- an instance failed or was stepped
    // alone -- and then nothing that is keyed on the companion conductance a0 is reused.
    int tr_method{};
    Pool integ_pool;
    bool integ_failed{};  // some instance's last step failed under BE / GEAR2: its history restarts before its next step
    long long n_symbolic{};  // symbolic analyses of the resident circuit so far (ensure_symbolic)
    Pool circ_pool;  // topology, params, state
    Pool sym_pool;   // symbolic arrays + factor storage
    pe::Symbolic sym;
    pe::DevView V{};
    double fact_dt{};           // (of resident.fact_valid)
    double a_static_dt{-1.0};   // (of resident.a_static)
    double analyze_ms{};
    bool refined_in_point{};  // a refinement round has run since the first iteration of the current solve point (m2_point)
    // captured launch sequences of the split schedule's Newton iteration (small sweeps; pe_kernels.hip launch_m2_iteration_graph): after
    // the pools above, so that it goes before them
    pe_eng::GraphsPtr graphs;

    // small-signal AC: a second engine holding the real-equivalent 2N system (pe_ac.hpp), built on first use
    struct Ac
    {
        pe_eng::EnginePtr eng;
        pe::AcCircuit circ;
        bool built{};
        double sym_omega{-1.0};  // frequency whose values the pivot matching of the current symbolic analysis saw
        std::vector<int> b_ptr0, b_src0;  // right-hand-side lists of the AC system (the device copy reads one slot per row)
        int rhs0{};                       // first of the 2N right-hand-side slots of the AC value vector
        std::vector<double> x;            // refined solution [batch][2N]
        pe_eng::DevBuf<double> d_xacc, d_b0, d_worst;  // device: accumulated solution, the point's right-hand side, worst backward error (refinement)
        bool b0_valid{};  // d_b0 holds the right-hand side of the last pe_hip_analyze_ac as stamped (pe_hip_get_matrix_ac)
        // frequency-batched sweep (pe_hip_analyze_ac_sweep): a third engine holding the same system with batch (circuit batch) x P -- the
        // points of one pass are extra instances --, the buffers of its kernels (pe_ac_sweep.hpp) and the stored result
        struct Sweep
        {
            pe_eng::EnginePtr eng;
            int P{};                          // points per pass the engine was built for
            bool b0_valid{};                  // V.b0 holds the right-hand sides of the last pass as stamped (pe_hip_get_matrix_ac)
            Pool pass_pool;                   // sized by batch x P: xacc, b0, worst, omega, point, n_above
            Pool circ_pool;                   // sized by the circuit: base vectors, scale flags, right-hand-side lists
            pe_eng::DevBuf<double> d_re, d_im;  // sized by the sweep: the result planes
            pe_eng::KeptRows kept;            // pe_hip_set_ac_sweep_rows
            pe::AcSweepView V{};
            long long bytes_per_instance{};   // of the AC system (pe_hip_info), measured once per circuit for the automatic P
            bool valid{};                     // `res` is the sweep of the current circuit at its current operating point
            int n_points{}, n_keep{}, batch{};
            std::vector<double> res;          // [2][n_points][batch][n_keep]: real parts, then imaginary parts
            Sweep& operator=(Sweep&&) = default;
            ~Sweep() { eng.reset(); }
            void drop() { eng.reset(), *this = Sweep{}; }  // the engine first (it synchronises its stream), then every buffer: a fresh Sweep
        } sweep;
        Ac& operator=(Ac&&) = default;
        ~Ac() { sweep.eng.reset(), eng.reset(); }
        void drop() { sweep.eng.reset(), eng.reset(), *this = Ac{}; }  // both engines, then every buffer: a fresh Ac
    } ac;
    // noise analysis (pe_hip_analyze_noise, pe_noise.hpp): the ADJOINT real-equivalent system with sweep state of its own -- its AcCircuit,
    // its single-point engine (only the automatic pass size is measured on it), its batched engine and pass buffers -- so that a stored
    // forward sweep is not disturbed; the source table of the circuit, the densities of the last call and its result
    struct Noise
    {
        bool have_pair{};
        int out_pos{-1}, out_neg{-1};     // the output pair the right-hand-side lists of `sys` select
        bool table_built{}, table_on_device{};
        std::vector<pe::NoiseSource> src; // definition order: resistors, junctions, three-pin devices
        std::vector<int> kind, index, part;
        Pool src_pool;                    // sized by the circuit: source table, row pairs, densities
        pe_eng::DevBuf<double> partial;   // sized by batch x P x chunks: chunk sums
        pe_eng::DevBuf<double> d_res;     // sized by the call: [psd | contributions]
        pe::NoiseView V{};
        bool valid{};                     // `res` is the noise of the current circuit at its current operating point
        bool kept{};                      // ... with contributions
        bool have_density{};              // V.S holds the densities of that call (not after a call refused for a failed operating point)
        int n_points{}, batch{};
        std::vector<double> res;          // [n_points][batch] densities, then [n_points][batch][n_src] contributions when kept
        std::vector<double> integrated;   // [batch]
        Ac sys;                           // (declared last: its engines go before the tables and buffers above)
    } noise;
    // DC sensitivity analysis (pe_hip_analyze_sens, pe_sens.hpp): the adjoint system at omega = 0 with sweep state of its own, like the noise
    // analysis -- the outputs of a call are the points of its passes --, the parameter table and the by-slot stamp lists of the circuit,
    // the raw columns of the last call and its result
    struct Sens
    {
        bool table_built{}, table_on_device{};
        std::vector<pe::SensParam> par;   // definition order of include/pe_hip.h
        std::vector<int> kind, index, column;
        std::vector<int> sl_ptr;          // stamps of every value slot of the main engine (pe_sens.hpp)
        std::vector<pe::SensEnt> sl_ent;
        Pool tab_pool;                    // sized by the circuit: parameter table, stamp lists, raw columns, weights
        pe_eng::DevBuf<int> d_out_pos, d_out_neg;  // the output rows: grown to the most outputs a call has had
        double *d_draw{}, *d_graw{}, *d_weight{};
        pe_eng::DevBuf<double> partial;   // sized by batch x P x chunks: chunk sums
        pe_eng::DevBuf<double> d_res;     // sized by the call: [rss | sensitivities]
        pe::SensView V{};
        bool valid{};                     // `res` belongs to the current circuit at its current operating point
        bool kept{}, weighted{};
        int n_outputs{}, batch{};
        std::vector<double> res;          // [n_outputs][batch] rss (weighted), then [n_outputs][batch][n_par] sensitivities (kept)
        Ac sys;                           // (declared last: its engines go before the tables and buffers above)
    } sens;
    // multi-port network analysis (pe_hip_analyze_net, pe_net.hpp): the FORWARD real-equivalent system with sweep state of its own, like the
    // noise analysis -- its right-hand-side lists hold port 0's selector instead of the circuit's AC sources, the other ports' selectors are
    // written per pass (k_net_rhs) --, the ports of the last call on the device and its result
    struct Net
    {
        bool have_port0{};
        int pos0{-1}, neg0{-1};           // the port the right-hand-side lists of `sys` select
        Pool port_pool;                   // port rows and reference resistances (PE_HIP_NET_MAX_PORTS each)
        int *d_pos{}, *d_neg{};
        double* d_z0{};
        pe_eng::DevBuf<double> d_res;     // sized by the call: [Z re | Z im | Y re | Y im | S re | S im]
        pe_eng::DevBuf<int> d_status;     // [2][n_points][batch]: Y, then S -- released together with d_res
        pe::NetView V{};
        bool valid{};                     // `res` belongs to the current circuit at its current operating point
        int n_points{}, batch{}, n_ports{};
        std::vector<double> res;          // the six planes, [n_points][batch][n_ports][n_ports] each
        std::vector<int> status;          // [2][n_points][batch]
        Ac sys;                           // (declared last: its engines go before the tables and buffers above)
    } net;
    // pole-zero analysis (pe_hip_analyze_pz, pe_pz.hpp): a FORWARD real-equivalent system with sweep state of its own, like the network
    // analysis -- its right-hand-side lists hold the input port's selector, its engine keeps the factors --, the Arnoldi buffers (sized by
    // batch x max_krylov x 2N: released when a call of another shape comes) and the result of the last call
    struct Pz
    {
        bool have_port{};
        int pos0{-1}, neg0{-1};           // the port the right-hand-side lists of `sys` select
        Pool buf_pool;                    // basis, Hessenberg matrices, z, gain, steps, parked
        size_t buf_batch{}, buf_rows{};
        int buf_m{};
        pe_eng::DevBuf<double> d_res;     // Ritz output [2 kinds][3][batch][max_krylov]: s re | s im | err_est (kind 0: the first kind the call ran)
        pe_eng::DevBuf<int> d_cnt;        // [2 kinds][5][batch]: n_found | n_converged | status of the Ritz kernel | parked | steps at the kind's end
        pe::PzView V{};
        bool valid{};                     // the results below belong to the current circuit at its current operating point
        int batch{}, capacity{}, what{};
        std::vector<double> res[2];       // poles, zeros: [3][batch][capacity]
        std::vector<int> n_found[2], n_conv[2], complete[2], status[2];  // [batch] each
        std::vector<double> gain;         // [batch][2] H(s0)
        Ac sys;                           // (declared last: its engines go before the buffers above)
    } pz;
    long long n_factor_launches{};  // batched numeric factorisations launched by dc_solve / dc_solve_kept on this engine (its first attempt and every retry group)
    // DC sweep (pe_hip_analyze_dc_sweep, pe_dc_sweep.hpp): an engine of its own holding this circuit with batch (circuit batch) x P -- the
    // points of one pass are extra instances --, the buffers of its kernels and the stored result.  The main engine is only read.
    struct DcSweep
    {
        pe_eng::EnginePtr eng;
        int P{};                          // slots per pass the engine was built for
        long long epoch{-1};              // param_epoch of the main engine it was built from (parameters, options, knobs)
        Pool pass_pool;                   // sized by batch x P
        Pool res_pool;                    // sized by the sweep: result and per-pair bookkeeping in the caller's order
        size_t res_pairs{}, res_len{};
        pe_eng::KeptRows kept;            // pe_hip_set_dc_sweep_rows
        pe::DcSweepView V{};
        bool valid{};
        int n_points{}, n_keep{}, batch{};
        std::vector<double> res;          // [n_points][batch][n_keep]
        std::vector<int> status, iters, seed;  // [n_points][batch]
        DcSweep& operator=(DcSweep&&) = default;
        ~DcSweep() { eng.reset(); }
        void drop() { eng.reset(), *this = DcSweep{}; }  // the engine first (it synchronises its stream), then every buffer: a fresh DcSweep
    } dcs;
    // operating point with gmin / source stepping (pe_hip_analyze_op_stepping, pe_op_step.hpp): the controller's per-instance arrays and
    // the shadow of the state a DC solve reads (allocated at the first call, dropped by a circuit load), the log (sized by the call's
    // log_capacity) and whether the arrays hold the outcome of a call on the resident circuit
    struct OpStep
    {
        Pool pool, log_pool;
        bool allocated{}, valid{};
        int log_capacity{-1};
        pe::OpStepView V{};
    } ops;
    long long param_epoch{};  // bumped by whatever changes hc's parameters, the options or the knobs (the DC sweep engine is rebuilt after it)
    std::vector<double> sym_values_override;  // representative |A| values for the row matching (AC engine)
    // A shard of a multi-device sweep (pe_sweep.cpp): the circuit of the SWEEP's first instance, batch 1.  The static pivot order is
    // matched on its values instead of this engine's own instance 0, so that an instance's result does not depend on which device held
    // it (with per-instance switch states the two orders differ, and next to r_open = 1e12 the rounding differs visibly).  Empty: hc.
    std::unique_ptr<pe::HostCircuit> sym_ref;
    // The engine holds the real-equivalent form of a circuit's complex AC system (the AC engine and its sweep engine; set once, where they
    // are built): every analysis of it keeps the greedy row matching (pe_symbolic.cpp).  Rows i and n + i of such a system carry the two
    // halves of the same complex entries, equal in magnitude; a matching that maximises magnitudes row by row is free to take the halves of
    // a complex pivot from two different entries, and on ac_linear_mix it ends on blocks that cancel exactly (a zero pivot).  The greedy one
    // is what the AC goldens were recorded with; these paths refine every solve and re-analyse on failure.
    bool greedy_match{};
    // Set around the analysis of the complex solver seam (pe_engine_seam.cpp), whose real-equivalent layout is known: the complex matrix is
    // matched on the moduli of its entries and every pivot is a 2 x 2 block (pe_symbolic.cpp match_paired).
    bool pair_match{};

    // solve_csr_real seam (separate small state)
    struct Csr
    {
        Pool pool;
        pe::Symbolic sym;
        pe::DevView V{};
        int n{-1}, nnz{-1};
        bool have{};
        bool on_these_values{};                 // the pivot order of the cached analysis was matched on the values of the current call
        double *d_xacc{}, *d_b0{}, *d_worst{};  // residual check: the (refined) solution, the right-hand side, the backward error (owned by pool)
    } csr;
    // ... and its complex twin (pe_engine_seam.cpp): the real-equivalent 2n system, its refinement buffers
    struct Csrz
    {
        Pool pool;
        pe::Symbolic sym;
        pe::DevView V{};
        int n{-1}, nnz{-1};
        bool have{};
        bool on_these_values{};            // the pivot order of the cached analysis was matched on the values of the current call
        std::vector<int> rp2, ci2, pos;    // real-equivalent pattern; the four positions of every complex entry
        std::vector<double> vals, rhs, x;  // host staging
        double *d_xacc{}, *d_b0{}, *d_worst{};  // (owned by pool)
    } csrz;
};

// a failed HIP call is NOT "no device" unless the runtime says so: out-of-memory at a large batch, a launch failure or a
// memcpy error are internal errors of a machine that has a GPU (callers and tests tell them apart)
static inline int hip_error_code(hipError_t e)
{
    return (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver) ? PE_HIP_ERR_NO_DEVICE : PE_HIP_ERR_INTERNAL;
}

#define HIPCHK(h, expr)                                                                             \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if(e__ != hipSuccess)                                                                       \
        {                                                                                           \
            (h)->err = std::string("HIP error: ") + hipGetErrorString(e__) + " at " #expr;          \
            return hip_error_code(e__);                                                             \
        }                                                                                           \
    } while(0)

// the contract of the solver seam's arrays (the reference builds them that way, circuit.h:1171-1226): 0-based CSR, row_ptr monotone from 0 to nnz,
// column indices inside [0, n) and strictly increasing inside a row.  Checked once per pattern: everything behind the seam indexes with these numbers.
static inline char const* csr_pattern_error(int n, int nnz, int const* row_ptr, int const* col_ind)
{
    if(n > 0 && (row_ptr[0] != 0 || row_ptr[n] != nnz)) return "row_ptr[0] != 0 or row_ptr[n] != nnz";
    for(int i = 0; i < n; ++i)
    {
        if(row_ptr[i + 1] < row_ptr[i]) return "row_ptr is not monotone";
        for(int e = row_ptr[i]; e < row_ptr[i + 1]; ++e)
            if(col_ind[e] < 0 || col_ind[e] >= n || (e > row_ptr[i] && col_ind[e] <= col_ind[e - 1])) return "column indices out of range or not sorted inside a row";
    }
    return nullptr;
}

namespace pe_eng PE_ENG_HIDDEN
{
    extern thread_local std::string g_create_error;

    // pe_engine.cpp
    int fail(pe_hip_engine* h, int code, std::string msg);
    double r_open_of(pe_hip_engine const* h);
    void apply_options(pe_hip_engine* h, pe::DevView& V);
    int stats_chunks(int batch);
    int finish_load(pe_hip_engine* h);
    // The one builder of an owned engine: a fresh one on `device` into `out`, emptied first.  With a parent h: under h's knobs and `opt`,
    // holding `hc`, loaded (finish_load) -- a failure is h's error "<name>: ...".  Without (pe_hip_sweep): the defaults, nothing loaded, the
    // message is pe_hip_last_error(nullptr).  On any failure `out` stays empty: nothing half-built is kept.
    int engine_build(int device, EnginePtr& out, pe_hip_engine* h = nullptr, std::string const& name = {}, pe_hip_options const* opt = nullptr, pe::HostCircuit hc = {});
    // a static value of the matrix may have changed: neither the factors nor the full transient stamps of the split schedule stand
    inline void invalidate_factors(pe_hip_engine* h)
    {
        h->resident.fact_valid = false;
        h->resident.a_static.clear();
    }
    void fill_static_dv(pe_hip_engine const* h, std::vector<double>& dv);
    int collect_stats(pe_hip_engine* h, std::vector<long long> const& steps0, std::vector<long long> const& iters0, pe_hip_run_stats* st);
    int snapshot_counters(pe_hip_engine* h, std::vector<long long>& s0, std::vector<long long>& i0);
    // pe_engine_policy.cpp
    bool split_launch(pe_hip_engine const* h);
    int env_int0(char const* name, int def);
    int knob(pe_hip_engine const* h, char const* name, int def);
    int upload_symbolic(pe_hip_engine* h, Pool& pool, pe::Symbolic& S, pe::SymbolicOptions const& so, pe::DevView& V, int batch);
    pe::SymbolicOptions symbolic_options(pe_hip_engine const* h, int batch_in, int rows, int panel_reserve = 384, int force_resident = 0);
    int analyze_fitting(pe_hip_engine* h, int batch, int geometry_rows, int n, int const* rp, int const* ci, double const* vals, pe::Symbolic& S,
                        pe::SymbolicOptions& so, std::vector<char> const* dyn_slots = nullptr, std::vector<char> const* dyn_rows = nullptr);
    int ensure_symbolic(pe_hip_engine* h, bool tr, double dt);
    // after pe_hip_load_circuit of a shard: `tables` as the whole sweep gave them (batched blocks starting at the sweep's instance 0)
    int set_symbolic_reference(pe_hip_engine* h, int n_nodes, int n_branches, int n_tables, pe_hip_device_table const* tables);
    // the solve + residual check + refinement both solver seams share (pe_engine_seam.cpp)
    bool all_finite(double const* x, size_t n);
    int seam_solve_refined(pe_hip_engine* h, pe::DevView const& V, double* xacc, double* b0, double* d_worst, double refine_above, pe_hip_timings& tm,
                           float& gpu_ms, int& status, double& worst);
    // pe_engine.cpp: transient probes
    pe::ProbedView probe_view(pe_hip_engine const* h);  // the engine's view + its armed window (probe_armed set)
    void probe_disarm(pe_hip_engine* h);             // whatever moves x or t other than pe_hip_analyze_tr ends the window (samples stay)
    void probe_drop(pe_hip_engine* h);               // configuration and buffers gone (pe_hip_load_circuit); the Fourier configuration with it
    void fourier_drop(pe_hip_engine* h);             // the Fourier configuration and its buffers gone
    int probe_record_step(pe_hip_engine* h, std::vector<int> const& accepted, double t);  // split schedule: one solved step
    // pe_engine_checkpoint.cpp: every array that makes up the state of an instance, in the order of the checkpoint blob -- shared with the
    // variable-step transient's device-side snapshot so that the two cannot drift
    struct CkPart
    {
        void* ptr;
        size_t bytes;
    };
    std::vector<CkPart> ck_parts(pe_hip_engine* h);
    // pe_engine_newton.cpp: backward Euler / Gear-2
    int integ_alloc(pe_hip_engine* h);    // V.tr_method := the engine's rule; the history array where that rule needs one (restarted); captured sequences dropped
    void integ_restart(pe_hip_engine* h); // h_p := 0 of every instance: the next step starts the history
    // what the bookkeeping of the companion conductances is keyed on: dt under the trapezoidal rule (2C/dt), a0 of the coming step otherwise
    // (NaN, which equals nothing, when the host cannot show that every instance has the same); and the dt whose trapezoidal conductance
    // 2C/dt equals a0 C, for the representative values of the pivot matching
    int integ_before_steps(pe_hip_engine* h);  // the history of the instances whose last step failed restarts (before their status is cleared)
    double integ_key(pe_hip_engine const* h, double dt);
    double integ_sym_dt(pe_hip_engine const* h, double dt);
    // pe_engine_newton.cpp: variable-step transient
    void tr_adaptive_drop(pe_hip_engine* h);  // shadow state, history ring and step log gone (pe_hip_load_circuit)
    void op_step_drop(pe_hip_engine* h);      // controller arrays, shadow and log of the stepped operating point gone (pe_hip_load_circuit)
    // pe_engine_ac.cpp: the stored AC sweep
    // its engine, buffers, row selection and result gone (pe_hip_load_circuit, pe_hip_destroy); the noise, sensitivity and network state
    // (each with its system, both engines, its tables and its result) too
    void ac_sweep_drop(pe_hip_engine* h);
    inline void ac_sweep_invalidate(pe_hip_engine* h)  // whatever moves the operating point or the circuit: the stored sweep, the stored noise and sensitivity results
    {
        h->ac.sweep.valid = false;
        h->noise.valid = false;
        h->sens.valid = false;
        h->net.valid = false;
        h->pz.valid = false;
    }
    // The check every getter of a stored result makes: there is one (`valid`, made at the batch the engine has now) -- else "<name>: no
    // <what> yet" --, and items [first, first + n) of its n_items and instances [first_instance, first_instance + count) lie inside it --
    // else "<name>: <noun> or instances out of range" (noun == nullptr, a per-instance getter: "<name>: instances out of range").
    // Compared as first > total - n: first + n may overflow.
    int stored_window(pe_hip_engine* h, char const* name, char const* what, char const* noun, bool valid, int stored_batch, int n_items, int first, int n,
                      int first_instance, int count);
    // the status of the main engine's instances: b_out = the first whose last analysis failed (it has no operating point to linearise at)
    // with its status, or -1
    int operating_point_status(pe_hip_engine* h, int& b_out, int& status_out);
    // the linearisation the small-signal stamps refer to, from the main engine's device state
    int read_operating_point(pe_hip_engine* h, pe::AcOperatingPoint& op);
    // budget of a sweep engine's automatic pass size, and the most instances one engine takes (the y extent of a launch grid)
    long long sweep_memory_budget();
    constexpr long long SWEEP_MAX_INSTANCES = 65535;
    // points (slots) per pass of a sweep engine at circuit batch B: the knob's value when it is set, else what fits the memory budget at
    // bytes_per_instance (0: unknown -- one per pass); never more than one engine takes as instances
    inline long long sweep_pass_cap(int knob_value, long long bytes_per_instance, int B)
    {
        long long cap = knob_value > 0 ? knob_value : 0;
        if(cap == 0) cap = bytes_per_instance > 0 ? sweep_memory_budget() / (bytes_per_instance * static_cast<long long>(B)) : 1;
        return std::clamp<long long>(cap, 1, std::max<long long>(1, SWEEP_MAX_INSTANCES / B));
    }
    // pe_engine_newton.cpp: the DC sweep
    void dc_sweep_drop(pe_hip_engine* h);  // its engine, buffers, row selection and result gone (pe_hip_load_circuit, pe_hip_destroy)
    // the body of pe_hip_analyze_dc after its argument checks.  clear_status = false: the instances whose status is not OK are left alone
    // (a subset solve: the DC sweep parks the others)
    int dc_solve(pe_hip_engine* h, int mode, pe_hip_run_stats* st, bool clear_status);
    // The same point of every instance with the factors of the last dc_solve KEPT: stamp, the two triangular solves, the residual check --
    // for a linear engine whose matrix values have not changed since that solve (only right-hand-side slots of the value vector have).
    // Built on the split schedule's iteration with do_factor = false, whatever schedule factored.  Where the safety net has to factor
    // again (a retry of the instances it flagged; after a re-match, every instance under the new order) that is counted in
    // n_factor_launches and those factors are the ones a later call keeps.  An engine that keeps no L21 (refactor_every_solve, a
    // non-linear circuit, an overlay) takes dc_solve.  Clears every instance's status first, leaves the stream synchronised.
    int dc_solve_kept(pe_hip_engine* h, int mode, pe_hip_run_stats* st);
    // pe_engine_newton.cpp
    bool has_overlay(pe_hip_engine const* h);
    int overlay_call(pe_hip_engine* h, int event, int mode, double t, double dt, int b = 0);
    int overlay_call_all(pe_hip_engine* h, int event, int mode, double t, double dt, std::vector<int> const* mask);
}  // namespace pe_eng
