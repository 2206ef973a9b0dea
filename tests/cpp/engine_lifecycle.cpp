// engine_lifecycle.cpp -- what an engine owns and what a circuit load resets, through the C ABI of include/pe_hip.h.
// Engine E runs every analysis that allocates something on circuit A (a source, two resistors, a capacitor and a diode), then loads
// circuit B (an R-C divider with another row count and batch); engine F gets the same settings and loads only B.  Whatever they compute
// from there must be the same bits, and every stored result of E must be gone.  Then the multi-device handle, and both engines go.
// With PE_LIFECYCLE_INTERNALS (the stand-alone sanitizer build of tests/test_engine_lifecycle.py, which compiles the engine's sources in)
// the owning types of pe_engine_internal.hpp are checked directly as well.  One main(), exit 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pe_hip.h"
#ifdef PE_LIFECYCLE_INTERNALS
    #include "pe_engine_internal.hpp"
#endif

namespace
{
    int failures = 0;
    void expect(bool ok, char const* what, int line)
    {
        if(ok) return;
        std::fprintf(stderr, "engine_lifecycle.cpp:%d: %s\n", line, what);
        ++failures;
    }
#define EXPECT(c) expect((c), #c, __LINE__)
    // a call that must succeed: the engine's message with the failure
    void ok_at(int rc, pe_hip_engine* h, char const* what, int line)
    {
        if(rc == PE_HIP_OK) return;
        std::fprintf(stderr, "engine_lifecycle.cpp:%d: %s: rc %d: %s\n", line, what, rc, pe_hip_last_error(h));
        ++failures;
    }
#define OK(h, call) ok_at((call), (h), #call, __LINE__)
    // a getter that must refuse with PE_HIP_ERR_ARG and a message that says there is nothing to read
    void refused_at(int rc, pe_hip_engine* h, char const* needle, char const* what, int line)
    {
        std::string const msg = pe_hip_last_error(h);
        if(rc == PE_HIP_ERR_ARG && msg.find(needle) != std::string::npos) return;
        std::fprintf(stderr, "engine_lifecycle.cpp:%d: %s: expected PE_HIP_ERR_ARG with \"%s\", got rc %d: %s\n", line, what, needle, rc, msg.c_str());
        ++failures;
    }
#define REFUSED(h, needle, call) refused_at((call), (h), (needle), #call, __LINE__)

    double const diode[PE_HIP_DIODE_NPARAM] = {1e-14, 1.0, 0.0, 2.0, 27.0, 1e-3, 40.0, 1.0, 1.0, 1e-8, 1.0};

    // circuit A: V 1-0 (branch 0), R1 1-2 (one value per instance), R2 2-3, C 3-0, D 3-0: 3 nodes + 1 branch = 4 rows
    int load_a(pe_hip_engine* h, int batch)
    {
        int const vn[2] = {1, 0}, vb[1] = {0}, rn[4] = {1, 2, 2, 3}, cn[2] = {3, 0}, dn[2] = {3, 0};
        double const vpar[1] = {2.0}, cpar[1] = {1e-9};
        std::vector<double> rpar(static_cast<size_t>(batch) * 2);
        for(int b = 0; b < batch; ++b) rpar[2 * b] = 500.0 + 37.0 * b, rpar[2 * b + 1] = 1000.0;
        pe_hip_device_table t[4]{};
        t[0] = {PE_HIP_VDC, 1, vn, vb, vpar, 0};
        t[1] = {PE_HIP_R, 2, rn, nullptr, rpar.data(), 1};
        t[2] = {PE_HIP_C, 1, cn, nullptr, cpar, 0};
        t[3] = {PE_HIP_DIODE, 1, dn, nullptr, diode, 0};
        return pe_hip_load_circuit(h, 3, 1, batch, 4, t);
    }
    // circuit B: V 1-0 (branch 0), R 1-2 (one value per instance), C 2-0: 2 nodes + 1 branch = 3 rows, batch 2
    constexpr int B_ROWS = 3, B_BATCH = 2;
    int load_b(pe_hip_engine* h)
    {
        int const vn[2] = {1, 0}, vb[1] = {0}, rn[2] = {1, 2}, cn[2] = {2, 0};
        double const vpar[1] = {1.5}, rpar[2] = {1000.0, 2200.0}, cpar[1] = {2e-9};
        pe_hip_device_table t[3]{};
        t[0] = {PE_HIP_VDC, 1, vn, vb, vpar, 0};
        t[1] = {PE_HIP_R, 1, rn, nullptr, rpar, 1};
        t[2] = {PE_HIP_C, 1, cn, nullptr, cpar, 0};
        return pe_hip_load_circuit(h, 2, 1, B_BATCH, 3, t);
    }

    pe_hip_engine* fresh_engine()
    {
        pe_hip_engine* h{};
        OK(nullptr, pe_hip_create(0, &h));
        if(!h) return nullptr;
        pe_hip_options opt{};
        opt.g_min = 1e-12;
        opt.refactor_every_solve = 1;
        OK(h, pe_hip_set_knob(h, "SPLIT", 1));
        OK(h, pe_hip_set_options(h, &opt));
        OK(h, pe_hip_set_tr_method(h, PE_HIP_TR_BE));
        return h;
    }

    // every analysis that allocates: what E does on circuit A before it loads B
    void run_everything_on_a(pe_hip_engine* h, int batch)
    {
        OK(h, load_a(h, batch));
        pe_hip_run_stats st{};
        OK(h, pe_hip_analyze_dc(h, PE_HIP_MODE_OP, &st));
        int const probe_rows[2] = {2, 3};
        pe_hip_measure const meas[1] = {{PE_HIP_MEAS_MAX, 0, 0, 1, 0.0}};
        OK(h, pe_hip_set_probes(h, 2, probe_rows, 16, 1, 1, meas));
        int const fp[1] = {0};
        pe_hip_fourier_control const four = {250e3, 0.0, 2, 3, 1, fp};
        OK(h, pe_hip_set_fourier(h, &four));
        OK(h, pe_hip_arm_probes(h));
        OK(h, pe_hip_analyze_tr(h, 1e-6, 8, &st));
        {
            std::vector<int> n_rec(static_cast<size_t>(batch));
            OK(h, pe_hip_get_probe_samples(h, 0, batch, nullptr, nullptr, n_rec.data(), nullptr));
            EXPECT(n_rec[0] == 9);  // (the point of arming + 8 steps)
            std::vector<double> covered(static_cast<size_t>(batch));
            OK(h, pe_hip_get_fourier(h, 0, batch, nullptr, nullptr, covered.data()));
            EXPECT(covered[0] > 0.0);
        }
        {
            pe_hip_tr_control c{};
            c.dt_init = 1e-6;
            c.max_steps = 4;
            pe_hip_tr_adaptive_stats ts{};
            OK(h, pe_hip_analyze_tr_adaptive(h, 1e-3, &c, &ts));
            EXPECT(ts.n_accepted + ts.n_rejected_lte + ts.n_rejected_newton == 4);
        }
        {
            pe_hip_op_step_control c{};
            c.method = PE_HIP_STEP_AUTO;
            c.log_capacity = 4;
            pe_hip_op_step_stats os{};
            OK(h, pe_hip_analyze_op_stepping(h, PE_HIP_MODE_OP, &c, &os));
            std::vector<int> phase(static_cast<size_t>(batch));
            OK(h, pe_hip_get_op_step_state(h, 0, batch, phase.data(), nullptr, nullptr, nullptr, nullptr));
        }
        double const omegas[3] = {1e3, 1e5, 1e7};
        std::vector<double> re(static_cast<size_t>(3) * batch * 4), im(re.size());
        {
            pe_hip_ac_sweep_stats as{};
            OK(h, pe_hip_analyze_ac_sweep(h, 3, omegas, nullptr, &as));
            OK(h, pe_hip_get_ac_sweep(h, 0, 3, 0, batch, re.data(), im.data()));
        }
        {
            pe_hip_noise_control const c = {2, -1, 0.0, 0};
            pe_hip_noise_stats ns{};
            OK(h, pe_hip_analyze_noise(h, 3, omegas, &c, nullptr, &ns));
            OK(h, pe_hip_get_noise(h, 0, 3, 0, batch, re.data(), nullptr));
        }
        {
            int const pos[1] = {2}, neg[1] = {-1};
            pe_hip_sens_control c{};
            c.n_outputs = 1;
            c.out_pos = pos;
            c.out_neg = neg;
            c.keep_sensitivities = 1;
            pe_hip_sens_stats ss{};
            OK(h, pe_hip_analyze_sens(h, &c, nullptr, &ss));
            std::vector<double> s(static_cast<size_t>(batch) * ss.n_params);
            OK(h, pe_hip_get_sens(h, 0, 1, 0, batch, s.data(), nullptr));  // (no weights: no weighted sum to read)
        }
        {
            int const pos[1] = {2}, neg[1] = {-1};
            pe_hip_net_control const c = {1, pos, neg, nullptr};
            pe_hip_net_stats ns{};
            OK(h, pe_hip_analyze_net(h, 3, omegas, &c, nullptr, &ns));
            OK(h, pe_hip_get_net(h, 0, 0, 3, 0, batch, re.data(), im.data()));
        }
        {
            double const values[3] = {1.0, 2.0, 3.0};
            pe_hip_dc_sweep_control const c = {PE_HIP_VDC, 0, 0, PE_HIP_MODE_OP, PE_HIP_DC_SWEEP_PARALLEL, 1, 0};
            pe_hip_dc_sweep_stats ds{};
            OK(h, pe_hip_analyze_dc_sweep(h, 3, values, &c, nullptr, &ds));
            OK(h, pe_hip_get_dc_sweep(h, 0, 3, 0, batch, re.data()));
        }
        std::vector<double> stat(4 * 4);
        OK(h, pe_hip_sweep_statistics(h, stat.data()));
    }

    // what an engine computes on B and reports about it, as bytes
    struct Outcome
    {
        std::vector<double> x, t;
        std::vector<int> status, trace;
        std::vector<long long> steps, iters;
        pe_hip_info info;
        long long refined, rematched, skipped, full, after_ref, skipped_after_ref;
        int careful, tr_method, knob, knob_set;
    };
    Outcome run_on_b(pe_hip_engine* h)
    {
        Outcome o{};
        pe_hip_run_stats st{};
        OK(h, pe_hip_analyze_dc(h, PE_HIP_MODE_OP, &st));
        OK(h, pe_hip_analyze_tr(h, 1e-6, 8, &st));
        o.x.resize(static_cast<size_t>(B_BATCH) * B_ROWS);
        o.t.resize(B_BATCH), o.status.resize(B_BATCH), o.steps.resize(B_BATCH), o.iters.resize(B_BATCH);
        OK(h, pe_hip_get_solution(h, 0, B_BATCH, o.x.data()));
        OK(h, pe_hip_get_instance_state(h, 0, B_BATCH, o.status.data(), o.steps.data(), o.iters.data(), o.t.data()));
        int n = 0;
        o.trace.resize(64);
        OK(h, pe_hip_get_newton_trace(h, 64, o.trace.data(), &n));
        o.trace.resize(static_cast<size_t>(n < 64 ? n : 64));
        OK(h, pe_hip_get_info(h, &o.info));
        OK(h, pe_hip_get_safety_net_counters(h, &o.refined, &o.rematched, &o.careful));
        OK(h, pe_hip_get_static_skip_stats(h, &o.skipped, &o.full));
        OK(h, pe_hip_get_static_skip_refinement_stats(h, &o.after_ref, &o.skipped_after_ref));
        OK(h, pe_hip_get_tr_method(h, &o.tr_method));
        OK(h, pe_hip_get_knob(h, "SPLIT", &o.knob, &o.knob_set));
        return o;
    }
    template <class T>
    bool same_bits(std::vector<T> const& a, std::vector<T> const& b)
    {
        return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
    }

    void lifecycle(int batch_a)
    {
        pe_hip_engine* E{};
        OK(nullptr, pe_hip_create(0, &E));
        pe_hip_destroy(E);  // (an engine that never held anything)
        E = fresh_engine();
        pe_hip_engine* F = fresh_engine();
        if(!E || !F) return;
        run_everything_on_a(E, batch_a);
        OK(E, load_b(E));
        OK(F, load_b(F));
        // every stored result of E belonged to A
        double d[64];
        int i[64];
        REFUSED(E, "no AC sweep yet", pe_hip_get_ac_sweep(E, 0, 1, 0, 1, d, d));
        REFUSED(E, "no noise analysis yet", pe_hip_get_noise(E, 0, 1, 0, 1, d, nullptr));
        REFUSED(E, "no sensitivity analysis yet", pe_hip_get_sens(E, 0, 1, 0, 1, d, d));
        REFUSED(E, "no network analysis yet", pe_hip_get_net(E, 0, 0, 1, 0, 1, d, d));
        REFUSED(E, "no DC sweep yet", pe_hip_get_dc_sweep(E, 0, 1, 0, 1, d));
        REFUSED(E, "no stepping call yet", pe_hip_get_op_step_state(E, 0, 1, i, nullptr, nullptr, nullptr, nullptr));
        REFUSED(E, "no probe configuration", pe_hip_get_probe_samples(E, 0, 1, nullptr, nullptr, i, nullptr));
        REFUSED(E, "no probe configuration", pe_hip_get_measures(E, 0, 1, d));
        Outcome const e = run_on_b(E), f = run_on_b(F);
        EXPECT(same_bits(e.x, f.x));
        EXPECT(same_bits(e.t, f.t));
        EXPECT(same_bits(e.status, f.status));
        EXPECT(same_bits(e.steps, f.steps));
        EXPECT(same_bits(e.iters, f.iters));
        EXPECT(same_bits(e.trace, f.trace));
        EXPECT(std::memcmp(&e.info, &f.info, sizeof(pe_hip_info)) == 0);
        EXPECT(e.refined == f.refined && e.rematched == f.rematched && e.careful == f.careful);
        EXPECT(e.skipped == f.skipped && e.full == f.full);
        EXPECT(e.after_ref == f.after_ref && e.skipped_after_ref == f.skipped_after_ref);
        EXPECT(e.tr_method == PE_HIP_TR_BE && f.tr_method == PE_HIP_TR_BE);
        EXPECT(e.knob == 1 && e.knob_set == 1 && f.knob == 1 && f.knob_set == 1);
        EXPECT(e.status[0] == PE_HIP_OK && e.steps[0] == 8 && std::isfinite(e.x[1]));
        // the multi-device handle: its engines go with it; a mask that names no device leaves nothing behind
        {
            pe_hip_sweep* s{};
            EXPECT(pe_hip_sweep_create(1u, &s) == PE_HIP_OK && s);
            if(s)
            {
                int const vn[2] = {1, 0}, vb[1] = {0}, rn[2] = {1, 2}, cn[2] = {2, 0};
                double const vpar[1] = {1.5}, rpar[2] = {1000.0, 2200.0}, cpar[1] = {2e-9};
                pe_hip_device_table t[3]{};
                t[0] = {PE_HIP_VDC, 1, vn, vb, vpar, 0};
                t[1] = {PE_HIP_R, 1, rn, nullptr, rpar, 1};
                t[2] = {PE_HIP_C, 1, cn, nullptr, cpar, 0};
                EXPECT(pe_hip_sweep_load_circuit(s, 2, 1, B_BATCH, 3, t) == PE_HIP_OK);
                pe_hip_run_stats st{};
                EXPECT(pe_hip_sweep_operating_point(s, PE_HIP_MODE_DC, &st) == PE_HIP_OK);
                pe_hip_sweep_destroy(s);
            }
            pe_hip_sweep* none = reinterpret_cast<pe_hip_sweep*>(&s);
            EXPECT(pe_hip_sweep_create(1u << 31, &none) == PE_HIP_ERR_ARG && none == nullptr);
        }
        pe_hip_destroy(E);
        pe_hip_destroy(F);
    }

#ifdef PE_LIFECYCLE_INTERNALS
    // the owning types themselves (the sanitizers check that nothing is freed twice and nothing is left)
    void owners()
    {
        using namespace pe_eng;
        {
            Pinned<int> p;
            EXPECT(p.ensure_at_least(8) == hipSuccess && p.data() && p.capacity() == 8);
            int* const first = p.data();
            EXPECT(p.ensure_at_least(5) == hipSuccess && p.data() == first && p.capacity() == 8);  // (kept while it is large enough)
            EXPECT(p.ensure_at_least(8) == hipSuccess && p.data() == first);
            p.data()[7] = 1;
            EXPECT(p.ensure_at_least(4096) == hipSuccess && p.capacity() == 4096);  // (replaced when more is asked for)
            p.data()[4095] = 1;
            Pinned<int> q{std::move(p)};
            EXPECT(!p.data() && p.capacity() == 0 && q.capacity() == 4096);  // (the moved-from one frees nothing)
            Pinned<int> r;
            EXPECT(r.ensure_at_least(2) == hipSuccess);
            r = std::move(q);  // (what r held is freed)
            EXPECT(!q.data() && r.capacity() == 4096);
            Pinned<char> m;
            EXPECT(m.ensure_at_least(64, hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess && m.device());
        }
        {
            Event a;
            EXPECT(a.create() == hipSuccess && a.h);
            Event b{std::move(a)};
            EXPECT(!a.h && b.h);
            Event c;
            EXPECT(c.create() == hipSuccess);
            c = std::move(b);  // (c's own event is destroyed)
            EXPECT(!b.h && c.h);
            Stream s;
            EXPECT(s.create() == hipSuccess);
        }
        {
            EnginePtr e;
            EXPECT(engine_build(0, e) == PE_HIP_OK && e);
            EnginePtr f{std::move(e)};
            EXPECT(!e && f);
            EXPECT(engine_build(0, f) == PE_HIP_OK && f);  // (the engine f held is destroyed first)
            EXPECT(engine_build(1 << 20, f) != PE_HIP_OK && !f);  // (a failure leaves nothing)
        }
        // a fresh state assigned over a built one, WITHOUT its drop(): the engine goes, then the buffers
        pe_hip_engine* G = fresh_engine();
        if(!G) return;
        run_everything_on_a(G, 3);
        EXPECT(G->dcs.eng && G->ac.sweep.eng && G->ac.eng);
        G->dcs = pe_hip_engine::DcSweep{};
        G->ac.sweep = pe_hip_engine::Ac::Sweep{};
        G->ac = pe_hip_engine::Ac{};
        EXPECT(!G->dcs.eng && !G->ac.eng && !G->ac.built);
        pe_hip_run_stats st{};
        OK(G, pe_hip_analyze_dc(G, PE_HIP_MODE_OP, &st));
        OK(G, pe_hip_analyze_ac(G, 1e4, &st));  // (built again from nothing)
        pe_hip_destroy(G);
    }
#endif
}  // namespace

int main()
{
    if(pe_hip_device_count() <= 0)
    {
        std::fprintf(stderr, "no HIP device visible: the MI355X engine has no CPU fallback\n");
        return 2;
    }
    bool const emulated = std::strcmp(pe_hip_build_id(), "host-emulation") == 0;
    lifecycle(3);
    if(!emulated) lifecycle(33);  // (captured launch sequences up to 32 instances, plain launches above)
#ifdef PE_LIFECYCLE_INTERNALS
    owners();
#endif
    if(failures) std::fprintf(stderr, "engine_lifecycle: %d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
