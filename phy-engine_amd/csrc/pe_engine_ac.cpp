// pe_engine_ac.cpp -- small-signal AC on the device: pe_hip_analyze_ac / pe_hip_get_solution_ac (the real-equivalent system of pe_ac.hpp
// solved by a second engine, iterative refinement on the device) and pe_hip_analyze_ac_sweep / pe_hip_get_ac_sweep (a whole frequency
// sweep as batches of that system on a third engine, pe_ac_sweep.hpp), and pe_hip_analyze_noise / pe_hip_get_noise* (the same sweep body
// on the adjoint system, pe_noise.hpp), and pe_hip_analyze_sens / pe_hip_get_sens* (the same body on the adjoint system at omega = 0, one
// point per output, pe_sens.hpp), and pe_hip_analyze_net / pe_hip_get_net* / pe_hip_convert_net (the same body on a forward system of its
// own with one right-hand side per port on one factorisation per pass, pe_net.hpp), and pe_hip_analyze_pz / pe_hip_get_pz* /
// pe_hip_eig_hessenberg (the same body once more: one pass of one point, every Arnoldi step a right-hand side on the kept factors, pe_pz.hpp).
#include "pe_engine_internal.hpp"

#include <functional>

using namespace pe_eng;

namespace
{
    // the real-equivalent AC system of the resident circuit and the second engine that solves it, built on first use (A: h->ac, or with
    // `adjoint` the transposed system of the noise analysis, h->noise.sys)
    int ensure_ac_built(pe_hip_engine* h, pe_hip_engine::Ac& A, pe::AcAdjoint const* adjoint = nullptr)
    {
        auto& hc = h->hc;
        if(A.built) return PE_HIP_OK;
        if(!pe::build_ac_circuit(hc, A.circ, has_overlay(h) ? &h->overlay : nullptr, adjoint)) return fail(h, PE_HIP_ERR_INTERNAL, "analyze_ac: could not build the AC system");
        // The right-hand side of the device copy comes from one value slot per row: the host evaluates the sources' lists
        // and, for the refinement steps below, writes residuals there.
        {
            auto& c = A.circ.hc;
            A.b_ptr0 = c.b_ptr;
            A.b_src0 = c.b_src;
            A.rhs0 = c.dv_len;
            c.dv_len += c.rows;
            c.b_ptr.resize(c.rows + 1);
            c.b_src.resize(c.rows);
            for(int r = 0; r <= c.rows; ++r) c.b_ptr[r] = r;
            for(int r = 0; r < c.rows; ++r) c.b_src[r] = (A.rhs0 + r) << 1;
        }
        // (the real-equivalent system is analysed under the same tuning knobs)
        if(int const rc = engine_build(h->device, A.eng, h, "analyze_ac", &h->opt, A.circ.hc); rc != PE_HIP_OK) return rc;
        A.eng->greedy_match = true;  // (every analysis of this engine: pe_engine_internal.hpp)
        A.built = true;
        A.sym_omega = -1.0;
        return PE_HIP_OK;
    }
    int ensure_ac_built(pe_hip_engine* h) { return ensure_ac_built(h, h->ac); }

    // ---- frequency-batched sweep (pe_hip_analyze_ac_sweep, and on the adjoint system pe_hip_analyze_noise)
    void sweep_engine_drop(pe_hip_engine::Ac::Sweep& W)
    {
        W.eng.reset();  // (synchronises its stream first: nothing reads the buffers below any more)
        W.P = 0;
        W.b0_valid = false;
        W.pass_pool.release();
    }

    // the third engine: the AC system with batch (circuit batch) x P, constructed like A.eng, and the buffers sized by that batch
    // keep_factors: the engine stores L21 too, so that a later solve can run on the factors of an earlier one (the network analysis decides
    // itself when they are valid: pe_hip_options.refactor_every_solve speaks of the main engine's transient)
    int sweep_engine_build(pe_hip_engine* h, pe_hip_engine::Ac& A, int P, std::string const& name, bool keep_factors = false)
    {
        auto& W = A.sweep;
        sweep_engine_drop(W);
        pe_hip_options opt = h->opt;
        if(keep_factors) opt.refactor_every_solve = 0;
        pe::HostCircuit c = A.circ.hc;
        c.batch = h->hc.batch * P;
        if(int const rc = engine_build(h->device, W.eng, h, name, &opt, std::move(c)); rc != PE_HIP_OK) return rc;
        W.eng->greedy_match = true;  // (as A.eng)
        size_t const Q = static_cast<size_t>(h->hc.batch) * P, R2 = static_cast<size_t>(A.circ.hc.rows);
        double* omega{};
        int* point{};
        HIPCHK(h, W.pass_pool.alloc(W.V.xacc, Q * R2));
        HIPCHK(h, W.pass_pool.alloc(W.V.b0, Q * R2));
        HIPCHK(h, W.pass_pool.alloc(W.V.worst, Q));
        HIPCHK(h, W.pass_pool.alloc(W.V.n_above, 1));
        HIPCHK(h, W.pass_pool.alloc(omega, static_cast<size_t>(P)));
        HIPCHK(h, W.pass_pool.alloc(point, static_cast<size_t>(P)));
        W.V.omega = omega;
        W.V.point = point;
        W.V.P = P;
        W.P = P;
        return PE_HIP_OK;
    }

}  // namespace

namespace pe_eng
{
    // budget of the automatic pass size: half of the device's free memory, at most 4 GiB -- every band's symbolic analysis allocates the
    // factor storage of the whole batch again, and past a few hundred instances of a large circuit a pass gains nothing (the band's
    // host-side analysis dominates it; measured: DESIGN.md).  Builds without HIP have no such query and take a fixed budget.
    long long sweep_memory_budget()
    {
#if defined(__HIPCC__)
        size_t free_b = 0, total_b = 0;
        if(hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) return std::min<long long>(static_cast<long long>(free_b / 2), 4ll << 30);
#endif
        return 256ll << 20;
    }

    // The forward sweep of h->ac (its single-point engine goes with h->ac.drop()), then the noise, sensitivity and network analyses: each
    // its system with both engines first, then -- by assigning a fresh state, whose pools free what they hold -- tables, buffers, result.
    void ac_sweep_drop(pe_hip_engine* h)
    {
        h->ac.sweep.drop();
        h->noise.sys.drop();
        h->noise = pe_hip_engine::Noise{};
        h->sens.sys.drop();
        h->sens = pe_hip_engine::Sens{};
        h->net.sys.drop();
        h->net = pe_hip_engine::Net{};
        h->pz.sys.drop();
        h->pz = pe_hip_engine::Pz{};
    }

    int KeptRows::set(pe_hip_engine* h, char const* name, int n_rows, int const* rows_in)
    {
        if(!h->loaded || n_rows < 0 || (n_rows > 0 && !rows_in)) return fail(h, PE_HIP_ERR_ARG, std::string(name) + ": bad arguments or no circuit");
        for(int k = 0; k < n_rows; ++k)
            if(rows_in[k] < 0 || rows_in[k] >= h->hc.rows) return fail(h, PE_HIP_ERR_ARG, std::string(name) + ": row out of range");
        rows.assign(rows_in, rows_in + n_rows);
        on_device = false;
        return PE_HIP_OK;
    }

    int KeptRows::upload(pe_hip_engine* h, int const*& keep_out)
    {
        if(on_device) return PE_HIP_OK;
        keep_out = nullptr;
        if(rows.size() > cap)
        {
            if(d_keep) (void)hipFree(d_keep);
            d_keep = nullptr;
            cap = 0;
            HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&d_keep), rows.size() * sizeof(int)));
            cap = rows.size();
        }
        if(!rows.empty())
        {
            HIPCHK(h, hipMemcpy(d_keep, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice));
            keep_out = d_keep;
        }
        on_device = true;
        return PE_HIP_OK;
    }

    int stored_window(pe_hip_engine* h, char const* name, char const* what, char const* noun, bool valid, int stored_batch, int n_items, int first, int n,
                      int first_instance, int count)
    {
        if(!valid || stored_batch != h->hc.batch) return fail(h, PE_HIP_ERR_ARG, std::string(name) + ": no " + what + " yet");
        bool const items_ok = !noun || (first >= 0 && n >= 0 && first <= n_items - n);
        if(!items_ok || first_instance < 0 || count < 0 || first_instance > stored_batch - count)
            return fail(h, PE_HIP_ERR_ARG, std::string(name) + ": " + (noun ? std::string(noun) + " or " : std::string()) + "instances out of range");
        return PE_HIP_OK;
    }

    int operating_point_status(pe_hip_engine* h, int& b_out, int& status_out)
    {
        int const B = h->hc.batch;
        std::vector<int> inst(static_cast<size_t>(B), 0);
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipMemcpy(inst.data(), h->V.status, static_cast<size_t>(B) * sizeof(int), hipMemcpyDeviceToHost));
        auto const bad = std::find_if(inst.begin(), inst.end(), [](int s) { return s != PE_HIP_OK; });
        b_out = bad == inst.end() ? -1 : static_cast<int>(bad - inst.begin());
        status_out = bad == inst.end() ? PE_HIP_OK : *bad;
        return PE_HIP_OK;
    }

    int read_operating_point(pe_hip_engine* h, pe::AcOperatingPoint& op)
    {
        auto const& hc = h->hc;
        size_t const B = static_cast<size_t>(hc.batch);
        op.d_geq.resize(B * hc.nD());
        op.dv.resize(B * hc.dv_len);
        op.rl_engaged.resize(B * hc.nRl());
        if(!op.d_geq.empty()) HIPCHK(h, hipMemcpy(op.d_geq.data(), h->V.d_geq, op.d_geq.size() * sizeof(double), hipMemcpyDeviceToHost));
        if(!op.dv.empty()) HIPCHK(h, hipMemcpy(op.dv.data(), h->V.dv, op.dv.size() * sizeof(double), hipMemcpyDeviceToHost));
        if(!op.rl_engaged.empty()) HIPCHK(h, hipMemcpy(op.rl_engaged.data(), h->V.rl_engaged, op.rl_engaged.size() * sizeof(int), hipMemcpyDeviceToHost));
        return PE_HIP_OK;
    }

    // The static pivot order of a batch is matched on instance 0's values and holds for every instance.  A contact cell -- (k, k) of a
    // switch or a relay -- is -r_open where the contact is open and exactly 0 where it is closed: with instance 0 open, the matching
    // takes that cell for a pivot and every instance with the contact closed meets a zero pivot.  `rep`: the representative values per
    // CSR slot of the AC system, from instance 0; vals [B][stride]: the value vectors of the instances.  A slot fed by a contact value
    // that is 0 in some instance gets the representative value 0: the order then pivots on the incidence entries, as it does when
    // instance 0's contact is closed.  Batches whose instances agree on their contact states keep the order they had.
    void ac_mask_contacts_closed_elsewhere(pe::HostCircuit const& hc, pe::AcCircuit const& circ, double const* vals, size_t stride, std::vector<double>& rep)
    {
        int const B = hc.batch;
        if(B < 2) return;
        std::vector<char> closed_elsewhere(static_cast<size_t>(pe::DV_FIXED) + circ.slots.size(), 0);
        bool any = false;
        for(size_t i = 0; i < circ.slots.size(); ++i)
        {
            auto const& sl = circ.slots[i];
            if(!(sl.kind == pe::AcSlot::RELAY_R || (sl.kind == pe::AcSlot::GEN_STATIC && hc.gen[static_cast<size_t>(sl.idx)].kind == PE_HIP_SWITCH))) continue;
            size_t const v = pe::DV_FIXED + i;
            if(vals[v] == 0.0) continue;
            for(int b = 1; b < B && !closed_elsewhere[v]; ++b) closed_elsewhere[v] = vals[static_cast<size_t>(b) * stride + v] == 0.0;
            any = any || closed_elsewhere[v];
        }
        if(!any) return;
        auto const& ah = circ.hc;
        for(size_t s = 0; s < ah.ci.size(); ++s)
            for(int e = ah.a_ptr[s]; e < ah.a_ptr[s + 1]; ++e)
                if(ah.a_src[e] >= 0 && closed_elsewhere[static_cast<size_t>(ah.a_src[e] >> 1)]) rep[s] = 0.0;
    }
}  // namespace pe_eng

extern "C" {

/* Small-signal AC at angular frequency omega (circult::solve_once with iterate_ac, run once per sweep point by
 * run_ac_analysis, circuit.h:389-431): complex MNA system of the devices' AC stamps, non-linear devices at their LAST
 * linearisation (run pe_hip_analyze_dc(OP) first, as circuit.h:196-209 / the ACOP case do), solved in real-equivalent form. */
int pe_hip_analyze_ac(pe_hip_engine* h, double omega, pe_hip_run_stats* st)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if(st) std::memset(st, 0, sizeof(*st));
    auto& hc = h->hc;
    if(hc.rows == 0) return PE_HIP_OK;
    auto& A = h->ac;
    if(int const brc = ensure_ac_built(h); brc != PE_HIP_OK) return brc;
    int const B = hc.batch;
    // the linearisation the small-signal stamps refer to
    pe::AcOperatingPoint op;
    if(int const rc = read_operating_point(h, op); rc != PE_HIP_OK) return rc;
    auto const& ah = A.circ.hc;
    std::vector<double> dv(static_cast<size_t>(B) * ah.dv_len);
    if(has_overlay(h))
    {
        h->ov_x.resize(static_cast<size_t>(hc.rows));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    for(int b = 0; b < B; ++b)
    {
        if(has_overlay(h))
        {
            // host-stamped models: their iterate_ac hooks stamp complex values at this omega around the operating point held in x -- per
            // instance, as the transient path does (PE_HIP_OVERLAY_INSTANCE tells the callback whose state the call concerns); the
            // reference runs every model's iterate_ac in its AC loop, circuit.h:389-431
            if(B > 1 && h->overlay_fn(h->overlay_user, PE_HIP_OVERLAY_INSTANCE, b, omega, 0.0, nullptr, nullptr, nullptr) != 0)
                return fail(h, PE_HIP_ERR_INTERNAL, "analyze_ac: host-stamp overlay: the callback refused PE_HIP_OVERLAY_INSTANCE (it does not support batches)");
            op.ov_a.assign(2 * static_cast<size_t>(hc.n_ov_a), 0.0);
            op.ov_b.assign(2 * static_cast<size_t>(hc.n_ov_b), 0.0);
            HIPCHK(h, hipMemcpy(h->ov_x.data(), h->V.x + static_cast<size_t>(b) * hc.rows, static_cast<size_t>(hc.rows) * sizeof(double), hipMemcpyDeviceToHost));
            if(h->overlay_fn(h->overlay_user, PE_HIP_OVERLAY_AC, PE_HIP_MODE_OP, omega, 0.0, h->ov_x.data(), op.ov_a.data(), op.ov_b.data()) != 0)
                return fail(h, PE_HIP_ERR_INTERNAL, "analyze_ac: host-stamp overlay: a model's iterate_ac hook failed");
        }
        pe::fill_ac_values(hc, A.circ, op, b, omega, h->opt.g_min, r_open_of(h), &dv[static_cast<size_t>(b) * ah.dv_len]);
    }
    // The pivot order is static (row matching + ordering on representative values): it is (re)made on the values of
    // instance 0 at this frequency when there is none yet, when omega moved more than a decade away from the one it was made
    // for (reactive entries scale with omega), or when a solve with a stale order hits a bad pivot.
    auto analyse_here = [&]()
    {
        int const nnz = static_cast<int>(ah.ci.size());
        A.eng->sym_values_override.assign(nnz, 0.0);
        for(int s = 0; s < nnz; ++s)
        {
            double acc = 0.0;
            for(int e = ah.a_ptr[s]; e < ah.a_ptr[s + 1]; ++e)
            {
                double const v = dv[ah.a_src[e] >> 1];
                acc = (ah.a_src[e] & 1) ? acc - v : acc + v;
            }
            A.eng->sym_values_override[s] = acc;
        }
        ac_mask_contacts_closed_elsewhere(hc, A.circ, dv.data(), static_cast<size_t>(ah.dv_len), A.eng->sym_values_override);
        A.eng->resident.sym_class = -1;
        A.sym_omega = omega;
    };
    bool const stale = A.sym_omega < 0.0 || (omega == 0.0) != (A.sym_omega == 0.0) ||
                       (omega != 0.0 && (omega > 10.0 * A.sym_omega || omega < 0.1 * A.sym_omega));
    if(stale) analyse_here();
    // the right-hand side of every instance goes into its value slots (the device copy of the system gathers it from there)
    int const R2 = ah.rows;
    auto gather = [&](int const* ptr, int const* src, double const* d, int s)
    {
        double acc = 0.0;
        for(int e = ptr[s]; e < ptr[s + 1]; ++e) acc = (src[e] & 1) ? acc - d[src[e] >> 1] : acc + d[src[e] >> 1];
        return acc;
    };
    for(int b = 0; b < B; ++b)
    {
        double* d = &dv[static_cast<size_t>(b) * ah.dv_len];
        for(int r = 0; r < R2; ++r) d[A.rhs0 + r] = gather(A.b_ptr0.data(), A.b_src0.data(), d, r);
    }
    HIPCHK(h, A.d_xacc.ensure(static_cast<size_t>(B) * R2, false));
    HIPCHK(h, A.d_b0.ensure(static_cast<size_t>(B) * R2, false));
    HIPCHK(h, A.d_worst.ensure(1, false));
    auto solve = [&](bool upload) -> int
    {
        // every AC point is an independent linear solve: no sticky failure state, no history.  A correction solve keeps the device's
        // value vector: its right-hand-side slots hold the residual the kernel before wrote there.
        if(upload) HIPCHK(h, hipMemcpy(A.eng->V.dv, dv.data(), dv.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemset(A.eng->V.status, 0, static_cast<size_t>(B) * sizeof(int)));
        return pe_hip_analyze_dc(A.eng.get(), PE_HIP_MODE_DC, st);
    };
    A.b0_valid = false;
    int rc = solve(true);
    if(rc == PE_HIP_ERR_SINGULAR && A.sym_omega != omega)
    {
        analyse_here();
        rc = solve(true);
    }
    if(rc != PE_HIP_OK) return fail(h, rc, "analyze_ac: " + A.eng->err);
    // Iterative refinement, on the device (the pivot order is static and the real-equivalent form separates the two halves of a
    // complex pivot: entries like r_open = 1e12 next to j omega C leave errors far above rounding): r = b - A x in fp64 from the
    // system as the device assembled it (k_ac_residual), A dx = r with the same pivot order, x += dx (k_ac_accumulate); at most
    // three rounds, stops once the componentwise backward error is at rounding level.  The host reads one double per round.
    // One rule with the sweep (run_pass below): a backward error that is not a number needs refinement like one above the threshold
    // (pe::ac_needs_refinement), the iterate the last correction produced gets a residual evaluation of its own, and phasors whose final
    // backward error is not finite are not returned as PE_HIP_OK.
    hipStream_t const es = A.eng->stream;
    HIPCHK(h, pe::launch_ac_accumulate(es, A.eng->V, A.d_xacc.p, A.d_b0.p, true));
    A.b0_valid = true;
    double worst = 0.0;
    for(int round = 0;; ++round)
    {
        HIPCHK(h, pe::launch_ac_residual(es, A.eng->V, A.d_xacc.p, A.d_b0.p, A.rhs0, A.d_worst.p));
        HIPCHK(h, hipMemcpyAsync(&worst, A.d_worst.p, sizeof(double), hipMemcpyDeviceToHost, es));
        HIPCHK(h, hipStreamSynchronize(es));
        if(!pe::ac_needs_refinement(worst) || round == 3) break;
        rc = solve(false);
        if(rc != PE_HIP_OK) return fail(h, rc, "analyze_ac (refinement): " + A.eng->err);
        HIPCHK(h, pe::launch_ac_accumulate(es, A.eng->V, A.d_xacc.p, A.d_b0.p, false));
    }
    if(!std::isfinite(worst)) return fail(h, PE_HIP_ERR_INACCURATE, "analyze_ac: the backward error of the refined solution is not finite");
    A.x.resize(A.d_xacc.len);
    HIPCHK(h, hipMemcpyAsync(A.x.data(), A.d_xacc.p, A.d_xacc.len * sizeof(double), hipMemcpyDeviceToHost, es));
    HIPCHK(h, hipStreamSynchronize(es));
    return PE_HIP_OK;
}

/* complex solution of the last pe_hip_analyze_ac: re / im [count][rows] (node voltage and branch current phasors) */
int pe_hip_get_solution_ac(pe_hip_engine* h, int first, int count, double* re, double* im)
{
    if(!h || !h->loaded || !h->ac.built || !re || !im || first < 0 || count < 0 || first + count > h->hc.batch) return PE_HIP_ERR_ARG;
    int const N = h->hc.rows;
    if(h->ac.x.size() != static_cast<size_t>(h->hc.batch) * 2 * N) return fail(h, PE_HIP_ERR_ARG, "get_solution_ac: no AC solution yet");
    for(int b = 0; b < count; ++b)
    {
        double const* x2 = &h->ac.x[static_cast<size_t>(first + b) * 2 * N];
        std::memcpy(re + static_cast<size_t>(b) * N, x2, N * sizeof(double));
        std::memcpy(im + static_cast<size_t>(b) * N, x2 + N, N * sizeof(double));
    }
    return PE_HIP_OK;
}

int pe_hip_set_ac_sweep_rows(pe_hip_engine* h, int n_rows, const int* rows)
{
    if(!h) return PE_HIP_ERR_ARG;
    int const rc = h->ac.sweep.kept.set(h, "set_ac_sweep_rows", n_rows, rows);
    if(rc == PE_HIP_OK) h->ac.sweep.valid = false;  // (the stored result has the layout of the rows it was made with)
    return rc;
}

}  // extern "C"

namespace
{
    bool numerical(int rc) { return rc == PE_HIP_ERR_SINGULAR || rc == PE_HIP_ERR_INACCURATE || rc == PE_HIP_ERR_NO_CONVERGENCE; }

    // Where point i of a sweep lives: doubles [i * per_point, (i + 1) * per_point) of the device array `dev`, and of the host result from
    // offset `host` on.  check: a value that is not finite fails the point.  collect: copied back after the passes (and again after a retry
    // of the point alone) -- the network analysis' converted planes are not: their caller fills them later.
    struct ResultBlock
    {
        double const* dev;
        size_t host, per_point;
        bool check, collect;
    };

    // What the forward sweep and the noise call do differently around the shared body below.
    struct SweepHooks
    {
        std::string name;                                       // prefix of the error messages
        std::function<int(int P)> prepare;                      // the batched engine stands with P points per pass: result buffers on the device (blocks[k].dev)
        std::function<int(pe_hip_engine* E)> epilogue;          // end of a pass, after refinement: gather the kept rows / accumulate the noise
        std::vector<double>* res = nullptr;                     // the host result and its layout: the body copies it back after the passes, fails the
        std::vector<ResultBlock> blocks;                        // points that are not finite, reads a retried point again, blanks a failed one
        std::function<int(int i)> single;                       // forward sweep: failed point i on the single-point path (sets its status)
        std::function<int(pe_hip_engine* E)> after_fill;        // sensitivity only (else empty): the value vectors of a pass stand -- its own right-hand sides
        char const* pass_knob = "AC_SWEEP_POINTS";              // the knob that sets the points per pass
        // network analysis only: n_rhs right-hand sides per pass on ONE factorisation -- the first as everywhere, then next_rhs(E, j) writes
        // the j-th and it is solved with the factors kept; every correction solve keeps them too; the epilogue runs once per right-hand side
        int n_rhs = 1;
        bool keep_factors = false;
        std::function<int(pe_hip_engine* E, int j)> next_rhs;
        int* n_factorisations = nullptr;                        // (counted from the engine's n_factor_launches)
        int* n_solves = nullptr;                                // kept-factor solves
        // pole-zero analysis only: the statuses the engine's instances carried in the last pass (it reports per instance, not per point)
        std::vector<int>* inst_status = nullptr;
    };

    // point i of the host result: every checked value finite / every block NaN
    bool point_finite(SweepHooks const& K, int i)
    {
        for(auto const& blk: K.blocks)
            for(size_t k = 0; blk.check && k < blk.per_point; ++k)
                if(!std::isfinite((*K.res)[blk.host + i * blk.per_point + k])) return false;
        return true;
    }
    void point_blank(SweepHooks const& K, int i)
    {
        for(auto const& blk: K.blocks) std::fill_n(K.res->begin() + blk.host + i * blk.per_point, blk.per_point, std::nan(""));
    }
    // device -> host of the collected blocks: points [first, first + n)
    int points_read(pe_hip_engine* h, SweepHooks const& K, int first, int n)
    {
        for(auto const& blk: K.blocks)
        {
            size_t const o = first * blk.per_point, len = n * blk.per_point;
            if(blk.collect && len > 0) HIPCHK(h, hipMemcpy(K.res->data() + blk.host + o, blk.dev + o, len * sizeof(double), hipMemcpyDeviceToHost));
        }
        return PE_HIP_OK;
    }

    // The body of a frequency sweep on the real-equivalent system A (forward: h->ac, adjoint: h->noise.sys): base vectors, bands,
    // representative values, pass size, the batched engine, the passes with their refinement, and the bookkeeping of the points that
    // failed in their batch.  pst: status per point (all PE_HIP_OK on entry).  S.n_fallback_points counts the failed points handled at the
    // end, by K.single or by a retry pass.
    int sweep_body(pe_hip_engine* h, pe_hip_engine::Ac& A, int n_points, double const* omegas, std::vector<int>& pst, pe_hip_ac_sweep_stats& S,
                   SweepHooks const& K)
    {
        auto& hc = h->hc;
        auto& W = A.sweep;
        int const B = hc.batch, N = hc.rows;
        auto const& ah = A.circ.hc;
        int const rhs0 = A.rhs0;
        if(rhs0 < pe::DV_FIXED + static_cast<int>(A.circ.slots.size())) return fail(h, PE_HIP_ERR_INTERNAL, K.name + ": value vector shorter than its slots");

        // ---- one base vector per circuit instance (the values at omega = 1) + how every value follows omega: uploaded once per sweep
        std::vector<double> base(static_cast<size_t>(B) * rhs0, 0.0);
        std::vector<int> scale(static_cast<size_t>(rhs0), pe::AC_CONST);
        {
            pe::AcOperatingPoint op;
            if(int const rc = read_operating_point(h, op); rc != PE_HIP_OK) return rc;
            std::vector<double> one(static_cast<size_t>(ah.dv_len), 0.0);
            for(int b = 0; b < B; ++b)
            {
                pe::fill_ac_values(hc, A.circ, op, b, 1.0, h->opt.g_min, r_open_of(h), one.data());
                std::copy(one.begin(), one.begin() + rhs0, base.begin() + static_cast<size_t>(b) * rhs0);
            }
            for(size_t i = 0; i < A.circ.slots.size(); ++i)
                switch(A.circ.slots[i].kind)
                {
                    case pe::AcSlot::C_W:
                    case pe::AcSlot::KL_W11:
                    case pe::AcSlot::KL_W12:
                    case pe::AcSlot::KL_W22: scale[pe::DV_FIXED + i] = pe::AC_OMEGA; break;
                    case pe::AcSlot::L_W:
                    case pe::AcSlot::D_WC: scale[pe::DV_FIXED + i] = pe::AC_OMEGA_ZERO; break;
                    default: break;
                }
        }
        if(!W.V.base)
        {
            double* d_base{};
            int* d_scale{};
            HIPCHK(h, W.circ_pool.alloc(d_base, base.size(), false));
            HIPCHK(h, W.circ_pool.alloc(d_scale, scale.size(), false));
            HIPCHK(h, W.circ_pool.upload(W.V.b_ptr0, A.b_ptr0));
            HIPCHK(h, W.circ_pool.upload(W.V.b_src0, A.b_src0));
            W.V.scale = d_scale;
            W.V.base = d_base;
            W.V.rhs0 = rhs0;
            W.V.n_inst = B;
            W.V.n_half = N;
        }
        HIPCHK(h, hipMemcpy(const_cast<double*>(W.V.base), base.data(), base.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(const_cast<int*>(W.V.scale), scale.data(), scale.size() * sizeof(int), hipMemcpyHostToDevice));

        // ---- frequency bands: the static pivot order is matched on representative values at one frequency and holds for a decade above it
        // (the rule of pe_hip_analyze_ac).  Points ascending; omega == 0 a band of its own; a band starts at its first omega w0 and takes every
        // point with omega <= 10 w0.
        std::vector<int> order(static_cast<size_t>(n_points));
        for(int i = 0; i < n_points; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return omegas[a] < omegas[b]; });
        std::vector<std::pair<int, int>> bands;  // [first, last) in `order`
        for(int i = 0; i < n_points;)
        {
            double const w0 = omegas[order[i]];
            int j = i + 1;
            while(j < n_points && (w0 == 0.0 ? omegas[order[j]] == 0.0 : omegas[order[j]] <= 10.0 * w0)) ++j;
            bands.emplace_back(i, j);
            i = j;
        }
        int largest_band = 0;
        for(auto const& bd: bands) largest_band = std::max(largest_band, bd.second - bd.first);

        // instance 0's matrix values at omega: what a band's symbolic analysis is matched on (analyse_here of the single-point path)
        auto representative = [&](double omega, std::vector<double>& out)
        {
            int const nnz = static_cast<int>(ah.ci.size());
            out.assign(static_cast<size_t>(nnz), 0.0);
            for(int s = 0; s < nnz; ++s)
            {
                double acc = 0.0;
                for(int e = ah.a_ptr[s]; e < ah.a_ptr[s + 1]; ++e)
                {
                    int const i = ah.a_src[e] >> 1;
                    double const v = pe::ac_sweep_value(base[i], scale[i], omega);
                    acc = (ah.a_src[e] & 1) ? acc - v : acc + v;
                }
                out[s] = acc;
            }
            ac_mask_contacts_closed_elsewhere(hc, A.circ, base.data(), static_cast<size_t>(rhs0), out);
        };

        // ---- points per pass: the knob, else what fits the memory budget; never more than the largest band needs
        int const knob_p = knob(h, K.pass_knob, 0);
        if(knob_p <= 0 && W.bytes_per_instance == 0)
        {
            // bytes of one instance of the AC system incl. its factor storage, from the single-point engine.  When that has no symbolic
            // analysis yet one is made on a band's values and forgotten again: pe_hip_analyze_ac then analyses as it always did.  A band
            // whose values cannot be analysed (a singular system at its omega) says nothing about the others: the next band is tried, and
            // when none can be analysed the sweep runs one point per pass -- its bands then fail one by one into the single-point path.
            bool const had = A.eng->resident.sym_class >= 0;
            int src = had ? PE_HIP_OK : PE_HIP_ERR_SINGULAR;
            for(size_t k = 0; !had && k < bands.size() && src != PE_HIP_OK; ++k)
            {
                representative(omegas[order[bands[k].first]], A.eng->sym_values_override);
                A.eng->resident.sym_class = -1;
                src = ensure_symbolic(A.eng.get(), false, 0.0);
                if(src != PE_HIP_OK && !numerical(src))
                {
                    A.eng->resident.sym_class = -1;
                    A.sym_omega = -1.0;
                    return fail(h, src, K.name + " (sizing): " + A.eng->err);
                }
            }
            pe_hip_info info{};
            int const rc = src == PE_HIP_OK ? pe_hip_get_info(A.eng.get(), &info) : PE_HIP_OK;
            if(!had)
            {
                A.eng->resident.sym_class = -1;
                A.sym_omega = -1.0;
            }
            if(rc != PE_HIP_OK) return fail(h, rc, K.name + " (sizing): " + A.eng->err);
            if(src == PE_HIP_OK) W.bytes_per_instance = std::max<long long>(1, info.bytes_per_instance);
        }
        long long const cap = sweep_pass_cap(knob_p, W.bytes_per_instance, B);
        int const P = static_cast<int>(std::min<long long>(cap, largest_band));
        if(!W.eng || W.P != P)
            if(int const rc = sweep_engine_build(h, A, P, K.name, K.keep_factors); rc != PE_HIP_OK) return rc;
        S.points_per_pass = 0;

        // ---- result buffers on the device
        if(int const rc = K.prepare(P); rc != PE_HIP_OK) return rc;

        pe_hip_engine* const E = W.eng.get();
        hipStream_t const es = E->stream;
        int const Q = B * P;
        std::vector<char> failed(static_cast<size_t>(n_points), 0);
        std::vector<int> inst_status(static_cast<size_t>(Q)), now(static_cast<size_t>(Q));
        std::vector<double> omega_h(static_cast<size_t>(P)), worst_h;
        std::vector<int> point_h(static_cast<size_t>(P));
        // one batched factor + solve of all Q instances from the device's value vectors; a numerical failure of some instances is theirs alone
        // (kept: with the factors of the pass's first solve -- the network analysis' further right-hand sides and its corrections)
        auto solve = [&](bool kept = false) -> int
        {
            HIPCHK(h, hipMemset(E->V.status, 0, static_cast<size_t>(Q) * sizeof(int)));
            long long const f0 = E->n_factor_launches, r0 = E->resident.n_rematched;
            int rc = kept ? dc_solve_kept(E, PE_HIP_MODE_DC, nullptr) : pe_hip_analyze_dc(E, PE_HIP_MODE_DC, nullptr);
            if(K.keep_factors && !kept && E->resident.n_rematched != r0 && (rc == PE_HIP_OK || numerical(rc)))
            {
                // the safety net re-matched the pivot order inside the factoring solve: only the instances it retried hold factors of the new
                // order, and the solves that follow keep them -- every instance factors again under it (as dc_solve_kept does for its own)
                HIPCHK(h, hipMemset(E->V.status, 0, static_cast<size_t>(Q) * sizeof(int)));
                rc = pe_hip_analyze_dc(E, PE_HIP_MODE_DC, nullptr);
            }
            if(K.n_factorisations) *K.n_factorisations += static_cast<int>(E->n_factor_launches - f0);
            if(kept && K.n_solves) ++*K.n_solves;
            if(rc != PE_HIP_OK && !numerical(rc)) return fail(h, rc, K.name + ": " + E->err);
            if(rc != PE_HIP_OK)
            {
                // (a status that no instance carries was raised before anything was launched: nothing of this solve is usable)
                HIPCHK(h, hipMemcpy(now.data(), E->V.status, static_cast<size_t>(Q) * sizeof(int), hipMemcpyDeviceToHost));
                bool const none = std::all_of(now.begin(), now.end(), [](int s) { return s == 0; });
                for(int q = 0; q < Q; ++q)
                    if(inst_status[q] == 0) inst_status[q] = none ? rc : now[q];
            }
            return PE_HIP_OK;
        };
        // one pass: the n <= P points pts[0 .. n) (the caller's indices) as instances of the engine, under its current symbolic analysis
        auto run_pass = [&](int const* pts, int n) -> int
        {
            for(int p = 0; p < P; ++p)
            {
                point_h[p] = p < n ? pts[p] : -1;
                omega_h[p] = omegas[pts[std::min(p, n - 1)]];
            }
            ++S.n_passes;
            S.points_per_pass = std::max(S.points_per_pass, n);
            HIPCHK(h, hipMemcpy(const_cast<double*>(W.V.omega), omega_h.data(), static_cast<size_t>(P) * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(const_cast<int*>(W.V.point), point_h.data(), static_cast<size_t>(P) * sizeof(int), hipMemcpyHostToDevice));
            std::fill(inst_status.begin(), inst_status.end(), 0);
            HIPCHK(h, hipEventRecord(h->ev0, es));
            W.b0_valid = false;
            HIPCHK(h, pe::launch_ac_sweep_fill(es, E->V, W.V));
            if(K.after_fill)
                if(int const rc = K.after_fill(E); rc != PE_HIP_OK) return rc;
            bool const keep = K.keep_factors;  // (the network analysis: one factorisation per pass)
            int last_above = 0;
            // the rounds ran out with instances still above the threshold: fine when their error is merely not at rounding level yet (the
            // single-point path stops there too), a failure when it is not a number
            auto check_above = [&]() -> int
            {
                if(last_above == 0) return PE_HIP_OK;
                HIPCHK(h, hipStreamSynchronize(es));
                worst_h.resize(static_cast<size_t>(Q));
                HIPCHK(h, hipMemcpy(worst_h.data(), W.V.worst, static_cast<size_t>(Q) * sizeof(double), hipMemcpyDeviceToHost));
                for(int q = 0; q < Q; ++q)
                    if(!std::isfinite(worst_h[q]) && inst_status[q] == 0) inst_status[q] = PE_HIP_ERR_INACCURATE;
                return PE_HIP_OK;
            };
            for(int j = 0; j < K.n_rhs; ++j)
            {
                if(j > 0)
                {
                    W.b0_valid = false;
                    if(int const rc = K.next_rhs(E, j); rc != PE_HIP_OK) return rc;
                }
                if(int const rc = solve(j > 0); rc != PE_HIP_OK) return rc;
                HIPCHK(h, pe::launch_ac_accumulate_each(es, E->V, W.V, true));
                W.b0_valid = true;
                // refinement as in pe_hip_analyze_ac (same threshold, at most three rounds, then one closing residual evaluation of the iterate
                // the third correction produced), decided per instance: the host reads one int per round
                int above = 0;
                for(int round = 0;; ++round)
                {
                    HIPCHK(h, pe::launch_ac_residual_each(es, E->V, W.V));
                    HIPCHK(h, hipMemcpyAsync(&above, W.V.n_above, sizeof(int), hipMemcpyDeviceToHost, es));
                    HIPCHK(h, hipStreamSynchronize(es));
                    if(above == 0 || round == 3) break;
                    if(int const rc = solve(keep); rc != PE_HIP_OK) return rc;
                    HIPCHK(h, pe::launch_ac_accumulate_each(es, E->V, W.V, false));
                    ++S.n_refine_rounds;
                }
                if(int const rc = K.epilogue(E); rc != PE_HIP_OK) return rc;
                last_above = above;
                if(j + 1 < K.n_rhs)  // (the next right-hand side overwrites the errors of this one)
                    if(int const rc = check_above(); rc != PE_HIP_OK) return rc;
            }
            HIPCHK(h, hipEventRecord(h->ev1, es));
            HIPCHK(h, hipStreamSynchronize(es));
            float ms = 0.f;
            HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
            S.gpu_ms += ms;
            if(int const rc = check_above(); rc != PE_HIP_OK) return rc;
            if(K.inst_status) *K.inst_status = inst_status;
            for(int p = 0; p < n; ++p)
                for(int b = 0; b < B; ++b)
                    if(inst_status[static_cast<size_t>(b) * P + p] != 0) failed[point_h[p]] = 1;
            return PE_HIP_OK;
        };
        for(auto const& bd: bands)
        {
            // the band's symbolic analysis, on the host, before its passes (so that gpu_ms is theirs alone).  Values that cannot be analysed
            // (a structurally or numerically singular system at w0, e.g. a node held by capacitors only at omega = 0) fail the BAND, not the
            // sweep: nothing is launched for it and each of its points goes to the single-point path, which reports that point's own status.
            representative(omegas[order[bd.first]], E->sym_values_override);
            E->resident.sym_class = -1;
            ++S.n_analyses;
            if(int const rc = ensure_symbolic(E, false, 0.0); rc != PE_HIP_OK)
            {
                if(!numerical(rc)) return fail(h, rc, K.name + ": " + E->err);
                for(int k = bd.first; k < bd.second; ++k) failed[order[k]] = 1;
                continue;
            }
            for(int first = bd.first; first < bd.second; first += P)
                if(int const rc = run_pass(&order[first], std::min(P, bd.second - first)); rc != PE_HIP_OK) return rc;
        }
        // ---- one copy of the results of every point, then the points that failed in their batch: the single-point path (forward sweep), or
        // alone in one pass of one point under an analysis on that point's own values (noise)
        if(int const rc = points_read(h, K, 0, n_points); rc != PE_HIP_OK) return rc;
        for(int i = 0; i < n_points; ++i)
            if(!failed[i] && !point_finite(K, i)) failed[i] = 1;
        for(int i = 0; i < n_points; ++i)
        {
            if(!failed[i]) continue;
            ++S.n_fallback_points;
            if(K.single)
            {
                if(int const rc = K.single(i); rc != PE_HIP_OK) return rc;
                continue;
            }
            representative(omegas[i], E->sym_values_override);
            E->resident.sym_class = -1;
            ++S.n_analyses;
            if(int const rc = ensure_symbolic(E, false, 0.0); rc != PE_HIP_OK)
            {
                if(!numerical(rc)) return fail(h, rc, K.name + ": " + E->err);
                pst[i] = rc;
                continue;
            }
            failed[i] = 0;
            if(int const rc = run_pass(&i, 1); rc != PE_HIP_OK) return rc;
            for(int b = 0; b < B && pst[i] == PE_HIP_OK; ++b) pst[i] = inst_status[static_cast<size_t>(b) * P];
            if(int const rc = points_read(h, K, i, 1); rc != PE_HIP_OK) return rc;
            if(pst[i] == PE_HIP_OK && !point_finite(K, i)) pst[i] = PE_HIP_ERR_INACCURATE;
        }
        // a failed point reads NaN
        for(int i = 0; i < n_points; ++i)
            if(pst[i] != PE_HIP_OK) point_blank(K, i);
        return PE_HIP_OK;
    }
}  // namespace

extern "C" {

/* A whole frequency sweep as batches of the real-equivalent system: the points of a pass are extra instances of a third engine
 * (h->ac.sweep.eng), the value vectors are made on the device from one base vector per circuit instance (k_ac_sweep_fill), refinement runs
 * per instance, the kept rows are gathered on the device and copied back once.  Bands, passes and the fallback: include/pe_hip.h. */
int pe_hip_analyze_ac_sweep(pe_hip_engine* h, int n_points, const double* omegas, int* point_status, pe_hip_ac_sweep_stats* stats)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    if(stats) std::memset(stats, 0, sizeof(*stats));
    if(n_points < 1 || !omegas) return fail(h, PE_HIP_ERR_ARG, "analyze_ac_sweep: n_points < 1 or no omegas");
    for(int i = 0; i < n_points; ++i)
        if(!std::isfinite(omegas[i]) || omegas[i] < 0.0) return fail(h, PE_HIP_ERR_ARG, "analyze_ac_sweep: negative or non-finite omega");
    HIPCHK(h, hipSetDevice(h->device));
    auto& hc = h->hc;
    auto& A = h->ac;
    auto& W = A.sweep;
    W.valid = false;
    int const B = hc.batch, N = hc.rows;
    int const K = W.kept.rows.empty() ? N : static_cast<int>(W.kept.rows.size());
    pe_hip_ac_sweep_stats S{};
    S.n_points = n_points;
    std::vector<int> pst(static_cast<size_t>(n_points), PE_HIP_OK);
    size_t const plane = static_cast<size_t>(n_points) * B * K;  // doubles of the real (and of the imaginary) parts
    W.res.assign(2 * plane, std::nan(""));
    auto finish = [&]() -> int
    {
        W.n_points = n_points;
        W.n_keep = K;
        W.batch = B;
        W.valid = true;
        if(point_status) std::copy(pst.begin(), pst.end(), point_status);
        if(stats) *stats = S;
        for(int i = 0; i < n_points; ++i)
            if(pst[i] != PE_HIP_OK) return fail(h, pst[i], "analyze_ac_sweep: point " + std::to_string(i) + ": " + h->err);
        return PE_HIP_OK;
    };
    if(N == 0) return finish();
    // the single-point path for point i (the fallback): pe_hip_analyze_ac analyses on that point's own values.  A numerical status is the
    // point's status; anything else (a HIP error) ends the call.
    auto single = [&](int i) -> int
    {
        int const rc = pe_hip_analyze_ac(h, omegas[i], nullptr);
        pst[i] = rc;
        double* re = &W.res[static_cast<size_t>(i) * B * K];
        double* im = re + plane;
        if(rc == PE_HIP_OK)
        {
            for(int b = 0; b < B; ++b)
                for(int k = 0; k < K; ++k)
                {
                    double const* x2 = &A.x[static_cast<size_t>(b) * 2 * N];
                    int const r = W.kept.rows.empty() ? k : W.kept.rows[k];
                    re[static_cast<size_t>(b) * K + k] = x2[r];
                    im[static_cast<size_t>(b) * K + k] = x2[N + r];
                }
            return PE_HIP_OK;
        }
        std::fill(re, re + static_cast<size_t>(B) * K, std::nan(""));
        std::fill(im, im + static_cast<size_t>(B) * K, std::nan(""));
        return numerical(rc) ? PE_HIP_OK : rc;
    };
    if(has_overlay(h))
    {
        // host-stamped models: their values come from callbacks per omega -- every point takes the single-point path
        for(int i = 0; i < n_points; ++i)
        {
            ++S.n_fallback_points;
            if(int const rc = single(i); rc != PE_HIP_OK) return rc;
        }
        return finish();
    }
    if(int const brc = ensure_ac_built(h); brc != PE_HIP_OK) return brc;
    SweepHooks hooks;
    hooks.name = "analyze_ac_sweep";
    // result buffer and kept rows on the device
    hooks.res = &W.res;
    hooks.blocks = {{nullptr, 0, static_cast<size_t>(B) * K, true, true}, {nullptr, plane, static_cast<size_t>(B) * K, true, true}};
    hooks.prepare = [&](int) -> int
    {
        HIPCHK(h, W.d_re.ensure(plane, false));
        HIPCHK(h, W.d_im.ensure(plane, false));
        hooks.blocks[0].dev = W.V.res_re = W.d_re.p;
        hooks.blocks[1].dev = W.V.res_im = W.d_im.p;
        if(int const rc = W.kept.upload(h, W.V.keep); rc != PE_HIP_OK) return rc;
        W.V.n_keep = K;
        return PE_HIP_OK;
    };
    hooks.epilogue = [&](pe_hip_engine* E) -> int
    {
        HIPCHK(h, pe::launch_ac_sweep_gather(E->stream, E->V, W.V));
        return PE_HIP_OK;
    };
    hooks.single = single;
    if(int const rc = sweep_body(h, A, n_points, omegas, pst, S, hooks); rc != PE_HIP_OK) return rc;
    return finish();
}

int pe_hip_get_ac_sweep(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, double* re, double* im)
{
    if(!h || !h->loaded || !re || !im) return PE_HIP_ERR_ARG;
    auto const& W = h->ac.sweep;
    if(int const rc = stored_window(h, "get_ac_sweep", "AC sweep", "points", W.valid, W.batch, W.n_points, first_point, n_points, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    size_t const K = static_cast<size_t>(W.n_keep), plane = static_cast<size_t>(W.n_points) * W.batch * K;
    for(int i = 0; i < n_points; ++i)
    {
        size_t const src = (static_cast<size_t>(first_point + i) * W.batch + first_instance) * K, dst = static_cast<size_t>(i) * count * K;
        if(count * K == 0) continue;
        std::memcpy(re + dst, &W.res[src], static_cast<size_t>(count) * K * sizeof(double));
        std::memcpy(im + dst, &W.res[plane + src], static_cast<size_t>(count) * K * sizeof(double));
    }
    return PE_HIP_OK;
}

/* Read-back of a small-signal system (include/pe_hip.h): the inner engine's pe_hip_get_matrix for pattern and values, the refinement's copy
 * of the right-hand side as stamped for rhs.  Launches nothing. */
int pe_hip_get_matrix_ac(pe_hip_engine* h, int which, int instance, int nnz_capacity, int* row_ptr, int* col_ind, double* vals, double* rhs, int* n_rows,
                         int* nnz)
{
    if(!h || !h->loaded || which < 0 || which > 4 || nnz_capacity < 0) return PE_HIP_ERR_ARG;
    auto& A = which < 2 ? h->ac : which < 4 ? h->noise.sys : h->sens.sys;
    bool const batched = (which & 1) != 0 || which == 4;
    pe_hip_engine* const E = batched ? A.sweep.eng.get() : A.eng.get();
    if(!A.built || !E || !E->loaded) return fail(h, PE_HIP_ERR_ARG, "get_matrix_ac: that engine does not exist yet");
    int const R2 = E->hc.rows, nz = static_cast<int>(E->hc.ci.size());
    if(n_rows) *n_rows = R2;
    if(nnz) *nnz = nz;
    if(nnz_capacity == 0) return PE_HIP_OK;
    if(nnz_capacity < nz) return fail(h, PE_HIP_ERR_ARG, "get_matrix_ac: nnz_capacity below the system's nnz");
    if(instance < 0 || instance >= E->hc.batch) return fail(h, PE_HIP_ERR_ARG, "get_matrix_ac: instance out of range");
    if(int const rc = pe_hip_get_matrix(E, instance, row_ptr, col_ind, vals, nullptr); rc != PE_HIP_OK) return fail(h, rc, "get_matrix_ac: " + E->err);
    if(rhs)
    {
        double const* b0 = batched ? A.sweep.V.b0 : A.d_b0.p;
        bool const valid = batched ? A.sweep.b0_valid : (A.b0_valid && A.d_xacc.len == static_cast<size_t>(E->hc.batch) * R2);
        if(!b0 || !valid) return fail(h, PE_HIP_ERR_ARG, "get_matrix_ac: no right-hand side has been stamped on that engine (its last solve failed, or none ran)");
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemcpy(rhs, b0 + static_cast<size_t>(instance) * R2, static_cast<size_t>(R2) * sizeof(double), hipMemcpyDeviceToHost));
    }
    return PE_HIP_OK;
}

int pe_hip_get_ac_analysis_omega(pe_hip_engine* h, double* omega)
{
    if(!h || !h->loaded || !omega) return PE_HIP_ERR_ARG;
    if(!h->ac.built) return fail(h, PE_HIP_ERR_ARG, "get_ac_analysis_omega: that engine does not exist yet");
    *omega = h->ac.sym_omega;
    return PE_HIP_OK;
}

int pe_hip_get_ac_pass_size(pe_hip_engine* h, int which, int* points_per_pass)
{
    if(!h || !h->loaded || !points_per_pass || (which != 1 && which != 3)) return PE_HIP_ERR_ARG;
    auto const& W = (which == 1 ? h->ac : h->noise.sys).sweep;
    if(!W.eng) return fail(h, PE_HIP_ERR_ARG, "get_ac_pass_size: that engine does not exist yet");
    *points_per_pass = W.P;
    return PE_HIP_OK;
}

}  // extern "C"

namespace
{
    static_assert(pe::NOISE_KIND_BJT_NPN == PE_HIP_BJT_NPN, "pe_noise.hpp names the kind without including the C header");

    // the source table of the resident circuit, in the definition order of include/pe_hip.h (host only)
    void noise_table_build(pe_hip_engine* h)
    {
        auto& Z = h->noise;
        if(Z.table_built) return;
        auto const& hc = h->hc;
        Z.src.clear();
        Z.kind.clear();
        Z.index.clear();
        Z.part.clear();
        auto add = [&](int type, int idx, int a, int b, int kind, int index, int part)
        {
            Z.src.push_back({type, idx, a, b});
            Z.kind.push_back(kind);
            Z.index.push_back(index);
            Z.part.push_back(part);
        };
        for(size_t i = 0; i < hc.map_r.size(); ++i)
        {
            int const c = hc.map_r[i];
            if(c < 0) add(pe::NOISE_NONE, 0, -1, -1, PE_HIP_R, static_cast<int>(i), 0);
            else
                add(pe::NOISE_R, c, hc.r_a[c], hc.r_b[c], PE_HIP_R, static_cast<int>(i), 0);
        }
        for(size_t i = 0; i < hc.map_d.size(); ++i)
        {
            int const c = hc.map_d[i];
            if(c < 0) add(pe::NOISE_NONE, 0, -1, -1, PE_HIP_DIODE, static_cast<int>(i), 0);
            else
                add(pe::NOISE_DIODE, c, hc.d_a[c], hc.d_c[c], PE_HIP_DIODE, static_cast<int>(i), 0);
        }
        // the three-pin tables as the caller passed them, each in table order: the order n3 was filled in, with the devices that have an
        // unconnected pin (no n3 entry, no stamp) in their place as sources of density 0
        for(int const kind : hc.n3_tables)
        {
            bool const mos = kind == PE_HIP_NMOS || kind == PE_HIP_PMOS;
            auto const& map = hc.map_gen[static_cast<size_t>(kind)];
            for(size_t p = 0; p < map.size(); ++p)
            {
                int const index = static_cast<int>(p);
                if(map[p] < 0)
                {
                    add(pe::NOISE_NONE, 0, -1, -1, kind, index, 0);
                    if(!mos) add(pe::NOISE_NONE, 0, -1, -1, kind, index, 1);
                    continue;
                }
                int const j = hc.gen[static_cast<size_t>(map[p])].aux;
                int const* n = &hc.n3_n[3 * static_cast<size_t>(j)];
                if(mos) add(pe::NOISE_MOS, j, n[0], n[2], kind, index, 0);  // D - S
                else
                {
                    add(pe::NOISE_BJT_B, j, n[0], n[2], kind, index, 0);  // B - E
                    add(pe::NOISE_BJT_C, j, n[1], n[2], kind, index, 1);  // C - E
                }
            }
        }
        Z.table_built = true;
        Z.table_on_device = false;
    }

    // The right-hand side of system A becomes the selector of the pair (pos, neg): its lists as build_ac_circuit makes them for an output
    // pair (a new pair changes only these), and what the sweep engine holds of the old ones dropped -- base vectors, scale flags and the
    // lists are uploaded again by the sweep body.
    void select_rhs(pe_hip_engine::Ac& A, int pos, int neg)
    {
        int const rows2 = A.circ.hc.rows;
        A.b_ptr0.assign(static_cast<size_t>(rows2) + 1, 0);
        A.b_src0.clear();
        for(int r = 0; r < rows2; ++r)
        {
            if(r == pos) A.b_src0.push_back((pe::DV_ONE << 1) | 0);
            if(r == neg) A.b_src0.push_back((pe::DV_ONE << 1) | 1);
            A.b_ptr0[static_cast<size_t>(r) + 1] = static_cast<int>(A.b_src0.size());
        }
        auto& W = A.sweep;
        W.circ_pool.release();
        W.V.base = nullptr;
        W.V.scale = nullptr;
        W.V.b_ptr0 = W.V.b_src0 = nullptr;
    }
}  // namespace

extern "C" {

/* Output noise density by the adjoint method: one solve of the transposed small-signal system per frequency point -- the sweep body of
 * pe_hip_analyze_ac_sweep on the adjoint system with state of its own (h->noise) --, the sources' densities from the resident operating
 * point (k_noise_sources), their reduction per (instance, point) on the device (k_noise_accumulate).  Definitions: include/pe_hip.h. */
int pe_hip_analyze_noise(pe_hip_engine* h, int n_points, const double* omegas, const pe_hip_noise_control* ctl, int* point_status, pe_hip_noise_stats* stats)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    if(stats) std::memset(stats, 0, sizeof(*stats));
    if(n_points < 1 || !omegas || !ctl) return fail(h, PE_HIP_ERR_ARG, "analyze_noise: n_points < 1, no omegas or no control");
    for(int i = 0; i < n_points; ++i)
        if(!std::isfinite(omegas[i]) || omegas[i] < 0.0) return fail(h, PE_HIP_ERR_ARG, "analyze_noise: negative or non-finite omega");
    auto& hc = h->hc;
    int const B = hc.batch, N = hc.rows;
    int const out_pos = ctl->out_pos, out_neg = ctl->out_neg;
    if(out_pos < -1 || out_pos >= N || out_neg < -1 || out_neg >= N) return fail(h, PE_HIP_ERR_ARG, "analyze_noise: output row out of range");
    if(out_pos == out_neg) return fail(h, PE_HIP_ERR_ARG, "analyze_noise: the output needs two different rows (-1: ground)");
    if(has_overlay(h)) return fail(h, PE_HIP_ERR_ARG, "analyze_noise: host-stamped overlay models have no noise description");
    HIPCHK(h, hipSetDevice(h->device));
    auto& Z = h->noise;
    auto& A = Z.sys;
    auto& W = A.sweep;
    Z.valid = false;
    bool const keep = ctl->keep_contributions != 0;

    // an instance whose last analysis failed has no operating point to linearise at: the call carries that status instead of numbers
    int bad = -1, bad_status = PE_HIP_OK;
    if(int const rc = operating_point_status(h, bad, bad_status); rc != PE_HIP_OK) return rc;
    if(bad >= 0)
    {
        noise_table_build(h);
        Z.res.assign(static_cast<size_t>(n_points) * B * (1 + (keep ? Z.src.size() : 0)), std::nan(""));
        Z.integrated.assign(static_cast<size_t>(B), std::nan(""));
        Z.n_points = n_points;
        Z.batch = B;
        Z.kept = keep;
        Z.have_density = false;  // (k_noise_sources has not run: the density getter reads NaN like the points)
        Z.valid = true;
        if(point_status) std::fill(point_status, point_status + n_points, bad_status);
        if(stats)
        {
            stats->n_points = n_points;
            stats->n_sources = static_cast<int>(Z.src.size());
        }
        return fail(h, bad_status, "analyze_noise: instance " + std::to_string(bad) + " has no operating point (its last analysis failed)");
    }

    // ---- the adjoint system for this output pair
    pe::AcAdjoint const adj{out_pos, out_neg};
    if(!A.built)
    {
        if(int const rc = ensure_ac_built(h, A, &adj); rc != PE_HIP_OK) return rc;
    }
    else if(!Z.have_pair || Z.out_pos != out_pos || Z.out_neg != out_neg)
        select_rhs(A, out_pos, out_neg);
    Z.have_pair = true;
    Z.out_pos = out_pos;
    Z.out_neg = out_neg;

    // ---- the sources: table once per circuit, densities once per call from the resident operating point
    noise_table_build(h);
    int const n_src = static_cast<int>(Z.src.size());
    if(!Z.table_on_device)
    {
        Z.src_pool.release();
        HIPCHK(h, Z.src_pool.upload(Z.V.src, Z.src));
        HIPCHK(h, Z.src_pool.alloc(Z.V.rows, static_cast<size_t>(n_src)));
        HIPCHK(h, Z.src_pool.alloc(Z.V.S, static_cast<size_t>(B) * n_src));
        Z.table_on_device = true;
    }
    Z.V.n_src = n_src;
    Z.V.n_chunks = std::max(1, (n_src + pe::NOISE_CHUNK - 1) / pe::NOISE_CHUNK);
    Z.V.n_inst = B;
    Z.V.n_half = N;
    Z.V.temp_k = ctl->temp_k > 0.0 ? ctl->temp_k : pe::NOISE_TEMP_DEFAULT;
    HIPCHK(h, pe::launch_noise_sources(h->stream, h->V, Z.V));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (the passes run on the adjoint engine's stream)

    // ---- result: densities, then the contributions when they are kept; one buffer, one copy back
    size_t const n_psd = static_cast<size_t>(n_points) * B;
    size_t const total = n_psd + (keep ? n_psd * static_cast<size_t>(n_src) : 0);
    Z.res.assign(total, std::nan(""));
    Z.integrated.assign(static_cast<size_t>(B), std::nan(""));
    pe_hip_ac_sweep_stats S{};
    S.n_points = n_points;
    std::vector<int> pst(static_cast<size_t>(n_points), PE_HIP_OK);

    SweepHooks hooks;
    hooks.name = "analyze_noise";
    // (a point is its row of densities -- what is not finite there fails it -- and, when they are kept, its block of contributions)
    hooks.res = &Z.res;
    hooks.blocks = {{nullptr, 0, static_cast<size_t>(B), true, true}};
    if(keep) hooks.blocks.push_back({nullptr, n_psd, static_cast<size_t>(B) * n_src, false, true});
    hooks.prepare = [&](int P) -> int
    {
        HIPCHK(h, Z.d_res.ensure(total, false));
        HIPCHK(h, Z.d_res.fill_nan());
        HIPCHK(h, Z.partial.ensure(static_cast<size_t>(B) * P * Z.V.n_chunks));
        Z.V.partial = Z.partial.p;
        Z.V.P = P;
        Z.V.xacc = W.V.xacc;
        Z.V.point = W.V.point;
        hooks.blocks[0].dev = Z.V.psd = Z.d_res.p;
        Z.V.contrib = keep ? Z.d_res.p + n_psd : nullptr;
        if(keep) hooks.blocks[1].dev = Z.V.contrib;
        return PE_HIP_OK;
    };
    hooks.epilogue = [&](pe_hip_engine* E) -> int
    {
        HIPCHK(h, pe::launch_noise_accumulate(E->stream, E->V, Z.V));
        return PE_HIP_OK;
    };
    if(int const rc = sweep_body(h, A, n_points, omegas, pst, S, hooks); rc != PE_HIP_OK) return rc;

    // ---- integrated noise: trapezoidal rule in linear f = omega / 2 pi over the distinct points, ascending, on the host in that fixed order
    {
        std::vector<int> order(static_cast<size_t>(n_points));
        for(int i = 0; i < n_points; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return omegas[a] < omegas[b]; });
        bool const any_failed = std::any_of(pst.begin(), pst.end(), [](int s) { return s != PE_HIP_OK; });
        constexpr double two_pi = 6.283185307179586476925286766559;
        for(int b = 0; b < B; ++b)
        {
            double acc = 0.0;
            int prev = order[0];
            for(int k = 1; k < n_points; ++k)
            {
                int const i = order[k];
                if(omegas[i] == omegas[prev]) continue;
                acc += (omegas[i] / two_pi - omegas[prev] / two_pi) * (Z.res[static_cast<size_t>(i) * B + b] + Z.res[static_cast<size_t>(prev) * B + b]) / 2.0;
                prev = i;
            }
            Z.integrated[static_cast<size_t>(b)] = any_failed ? std::nan("") : acc;
        }
    }
    Z.n_points = n_points;
    Z.batch = B;
    Z.kept = keep;
    Z.have_density = true;
    Z.valid = true;
    if(point_status) std::copy(pst.begin(), pst.end(), point_status);
    if(stats)
    {
        stats->n_points = n_points;
        stats->n_sources = n_src;
        stats->n_passes = S.n_passes;
        stats->points_per_pass = S.points_per_pass;
        stats->n_analyses = S.n_analyses;
        stats->n_refine_rounds = S.n_refine_rounds;
        stats->n_retried_points = S.n_fallback_points;
        stats->gpu_ms = S.gpu_ms;
    }
    for(int i = 0; i < n_points; ++i)
        if(pst[i] != PE_HIP_OK) return fail(h, pst[i], "analyze_noise: point " + std::to_string(i) + " failed");
    return PE_HIP_OK;
}

int pe_hip_get_noise(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, double* psd, double* contrib)
{
    if(!h || !h->loaded || !psd) return PE_HIP_ERR_ARG;
    auto const& Z = h->noise;
    if(int const rc = stored_window(h, "get_noise", "noise analysis", "points", Z.valid, Z.batch, Z.n_points, first_point, n_points, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    if(contrib && !Z.kept) return fail(h, PE_HIP_ERR_ARG, "get_noise: the contributions were not kept (pe_hip_noise_control.keep_contributions)");
    size_t const n_src = Z.src.size(), n_psd = static_cast<size_t>(Z.n_points) * Z.batch;
    for(int i = 0; i < n_points && count > 0; ++i)
    {
        size_t const src = static_cast<size_t>(first_point + i) * Z.batch + first_instance, dst = static_cast<size_t>(i) * count;
        std::memcpy(psd + dst, &Z.res[src], static_cast<size_t>(count) * sizeof(double));
        if(contrib && n_src > 0) std::memcpy(contrib + dst * n_src, &Z.res[n_psd + src * n_src], static_cast<size_t>(count) * n_src * sizeof(double));
    }
    return PE_HIP_OK;
}

int pe_hip_get_noise_sources(pe_hip_engine* h, int capacity, int* kind, int* index, int* part, int* row_a, int* row_b, int* n_sources)
{
    if(!h || !h->loaded || capacity < 0) return PE_HIP_ERR_ARG;
    noise_table_build(h);
    auto const& Z = h->noise;
    int const n = static_cast<int>(Z.src.size());
    if(n_sources) *n_sources = n;
    for(int k = 0; k < std::min(n, capacity); ++k)
    {
        if(kind) kind[k] = Z.kind[static_cast<size_t>(k)];
        if(index) index[k] = Z.index[static_cast<size_t>(k)];
        if(part) part[k] = Z.part[static_cast<size_t>(k)];
        if(row_a) row_a[k] = Z.src[static_cast<size_t>(k)].a;
        if(row_b) row_b[k] = Z.src[static_cast<size_t>(k)].b;
    }
    return PE_HIP_OK;
}

int pe_hip_get_noise_source_density(pe_hip_engine* h, int first_instance, int count, double* s)
{
    if(!h || !h->loaded || !s) return PE_HIP_ERR_ARG;
    auto const& Z = h->noise;
    if(int const rc = stored_window(h, "get_noise_source_density", "noise analysis", nullptr, Z.valid, Z.batch, 0, 0, 0, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    size_t const n_src = Z.src.size();
    if(!Z.have_density) std::fill(s, s + static_cast<size_t>(count) * n_src, std::nan(""));
    else if(count > 0 && n_src > 0)
    {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipMemcpy(s, Z.V.S + static_cast<size_t>(first_instance) * n_src, static_cast<size_t>(count) * n_src * sizeof(double), hipMemcpyDeviceToHost));
    }
    return PE_HIP_OK;
}

int pe_hip_get_noise_integrated(pe_hip_engine* h, int first_instance, int count, double* v2)
{
    if(!h || !h->loaded || !v2) return PE_HIP_ERR_ARG;
    auto const& Z = h->noise;
    if(int const rc = stored_window(h, "get_noise_integrated", "noise analysis", nullptr, Z.valid, Z.batch, 0, 0, 0, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    std::copy(Z.integrated.begin() + first_instance, Z.integrated.begin() + first_instance + count, v2);
    return PE_HIP_OK;
}

}  // extern "C"

namespace
{
    static_assert(pe::SENS_DIODE_NRAW == PE_HIP_DIODE_NPARAM && pe::SENS_KIND_NMOS == PE_HIP_NMOS && pe::SENS_KIND_BJT_NPN == PE_HIP_BJT_NPN,
                  "pe_sens.hpp names these without including the C header");

    // the parameter table of the resident circuit in the definition order of include/pe_hip.h, and the stamps of every value slot (host only)
    void sens_table_build(pe_hip_engine* h)
    {
        auto& Y = h->sens;
        if(Y.table_built) return;
        auto const& hc = h->hc;
        Y.par.clear();
        Y.kind.clear();
        Y.index.clear();
        Y.column.clear();
        auto add = [&](int type, int idx, int col, int aux, int kind, int index)
        {
            Y.par.push_back({type, idx, col, aux});
            Y.kind.push_back(kind);
            Y.index.push_back(index);
            Y.column.push_back(col);
        };
        auto two_pin = [&](std::vector<int> const& map, int kind, int type, int dv0)
        {
            for(size_t i = 0; i < map.size(); ++i)
            {
                if(map[i] < 0) add(pe::SENS_NONE, 0, 0, 0, kind, static_cast<int>(i));
                else
                    add(type, map[i], 0, dv0 + map[i], kind, static_cast<int>(i));
            }
        };
        two_pin(hc.map_r, PE_HIP_R, pe::SENS_R, hc.dv_r);
        two_pin(hc.map_vdc, PE_HIP_VDC, pe::SENS_UNIT, hc.dv_vdc);
        two_pin(hc.map_idc, PE_HIP_IDC, pe::SENS_UNIT, hc.dv_idc);
        static constexpr int diode_cols[] = {0, 1, 2, 3, 4, 5, 6, 8};
        for(size_t i = 0; i < hc.map_d.size(); ++i)
            for(int const col : diode_cols)
            {
                int const c = hc.map_d[i];
                if(c < 0) add(pe::SENS_NONE, 0, col, 0, PE_HIP_DIODE, static_cast<int>(i));
                else
                    add(pe::SENS_DIODE, c, col, hc.dv_di + c, PE_HIP_DIODE, static_cast<int>(i));
            }
        for(int const kind : hc.gen_tables)
        {
            bool const mos = kind == PE_HIP_NMOS || kind == PE_HIP_PMOS, bjt = kind == PE_HIP_BJT_NPN || kind == PE_HIP_BJT_PNP;
            bool const unit = kind == PE_HIP_VCCS || kind == PE_HIP_VCVS || kind == PE_HIP_CCCS || kind == PE_HIP_CCVS || kind == PE_HIP_OPAMP || kind == PE_HIP_XFMR;
            if(!mos && !bjt && !unit && kind != PE_HIP_XFMR_CT) continue;
            int const ncol = mos ? 3 : bjt ? 5 : 1;
            auto const& map = hc.map_gen[static_cast<size_t>(kind)];
            for(size_t p = 0; p < map.size(); ++p)
                for(int col = 0; col < ncol; ++col)
                {
                    int const index = static_cast<int>(p);
                    if(map[p] < 0)
                    {
                        add(pe::SENS_NONE, 0, col, 0, kind, index);
                        continue;
                    }
                    auto const& d = hc.gen[static_cast<size_t>(map[p])];
                    if(mos) add(pe::SENS_MOS, d.aux, col, 0, kind, index);
                    else if(bjt)
                        add(pe::SENS_BJT, d.aux, col, d.par, kind, index);
                    else
                        add(unit ? pe::SENS_UNIT : pe::SENS_XCT, 0, col, d.dv, kind, index);
                }
        }
        // the contribution lists by value slot, in list order: A entries (row of the CSR slot, its column), then right-hand-side entries
        std::vector<int> cnt(static_cast<size_t>(hc.dv_len) + 1, 0);
        for(int const e : hc.a_src) ++cnt[static_cast<size_t>(e >> 1) + 1];
        for(int const e : hc.b_src) ++cnt[static_cast<size_t>(e >> 1) + 1];
        for(int j = 0; j < hc.dv_len; ++j) cnt[static_cast<size_t>(j) + 1] += cnt[static_cast<size_t>(j)];
        Y.sl_ptr = cnt;
        Y.sl_ent.assign(static_cast<size_t>(cnt[static_cast<size_t>(hc.dv_len)]), pe::SensEnt{0, -1});
        std::vector<int> cur(cnt.begin(), cnt.end() - 1);
        for(int r = 0; r < hc.rows; ++r)
            for(int sl = hc.rp[r]; sl < hc.rp[r + 1]; ++sl)
                for(int e = hc.a_ptr[sl]; e < hc.a_ptr[sl + 1]; ++e) Y.sl_ent[static_cast<size_t>(cur[static_cast<size_t>(hc.a_src[e] >> 1)]++)] = {(r << 1) | (hc.a_src[e] & 1), hc.ci[sl]};
        for(int r = 0; r < hc.rows; ++r)
            for(int e = hc.b_ptr[r]; e < hc.b_ptr[r + 1]; ++e) Y.sl_ent[static_cast<size_t>(cur[static_cast<size_t>(hc.b_src[e] >> 1)]++)] = {(r << 1) | (hc.b_src[e] & 1), -1};
        Y.table_built = true;
        Y.table_on_device = false;
    }
}  // namespace

extern "C" {

int pe_hip_get_sens_params(pe_hip_engine* h, int capacity, int* kind, int* index, int* column, int* n_params)
{
    if(!h || !h->loaded || capacity < 0) return PE_HIP_ERR_ARG;
    sens_table_build(h);
    auto const& Y = h->sens;
    int const n = static_cast<int>(Y.par.size());
    if(n_params) *n_params = n;
    for(int k = 0; k < std::min(n, capacity); ++k)
    {
        if(kind) kind[k] = Y.kind[static_cast<size_t>(k)];
        if(index) index[k] = Y.index[static_cast<size_t>(k)];
        if(column) column[k] = Y.column[static_cast<size_t>(k)];
    }
    return PE_HIP_OK;
}

/* DC sensitivities by the adjoint method: one solve of the transposed small-signal system at omega = 0 per output -- the sweep body of
 * pe_hip_analyze_ac_sweep on the adjoint system with state of its own (h->sens), every slot of a pass with the selector of its own output
 * (k_sens_rhs) --, then d f / d p against the adjoint solution and the weighted sum of squares on the device (k_sens_accumulate).
 * Definitions: include/pe_hip.h. */
int pe_hip_analyze_sens(pe_hip_engine* h, const pe_hip_sens_control* ctl, int* output_status, pe_hip_sens_stats* stats)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    if(stats) std::memset(stats, 0, sizeof(*stats));
    if(!ctl || ctl->n_outputs < 1 || !ctl->out_pos || !ctl->out_neg) return fail(h, PE_HIP_ERR_ARG, "analyze_sens: no control, n_outputs < 1 or no output rows");
    auto& hc = h->hc;
    int const B = hc.batch, N = hc.rows, n_out = ctl->n_outputs;
    for(int o = 0; o < n_out; ++o)
    {
        int const pos = ctl->out_pos[o], neg = ctl->out_neg[o];
        if(pos < -1 || pos >= N || neg < -1 || neg >= N) return fail(h, PE_HIP_ERR_ARG, "analyze_sens: output row out of range");
        if(pos == neg) return fail(h, PE_HIP_ERR_ARG, "analyze_sens: an output needs two different rows (-1: ground)");
    }
    if(has_overlay(h)) return fail(h, PE_HIP_ERR_ARG, "analyze_sens: host-stamped overlay models have no parameter description");
    sens_table_build(h);
    auto& Y = h->sens;
    int const n_par = static_cast<int>(Y.par.size());
    bool const keep = ctl->keep_sensitivities != 0, weighted = ctl->weight != nullptr;
    if(!keep && !weighted) return fail(h, PE_HIP_ERR_ARG, "analyze_sens: neither sensitivities nor a weighted sum asked for");
    for(int k = 0; weighted && k < n_par; ++k)
        if(!std::isfinite(ctl->weight[k])) return fail(h, PE_HIP_ERR_ARG, "analyze_sens: non-finite weight");
    HIPCHK(h, hipSetDevice(h->device));
    auto& A = Y.sys;
    auto& W = A.sweep;
    Y.valid = false;
    size_t const n_rss = weighted ? static_cast<size_t>(n_out) * B : 0;
    size_t const total = n_rss + (keep ? static_cast<size_t>(n_out) * B * n_par : 0);
    auto publish = [&](std::vector<int> const* pst, pe_hip_ac_sweep_stats const& S)
    {
        Y.n_outputs = n_out;
        Y.batch = B;
        Y.kept = keep;
        Y.weighted = weighted;
        Y.valid = true;
        if(output_status && pst) std::copy(pst->begin(), pst->end(), output_status);
        if(stats)
        {
            stats->n_outputs = n_out;
            stats->n_params = n_par;
            stats->n_passes = S.n_passes;
            stats->outputs_per_pass = S.points_per_pass;
            stats->n_analyses = S.n_analyses;
            stats->n_refine_rounds = S.n_refine_rounds;
            stats->n_retried_outputs = S.n_fallback_points;
            stats->gpu_ms = S.gpu_ms;
        }
    };

    // an instance whose last analysis failed has no operating point to linearise at: the call carries that status instead of numbers
    int bad = -1, bad_status = PE_HIP_OK;
    if(int const rc = operating_point_status(h, bad, bad_status); rc != PE_HIP_OK) return rc;
    Y.res.assign(total, std::nan(""));
    if(bad >= 0)
    {
        std::vector<int> const pst(static_cast<size_t>(n_out), bad_status);
        publish(&pst, pe_hip_ac_sweep_stats{});
        return fail(h, bad_status, "analyze_sens: instance " + std::to_string(bad) + " has no operating point (its last analysis failed)");
    }
    pe_hip_ac_sweep_stats S{};
    std::vector<int> pst(static_cast<size_t>(n_out), PE_HIP_OK);
    if(N == 0)
    {
        publish(&pst, S);
        return PE_HIP_OK;
    }

    // ---- the adjoint system (its right-hand-side lists hold the first output's selector; every pass writes its own: k_sens_rhs)
    if(!A.built)
    {
        pe::AcAdjoint const adj{ctl->out_pos[0], ctl->out_neg[0]};
        if(int const rc = ensure_ac_built(h, A, &adj); rc != PE_HIP_OK) return rc;
    }

    // ---- per circuit: parameter table and stamp lists; per call: raw columns, weights, output rows
    if(!Y.table_on_device)
    {
        Y.tab_pool.release();
        Y.d_draw = Y.d_graw = Y.d_weight = nullptr;
        HIPCHK(h, Y.tab_pool.upload(Y.V.par, Y.par));
        HIPCHK(h, Y.tab_pool.upload(Y.V.sl_ptr, Y.sl_ptr));
        HIPCHK(h, Y.tab_pool.upload(Y.V.sl_ent, Y.sl_ent));
        HIPCHK(h, Y.tab_pool.alloc(Y.d_draw, hc.d_raw.size(), false));
        HIPCHK(h, Y.tab_pool.alloc(Y.d_graw, hc.gen_par.size(), false));
        HIPCHK(h, Y.tab_pool.alloc(Y.d_weight, static_cast<size_t>(n_par), false));
        Y.table_on_device = true;
    }
    if(!hc.d_raw.empty()) HIPCHK(h, hipMemcpy(Y.d_draw, hc.d_raw.data(), hc.d_raw.size() * sizeof(double), hipMemcpyHostToDevice));
    if(!hc.gen_par.empty()) HIPCHK(h, hipMemcpy(Y.d_graw, hc.gen_par.data(), hc.gen_par.size() * sizeof(double), hipMemcpyHostToDevice));
    if(weighted && n_par > 0) HIPCHK(h, hipMemcpy(Y.d_weight, ctl->weight, static_cast<size_t>(n_par) * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, Y.d_out_pos.ensure_at_least(static_cast<size_t>(n_out), false));
    HIPCHK(h, Y.d_out_neg.ensure_at_least(static_cast<size_t>(n_out), false));
    HIPCHK(h, hipMemcpy(Y.d_out_pos.p, ctl->out_pos, static_cast<size_t>(n_out) * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(Y.d_out_neg.p, ctl->out_neg, static_cast<size_t>(n_out) * sizeof(int), hipMemcpyHostToDevice));
    Y.V.n_par = n_par;
    Y.V.n_chunks = std::max(1, (n_par + pe::SENS_CHUNK - 1) / pe::SENS_CHUNK);
    Y.V.n_inst = B;
    Y.V.n_half = N;
    Y.V.gen_par_len = hc.gen_par_len;
    Y.V.normalized = ctl->normalized != 0 ? 1 : 0;
    Y.V.rhs0 = A.rhs0;
    Y.V.d_raw = Y.d_draw;
    Y.V.g_raw = Y.d_graw;
    Y.V.weight = weighted ? Y.d_weight : nullptr;
    Y.V.out_pos = Y.d_out_pos.p;
    Y.V.out_neg = Y.d_out_neg.p;

    std::vector<double> const omegas(static_cast<size_t>(n_out), 0.0);  // every output is a point at omega = 0: one band, one analysis
    SweepHooks hooks;
    hooks.name = "analyze_sens";
    hooks.pass_knob = "SENS_OUTPUTS";
    // what belongs to output i in the result buffer: its rss row (weighted), its block of sensitivities (kept)
    hooks.res = &Y.res;
    if(weighted) hooks.blocks.push_back({nullptr, 0, static_cast<size_t>(B), true, true});
    if(keep) hooks.blocks.push_back({nullptr, n_rss, static_cast<size_t>(B) * n_par, true, true});
    hooks.prepare = [&](int P) -> int
    {
        HIPCHK(h, Y.d_res.ensure(total, false));
        HIPCHK(h, Y.d_res.fill_nan());
        HIPCHK(h, Y.partial.ensure(static_cast<size_t>(B) * P * Y.V.n_chunks));
        Y.V.partial = Y.partial.p;
        Y.V.P = P;
        Y.V.xacc = W.V.xacc;
        Y.V.point = W.V.point;
        Y.V.rss = weighted ? Y.d_res.p : nullptr;
        Y.V.s = keep ? Y.d_res.p + n_rss : nullptr;
        for(auto& blk: hooks.blocks) blk.dev = Y.d_res.p + blk.host;
        return PE_HIP_OK;
    };
    hooks.after_fill = [&](pe_hip_engine* E) -> int
    {
        HIPCHK(h, pe::launch_sens_rhs(E->stream, E->V, Y.V));
        return PE_HIP_OK;
    };
    hooks.epilogue = [&](pe_hip_engine* E) -> int
    {
        HIPCHK(h, pe::launch_sens_accumulate(E->stream, E->V, h->V, Y.V));
        return PE_HIP_OK;
    };
    if(int const rc = sweep_body(h, A, n_out, omegas.data(), pst, S, hooks); rc != PE_HIP_OK) return rc;
    publish(&pst, S);
    for(int i = 0; i < n_out; ++i)
        if(pst[i] != PE_HIP_OK) return fail(h, pst[i], "analyze_sens: output " + std::to_string(i) + " failed");
    return PE_HIP_OK;
}

int pe_hip_get_sens(pe_hip_engine* h, int first_output, int n_outputs, int first_instance, int count, double* s, double* rss)
{
    if(!h || !h->loaded || (!s && !rss)) return PE_HIP_ERR_ARG;
    auto const& Y = h->sens;
    if(int const rc = stored_window(h, "get_sens", "sensitivity analysis", "outputs", Y.valid, Y.batch, Y.n_outputs, first_output, n_outputs, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    if(s && !Y.kept) return fail(h, PE_HIP_ERR_ARG, "get_sens: the sensitivities were not kept (pe_hip_sens_control.keep_sensitivities)");
    if(rss && !Y.weighted) return fail(h, PE_HIP_ERR_ARG, "get_sens: no weighted sum was formed (pe_hip_sens_control.weight)");
    size_t const n_par = Y.par.size(), n_rss = Y.weighted ? static_cast<size_t>(Y.n_outputs) * Y.batch : 0;
    for(int i = 0; i < n_outputs && count > 0; ++i)
    {
        size_t const src = static_cast<size_t>(first_output + i) * Y.batch + first_instance, dst = static_cast<size_t>(i) * count;
        if(rss) std::memcpy(rss + dst, &Y.res[src], static_cast<size_t>(count) * sizeof(double));
        if(s && n_par > 0) std::memcpy(s + dst * n_par, &Y.res[n_rss + src * n_par], static_cast<size_t>(count) * n_par * sizeof(double));
    }
    return PE_HIP_OK;
}

}  // extern "C"


namespace
{
    static_assert(pe::NET_MAX_PORTS == PE_HIP_NET_MAX_PORTS && pe::NET_ERR_SINGULAR == PE_HIP_ERR_SINGULAR, "pe_net.hpp names these without including the C header");

    bool net_z0_ok(double const* z0, int n)
    {
        for(int i = 0; z0 && i < n; ++i)
            if(!std::isfinite(z0[i]) || !(z0[i] > 0.0)) return false;
        return true;
    }
}  // namespace

extern "C" {

/* Z, Y and S of the circuit between n ports over a frequency sweep: the sweep body of pe_hip_analyze_ac_sweep on a forward system with
 * state of its own (h->net) whose right-hand side is a port's selector -- one factorisation per pass, the ports after the first solved
 * with the factors kept (dc_solve_kept) --, columns gathered on the device (k_net_gather), the dense conversion there too (k_net_convert).
 * Definitions: include/pe_hip.h. */
int pe_hip_analyze_net(pe_hip_engine* h, int n_points, const double* omegas, const pe_hip_net_control* ctl, int* point_status, pe_hip_net_stats* stats)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    if(stats) std::memset(stats, 0, sizeof(*stats));
    if(n_points < 1 || !omegas || !ctl) return fail(h, PE_HIP_ERR_ARG, "analyze_net: n_points < 1, no omegas or no control");
    for(int i = 0; i < n_points; ++i)
        if(!std::isfinite(omegas[i]) || omegas[i] < 0.0) return fail(h, PE_HIP_ERR_ARG, "analyze_net: negative or non-finite omega");
    auto& hc = h->hc;
    int const B = hc.batch, N = hc.rows, n = ctl->n_ports;
    if(n < 1 || n > PE_HIP_NET_MAX_PORTS || !ctl->port_pos || !ctl->port_neg) return fail(h, PE_HIP_ERR_ARG, "analyze_net: n_ports out of range or no port rows");
    for(int i = 0; i < n; ++i)
    {
        int const pos = ctl->port_pos[i], neg = ctl->port_neg[i];
        if(pos < -1 || pos >= N || neg < -1 || neg >= N) return fail(h, PE_HIP_ERR_ARG, "analyze_net: port row out of range");
        if(pos == neg) return fail(h, PE_HIP_ERR_ARG, "analyze_net: a port needs two different rows (-1: ground)");
        for(int k = 0; k < i; ++k)
            if(ctl->port_pos[k] == pos && ctl->port_neg[k] == neg) return fail(h, PE_HIP_ERR_ARG, "analyze_net: two identical ports");
    }
    if(!net_z0_ok(ctl->z0, n)) return fail(h, PE_HIP_ERR_ARG, "analyze_net: a reference resistance is not finite or not positive");
    if(has_overlay(h)) return fail(h, PE_HIP_ERR_ARG, "analyze_net: host-stamped overlay models are not supported");
    HIPCHK(h, hipSetDevice(h->device));
    auto& Z = h->net;
    auto& A = Z.sys;
    auto& W = A.sweep;
    Z.valid = false;
    size_t const nn = static_cast<size_t>(n) * n, n_mats = static_cast<size_t>(n_points) * B, plane = n_mats * nn;
    pe_hip_ac_sweep_stats S{};
    S.n_points = n_points;
    int n_fact = 0, n_solves = 0;
    std::vector<int> pst(static_cast<size_t>(n_points), PE_HIP_OK);
    auto publish = [&]()
    {
        Z.n_points = n_points;
        Z.batch = B;
        Z.n_ports = n;
        Z.valid = true;
        if(point_status) std::copy(pst.begin(), pst.end(), point_status);
        if(stats)
        {
            stats->n_points = n_points;
            stats->n_ports = n;
            stats->n_passes = S.n_passes;
            stats->points_per_pass = S.points_per_pass;
            stats->n_analyses = S.n_analyses;
            stats->n_factorisations = n_fact;
            stats->n_solves = n_solves;
            stats->n_refine_rounds = S.n_refine_rounds;
            stats->n_retried_points = S.n_fallback_points;
            stats->gpu_ms = S.gpu_ms;
        }
    };
    // what belongs to point i: its block of every plane -- the sweep body copies and checks the two of Z; Y and S are made after it --, its statuses
    SweepHooks hooks;
    hooks.res = &Z.res;
    for(size_t pl = 0; pl < 6; ++pl) hooks.blocks.push_back({nullptr, pl * plane, static_cast<size_t>(B) * nn, pl < 2, pl < 2});
    auto blank = [&](int i, int status)
    {
        point_blank(hooks, i);
        for(int w = 0; w < 2; ++w) std::fill_n(Z.status.begin() + w * n_mats + static_cast<size_t>(i) * B, static_cast<size_t>(B), status);
    };
    Z.res.assign(6 * plane, std::nan(""));
    Z.status.assign(2 * n_mats, PE_HIP_OK);

    // an instance whose last analysis failed has no operating point to linearise at: the call carries that status instead of numbers
    int bad = -1, bad_status = PE_HIP_OK;
    if(int const rc = operating_point_status(h, bad, bad_status); rc != PE_HIP_OK) return rc;
    if(bad >= 0)
    {
        std::fill(pst.begin(), pst.end(), bad_status);
        for(int i = 0; i < n_points; ++i) blank(i, bad_status);
        publish();
        return fail(h, bad_status, "analyze_net: instance " + std::to_string(bad) + " has no operating point (its last analysis failed)");
    }

    // ---- the forward system; its right-hand-side lists select port 0 (the circuit's own AC sources are switched off)
    int const pos0 = ctl->port_pos[0], neg0 = ctl->port_neg[0];
    if(!A.built)
    {
        if(int const rc = ensure_ac_built(h, A); rc != PE_HIP_OK) return rc;
        Z.have_port0 = false;
    }
    if(!Z.have_port0 || Z.pos0 != pos0 || Z.neg0 != neg0) select_rhs(A, pos0, neg0);
    Z.have_port0 = true;
    Z.pos0 = pos0;
    Z.neg0 = neg0;

    // ---- the ports of this call
    if(!Z.d_pos)
    {
        HIPCHK(h, Z.port_pool.alloc(Z.d_pos, PE_HIP_NET_MAX_PORTS));
        HIPCHK(h, Z.port_pool.alloc(Z.d_neg, PE_HIP_NET_MAX_PORTS));
        HIPCHK(h, Z.port_pool.alloc(Z.d_z0, PE_HIP_NET_MAX_PORTS));
    }
    {
        double z0[PE_HIP_NET_MAX_PORTS];
        for(int i = 0; i < n; ++i) z0[i] = ctl->z0 ? ctl->z0[i] : 50.0;
        HIPCHK(h, hipMemcpy(Z.d_pos, ctl->port_pos, static_cast<size_t>(n) * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(Z.d_neg, ctl->port_neg, static_cast<size_t>(n) * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(Z.d_z0, z0, static_cast<size_t>(n) * sizeof(double), hipMemcpyHostToDevice));
    }

    int cur = 0;  // the port whose right-hand side the pass is solving
    hooks.name = "analyze_net";
    hooks.pass_knob = "NET_POINTS";
    hooks.n_rhs = n;
    hooks.keep_factors = true;
    hooks.n_factorisations = &n_fact;
    hooks.n_solves = &n_solves;
    hooks.prepare = [&](int P) -> int
    {
        // (the planes are sized by n_points x batch x n^2, the statuses by n_points x batch: two calls can agree in one and not in the other)
        if(Z.d_res.len != 6 * plane || Z.d_status.len != 2 * n_mats)
        {
            Z.d_res.release();
            Z.d_status.release();
        }
        HIPCHK(h, Z.d_res.ensure(6 * plane, false));
        HIPCHK(h, Z.d_status.ensure(2 * n_mats, false));
        HIPCHK(h, Z.d_res.fill_nan());
        for(auto& blk: hooks.blocks) blk.dev = Z.d_res.p + blk.host;
        Z.V.n_ports = n;
        Z.V.P = P;
        Z.V.n_inst = B;
        Z.V.n_half = N;
        Z.V.rhs0 = A.rhs0;
        Z.V.pos = Z.d_pos;
        Z.V.neg = Z.d_neg;
        Z.V.z0 = Z.d_z0;
        Z.V.point = W.V.point;
        Z.V.xacc = W.V.xacc;
        Z.V.b0 = W.V.b0;
        Z.V.z_re = Z.d_res.p;
        Z.V.z_im = Z.d_res.p + plane;
        cur = 0;
        return PE_HIP_OK;
    };
    hooks.next_rhs = [&](pe_hip_engine* E, int j) -> int
    {
        cur = j;
        HIPCHK(h, pe::launch_net_rhs(E->stream, E->V, Z.V, j));
        return PE_HIP_OK;
    };
    hooks.epilogue = [&](pe_hip_engine* E) -> int
    {
        HIPCHK(h, pe::launch_net_gather(E->stream, E->V, Z.V, cur));
        if(cur == n - 1) cur = 0;
        return PE_HIP_OK;
    };
    if(int const rc = sweep_body(h, A, n_points, omegas, pst, S, hooks); rc != PE_HIP_OK) return rc;

    // ---- Y and S of every (point, instance) on the device, from the impedance matrices as they stand there
    {
        double* const d = Z.d_res.p;
        HIPCHK(h, hipEventRecord(h->ev0, h->stream));
        HIPCHK(h, pe::launch_net_convert(h->stream, n, static_cast<int>(n_mats), d, d + plane, Z.d_z0, d + 2 * plane, d + 3 * plane, d + 4 * plane, d + 5 * plane,
                                         Z.d_status.p, Z.d_status.p + n_mats));
        HIPCHK(h, hipEventRecord(h->ev1, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        S.gpu_ms += ms;
        HIPCHK(h, hipMemcpy(Z.res.data() + 2 * plane, d + 2 * plane, 4 * plane * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(Z.status.data(), Z.d_status.p, 2 * n_mats * sizeof(int), hipMemcpyDeviceToHost));
    }
    // a failed point reads NaN and carries its status
    for(int i = 0; i < n_points; ++i)
        if(pst[i] != PE_HIP_OK) blank(i, pst[i]);
    publish();
    for(int i = 0; i < n_points; ++i)
        if(pst[i] != PE_HIP_OK) return fail(h, pst[i], "analyze_net: point " + std::to_string(i) + " failed");
    return PE_HIP_OK;
}

int pe_hip_get_net(pe_hip_engine* h, int which, int first_point, int n_points, int first_instance, int count, double* re, double* im)
{
    if(!h || !h->loaded || !re || !im || which < PE_HIP_NET_Z || which > PE_HIP_NET_S) return PE_HIP_ERR_ARG;
    auto const& Z = h->net;
    if(int const rc = stored_window(h, "get_net", "network analysis", "points", Z.valid, Z.batch, Z.n_points, first_point, n_points, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    size_t const nn = static_cast<size_t>(Z.n_ports) * Z.n_ports, plane = static_cast<size_t>(Z.n_points) * Z.batch * nn;
    for(int i = 0; i < n_points && count > 0; ++i)
    {
        size_t const src = (static_cast<size_t>(first_point + i) * Z.batch + first_instance) * nn, dst = static_cast<size_t>(i) * count * nn;
        std::memcpy(re + dst, &Z.res[2 * which * plane + src], static_cast<size_t>(count) * nn * sizeof(double));
        std::memcpy(im + dst, &Z.res[(2 * which + 1) * plane + src], static_cast<size_t>(count) * nn * sizeof(double));
    }
    return PE_HIP_OK;
}

int pe_hip_get_net_status(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, int* y_status, int* s_status)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    auto const& Z = h->net;
    if(int const rc = stored_window(h, "get_net_status", "network analysis", "points", Z.valid, Z.batch, Z.n_points, first_point, n_points, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    size_t const n_mats = static_cast<size_t>(Z.n_points) * Z.batch;
    for(int i = 0; i < n_points && count > 0; ++i)
    {
        size_t const src = static_cast<size_t>(first_point + i) * Z.batch + first_instance, dst = static_cast<size_t>(i) * count;
        if(y_status) std::memcpy(y_status + dst, &Z.status[src], static_cast<size_t>(count) * sizeof(int));
        if(s_status) std::memcpy(s_status + dst, &Z.status[n_mats + src], static_cast<size_t>(count) * sizeof(int));
    }
    return PE_HIP_OK;
}

/* the conversion kernel of pe_hip_analyze_net on the caller's matrices */
int pe_hip_convert_net(pe_hip_engine* h, int n_ports, int n_mats, const double* z_re, const double* z_im, const double* z0, double* y_re, double* y_im,
                       double* s_re, double* s_im, int* y_status, int* s_status)
{
    if(!h) return PE_HIP_ERR_ARG;
    if(n_ports < 1 || n_ports > PE_HIP_NET_MAX_PORTS || n_mats < 1 || !z_re || !z_im) return fail(h, PE_HIP_ERR_ARG, "convert_net: n_ports out of range, n_mats < 1 or no matrices");
    if(!net_z0_ok(z0, n_ports)) return fail(h, PE_HIP_ERR_ARG, "convert_net: a reference resistance is not finite or not positive");
    HIPCHK(h, hipSetDevice(h->device));
    size_t const plane = static_cast<size_t>(n_mats) * n_ports * n_ports;
    Pool pool;
    double *d{}, *d_z0{};
    int* d_status{};
    HIPCHK(h, pool.alloc(d, 6 * plane, false));
    HIPCHK(h, pool.alloc(d_z0, PE_HIP_NET_MAX_PORTS));
    HIPCHK(h, pool.alloc(d_status, 2 * static_cast<size_t>(n_mats), false));
    double ref[PE_HIP_NET_MAX_PORTS];
    for(int i = 0; i < n_ports; ++i) ref[i] = z0 ? z0[i] : 50.0;
    HIPCHK(h, hipMemcpy(d, z_re, plane * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d + plane, z_im, plane * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d_z0, ref, static_cast<size_t>(n_ports) * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, pe::launch_net_convert(h->stream, n_ports, n_mats, d, d + plane, d_z0, d + 2 * plane, d + 3 * plane, d + 4 * plane, d + 5 * plane, d_status,
                                     d_status + n_mats));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double* const out[4] = {y_re, y_im, s_re, s_im};
    for(int k = 0; k < 4; ++k)
        if(out[k]) HIPCHK(h, hipMemcpy(out[k], d + (2 + k) * plane, plane * sizeof(double), hipMemcpyDeviceToHost));
    if(y_status) HIPCHK(h, hipMemcpy(y_status, d_status, static_cast<size_t>(n_mats) * sizeof(int), hipMemcpyDeviceToHost));
    if(s_status) HIPCHK(h, hipMemcpy(s_status, d_status + n_mats, static_cast<size_t>(n_mats) * sizeof(int), hipMemcpyDeviceToHost));
    return PE_HIP_OK;
}

}  // extern "C"

static_assert(pe::PZ_MAX_KRYLOV == PE_HIP_PZ_MAX_KRYLOV && pe::PZ_ERR_SINGULAR == PE_HIP_ERR_SINGULAR && pe::PZ_ERR_NO_CONVERGENCE == PE_HIP_ERR_NO_CONVERGENCE,
              "pe_pz.hpp names these without including the C header");

extern "C" {

/* Poles and zeros nearest to s0 = j omega0: the sweep body of pe_hip_analyze_ac_sweep on a forward system with state of its own (h->pz),
 * ONE pass of ONE point whose engine keeps its factors -- the first right-hand side is b (z = A0^-1 b, H(s0)), then every Arnoldi step is
 * one more: (omega0 B) v written by k_pz_bmul, the refined kept-factor solve, k_pz_orth in the epilogue; k_pz_ritz after the last step of
 * a kind.  Definitions: include/pe_hip.h. */
int pe_hip_analyze_pz(pe_hip_engine* h, const pe_hip_pz_control* ctl, int* instance_status, pe_hip_pz_stats* stats)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    if(stats) std::memset(stats, 0, sizeof(*stats));
    if(!ctl) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: no control");
    auto& hc = h->hc;
    int const B = hc.batch, N = hc.rows;
    int const what = ctl->what, m = ctl->max_krylov == 0 ? 32 : ctl->max_krylov;
    if(what < 1 || what > 3) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: what must be 1 (poles), 2 (zeros) or 3 (both)");
    if(!std::isfinite(ctl->omega0) || !(ctl->omega0 > 0.0)) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: omega0 must be finite and positive");
    if(m < 1 || m > PE_HIP_PZ_MAX_KRYLOV) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: max_krylov out of range");
    if(ctl->n_wanted < 1 || ctl->n_wanted > PE_HIP_PZ_MAX_KRYLOV) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: n_wanted out of range");
    if(ctl->n_wanted > m) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: n_wanted > max_krylov");
    for(double const v: {ctl->tol, ctl->theta_floor, ctl->breakdown_tol})
        if(!std::isfinite(v) || v < 0.0) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: tol, theta_floor and breakdown_tol must be finite and not negative");
    bool const zeros = (what & PE_HIP_PZ_ZEROS) != 0, poles = (what & PE_HIP_PZ_POLES) != 0;
    if(zeros)
    {
        for(int const r: {ctl->in_pos, ctl->in_neg, ctl->out_pos, ctl->out_neg})
            if(r < -1 || r >= N) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: port row out of range");
        if(ctl->in_pos == ctl->in_neg || ctl->out_pos == ctl->out_neg) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: a port needs two different rows (-1: ground)");
    }
    if(has_overlay(h)) return fail(h, PE_HIP_ERR_ARG, "analyze_pz: host-stamped overlay models are not supported");
    size_t const R2 = 2 * static_cast<size_t>(N);
    if(static_cast<long long>(static_cast<size_t>(B) * (m + 1) * R2 * sizeof(double)) > sweep_memory_budget())
        return fail(h, PE_HIP_ERR_ARG, "analyze_pz: the Krylov basis (batch x (max_krylov + 1) x 2 rows doubles) does not fit the memory budget");
    HIPCHK(h, hipSetDevice(h->device));
    auto& Z = h->pz;
    auto& A = Z.sys;
    auto& W = A.sweep;
    Z.valid = false;
    double const tol = ctl->tol == 0.0 ? 1.0e-10 : ctl->tol, theta_floor = ctl->theta_floor == 0.0 ? 1.0e-12 : ctl->theta_floor;
    double const breakdown_tol = ctl->breakdown_tol == 0.0 ? 0x1p-40 : ctl->breakdown_tol;
    int const kinds[2] = {poles ? PE_HIP_PZ_POLES : PE_HIP_PZ_ZEROS, PE_HIP_PZ_ZEROS}, n_kinds = (poles && zeros) ? 2 : 1;
    size_t const plane = static_cast<size_t>(B) * m;
    for(int t = 0; t < 2; ++t)
    {
        Z.res[t].assign(3 * plane, std::nan(""));
        Z.n_found[t].assign(static_cast<size_t>(B), 0);
        Z.n_conv[t].assign(static_cast<size_t>(B), 0);
        Z.complete[t].assign(static_cast<size_t>(B), 0);
        Z.status[t].assign(static_cast<size_t>(B), PE_HIP_OK);
    }
    Z.gain.assign(2 * static_cast<size_t>(B), std::nan(""));
    std::vector<int> worst(static_cast<size_t>(B), PE_HIP_OK);
    pe_hip_ac_sweep_stats S{};
    int n_fact = 0, n_solves = 0, steps_run = 0;
    auto publish = [&]() -> int
    {
        Z.batch = B;
        Z.capacity = m;
        Z.what = what;
        Z.valid = true;
        for(int t = 0; t < n_kinds; ++t)
            for(int b = 0; b < B; ++b)
                if(worst[b] == PE_HIP_OK) worst[b] = Z.status[kinds[t] - 1][b];
        if(instance_status) std::copy(worst.begin(), worst.end(), instance_status);
        if(stats)
        {
            stats->n_steps = steps_run;
            stats->n_factorisations = n_fact;
            stats->n_solves = n_solves;
            stats->n_refine_rounds = S.n_refine_rounds;
            auto const& done = Z.complete[kinds[0] - 1];
            stats->n_complete = static_cast<int>(std::count(done.begin(), done.end(), 1));
            stats->gpu_ms = S.gpu_ms;
        }
        for(int b = 0; b < B; ++b)
            if(worst[b] != PE_HIP_OK) return fail(h, worst[b], "analyze_pz: instance " + std::to_string(b) + " failed");
        return PE_HIP_OK;
    };
    if(N == 0) return publish();

    // an instance whose last analysis failed has no operating point to linearise at: the call carries that status instead of numbers
    int bad = -1, bad_status = PE_HIP_OK;
    if(int const rc = operating_point_status(h, bad, bad_status); rc != PE_HIP_OK) return rc;
    if(bad >= 0)
    {
        for(int t = 0; t < n_kinds; ++t) std::fill(Z.status[kinds[t] - 1].begin(), Z.status[kinds[t] - 1].end(), bad_status);
        (void)publish();
        return fail(h, bad_status, "analyze_pz: instance " + std::to_string(bad) + " has no operating point (its last analysis failed)");
    }

    // ---- the forward system; its right-hand-side lists select the input port (poles alone: row 0 -- the first solve is the one that factors)
    int const pos0 = zeros ? ctl->in_pos : 0, neg0 = zeros ? ctl->in_neg : -1;
    if(!A.built)
    {
        if(int const rc = ensure_ac_built(h, A); rc != PE_HIP_OK) return rc;
        Z.have_port = false;
    }
    if(!Z.have_port || Z.pos0 != pos0 || Z.neg0 != neg0) select_rhs(A, pos0, neg0);
    Z.have_port = true;
    Z.pos0 = pos0;
    Z.neg0 = neg0;

    std::vector<int> pst(1, PE_HIP_OK), inst;
    bool unanalysable = false;
    int kind_at = 0, step_at = -1;  // the right-hand side the pass is solving: -1: b; else step `step_at` of kind `kind_at`
    size_t const cnt = 5 * static_cast<size_t>(B);  // per kind: n_found | n_converged | Ritz status | parked | steps
    SweepHooks hooks;
    hooks.name = "analyze_pz";
    hooks.pass_knob = "PZ_POINTS";
    hooks.n_rhs = 1 + n_kinds * (m + 1);
    hooks.keep_factors = true;
    hooks.n_factorisations = &n_fact;
    hooks.n_solves = &n_solves;
    hooks.inst_status = &inst;
    hooks.single = [&](int) -> int
    {
        unanalysable = inst.empty();  // (no pass ran: the band's values could not be analysed)
        return PE_HIP_OK;
    };
    hooks.prepare = [&](int P) -> int
    {
        if(P != 1) return fail(h, PE_HIP_ERR_INTERNAL, "analyze_pz: more than one point per pass");
        if(Z.buf_batch != static_cast<size_t>(B) || Z.buf_rows != R2 || Z.buf_m != m)
        {
            Z.buf_pool.release();
            Z.V = pe::PzView{};
            Z.buf_batch = Z.buf_rows = 0;
            Z.buf_m = 0;
            HIPCHK(h, Z.buf_pool.alloc(Z.V.basis, static_cast<size_t>(B) * (m + 1) * R2));
            HIPCHK(h, Z.buf_pool.alloc(Z.V.h_re, static_cast<size_t>(B) * (m + 1) * m));
            HIPCHK(h, Z.buf_pool.alloc(Z.V.h_im, static_cast<size_t>(B) * (m + 1) * m));
            HIPCHK(h, Z.buf_pool.alloc(Z.V.zvec, static_cast<size_t>(B) * R2));
            HIPCHK(h, Z.buf_pool.alloc(Z.V.gain, 2 * static_cast<size_t>(B)));
            HIPCHK(h, Z.buf_pool.alloc(Z.V.steps, static_cast<size_t>(B)));
            HIPCHK(h, Z.buf_pool.alloc(Z.V.parked, static_cast<size_t>(B)));
            Z.buf_batch = static_cast<size_t>(B);
            Z.buf_rows = R2;
            Z.buf_m = m;
        }
        HIPCHK(h, Z.d_res.ensure(2 * 3 * plane, false));
        HIPCHK(h, Z.d_cnt.ensure(2 * cnt, false));
        HIPCHK(h, Z.d_res.fill_nan());
        HIPCHK(h, hipMemset(Z.d_cnt.p, 0, Z.d_cnt.len * sizeof(int)));
        Z.V.n_half = N;
        Z.V.rhs0 = A.rhs0;
        Z.V.m_max = m;
        Z.V.in_pos = zeros ? ctl->in_pos : -1;
        Z.V.in_neg = zeros ? ctl->in_neg : -1;
        Z.V.out_pos = zeros ? ctl->out_pos : -1;
        Z.V.out_neg = zeros ? ctl->out_neg : -1;
        Z.V.breakdown_tol = breakdown_tol;
        Z.V.xacc = W.V.xacc;
        Z.V.b0 = W.V.b0;
        return PE_HIP_OK;
    };
    hooks.after_fill = [&](pe_hip_engine*) -> int
    {
        kind_at = 0;
        step_at = -1;
        return PE_HIP_OK;
    };
    hooks.next_rhs = [&](pe_hip_engine* E, int j) -> int
    {
        kind_at = (j - 1) / (m + 1);
        step_at = (j - 1) % (m + 1);
        if(step_at == 0)  // a kind starts: every instance runs again, the Hessenberg matrices are this kind's
        {
            HIPCHK(h, hipMemsetAsync(Z.V.steps, 0, static_cast<size_t>(B) * sizeof(int), E->stream));
            HIPCHK(h, hipMemsetAsync(Z.V.parked, 0, static_cast<size_t>(B) * sizeof(int), E->stream));
            HIPCHK(h, hipMemsetAsync(Z.V.h_re, 0, static_cast<size_t>(B) * (m + 1) * m * sizeof(double), E->stream));
            HIPCHK(h, hipMemsetAsync(Z.V.h_im, 0, static_cast<size_t>(B) * (m + 1) * m * sizeof(double), E->stream));
        }
        HIPCHK(h, pe::launch_pz_bmul(E->stream, E->V, Z.V, step_at - 1));
        return PE_HIP_OK;
    };
    hooks.epilogue = [&](pe_hip_engine* E) -> int
    {
        if(step_at < 0)
        {
            HIPCHK(h, pe::launch_pz_store_z(E->stream, E->V, Z.V));
            return PE_HIP_OK;
        }
        bool const kz = kinds[kind_at] == PE_HIP_PZ_ZEROS;
        HIPCHK(h, pe::launch_pz_orth(E->stream, E->V, Z.V, step_at, kz));
        if(step_at < m) return PE_HIP_OK;
        // the last step of a kind: its Ritz values, and what the next kind overwrites
        double* const d = Z.d_res.p + static_cast<size_t>(kind_at) * 3 * plane;
        int* const c = Z.d_cnt.p + static_cast<size_t>(kind_at) * cnt;
        pe::PzRitzView R{};
        R.n_mats = B;
        R.m = m;
        R.steps = Z.V.steps;
        R.parked = Z.V.parked;
        R.h_re = Z.V.h_re;
        R.h_im = Z.V.h_im;
        R.mat_stride = static_cast<long long>(m + 1) * m;
        R.ld = m;
        R.omega0 = ctl->omega0;
        R.theta_floor = theta_floor;
        R.tol = tol;
        R.s_re = d;
        R.s_im = d + plane;
        R.s_err = d + 2 * plane;
        R.n_found = c;
        R.n_conv = c + B;
        R.status = c + 2 * B;
        HIPCHK(h, pe::launch_pz_ritz(E->stream, R));
        HIPCHK(h, hipMemcpyAsync(c + 3 * B, Z.V.parked, static_cast<size_t>(B) * sizeof(int), hipMemcpyDeviceToDevice, E->stream));
        HIPCHK(h, hipMemcpyAsync(c + 4 * B, Z.V.steps, static_cast<size_t>(B) * sizeof(int), hipMemcpyDeviceToDevice, E->stream));
        return PE_HIP_OK;
    };
    if(int const rc = sweep_body(h, A, 1, &ctl->omega0, pst, S, hooks); rc != PE_HIP_OK) return rc;
    steps_run = inst.empty() ? 0 : m;  // (no pass ran where the band's values could not be analysed)

    // ---- results and statuses per instance
    std::vector<double> res(2 * 3 * plane);
    std::vector<int> c(2 * cnt);
    HIPCHK(h, hipMemcpy(res.data(), Z.d_res.p, res.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(c.data(), Z.d_cnt.p, c.size() * sizeof(int), hipMemcpyDeviceToHost));
    if(zeros) HIPCHK(h, hipMemcpy(Z.gain.data(), Z.V.gain, Z.gain.size() * sizeof(double), hipMemcpyDeviceToHost));
    for(int t = 0; t < n_kinds; ++t)
    {
        int const k = kinds[t] - 1;
        int const* ct = c.data() + static_cast<size_t>(t) * cnt;
        for(int b = 0; b < B; ++b)
        {
            int st = unanalysable ? PE_HIP_ERR_SINGULAR : (b < static_cast<int>(inst.size()) ? inst[b] : PE_HIP_OK);
            if(st == PE_HIP_OK && ct[3 * B + b] == pe::PZ_PARKED_FAILED) st = PE_HIP_ERR_SINGULAR;  // zeros: H(s0) is 0 or not finite; else a vector was not finite
            if(st == PE_HIP_OK) st = ct[2 * B + b];
            Z.status[k][b] = st;
            if(st != PE_HIP_OK) continue;
            for(int pl = 0; pl < 3; ++pl)
                std::copy_n(res.data() + (static_cast<size_t>(t) * 3 + pl) * plane + static_cast<size_t>(b) * m, m, Z.res[k].data() + pl * plane + static_cast<size_t>(b) * m);
            Z.n_found[k][b] = ct[b];
            Z.n_conv[k][b] = ct[B + b];
            Z.complete[k][b] = ct[3 * B + b] == pe::PZ_PARKED_COMPLETE ? 1 : 0;
        }
    }
    for(int b = 0; b < B; ++b)  // (an instance the engine failed has no gain either)
        if(unanalysable || (b < static_cast<int>(inst.size()) && inst[b] != PE_HIP_OK)) Z.gain[2 * b] = Z.gain[2 * b + 1] = std::nan("");
    return publish();
}

int pe_hip_get_pz(pe_hip_engine* h, int which, int first_instance, int count, int capacity, double* re, double* im, double* err_est, int* n_found,
                  int* n_converged, int* complete)
{
    if(!h || !h->loaded || (which != PE_HIP_PZ_POLES && which != PE_HIP_PZ_ZEROS) || capacity < 0) return PE_HIP_ERR_ARG;
    auto const& Z = h->pz;
    if(int const rc = stored_window(h, "get_pz", "pole-zero analysis", nullptr, Z.valid, Z.batch, 0, 0, 0, first_instance, count); rc != PE_HIP_OK) return rc;
    if(!(Z.what & which)) return fail(h, PE_HIP_ERR_ARG, "get_pz: the last call did not ask for this kind");
    int const k = which - 1;
    size_t const plane = static_cast<size_t>(Z.batch) * Z.capacity;
    double* const out[3] = {re, im, err_est};
    for(int pl = 0; pl < 3; ++pl)
        for(int b = 0; out[pl] && b < count; ++b)
            for(int i = 0; i < capacity; ++i)
                out[pl][static_cast<size_t>(b) * capacity + i] = i < Z.capacity ? Z.res[k][pl * plane + static_cast<size_t>(first_instance + b) * Z.capacity + i] : std::nan("");
    for(int b = 0; b < count; ++b)
    {
        if(n_found) n_found[b] = Z.n_found[k][first_instance + b];
        if(n_converged) n_converged[b] = Z.n_conv[k][first_instance + b];
        if(complete) complete[b] = Z.complete[k][first_instance + b];
    }
    return PE_HIP_OK;
}

int pe_hip_get_pz_gain(pe_hip_engine* h, int first_instance, int count, double* re, double* im)
{
    if(!h || !h->loaded || !re || !im) return PE_HIP_ERR_ARG;
    auto const& Z = h->pz;
    if(int const rc = stored_window(h, "get_pz_gain", "pole-zero analysis", nullptr, Z.valid, Z.batch, 0, 0, 0, first_instance, count); rc != PE_HIP_OK) return rc;
    if(!(Z.what & PE_HIP_PZ_ZEROS)) return fail(h, PE_HIP_ERR_ARG, "get_pz_gain: the last call did not ask for zeros");
    for(int b = 0; b < count; ++b)
    {
        re[b] = Z.gain[2 * static_cast<size_t>(first_instance + b)];
        im[b] = Z.gain[2 * static_cast<size_t>(first_instance + b) + 1];
    }
    return PE_HIP_OK;
}

/* the Ritz kernel of pe_hip_analyze_pz on the caller's matrices */
int pe_hip_eig_hessenberg(pe_hip_engine* h, int m, int n_mats, const double* h_re, const double* h_im, double* theta_re, double* theta_im, double* last_re,
                          double* last_im, int* status)
{
    if(!h) return PE_HIP_ERR_ARG;
    if(m < 1 || m > PE_HIP_PZ_MAX_KRYLOV || n_mats < 1 || !h_re || !h_im || !theta_re || !theta_im || !last_re || !last_im || !status)
        return fail(h, PE_HIP_ERR_ARG, "eig_hessenberg: m out of range, n_mats < 1 or a null pointer");
    HIPCHK(h, hipSetDevice(h->device));
    size_t const mm = static_cast<size_t>(n_mats) * m * m, nm = static_cast<size_t>(n_mats) * m;
    Pool pool;
    double *d_h{}, *d_o{};
    int* d_status{};
    HIPCHK(h, pool.alloc(d_h, 2 * mm, false));
    HIPCHK(h, pool.alloc(d_o, 4 * nm, false));
    HIPCHK(h, pool.alloc(d_status, static_cast<size_t>(n_mats)));
    HIPCHK(h, hipMemcpy(d_h, h_re, mm * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d_h + mm, h_im, mm * sizeof(double), hipMemcpyHostToDevice));
    pe::PzRitzView R{};
    R.n_mats = n_mats;
    R.m = m;
    R.h_re = d_h;
    R.h_im = d_h + mm;
    R.mat_stride = static_cast<long long>(m) * m;
    R.ld = m;
    R.theta_re = d_o;
    R.theta_im = d_o + nm;
    R.last_re = d_o + 2 * nm;
    R.last_im = d_o + 3 * nm;
    R.status = d_status;
    HIPCHK(h, pe::launch_pz_ritz(h->stream, R));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double* const out[4] = {theta_re, theta_im, last_re, last_im};
    for(int k = 0; k < 4; ++k) HIPCHK(h, hipMemcpy(out[k], d_o + k * nm, nm * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(status, d_status, static_cast<size_t>(n_mats) * sizeof(int), hipMemcpyDeviceToHost));
    return PE_HIP_OK;
}

}  // extern "C"

#if !defined(__HIPCC__)
// Builds without HIP (the emulation library of tests/emu): the sweep's launchers as serial loops over the instances, with a one-thread
// team running the text of pe_ac_sweep.hpp
namespace pe
{
    namespace
    {
        struct SweepHostTeam
        {
            int tid() const { return 0; }
            int size() const { return 1; }
        };
    }  // namespace
    hipError_t launch_ac_sweep_fill(hipStream_t, DevView const& V, AcSweepView const& S)
    {
        for(int q = 0; q < V.batch; ++q) ac_sweep_fill(SweepHostTeam{}, V, S, q);
        return hipSuccess;
    }
    hipError_t launch_ac_residual_each(hipStream_t, DevView const& V, AcSweepView const& S)
    {
        *S.n_above = 0;
        for(int q = 0; q < V.batch; ++q)
        {
            S.worst[q] = ac_residual_each(SweepHostTeam{}, V, S, q);
            if(ac_needs_refinement(S.worst[q])) ++*S.n_above;
        }
        return hipSuccess;
    }
    hipError_t launch_ac_accumulate_each(hipStream_t, DevView const& V, AcSweepView const& S, bool first)
    {
        for(int q = 0; q < V.batch; ++q) ac_accumulate_each(SweepHostTeam{}, V, S, q, first);
        return hipSuccess;
    }
    hipError_t launch_ac_sweep_gather(hipStream_t, DevView const& V, AcSweepView const& S)
    {
        for(int q = 0; q < V.batch; ++q) ac_sweep_gather(SweepHostTeam{}, V, S, q);
        return hipSuccess;
    }
    // ... and the noise launchers with the text of pe_noise.hpp (one thread: every chunk is summed in ascending order)
    hipError_t launch_noise_sources(hipStream_t, DevView const& V, NoiseView const& Z)
    {
        for(int b = 0; b < V.batch; ++b) noise_sources(SweepHostTeam{}, V, Z, b);
        return hipSuccess;
    }
    hipError_t launch_noise_accumulate(hipStream_t, DevView const& V, NoiseView const& Z)
    {
        for(int q = 0; q < V.batch; ++q)
        {
            for(int c = 0; c < Z.n_chunks; ++c)
            {
                double const sum = noise_accumulate_chunk(SweepHostTeam{}, Z, V.rows, q, c);
                if(Z.n_chunks > 1) Z.partial[static_cast<long long>(q) * Z.n_chunks + c] = sum;
                else if(double* dst = noise_slot_psd(Z, q))
                    *dst = sum;
            }
            if(Z.n_chunks > 1) noise_finish(Z, q);
        }
        return hipSuccess;
    }
    // ... and the sensitivity launchers with the text of pe_sens.hpp
    hipError_t launch_sens_rhs(hipStream_t, DevView const& V, SensView const& Z)
    {
        for(int q = 0; q < V.batch; ++q) sens_rhs(SweepHostTeam{}, V, Z, q);
        return hipSuccess;
    }
    hipError_t launch_sens_accumulate(hipStream_t, DevView const& V, DevView const& M, SensView const& Z)
    {
        if(!Z.s && !Z.weight) return hipSuccess;
        for(int q = 0; q < V.batch; ++q)
        {
            for(int c = 0; c < Z.n_chunks; ++c)
            {
                double const sum = sens_accumulate_chunk(SweepHostTeam{}, M, Z, V.rows, q, c);
                if(!Z.weight) continue;
                if(Z.n_chunks > 1) Z.partial[static_cast<long long>(q) * Z.n_chunks + c] = sum;
                else if(double* dst = sens_slot_rss(Z, q))
                    *dst = sum;
            }
            if(Z.weight && Z.n_chunks > 1) sens_finish(Z, q);
        }
        return hipSuccess;
    }
    // ... and the network launchers with the text of pe_net.hpp (the conversion: a one-lane wave that holds the whole augmented matrix)
    hipError_t launch_net_rhs(hipStream_t, DevView const& V, NetView const& Z, int j)
    {
        for(int q = 0; q < V.batch; ++q) net_rhs(SweepHostTeam{}, V, Z, q, j);
        return hipSuccess;
    }
    hipError_t launch_net_gather(hipStream_t, DevView const& V, NetView const& Z, int j)
    {
        for(int q = 0; q < V.batch; ++q) net_gather(SweepHostTeam{}, V, Z, q, j);
        return hipSuccess;
    }
    hipError_t launch_net_convert(hipStream_t, int n, int n_mats, double const* z_re, double const* z_im, double const* z0, double* y_re, double* y_im,
                                  double* s_re, double* s_im, int* y_status, int* s_status)
    {
        for(long long m = 0; m < n_mats; ++m)  // (both callers have checked n)
        {
            long long const o = m * n * n;
            net_convert(NetSerialWave{}, n, z_re + o, z_im + o, z0, y_re ? y_re + o : nullptr, y_im ? y_im + o : nullptr, s_re ? s_re + o : nullptr,
                        s_im ? s_im + o : nullptr, y_status ? y_status + m : nullptr, s_status ? s_status + m : nullptr);
        }
        return hipSuccess;
    }
    // ... and the pole-zero launchers with the text of pe_pz.hpp (one thread sums in ascending order; the Ritz kernel's LDS is a heap buffer
    // of exactly its size)
    namespace
    {
        struct PzHostTeam
        {
            mutable double cr[PZ_MAX_KRYLOV], ci[PZ_MAX_KRYLOV];
            int tid() const { return 0; }
            int size() const { return 1; }
            void sync() const {}
            void sum2(double&, double&) const {}
            void keep(int j, double re, double im) const { cr[j] = re, ci[j] = im; }
            void kept(int j, double& re, double& im) const { re = cr[j], im = ci[j]; }
        };
    }  // namespace
    hipError_t launch_pz_bmul(hipStream_t, DevView const& V, PzView const& Z, int src)
    {
        for(int q = 0; q < V.batch; ++q) pz_bmul(SweepHostTeam{}, V, Z, q, src);
        return hipSuccess;
    }
    hipError_t launch_pz_store_z(hipStream_t, DevView const& V, PzView const& Z)
    {
        for(int q = 0; q < V.batch; ++q) pz_store_z(SweepHostTeam{}, V, Z, q);
        return hipSuccess;
    }
    hipError_t launch_pz_orth(hipStream_t, DevView const& V, PzView const& Z, int k, bool zeros)
    {
        PzHostTeam const tm{};  // (the caller has checked k)
        for(int q = 0; q < V.batch; ++q) pz_orth(tm, V, Z, q, k, zeros);
        return hipSuccess;
    }
    hipError_t launch_pz_ritz(hipStream_t, PzRitzView const& R)
    {
        std::vector<double> lds(static_cast<size_t>(pz_ritz_doubles(R.m)));
        for(int i = 0; i < R.n_mats; ++i) pz_ritz(PzSerialWave{}, R, i, lds.data());  // (both callers have checked R.m)
        return hipSuccess;
    }
}  // namespace pe
#endif
