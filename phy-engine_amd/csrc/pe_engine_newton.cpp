// pe_engine_newton.cpp -- the host-driven schedule: Newton and transient loops of circult::solve / analyze (circuit.h:892-985, 233-256)
// over the per-phase kernels of the split schedule, the host-stamp overlay callbacks, the residual safety net of the static-pivot LU,
// and the two analysis entry points pe_hip_analyze_tr / pe_hip_analyze_dc (resident kernel or split schedule).
#include "pe_engine_internal.hpp"

using namespace pe_eng;

namespace pe_eng PE_ENG_HIDDEN
{
    // host-stamp overlay: one callback (+ the upload of its values for ITERATE) on the current x of instance b.  In a batch the
    // callback is told first which instance the calls that follow concern (PE_HIP_OVERLAY_INSTANCE): models with state of their own
    // (a junction's last voltage, a companion history) keep one copy per instance.
    int overlay_call(pe_hip_engine* h, int event, int mode, double t, double dt, int b)
    {
        auto const& hc = h->hc;
        h->ov_x.resize(static_cast<size_t>(hc.rows));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if(hc.batch > 1 && h->overlay_fn(h->overlay_user, PE_HIP_OVERLAY_INSTANCE, b, t, dt, nullptr, nullptr, nullptr) != 0)
            return fail(h, PE_HIP_ERR_INTERNAL, "host-stamp overlay: the callback refused PE_HIP_OVERLAY_INSTANCE (it does not support batches)");
        if(hc.rows) HIPCHK(h, hipMemcpy(h->ov_x.data(), h->V.x + static_cast<size_t>(b) * hc.rows, static_cast<size_t>(hc.rows) * sizeof(double), hipMemcpyDeviceToHost));
        bool const iter = event == PE_HIP_OVERLAY_ITERATE;
        h->ov_a.assign(static_cast<size_t>(hc.n_ov_a), 0.0);
        h->ov_b.assign(static_cast<size_t>(hc.n_ov_b), 0.0);
        int const orc = h->overlay_fn(h->overlay_user, event, mode, t, dt, h->ov_x.data(), iter ? h->ov_a.data() : nullptr, iter ? h->ov_b.data() : nullptr);
        if(event == PE_HIP_OVERLAY_CONVERGED && orc == PE_HIP_OVERLAY_VETO) return PE_HIP_OVERLAY_VETO;  // (positive: not a pe_hip_status)
        if(orc != 0) return fail(h, PE_HIP_ERR_INTERNAL, "host-stamp overlay: a model hook failed");
        if(iter)
        {
            double* dv = h->V.dv + static_cast<size_t>(b) * h->V.dv_len;
            if(hc.n_ov_a) HIPCHK(h, hipMemcpy(dv + hc.dv_ova, h->ov_a.data(), static_cast<size_t>(hc.n_ov_a) * sizeof(double), hipMemcpyHostToDevice));
            if(hc.n_ov_b) HIPCHK(h, hipMemcpy(dv + hc.dv_ovb, h->ov_b.data(), static_cast<size_t>(hc.n_ov_b) * sizeof(double), hipMemcpyHostToDevice));
        }
        return PE_HIP_OK;
    }
    // the same for every instance of `mask` (null: all)
    int overlay_call_all(pe_hip_engine* h, int event, int mode, double t, double dt, std::vector<int> const* mask)
    {
        for(int b = 0; b < h->hc.batch; ++b)
            if(!mask || (*mask)[b])
                if(int const rc = overlay_call(h, event, mode, t, dt, b); rc != PE_HIP_OK) return rc;
        return PE_HIP_OK;
    }
    bool has_overlay(pe_hip_engine const* h) { return h->overlay_fn && (h->hc.n_ov_a || h->hc.n_ov_b); }

    // ---------------- multi-workgroup mode: the Newton / TR loops of circult::solve / analyze (circuit.h:892-985, 233-256)
    // driven from the host, one kernel sequence per Newton iteration (pe_kernels.hip: launch_m2_iteration)
    struct M2State
    {
        std::vector<int> status, active, flags;
        std::vector<long long> steps, iters;
        std::vector<double> t;
        std::vector<int> trace;
    };

    int m2_pull(pe_hip_engine* h, M2State& S)
    {
        int const B = h->hc.batch;
        S.status.resize(B);
        S.active.assign(B, 0);
        S.flags.assign(B, 0);
        S.steps.resize(B);
        S.iters.resize(B);
        S.t.resize(B);
        HIPCHK(h, hipMemcpy(S.status.data(), h->V.status, B * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(S.steps.data(), h->V.n_steps, B * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(S.iters.data(), h->V.n_iters, B * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(S.t.data(), h->V.t_now, B * sizeof(double), hipMemcpyDeviceToHost));
        return PE_HIP_OK;
    }

    int m2_push(pe_hip_engine* h, M2State const& S, double last_step, bool write_last_step)
    {
        int const B = h->hc.batch;
        HIPCHK(h, hipMemcpy(h->V.status, S.status.data(), B * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->V.n_steps, S.steps.data(), B * sizeof(long long), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->V.n_iters, S.iters.data(), B * sizeof(long long), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->V.t_now, S.t.data(), B * sizeof(double), hipMemcpyHostToDevice));
        if(write_last_step)
        {
            std::vector<double> ls(B, last_step);
            HIPCHK(h, hipMemcpy(h->V.last_step, ls.data(), B * sizeof(double), hipMemcpyHostToDevice));
        }
        if(!S.trace.empty())
        {
            int len = 0;
            HIPCHK(h, hipMemcpy(&len, h->V.trace_len, sizeof(int), hipMemcpyDeviceToHost));
            int const room = std::max(0, h->V.trace_cap - len);
            int const n = std::min<int>(room, static_cast<int>(S.trace.size()));
            if(n > 0) HIPCHK(h, hipMemcpy(h->V.trace + len, S.trace.data(), n * sizeof(int), hipMemcpyHostToDevice));
            len += static_cast<int>(S.trace.size());
            HIPCHK(h, hipMemcpy(h->V.trace_len, &len, sizeof(int), hipMemcpyHostToDevice));
        }
        return PE_HIP_OK;
    }

    int ensure_pinned(pe_hip_engine* h, size_t n)
    {
        HIPCHK(h, h->pin_active.ensure_at_least(n));
        HIPCHK(h, h->pin_flags.ensure_at_least(n));
        return PE_HIP_OK;
    }
    // `active` mask of the next launches (stream-ordered).  The caller synchronises the stream before it changes the mask again,
    // so the one pinned staging buffer is free by then.
    // Quad mode: the active instances, ascending, are packed four to a wavefront of the lane-group kernel (pe_quad.hpp) -- behind the
    // mask in the same buffer / the same copy.  A quad addresses its members by 32-bit byte offsets from its first one, so it only
    // takes instances inside that window (a sparse tail of a sweep gives short quads, padded with -1).
    int upload_active(pe_hip_engine* h, std::vector<int> const& mask)
    {
        if(h->resident.active_dev == mask) return PE_HIP_OK;
        size_t const B = mask.size();
        if(int const rc = ensure_pinned(h, 5 * B); rc != PE_HIP_OK) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));  // (an earlier upload from the staging buffer may still be in flight)
        std::copy(mask.begin(), mask.end(), h->pin_active.data());
        size_t words = B;
        if(h->V.quad)
        {
            long long const stride = 8 * std::max({static_cast<long long>(h->V.nnzA), h->V.factor_doubles, h->V.arena_doubles, static_cast<long long>(h->V.rows)});
            long long const span = std::max<long long>(0, ((1ll << 32) - 1) / std::max<long long>(stride, 1) - 2);
            int* ql = h->pin_active.data() + B;
            int nq = 0, cnt = 0, first = 0;
            for(size_t b = 0; b < B; ++b)
            {
                if(!mask[b]) continue;
                if(cnt == 0 || cnt == 4 || static_cast<long long>(b) - first > span)
                {
                    for(; cnt > 0 && cnt < 4; ++cnt) ql[4 * (nq - 1) + cnt] = -1;
                    ++nq;
                    cnt = 0;
                    first = static_cast<int>(b);
                }
                ql[4 * (nq - 1) + cnt++] = static_cast<int>(b);
            }
            for(; cnt > 0 && cnt < 4; ++cnt) ql[4 * (nq - 1) + cnt] = -1;
            // captured launch sequences (m2_point: graph mode) keep ONE grid: the quads of the full sweep, the ones behind the active
            // instances empty (the lane-group kernels return on a first member < 0)
            if(h->graph_mode)
                for(int const nq_all = static_cast<int>((B + 3) / 4); nq < nq_all; ++nq)
                    for(int c = 0; c < 4; ++c) ql[4 * nq + c] = -1;
            h->V.n_quads = nq;
            h->V.q_list = h->V.active + B;
            words = B + 4 * static_cast<size_t>(nq);
        }
        HIPCHK(h, hipMemcpyAsync(h->V.active, h->pin_active.data(), words * sizeof(int), hipMemcpyHostToDevice, h->stream));
        h->resident.active_dev = mask;
        return PE_HIP_OK;
    }
    int download_flags(pe_hip_engine* h, std::vector<int>& flags)
    {
        if(int const rc = ensure_pinned(h, flags.size()); rc != PE_HIP_OK) return rc;
        HIPCHK(h, hipMemcpyAsync(h->pin_flags.data(), h->V.flags, flags.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::copy(h->pin_flags.data(), h->pin_flags.data() + flags.size(), flags.begin());
        return PE_HIP_OK;
    }

    // The same without a copy command: the iteration's last launch (k_m2_publish) writes flags + residual norms into pinned host memory
    // and then a sequence number; the host polls that word.  Falls back to the stream's completion if the word does not arrive (a failed
    // launch): the caller then sees the error of the synchronisation.
    struct Published
    {
        unsigned long long* seq;
        int* flags;
        double* eta;
    };
    Published pub_view(void* base, size_t B)
    {
        auto* p = static_cast<char*>(base);
        return {reinterpret_cast<unsigned long long*>(p), reinterpret_cast<int*>(p + 64), reinterpret_cast<double*>(p + 64 + ((B * sizeof(int) + 63) / 64) * 64)};
    }
    int ensure_published(pe_hip_engine* h, size_t B)
    {
        size_t const need = 64 + ((B * sizeof(int) + 63) / 64) * 64 + 4 * B * sizeof(double);
        if(h->pub.capacity() >= need && h->pub.data()) return PE_HIP_OK;
        // (coherent + mapped, explicitly: the device's system-scope release of the sequence word must reach the polling host even where
        //  HIP_HOST_COHERENT=0 makes default pinned allocations non-coherent)
        HIPCHK(h, h->pub.ensure_at_least(need, hipHostMallocCoherent | hipHostMallocMapped));
        std::memset(h->pub.data(), 0, need);
        return PE_HIP_OK;
    }
    // waits for the publication with sequence number `seq` (launched by the caller: launch_m2_publish, or the last node of a captured
    // iteration); `eta` (4 doubles per instance) may be null
    int wait_published(pe_hip_engine* h, std::vector<int>& flags, std::vector<double>* eta, unsigned long long seq)
    {
        size_t const B = flags.size();
        auto const host = pub_view(h->pub.data(), B);
        for(unsigned spins = 0; __atomic_load_n(host.seq, __ATOMIC_ACQUIRE) != seq; ++spins)
        {
            if((spins & 1023u) == 1023u)
            {
                hipError_t const q = hipStreamQuery(h->stream);
                if(q == hipSuccess)
                {
                    if(__atomic_load_n(host.seq, __ATOMIC_ACQUIRE) == seq) break;
                    return fail(h, PE_HIP_ERR_INTERNAL, "the iteration's results were not published (k_m2_publish did not run)");
                }
                if(q != hipErrorNotReady) HIPCHK(h, q);
                if(spins > (1u << 16)) std::this_thread::yield();  // (a long iteration of a large sweep: leave the core to others)
            }
        }
        std::copy(host.flags, host.flags + B, flags.begin());
        if(eta && h->V.residual_tol > 0.0) eta->assign(host.eta, host.eta + 4 * B);
        return PE_HIP_OK;
    }
    // launches the publication of the iteration just enqueued and waits for it
    int publish_and_wait(pe_hip_engine* h, std::vector<int>& flags, std::vector<double>* eta)
    {
        size_t const B = flags.size();
        if(int const rc = ensure_published(h, B); rc != PE_HIP_OK) return rc;
        auto const dev = pub_view(h->pub.device(), B);
        unsigned long long const seq = ++h->pub_seq;
        HIPCHK(h, pe::launch_m2_publish(h->stream, h->V, dev.flags, dev.eta, dev.seq, seq));
        return wait_published(h, flags, eta, seq);
    }

    // Residual safety net on the host-driven schedule.  The iteration just launched left the four norms of every active instance's
    // solve in eta_acc.  Instances above the tolerance get up to two rounds of iterative refinement (launch_m2_refine: active =
    // exactly those); their flags are then the Newton / finiteness bits of the corrected x.  What refinement cannot repair leaves
    // the iteration as PE_HIP_ERR_INACCURATE (the caller re-matches on that instance's values and retries the step).
    // `published`: the norms of this iteration as k_m2_publish handed them over (empty: read them from the device)
    // `owes`: instances whose solve needed a refinement earlier at this solve point.  Where the corrected x then violated the Newton test,
    // the iterates that follow come from the same pivot order and are as inaccurate as the flagged one -- but an iterate that violates
    // is not checked, and its step back from the corrected x is the size of the correction: the violation would repeat until max_newton
    // runs out.  So every further solve of such an instance is refined before its Newton bits count.
    int m2_check_residuals(pe_hip_engine* h, M2State& S, std::vector<int>& result, int& n_active, std::vector<double> const& published,
                           std::vector<char>& owes)
    {
        int const B = h->hc.batch;
        std::vector<double> eta(static_cast<size_t>(B) * 4);
        bool first = published.size() == eta.size();
        auto pull_eta = [&]() -> int
        {
            if(first)  // (the iteration's own norms came with its flags; later calls follow a refinement launch)
            {
                eta = published;
                first = false;
                return PE_HIP_OK;
            }
            HIPCHK(h, hipMemcpy(eta.data(), h->V.eta_acc, eta.size() * sizeof(double), hipMemcpyDeviceToHost));
            return PE_HIP_OK;
        };
        auto bad = [&](int b)
        {
            double const* n = &eta[4 * static_cast<size_t>(b)];
            double const den = n[1] * n[2] + n[3];
            double const e = den > 0.0 ? n[0] / den : (n[0] > 0.0 ? INFINITY : 0.0);
            return !(e <= h->V.residual_tol);
        };
        // only iterates about to be accepted were checked on the device (k_m2_residual): nothing to read while every active instance
        // still shows a Newton violation
        auto checked = [&](int b) { return S.active[b] && !(S.flags[b] & 5) && !(h->hc.nonlinear && (S.flags[b] & 2)); };
        auto owed = [&](int b) { return S.active[b] && !(S.flags[b] & 5) && h->hc.nonlinear && (S.flags[b] & 2) && owes[static_cast<size_t>(b)]; };
        bool any = false;
        for(int b = 0; b < B && !any; ++b) any = checked(b) || owed(b);
        if(!any) return PE_HIP_OK;
        if(int const rc = pull_eta(); rc != PE_HIP_OK) return rc;
        std::vector<int> todo;
        for(int b = 0; b < B; ++b)
            if((checked(b) && bad(b)) || owed(b)) todo.push_back(b);
        if(todo.empty()) return PE_HIP_OK;
        for(int b: todo) owes[static_cast<size_t>(b)] = 1;
        std::vector<int> mask(B);
        for(int round = 0; round < 2 && !todo.empty(); ++round)
        {
            std::fill(mask.begin(), mask.end(), 0);
            for(int b: todo) mask[b] = 1;
            if(int const urc = upload_active(h, mask); urc != PE_HIP_OK) return urc;
            HIPCHK(h, pe::launch_m2_refine(h->stream, h->V));
            // (a refactorisation with the residual riding along: the update vectors of the static roots and the kept forward-substituted
            //  pivots no longer belong to this point's right-hand side -- no later iteration of the point may skip the static fronts)
            h->refined_in_point = true;
            if(h->V.quad && h->V.n_quads > 0) ++h->resident.quad_full_launches;
            HIPCHK(h, hipStreamSynchronize(h->stream));
            if(int const rc = pull_eta(); rc != PE_HIP_OK) return rc;
            std::vector<int> fl(B);
            HIPCHK(h, hipMemcpy(fl.data(), h->V.flags, B * sizeof(int), hipMemcpyDeviceToHost));
            std::vector<int> still;
            for(int b: todo)
            {
                S.flags[b] = fl[b];
                if((fl[b] & 5) == 0 && bad(b)) still.push_back(b);
                else
                    ++h->resident.n_refined;
            }
            todo.swap(still);
        }
        for(int b: todo)
        {
            result[b] = PE_HIP_ERR_INACCURATE;
            S.active[b] = 0;
            --n_active;
        }
        return PE_HIP_OK;
    }

    // one solve point of every instance whose status is OK; result[b] = iterations (> 0) or a negative status
    // companion_dt != null: a transient step -- its companion update rides in the first iteration's evaluation launch (k_m2_eval)
    // a_static_ok: the non-x-dependent part of every active instance's matrix already holds the stamp of this (mode, dt) -- the first iteration
    // stamps the x-dependent slots + the whole right-hand side only (stamp mode 2)
    int m2_point(pe_hip_engine* h, M2State& S, int mode, double t, double last_step, bool do_factor, std::vector<int>& result, int& launches,
                 double const* companion_dt = nullptr, bool a_static_ok = false)
    {
        int const B = h->hc.batch;
        result.assign(B, 0);
        int n_active = 0;
        for(int b = 0; b < B; ++b)
        {
            S.active[b] = S.status[b] == PE_HIP_OK ? 1 : 0;
            n_active += S.active[b];
        }
        int const max_it = h->hc.nonlinear ? h->V.max_newton : 1;
        std::vector<char> owes_refinement(static_cast<size_t>(B), 0);  // (m2_check_residuals)
        // Small sweeps replay a captured launch sequence per iteration (pe_kernels.hip launch_m2_iteration_graph): the 15-20 launches of an
        // iteration cost more host time than some of them run.  Large sweeps keep the plain launches -- their iteration is milliseconds,
        // and the HIP events around the dominant pair (bench.py's roofline) live there.  Knob GRAPH = 0 / 1 forces either.
        static bool const use_publish = env_int0("PHY_ENGINE_HIP_PUBLISH", 1) != 0;
        // (measured, profiles/r04_ab_runs.log: -3.3 % per iteration for the single circuit, -0.8 % at 16 instances, nothing from 128 on --
        //  there the kernels are long enough for the host to stay ahead of the stream)
        bool const graph_mode = use_publish && knob(h, "GRAPH", B <= 32 ? 1 : 0) != 0;
        if(graph_mode != h->graph_mode)
        {
            h->graph_mode = graph_mode;
            h->resident.active_dev.clear();  // (the quad list behind the mask is laid out differently)
        }
        if(graph_mode && !h->graphs) h->graphs.reset(pe::m2_graphs_create());
        // Static fronts of the lane-group kernel: the iterations after the first of this point skip them -- unless anything but the
        // x-dependent stamp may have touched the matrix, the right-hand side or what the first iteration left behind.  Knob STATIC_SKIP = 0: never.
        h->refined_in_point = false;
        bool const may_skip_static = h->resident.static_skip.q_prog_dyn && h->hc.nonlinear && do_factor && !has_overlay(h) && h->V.quad && h->V.n_mid == 0 &&
                                     h->V.q_lds_stride == 0 && h->V.dyn_a && h->V.dyn_b && knob(h, "STATIC_SKIP", 1) != 0;
        for(int it = 0; it < max_it && n_active > 0; ++it)
        {
            if(has_overlay(h))
                if(int const rc = overlay_call_all(h, PE_HIP_OVERLAY_ITERATE, mode, t, last_step, &S.active); rc != PE_HIP_OK) return rc;
            if(int const urc = upload_active(h, S.active); urc != PE_HIP_OK) return urc;
            // (test knob PHY_ENGINE_HIP_FULL_STAMP=1: every iteration stamps everything -- the x-dependent-only path must match it bit for bit)
            static bool const full_stamp = env_int0("PHY_ENGINE_HIP_FULL_STAMP", 0) != 0;
            int const dyn = full_stamp ? 0 : (it > 0 ? 1 : (a_static_ok ? 2 : 0));
            bool const comp = it == 0 && companion_dt != nullptr;
            pe::StaticSkip sk = h->resident.static_skip;
            sk.save = (may_skip_static && !full_stamp && it == 0) ? 1 : 0;
            sk.skip = (may_skip_static && !full_stamp && it > 0 && dyn == 1 && !h->refined_in_point) ? 1 : 0;
            if(do_factor && h->V.quad && h->V.n_quads > 0)
            {
                ++(sk.skip ? h->resident.quad_skipped_launches : h->resident.quad_full_launches);
                if(it > 0 && h->refined_in_point)  // (counted whatever the knob says: the second must stay 0)
                {
                    ++h->resident.quad_launches_after_refinement;
                    if(sk.skip) ++h->resident.quad_skipped_after_refinement;
                }
            }
            std::vector<double> eta_now;
            if(graph_mode)
            {
                if(int const prc = ensure_published(h, static_cast<size_t>(B)); prc != PE_HIP_OK) return prc;
                auto const dev = pub_view(h->pub.device(), static_cast<size_t>(B));
                unsigned long long const seq = ++h->pub_seq;
                HIPCHK(h, pe::launch_m2_iteration_graph_static(h->stream, h->graphs.get(), h->V, mode, t, last_step, do_factor, dyn, comp, companion_dt ? *companion_dt : 0.0,
                                                               dev.flags, dev.eta, dev.seq, seq, sk));
                ++launches;
                if(int const prc = wait_published(h, S.flags, &eta_now, seq); prc != PE_HIP_OK) return prc;
            }
            else
            {
                HIPCHK(h, pe::launch_m2_iteration_static(h->stream, h->V, mode, t, last_step, do_factor, h->evk0, h->evk1, /*stamp_mode=*/dyn, /*companion=*/comp,
                                                         companion_dt ? *companion_dt : 0.0, sk));
                ++launches;
                // flags + residual norms of this iteration: published into pinned host memory by the iteration's last launch and polled
                // (no copy command, no stream synchronisation); PHY_ENGINE_HIP_PUBLISH=0: the copy + synchronise of rounds 1-2
                if(use_publish)
                {
                    if(int const prc = publish_and_wait(h, S.flags, &eta_now); prc != PE_HIP_OK) return prc;
                }
                else if(int const drc = download_flags(h, S.flags); drc != PE_HIP_OK)
                    return drc;  // (synchronises the stream)
                float kms = 0.f;
                if(hipEventElapsedTime(&kms, h->evk0, h->evk1) == hipSuccess)
                {
                    h->dominant_ms += kms;
                    ++h->dominant_launches;
                }
            }
            if(h->V.residual_tol > 0.0)
                if(int const rrc = m2_check_residuals(h, S, result, n_active, eta_now, owes_refinement); rrc != PE_HIP_OK) return rrc;
            for(int b = 0; b < B; ++b)
            {
                if(!S.active[b]) continue;
                int const f = S.flags[b];
                if(f & 8) return fail(h, PE_HIP_ERR_INTERNAL, "a front's LDS layout exceeds the LDS of the launch that ran it (launch plan / layout mismatch)");
                if(f & 5) result[b] = PE_HIP_ERR_SINGULAR;
                else if(!h->hc.nonlinear || !(f & 2))
                {
                    // circuit.h:950-963: an iterate that passed the Newton test is still subject to the models' check_convergence
                    // hooks -- host-stamped models only (the built-in ones have none); a veto costs one more iteration
                    if(has_overlay(h) && h->hc.nonlinear)
                    {
                        int const crc = overlay_call(h, PE_HIP_OVERLAY_CONVERGED, mode, t, last_step, b);
                        if(crc == PE_HIP_OVERLAY_VETO) continue;
                        if(crc != PE_HIP_OK) return crc;
                    }
                    result[b] = it + 1;
                }
                else
                    continue;
                S.active[b] = 0;
                --n_active;
            }
        }
        for(int b = 0; b < B; ++b)
            if(S.active[b])
            {
                result[b] = PE_HIP_ERR_NO_CONVERGENCE;
                S.active[b] = 0;
            }
        return PE_HIP_OK;
    }

    // `only` != null: a retry of exactly those instances after a rolled-back step -- the companion update of that step has already
    // been applied (update_tr_step precedes the failing solve, circuit.h:246-248), so the first step of the retry skips it
    // `retry`: the first step's companion update has already been applied (see above); false for a plain subset of the instances
    int run_m2_tr(pe_hip_engine* h, double dt, int nsteps, int& launches, std::vector<int> const* only = nullptr, bool retry = true)
    {
        M2State S;
        int rc = m2_pull(h, S);
        if(rc != PE_HIP_OK) return rc;
        int const B = h->hc.batch;
        if(!only)
        {
            // The batch is solved in lockstep at ONE time point per launch sequence (sources are evaluated at that t).  Instances that
            // sit at different time points -- one failed and was rolled back in an earlier call while the others went on -- are
            // therefore run group by group, each at its own t (a revived instance must not be solved at the group's time).
            std::vector<double> ts;
            for(int b = 0; b < B; ++b)
                if(S.status[b] == PE_HIP_OK && std::find(ts.begin(), ts.end(), S.t[b]) == ts.end()) ts.push_back(S.t[b]);
            if(ts.size() > 1)
            {
                for(double const tg: ts)
                {
                    std::vector<int> mask(B, 0);
                    for(int b = 0; b < B; ++b) mask[b] = (S.status[b] == PE_HIP_OK && S.t[b] == tg) ? 1 : 0;
                    if(int const grc = run_m2_tr(h, dt, nsteps, launches, &mask, false); grc != PE_HIP_OK) return grc;
                }
                return PE_HIP_OK;
            }
        }
        bool const skip_first = only && retry;
        bool const may_reuse = !h->hc.nonlinear && !h->opt.refactor_every_solve && !has_overlay(h);  // (overlay values may change every solve)
        std::vector<int> res, accepted;
        for(int s = 0; s < nsteps; ++s)
        {
            int alive = 0;
            for(int b = 0; b < B; ++b)
            {
                S.active[b] = (S.status[b] == PE_HIP_OK && (!only || (*only)[b])) ? 1 : 0;
                alive += S.active[b];
            }
            if(!alive) break;
            if(only)  // (a retry of some instances: the others must not be touched by m2_point either)
                for(int b = 0; b < B; ++b)
                    if(!(*only)[b] && S.status[b] == PE_HIP_OK) S.status[b] = -1000;
            if(has_overlay(h) && !(skip_first && s == 0))
                if(int const orc = overlay_call_all(h, PE_HIP_OVERLAY_STEP, PE_HIP_MODE_TR, S.t[0], dt, &S.active); orc != PE_HIP_OK) return orc;
            if(int const urc = upload_active(h, S.active); urc != PE_HIP_OK) return urc;
            // (the companion update of this step runs inside the first iteration's evaluation launch: m2_point / k_m2_eval -- one launch
            //  less per step; knob COMPANION_LAUNCH=1 keeps it a launch of its own)
            bool const with_companion = !(skip_first && s == 0);
            static bool const own_launch = env_int0("PHY_ENGINE_HIP_COMPANION_LAUNCH", 0) != 0;
            if(with_companion && own_launch) HIPCHK(h, pe::launch_m2_companion(h->stream, h->V, dt));
            // every live instance sits at the same time point (same dt, lockstep); take it from the first live one
            double t_prev = 0.0;
            for(int b = 0; b < B; ++b)
                if(S.active[b])
                {
                    t_prev = S.t[b];
                    break;
                }
            double const t = t_prev + dt;
            // linear circuit, same dt as the last factorisation: stamp + triangular solves only
            // (what the companion conductances of this step are a function of: dt under the trapezoidal rule, a0 under BE / GEAR2 -- a GEAR2 step after
            //  a restart has a0 = 1 / h, the following ones 3 / (2 h) at the same dt; NaN, equal to nothing, where the instances may differ)
            double const key = integ_key(h, dt);
            bool const reuse = may_reuse && h->resident.fact_valid && h->fact_dt == key;
            // The matrix of a transient step differs from the last step's only in its x-dependent slots while dt and the parameters stay (the
            // companion conductances 2C/dt, 2L/dt are constants of the step size): instances whose matrix holds a full stamp of this dt skip the
            // other 97 % of the matrix gather on the first iteration too (k_m2_stamp 0.56 -> 0.2 ms per time point at 1 024 instances).  The
            // set is cleared wherever a static value can change (invalidate_factors: parameters, options, load, checkpoint, re-analysis,
            // any OP / DC / TROP solve -- they stamp other companions); knob STATIC_A=0: always the full stamp.
            static bool const static_a = env_int0("PHY_ENGINE_HIP_STATIC_A", 1) != 0;
            bool a_static_ok = static_a && h->a_static_dt == key && h->resident.a_static.size() == static_cast<size_t>(B);
            for(int b = 0; b < B && a_static_ok; ++b)
                if(S.active[b] && !h->resident.a_static[static_cast<size_t>(b)]) a_static_ok = false;
            rc = m2_point(h, S, PE_HIP_MODE_TR, t, dt, !reuse, res, launches, (with_companion && !own_launch) ? &dt : nullptr, a_static_ok);
            if(rc == PE_HIP_OK && !a_static_ok)
            {
                // the first iteration of this step stamped everything for the instances that were active at its start (S.active is spent by now:
                // the mask of the step is status OK && (!only || only[b]) -- recomputed)
                if(h->a_static_dt != key || h->resident.a_static.size() != static_cast<size_t>(B)) h->resident.a_static.assign(static_cast<size_t>(B), 0);
                h->a_static_dt = key;
                for(int b = 0; b < B; ++b)
                    if(res[b] != 0) h->resident.a_static[static_cast<size_t>(b)] = 1;  // (res != 0: the instance took part in this point)
            }
            if(rc != PE_HIP_OK) return rc;
            if(may_reuse)
            {
                h->resident.fact_valid = true;
                h->fact_dt = key;
            }
            if(h->tr_method != PE_HIP_TR_TRAP)
            {
                // every instance took this step and holds h_p = dt now, or the host no longer knows one h_p for all of them
                bool all = !only;
                for(int b = 0; b < B && all; ++b) all = S.status[b] == PE_HIP_OK && res[b] > 0;
                h->resident.integ_hp = all ? dt : std::nan("");
            }
            if(h->probe.armed) accepted.assign(B, 0);
            for(int b = 0; b < B; ++b)
            {
                if(S.status[b] != PE_HIP_OK || res[b] == 0) continue;
                if(b == 0) S.trace.push_back(res[b]);
                if(res[b] < 0) S.status[b] = res[b];  // the failing step is rolled back: t stays at t_prev (circuit.h:249-253)
                else
                {
                    S.t[b] = t;
                    ++S.steps[b];
                    S.iters[b] += res[b];
                    if(h->probe.armed) accepted[b] = 1;
                }
            }
            // transient probes: only the host knows which instances' steps were accepted (residual check, overlay veto)
            if(h->probe.armed)
                if(int const prc = probe_record_step(h, accepted, t); prc != PE_HIP_OK) return prc;
        }
        for(int b = 0; b < B; ++b)
            if(S.status[b] == -1000) S.status[b] = PE_HIP_OK;
        return m2_push(h, S, dt, true);
    }

    // do_factor = false: the factors of the last factorisation are kept (dc_solve_kept: a linear engine with unchanged matrix values)
    int run_m2_dc(pe_hip_engine* h, int mode, int& launches, std::vector<int> const* only = nullptr, bool do_factor = true)
    {
        M2State S;
        int rc = m2_pull(h, S);
        if(rc != PE_HIP_OK) return rc;
        int const B = h->hc.batch;
        if(only)
            for(int b = 0; b < B; ++b)
                if(!(*only)[b] && S.status[b] == PE_HIP_OK) S.status[b] = -1000;
        std::vector<double> ls(B);
        HIPCHK(h, hipMemcpy(ls.data(), h->V.last_step, B * sizeof(double), hipMemcpyDeviceToHost));
        std::vector<int> res;
        h->resident.a_static.clear();  // (an OP / DC / TROP stamp overwrites the transient companions in the matrix)
        rc = m2_point(h, S, mode, S.t[0], ls[0], do_factor, res, launches);
        if(rc != PE_HIP_OK) return rc;
        for(int b = 0; b < B; ++b)
        {
            if(S.status[b] != PE_HIP_OK || res[b] == 0) continue;
            if(b == 0) S.trace.push_back(res[b]);
            if(res[b] < 0) S.status[b] = res[b];
            else
                S.iters[b] += res[b];
        }
        for(int b = 0; b < B; ++b)
            if(S.status[b] == -1000) S.status[b] = PE_HIP_OK;
        return m2_push(h, S, 0.0, false);
    }

    // Residual safety net, last resort: instances whose solve stayed inaccurate (status PE_HIP_ERR_INACCURATE, step rolled back).
    // First time: leave the resident kernel for the host-driven schedule, which refines.  After that: a new static pivot order
    // from the values of the first failing instance (the order of load time came from instance 0 at the first dt).  Returns the
    // instances to retry (status cleared) grouped by the steps they still owe, or an empty list when nothing more can be done.
    int prepare_inaccurate_retry(pe_hip_engine* h, bool tr, double dt, int attempt, std::vector<long long> const& steps0, int nsteps,
                                 std::vector<std::pair<int, std::vector<int>>>& groups)
    {
        groups.clear();
        int const B = h->hc.batch;
        std::vector<int> status(B);
        std::vector<long long> s1(B);
        HIPCHK(h, hipMemcpy(status.data(), h->V.status, B * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(s1.data(), h->V.n_steps, B * sizeof(long long), hipMemcpyDeviceToHost));
        // a zero / non-finite pivot under the order matched at load time gets ONE re-match on the instance's own values too (a switch
        // toggled through update_param, a parameter that moved by orders of magnitude): the reference would simply pivot elsewhere
        std::vector<int> failed;
        bool any_inaccurate = false;
        for(int b = 0; b < B; ++b)
            if(status[b] == PE_HIP_ERR_INACCURATE || (status[b] == PE_HIP_ERR_SINGULAR && !h->resident.singular_rematched))
            {
                failed.push_back(b);
                any_inaccurate = any_inaccurate || status[b] == PE_HIP_ERR_INACCURATE;
            }
        if(failed.empty() || attempt >= 2) return PE_HIP_OK;
        if(!any_inaccurate) h->resident.singular_rematched = true;  // (once per resident circuit: a structurally singular system stays singular)
        // (knob SPLIT = 0 keeps the first attempt of every call on the resident kernel, which only detects: the first retry of such a call
        //  is the one that refines, whether an earlier call had tripped the net already or not)
        if(any_inaccurate && attempt == 0 && (!h->resident.careful || !split_launch(h))) h->resident.careful = true;
        else
        {
            // re-match on the failing instance's own assembled values (device order = front-assembly order -> CSR slots)
            int const b = failed[0];
            size_t const nnz = h->hc.ci.size();
            std::vector<double> tmp(nnz);
            HIPCHK(h, hipMemcpy(tmp.data(), h->V.aval + static_cast<size_t>(b) * nnz, nnz * sizeof(double), hipMemcpyDeviceToHost));
            h->sym_values_override.assign(nnz, 0.0);
            for(size_t e = 0; e < nnz; ++e)
            {
                double const v = std::fabs(tmp[e]);
                h->sym_values_override[h->sym.asm_slot[e]] = v <= 1.7976931348623157e308 ? v : 1.0;  // (a non-finite entry says nothing about magnitude)
            }
            h->resident.sym_class = -1;
            int const rc = ensure_symbolic(h, tr, dt);
            h->sym_values_override.clear();
            if(rc != PE_HIP_OK) return rc;
            ++h->resident.n_rematched;
        }
        for(int b: failed) status[b] = PE_HIP_OK;
        HIPCHK(h, hipMemcpy(h->V.status, status.data(), B * sizeof(int), hipMemcpyHostToDevice));
        for(int b: failed)
        {
            int const owe = tr ? nsteps - static_cast<int>(s1[b] - steps0[b]) : 1;
            auto it = std::find_if(groups.begin(), groups.end(), [&](auto const& g) { return g.first == owe; });
            if(it == groups.end())
            {
                groups.emplace_back(owe, std::vector<int>(B, 0));
                it = groups.end() - 1;
            }
            it->second[b] = 1;
        }
        return PE_HIP_OK;
    }
}  // namespace pe_eng

#if !defined(__HIPCC__)
// Builds without HIP (the emulation library of tests/emu, which compiles the engine's translation units with a host compiler): the probe
// launchers as serial loops over the instances, with a one-thread team
    #include "pe_probe.hpp"
namespace pe
{
    namespace
    {
        struct ProbeHostTeam
        {
            int tid() const { return 0; }
            int size() const { return 1; }
            void sync() const {}
        };
    }  // namespace
    // the iteration with the static fronts of the lane-group kernel kept / skipped: the emulation's launcher runs the whole iteration from the
    // view alone, so the tables reach the code it walks through pe::host_static_skip (pe_device.hpp) -- under m2_sequence's own conditions
    namespace
    {
        struct HostStaticSkip
        {
            StaticSkip eff;
            HostStaticSkip(DevView const& V, bool do_factor, int stamp_mode, StaticSkip const& sk) : eff(static_skip_effective(V, do_factor, stamp_mode, false, &sk))
            {
                host_static_skip = (eff.skip || eff.save) ? &eff : nullptr;
            }
            ~HostStaticSkip() { host_static_skip = nullptr; }
        };
    }  // namespace
    hipError_t launch_m2_iteration_static(hipStream_t st, DevView const& V, int mode, double t, double last_step, bool do_factor, hipEvent_t ev0, hipEvent_t ev1,
                                          int stamp_mode, bool companion, double companion_dt, StaticSkip const& sk)
    {
        HostStaticSkip const scope(V, do_factor, stamp_mode, sk);
        return launch_m2_iteration(st, V, mode, t, last_step, do_factor, ev0, ev1, stamp_mode, companion, companion_dt);
    }
    hipError_t launch_m2_iteration_graph_static(hipStream_t st, M2GraphCache* cache, DevView const& V, int mode, double t, double last_step, bool do_factor,
                                                int stamp_mode, bool companion, double companion_dt, int* pub_flags, double* pub_eta, unsigned long long* pub_seq,
                                                unsigned long long seq, StaticSkip const& sk)
    {
        HostStaticSkip const scope(V, do_factor, stamp_mode, sk);
        return launch_m2_iteration_graph(st, cache, V, mode, t, last_step, do_factor, stamp_mode, companion, companion_dt, pub_flags, pub_eta, pub_seq, seq);
    }
    hipError_t launch_probe_arm(hipStream_t, ProbedView const& V)
    {
        for(int b = 0; b < V.batch; ++b)
        {
            probe_arm(ProbeHostTeam{}, V, b);
            if(V.fo) fourier_arm(ProbeHostTeam{}, V, b);
        }
        return hipSuccess;
    }
    hipError_t launch_probe_record(hipStream_t, ProbedView const& V, double t)
    {
        for(int b = 0; b < V.batch; ++b)
            if(V.pr.accept[b]) probe_record(ProbeHostTeam{}, V, b, t);
        return hipSuccess;
    }
    hipError_t launch_fourier_finish(hipStream_t, FourierView const& F, int first, int count, double* coef, double* thd)
    {
        for(long long i = 0; i < static_cast<long long>(count) * F.n_fp; ++i)
            fourier_finish(F, first + static_cast<int>(i / F.n_fp), static_cast<int>(i % F.n_fp), coef + i * (F.H + 1) * 4, thd + i);
        return hipSuccess;
    }
    // ... and those of the variable-step transient (pe_lte.hpp)
    hipError_t launch_tr_lte(hipStream_t, DevView const& V, LteView const& L)
    {
        *L.result = LteResult{};
        for(int b = 0; b < V.batch; ++b)
        {
            int nonfinite = 0;
            unsigned long long const u = lte_partial(ProbeHostTeam{}, V, L, b, nonfinite);
            if(L.test)
            {
                L.q_each[b] = u;
                if(u > L.result->q) L.result->q = u;
            }
            L.result->n_nonfinite += nonfinite;
            if(V.status[b] != 0) ++L.result->n_failed;
            L.result->iters_spent += L.iters_now[b] - L.iters_before[b];
        }
        return hipSuccess;
    }
    // ... and those of the BE / GEAR2 rules (pe_integ.hpp)
    hipError_t launch_tr_lte_integ(hipStream_t, DevView const& V, LteView const& L, int method)
    {
        *L.result = LteResult{};
        for(int b = 0; b < V.batch; ++b)
        {
            int nonfinite = 0;
            unsigned long long const u = integ_lte_partial(ProbeHostTeam{}, V, L, method, b, nonfinite);
            if(L.test)
            {
                L.q_each[b] = u;
                if(u > L.result->q) L.result->q = u;
            }
            L.result->n_nonfinite += nonfinite;
            if(V.status[b] != 0) ++L.result->n_failed;
            L.result->iters_spent += L.iters_now[b] - L.iters_before[b];
        }
        return hipSuccess;
    }
    hipError_t launch_integ_restart(hipStream_t, DevView const& V, bool only_failed)
    {
        if(!V.tr_hist) return hipSuccess;
        for(int b = 0; b < V.batch; ++b) integ_restart(ProbeHostTeam{}, V, b, only_failed);
        return hipSuccess;
    }
    hipError_t launch_tr_history_push(hipStream_t, DevView const& V, double* hist, int slot)
    {
        lte_history_push(ProbeHostTeam{}, V, hist, slot);
        return hipSuccess;
    }
    hipError_t launch_tr_state_copy(hipStream_t, StateCopy const& S)
    {
        for(int p = 0; p < S.n; ++p)
            if(S.bytes[p]) std::memcpy(S.dst[p], S.src[p], S.bytes[p]);
        return hipSuccess;
    }
    // ... and those of the DC sweep (pe_dc_sweep.hpp)
    hipError_t launch_dc_sweep_fill(hipStream_t, DevView const& V, DcSweepView const& S)
    {
        dc_sweep_fill(ProbeHostTeam{}, V, S);
        return hipSuccess;
    }
    hipError_t launch_dc_sweep_seed(hipStream_t, DevView const& V, DcSweepView const& S, bool from_main)
    {
        for(int q = 0; q < V.batch; ++q) dc_sweep_seed(ProbeHostTeam{}, V, S, q, from_main);
        return hipSuccess;
    }
    hipError_t launch_dc_sweep_classify(hipStream_t, DevView const& V, DcSweepView const& S, bool reseed)
    {
        dc_sweep_classify_serial(V, S, reseed);
        return hipSuccess;
    }
    hipError_t launch_dc_sweep_gather(hipStream_t, DevView const& V, DcSweepView const& S)
    {
        for(int q = 0; q < V.batch; ++q) dc_sweep_gather(ProbeHostTeam{}, V, S, q);
        return hipSuccess;
    }
    // ... and the controller of the stepped operating point (pe_op_step.hpp)
    hipError_t launch_op_step_control(hipStream_t, DevView const& V, OpStepView const& S, int role)
    {
        op_step_control_serial(V, S, role);
        return hipSuccess;
    }
}  // namespace pe
#endif

namespace pe_eng PE_ENG_HIDDEN
{
    // ---- the shell around a DC point (dc_solve, dc_solve_kept) and around a run of transient steps (pe_hip_analyze_tr, tr_run_steps)
    struct SolveRun
    {
        std::vector<long long> s0, i0;  // n_steps and n_iters of every instance before the solve
    };
    // a call's statistics start from zero -- before anything that can end the call early
    void solve_reset(pe_hip_engine* h, pe_hip_run_stats* st)
    {
        if(st) std::memset(st, 0, sizeof(*st));
        h->dominant_ms = 0.0;
        h->dominant_launches = 0;
    }
    // the counters before the solve (after the caller has cleared the status it wants cleared), then the event in front of its first launch
    int solve_begin(pe_hip_engine* h, SolveRun& run)
    {
        if(int const rc = snapshot_counters(h, run.s0, run.i0); rc != PE_HIP_OK) return rc;
        HIPCHK(h, hipEventRecord(h->ev0, h->stream));
        return PE_HIP_OK;
    }
    // the event behind its last launch, the stream synchronised, and what the call reports; launches: launches of the resident kernel
    int solve_end(pe_hip_engine* h, pe_hip_run_stats* st, SolveRun const& run, int launches)
    {
        HIPCHK(h, hipEventRecord(h->ev1, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
        int const rc = collect_stats(h, run.s0, run.i0, st);
        if(st)
        {
            st->gpu_ms = ms;
            st->n_launches = launches;
            bool const split = h->dominant_launches > 0;
            st->dominant_ms = split ? h->dominant_ms : ms;
            st->dominant_launches = split ? h->dominant_launches : launches;
        }
        return rc;
    }
    // The residual safety net around a solve that has been launched: at most two rounds of prepare_inaccurate_retry, each followed by
    // rerun(group) -- run_m2_dc / run_m2_tr on the group's instances for the steps they owe -- for every group it returns.
    template <class Rerun>
    int retry_inaccurate(pe_hip_engine* h, bool tr, double dt, int nsteps, std::vector<long long> const& s0, Rerun&& rerun)
    {
        for(int attempt = 0; attempt < 2; ++attempt)
        {
            HIPCHK(h, hipStreamSynchronize(h->stream));
            std::vector<std::pair<int, std::vector<int>>> groups;
            if(int const rc = prepare_inaccurate_retry(h, tr, dt, attempt, s0, nsteps, groups); rc != PE_HIP_OK) return rc;
            if(groups.empty()) break;
            for(auto const& g: groups)
                if(int const rc = rerun(g); rc != PE_HIP_OK) return rc;
        }
        return PE_HIP_OK;
    }

    // The stepping part of pe_hip_analyze_tr: `nsteps` steps of dt on the schedule in effect, then the residual safety net's retries of
    // the instances whose solve stayed inaccurate.  The caller has run ensure_symbolic and cleared the status; s0 = n_steps before the
    // steps.  Leaves the stream synchronised.  pe_hip_analyze_tr_adaptive takes its single steps through here too.
    int tr_run_steps(pe_hip_engine* h, double dt, int nsteps, std::vector<long long> const& s0, int& launches)
    {
        int rc = PE_HIP_OK;
        bool const may_reuse = !h->hc.nonlinear && !h->opt.refactor_every_solve && !has_overlay(h);
        int const chunk = h->hc.rows > 2000 ? 32 : (h->hc.rows > 200 ? 256 : 2048);
        int done = 0;
        if(split_launch(h))
        {
            rc = run_m2_tr(h, dt, nsteps, launches);
            if(rc != PE_HIP_OK) return rc;
            done = nsteps;
        }
        if(done < nsteps) h->resident.a_static.clear();  // (the resident kernel stamps the matrix itself: what the split schedule knew about it is void)
        bool const integ = h->tr_method != PE_HIP_TR_TRAP;
        while(done < nsteps)
        {
            double const key = integ_key(h, dt);
            bool const reuse = may_reuse && h->resident.fact_valid && h->fact_dt == key;
            int n = reuse || !may_reuse ? std::min(chunk, nsteps - done) : 1;  // first step factors, the rest may reuse
            // (GEAR2: one launch reuses one factorisation -- a step whose a0 is not that of the steps behind it, the first after a restart, goes alone)
            if(integ && reuse && !(h->resident.integ_hp == dt)) n = 1;
            if(h->probe.armed)
            {
                pe::ProbedView const pv = probe_view(h);
                HIPCHK(h, pe::launch_tr_steps(h->stream, pv, dt, n, reuse));  // (probe_armed set: the kernel that records)
            }
            else
                HIPCHK(h, pe::launch_tr_steps(h->stream, h->V, dt, n, reuse));
            ++launches;
            done += n;
            if(may_reuse)
            {
                h->resident.fact_valid = true;
                h->fact_dt = key;
            }
            if(integ) h->resident.integ_hp = dt;  // (put right below should an instance have failed)
        }
        rc = retry_inaccurate(h, true, dt, nsteps, s0,
                              [&](auto const& g)
                              {
                                  if(integ) h->resident.integ_hp = std::nan("");  // (instances stepped alone)
                                  return run_m2_tr(h, dt, g.first, launches, &g.second);
                              });
        if(rc != PE_HIP_OK) return rc;
        if(integ && nsteps > 0)
        {
            // every instance that is OK has taken its nsteps steps of dt: h_p = dt.  One that failed holds the point its failed step stored:
            // its history restarts before its next step (integ_before_steps), and until then the host knows no common h_p
            HIPCHK(h, hipStreamSynchronize(h->stream));
            std::vector<int> status(static_cast<size_t>(h->hc.batch));
            HIPCHK(h, hipMemcpy(status.data(), h->V.status, status.size() * sizeof(int), hipMemcpyDeviceToHost));
            bool const all_ok = std::all_of(status.begin(), status.end(), [](int v) { return v == PE_HIP_OK; });
            h->resident.integ_hp = all_ok ? dt : std::nan("");
            if(!all_ok) h->integ_failed = true;
        }
        return PE_HIP_OK;
    }

    // before the status of the instances is cleared for new steps: the history of the instances whose last step failed restarts
    int integ_before_steps(pe_hip_engine* h)
    {
        if(h->tr_method == PE_HIP_TR_TRAP || !h->integ_failed) return PE_HIP_OK;
        HIPCHK(h, pe::launch_integ_restart(h->stream, h->V, true));
        h->integ_failed = false;
        h->resident.integ_hp = std::nan("");
        invalidate_factors(h);
        return PE_HIP_OK;
    }

    int integ_alloc(pe_hip_engine* h)
    {
        h->V.tr_method = h->tr_method;
        if(!h->loaded) return PE_HIP_OK;
        // whatever was keyed on the other rule's companion conductances is void; captured launch sequences hold the old view; the snapshot
        // table of the variable-step transient is built again, with or without the history array
        invalidate_factors(h);
        h->resident.sym_dt = 0.0;
        pe::m2_graphs_clear(h->graphs.get());
        tr_adaptive_drop(h);
        h->integ_failed = false;
        h->resident.integ_hp = 0.0;
        if(h->tr_method == PE_HIP_TR_TRAP)
        {
            h->integ_pool.release();
            h->V.tr_hist = nullptr;
            return PE_HIP_OK;
        }
        if(!h->V.tr_hist) HIPCHK(h, h->integ_pool.alloc(h->V.tr_hist, static_cast<size_t>(h->hc.batch) * static_cast<size_t>(pe::integ_stride(h->V))));
        integ_restart(h);
        return PE_HIP_OK;
    }

    void integ_restart(pe_hip_engine* h)
    {
        if(!h->loaded || !h->V.tr_hist) return;
        (void)pe::launch_integ_restart(h->stream, h->V, false);
        (void)hipStreamSynchronize(h->stream);  // (the calls that restart go on with blocking copies)
        h->integ_failed = false;
        h->resident.integ_hp = 0.0;
        if(h->tr_method != PE_HIP_TR_TRAP)
        {
            invalidate_factors(h);  // (the a0 of the coming step is another)
        }
    }

    double integ_key(pe_hip_engine const* h, double dt)
    {
        if(h->tr_method == PE_HIP_TR_TRAP) return dt;
        if(std::isnan(h->resident.integ_hp)) return h->resident.integ_hp;
        return pe::integ_coef(h->tr_method, dt, h->resident.integ_hp).a0;
    }
    double integ_sym_dt(pe_hip_engine const* h, double dt)
    {
        if(h->tr_method == PE_HIP_TR_TRAP) return dt;
        return 2.0 / pe::integ_coef(h->tr_method, dt, std::isnan(h->resident.integ_hp) ? 0.0 : h->resident.integ_hp).a0;
    }
}  // namespace pe_eng

namespace pe_eng PE_ENG_HIDDEN
{
    void tr_adaptive_drop(pe_hip_engine* h)
    {
        auto& A = h->tra;
        if(A.allocated) (void)hipStreamSynchronize(h->stream);
        A = pe_hip_engine::TrAdaptive{};  // (its pool frees what it holds)
    }

    // shadow set of the state of a step (tr_state_parts = the arrays of a checkpoint, + the cursor of the Newton trace so that the trace
    // keeps accepted steps only), history ring and result slots: allocated once per resident circuit
    int tr_adaptive_alloc(pe_hip_engine* h)
    {
        auto& A = h->tra;
        if(A.allocated) return PE_HIP_OK;
        auto parts = ck_parts(h);
        parts.push_back({h->V.trace_len, sizeof(int)});
        if(h->tr_method != PE_HIP_TR_TRAP && h->V.tr_hist)  // (the one entry the table has left: the history of BE / GEAR2, values and h_p in ONE array)
            parts.push_back({h->V.tr_hist, static_cast<size_t>(h->hc.batch) * static_cast<size_t>(pe::integ_stride(h->V)) * sizeof(double)});
        if(parts.size() > 16) return fail(h, PE_HIP_ERR_INTERNAL, "analyze_tr_adaptive: the state of an instance has more arrays than the snapshot table holds");
        A.save = A.restore = pe::StateCopy{};
        for(auto const& p: parts)
        {
            if(p.bytes == 0) continue;
            char* shadow{};
            HIPCHK(h, A.pool.alloc(shadow, p.bytes, false));
            int const k = A.save.n++;
            A.save.dst[k] = shadow;
            A.save.src[k] = p.ptr;
            A.save.bytes[k] = p.bytes;
            A.restore.dst[k] = p.ptr;
            A.restore.src[k] = shadow;
            A.restore.bytes[k] = p.bytes;
            if(p.ptr == h->V.n_iters) A.shadow_iters = reinterpret_cast<long long*>(shadow);
        }
        A.restore.n = A.save.n;
        size_t const B = static_cast<size_t>(h->hc.batch);
        HIPCHK(h, A.pool.alloc(A.hist, 3 * B * h->hc.rows));
        HIPCHK(h, A.pool.alloc(A.q_each, B));
        HIPCHK(h, A.pool.alloc(A.result, 1));
        A.n_pts = 0;
        A.allocated = true;
        return PE_HIP_OK;
    }

    // corners of the generators whose parameters every instance shares (pe_front.hpp eval_devices: t0 = t + phase / (2 pi f), tm = fmod(t0, T);
    // sawtooth 0; square 0, duty T; pulse 0, tr, duty T - tf, duty T; triangle 0, T / 2) inside (t0, t1]
    void source_breakpoints(pe_hip_engine const* h, double t0, double t1, std::vector<double>& out)
    {
        auto const& hc = h->hc;
        int const n = hc.nTs();
        for(int i = 0; i < n; ++i)
        {
            int const kind = hc.ts_kind[static_cast<size_t>(i)];
            if(kind == 0) continue;  // IAC: smooth
            double const* p = &hc.ts_par[static_cast<size_t>(i) * 8];
            bool shared = true;
            for(int b = 1; b < hc.batch && shared; ++b)
                shared = std::memcmp(p, &hc.ts_par[(static_cast<size_t>(b) * n + i) * 8], 8 * sizeof(double)) == 0;
            double const freq = p[3];
            if(!shared || !(freq > 0.0) || !((t1 - t0) * freq <= 1e5)) continue;
            double const T = 1.0 / freq, shift = p[5] / (2.0 * 3.14159265358979323846) / freq;
            double corner[4] = {0.0, 0.0, 0.0, 0.0};
            int nc = 1;
            if(kind == 2) corner[nc++] = p[4] * T;
            else if(kind == 3)
            {
                corner[nc++] = p[6];
                corner[nc++] = p[4] * T - p[7];
                corner[nc++] = p[4] * T;
            }
            else if(kind == 4)
                corner[nc++] = 0.5 * T;
            double const k0 = std::floor((t0 + shift) / T) - 1.0, k1 = std::floor((t1 + shift) / T) + 1.0;
            for(double k = k0; k <= k1; k += 1.0)
                for(int c = 0; c < nc; ++c)
                {
                    double const tb = k * T + corner[c] - shift;
                    if(corner[c] >= 0.0 && corner[c] < T && tb > t0 && tb <= t1) out.push_back(tb);
                }
        }
    }
}  // namespace pe_eng

extern "C" {

int pe_hip_analyze_tr(pe_hip_engine* h, double dt, int nsteps, pe_hip_run_stats* st)
{
    if(!h || !h->loaded || nsteps < 0 || !(dt > 0.0)) return h ? fail(h, PE_HIP_ERR_ARG, "analyze_tr: bad arguments or no circuit") : PE_HIP_ERR_ARG;
    if(h->tr_method != PE_HIP_TR_TRAP && has_overlay(h))
        return fail(h, PE_HIP_ERR_ARG, "analyze_tr: a host-stamp overlay integrates in its own hooks, with the trapezoidal rule: set PE_HIP_TR_TRAP");
    HIPCHK(h, hipSetDevice(h->device));
    ac_sweep_invalidate(h);
    h->tra.n_pts = 0;  // (fixed steps restart the history of the variable-step transient)
    solve_reset(h, st);
    if(h->hc.rows == 0 || nsteps == 0) return PE_HIP_OK;
    int rc = ensure_symbolic(h, true, integ_sym_dt(h, dt));
    if(rc != PE_HIP_OK) return rc;
    rc = integ_before_steps(h);
    if(rc != PE_HIP_OK) return rc;
    // A failed solve is not sticky (circuit.h:242-254: the reference rolls tr_duration back, returns false, and the next
    // analyze() simply tries again from that state -- e.g. after the caller raised g_min): every run starts with all instances live.
    HIPCHK(h, hipMemsetAsync(h->V.status, 0, static_cast<size_t>(h->hc.batch) * sizeof(int), h->stream));
    SolveRun run;
    rc = solve_begin(h, run);
    if(rc != PE_HIP_OK) return rc;
    bool const may_reuse = !h->hc.nonlinear && !h->opt.refactor_every_solve && !has_overlay(h);
    int launches = 0;
    rc = tr_run_steps(h, dt, nsteps, run.s0, launches);
    if(rc != PE_HIP_OK) return rc;
    if(!may_reuse) h->resident.fact_valid = false;
    return solve_end(h, st, run, launches);
}

int pe_hip_analyze_tr_adaptive(pe_hip_engine* h, double t_stop, const pe_hip_tr_control* c, pe_hip_tr_adaptive_stats* out)
{
    if(!h) return PE_HIP_ERR_ARG;
    if(out) std::memset(out, 0, sizeof(*out));
    if(!h->loaded || !c) return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: no circuit or no control block");
    auto const fin = [](double v) { return std::isfinite(v); };
    if(!fin(t_stop) || !fin(c->dt_init) || !fin(c->dt_min) || !fin(c->dt_max) || !fin(c->lte_reltol) || !fin(c->lte_abstol_v) || !fin(c->lte_abstol_i) || !fin(c->trtol))
        return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: non-finite argument");
    if(!(c->dt_init > 0.0)) return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: dt_init must be > 0");
    if(c->n_breakpoints < 0 || (c->n_breakpoints > 0 && !c->breakpoints)) return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: bad breakpoint list");
    for(int k = 0; k < c->n_breakpoints; ++k)
        if(!fin(c->breakpoints[k])) return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: non-finite breakpoint");
    int const method = h->tr_method;
    if(has_overlay(h)) return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: a host-stamp overlay keeps host state that a rejected step cannot roll back");
    HIPCHK(h, hipSetDevice(h->device));
    int const B = h->hc.batch;
    std::vector<double> tb(static_cast<size_t>(B));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if(B) HIPCHK(h, hipMemcpy(tb.data(), h->V.t_now, tb.size() * sizeof(double), hipMemcpyDeviceToHost));
    for(int b = 1; b < B; ++b)
        if(tb[static_cast<size_t>(b)] != tb[0]) return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: the instances sit at different time points");
    double t = B ? tb[0] : 0.0;
    if(!(t_stop > t)) return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: t_stop must lie after the current time");
    double const dt_min = c->dt_min > 0.0 ? c->dt_min : c->dt_init * 1e-9;
    double const dt_max = c->dt_max > 0.0 ? c->dt_max : (t_stop - t) / 50.0;
    if(dt_min > dt_max) return fail(h, PE_HIP_ERR_ARG, "analyze_tr_adaptive: dt_min > dt_max");
    bool const lte_on = !(c->lte_reltol < 0.0);
    double const reltol = c->lte_reltol > 0.0 ? c->lte_reltol : 1e-3;
    double const abstol_v = c->lte_abstol_v > 0.0 ? c->lte_abstol_v : 1e-6, abstol_i = c->lte_abstol_i > 0.0 ? c->lte_abstol_i : 1e-9;
    double const trtol = c->trtol > 0.0 ? c->trtol : 7.0;
    // ---- from here on the engine changes
    ac_sweep_invalidate(h);
    auto& A = h->tra;
    A.log_dt.clear();
    A.log_outcome.clear();
    h->dominant_ms = 0.0;
    h->dominant_launches = 0;
    if(out) out->t_end = t;
    if(h->hc.rows == 0 || B == 0) return PE_HIP_OK;
    int rc = tr_adaptive_alloc(h);
    if(rc != PE_HIP_OK) return rc;
    // breakpoints after t, ascending; t_stop is the last one
    std::vector<double> bps(c->breakpoints, c->breakpoints + c->n_breakpoints);
    if(c->source_breakpoints) source_breakpoints(h, t, t_stop, bps);
    bps.erase(std::remove_if(bps.begin(), bps.end(), [&](double v) { return !(v < t_stop); }), bps.end());
    bps.push_back(t_stop);
    std::sort(bps.begin(), bps.end());
    constexpr double eps4 = 4.0 * 2.220446049250313e-16;
    auto const reached = [&](double at, double bp) { return at >= bp || std::fabs(at - bp) <= eps4 * std::fabs(bp); };
    size_t next_bp = 0;

    std::vector<long long> s0, i0, s_now;
    rc = snapshot_counters(h, s0, i0);
    if(rc != PE_HIP_OK) return rc;
    s_now = s0;
    long long const analyses0 = h->n_symbolic;
    bool const may_reuse = !h->hc.nonlinear && !h->opt.refactor_every_solve;
    std::vector<int> const all(static_cast<size_t>(B), 1);
    std::vector<int> status(static_cast<size_t>(B));
    pe_hip_tr_adaptive_stats S{};
    S.dt_smallest = INFINITY;
    int launches = 0;
    int final_rc = PE_HIP_OK;
    bool failed_at_dt_min = false;
    double dt = c->dt_init;
    HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    // (the controller's exponent: the trapezoidal rule and GEAR2 are of second order, err ~ h^3; BE of first, err ~ h^2)
    double const q_exp = method == PE_HIP_TR_BE ? -1.0 / 2.0 : -1.0 / 3.0;
    double hp_snapshot = h->resident.integ_hp;
    bool failed_snapshot = h->integ_failed;
    auto const roll_back = [&]() -> int
    {
        // the state of the snapshot; the host side as pe_hip_checkpoint_load leaves it (what the step spent came with the LTE result)
        HIPCHK(h, pe::launch_tr_state_copy(h->stream, A.restore));
        h->resident.integ_hp = hp_snapshot;  // (the history array of BE / GEAR2 is part of the snapshot: the host's knowledge of its h_p goes back with it)
        h->integ_failed = failed_snapshot;
        invalidate_factors(h);
        return PE_HIP_OK;
    };
    // (the loop in a function of its own: whichever way it ends, the statistics below are filled -- the log and t may have advanced)
    auto const stepping = [&]() -> int
    {
        while(!reached(t, t_stop) && (c->max_steps <= 0 || static_cast<long long>(A.log_dt.size()) < c->max_steps))
        {
            while(next_bp + 1 < bps.size() && reached(t, bps[next_bp])) ++next_bp;
            double const t_bp = bps[next_bp];
            double const hs = std::min({dt, dt_max, t_bp - t});
            if(!(hs > 0.0)) return fail(h, PE_HIP_ERR_INTERNAL, "analyze_tr_adaptive: the step underflowed");
            // snapshot, then one ordinary step that records nothing (the probes see it once it is accepted)
            rc = integ_before_steps(h);
            if(rc != PE_HIP_OK) return rc;
            HIPCHK(h, pe::launch_tr_state_copy(h->stream, A.save));
            hp_snapshot = h->resident.integ_hp;
            failed_snapshot = h->integ_failed;
            rc = ensure_symbolic(h, true, integ_sym_dt(h, hs));
            if(rc != PE_HIP_OK) return rc;
            HIPCHK(h, hipMemsetAsync(h->V.status, 0, static_cast<size_t>(B) * sizeof(int), h->stream));
            bool const armed = h->probe.armed;
            h->probe.armed = false;
            rc = tr_run_steps(h, hs, 1, s_now, launches);
            h->probe.armed = armed;
            if(rc != PE_HIP_OK) return rc;
            if(!may_reuse) h->resident.fact_valid = false;
            // the test on the device, the decision from one small copy
            bool const test = lte_on && A.n_pts >= 3;
            double const t_new = t + hs;
            pe::LteView L{};
            L.hist = A.hist;
            L.s2 = A.head;
            L.s1 = (A.head + 2) % 3;
            L.s0 = (A.head + 1) % 3;
            L.t0 = A.t_pts[L.s0];
            L.t1 = A.t_pts[L.s1];
            L.t2 = A.t_pts[L.s2];
            L.tn = t_new;
            L.h = hs;
            L.reltol = reltol;
            L.abstol_v = abstol_v;
            L.abstol_i = abstol_i;
            L.trtol = trtol;
            L.test = test ? 1 : 0;
            L.q_each = A.q_each;
            L.iters_now = h->V.n_iters;
            L.iters_before = A.shadow_iters;
            L.result = A.result;
            if(method == PE_HIP_TR_TRAP) HIPCHK(h, pe::launch_tr_lte(h->stream, h->V, L));
            else
                HIPCHK(h, pe::launch_tr_lte_integ(h->stream, h->V, L, method));
            pe::LteResult res{};
            HIPCHK(h, hipMemcpyAsync(&res, A.result, sizeof(res), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            double const q = test ? pe::lte_value(res.q) : 0.0;
            A.log_dt.push_back(hs);
            S.dt_smallest = std::min(S.dt_smallest, hs);
            S.dt_largest = std::max(S.dt_largest, hs);
            bool const at_min = hs <= dt_min;
            if(res.n_failed > 0 || res.n_nonfinite > 0)
            {
                A.log_outcome.push_back(2);
                ++S.n_rejected_newton;
                S.newton_iters_rejected += res.iters_spent;
                if(at_min)
                {
                    // ends as pe_hip_analyze_tr does: the step rolled back, the failed instances keep their status
                    HIPCHK(h, hipMemcpy(status.data(), h->V.status, status.size() * sizeof(int), hipMemcpyDeviceToHost));
                    if(res.n_failed == 0)
                        for(auto& v: status) v = PE_HIP_ERR_NO_CONVERGENCE;  // (defensive: a non-finite candidate that passed for converged; the step's own finiteness flag fails it first, not reachable through the public calls)
                    if(int const rrc = roll_back(); rrc != PE_HIP_OK) return rrc;
                    HIPCHK(h, hipMemcpyAsync(h->V.status, status.data(), status.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
                    HIPCHK(h, hipStreamSynchronize(h->stream));
                    failed_at_dt_min = true;
                    break;
                }
                if(int const rrc = roll_back(); rrc != PE_HIP_OK) return rrc;
                dt = std::max(hs / 8.0, dt_min);
                continue;
            }
            if(test && !pe::lte_passes(q))
            {
                if(!at_min)
                {
                    A.log_outcome.push_back(1);
                    ++S.n_rejected_lte;
                    S.newton_iters_rejected += res.iters_spent;
                    if(int const rrc = roll_back(); rrc != PE_HIP_OK) return rrc;
                    double const f = q > 1.0 ? std::max(0.1, 0.9 * std::pow(q, q_exp)) : 0.1;  // (defensive: q is a NaN only with a NaN in the history, not reachable through the public calls -- the smallest factor)
                    dt = std::max(hs * f, dt_min);
                    continue;
                }
                ++S.n_at_dt_min;
            }
            // accepted
            A.log_outcome.push_back(0);
            ++S.n_accepted;
            t = t_new;
            for(auto& v: s_now) ++v;
            if(armed)
                if(int const prc = probe_record_step(h, all, t); prc != PE_HIP_OK) return prc;
            bool const at_bp = next_bp + 1 < bps.size() && reached(t, t_bp);
            if(at_bp) A.n_pts = 0;  // (the history restarts AT the breakpoint: the point pushed below is its first)
            if(at_bp) integ_restart(h);  // (... and so does that of BE / GEAR2: x' jumps at a source corner, a two-step formula must not look across it)
            A.head = (A.head + 1) % 3;
            HIPCHK(h, pe::launch_tr_history_push(h->stream, h->V, A.hist, A.head));
            A.t_pts[A.head] = t;
            A.n_pts = std::min(A.n_pts + 1, 4);
            if(at_bp) dt = c->dt_init;
            else if(test)
                dt = hs * (q > 0.0 ? std::min(2.0, 0.9 * std::pow(q, q_exp)) : (q == 0.0 ? 2.0 : 1.0));  // (a NaN q accepted at dt_min: no growth)
            else
                dt = hs;
            dt = std::max(dt, dt_min);
        }
        return PE_HIP_OK;
    };
    int const loop_rc = stepping();
    S.n_analyses = static_cast<int>(h->n_symbolic - analyses0);
    S.t_end = t;
    if(A.log_dt.empty()) S.dt_smallest = 0.0;
    S.run.n_launches = launches;
    if(loop_rc != PE_HIP_OK)
    {
        A.n_pts = 0;  // (a step broken off half-way: the history no longer ends at the engine's state)
        (void)hipStreamSynchronize(h->stream);
        if(out) *out = S;
        return loop_rc;
    }
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    final_rc = collect_stats(h, s0, i0, &S.run);
    if(failed_at_dt_min && final_rc == PE_HIP_OK) final_rc = PE_HIP_ERR_NO_CONVERGENCE;
    S.run.gpu_ms = ms;
    S.run.n_launches = launches;
    bool const split = h->dominant_launches > 0;
    S.run.dominant_ms = split ? h->dominant_ms : ms;
    S.run.dominant_launches = split ? h->dominant_launches : launches;
    if(out) *out = S;
    return final_rc;
}

int pe_hip_get_tr_step_log(pe_hip_engine* h, long long first, int capacity, double* dt, int* outcome, long long* n_total)
{
    if(!h || first < 0 || capacity < 0) return PE_HIP_ERR_ARG;
    auto const& A = h->tra;
    long long const n = static_cast<long long>(A.log_dt.size());
    if(n_total) *n_total = n;
    for(long long k = first; k < n && k - first < capacity; ++k)
    {
        if(dt) dt[k - first] = A.log_dt[static_cast<size_t>(k)];
        if(outcome) outcome[k - first] = A.log_outcome[static_cast<size_t>(k)];
    }
    return PE_HIP_OK;
}

}  // extern "C"

namespace pe_eng
{
// The solving part of pe_hip_analyze_dc: one OP / DC / TROP point of every instance whose status is OK on the schedule in effect, then the
// residual safety net's retries.  clear_status: every instance takes part (what pe_hip_analyze_dc does); else the instances that are not OK
// stay as they are -- the DC sweep solves subsets that way, with the others parked.  Leaves the stream synchronised.
// kept (dc_solve_kept, pe_engine_internal.hpp): the factors of the last factorisation are kept -- the split schedule's iteration with
// do_factor = false on every instance, whatever schedule factored; the safety net's retries run exactly as without it, and those factor.
namespace
{
int dc_point(pe_hip_engine* h, int mode, pe_hip_run_stats* st, bool clear_status, bool kept)
{
    probe_disarm(h);  // (moves x: ends a probe window)
    ac_sweep_invalidate(h);
    solve_reset(h, st);
    if(h->hc.rows == 0) return PE_HIP_OK;
    int rc = kept ? PE_HIP_OK : ensure_symbolic(h, false, 0.0);
    if(rc != PE_HIP_OK) return rc;
    if(clear_status) HIPCHK(h, hipMemsetAsync(h->V.status, 0, static_cast<size_t>(h->hc.batch) * sizeof(int), h->stream));  // no sticky failure (see analyze_tr)
    SolveRun run;
    rc = solve_begin(h, run);
    if(rc != PE_HIP_OK) return rc;
    if(!kept) h->resident.fact_valid = false;
    h->resident.a_static.clear();  // (an OP / DC / TROP solve stamps other companion values into the matrix, on either schedule)
    long long const rematched0 = h->resident.n_rematched;
    int launches = 0;
    if(kept) rc = run_m2_dc(h, mode, launches, nullptr, false);  // (no factorisation: n_factor_launches does not count this attempt)
    else
    {
        ++h->n_factor_launches;
        if(split_launch(h)) rc = run_m2_dc(h, mode, launches);
        else
            HIPCHK(h, pe::launch_dc_point(h->stream, h->V, mode));
    }
    if(rc != PE_HIP_OK) return rc;
    rc = retry_inaccurate(h, false, 0.0, 1, run.s0,
                          [&](auto const& g)
                          {
                              ++h->n_factor_launches;
                              return run_m2_dc(h, mode, launches, &g.second);
                          });
    if(rc != PE_HIP_OK) return rc;
    // a re-match gave the engine another pivot order: only the retried instances hold factors of it -- every instance factors again
    if(kept && h->resident.n_rematched != rematched0) return dc_point(h, mode, st, true, false);
    return solve_end(h, st, run, 1);
}
}  // namespace

int dc_solve(pe_hip_engine* h, int mode, pe_hip_run_stats* st, bool clear_status) { return dc_point(h, mode, st, clear_status, false); }

int dc_solve_kept(pe_hip_engine* h, int mode, pe_hip_run_stats* st)
{
    // an engine that keeps no L21, or whose factors are not those of a DC point of a linear circuit, factors: dc_solve
    bool const keeps = !h->hc.nonlinear && h->V.keep_l21 && !has_overlay(h) && h->resident.sym_class == 0;
    return dc_point(h, mode, st, true, keeps);
}

}  // namespace pe_eng

extern "C" {

int pe_hip_analyze_dc(pe_hip_engine* h, int mode, pe_hip_run_stats* st)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    if(mode != PE_HIP_MODE_OP && mode != PE_HIP_MODE_DC && mode != PE_HIP_MODE_TROP) return fail(h, PE_HIP_ERR_ARG, "analyze_dc: mode must be OP, DC or TROP");
    HIPCHK(h, hipSetDevice(h->device));
    return dc_solve(h, mode, st, true);
}

}  // extern "C"

// ---------------- operating point with gmin / source stepping: dc_solve per level, the controller on the device (include/pe_hip.h, pe_op_step.hpp)
namespace pe_eng
{
    void op_step_drop(pe_hip_engine* h)
    {
        auto& O = h->ops;
        if(O.allocated) (void)hipStreamSynchronize(h->stream);
        O = pe_hip_engine::OpStep{};  // (its pools free what they hold)
    }
}  // namespace pe_eng

namespace
{
    // the controller's arrays and the shadow, sized by the circuit; the log, sized by the call
    int op_step_alloc(pe_hip_engine* h, int log_capacity)
    {
        auto& O = h->ops;
        auto& S = O.V;
        auto const& hc = h->hc;
        size_t const B = static_cast<size_t>(hc.batch);
        if(!O.allocated)
        {
            auto& P = O.pool;
            HIPCHK(h, P.alloc(S.state, B));
            HIPCHK(h, P.alloc(S.phase, B));
            HIPCHK(h, P.alloc(S.first, B));
            HIPCHK(h, P.alloc(S.have_shadow, B));
            HIPCHK(h, P.alloc(S.lambda, B));
            HIPCHK(h, P.alloc(S.delta, B));
            HIPCHK(h, P.alloc(S.cand, B));
            HIPCHK(h, P.alloc(S.final_status, B));
            HIPCHK(h, P.alloc(S.levels, B));
            HIPCHK(h, P.alloc(S.rejected, B));
            HIPCHK(h, P.alloc(S.iters, B));
            HIPCHK(h, P.alloc(S.it_prev, B));
            HIPCHK(h, P.alloc(S.log_n, B));
            HIPCHK(h, P.alloc(S.sx, B * hc.rows));
            HIPCHK(h, P.alloc(S.su, B * hc.nD()));
            HIPCHK(h, P.alloc(S.sg, B * hc.nD()));
            HIPCHK(h, P.alloc(S.sr, B * hc.nRl()));
            HIPCHK(h, P.alloc(S.rec, 1));
            O.allocated = true;
        }
        if(O.log_capacity != log_capacity)
        {
            HIPCHK(h, hipStreamSynchronize(h->stream));
            O.log_pool.release();
            O.log_capacity = -1;
            size_t const n = B * static_cast<size_t>(log_capacity);
            HIPCHK(h, O.log_pool.alloc(S.log_phase, n));
            HIPCHK(h, O.log_pool.alloc(S.log_outcome, n));
            HIPCHK(h, O.log_pool.alloc(S.log_iters, n));
            HIPCHK(h, O.log_pool.alloc(S.log_lambda, n));
            HIPCHK(h, O.log_pool.alloc(S.log_value, n));
            O.log_capacity = log_capacity;
        }
        return PE_HIP_OK;
    }
}  // namespace

extern "C" {

int pe_hip_analyze_op_stepping(pe_hip_engine* h, int mode, const pe_hip_op_step_control* c, pe_hip_op_step_stats* stats)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    if(stats) std::memset(stats, 0, sizeof(*stats));
    if(!c) return fail(h, PE_HIP_ERR_ARG, "analyze_op_stepping: no control");
    if(mode != PE_HIP_MODE_OP && mode != PE_HIP_MODE_DC && mode != PE_HIP_MODE_TROP) return fail(h, PE_HIP_ERR_ARG, "analyze_op_stepping: mode must be OP, DC or TROP");
    if(c->method != PE_HIP_STEP_GMIN && c->method != PE_HIP_STEP_SOURCE && c->method != PE_HIP_STEP_AUTO)
        return fail(h, PE_HIP_ERR_ARG, "analyze_op_stepping: unknown method");
    double const fields[5] = {c->dl_init, c->grow, c->shrink, c->dl_min, c->g_start};
    for(double const f: fields)
        if(!(f >= 0.0) || !std::isfinite(f)) return fail(h, PE_HIP_ERR_ARG, "analyze_op_stepping: a negative or non-finite control field");
    if(c->max_levels < 0 || c->step_max_newton < 0 || c->log_capacity < 0) return fail(h, PE_HIP_ERR_ARG, "analyze_op_stepping: a negative control field");
    if(c->method == PE_HIP_STEP_SOURCE && has_overlay(h))
        return fail(h, PE_HIP_ERR_ARG, "analyze_op_stepping: the sources of a host-stamp overlay cannot be stepped -- use PE_HIP_STEP_GMIN or PE_HIP_STEP_AUTO");
    HIPCHK(h, hipSetDevice(h->device));
    auto const& hc = h->hc;
    int const B = hc.batch;
    auto& O = h->ops;
    O.valid = false;
    // (a structurally singular circuit fails here as it does in pe_hip_analyze_dc: before anything is solved, so nothing can step)
    if(hc.rows > 0)
        if(int const rc = ensure_symbolic(h, false, 0.0); rc != PE_HIP_OK) return rc;
    if(int const rc = op_step_alloc(h, c->log_capacity); rc != PE_HIP_OK) return rc;
    auto& S = O.V;
    int const engine_newton = h->V.max_newton;
    S.method = has_overlay(h) ? (c->method & PE_HIP_STEP_GMIN) : c->method;
    S.max_levels = c->max_levels > 0 ? c->max_levels : 200;
    S.log_capacity = c->log_capacity;
    S.direct_cap = hc.nonlinear ? engine_newton : 1;
    S.attempt_cap = hc.nonlinear ? (c->step_max_newton > 0 ? c->step_max_newton : engine_newton) : 1;
    S.dl_init = c->dl_init > 0.0 ? c->dl_init : 0.125;
    S.grow = c->grow > 0.0 ? c->grow : 2.0;
    S.shrink = c->shrink > 0.0 ? c->shrink : 0.25;
    S.dl_min = c->dl_min > 0.0 ? c->dl_min : 0x1p-20;
    S.g_min = h->opt.g_min;
    S.g_start = c->g_start > 0.0 ? c->g_start : 1e-2;
    S.g_ratio = std::max(h->opt.g_min, 1e-13) / S.g_start;
    // the source slots and their real values: what fill_static_dv writes for VDC, IDC and the digital drives (the host circuit mirrors the
    // resident values).  The other load-time values -- a switch's resistance among them -- are not in the list: nothing scales them.
    std::vector<int> slot;
    for(int i = 0; i < hc.nVdc(); ++i) slot.push_back(hc.dv_vdc + i);
    for(int i = 0; i < hc.nIdc(); ++i) slot.push_back(hc.dv_idc + i);
    for(int k = 0; k < hc.n_drives; ++k) slot.push_back(hc.dv_drv + k);
    S.n_src = static_cast<int>(slot.size());
    std::vector<double> base(static_cast<size_t>(B) * slot.size());
    {
        std::vector<double> dv(static_cast<size_t>(B) * hc.dv_len, 0.0);
        fill_static_dv(h, dv);
        for(int b = 0; b < B; ++b)
            for(size_t j = 0; j < slot.size(); ++j) base[static_cast<size_t>(b) * slot.size() + j] = dv[static_cast<size_t>(b) * hc.dv_len + slot[j]];
    }
    Pool tabs;  // (uploaded once per call)
    int const* d_slot{};
    double const* d_base{};
    HIPCHK(h, tabs.upload(d_slot, slot));
    HIPCHK(h, tabs.upload(d_base, base));
    S.src_slot = d_slot;
    S.src_base = d_base;

    pe_hip_op_step_stats T{};
    hipStream_t const st = h->stream;
    pe_eng::Event ev_a, ev_b;  // (dc_solve records the engine's own pair)
    HIPCHK(h, ev_a.create());
    HIPCHK(h, ev_b.create());
    pe::OpStepRecord rec{};
    auto control = [&](int role) -> int
    {
        auto const t0 = clk::now();
        HIPCHK(h, hipMemsetAsync(S.rec, 0, sizeof(rec), st));
        HIPCHK(h, pe::launch_op_step_control(st, h->V, S, role));
        HIPCHK(h, hipMemcpyAsync(&rec, S.rec, sizeof(rec), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        ++T.n_launches;
        T.control_ms += ms_since(t0);
        return PE_HIP_OK;
    };
    // a numerical failure (or the parked status of the others) is an instance's own: everything else ends the call
    auto numerical = [](int rc)
    { return rc == PE_HIP_OK || rc == PE_HIP_ERR_SINGULAR || rc == PE_HIP_ERR_INACCURATE || rc == PE_HIP_ERR_NO_CONVERGENCE || rc == pe::DC_SWEEP_PARKED; };
    bool stepping = false;  // (slots may hold scaled values: the finish role must run)
    auto body = [&]() -> int
    {
        HIPCHK(h, hipEventRecord(ev_a, st));
        HIPCHK(h, hipMemcpyAsync(S.it_prev, h->V.n_iters, static_cast<size_t>(B) * sizeof(long long), hipMemcpyDeviceToDevice, st));
        int rc = dc_solve(h, mode, nullptr, true);  // 1. the direct attempt: pe_hip_analyze_dc itself
        ++T.n_solves;
        if(!numerical(rc)) return rc;
        if(hc.rows == 0) return PE_HIP_OK;
        stepping = true;
        if(rc = control(pe::OP_STEP_ROLE_BEGIN); rc != PE_HIP_OK) return rc;
        T.n_direct = rec.n_direct;
        T.newton_iters += rec.iters;
        T.n_failed += rec.n_failed;
        if(rec.n_active == 0 && rec.n_failed == 0)
        {
            // nothing failed: no slot was touched, and the parked statuses are all PE_HIP_OK again without another launch
            HIPCHK(h, hipMemsetAsync(h->V.status, 0, static_cast<size_t>(B) * sizeof(int), st));
            HIPCHK(h, hipStreamSynchronize(st));
            stepping = false;
            return PE_HIP_OK;
        }
        h->V.max_newton = hc.nonlinear ? S.attempt_cap : engine_newton;
        while(rec.n_active > 0)
        {
            T.n_levels += rec.n_active;
            rc = dc_solve(h, mode, nullptr, false);  // (a level is a new solve point: nothing of the last one is reused)
            ++T.n_solves;
            if(!numerical(rc)) return rc;
            if(rc = control(pe::OP_STEP_ROLE_CONTROL); rc != PE_HIP_OK) return rc;
            T.n_accepted += rec.n_accepted;
            T.n_rejected += rec.n_rejected;
            T.n_failed += rec.n_failed;
            T.newton_iters += rec.iters;
        }
        return PE_HIP_OK;
    };
    int rc = body();
    h->V.max_newton = engine_newton;
    if(stepping)
    {
        // whatever happened: real values in every slot, final statuses, failed instances back to their last accepted level
        std::string const err = h->err;
        int const frc = control(pe::OP_STEP_ROLE_FINISH);
        if(rc == PE_HIP_OK) rc = frc;
        else
            h->err = err;
        invalidate_factors(h);
    }
    float ms = 0.f;
    if(hipEventRecord(ev_b, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess) (void)hipEventElapsedTime(&ms, ev_a, ev_b);
    T.gpu_ms = ms;
    if(rc != PE_HIP_OK)
    {
        if(stats) *stats = T;
        return rc;
    }
    if(hc.rows == 0)
    {
        if(stats) *stats = T;
        return PE_HIP_OK;
    }
    // the outcome: one read of the final statuses and phases (no solution)
    std::vector<int> status(static_cast<size_t>(B)), phase(static_cast<size_t>(B)), state(static_cast<size_t>(B));
    HIPCHK(h, hipMemcpy(status.data(), h->V.status, static_cast<size_t>(B) * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(phase.data(), S.phase, static_cast<size_t>(B) * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(state.data(), S.state, static_cast<size_t>(B) * sizeof(int), hipMemcpyDeviceToHost));
    int first = PE_HIP_OK;
    for(int b = 0; b < B; ++b)
    {
        if(state[b] == pe::OP_STEP_SOLVED)
        {
            if(phase[b] == pe::OP_STEP_GMIN) ++T.n_gmin;
            else if(phase[b] == pe::OP_STEP_SOURCE)
                ++T.n_source;
        }
        else if(first == PE_HIP_OK)
            first = status[b] != PE_HIP_OK ? status[b] : PE_HIP_ERR_NO_CONVERGENCE;
    }
    O.valid = true;
    if(stats) *stats = T;
    if(first != PE_HIP_OK)
        return fail(h, first, first == PE_HIP_ERR_SINGULAR ? "analyze_op_stepping: singular matrix (zero / non-finite pivot) at the last attempt of an instance"
                                                            : "analyze_op_stepping: not every instance reached its operating point");
    return PE_HIP_OK;
}

int pe_hip_get_op_step_state(pe_hip_engine* h, int first, int count, int* phase_solved_in, double* lambda_reached, int* levels, int* rejected,
                             long long* newton_iters)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    auto const& O = h->ops;
    if(!O.valid) return fail(h, PE_HIP_ERR_ARG, "get_op_step_state: no stepping call yet");
    if(first < 0 || count < 0 || first + count > h->hc.batch) return fail(h, PE_HIP_ERR_ARG, "get_op_step_state: instances out of range");
    HIPCHK(h, hipSetDevice(h->device));
    size_t const n = static_cast<size_t>(count);
    if(phase_solved_in)
    {
        std::vector<int> state(n);
        HIPCHK(h, hipMemcpy(state.data(), O.V.state + first, n * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(phase_solved_in, O.V.phase + first, n * sizeof(int), hipMemcpyDeviceToHost));
        for(size_t i = 0; i < n; ++i)
            if(state[i] != pe::OP_STEP_SOLVED) phase_solved_in[i] = -1;
    }
    if(lambda_reached) HIPCHK(h, hipMemcpy(lambda_reached, O.V.lambda + first, n * sizeof(double), hipMemcpyDeviceToHost));
    if(levels) HIPCHK(h, hipMemcpy(levels, O.V.levels + first, n * sizeof(int), hipMemcpyDeviceToHost));
    if(rejected) HIPCHK(h, hipMemcpy(rejected, O.V.rejected + first, n * sizeof(int), hipMemcpyDeviceToHost));
    if(newton_iters) HIPCHK(h, hipMemcpy(newton_iters, O.V.iters + first, n * sizeof(long long), hipMemcpyDeviceToHost));
    return PE_HIP_OK;
}

int pe_hip_get_op_step_log(pe_hip_engine* h, int instance, int capacity, int* phase, double* lambda, double* value, int* outcome, int* iters,
                           int* n_total)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    auto const& O = h->ops;
    if(!O.valid) return fail(h, PE_HIP_ERR_ARG, "get_op_step_log: no stepping call yet");
    if(instance < 0 || instance >= h->hc.batch || capacity < 0) return fail(h, PE_HIP_ERR_ARG, "get_op_step_log: instance or capacity out of range");
    HIPCHK(h, hipSetDevice(h->device));
    int total = 0;
    HIPCHK(h, hipMemcpy(&total, O.V.log_n + instance, sizeof(int), hipMemcpyDeviceToHost));
    if(n_total) *n_total = total;
    size_t const n = static_cast<size_t>(std::min({capacity, total, O.log_capacity}));
    size_t const o = static_cast<size_t>(instance) * static_cast<size_t>(O.log_capacity);
    if(n == 0) return PE_HIP_OK;
    if(phase) HIPCHK(h, hipMemcpy(phase, O.V.log_phase + o, n * sizeof(int), hipMemcpyDeviceToHost));
    if(lambda) HIPCHK(h, hipMemcpy(lambda, O.V.log_lambda + o, n * sizeof(double), hipMemcpyDeviceToHost));
    if(value) HIPCHK(h, hipMemcpy(value, O.V.log_value + o, n * sizeof(double), hipMemcpyDeviceToHost));
    if(outcome) HIPCHK(h, hipMemcpy(outcome, O.V.log_outcome + o, n * sizeof(int), hipMemcpyDeviceToHost));
    if(iters) HIPCHK(h, hipMemcpy(iters, O.V.log_iters + o, n * sizeof(int), hipMemcpyDeviceToHost));
    return PE_HIP_OK;
}

}  // extern "C"

// ---------------- DC sweep: the points of a pass as extra instances of an engine of its own (include/pe_hip.h, pe_dc_sweep.hpp)
namespace pe_eng
{
    void dc_sweep_drop(pe_hip_engine* h)
    {
        h->dcs.drop();
    }
}  // namespace pe_eng

namespace
{
    // [batch][n] -> [batch * P][n]: instance b * P + p is a copy of instance b
    template <class T>
    void repeat_instances(std::vector<T>& v, int B, int P)
    {
        if(v.empty() || P == 1) return;
        size_t const per = v.size() / static_cast<size_t>(B);
        std::vector<T> o(v.size() * static_cast<size_t>(P));
        for(int b = 0; b < B; ++b)
            for(int p = 0; p < P; ++p) std::copy(v.begin() + b * per, v.begin() + (b + 1) * per, o.begin() + (static_cast<size_t>(b) * P + p) * per);
        v.swap(o);
    }

    // the sweep engine: the main engine's circuit with every per-instance array repeated P times, loaded like any circuit (what
    // sweep_engine_build of pe_engine_ac.cpp does for the AC system), and the buffers sized by its batch.  first_value: what the swept
    // parameter of instance 0 holds for the symbolic analysis.
    int dc_sweep_engine_build(pe_hip_engine* h, int P, int kind, int j, double first_value)
    {
        auto& D = h->dcs;
        D.eng.reset();  // (synchronises its stream first: nothing reads the buffers freed next any more)
        D.P = 0;
        D.pass_pool.release();
        pe::HostCircuit c = h->hc;
        int const B = h->hc.batch;
        repeat_instances(c.r_g, B, P);
        repeat_instances(c.c_cap, B, P);
        repeat_instances(c.l_ind, B, P);
        repeat_instances(c.vdc_v, B, P);
        repeat_instances(c.vac_par, B, P);
        repeat_instances(c.idc_i, B, P);
        repeat_instances(c.d_par, B, P);
        repeat_instances(c.d_raw, B, P);
        repeat_instances(c.gen_par, B, P);
        repeat_instances(c.ts_par, B, P);
        repeat_instances(c.cl_par, B, P);
        repeat_instances(c.rl_par, B, P);
        repeat_instances(c.n3_par, B, P);
        c.batch = B * P;
        if(j >= 0)
        {
            if(kind == PE_HIP_R) c.r_g[static_cast<size_t>(j)] = 1.0 / first_value;
            else if(kind == PE_HIP_VDC)
                c.vdc_v[static_cast<size_t>(j)] = first_value;
            else
                c.idc_i[static_cast<size_t>(j)] = first_value;
        }
        if(int const rc = engine_build(h->device, D.eng, h, "analyze_dc_sweep", &h->opt, std::move(c)); rc != PE_HIP_OK) return rc;
        size_t const Q = static_cast<size_t>(B) * P;
        auto& S = D.V;
        HIPCHK(h, D.pass_pool.alloc(S.seed_of, Q));
        HIPCHK(h, D.pass_pool.alloc(S.scan, Q));
        HIPCHK(h, D.pass_pool.alloc(S.pair_status, Q));
        HIPCHK(h, D.pass_pool.alloc(S.pair_iters, Q));
        HIPCHK(h, D.pass_pool.alloc(S.pair_seed, Q));
        HIPCHK(h, D.pass_pool.alloc(S.rec, 1));
        D.P = P;
        D.epoch = h->param_epoch;
        return PE_HIP_OK;
    }
}  // namespace

extern "C" {

int pe_hip_set_dc_sweep_rows(pe_hip_engine* h, int n_rows, const int* rows)
{
    if(!h) return PE_HIP_ERR_ARG;
    int const rc = h->dcs.kept.set(h, "set_dc_sweep_rows", n_rows, rows);
    if(rc == PE_HIP_OK) h->dcs.valid = false;  // (the stored result has the layout of the rows it was made with)
    return rc;
}

int pe_hip_analyze_dc_sweep(pe_hip_engine* h, int n_points, const double* values, const pe_hip_dc_sweep_control* c, int* point_status,
                            pe_hip_dc_sweep_stats* stats)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    if(stats) std::memset(stats, 0, sizeof(*stats));
    if(n_points < 1 || !values || !c) return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: n_points < 1, no values or no control");
    auto const& hc = h->hc;
    if(c->mode != PE_HIP_MODE_OP && c->mode != PE_HIP_MODE_DC) return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: mode must be OP or DC");
    if(c->order != PE_HIP_DC_SWEEP_PARALLEL && c->order != PE_HIP_DC_SWEEP_TRACE) return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: unknown order");
    std::vector<int> const* map = c->kind == PE_HIP_R ? &hc.map_r : c->kind == PE_HIP_VDC ? &hc.map_vdc : c->kind == PE_HIP_IDC ? &hc.map_idc : nullptr;
    if(!map || c->column != 0) return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: the swept parameter must be column 0 of a PE_HIP_VDC, PE_HIP_IDC or PE_HIP_R");
    if(c->index < 0 || c->index >= static_cast<int>(map->size())) return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: index out of range");
    for(int i = 0; i < n_points; ++i)
        if(!std::isfinite(values[i]) || (c->kind == PE_HIP_R && values[i] == 0.0)) return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: a non-finite value, or r == 0");
    if(has_overlay(h)) return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: a circuit with a host-stamp overlay cannot be swept on the device");
    bool const trace = c->order == PE_HIP_DC_SWEEP_TRACE;
    if(!trace && hc.nRl() > 0) return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: a relay's state depends on history -- use PE_HIP_DC_SWEEP_TRACE");
    HIPCHK(h, hipSetDevice(h->device));
    auto& D = h->dcs;
    D.valid = false;
    int const B = hc.batch, N = hc.rows;
    int const K = D.kept.rows.empty() ? N : static_cast<int>(D.kept.rows.size());
    pe_hip_dc_sweep_stats T{};
    T.n_points = n_points;
    size_t const pairs = static_cast<size_t>(n_points) * B;
    D.res.assign(pairs * K, std::nan(""));
    D.status.assign(pairs, PE_HIP_OK);
    D.iters.assign(pairs, 0);
    D.seed.assign(pairs, -1);
    auto finish = [&]() -> int
    {
        D.n_points = n_points;
        D.n_keep = K;
        D.batch = B;
        D.valid = true;
        if(stats) *stats = T;
        int first = PE_HIP_OK;
        for(int i = 0; i < n_points; ++i)
        {
            int st = PE_HIP_OK;
            for(int b = 0; b < B && st == PE_HIP_OK; ++b) st = D.status[static_cast<size_t>(i) * B + b];
            if(point_status) point_status[i] = st;
            if(first == PE_HIP_OK) first = st;
        }
        if(first != PE_HIP_OK) return fail(h, first, "analyze_dc_sweep: not every point converged");
        return PE_HIP_OK;
    };
    if(N == 0) return finish();

    // ---- the slots: PARALLEL -- the values sorted ascending (ties in the caller's order), cut into passes of P, the last one padded with its
    // last point; TRACE -- the caller's order, two slots per point (working copy, shadow)
    int const j = (*map)[c->index];
    int const slot = j < 0 ? -1 : (c->kind == PE_HIP_R ? hc.dv_r : c->kind == PE_HIP_VDC ? hc.dv_vdc : hc.dv_idc) + j;
    auto slot_value = [&](double v) { return c->kind == PE_HIP_R ? 1.0 / v : v; };
    std::vector<int> order(static_cast<size_t>(n_points));
    for(int i = 0; i < n_points; ++i) order[i] = i;
    if(!trace) std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return values[a] < values[b]; });
    int P = 2;
    if(!trace)
    {
        // (the main engine's arrays per instance; its factor storage is part of them once it has been analysed)
        long long bpi = static_cast<long long>((h->circ_pool.bytes + h->sym_pool.bytes) / static_cast<size_t>(std::max(1, B)));
        if(h->resident.sym_class < 0) bpi = 4 * static_cast<long long>(h->circ_pool.bytes / static_cast<size_t>(std::max(1, B)));
        P = static_cast<int>(std::min<long long>(sweep_pass_cap(knob(h, "DC_SWEEP_POINTS", 0), std::max<long long>(1, bpi), B), n_points));
    }
    else if(2ll * B > SWEEP_MAX_INSTANCES)
        return fail(h, PE_HIP_ERR_ARG, "analyze_dc_sweep: the batch is too large for a TRACE sweep");
    int const n_passes = trace ? n_points : (n_points + P - 1) / P;
    size_t const L = static_cast<size_t>(n_passes) * P;
    std::vector<double> val_h(L);
    std::vector<int> pt_h(L), rk_h(L, 0);
    for(int s = 0; s < n_passes; ++s)
    {
        if(trace)
        {
            val_h[2 * s] = val_h[2 * s + 1] = slot_value(values[s]);
            pt_h[2 * s] = s;
            pt_h[2 * s + 1] = -1;
            continue;
        }
        int const n = std::min(P, n_points - s * P);
        for(int p = 0; p < P; ++p)
        {
            int const k = s * P + std::min(p, n - 1);
            val_h[static_cast<size_t>(s) * P + p] = slot_value(values[order[k]]);
            pt_h[static_cast<size_t>(s) * P + p] = p < n ? order[k] : -1;
            rk_h[static_cast<size_t>(s) * P + p] = p == 0 ? 0 : rk_h[static_cast<size_t>(s) * P + p - 1] + (values[order[k]] != values[order[s * P + std::min(p - 1, n - 1)]] ? 1 : 0);
        }
    }

    // ---- the sweep engine (rebuilt when P or anything it was built from has changed), its one symbolic analysis
    if(!D.eng || D.P != P || D.epoch != h->param_epoch)
        if(int const rc = dc_sweep_engine_build(h, P, c->kind, j, values[order[0]]); rc != PE_HIP_OK) return rc;
    pe_hip_engine* const E = D.eng.get();
    hipStream_t const es = E->stream;
    long long const analyses0 = E->n_symbolic;
    if(int const rc = ensure_symbolic(E, false, 0.0); rc != PE_HIP_OK) return fail(h, rc, "analyze_dc_sweep (symbolic analysis): " + E->err);
    int const Q = B * P;

    // ---- buffers sized by the call: the slot tables, the result in the caller's order, the kept rows
    auto& S = D.V;
    if(D.res_pairs != pairs || D.res_len != pairs * K || !S.res)
    {
        D.res_pool.release();
        S.res = nullptr;
        HIPCHK(h, D.res_pool.alloc(S.res, pairs * K, false));
        HIPCHK(h, D.res_pool.alloc(S.res_status, pairs));
        HIPCHK(h, D.res_pool.alloc(S.res_iters, pairs));
        HIPCHK(h, D.res_pool.alloc(S.res_seed, pairs));
        D.res_pairs = pairs;
        D.res_len = pairs * K;
    }
    Pool slots;  // (value / point / rank of every slot of every pass: uploaded once per call)
    double* d_val{};
    int *d_pt{}, *d_rk{};
    HIPCHK(h, slots.alloc(d_val, L, false));
    HIPCHK(h, slots.alloc(d_pt, L, false));
    HIPCHK(h, slots.alloc(d_rk, L, false));
    HIPCHK(h, hipMemcpy(d_val, val_h.data(), L * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d_pt, pt_h.data(), L * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d_rk, rk_h.data(), L * sizeof(int), hipMemcpyHostToDevice));
    if(int const rc = D.kept.upload(h, S.keep); rc != PE_HIP_OK) return rc;
    S.P = P;
    S.n_inst = B;
    S.slot = slot;
    S.trace = trace ? 1 : 0;
    S.attempt_cap = hc.nonlinear ? E->V.max_newton : 1;
    S.n_keep = K;
    S.m_x = h->V.x;
    S.m_udlast = h->V.d_udlast;
    S.m_geq = h->V.d_geq;
    S.m_dv = h->V.dv;
    S.m_t_now = h->V.t_now;
    S.m_last_step = h->V.last_step;
    S.m_rl = h->V.rl_engaged;

    // round 0 of every pass: every slot from the main engine's state of its circuit instance, everything open (TRACE: the shadows parked)
    std::vector<int> seed0(static_cast<size_t>(Q)), status0(static_cast<size_t>(Q), PE_HIP_OK);
    for(int q = 0; q < Q; ++q) seed0[q] = q / P;
    if(trace)
        for(int b = 0; b < B; ++b) status0[2 * b + 1] = pe::DC_SWEEP_PARKED;
    auto start_from_main = [&]() -> int
    {
        HIPCHK(h, hipMemcpyAsync(S.seed_of, seed0.data(), static_cast<size_t>(Q) * sizeof(int), hipMemcpyHostToDevice, es));
        HIPCHK(h, hipMemcpyAsync(E->V.status, status0.data(), static_cast<size_t>(Q) * sizeof(int), hipMemcpyHostToDevice, es));
        HIPCHK(h, pe::launch_dc_sweep_seed(es, E->V, S, true));
        return PE_HIP_OK;
    };
    // one batched solve of the instances whose status is OK; a numerical failure (or the parked status of the others) is theirs alone
    auto solve = [&]() -> int
    {
        int const rc = dc_solve(E, c->mode, nullptr, false);
        if(rc == PE_HIP_OK || rc == PE_HIP_ERR_SINGULAR || rc == PE_HIP_ERR_INACCURATE || rc == PE_HIP_ERR_NO_CONVERGENCE || rc == pe::DC_SWEEP_PARKED) return PE_HIP_OK;
        return fail(h, rc, "analyze_dc_sweep: " + E->err);
    };
    pe::DcSweepRecord rec{};
    auto classify = [&](bool reseed, bool read) -> int
    {
        HIPCHK(h, pe::launch_dc_sweep_classify(es, E->V, S, reseed));
        if(!read) return PE_HIP_OK;
        HIPCHK(h, hipMemcpyAsync(&rec, S.rec, sizeof(rec), hipMemcpyDeviceToHost, es));
        HIPCHK(h, hipStreamSynchronize(es));
        return PE_HIP_OK;
    };
    HIPCHK(h, hipEventRecord(h->ev0, es));
    if(trace)
    {
        if(int const rc = start_from_main(); rc != PE_HIP_OK) return rc;
        HIPCHK(h, hipMemsetAsync(S.rec, 0, sizeof(rec), es));
        S.n_valid = 1;
        for(int i = 0; i < n_points; ++i)
        {
            S.value = d_val + 2 * static_cast<size_t>(i);
            S.point = d_pt + 2 * static_cast<size_t>(i);
            S.rank = d_rk + 2 * static_cast<size_t>(i);
            HIPCHK(h, pe::launch_dc_sweep_fill(es, E->V, S));
            if(int const rc = solve(); rc != PE_HIP_OK) return rc;
            // bookkeeping, result of the point, then shadow <- working copy (converged) or working copy <- shadow (failed): nothing is read here
            if(int const rc = classify(false, i == n_points - 1); rc != PE_HIP_OK) return rc;
            HIPCHK(h, pe::launch_dc_sweep_gather(es, E->V, S));
            HIPCHK(h, pe::launch_dc_sweep_seed(es, E->V, S, false));
        }
        T.n_passes = n_points;
        T.points_per_pass = 1;
        T.n_failed_cold = T.n_failed = rec.n_failing;
        T.newton_iters = rec.iters;
    }
    else
        for(int s = 0; s < n_passes; ++s)
        {
            int const n = std::min(P, n_points - s * P);
            S.value = d_val + static_cast<size_t>(s) * P;
            S.point = d_pt + static_cast<size_t>(s) * P;
            S.rank = d_rk + static_cast<size_t>(s) * P;
            S.n_valid = n;
            ++T.n_passes;
            T.points_per_pass = std::max(T.points_per_pass, n);
            if(int const rc = start_from_main(); rc != PE_HIP_OK) return rc;
            HIPCHK(h, pe::launch_dc_sweep_fill(es, E->V, S));
            if(int const rc = solve(); rc != PE_HIP_OK) return rc;
            HIPCHK(h, hipMemsetAsync(S.rec, 0, sizeof(rec), es));
            if(int const rc = classify(c->continuation != 0, true); rc != PE_HIP_OK) return rc;
            T.n_failed_cold += rec.n_failing;
            T.newton_iters += rec.iters;
            int const max_rounds = c->max_rounds > 0 ? c->max_rounds : n;
            int rounds = 0;
            while(c->continuation != 0 && rec.n_failing > 0 && rec.n_reseeded > 0 && rounds < max_rounds)
            {
                T.n_reseeded += rec.n_reseeded;
                HIPCHK(h, pe::launch_dc_sweep_seed(es, E->V, S, false));
                if(int const rc = solve(); rc != PE_HIP_OK) return rc;
                HIPCHK(h, hipMemsetAsync(S.rec, 0, sizeof(rec), es));
                if(int const rc = classify(true, true); rc != PE_HIP_OK) return rc;
                ++rounds;
                T.newton_iters += rec.iters;
                if(rec.n_newly_converged == 0) break;  // (the round converged no new pair: the same seeds would be tried again)
            }
            T.n_rounds = std::max(T.n_rounds, rounds);
            T.n_failed += rec.n_failing;
            HIPCHK(h, pe::launch_dc_sweep_gather(es, E->V, S));
        }
    HIPCHK(h, hipEventRecord(h->ev1, es));
    HIPCHK(h, hipStreamSynchronize(es));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    T.gpu_ms = ms;
    T.n_analyses = static_cast<int>(E->n_symbolic - analyses0);
    // ---- the one copy of the results, and the pairs' bookkeeping beside it
    if(pairs * K) HIPCHK(h, hipMemcpy(D.res.data(), S.res, pairs * K * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(D.status.data(), S.res_status, pairs * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(D.iters.data(), S.res_iters, pairs * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(D.seed.data(), S.res_seed, pairs * sizeof(int), hipMemcpyDeviceToHost));
    return finish();
}

int pe_hip_get_dc_sweep(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, double* x)
{
    if(!h || !h->loaded || !x) return PE_HIP_ERR_ARG;
    auto const& D = h->dcs;
    if(int const rc = stored_window(h, "get_dc_sweep", "DC sweep", "points", D.valid, D.batch, D.n_points, first_point, n_points, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    size_t const K = static_cast<size_t>(D.n_keep);
    for(int i = 0; i < n_points && count * K != 0; ++i)
        std::memcpy(x + static_cast<size_t>(i) * count * K, &D.res[(static_cast<size_t>(first_point + i) * D.batch + first_instance) * K],
                    static_cast<size_t>(count) * K * sizeof(double));
    return PE_HIP_OK;
}

int pe_hip_get_dc_sweep_status(pe_hip_engine* h, int first_point, int n_points, int first_instance, int count, int* status, int* newton_iters,
                               int* seed_point)
{
    if(!h || !h->loaded) return PE_HIP_ERR_ARG;
    auto const& D = h->dcs;
    if(int const rc = stored_window(h, "get_dc_sweep_status", "DC sweep", "points", D.valid, D.batch, D.n_points, first_point, n_points, first_instance, count);
       rc != PE_HIP_OK)
        return rc;
    for(int i = 0; i < n_points; ++i)
        for(int b = 0; b < count; ++b)
        {
            size_t const src = static_cast<size_t>(first_point + i) * D.batch + first_instance + b, dst = static_cast<size_t>(i) * count + b;
            if(status) status[dst] = D.status[src];
            if(newton_iters) newton_iters[dst] = D.iters[src];
            if(seed_point) seed_point[dst] = D.seed[src];
        }
    return PE_HIP_OK;
}

}  // extern "C"
