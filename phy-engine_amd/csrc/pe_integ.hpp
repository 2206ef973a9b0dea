// pe_integ.hpp -- the integration rules of the transient other than the trapezoidal one (pe_hip_set_tr_method): backward Euler and the
// variable-step second-order Gear rule (BDF2), written against a "team" like pe_lte.hpp / pe_probe.hpp.  Only tid() and size() of the
// team are used.
//
// For a step from t_n to t_n + h, with h_p the accepted step that led to t_n and rho = h / h_p, the derivative at the new point is
//   y' = a0 y_{n+1} + a1 y_n + a2 y_{n-1}
//     BE     a0 = 1 / h                          a1 = -1 / h            a2 = 0
//     GEAR2  a0 = (1 + 2 rho) / (h (1 + rho))    a1 = -(1 + rho) / h    a2 = rho^2 / (h (1 + rho))
// A GEAR2 step takes the BE coefficients, decided per instance, when the instance has no second point (h_p = 0) or when
// rho > 1 + sqrt 2: the zero-stability limit of variable-step BDF2 (a slope extrapolated from a much shorter previous step also
// multiplies the rounding error of y_n - y_{n-1} by rho).
//
// The companions, in the form the stamp (pe_front.hpp eval_devices) reads:
//   capacitor          prevg = a0 C            hist  = C (a1 v_n + a2 v_{n-1})
//   inductor           dv_lr = -a0 L           dv_lu = L (a1 i_n + a2 i_{n-1})
//   coupled inductors  Req = a0 [[L1 M],[M L2]]    u = [[L1 M],[M L2]] (a1 i_n + a2 i_{n-1})
//   junction           cd = tt geq of the last linearisation -- FROZEN at the start of the step, as it is for the trapezoidal rule --
//                      under the trapezoidal rule's guards: prevg = a0 cd, hist = cd (a1 vd_n + a2 vd_{n-1}); otherwise both 0
//
// State: ONE array per engine, V.tr_hist [batch][integ_stride(V)].  Per instance: v_{n-1} of every capacitor, i_{n-1} of every inductor,
// i1 and i2 of every coupled pair, vd_{n-1} of every junction, then the slot h_p (0: the next step starts the history).  The companion
// update of a step reads the old values, computes from x (= x_n) and stores the values of x_n; h_p := h is a step of its own
// (integ_commit) behind a barrier, because every thread of the team reads the slot: a team that can synchronise does both in
// companion_update, the grid-wide team of the split schedule gets the commit as a launch of its own behind the update.
#pragma once
#include "pe_device.hpp"
#include "pe_lte.hpp"

#include <cmath>

#ifndef PE_DEV
    #if defined(__HIPCC__)
        #define PE_DEV __device__ __forceinline__
    #else
        #define PE_DEV inline
    #endif
#endif
#if defined(__HIPCC__)
    #define PE_HOST_DEV __host__ __device__ inline
#else
    #define PE_HOST_DEV inline
#endif

namespace pe
{
    enum : int
    {
        TR_TRAP = 0,
        TR_BE = 1,
        TR_GEAR2 = 2
    };
    struct IntegCoef
    {
        double a0, a1, a2;
    };
    // 1 + sqrt 2
    constexpr double INTEG_RHO_MAX = 2.414213562373095;

    // (the host keys its bookkeeping of the companion conductances on a0 of this very function)
    PE_HOST_DEV IntegCoef integ_coef(int method, double h, double hp)
    {
        IntegCoef c;
        c.a0 = 1.0 / h;
        c.a1 = -1.0 / h;
        c.a2 = 0.0;
        if(method == TR_GEAR2 && hp > 0.0)
        {
            double const rho = h / hp;
            if(!(rho > INTEG_RHO_MAX))
            {
                c.a0 = (1.0 + 2.0 * rho) / (h * (1.0 + rho));
                c.a1 = -(1.0 + rho) / h;
                c.a2 = rho * rho / (h * (1.0 + rho));
            }
        }
        return c;
    }

    PE_HOST_DEV long long integ_stride(DevView const& V) { return static_cast<long long>(V.nC) + V.nL + 2LL * V.nCl + V.nD + 1; }

    PE_DEV double integ_volt(double const* x, int row) { return row >= 0 ? x[row] : 0.0; }

    // the companion update of a step of size dt under V.tr_method (BE / GEAR2); leaves h_p alone
    template <class Team>
    PE_DEV void integ_companion_update(Team const& tm, DevView const& V, int b, double dt)
    {
        double const* x = V.x + static_cast<long long>(b) * V.rows;
        double* dv = V.dv + static_cast<long long>(b) * V.dv_len;
        long long const stride = integ_stride(V);
        double* old = V.tr_hist + static_cast<long long>(b) * stride;
        bool const on = dt > 0.0;
        IntegCoef k{0.0, 0.0, 0.0};
        if(on) k = integ_coef(V.tr_method, dt, old[stride - 1]);
        if(on)
        {
            double* hist = V.c_hist + static_cast<long long>(b) * V.nC;
            double* prevg = V.c_prevg + static_cast<long long>(b) * V.nC;
            double const* cap = V.c_cap + static_cast<long long>(b) * V.nC;
            for(int i = tm.tid(); i < V.nC; i += tm.size())
            {
                double const v_n = integ_volt(x, V.c_a[i]) - integ_volt(x, V.c_b[i]);
                prevg[i] = k.a0 * cap[i];
                hist[i] = cap[i] * (k.a1 * v_n + k.a2 * old[i]);
                old[i] = v_n;
            }
        }
        {
            double const* ind = V.l_ind + static_cast<long long>(b) * V.nL;
            double* o = old + V.nC;
            for(int i = tm.tid(); i < V.nL; i += tm.size())
            {
                double req = 0.0, ueq = 0.0;
                if(on)
                {
                    double const i_n = x[V.l_k[i]];
                    req = k.a0 * ind[i];
                    ueq = ind[i] * (k.a1 * i_n + k.a2 * o[i]);
                    o[i] = i_n;
                }
                dv[V.dv_lr + i] = -req;
                dv[V.dv_lu + i] = ueq;
            }
        }
        {
            double const* par = V.cl_par + static_cast<long long>(b) * V.nCl * 3;
            double* o = old + V.nC + V.nL;
            for(int i = tm.tid(); i < V.nCl; i += tm.size())
            {
                double r11 = 0.0, r12 = 0.0, r22 = 0.0, u1 = 0.0, u2 = 0.0;
                if(on)
                {
                    double const L1 = par[3 * i], L2 = par[3 * i + 1], kc = par[3 * i + 2];
                    double const M = kc * sqrt(L1 * L2);
                    r11 = k.a0 * L1;
                    r12 = k.a0 * M;
                    r22 = k.a0 * L2;
                    double const i1 = x[V.cl_k[2 * i]], i2 = x[V.cl_k[2 * i + 1]];
                    double const s1 = k.a1 * i1 + k.a2 * o[2 * i], s2 = k.a1 * i2 + k.a2 * o[2 * i + 1];
                    u1 = L1 * s1 + M * s2;
                    u2 = M * s1 + L2 * s2;
                    o[2 * i] = i1;
                    o[2 * i + 1] = i2;
                }
                int const q = V.cl_dv[i];
                dv[q] = r11;
                dv[q + 1] = r12;
                dv[q + 2] = r22;
                dv[q + 3] = u1;
                dv[q + 4] = u2;
            }
        }
        {
            double* udl = V.d_udlast + static_cast<long long>(b) * V.nD;
            double* geq = V.d_geq + static_cast<long long>(b) * V.nD;
            double* hist = V.d_hist + static_cast<long long>(b) * V.nD;
            double* prevg = V.d_prevg + static_cast<long long>(b) * V.nD;
            double const* par = V.d_par + static_cast<long long>(b) * V.nD * DP_NCOL;
            double* o = old + V.nC + V.nL + 2 * V.nCl;
            for(int i = tm.tid(); i < V.nD; i += tm.size())
            {
                double const vd = integ_volt(x, V.d_a[i]) - integ_volt(x, V.d_c[i]);
                udl[i] = vd;
                double const tt = par[i * DP_NCOL + DP_TT];
                double const cd = tt * geq[i];
                if(!on || !(tt > 0.0) || !(geq[i] > 0.0) || !(cd > 0.0))
                {
                    hist[i] = 0.0;
                    prevg[i] = 0.0;
                }
                else
                {
                    prevg[i] = k.a0 * cd;
                    hist[i] = cd * (k.a1 * vd + k.a2 * o[i]);
                }
                if(on) o[i] = vd;
            }
        }
    }

    // h_p := dt of instance b, once every thread of the team has read the slot
    template <class Team>
    PE_DEV void integ_commit(Team const& tm, DevView const& V, int b, double dt)
    {
        if(tm.tid() == 0 && dt > 0.0)
        {
            long long const stride = integ_stride(V);
            V.tr_hist[static_cast<long long>(b) * stride + stride - 1] = dt;
        }
    }

    // the history of instance b restarts: its next step is a BE step.  only_failed: only where the instance's status is not OK (a failed
    // step has applied its companion update; the step that follows must not take the point it stored for the one before)
    template <class Team>
    PE_DEV void integ_restart(Team const& tm, DevView const& V, int b, bool only_failed)
    {
        if(tm.tid() != 0 || (only_failed && V.status[b] == 0)) return;
        long long const stride = integ_stride(V);
        V.tr_hist[static_cast<long long>(b) * stride + stride - 1] = 0.0;
    }

    // ---- truncation error of the two rules for the variable-step controller (pe_lte.hpp has the trapezoidal one and the conventions:
    // tolerances, the order-preserving integer image of the maximum, true divisions in the order of a host recomputation)
    //   BE     h^2 / 2 x'', x'' ~ 2 DD2 over (t1, b), (t2, c), (tn, x):            err_r = h^2 |DD2_r|
    //   GEAR2  x''' h^3 (1 + rho)^2 / (6 rho (1 + 2 rho)), x''' ~ 6 DD3,
    //          rho = h / (t2 - t1):                                                 err_r = h^3 (1 + rho)^2 / (rho (1 + 2 rho)) |DD3_r|
    template <class Team>
    PE_DEV unsigned long long integ_lte_partial(Team const& tm, DevView const& V, LteView const& L, int method, int b, int& nonfinite)
    {
        long long const plane = static_cast<long long>(V.batch) * V.rows, off = static_cast<long long>(b) * V.rows;
        double const* x = V.x + off;
        double const* a = L.hist + L.s0 * plane + off;
        double const* bb = L.hist + L.s1 * plane + off;
        double const* c = L.hist + L.s2 * plane + off;
        double const h10 = L.t1 - L.t0, h21 = L.t2 - L.t1, hn2 = L.tn - L.t2, h20 = L.t2 - L.t0, hn1 = L.tn - L.t1, hn0 = L.tn - L.t0;
        double const rho = L.h / h21;
        double const scale = method == TR_BE ? L.h * L.h : L.h * L.h * L.h * ((1.0 + rho) * (1.0 + rho)) / (rho * (1.0 + 2.0 * rho));
        unsigned long long u = 0;
        for(int r = tm.tid(); r < V.rows; r += tm.size())
        {
            double const xr = x[r];
            double const ax = xr < 0.0 ? -xr : xr;
            if(!(ax <= 1.7976931348623157e308)) nonfinite = 1;
            if(!L.test) continue;
            double const cr = c[r];
            double const d21 = (cr - bb[r]) / h21, dn2 = (xr - cr) / hn2;
            double const e1 = (dn2 - d21) / hn1;
            double dd = e1;
            if(method != TR_BE)
            {
                double const d10 = (bb[r] - a[r]) / h10;
                double const e0 = (d21 - d10) / h20;
                dd = (e1 - e0) / hn0;
            }
            double const ac = cr < 0.0 ? -cr : cr;
            double const big = ax > ac ? ax : ac;
            double const tol = L.trtol * (L.reltol * big + (r < V.n_nodes ? L.abstol_v : L.abstol_i));
            unsigned long long const i = lte_image(scale * (dd < 0.0 ? -dd : dd) / tol);
            u = i > u ? i : u;
        }
        return u;
    }
}  // namespace pe
