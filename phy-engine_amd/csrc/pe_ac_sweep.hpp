// pe_ac_sweep.hpp -- frequency-batched small-signal AC (pe_engine_ac.cpp pe_hip_analyze_ac_sweep): the per-element code of the sweep's
// kernels, team-generic like ac_residual in pe_front.hpp.  The points of one pass are extra instances of the real-equivalent system:
// AC-engine instance q = b * P + p is circuit instance b at point p of the pass.  pe_kernels.hip runs this text with a grid team
// (k_ac_sweep_fill / k_ac_residual_each / k_ac_accumulate_each / k_ac_sweep_gather), builds without HIP with a one-thread team (the
// serial launchers at the end of pe_engine_ac.cpp).  Only tid() and size() of the team are used.
#pragma once
#include "pe_device.hpp"

#include <cmath>

#ifndef PE_DEV
    #if defined(__HIPCC__)
        #define PE_DEV __device__ __forceinline__
    #else
        #define PE_DEV inline
    #endif
#endif

// (also called by the host: the sweep matches its pivot orders on the values of instance 0)
#if defined(__HIPCC__)
    #define PE_AC_HD __host__ __device__ __forceinline__
#else
    #define PE_AC_HD inline
#endif

namespace pe
{
    // how a value of the AC value vector follows omega (pe::AcSlot, pe_ac.hpp: every slot is constant or omega x a per-instance constant)
    enum AcScale : int
    {
        AC_CONST = 0,      // base
        AC_OMEGA = 1,      // base * omega                      (C_W, KL_W11 / 12 / 22)
        AC_OMEGA_ZERO = 2  // base * omega, +0.0 at omega == 0  (L_W, D_WC: the host writes +0.0 there whatever the sign of the parameter)
    };

    // What the sweep's kernels read and write besides the AC engine's view (kept out of DevView: its size is part of k_tr_steps' register
    // allocation).  All pointers are device memory.
    struct AcSweepView
    {
        int P;                  // points per pass: the AC engine's batch is (circuit batch) x P
        int n_inst;             // circuit batch
        int rhs0;               // first of the 2N right-hand-side slots of the AC value vector = length of one base vector
        double const* base;     // [n_inst][rhs0] value vector at omega = 1 (fill_ac_values), DV_ONE / DV_GMIN included
        int const* scale;       // [rhs0] AcScale of every value
        double const* omega;    // [P] omega of the points of this pass (unused points repeat the last one)
        int const* point;       // [P] the caller's index of each point of this pass, -1: unused (solved, not gathered)
        int const* b_ptr0;      // [2N + 1] the right-hand-side lists of the AC system over the value vector (sign: low bit of the source)
        int const* b_src0;
        double* xacc;           // [n_inst * P][2N] accumulated solution
        double* b0;             // [n_inst * P][2N] right-hand side as stamped
        double* worst;          // [n_inst * P] componentwise backward error of the last residual
        int* n_above;           // one int: instances whose backward error is above the refinement threshold (NaN counts)
        int n_keep;             // kept rows per point (n_rows == 0: N, every row)
        int const* keep;        // [n_keep] rows of x, or null: all rows
        int n_half;             // N: rows of the complex system
        double* res_re;         // [n_points][n_inst][n_keep] results in the caller's point order
        double* res_im;
    };

    constexpr double AC_REFINE_TOL = 4.0e-16;  // backward error at rounding level (pe_hip_analyze_ac stops refining there)

    PE_AC_HD double ac_sweep_value(double base, int scale, double omega)
    {
        if(scale == AC_CONST) return base;
        if(scale == AC_OMEGA_ZERO && omega == 0.0) return 0.0;
        return base * omega;  // (the product the host forms: omega * C, cd * omega)
    }

    // value vector of AC-engine instance q: the values below rhs0 from the base vector of its circuit instance, the 2N right-hand-side slots
    // gathered through the original lists.  One pass over the slot index: consecutive threads store consecutive doubles.
    template <class Team>
    PE_DEV void ac_sweep_fill(Team const& tm, DevView const& V, AcSweepView const& S, int q)
    {
        int const b = q / S.P;
        double const omega = S.omega[q - b * S.P];
        double const* base = S.base + static_cast<long long>(b) * S.rhs0;
        double* dv = V.dv + static_cast<long long>(q) * V.dv_len;
        for(int i = tm.tid(); i < V.dv_len; i += tm.size())
        {
            if(i < S.rhs0)
            {
                dv[i] = ac_sweep_value(base[i], S.scale[i], omega);
                continue;
            }
            int const r = i - S.rhs0;
            double acc = 0.0;
            int const e1 = S.b_ptr0[r + 1];
            for(int e = S.b_ptr0[r]; e < e1; ++e)
            {
                int const s = S.b_src0[e] >> 1;
                double const v = ac_sweep_value(base[s], S.scale[s], omega);
                acc = (S.b_src0[e] & 1) ? acc - v : acc + v;
            }
            dv[i] = acc;
        }
    }

    // NaN-keeping maximum of non-negative values (fmax would drop the NaN a broken instance must show)
    PE_DEV double ac_nanmax(double a, double b) { return (b > a || b != b) ? b : a; }
    // (also the host's test in pe_hip_analyze_ac: one rule on both paths, a NaN needs refinement)
    PE_AC_HD bool ac_needs_refinement(double worst) { return !(worst <= AC_REFINE_TOL); }

    // ac_residual (pe_front.hpp) of instance q with a NaN-keeping maximum: r = b0 - A xacc into the right-hand-side value slots, returns
    // this thread's worst componentwise backward error
    template <class Team>
    PE_DEV double ac_residual_each(Team const& tm, DevView const& V, AcSweepView const& S, int q)
    {
        double const* a = V.aval + static_cast<long long>(q) * V.nnzA;
        double const* x = S.xacc + static_cast<long long>(q) * V.rows;
        double const* b0 = S.b0 + static_cast<long long>(q) * V.rows;
        double* dv = V.dv + static_cast<long long>(q) * V.dv_len;
        double worst = 0.0;
        for(int r = tm.tid(); r < V.rows; r += tm.size())
        {
            double acc = b0[r], mag = fabs(acc);
            int const e1 = V.csr_rp[r + 1];
            for(int e = V.csr_rp[r]; e < e1; ++e)
            {
                double const t = a[V.slot_e ? V.slot_e[e] : e] * x[V.csr_ci[e]];
                acc -= t;
                mag += fabs(t);
            }
            dv[S.rhs0 + r] = acc;
            worst = ac_nanmax(worst, fabs(acc) / (mag > 0.0 ? mag : 1.0));
        }
        return worst;
    }

    // xacc = first ? x : xacc + x for the instances that still need it (first: every instance, and b0 = the stamped right-hand side)
    template <class Team>
    PE_DEV void ac_accumulate_each(Team const& tm, DevView const& V, AcSweepView const& S, int q, bool first)
    {
        if(!first && !ac_needs_refinement(S.worst[q])) return;
        long long const o = static_cast<long long>(q) * V.rows;
        for(int r = tm.tid(); r < V.rows; r += tm.size())
        {
            if(first)
            {
                S.xacc[o + r] = V.x[o + r];
                S.b0[o + r] = V.rhs[o + r];
            }
            else
                S.xacc[o + r] += V.x[o + r];
        }
    }

    // the kept rows of instance q, real and imaginary half, into the result buffer at the caller's index of its point
    template <class Team>
    PE_DEV void ac_sweep_gather(Team const& tm, DevView const& V, AcSweepView const& S, int q)
    {
        int const b = q / S.P;
        int const pt = S.point[q - b * S.P];
        if(pt < 0) return;
        double const* x = S.xacc + static_cast<long long>(q) * V.rows;
        long long const o = (static_cast<long long>(pt) * S.n_inst + b) * S.n_keep;
        for(int k = tm.tid(); k < S.n_keep; k += tm.size())
        {
            int const r = S.keep ? S.keep[k] : k;
            S.res_re[o + k] = x[r];
            S.res_im[o + k] = x[S.n_half + r];
        }
    }
}  // namespace pe
