// pe_lte.hpp -- device side of the variable-step transient (pe_hip_analyze_tr_adaptive, pe_engine_newton.cpp), written against a "team"
// like pe_probe.hpp / pe_ac_sweep.hpp: on the GPU the team is the grid slice of one instance (GridTeam of pe_kernels.hip), the emulation
// runs it with a one-thread team.  Only tid() and size() of the team are used.
//
// The controller keeps the three previous accepted solutions of every instance in a ring of three planes laid out like x
// ([slot][batch][rows], addressed by slot index, never copied) and their times on the host.  With those points (t0, a), (t1, b), (t2, c)
// and the candidate (tn, x) of a step of size h the local truncation error of the trapezoidal rule, h^3 / 12 x''', is estimated per row
// from the third divided difference (x''' ~ 6 DD3):
//   err_r = h^3 / 2 |DD3_r|      tol_r = trtol (reltol max(|x_r|, |c_r|) + abstol)      q = max_r err_r / tol_r
// abstol_v for node rows, abstol_i for branch rows.  The maximum is taken over the ORDER-PRESERVING INTEGER IMAGE of the non-negative
// double (non-negative doubles order like their bit patterns and a NaN has the largest pattern), so that a NaN is never dropped the way
// fmax drops it: a NaN anywhere in the candidate or the history arrives at the host as a NaN q, which never passes (lte_passes).
#pragma once
#include "pe_device.hpp"

#include <cmath>
#include <cstring>

#ifndef PE_DEV
    #if defined(__HIPCC__)
        #define PE_DEV __device__ __forceinline__
    #else
        #define PE_DEV inline
    #endif
#endif

namespace pe
{
    // what the host reads back per attempted step, in ONE small copy
    struct LteResult
    {
        unsigned long long q;  // image of max_r err_r / tol_r over all rows of all instances (0 when the test is off)
        int n_failed;          // instances whose status is not PE_HIP_OK after the step
        int n_nonfinite;       // != 0: some instance's candidate holds a non-finite value
        long long iters_spent; // solve_once-equivalents the step spent, summed over instances (n_iters now - n_iters of the snapshot)
    };
    struct LteView
    {
        double* hist;              // [3][batch][rows] ring of accepted solutions
        int s0, s1, s2;            // slots of the oldest .. newest of the three points
        double t0, t1, t2, tn, h;  // their times, the candidate's time, the step
        double reltol, abstol_v, abstol_i, trtol;
        int test;                  // 0: history too short or LTE test off -- only the finiteness / status part runs
        unsigned long long* q_each;  // [batch] image of every instance's own q
        long long const *iters_now, *iters_before;  // [batch] n_iters after the step / in the snapshot
        LteResult* result;
    };
    // shadow copy of the state of a step (the arrays pe_hip_checkpoint_save writes): up to 16 (destination, source, bytes) triples,
    // every size a multiple of 4 and every pointer 16-byte aligned
    struct StateCopy
    {
        void* dst[16];
        void const* src[16];
        unsigned long long bytes[16];
        int n;
    };

    PE_DEV unsigned long long lte_image(double v)
    {
        double const a = v < 0.0 ? -v : v;  // (a NaN stays a NaN)
        unsigned long long const u = __builtin_bit_cast(unsigned long long, a);
        return u & 0x7fffffffffffffffull;  // (the sign bit of a negative NaN must not outrank everything else twice over: images compare as magnitudes)
    }
    inline double lte_value(unsigned long long u)
    {
        double v;
        std::memcpy(&v, &u, sizeof(v));
        return v;
    }
    // the host's acceptance test: true only for a q that is a number and at most 1
    inline bool lte_passes(double q) { return q <= 1.0; }

    // this thread's share of instance b: image of the largest err / tol over its rows; nonfinite is set when one of its candidate values
    // is not finite (tested whether or not the LTE test runs)
    template <class Team>
    PE_DEV unsigned long long lte_partial(Team const& tm, DevView const& V, LteView const& L, int b, int& nonfinite)
    {
        long long const plane = static_cast<long long>(V.batch) * V.rows, off = static_cast<long long>(b) * V.rows;
        double const* x = V.x + off;
        double const* a = L.hist + L.s0 * plane + off;
        double const* bb = L.hist + L.s1 * plane + off;
        double const* c = L.hist + L.s2 * plane + off;
        // (true divisions, in the order a host recomputation takes them: a chain of subtractions and divisions leaves the compiler nothing to
        //  contract, so q is reproducible bit for bit from the recorded samples -- the differences cancel, a reciprocal's rounding would show)
        double const h10 = L.t1 - L.t0, h21 = L.t2 - L.t1, hn2 = L.tn - L.t2, h20 = L.t2 - L.t0, hn1 = L.tn - L.t1, hn0 = L.tn - L.t0;
        double const h3 = 0.5 * L.h * L.h * L.h;
        unsigned long long u = 0;
        for(int r = tm.tid(); r < V.rows; r += tm.size())
        {
            double const xr = x[r];
            double const ax = xr < 0.0 ? -xr : xr;
            if(!(ax <= 1.7976931348623157e308)) nonfinite = 1;
            if(!L.test) continue;
            double const cr = c[r];
            double const d10 = (bb[r] - a[r]) / h10, d21 = (cr - bb[r]) / h21, dn2 = (xr - cr) / hn2;
            double const e0 = (d21 - d10) / h20, e1 = (dn2 - d21) / hn1;
            double const dd3 = (e1 - e0) / hn0;
            double const ac = cr < 0.0 ? -cr : cr;
            double const big = ax > ac ? ax : ac;  // (either NaN makes dd3 a NaN already: q is a NaN whatever this picks)
            double const tol = L.trtol * (L.reltol * big + (r < V.n_nodes ? L.abstol_v : L.abstol_i));
            unsigned long long const i = lte_image(h3 * (dd3 < 0.0 ? -dd3 : dd3) / tol);
            u = i > u ? i : u;
        }
        return u;
    }

    // accepted candidate -> ring slot `slot` (every instance)
    template <class Team>
    PE_DEV void lte_history_push(Team const& tm, DevView const& V, double* hist, int slot)
    {
        long long const plane = static_cast<long long>(V.batch) * V.rows;
        double* dst = hist + slot * plane;
        for(long long i = tm.tid(); i < plane; i += tm.size()) dst[i] = V.x[i];
    }
}  // namespace pe
