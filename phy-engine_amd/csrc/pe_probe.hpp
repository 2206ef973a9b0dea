// pe_probe.hpp -- transient probes and streaming measurements (pe_hip_set_probes / pe_hip_arm_probes), written against a "team" like
// pe_front.hpp: on the GPU the team is the resident kernel's workgroup (tr_steps_run, PROBES = true) or the one-wavefront workgroup of
// k_probe_arm / k_probe_record; the emulation runs it with a one-thread team.  Only tid(), size() and sync() of the team are used.
//
// Per instance b, all in HBM (ProbedView::pr, pe_device.hpp): the samples [capacity] (t) and [capacity][n_probes] (v), contiguous per instance so
// that the lanes of one sample store side by side; the cursor n_rec; n_drop; the accepted steps since arming n_acc; the last accepted point
// (t_arm, t, v[probes]); two doubles of state per measure.  With (t0, v0) -> (t1, v1) two consecutive accepted points of the window:
//   MIN / MAX     state = (extreme value, time of its first occurrence)      strict compare
//   INTEG / AVG   state = (sum (t1 - t0) (v0 + v1) / 2, -)                   T = t - t_arm from `last`; AVG = INTEG / T (the host finishes)
//   RMS           state = (sum (t1 - t0) (v0^2 + v1^2) / 2, -)               RMS = sqrt(state / T)
//   CROSS         state = (time of the k-th selected crossing, crossings seen)  rise v0 < level <= v1, fall v0 > level >= v1
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
#include "pe_fourier.hpp"  // (after PE_DEV)

namespace pe
{
    // sample 0 = (t_now, x[rows]) and the initial state of every measure, at the instance's current point
    template <class Team>
    PE_DEV void probe_arm(Team const& tm, ProbedView const& V, int b)
    {
        ProbeView const& P = V.pr;
        double const* x = V.x + static_cast<long long>(b) * V.rows;
        int const np = P.n_probes;
        double const t = V.t_now[b];
        double* last = P.last + static_cast<long long>(b) * (np + 2);
        double* sv = P.v + static_cast<long long>(b) * P.capacity * np;
        for(int p = tm.tid(); p < np; p += tm.size())
        {
            double const v = x[P.rows[p]];
            last[2 + p] = v;
            sv[p] = v;
        }
        for(int m = tm.tid(); m < P.n_meas; m += tm.size())
        {
            int const kind = P.m_desc[4 * m];
            double* s = P.ms + (static_cast<long long>(b) * P.n_meas + m) * 2;
            if(kind == MEAS_MIN || kind == MEAS_MAX)
            {
                s[0] = x[P.rows[P.m_desc[4 * m + 1]]];
                s[1] = t;
            }
            else
            {
                s[0] = kind == MEAS_CROSS ? __builtin_nan("") : 0.0;
                s[1] = 0.0;
            }
        }
        if(tm.tid() == 0)
        {
            last[0] = t;
            last[1] = t;
            P.t[static_cast<long long>(b) * P.capacity] = t;
            P.n_rec[b] = 1;
            P.n_drop[b] = 0;
            P.n_acc[b] = 0;
        }
    }

    // one measure of one instance, from the last accepted point (t0, v0) to the new one (t1, v1)
    PE_DEV void measure_update(ProbeView const& P, int m, double* s, double t0, double v0, double t1, double v1)
    {
        int const kind = P.m_desc[4 * m];
        if(kind == MEAS_MIN)
        {
            if(v1 < s[0])
            {
                s[0] = v1;
                s[1] = t1;
            }
        }
        else if(kind == MEAS_MAX)
        {
            if(v1 > s[0])
            {
                s[0] = v1;
                s[1] = t1;
            }
        }
        else if(kind == MEAS_RMS)
            s[0] += (t1 - t0) * (v0 * v0 + v1 * v1) * 0.5;
        else if(kind == MEAS_CROSS)
        {
            double const level = P.m_level[m];
            int const edge = P.m_desc[4 * m + 2];
            bool const rise = v0 < level && level <= v1, fall = v0 > level && level >= v1;
            if(edge > 0 ? rise : (edge < 0 ? fall : (rise || fall)))
            {
                double const n = s[1] + 1.0;
                s[1] = n;
                if(n == static_cast<double>(P.m_desc[4 * m + 3])) s[0] = t0 + (level - v0) * (t1 - t0) / (v1 - v0);
            }
        }
        else  // INTEG, AVG
            s[0] += (t1 - t0) * (v0 + v1) * 0.5;
    }

    // an accepted TR step of an armed instance, solution x at time t1: every measure sees it; every stride-th one since arming is
    // appended as a sample while there is room, else counted in n_drop.  x must be complete (behind a team barrier) on entry.
    // FOURIER = false compiles the Fourier analysis out: the resident kernel of the probes alone is the code it was before there was one.
    template <bool FOURIER = true, class Team>
    PE_DEV void probe_record(Team const& tm, ProbedView const& V, int b, double t1)
    {
        ProbeView const& P = V.pr;
        double const* x = V.x + static_cast<long long>(b) * V.rows;
        int const np = P.n_probes;
        double* last = P.last + static_cast<long long>(b) * (np + 2);
        double const t0 = last[1];
        long long const acc = P.n_acc[b] + 1;
        int const slot = P.n_rec[b];
        bool const take = acc % P.stride == 0;
        bool const store = take && slot < P.capacity;
        for(int m = tm.tid(); m < P.n_meas; m += tm.size())
        {
            int const p = P.m_desc[4 * m + 1];
            measure_update(P, m, P.ms + (static_cast<long long>(b) * P.n_meas + m) * 2, t0, last[2 + p], t1, x[P.rows[p]]);
        }
        if constexpr(FOURIER)
            if(V.fo) fourier_record(tm, V, b, t0, t1);  // (sees every accepted step, whatever stride and capacity keep of it)
        tm.sync();  // (every lane has read the last point and the cursor before they move on)
        double* sv = P.v + (static_cast<long long>(b) * P.capacity + slot) * np;
        for(int p = tm.tid(); p < np; p += tm.size())
        {
            double const v = x[P.rows[p]];
            last[2 + p] = v;
            if(store) sv[p] = v;
        }
        if(tm.tid() == 0)
        {
            last[1] = t1;
            P.n_acc[b] = acc;
            if(store)
            {
                P.t[static_cast<long long>(b) * P.capacity + slot] = t1;
                P.n_rec[b] = slot + 1;
            }
            else if(take)
                P.n_drop[b] += 1;
        }
    }
}  // namespace pe
