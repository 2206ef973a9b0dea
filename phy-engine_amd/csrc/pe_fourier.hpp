// pe_fourier.hpp -- Fourier analysis of transient probes (pe_hip_set_fourier / pe_hip_get_fourier), written against a "team" like
// pe_probe.hpp: the resident kernel's workgroup (tr_steps_run, PROBES = true), the one-wavefront workgroup of k_probe_arm /
// k_probe_record, or the emulation's one-thread team.  Only tid(), size() and sync() of the team are used.
//
// v(t) is the piecewise-linear interpolant through the accepted points of the armed window.  Per accepted step (t0, v0) -> (t1, v1),
// clipped to [t_start, t_end] (end values by linear interpolation), with tau = t - t_start, h = tau_b - tau_a, tau_m = tau_a + h / 2,
// vm = (va + vb) / 2, d = vb - va, w = k w0 and phi = w h / 2, the exact integrals of the interpolant over the segment are
//   int v cos(w tau) dtau = h (vm A cos(w tau_m) - d B sin(w tau_m))
//   int v sin(w tau) dtau = h (vm A sin(w tau_m) + d B cos(w tau_m))
//   A = sin(phi) / phi          B = (sin(phi) - phi cos(phi)) / (2 phi^2)
// (the Filon-trapezoidal rule, written about the segment's midpoint: one phasor and two real weights per harmonic and step, all three
// functions of k alone).  Below |phi| = FOURIER_SERIES_BELOW both weights come from their Taylor series -- B's closed form cancels like
// u / phi there; above it the closed form holds for every phi, beyond 2 pi too.  k = 0 takes A = 1, B = 0 and no libm call: h (va + vb) / 2.
//
// Work items are the pairs (configured probe, k), k fastest: with H + 1 <= 64 a wavefront of k_probe_record holds the harmonics of one
// probe, and a lane whose k does not change between its items computes phasor and weights once per step.  State per item: sum and
// compensation (TwoSum) of each integral, [batch][n_fp][H + 1][4], added in the order of the accepted steps by the one lane that owns
// the item: no atomics.  Every product that feeds a sum is an explicit fma, so that the device and a host build agree apart from libm.
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

namespace pe
{
    constexpr double FOURIER_SERIES_BELOW = 0.25;  // series: truncation < 2e-18 relative; closed form of B: error <= about 8 u absolute

    // the window opens: every accumulator of instance b is zero
    template <class Team>
    PE_DEV void fourier_arm(Team const& tm, ProbedView const& V, int b)
    {
        FourierView const& F = *V.fo;
        long long const n = static_cast<long long>(F.n_fp) * (F.H + 1) * 4;
        double* acc = F.acc + static_cast<long long>(b) * n;
        for(long long i = tm.tid(); i < n; i += tm.size()) acc[i] = 0.0;
        if(tm.tid() == 0) F.cov[b] = 0.0;
    }

    // A = sin(phi) / phi and B = (sin(phi) - phi cos(phi)) / (2 phi^2), phi != 0 or the series
    PE_DEV void fourier_weights(double phi, double& A, double& B)
    {
        if(std::fabs(phi) < FOURIER_SERIES_BELOW)
        {
            double const q = phi * phi;
            double a = 1.0 / 6227020800.0;
            a = std::fma(a, q, -1.0 / 39916800.0);
            a = std::fma(a, q, 1.0 / 362880.0);
            a = std::fma(a, q, -1.0 / 5040.0);
            a = std::fma(a, q, 1.0 / 120.0);
            a = std::fma(a, q, -1.0 / 6.0);
            A = std::fma(a, q, 1.0);
            double c = -1.0 / 1037836800.0;
            c = std::fma(c, q, 1.0 / 7983360.0);
            c = std::fma(c, q, -1.0 / 90720.0);
            c = std::fma(c, q, 1.0 / 1680.0);
            c = std::fma(c, q, -1.0 / 60.0);
            c = std::fma(c, q, 1.0 / 6.0);
            B = c * phi;
        }
        else
        {
            double s, c;
            ::sincos(phi, &s, &c);
            A = s / phi;
            B = std::fma(-phi, c, s) / (2.0 * phi * phi);
        }
    }

    // acc[0] + acc[1] += x: Knuth's TwoSum, the rounding error of every addition kept in acc[1]
    PE_DEV void fourier_add(double* acc, double x)
    {
        double const s = acc[0];
        double const t = s + x;
        double const bp = t - s;
        double const e = (s - (t - bp)) + (x - bp);
        acc[0] = t;
        acc[1] += e;
    }

    // an accepted step (t0, last[]) -> (t1, x) of an armed instance; called before last[] moves, with x complete
    template <class Team>
    PE_DEV void fourier_record(Team const& tm, ProbedView const& V, int b, double t0, double t1)
    {
        FourierView const& F = *V.fo;
        if(!(t1 > F.t_start) || !(t0 < F.t_end) || !(t1 > t0)) return;  // (wholly outside the window)
        ProbeView const& P = V.pr;
        bool const clip_a = t0 < F.t_start, clip_b = t1 > F.t_end;
        double const ta = clip_a ? F.t_start : t0, tb = clip_b ? F.t_end : t1;
        double const ra = (ta - t0) / (t1 - t0), rb = (tb - t0) / (t1 - t0);
        double const tau_a = ta - F.t_start, tau_b = tb - F.t_start;
        double const h = tau_b - tau_a, tau_m = std::fma(0.5, h, tau_a);
        double const* x = V.x + static_cast<long long>(b) * V.rows;
        double const* last = P.last + static_cast<long long>(b) * (P.n_probes + 2);
        int const K = F.H + 1, n = F.n_fp * K;
        double* acc = F.acc + static_cast<long long>(b) * n * 4;
        int kc = -1;
        double A = 1.0, B = 0.0, cm = 1.0, sm = 0.0;
        for(int i = tm.tid(); i < n; i += tm.size())
        {
            int const ip = i / K, k = i - ip * K;
            if(k != kc)  // (phasor and weights depend on k alone)
            {
                kc = k;
                if(k == 0)
                {
                    A = 1.0;
                    B = 0.0;
                    cm = 1.0;
                    sm = 0.0;
                }
                else
                {
                    double const w = static_cast<double>(k) * F.w0;
                    fourier_weights(0.5 * w * h, A, B);
                    ::sincos(w * tau_m, &sm, &cm);
                }
            }
            int const p = F.probes[ip];
            double const v0 = last[2 + p], v1 = x[P.rows[p]];
            double const d01 = v1 - v0;
            double const va = clip_a ? std::fma(d01, ra, v0) : v0, vb = clip_b ? std::fma(d01, rb, v0) : v1;
            double const pa = 0.5 * (va + vb) * A, pb = (vb - va) * B;
            double const nbs = -(pb * sm), bc = pb * cm;
            fourier_add(acc + 4 * static_cast<long long>(i), h * std::fma(pa, cm, nbs));
            fourier_add(acc + 4 * static_cast<long long>(i) + 2, h * std::fma(pa, sm, bc));
        }
        if(tm.tid() == 0) F.cov[b] += h;
    }

    // one (instance, configured probe): a, b, amp, phase of k = 0 .. H into coef [H + 1][4] and the THD, normalised by the nominal window;
    // NaN while nothing has been integrated
    PE_DEV void fourier_finish(FourierView const& F, int b, int ip, double* coef, double* thd)
    {
        int const K = F.H + 1;
        double const* acc = F.acc + (static_cast<long long>(b) * F.n_fp + ip) * K * 4;
        double const Tw = F.t_end - F.t_start;
        if(!(F.cov[b] != 0.0))
        {
            double const nan = __builtin_nan("");
            for(int i = 0; i < 4 * K; ++i) coef[i] = nan;
            *thd = nan;
            return;
        }
        double sum2 = 0.0, amp1 = 0.0;
        for(int k = 0; k < K; ++k)
        {
            double const C = acc[4 * k] + acc[4 * k + 1], S = acc[4 * k + 2] + acc[4 * k + 3];
            double const ak = (k ? 2.0 * C : C) / Tw, bk = k ? 2.0 * S / Tw : 0.0;
            double const bb = bk * bk;
            double const amp = k ? std::sqrt(std::fma(ak, ak, bb)) : std::fabs(ak);
            coef[4 * k] = ak;
            coef[4 * k + 1] = bk;
            coef[4 * k + 2] = amp;
            coef[4 * k + 3] = std::atan2(k ? -bk : 0.0, ak);
            if(k == 1) amp1 = amp;
            if(k >= 2) sum2 = std::fma(amp, amp, sum2);
        }
        *thd = std::sqrt(sum2) / amp1;
    }
}  // namespace pe
