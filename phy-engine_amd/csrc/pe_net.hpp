// pe_net.hpp -- multi-port network analysis (pe_engine_ac.cpp pe_hip_analyze_net / pe_hip_convert_net): the per-element code of its
// kernels, team-generic like pe_noise.hpp.  The impedance matrix of n ports comes column by column from the forward small-signal system
// A x = e_j (e_j: a unit current into port j's positive terminal, out of its negative one; every independent AC source switched off):
// Z[i][j] = x[pos_i] - x[neg_i].  The matrix of a frequency point is the same for every port, so a pass of the sweep's engine factors once
// (port 0) and solves ports 1 .. n-1 with the factors kept; the ports go one after another through one xacc / b0 pair.
//   net_rhs      port j's selector into the right-hand-side value slots of every instance of the pass, and into the refinement's b0
//   net_gather   column j of Z[point][instance] from the refined solution
//   net_convert  Y = Z^-1 and S = D^-1 (Z - Z0) (Z + Z0)^-1 D of one (point, instance) matrix, each with a status of its own
// pe_kernels.hip runs net_rhs / net_gather with a grid team (k_net_rhs, k_net_gather) and net_convert with one wavefront per matrix
// (k_net_convert: the 8 x 16 augmented matrix two elements per lane, cross-lane shuffles); builds without HIP run everything with a
// one-thread team that holds all 128 elements (the serial launchers at the end of pe_engine_ac.cpp, scripts/net_kernel_host.cpp).
#pragma once
#include "pe_ac_sweep.hpp"
#include "pe_device.hpp"

#include <cmath>

namespace pe
{
    constexpr int NET_MAX_PORTS = 8;               // PE_HIP_NET_MAX_PORTS (checked against the C header in pe_engine_ac.cpp)
    constexpr int NET_AUG = 2 * NET_MAX_PORTS;     // columns of the augmented matrix [M | I]
    constexpr int NET_ELEMS = NET_MAX_PORTS * NET_AUG;
    constexpr int NET_MATS_PER_GROUP = 4;          // k_net_convert: one wavefront per matrix, four to a workgroup
    constexpr int NET_ERR_SINGULAR = -3;           // PE_HIP_ERR_SINGULAR (checked likewise)
    constexpr double NET_EPS = 2.220446049250313e-16;    // 2^-52
    constexpr double NET_DBL_MAX = 1.7976931348623157e308;

    // What the network kernels read and write besides the sweep engine's view (kept out of DevView like NoiseView).  Device memory.
    struct NetView
    {
        int n_ports;
        int P;                // points per pass of the sweep's engine: its instance q = b * P + p
        int n_inst;           // circuit batch
        int n_half;           // N: rows of the complex system (the real half of the engine's 2N)
        int rhs0;             // first of the 2N right-hand-side slots of the engine's value vector
        int const* pos;       // [n_ports] rows of every port (-1: ground)
        int const* neg;
        double const* z0;     // [n_ports] reference resistances
        int const* point;     // [P] the caller's index of each point of this pass, -1: unused (AcSweepView::point)
        double const* xacc;   // [n_inst * P][2N] refined solution (AcSweepView::xacc)
        double* b0;           // [n_inst * P][2N] right-hand side as stamped (AcSweepView::b0)
        double* z_re;         // [n_points][n_inst][n_ports][n_ports] in the caller's point order, entry [i][j]: port i's response to port j
        double* z_im;
    };

    // right-hand side of instance q for port j: +1 at pos_j, -1 at neg_j in the real half, zero elsewhere (a ground terminal matches no
    // row: nothing is written for it).  The slots held the selector of the port before, or the residual its refinement left there.
    // The copy into b0 is not what the refinement reads in the end: ac_accumulate_each(first) takes b0 from the stamped V.rhs right after
    // the solve and overwrites it with the same values.  It is written here so that b0 is this port's right-hand side from the moment the
    // slots are, whatever runs in between.
    template <class Team>
    PE_DEV void net_rhs(Team const& tm, DevView const& V, NetView const& Z, int q, int j)
    {
        int const pos = Z.pos[j], neg = Z.neg[j];
        double* rhs = V.dv + static_cast<long long>(q) * V.dv_len + Z.rhs0;
        double* b0 = Z.b0 + static_cast<long long>(q) * V.rows;
        for(int r = tm.tid(); r < V.rows; r += tm.size())
        {
            double const v = (r == pos ? 1.0 : 0.0) - (r == neg ? 1.0 : 0.0);
            rhs[r] = v;
            b0[r] = v;
        }
    }

    // column j of the impedance matrix of instance q: x[pos_i] - x[neg_i] of every port i, a ground terminal reading 0; an unused slot of
    // the pass (point -1) stores nothing
    template <class Team>
    PE_DEV void net_gather(Team const& tm, DevView const& V, NetView const& Z, int q, int j)
    {
        int const b = q / Z.P;
        int const pt = Z.point[q - b * Z.P];
        if(pt < 0) return;
        double const* x = Z.xacc + static_cast<long long>(q) * V.rows;
        long long const o = (static_cast<long long>(pt) * Z.n_inst + b) * Z.n_ports * Z.n_ports;
        for(int i = tm.tid(); i < Z.n_ports; i += tm.size())
        {
            int const p = Z.pos[i], n = Z.neg[i];
            Z.z_re[o + static_cast<long long>(i) * Z.n_ports + j] = (p >= 0 ? x[p] : 0.0) - (n >= 0 ? x[n] : 0.0);
            Z.z_im[o + static_cast<long long>(i) * Z.n_ports + j] = (p >= 0 ? x[Z.n_half + p] : 0.0) - (n >= 0 ? x[Z.n_half + n] : 0.0);
        }
    }

    // ---- the dense conversion.  A `Wave` owns one matrix: LANES lanes hold EPL elements each of the NET_MAX_PORTS x NET_AUG augmented
    // matrix, element e of lane l being number g = l + e * LANES, row g / NET_AUG, column g % NET_AUG.  What it provides:
    //   lane()              this lane
    //   get(a, row, col)    element (row, col) of the distributed array a, whichever lane holds it (row, col may differ per lane)
    //   argmax(m, r)        the largest m of the wave and its r; among equal m the smallest r
    //   nanmax(v)           NaN-keeping maximum over the wave
    //   any(f)              f of some lane
    // Every read of a phase precedes its writes (a one-lane wave runs the element loops serially).  Rows and columns past n are never
    // read for a decision: a smaller matrix is handled by bounds, not by padding.

    // q = a / b (Smith's method: no intermediate overflow for representable quotients)
    PE_DEV void net_cdiv(double ar, double ai, double br, double bi, double& qr, double& qi)
    {
        if(fabs(br) >= fabs(bi))
        {
            double const t = bi / br, d = br + bi * t;
            qr = (ar + ai * t) / d;
            qi = (ai - ar * t) / d;
        }
        else
        {
            double const t = br / bi, d = br * t + bi;
            qr = (ar * t + ai) / d;
            qi = (ai * t - ar) / d;
        }
    }

    // [M | I] -> [. | M^-1] in place by Gauss-Jordan elimination with partial pivoting by modulus.  False: no inverse -- an entry of M is
    // not finite, or a pivot is not finite or has |pivot| <= n 2^-52 max |M_ij|, or the result is not finite.
    template <class Wave>
    PE_DEV bool net_invert(Wave const& w, int n, double (&re)[Wave::EPL], double (&im)[Wave::EPL])
    {
        double mx = 0.0;
#pragma unroll
        for(int e = 0; e < Wave::EPL; ++e)
        {
            int const g = w.lane() + e * Wave::LANES, r = g / NET_AUG, c = g % NET_AUG;
            if(r < n && c < n) mx = ac_nanmax(mx, hypot(re[e], im[e]));
        }
        mx = w.nanmax(mx);
        if(!(mx <= NET_DBL_MAX)) return false;
        double const thr = static_cast<double>(n) * NET_EPS * mx;
        for(int k = 0; k < n; ++k)
        {
            // pivot: the largest modulus of column k from row k on (the first of equal ones)
            double bm = -1.0;
            int br = k;
#pragma unroll
            for(int e = 0; e < Wave::EPL; ++e)
            {
                int const g = w.lane() + e * Wave::LANES, r = g / NET_AUG, c = g % NET_AUG;
                if(c != k || r < k || r >= n) continue;
                double const m = hypot(re[e], im[e]);
                if(m > bm)
                {
                    bm = m;
                    br = r;
                }
            }
            w.argmax(bm, br);
            double const pr = w.get(re, br, k), pi = w.get(im, br, k);
            double const pm = hypot(pr, pi);
            if(!(pm <= NET_DBL_MAX) || pm <= thr) return false;  // (the same on every lane)
            // reads: the pivot row and row k in this element's column, and this element's row (after the exchange) in column k
            double vpr[Wave::EPL], vpi[Wave::EPL], vkr[Wave::EPL], vki[Wave::EPL], mr[Wave::EPL], mi[Wave::EPL];
#pragma unroll
            for(int e = 0; e < Wave::EPL; ++e)
            {
                int const g = w.lane() + e * Wave::LANES, r = g / NET_AUG, c = g % NET_AUG;
                int const rs = r == k ? br : (r == br ? k : r);
                vpr[e] = w.get(re, br, c);
                vpi[e] = w.get(im, br, c);
                vkr[e] = w.get(re, k, c);
                vki[e] = w.get(im, k, c);
                mr[e] = w.get(re, rs, k);
                mi[e] = w.get(im, rs, k);
            }
            // writes: rows k and br exchanged, every other row minus its multiple of the pivot row (its column k exactly zero)
#pragma unroll
            for(int e = 0; e < Wave::EPL; ++e)
            {
                int const g = w.lane() + e * Wave::LANES, r = g / NET_AUG, c = g % NET_AUG;
                double cr = r == k ? vpr[e] : (r == br ? vkr[e] : re[e]);
                double ci = r == k ? vpi[e] : (r == br ? vki[e] : im[e]);
                if(r != k && r < n)
                {
                    if(c == k) cr = ci = 0.0;
                    else
                    {
                        double fr, fi;
                        net_cdiv(mr[e], mi[e], pr, pi, fr, fi);
                        cr -= fr * vpr[e] - fi * vpi[e];
                        ci -= fr * vpi[e] + fi * vpr[e];
                    }
                }
                re[e] = cr;
                im[e] = ci;
            }
        }
        // every row by its diagonal
        double dr[Wave::EPL], di[Wave::EPL];
#pragma unroll
        for(int e = 0; e < Wave::EPL; ++e)
        {
            int const g = w.lane() + e * Wave::LANES, r = g / NET_AUG;
            dr[e] = w.get(re, r, r);
            di[e] = w.get(im, r, r);
        }
        bool bad = false;
#pragma unroll
        for(int e = 0; e < Wave::EPL; ++e)
        {
            int const g = w.lane() + e * Wave::LANES, r = g / NET_AUG, c = g % NET_AUG;
            if(r >= n || c < NET_MAX_PORTS || c - NET_MAX_PORTS >= n) continue;
            double qr, qi;
            net_cdiv(re[e], im[e], dr[e], di[e], qr, qi);
            re[e] = qr;
            im[e] = qi;
            bad = bad || !(fabs(qr) <= NET_DBL_MAX) || !(fabs(qi) <= NET_DBL_MAX);
        }
        return !w.any(bad);
    }

    // Y, S and their statuses of ONE matrix (the pointers address it: [n][n] each; z0: [n]; an output may be null).  The result depends on
    // the matrix alone.
    // S = D^-1 (Z - Z0) W D with W = (Z + Z0)^-1 is formed as I - 2 D W D (Z - Z0 = (Z + Z0) - 2 Z0): it needs W only, which exists
    // where a port on a node held by a voltage source makes Z itself singular.
    template <class Wave>
    PE_DEV void net_convert(Wave const& w, int n, double const* z_re, double const* z_im, double const* z0, double* y_re, double* y_im, double* s_re,
                            double* s_im, int* y_status, int* s_status)
    {
        double const nan = __builtin_nan("");
        for(int which = 0; which < 2; ++which)
        {
            double re[Wave::EPL], im[Wave::EPL];
#pragma unroll
            for(int e = 0; e < Wave::EPL; ++e)
            {
                int const g = w.lane() + e * Wave::LANES, r = g / NET_AUG, c = g % NET_AUG;
                re[e] = im[e] = 0.0;
                if(r >= n) continue;
                if(c < n)
                {
                    re[e] = z_re[r * n + c] + ((which == 1 && r == c) ? z0[r] : 0.0);
                    im[e] = z_im[r * n + c];
                }
                else if(c - NET_MAX_PORTS == r)
                    re[e] = 1.0;
            }
            bool const ok = net_invert(w, n, re, im);
            double* o_re = which == 0 ? y_re : s_re;
            double* o_im = which == 0 ? y_im : s_im;
#pragma unroll
            for(int e = 0; e < Wave::EPL; ++e)
            {
                int const g = w.lane() + e * Wave::LANES, r = g / NET_AUG, c = g % NET_AUG - NET_MAX_PORTS;
                if(r >= n || c < 0 || c >= n) continue;
                double vr = re[e], vi = im[e];
                if(which == 1)
                {
                    double const f = 2.0 * sqrt(z0[r]) * sqrt(z0[c]);
                    vr = (r == c ? 1.0 : 0.0) - f * vr;
                    vi = -f * vi;
                }
                if(o_re) o_re[r * n + c] = ok ? vr : nan;
                if(o_im) o_im[r * n + c] = ok ? vi : nan;
            }
            int* const o_status = which == 0 ? y_status : s_status;
            if(w.lane() == 0 && o_status) *o_status = ok ? 0 : NET_ERR_SINGULAR;
        }
    }

    // the wave of a one-thread team: it holds every element
    struct NetSerialWave
    {
        static constexpr int LANES = 1, EPL = NET_ELEMS;
        int lane() const { return 0; }
        double get(double const (&a)[EPL], int row, int col) const { return a[row * NET_AUG + col]; }
        void argmax(double&, int&) const {}
        double nanmax(double v) const { return v; }
        bool any(bool f) const { return f; }
    };
}  // namespace pe
