// pe_pz.hpp -- pole-zero analysis (pe_engine_ac.cpp pe_hip_analyze_pz / pe_hip_eig_hessenberg): the per-element code of its kernels, team- and
// wave-generic like pe_net.hpp.  The small-signal matrix is affine in omega, A(s) = G + s B with real G, B; at the shift s0 = j omega0 the
// engine's real-equivalent system [[G, -omega0 B], [omega0 B, G]] IS A0 = G + j omega0 B, and its lower-left block is omega0 B.  The poles
// are s = s0 - omega0 / theta' over the eigenvalues theta' of M' = A0^-1 (omega0 B), found by Arnoldi on the kept factors of A0 (one pass of
// one point of the sweep body, every Arnoldi step one right-hand side); the zeros of H(s) = c^T A(s)^-1 b the same with the rank-one
// correction M'_z v = w - z (c^T w) / (c^T z), w = M' v, z = A0^-1 b.
//   pz_bmul   (omega0 B) v of every instance into the right-hand-side value slots and the refinement's b0; zeros for a parked instance
//   pz_orth   after the refined solve: rank-one correction (zeros), classical Gram-Schmidt twice against the basis, norm, breakdown test,
//             Hessenberg column, the normalised vector.  Sums go through the team's fixed tree: no atomics, an instance's numbers depend
//             on that instance alone
//   pz_ritz   eigenvalues of one upper Hessenberg matrix (complex single-shift QR, Wilkinson shifts, deflation), the last component of
//             every unit eigenvector, then the theta' floor, the map to s, err_est, the sort and the converged run
// pe_kernels.hip runs pz_bmul with a grid team (k_pz_bmul), pz_orth with one workgroup per instance (k_pz_orth), pz_ritz with one wavefront
// per matrix and the matrix in LDS (k_pz_ritz); builds without HIP run everything with a one-thread team and a one-lane wave on a heap
// buffer (the serial launchers at the end of pe_engine_ac.cpp, scripts/pz_kernel_host.cpp).
#pragma once
#include "pe_ac_sweep.hpp"
#include "pe_device.hpp"
#include "pe_net.hpp"

#include <cmath>

namespace pe
{
    constexpr int PZ_MAX_KRYLOV = 64;          // PE_HIP_PZ_MAX_KRYLOV (checked against the C header in pe_engine_ac.cpp)
    constexpr int PZ_QR_SWEEPS_PER_EIG = 30;   // QR iteration cap: 30 m sweeps for a matrix of order m (LAPACK's zlahqr allows 30 per eigenvalue)
    constexpr int PZ_ERR_SINGULAR = -3;        // PE_HIP_ERR_SINGULAR (checked likewise)
    constexpr int PZ_ERR_NO_CONVERGENCE = -4;  // PE_HIP_ERR_NO_CONVERGENCE
    constexpr double PZ_EPS = 2.220446049250313e-16;
    constexpr double PZ_DBL_MAX = 1.7976931348623157e308;
    constexpr int PZ_ORTH_THREADS = 256;       // k_pz_orth: one workgroup per instance
    constexpr int PZ_PARKED_COMPLETE = 1;      // PzView::parked: the Krylov space is invariant
    constexpr int PZ_PARKED_FAILED = 2;        // ... a vector of the instance was not finite, or H(s0) is 0 or not finite (zeros)

    // doubles of LDS (or heap) pz_ritz needs for a matrix of order m: m + 1 rows (the last: row m of the accumulated unitary factor) of
    // m + 1 columns (one of padding: consecutive rows start in different banks), real and imaginary plane, and five vectors of m
    PE_AC_HD int pz_ritz_doubles(int m) { return 2 * (m + 1) * (m + 1) + 5 * m; }

    // What the Arnoldi kernels read and write besides the sweep engine's view.  Device memory.  The engine runs one point per pass: its
    // instance q is circuit instance q.
    struct PzView
    {
        int n_half;           // N: rows of the complex system
        int rhs0;             // first of the 2N right-hand-side slots of the engine's value vector
        int m_max;            // max_krylov of the call
        int in_pos, in_neg, out_pos, out_neg;  // rows of b and c (-1: ground); read for zeros only
        double breakdown_tol;
        double const* xacc;   // [n_inst][2N] refined solution (AcSweepView::xacc)
        double* b0;           // [n_inst][2N] right-hand side as stamped (AcSweepView::b0)
        double* basis;        // [n_inst][m_max + 1][2N]
        double* h_re;         // [n_inst][m_max + 1][m_max]: column k the coefficients of step k + 1, entry [k + 1][k] the norm left
        double* h_im;
        double* zvec;         // [n_inst][2N] z = A0^-1 b
        double* gain;         // [n_inst][2] H(s0) = c^T z
        int* steps;           // [n_inst] Arnoldi steps taken = order of the instance's Hessenberg matrix
        int* parked;          // [n_inst] 0: running, PZ_PARKED_*
    };

    // the start vector's pre-image r: a fixed function of the row index, the same for every instance and every run
    PE_DEV void pz_start(int i, double& re, double& im)
    {
        re = 1.0 + static_cast<double>((i * 7 + 3) % 11) * 0.0625;
        im = static_cast<double>((i * 5 + 1) % 13) * 0.0625;
    }

    // right-hand side of instance q: (omega0 B) v from the lower-left block of the matrix as the engine assembled it, applied to both
    // halves of v = basis vector `src` (src < 0: r).  Written into the value slots and into b0 for the reason net_rhs gives.
    template <class Team>
    PE_DEV void pz_bmul(Team const& tm, DevView const& V, PzView const& Z, int q, int src)
    {
        int const N = Z.n_half;
        double* rhs = V.dv + static_cast<long long>(q) * V.dv_len + Z.rhs0;
        double* b0 = Z.b0 + static_cast<long long>(q) * V.rows;
        bool const parked = Z.parked[q] != 0;
        double const* a = V.aval + static_cast<long long>(q) * V.nnzA;
        double const* v = src < 0 ? nullptr : Z.basis + (static_cast<long long>(q) * (Z.m_max + 1) + src) * V.rows;
        for(int r = tm.tid(); r < N; r += tm.size())
        {
            double sr = 0.0, si = 0.0;
            if(!parked)
            {
                int const e1 = V.csr_rp[N + r + 1];
                for(int e = V.csr_rp[N + r]; e < e1; ++e)
                {
                    int const c = V.csr_ci[e];
                    if(c >= N) continue;
                    double const av = a[V.slot_e ? V.slot_e[e] : e];
                    double vr, vi;
                    if(v)
                    {
                        vr = v[c];
                        vi = v[N + c];
                    }
                    else
                        pz_start(c, vr, vi);
                    sr += av * vr;
                    si += av * vi;
                }
            }
            rhs[r] = sr;
            b0[r] = sr;
            rhs[N + r] = si;
            b0[N + r] = si;
        }
    }

    // x[pos] - x[neg] of a complex vector stored as two halves
    PE_DEV void pz_pick(double const* x, int N, int pos, int neg, double& re, double& im)
    {
        re = (pos >= 0 ? x[pos] : 0.0) - (neg >= 0 ? x[neg] : 0.0);
        im = (pos >= 0 ? x[N + pos] : 0.0) - (neg >= 0 ? x[N + neg] : 0.0);
    }

    // z = A0^-1 b of instance q from the refined solution, and H(s0) = c^T z.  H(s0) == 0 or not finite: no zeros for this instance.
    template <class Team>
    PE_DEV void pz_store_z(Team const& tm, DevView const& V, PzView const& Z, int q)
    {
        int const N = Z.n_half;
        double const* x = Z.xacc + static_cast<long long>(q) * V.rows;
        double* z = Z.zvec + static_cast<long long>(q) * V.rows;
        for(int r = tm.tid(); r < V.rows; r += tm.size()) z[r] = x[r];
        if(tm.tid() == 0)
        {
            double gr, gi;
            pz_pick(x, N, Z.out_pos, Z.out_neg, gr, gi);
            Z.gain[2 * q] = gr;
            Z.gain[2 * q + 1] = gi;
        }
    }

    // One Arnoldi step of instance q after the refined solve of M' v_{k-1} (k = 0: of M' r, the start vector -- it is only normalised).
    // The team provides tid(), size(), sync(), sum2(a, b): the sums of a and of b over the team, on every thread, in a fixed order, and
    // keep(j, re, im) / kept(j, re, im): PZ_MAX_KRYLOV complex numbers every thread can read back after a sync().
    // The working vector lives in basis slot k.  A parked instance is left alone: nothing of it is overwritten.
    template <class Team>
    PE_DEV void pz_orth(Team const& tm, DevView const& V, PzView const& Z, int q, int k, bool zeros)
    {
        if(Z.parked[q] != 0) return;
        int const N = Z.n_half;
        double const* x = Z.xacc + static_cast<long long>(q) * V.rows;
        double* base = Z.basis + static_cast<long long>(q) * (Z.m_max + 1) * V.rows;
        double* w = base + static_cast<long long>(k) * V.rows;
        // w = M' v, for zeros minus z (c^T w) / (c^T z)
        double fr = 0.0, fi = 0.0;
        bool bad = false;
        if(zeros)
        {
            double dr, di;
            pz_pick(x, N, Z.out_pos, Z.out_neg, dr, di);
            double const gr = Z.gain[2 * q], gi = Z.gain[2 * q + 1];
            bad = !(fabs(gr) <= PZ_DBL_MAX) || !(fabs(gi) <= PZ_DBL_MAX) || (gr == 0.0 && gi == 0.0);
            if(!bad) net_cdiv(dr, di, gr, gi, fr, fi);
        }
        double const* z = Z.zvec + static_cast<long long>(q) * V.rows;
        double n2 = 0.0, unused = 0.0;
        for(int i = tm.tid(); i < N; i += tm.size())
        {
            double wr = x[i], wi = x[N + i];
            if(zeros && !bad)
            {
                wr -= fr * z[i] - fi * z[N + i];
                wi -= fr * z[N + i] + fi * z[i];
            }
            w[i] = wr;
            w[N + i] = wi;
            n2 += wr * wr + wi * wi;
        }
        tm.sum2(n2, unused);
        double const norm_w = sqrt(n2);  // (before orthogonalisation: what the breakdown test compares with)
        if(bad || !(norm_w <= PZ_DBL_MAX))
        {
            if(tm.tid() == 0) Z.parked[q] = PZ_PARKED_FAILED;
            return;
        }
        double* hr = Z.h_re + static_cast<long long>(q) * (Z.m_max + 1) * Z.m_max;
        double* hi = Z.h_im + static_cast<long long>(q) * (Z.m_max + 1) * Z.m_max;
        // classical Gram-Schmidt, twice: every coefficient of a pass from the same w, then one update; the second pass's coefficients are
        // added to the first's.  <v, w> = sum conj(v_i) w_i.
        for(int pass = 0; pass < 2 && k > 0; ++pass)
        {
            for(int j = 0; j < k; ++j)
            {
                double const* v = base + static_cast<long long>(j) * V.rows;
                double cr = 0.0, ci = 0.0;
                for(int i = tm.tid(); i < N; i += tm.size())
                {
                    cr += v[i] * w[i] + v[N + i] * w[N + i];
                    ci += v[i] * w[N + i] - v[N + i] * w[i];
                }
                tm.sum2(cr, ci);
                if(tm.tid() == 0)
                {
                    hr[j * Z.m_max + (k - 1)] = pass == 0 ? cr : hr[j * Z.m_max + (k - 1)] + cr;
                    hi[j * Z.m_max + (k - 1)] = pass == 0 ? ci : hi[j * Z.m_max + (k - 1)] + ci;
                }
                tm.keep(j, cr, ci);  // (where every thread reads it again in the update below: kept(), after a sync())
            }
            tm.sync();
            for(int i = tm.tid(); i < N; i += tm.size())
            {
                double wr = w[i], wi = w[N + i];
                for(int j = 0; j < k; ++j)
                {
                    double const* v = base + static_cast<long long>(j) * V.rows;
                    double cr, ci;
                    tm.kept(j, cr, ci);
                    wr -= cr * v[i] - ci * v[N + i];
                    wi -= cr * v[N + i] + ci * v[i];
                }
                w[i] = wr;
                w[N + i] = wi;
            }
            tm.sync();
        }
        double m2 = 0.0;
        for(int i = tm.tid(); i < N; i += tm.size()) m2 += w[i] * w[i] + w[N + i] * w[N + i];
        tm.sum2(m2, unused);
        double const h = sqrt(m2);
        bool const broke = !(h > Z.breakdown_tol * norm_w);  // (a NaN parks the instance as well)
        if(tm.tid() == 0)
        {
            if(k > 0)
            {
                hr[k * Z.m_max + (k - 1)] = h;
                hi[k * Z.m_max + (k - 1)] = 0.0;
            }
            Z.steps[q] = k;
            if(broke) Z.parked[q] = (h == h) ? PZ_PARKED_COMPLETE : PZ_PARKED_FAILED;
        }
        if(broke) return;
        double const inv = 1.0 / h;
        for(int i = tm.tid(); i < N; i += tm.size())
        {
            w[i] *= inv;
            w[N + i] *= inv;
        }
    }

    // ---- the dense eigenvalue solver.  A `Wave` owns one matrix in memory all its lanes address (LDS): lane(), lanes(), sync() -- every
    // lane's stores before it are visible to every lane after it.  The lanes run in lock-step and take every decision from the same
    // values, so the control flow is the same on all of them.

    PE_DEV double pz_abs1(double re, double im) { return fabs(re) + fabs(im); }

    // principal square root of a complex number
    PE_DEV void pz_csqrt(double ar, double ai, double& sr, double& si)
    {
        double const m = hypot(ar, ai);
        if(m == 0.0)
        {
            sr = si = 0.0;
            return;
        }
        if(ar >= 0.0)
        {
            sr = sqrt(0.5 * (m + ar));
            si = ai / (2.0 * sr);
        }
        else
        {
            double const t = sqrt(0.5 * (m - ar));
            sr = fabs(ai) / (2.0 * t);
            si = ai < 0.0 ? -t : t;
        }
    }

    struct PzRitzView
    {
        int n_mats;
        int m;                    // order of every matrix (steps == nullptr), else the most an instance can have (m_max)
        int const* steps;         // [n_mats] order of each matrix, or null
        int const* parked;        // [n_mats] or null: PZ_PARKED_COMPLETE makes err_est 0, PZ_PARKED_FAILED leaves the outputs NaN
        double const* h_re;       // matrix i at h_re + i * mat_stride, entry (r, c) at r * ld + c
        double const* h_im;
        long long mat_stride;
        int ld;
        double* theta_re;         // raw results [n_mats][m] (or null): eigenvalues in the order of the Schur form's diagonal and the last
        double* theta_im;         // component of each unit eigenvector
        double* last_re;
        double* last_im;
        double omega0, theta_floor, tol;
        double* s_re;             // mapped results [n_mats][m] (or null), padded with NaN: s = j omega0 - omega0 / theta' sorted by
        double* s_im;             // |s - s0| ascending (ties: larger imaginary part first), err_est
        double* s_err;
        int* n_found;             // [n_mats]
        int* n_conv;              // [n_mats] length of the leading converged run
        int* status;              // [n_mats] 0, PZ_ERR_SINGULAR (an entry is not finite), PZ_ERR_NO_CONVERGENCE (the QR cap)
    };

    // Schur form of the upper Hessenberg matrix in H (rows 0 .. m-1; row m: the last row of the unitary factor, e_m^T on entry) by explicit
    // single-shift QR sweeps on the active block [lo, hi]: the left rotations one after another, each applied by column (lane j owns column
    // j), then every row takes all right rotations on its own (lane i owns row i; row m with them).  rot: 3 m doubles.
    // Returns 0, or PZ_ERR_NO_CONVERGENCE after PZ_QR_SWEEPS_PER_EIG * m sweeps.
    template <class Wave>
    PE_DEV int pz_schur(Wave const& w, int m, double* Hr, double* Hi, int ld, double* rot, double hnorm)
    {
        double* const rc = rot;
        double* const rsr = rot + m;
        double* const rsi = rot + 2 * m;
        int hi_ = m - 1, its = 0, total = 0;
        int const cap = PZ_QR_SWEEPS_PER_EIG * m;
        while(hi_ >= 0)
        {
            int lo = hi_;
            while(lo > 0)
            {
                double const sub = pz_abs1(Hr[lo * ld + lo - 1], Hi[lo * ld + lo - 1]);
                if(sub == 0.0) break;
                double s = pz_abs1(Hr[(lo - 1) * ld + lo - 1], Hi[(lo - 1) * ld + lo - 1]) + pz_abs1(Hr[lo * ld + lo], Hi[lo * ld + lo]);
                if(s == 0.0) s = hnorm;
                if(sub <= PZ_EPS * s) break;
                --lo;
            }
            w.sync();
            if(lo > 0 && w.lane() == 0) Hr[lo * ld + lo - 1] = Hi[lo * ld + lo - 1] = 0.0;
            w.sync();
            if(lo == hi_)
            {
                --hi_;
                its = 0;
                continue;
            }
            if(++total > cap) return PZ_ERR_NO_CONVERGENCE;
            ++its;
            // the shift: the eigenvalue of the trailing 2 x 2 block nearer to its last diagonal entry; every tenth sweep on one eigenvalue an
            // exceptional one
            double mur, mui;
            {
                double const ar = Hr[(hi_ - 1) * ld + hi_ - 1], ai = Hi[(hi_ - 1) * ld + hi_ - 1];
                double const br = Hr[(hi_ - 1) * ld + hi_], bi = Hi[(hi_ - 1) * ld + hi_];
                double const cr = Hr[hi_ * ld + hi_ - 1], ci = Hi[hi_ * ld + hi_ - 1];
                double const dr = Hr[hi_ * ld + hi_], di = Hi[hi_ * ld + hi_];
                mur = dr;
                mui = di;
                if(its % 10 == 0)
                    mur += 0.75 * pz_abs1(cr, ci);
                else
                {
                    double const er = 0.5 * (ar - dr), ei = 0.5 * (ai - di);
                    double const pr = br * cr - bi * ci, pi = br * ci + bi * cr;  // b c
                    double qr, qi;
                    pz_csqrt(er * er - ei * ei + pr, 2.0 * er * ei + pi, qr, qi);
                    // d - b c / (e +- q), the sign that makes the denominator larger
                    double nr = er + qr, ni = ei + qi;
                    if(pz_abs1(er - qr, ei - qi) > pz_abs1(nr, ni))
                    {
                        nr = er - qr;
                        ni = ei - qi;
                    }
                    if(nr != 0.0 || ni != 0.0)
                    {
                        double tr, ti;
                        net_cdiv(pr, pi, nr, ni, tr, ti);
                        mur = dr - tr;
                        mui = di - ti;
                    }
                }
            }
            w.sync();
            for(int j = lo + w.lane(); j <= hi_; j += w.lanes())
            {
                Hr[j * ld + j] -= mur;
                Hi[j * ld + j] -= mui;
            }
            w.sync();
            for(int k = lo; k < hi_; ++k)
            {
                // G = [c s; -conj(s) c] with G (x, y)^T = (r, 0)^T
                double const xr = Hr[k * ld + k], xi = Hi[k * ld + k], yr = Hr[(k + 1) * ld + k], yi = Hi[(k + 1) * ld + k];
                double c = 1.0, sr = 0.0, si = 0.0;
                if(yr != 0.0 || yi != 0.0)
                {
                    double const ax = hypot(xr, xi), ay = hypot(yr, yi), n = hypot(ax, ay);
                    if(ax == 0.0)
                    {
                        c = 0.0;
                        sr = yr / ay;
                        si = -yi / ay;
                    }
                    else
                    {
                        c = ax / n;
                        double const ur = xr / ax, ui = xi / ax;  // x / |x|
                        sr = (ur * yr + ui * yi) / n;             // (x / |x|) conj(y) / n
                        si = (ui * yr - ur * yi) / n;
                    }
                }
                w.sync();  // (every lane has read column k before its owner rewrites it)
                for(int j = w.lane(); j < m; j += w.lanes())
                {
                    if(j < k) continue;
                    double const ar = Hr[k * ld + j], ai = Hi[k * ld + j], br = Hr[(k + 1) * ld + j], bi = Hi[(k + 1) * ld + j];
                    Hr[k * ld + j] = c * ar + (sr * br - si * bi);
                    Hi[k * ld + j] = c * ai + (sr * bi + si * br);
                    Hr[(k + 1) * ld + j] = j == k ? 0.0 : c * br - (sr * ar + si * ai);
                    Hi[(k + 1) * ld + j] = j == k ? 0.0 : c * bi - (sr * ai - si * ar);
                }
                if(w.lane() == 0)
                {
                    rc[k] = c;
                    rsr[k] = sr;
                    rsi[k] = si;
                }
                w.sync();
            }
            // R G_lo^H G_{lo+1}^H ...: columns k, k + 1 of rows 0 .. k + 1, and of row m
            for(int i = w.lane(); i <= m; i += w.lanes())
            {
                if(i > hi_ && i != m) continue;
                for(int k = (i == m || i - 1 < lo) ? lo : i - 1; k < hi_; ++k)
                {
                    double const c = rc[k], sr = rsr[k], si = rsi[k];
                    double const ar = Hr[i * ld + k], ai = Hi[i * ld + k], br = Hr[i * ld + k + 1], bi = Hi[i * ld + k + 1];
                    Hr[i * ld + k] = c * ar + (sr * br + si * bi);  // c a + conj(s) b
                    Hi[i * ld + k] = c * ai + (sr * bi - si * br);
                    Hr[i * ld + k + 1] = c * br - (sr * ar - si * ai);  // c b - s a
                    Hi[i * ld + k + 1] = c * bi - (sr * ai + si * ar);
                }
            }
            w.sync();
            for(int j = lo + w.lane(); j <= hi_; j += w.lanes())
            {
                Hr[j * ld + j] += mur;
                Hi[j * ld + j] += mui;
            }
            w.sync();
        }
        return 0;
    }

    // Matrix `mat` of R: load, Schur form, eigenvectors of the triangular factor by back-substitution (eigenvector i into the free lower
    // part of row i), their last components through row m of the unitary factor; then the raw and / or the mapped outputs.
    template <class Wave>
    PE_DEV void pz_ritz(Wave const& w, PzRitzView const& R, int mat, double* lds)
    {
        double const nan = __builtin_nan("");
        int const m = R.steps ? R.steps[mat] : R.m;
        int const parked = R.parked ? R.parked[mat] : 0;
        long long const o = static_cast<long long>(mat) * R.m;
        // outputs first: NaN padding, counts
        for(int i = w.lane(); i < R.m; i += w.lanes())
        {
            if(R.theta_re) R.theta_re[o + i] = R.theta_im[o + i] = R.last_re[o + i] = R.last_im[o + i] = nan;
            if(R.s_re) R.s_re[o + i] = R.s_im[o + i] = R.s_err[o + i] = nan;
        }
        if(w.lane() == 0)
        {
            if(R.n_found) R.n_found[mat] = 0;
            if(R.n_conv) R.n_conv[mat] = 0;
            R.status[mat] = 0;
        }
        if(m < 1 || m > R.m || parked == PZ_PARKED_FAILED) return;
        int const ld = m + 1;
        double* const Hr = lds;
        double* const Hi = lds + (m + 1) * ld;
        double* const aux = lds + 2 * (m + 1) * ld;  // 5 m doubles
        double const* gr = R.h_re + static_cast<long long>(mat) * R.mat_stride;
        double const* gi = R.h_im + static_cast<long long>(mat) * R.mat_stride;
        // load: the upper Hessenberg part (what lies below the subdiagonal is not read), row m = e_m^T; the largest modulus, NaN-keeping
        double mx = 0.0;
        for(int e = w.lane(); e < (m + 1) * m; e += w.lanes())
        {
            int const r = e / m, c = e - r * m;
            double vr = 0.0, vi = 0.0;
            if(r == m) vr = c == m - 1 ? 1.0 : 0.0;
            else if(r <= c + 1)
            {
                vr = gr[static_cast<long long>(r) * R.ld + c];
                vi = gi[static_cast<long long>(r) * R.ld + c];
                mx = ac_nanmax(mx, ac_nanmax(fabs(vr), fabs(vi)));
            }
            Hr[r * ld + c] = vr;
            Hi[r * ld + c] = vi;
        }
        mx = w.nanmax(mx, aux);
        if(!(mx <= PZ_DBL_MAX))
        {
            if(w.lane() == 0) R.status[mat] = PZ_ERR_SINGULAR;
            return;
        }
        double const beta = (R.steps && parked == 0) ? hypot(gr[static_cast<long long>(m) * R.ld + m - 1], gi[static_cast<long long>(m) * R.ld + m - 1]) : 0.0;
        w.sync();
        if(int const rc = pz_schur(w, m, Hr, Hi, ld, aux, mx); rc != 0)
        {
            if(w.lane() == 0) R.status[mat] = rc;
            return;
        }
        // eigenvector i of the triangular factor: x_i = 1, x_j = -(sum_{l = j+1 .. i} T_jl x_l) / (T_jj - T_ii) for j = i-1 .. 0, a
        // denominator below smin replaced by it; x_j goes to H(i, j).  Its image's last component: (row m) . x / |x|.
        double* const lr = aux;
        double* const li = aux + m;
        for(int i = w.lane(); i < m; i += w.lanes())
        {
            double const tr = Hr[i * ld + i], ti = Hi[i * ld + i];
            double const smin = fmax(PZ_EPS * fmax(pz_abs1(tr, ti), mx), 1.0e-300);
            double ar = Hr[m * ld + i], ai = Hi[m * ld + i], n2 = 1.0;
            for(int j = i - 1; j >= 0; --j)
            {
                double sr = Hr[j * ld + i], si = Hi[j * ld + i];  // T_ji x_i
                for(int l = j + 1; l < i; ++l)
                {
                    double const xr = Hr[i * ld + l], xi = Hi[i * ld + l];
                    sr += Hr[j * ld + l] * xr - Hi[j * ld + l] * xi;
                    si += Hr[j * ld + l] * xi + Hi[j * ld + l] * xr;
                }
                double dr = Hr[j * ld + j] - tr, di = Hi[j * ld + j] - ti;
                if(pz_abs1(dr, di) < smin)
                {
                    dr = smin;
                    di = 0.0;
                }
                double xr, xi;
                net_cdiv(-sr, -si, dr, di, xr, xi);
                Hr[i * ld + j] = xr;
                Hi[i * ld + j] = xi;
                n2 += xr * xr + xi * xi;
                ar += Hr[m * ld + j] * xr - Hi[m * ld + j] * xi;
                ai += Hr[m * ld + j] * xi + Hi[m * ld + j] * xr;
            }
            double const inv = 1.0 / sqrt(n2);
            lr[i] = ar * inv;
            li[i] = ai * inv;
        }
        w.sync();
        if(R.theta_re)
            for(int i = w.lane(); i < m; i += w.lanes())
            {
                R.theta_re[o + i] = Hr[i * ld + i];
                R.theta_im[o + i] = Hi[i * ld + i];
                R.last_re[o + i] = lr[i];
                R.last_im[o + i] = li[i];
            }
        if(!R.s_re) return;
        // the theta' floor, the map, err_est; then the rank of every kept eigenvalue
        double* const dist = aux + 2 * m;
        double* const sim = aux + 3 * m;
        double* const serr = aux + 4 * m;
        double big = 0.0;
        for(int i = 0; i < m; ++i) big = fmax(big, hypot(Hr[i * ld + i], Hi[i * ld + i]));
        double const inf = __builtin_inf();
        for(int i = w.lane(); i < m; i += w.lanes())
        {
            double const mag = hypot(Hr[i * ld + i], Hi[i * ld + i]);
            bool const keep = mag > R.theta_floor * big;  // (drops everything when big == 0)
            double qr = 0.0, qi = 0.0;
            if(keep) net_cdiv(R.omega0, 0.0, Hr[i * ld + i], Hi[i * ld + i], qr, qi);
            dist[i] = keep ? hypot(qr, qi) : inf;
            sim[i] = R.omega0 - qi;
            // (lr / li are read here for the last time; the real part of s travels in lr)
            double const last = hypot(lr[i], li[i]);
            li[i] = keep ? beta * last / mag : 0.0;
            lr[i] = -qr;
        }
        w.sync();
        int found = 0;
        for(int i = 0; i < m; ++i) found += dist[i] < inf ? 1 : 0;
        for(int i = w.lane(); i < m; i += w.lanes())
        {
            int rank = 0;
            for(int j = 0; j < m; ++j)
                rank += (dist[j] < dist[i] || (dist[j] == dist[i] && (sim[j] > sim[i] || (sim[j] == sim[i] && j < i)))) ? 1 : 0;
            serr[rank] = li[i];
            if(dist[i] < inf)
            {
                R.s_re[o + rank] = lr[i];
                R.s_im[o + rank] = sim[i];
                R.s_err[o + rank] = li[i];
            }
        }
        w.sync();
        if(w.lane() == 0)
        {
            int run = 0;
            while(run < found && serr[run] <= R.tol) ++run;
            R.n_found[mat] = found;
            R.n_conv[mat] = run;
        }
    }

    // the wave of a one-thread team
    struct PzSerialWave
    {
        int lane() const { return 0; }
        int lanes() const { return 1; }
        void sync() const {}
        double nanmax(double v, double*) const { return v; }
    };
}  // namespace pe
