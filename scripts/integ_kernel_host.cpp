// integ_kernel_host.cpp -- the kernel text of the backward-Euler / Gear-2 rules (phy-engine_amd/csrc/pe_integ.hpp: integ_coef,
// integ_companion_update, integ_commit, integ_restart, integ_lte_partial) run on the host with a one-thread team over a hand-made view:
// 2 instances of a circuit with 2 capacitors, 1 inductor, 1 coupled pair and 2 junctions (one without transit time), so that every block
// of the packed history array has a non-empty block before it.  Steps of 2, 1, 1, 3.5 (ratios 0.5, 1 and the fallback at 3.5) under GEAR2
// and BE, a restart of the failed instance only, dt = 0.  A program of its own for the sanitizers:
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iphy-engine_amd/csrc scripts/integ_kernel_host.cpp -o integ_kernel_host
// Every buffer is a std::vector of exactly the size the engine allocates, so an index one past any of them is reported.  exit 0 = every
// companion value equals the formula of include/pe_hip.h evaluated in long double from a history the program keeps itself, to 1e-13
// relative, the history array holds what the header says, and the two error estimates equal their divided differences.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pe_integ.hpp"

namespace
{
    int failures = 0;
    struct Team
    {
        int tid() const { return 0; }
        int size() const { return 1; }
        void sync() const {}
    };
    void expect(char const* what, int b, int i, double got, long double want)
    {
        long double const tol = 1e-13L * std::fabs(want) + 1e-300L;
        if(!(std::fabs(static_cast<long double>(got) - want) <= tol))
        {
            std::fprintf(stderr, "integ_kernel_host: %s [%d][%d] = %.17g, expected %.17Lg\n", what, b, i, got, want);
            ++failures;
        }
    }
    constexpr int B = 2, nC = 2, nL = 1, nCl = 1, nD = 2, n_nodes = 6, rows = n_nodes + nL + 2 * nCl, dv_len = 2 + 2 * nL + 5 * nCl;
    double xval(int b, int r, int step) { return std::sin(0.7 * r + 1.3 * step + 0.4 * b) + 0.1 * r; }
}  // namespace

static void scenario(int method)
{
    using namespace pe;
    DevView V{};
    V.batch = B;
    V.rows = rows;
    V.n_nodes = n_nodes;
    V.nC = nC;
    V.nL = nL;
    V.nCl = nCl;
    V.nD = nD;
    V.dv_len = dv_len;
    V.dv_lr = 2;
    V.dv_lu = 3;
    V.tr_method = method;
    std::vector<int> c_a{0, 2}, c_b{1, -1}, l_a{2}, l_b{3}, l_k{n_nodes}, cl_n{3, -1, 4, 5}, cl_k{n_nodes + 1, n_nodes + 2}, cl_dv{4}, d_a{4, 5}, d_c{-1, 0}, status(B);
    std::vector<double> x(B * rows), dv(B * dv_len), cap{1e-9, 2e-9, 3e-9, 4e-9}, ind{1e-3, 2e-3}, clp{1e-3, 4e-3, 0.5, 2e-3, 1e-3, 0.9};
    std::vector<double> dpar(B * nD * DP_NCOL, 0.0), c_hist(B * nC), c_prevg(B * nC), d_udlast(B * nD), d_geq(B * nD), d_hist(B * nD), d_prevg(B * nD);
    std::vector<double> hist(B * integ_stride(V), 0.0);
    V.c_a = c_a.data(); V.c_b = c_b.data(); V.l_a = l_a.data(); V.l_b = l_b.data(); V.l_k = l_k.data();
    V.cl_n = cl_n.data(); V.cl_k = cl_k.data(); V.cl_dv = cl_dv.data(); V.d_a = d_a.data(); V.d_c = d_c.data();
    V.x = x.data(); V.dv = dv.data(); V.c_cap = cap.data(); V.l_ind = ind.data(); V.cl_par = clp.data(); V.d_par = dpar.data();
    V.c_hist = c_hist.data(); V.c_prevg = c_prevg.data(); V.d_udlast = d_udlast.data(); V.d_geq = d_geq.data(); V.d_hist = d_hist.data(); V.d_prevg = d_prevg.data();
    V.status = status.data();
    V.tr_hist = hist.data();
    for(int b = 0; b < B; ++b)
    {
        dpar[(b * nD + 0) * DP_NCOL + DP_TT] = 1e-7;  // junction 1 has no transit time: both of its values stay 0
        d_geq[b * nD + 0] = 0.02 + 0.01 * b;
        d_geq[b * nD + 1] = 0.03;
    }
    int const stride = static_cast<int>(integ_stride(V));
    if(stride != nC + nL + 2 * nCl + nD + 1)
    {
        std::fprintf(stderr, "integ_kernel_host: stride %d\n", stride);
        ++failures;
    }
    auto volt = [&](int b, int step, int r) -> long double { return r >= 0 ? static_cast<long double>(xval(b, r, step)) : 0.0L; };
    // the quantities the history holds, in its order: v of the capacitors, i of the inductor, i1 and i2 of the pair, vd of the junctions
    auto quantity = [&](int b, int step, int q) -> long double
    {
        if(q < nC) return volt(b, step, c_a[q]) - volt(b, step, c_b[q]);
        if(q < nC + nL) return volt(b, step, l_k[q - nC]);
        if(q < nC + nL + 2 * nCl) return volt(b, step, cl_k[q - nC - nL]);
        int const i = q - nC - nL - 2 * nCl;
        return volt(b, step, d_a[i]) - volt(b, step, d_c[i]);
    };
    double const hs[4] = {2.0, 1.0, 1.0, 3.5};
    double hp = 0.0;
    Team tm;
    for(int step = 0; step < 4; ++step)
    {
        double const h = hs[step];
        for(int b = 0; b < B; ++b)
            for(int r = 0; r < rows; ++r) x[b * rows + r] = xval(b, r, step);
        bool const two = method == TR_GEAR2 && hp > 0.0 && !(h / hp > 1.0 + std::sqrt(2.0));
        long double const rho = two ? static_cast<long double>(h) / hp : 0.0L;
        long double const a0 = two ? (1 + 2 * rho) / (h * (1 + rho)) : 1.0L / h, a1 = two ? -(1 + rho) / h : -1.0L / h, a2 = two ? rho * rho / (h * (1 + rho)) : 0.0L;
        if(step == 3 && two)
        {
            std::fprintf(stderr, "integ_kernel_host: the scenario has no fallback step\n");
            ++failures;
        }
        for(int b = 0; b < B; ++b)
        {
            integ_companion_update(tm, V, b, h);
            if(hist[b * stride + stride - 1] != hp)
            {
                std::fprintf(stderr, "integ_kernel_host: the update moved h_p\n");
                ++failures;
            }
            integ_commit(tm, V, b, h);
            auto y = [&](int q) { return a1 * quantity(b, step, q) + (step > 0 ? a2 * quantity(b, step - 1, q) : 0.0L); };
            for(int i = 0; i < nC; ++i)
            {
                expect("c_prevg", b, i, c_prevg[b * nC + i], a0 * cap[b * nC + i]);
                expect("c_hist", b, i, c_hist[b * nC + i], cap[b * nC + i] * y(i));
            }
            expect("dv_lr", b, 0, dv[b * dv_len + V.dv_lr], -a0 * ind[b]);
            expect("dv_lu", b, 0, dv[b * dv_len + V.dv_lu], ind[b] * y(nC));
            {
                long double const L1 = clp[3 * b], L2 = clp[3 * b + 1], M = clp[3 * b + 2] * std::sqrt(L1 * L2);
                double const* o = &dv[b * dv_len + cl_dv[0]];
                expect("r11", b, 0, o[0], a0 * L1);
                expect("r12", b, 0, o[1], a0 * M);
                expect("r22", b, 0, o[2], a0 * L2);
                expect("u1", b, 0, o[3], L1 * y(nC + nL) + M * y(nC + nL + 1));
                expect("u2", b, 0, o[4], M * y(nC + nL) + L2 * y(nC + nL + 1));
            }
            for(int i = 0; i < nD; ++i)
            {
                long double const cd = static_cast<long double>(dpar[(b * nD + i) * DP_NCOL + DP_TT]) * d_geq[b * nD + i];
                expect("d_prevg", b, i, d_prevg[b * nD + i], i == 0 ? a0 * cd : 0.0L);
                expect("d_hist", b, i, d_hist[b * nD + i], i == 0 ? cd * y(nC + nL + 2 * nCl + i) : 0.0L);
                expect("d_udlast", b, i, d_udlast[b * nD + i], quantity(b, step, nC + nL + 2 * nCl + i));
            }
            for(int q = 0; q < stride - 1; ++q) expect("history", b, q, hist[b * stride + q], quantity(b, step, q));
            expect("h_p", b, 0, hist[b * stride + stride - 1], h);
        }
        hp = h;
    }
    // dt = 0: the companions of the inductors are taken out, nothing of the history moves
    std::vector<double> const before = hist;
    for(int b = 0; b < B; ++b)
    {
        integ_companion_update(tm, V, b, 0.0);
        integ_commit(tm, V, b, 0.0);
        expect("dv_lr at dt = 0", b, 0, dv[b * dv_len + V.dv_lr], 0.0L);
        expect("u1 at dt = 0", b, 0, dv[b * dv_len + cl_dv[0] + 3], 0.0L);
    }
    if(hist != before)
    {
        std::fprintf(stderr, "integ_kernel_host: dt = 0 moved the history\n");
        ++failures;
    }
    // restart of the failed instance only, then of every instance
    status[1] = -4;
    for(int b = 0; b < B; ++b) integ_restart(tm, V, b, true);
    expect("h_p of the instance that is OK", 0, 0, hist[stride - 1], hp);
    expect("h_p of the failed instance", 1, 0, hist[2 * stride - 1], 0.0L);
    for(int b = 0; b < B; ++b) integ_restart(tm, V, b, false);
    expect("h_p after the restart", 0, 0, hist[stride - 1], 0.0L);

    // ---- the error estimate
    std::vector<double> ring(3 * B * rows);
    std::vector<unsigned long long> q_each(B);
    LteView L{};
    L.hist = ring.data();
    L.s0 = 1;
    L.s1 = 2;
    L.s2 = 0;
    L.t0 = 0.0;
    L.t1 = 1.0;
    L.t2 = 2.5;
    L.tn = 4.0;
    L.h = 1.5;
    L.reltol = 1e-3;
    L.abstol_v = 1e-6;
    L.abstol_i = 1e-9;
    L.trtol = 7.0;
    L.test = 1;
    L.q_each = q_each.data();
    int const slot[3] = {1, 2, 0};
    for(int p = 0; p < 3; ++p)
        for(int b = 0; b < B; ++b)
            for(int r = 0; r < rows; ++r) ring[(slot[p] * B + b) * rows + r] = xval(b, r, 10 + p);
    for(int b = 0; b < B; ++b)
    {
        for(int r = 0; r < rows; ++r) x[b * rows + r] = xval(b, r, 13);
        int nonfinite = 0;
        double const got = lte_value(integ_lte_partial(tm, V, L, method, b, nonfinite));
        long double worst = 0.0L;
        for(int r = 0; r < rows; ++r)
        {
            long double const ya = xval(b, r, 10), yb = xval(b, r, 11), yc = xval(b, r, 12), yn = xval(b, r, 13);
            long double const d10 = (yb - ya) / 1.0L, d21 = (yc - yb) / 1.5L, dn2 = (yn - yc) / 1.5L;
            long double const e0 = (d21 - d10) / 2.5L, e1 = (dn2 - d21) / 3.0L, dd3 = (e1 - e0) / 4.0L;
            long double const rho = 1.5L / 1.5L;
            long double const err = method == TR_BE ? 1.5L * 1.5L * std::fabs(e1) : 1.5L * 1.5L * 1.5L * (1 + rho) * (1 + rho) / (rho * (1 + 2 * rho)) * std::fabs(dd3);
            long double const tol = 7.0L * (1e-3L * std::fmax(std::fabs(yn), std::fabs(yc)) + (r < n_nodes ? 1e-6L : 1e-9L));
            worst = std::fmax(worst, err / tol);
        }
        if(!(std::fabs(got - worst) <= 1e-12L * worst) || nonfinite)
        {
            std::fprintf(stderr, "integ_kernel_host: q [%d] = %.17g, expected %.17Lg (method %d)\n", b, got, worst, method);
            ++failures;
        }
    }
    // a NaN in the candidate is a NaN q and is flagged
    x[1 * rows + 2] = std::nan("");
    int nonfinite = 0;
    double const q = lte_value(integ_lte_partial(tm, V, L, method, 1, nonfinite));
    if(!std::isnan(q) || !nonfinite || lte_passes(q))
    {
        std::fprintf(stderr, "integ_kernel_host: a NaN candidate gave q = %g, nonfinite = %d\n", q, nonfinite);
        ++failures;
    }
}

int main()
{
    scenario(pe::TR_GEAR2);
    scenario(pe::TR_BE);
    if(failures) std::fprintf(stderr, "integ_kernel_host: %d failure(s)\n", failures);
    else
        std::printf("integ_kernel_host: ok\n");
    return failures ? 1 : 0;
}
