// fourier_kernel_host.cpp -- the kernel text of the Fourier analysis of probes (phy-engine_amd/csrc/pe_fourier.hpp: fourier_arm,
// fourier_record through probe_record, fourier_finish) run on the host with a one-thread team over a hand-made view: 2 instances, 2 probes,
// 3 configured probes of which one is a duplicate, H = 63 and H = 1, the window [1, 2] of f0 = 1.  Instance 0 takes segments before the
// window, across its start, inside it, across its end and after it; instance 1 is armed at 0.5 and takes one step to 2.5, across both
// edges at once, then one more.  capacity = 1 and stride = 3: the sample buffer keeps nothing of it.  A program of its own for the sanitizers:
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iphy-engine_amd/csrc scripts/fourier_kernel_host.cpp -o fourier_kernel_host
// Every buffer is a std::vector of exactly the size the engine allocates, so an index one past any of them is reported.  exit 0 = every
// coefficient equals the integral of the clipped interpolant, taken in long double from the antiderivative at the segment ends, to 1e-13.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pe_probe.hpp"

namespace
{
    int failures = 0;
    struct Team
    {
        int tid() const { return 0; }
        int size() const { return 1; }
        void sync() const {}
    };
    double value(int row, double t) { return row == 0 ? 1.0 + std::sin(5.0 * t) + 0.3 * t : t * t - 1.5; }
    // int_{ta}^{tb} (line through (ta, va), (tb, vb)) e^{-j w (t - ts)} dt, real and minus imaginary part
    void segment(long double ta, long double va, long double tb, long double vb, long double w, long double ts, long double& c, long double& s)
    {
        if(w == 0.0L)
        {
            c += (tb - ta) * (va + vb) / 2;
            return;
        }
        long double const beta = (vb - va) / (tb - ta);
        auto G = [&](long double t, long double v, long double& re, long double& im)
        {  // e^{-j w tau} (j v / w + beta / w^2)
            long double const cs = std::cos(w * (t - ts)), sn = std::sin(w * (t - ts)), p = beta / (w * w), q = v / w;
            re = cs * p + sn * q;
            im = cs * q - sn * p;
        };
        long double r1, i1, r0, i0;
        G(tb, vb, r1, i1);
        G(ta, va, r0, i0);
        c += r1 - r0;
        s -= i1 - i0;
    }
}  // namespace

static void scenario(int H)
{
    using namespace pe;
    constexpr int B = 2, rows = 3, np = 2, n_fp = 3, cap = 1;
    int const K = H + 1;
    ProbedView V{};
    V.batch = B;
    V.rows = rows;
    V.probe_armed = 1;
    std::vector<double> x(B * rows), t_now(B);
    V.x = x.data();
    V.t_now = t_now.data();
    std::vector<int> prow{2, 0}, n_rec(B), fprobe{0, 1, 0};
    std::vector<long long> n_drop(B), n_acc(B);
    std::vector<double> st(B * cap), sv(B * cap * np), last(B * (np + 2)), ms(0);
    V.pr.n_probes = np;
    V.pr.n_meas = 0;
    V.pr.capacity = cap;
    V.pr.stride = 3;
    V.pr.rows = prow.data();
    V.pr.t = st.data();
    V.pr.v = sv.data();
    V.pr.n_rec = n_rec.data();
    V.pr.n_drop = n_drop.data();
    V.pr.n_acc = n_acc.data();
    V.pr.last = last.data();
    V.pr.ms = ms.data();
    std::vector<double> acc(static_cast<size_t>(B) * n_fp * K * 4, 7.0), cov(B, 7.0), coef(acc.size()), thd(B * n_fp);  // (7: arming must zero)
    double const f0 = 1.0, t_start = 1.0, t_end = t_start + 1.0 / f0;
    FourierView F{};
    F.n_fp = n_fp;
    F.H = H;
    F.probes = fprobe.data();
    F.w0 = 6.283185307179586476925286766559 * f0;
    F.t_start = t_start;
    F.t_end = t_end;
    F.acc = acc.data();
    F.cov = cov.data();
    V.fo = &F;

    std::vector<std::vector<double>> times{{0.0, 0.5, 0.9, 1.25, 1.5, 1.75, 1.78125, 2.3, 2.6}, {0.5, 2.5, 3.0}};
    int const row_of[2] = {2, 0};
    for(int b = 0; b < B; ++b)
    {
        auto put = [&](double t)
        {
            for(int r = 0; r < rows; ++r) x[b * rows + r] = value(r, t) * (b + 1);
        };
        put(times[b][0]);
        t_now[b] = times[b][0];
        probe_arm(Team{}, V, b);
        fourier_arm(Team{}, V, b);
        for(size_t i = 1; i < times[b].size(); ++i)
        {
            put(times[b][i]);
            probe_record(Team{}, V, b, times[b][i]);
        }
    }
    for(int i = 0; i < B * n_fp; ++i) fourier_finish(F, i / n_fp, i % n_fp, coef.data() + static_cast<size_t>(i) * K * 4, thd.data() + i);
    for(int b = 0; b < B; ++b)
    {
        if(std::fabs(cov[b] - 1.0) > 1e-15)
        {
            std::fprintf(stderr, "fourier_kernel_host: H %d instance %d covered %.17g\n", H, b, cov[b]);
            ++failures;
        }
        if(n_rec[b] != 1 || n_acc[b] != static_cast<long long>(times[b].size()) - 1)
        {
            std::fprintf(stderr, "fourier_kernel_host: H %d instance %d n_rec %d n_acc %lld\n", H, b, n_rec[b], n_acc[b]);
            ++failures;
        }
        for(int ip = 0; ip < n_fp; ++ip)
        {
            int const row = row_of[fprobe[ip]];
            double const* got = coef.data() + (static_cast<size_t>(b) * n_fp + ip) * K * 4;
            long double sum2 = 0, amp1 = 0;
            for(int k = 0; k < K; ++k)
            {
                long double c = 0, s = 0;
                for(size_t i = 1; i < times[b].size(); ++i)
                {
                    long double const t0 = times[b][i - 1], t1 = times[b][i], v0 = value(row, times[b][i - 1]) * (b + 1), v1 = value(row, times[b][i]) * (b + 1);
                    long double const ta = std::fmax(t0, static_cast<long double>(t_start)), tb = std::fmin(t1, static_cast<long double>(t_end));
                    if(!(tb > ta)) continue;
                    segment(ta, v0 + (v1 - v0) * (ta - t0) / (t1 - t0), tb, v0 + (v1 - v0) * (tb - t0) / (t1 - t0), k * 6.283185307179586476925286766559L * f0, t_start, c, s);
                }
                long double const a = (k ? 2 : 1) * c, bq = k ? 2 * s : 0, amp = std::sqrt(a * a + bq * bq);
                if(k == 1) amp1 = amp;
                if(k >= 2) sum2 += amp * amp;
                if(std::fabs(got[4 * k] - static_cast<double>(a)) > 1e-13 * (b + 1) * 4 || std::fabs(got[4 * k + 1] - static_cast<double>(bq)) > 1e-13 * (b + 1) * 4 ||
                   std::fabs(got[4 * k + 2] - static_cast<double>(amp)) > 1e-13 * (b + 1) * 4)
                {
                    std::fprintf(stderr, "fourier_kernel_host: H %d instance %d probe %d k %d: a %.17g b %.17g, expected %.17Lg %.17Lg\n", H, b, ip, k, got[4 * k], got[4 * k + 1], a, bq);
                    ++failures;
                }
            }
            double const want = static_cast<double>(std::sqrt(sum2) / amp1);
            if(std::fabs(thd[b * n_fp + ip] - want) > 1e-12 * (1.0 + want))
            {
                std::fprintf(stderr, "fourier_kernel_host: H %d instance %d probe %d thd %.17g, expected %.17g\n", H, b, ip, thd[b * n_fp + ip], want);
                ++failures;
            }
        }
        // the duplicate's rows are the same bits
        for(int i = 0; i < K * 4; ++i)
            if(coef[(static_cast<size_t>(b) * n_fp) * K * 4 + i] != coef[(static_cast<size_t>(b) * n_fp + 2) * K * 4 + i]) ++failures;
    }
}

int main()
{
    scenario(63);
    scenario(1);
    if(failures) std::fprintf(stderr, "fourier_kernel_host: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
