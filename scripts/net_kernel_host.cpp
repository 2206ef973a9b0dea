// net_kernel_host.cpp -- the kernel text of the network analysis (phy-engine_amd/csrc/pe_net.hpp: net_rhs, net_gather, net_convert) run on
// the host with a one-thread team / a one-lane wave over a hand-made view: 3 ports (one against ground, one differential, one against
// ground from the negative side), 2 circuit instances, 2 points per pass with the second slot unused, and the conversion on matrices of
// every size 1 .. 8 -- a plain one, one that needs a row exchange, a singular one, one with a NaN.  A program of its own for the sanitizers:
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iphy-engine_amd/csrc scripts/net_kernel_host.cpp -o net_kernel_host
// Every buffer is a std::vector of exactly the size the engine allocates, so an index one past any of them is reported.  exit 0 = the
// selectors and columns are right, an unused slot wrote nothing, Y Z = I and the S of a diagonal Z is the reflection coefficient.
#include <cmath>
#include <complex>
#include <cstdio>
#include <vector>

#include "pe_net.hpp"

namespace
{
    struct OneThread
    {
        int tid() const { return 0; }
        int size() const { return 1; }
    };
    int failures = 0;
    void expect(bool ok, char const* what)
    {
        if(ok) return;
        std::fprintf(stderr, "net_kernel_host: %s\n", what);
        ++failures;
    }
}  // namespace

int main()
{
    using namespace pe;
    using cplx = std::complex<double>;
    // ---- right-hand sides and columns
    {
        constexpr int N = 4, B = 2, P = 2, n = 3, n_points = 3, rhs0 = 5, dv_len = rhs0 + 2 * N, Q = B * P;
        DevView V{};
        V.rows = 2 * N;
        V.batch = Q;
        V.dv_len = dv_len;
        std::vector<double> dv(Q * dv_len, 7.0), xacc(Q * 2 * N), b0(Q * 2 * N, 7.0), z_re(n_points * B * n * n, -9.0), z_im(z_re.size(), -9.0), z0{50.0, 75.0, 600.0};
        std::vector<int> pos{2, 3, -1}, neg{-1, 0, 1}, point{2, -1};
        V.dv = dv.data();
        for(int q = 0; q < Q; ++q)
            for(int r = 0; r < 2 * N; ++r) xacc[q * 2 * N + r] = 100.0 * q + r;
        NetView Z{};
        Z.n_ports = n;
        Z.P = P;
        Z.n_inst = B;
        Z.n_half = N;
        Z.rhs0 = rhs0;
        Z.pos = pos.data();
        Z.neg = neg.data();
        Z.z0 = z0.data();
        Z.point = point.data();
        Z.xacc = xacc.data();
        Z.b0 = b0.data();
        Z.z_re = z_re.data();
        Z.z_im = z_im.data();
        for(int j = 0; j < n; ++j)
        {
            for(int q = 0; q < Q; ++q) net_rhs(OneThread{}, V, Z, q, j);
            for(int q = 0; q < Q; ++q)
                for(int r = 0; r < 2 * N; ++r)
                {
                    double const want = (r == pos[j] ? 1.0 : 0.0) - (r == neg[j] ? 1.0 : 0.0);
                    expect(dv[q * dv_len + rhs0 + r] == want && b0[q * 2 * N + r] == want, "selector");
                }
            for(int q = 0; q < Q; ++q) expect(dv[q * dv_len + rhs0 - 1] == 7.0, "the slot below the right-hand side is untouched");
            for(int q = 0; q < Q; ++q) net_gather(OneThread{}, V, Z, q, j);
        }
        for(int pt = 0; pt < n_points; ++pt)
            for(int b = 0; b < B; ++b)
                for(int i = 0; i < n; ++i)
                    for(int j = 0; j < n; ++j)
                    {
                        int const o = ((pt * B + b) * n + i) * n + j, q = b * P;
                        auto at = [&](int r, int half) { return r >= 0 ? xacc[q * 2 * N + half * N + r] : 0.0; };
                        if(pt != 2) expect(z_re[o] == -9.0 && z_im[o] == -9.0, "a point no slot of the pass holds is not written");
                        else
                            expect(z_re[o] == at(pos[i], 0) - at(neg[i], 0) && z_im[o] == at(pos[i], 1) - at(neg[i], 1), "column entry");
                    }
    }
    // ---- the conversion
    for(int n = 1; n <= NET_MAX_PORTS; ++n)
    {
        int const n_mats = 4, nn = n * n;
        std::vector<double> zr(n_mats * nn), zi(n_mats * nn), yr(n_mats * nn), yi(n_mats * nn), sr(n_mats * nn), si(n_mats * nn), z0(n);
        std::vector<int> ys(n_mats, 99), ss(n_mats, 99);
        for(int i = 0; i < n; ++i) z0[i] = 50.0 + 25.0 * i;
        for(int i = 0; i < n; ++i)
            for(int j = 0; j < n; ++j)
            {
                // 0: diagonally dominant; 1: a cyclic shift of it (zero diagonal for n > 1: row exchanges); 2: two equal rows (n > 1) / zero (n = 1); 3: a NaN
                double const a = (i == j ? 10.0 * n : 0.0) + std::sin(1.0 + i + 2.0 * j), c = std::cos(2.0 + 3.0 * i + j);
                zr[0 * nn + i * n + j] = a;
                zi[0 * nn + i * n + j] = c;
                zr[1 * nn + ((i + 1) % n) * n + j] = (n > 1 && i == j) ? 0.0 : a;   // (row i of matrix 0 without its diagonal, one row down)
                zi[1 * nn + ((i + 1) % n) * n + j] = (n > 1 && i == j) ? 0.0 : c;
                zr[2 * nn + i * n + j] = n > 1 ? (i == n - 1 ? zr[0 * nn + j] : a) : 0.0;
                zi[2 * nn + i * n + j] = n > 1 ? (i == n - 1 ? zi[0 * nn + j] : c) : 0.0;
                zr[3 * nn + i * n + j] = (i == n - 1 && j == 0) ? std::nan("") : a;
                zi[3 * nn + i * n + j] = c;
            }
        for(int m = 0; m < n_mats; ++m)
            net_convert(NetSerialWave{}, n, &zr[m * nn], &zi[m * nn], z0.data(), &yr[m * nn], &yi[m * nn], &sr[m * nn], &si[m * nn], &ys[m], &ss[m]);
        for(int m = 0; m < 2; ++m)
        {
            expect(ys[m] == 0 && ss[m] == 0, "a regular matrix has both inverses");
            double worst = 0.0, worst_s = 0.0;
            for(int i = 0; i < n; ++i)
                for(int j = 0; j < n; ++j)
                {
                    cplx acc = 0.0, acs = 0.0;
                    for(int k = 0; k < n; ++k)
                    {
                        cplx const y{yr[m * nn + i * n + k], yi[m * nn + i * n + k]}, z{zr[m * nn + k * n + j], zi[m * nn + k * n + j]};
                        cplx const s{sr[m * nn + i * n + k], si[m * nn + i * n + k]};
                        acc += y * z;
                        // S D^-1 (Z + Z0) D = D^-1 (Z - Z0) D
                        acs += s * (z + (k == j ? z0[k] : 0.0)) * std::sqrt(z0[j] / z0[k]);
                    }
                    cplx const z{zr[m * nn + i * n + j], zi[m * nn + i * n + j]};
                    worst = std::fmax(worst, std::abs(acc - (i == j ? 1.0 : 0.0)));
                    worst_s = std::fmax(worst_s, std::abs(acs - (z - (i == j ? z0[i] : 0.0)) * std::sqrt(z0[j] / z0[i])));
                }
            expect(worst <= 1e-12, "Y Z = I");
            expect(worst_s <= 1e-9, "S (Z + Z0) = Z - Z0 in power waves");
        }
        expect(ys[2] == NET_ERR_SINGULAR && std::isnan(yr[2 * nn]) && std::isnan(yi[3 * nn - 1]), "a singular Z has no Y");
        expect(ss[2] == 0 && std::isfinite(sr[2 * nn]), "... and still an S");
        expect(ys[3] == NET_ERR_SINGULAR && ss[3] == NET_ERR_SINGULAR && std::isnan(yr[3 * nn]) && std::isnan(sr[4 * nn - 1]), "a NaN entry: no inverse");
        // null outputs are skipped
        net_convert(NetSerialWave{}, n, &zr[0], &zi[0], z0.data(), nullptr, nullptr, &sr[0], nullptr, nullptr, &ss[0]);
    }
    // a one-port: S = (Z - z0) / (Z + z0)
    {
        double zr = 500.0, zi = -500.0, z0 = 50.0, yr, yi, sr, si;
        int ys, ss;
        net_convert(NetSerialWave{}, 1, &zr, &zi, &z0, &yr, &yi, &sr, &si, &ys, &ss);
        cplx const z{zr, zi};
        expect(std::abs(cplx{sr, si} - (z - z0) / (z + z0)) <= 1e-15 && std::abs(cplx{yr, yi} - 1.0 / z) <= 1e-18, "one-port");
    }
    if(failures) return 1;
    std::printf("net_kernel_host: ok\n");
    return 0;
}
