// Multi-port network analysis through the plug-in API (circult::analyze_net -> pe_hip_analyze_net: one factorisation per pass, the second
// port solved on the kept factors, Y and S by the device's dense conversion).  Known answer: VAC - R - C low pass, port 1 at the source
// node (held by the source: its row and column of Z are zero), port 2 at the capacitor: Z22 = R / (1 + j omega R C), Y does not exist,
// S11 = -1, S12 = S21 = 0, S22 = (Z22 - z0) / (Z22 + z0).  Tolerance: the project's AC tolerance on every phasor (1e-9 + 1e-6 |x_r|)
// propagated to first order with a factor 2, as tests/net_common.py does: E on Z, 2 (E |W| + |Z - z0| |W| E |W|) on S with W = 1 / (Z + z0).
// exit 0 = pass.
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdio>
#include <vector>

#include <phy_engine/circuits/circuit.h>
#include <phy_engine/model/models/linear/VAC.h>
#include <phy_engine/model/models/linear/capacitor.h>
#include <phy_engine/model/models/linear/resistance.h>
#include <phy_engine/netlist/impl.h>

namespace pm = ::phy_engine::model;
using cplx = std::complex<double>;

static int failures = 0;
static void expect(char const* what, cplx got, cplx want, double tol)
{
    if(!(std::abs(got - want) <= tol))
    {
        std::fprintf(stderr, "net_twoport: %s = %.15g%+.15gj, expected %.15g%+.15gj (tol %g)\n", what, got.real(), got.imag(), want.real(), want.imag(), tol);
        ++failures;
    }
}

int main()
{
    constexpr double R = 1000.0, C = 1e-6, z0 = 50.0;
    ::phy_engine::circult c{};
    c.set_analyze_type(::phy_engine::analyze_type::OP);
    auto& nl{c.get_netlist()};
    auto [vac, p0]{add_model(nl, pm::VAC{.m_Vp = 1.0, .m_omega = 1000.0})};
    auto [r1, p1]{add_model(nl, pm::resistance{.r = R})};
    auto [c1, p2]{add_model(nl, pm::capacitor{.m_kZimag = C})};
    auto& n_in{create_node(nl)};
    auto& n_out{create_node(nl)};
    auto& gnd{nl.ground_node};
    add_to_node(nl, *vac, 0, n_in);
    add_to_node(nl, *vac, 1, gnd);
    add_to_node(nl, *r1, 0, n_in);
    add_to_node(nl, *r1, 1, n_out);
    add_to_node(nl, *c1, 0, n_out);
    add_to_node(nl, *c1, 1, gnd);

    std::vector<double> const w{0.0, 1000.0, 1e5};
    if(!c.analyze_net(w, {{&n_in, nullptr}, {&n_out, &gnd}}))
    {
        std::fprintf(stderr, "net_twoport: analyze_net failed: %s\n", c.last_error.c_str());
        return 1;
    }
    auto const& st{c.last_net_stats};
    if(st.n_ports != 2 || st.n_points != 3 || st.n_factorisations != st.n_passes || st.n_solves < st.n_passes || st.n_retried_points != 0)
    {
        std::fprintf(stderr, "net_twoport: stats: ports %d points %d passes %d factorisations %d solves %d retried %d\n", st.n_ports, st.n_points, st.n_passes,
                     st.n_factorisations, st.n_solves, st.n_retried_points);
        ++failures;
    }
    for(std::size_t k = 0; k < w.size(); ++k)
    {
        cplx const z22 = R / cplx{1.0, w[k] * R * C};
        double const e22 = 1e-9 + 1e-6 * std::abs(z22), e0 = 1e-9;
        auto const* Z = c.get_net(PE_HIP_NET_Z, k);
        auto const* Y = c.get_net(PE_HIP_NET_Y, k);
        auto const* S = c.get_net(PE_HIP_NET_S, k);
        if(!Z || !Y || !S)
        {
            std::fprintf(stderr, "net_twoport: no result at point %zu\n", k);
            return 1;
        }
        expect("Z11", Z[0], 0.0, e0);
        expect("Z12", Z[1], 0.0, e0);
        expect("Z21", Z[2], 0.0, e22);  // (column 1's phasor at the output node is 0: its own tolerance is the absolute part; e22 covers it)
        expect("Z22", Z[3], z22, e22);
        if(c.net_y_status[k] != PE_HIP_ERR_SINGULAR || !std::isnan(Y[0].real()) || !std::isnan(Y[3].imag()))
        {
            std::fprintf(stderr, "net_twoport: Y of a singular Z must read NaN with PE_HIP_ERR_SINGULAR (status %d)\n", c.net_y_status[k]);
            ++failures;
        }
        if(c.net_s_status[k] != PE_HIP_OK || c.net_point_status[k] != PE_HIP_OK) ++failures;
        double const w11 = 1.0 / z0, w22 = 1.0 / std::abs(z22 + z0);
        expect("S11", S[0], -1.0, 2.0 * (e0 * w11 + z0 * w11 * e0 * w11));
        expect("S22", S[3], (z22 - z0) / (z22 + z0), 2.0 * (e22 * w22 + std::abs(z22 - z0) * w22 * e22 * w22));
        expect("S12", S[1], 0.0, 2.0 * (e0 * w22 + z0 * w11 * e0 * w22));
        expect("S21", S[2], 0.0, 2.0 * (e22 * w11 + std::abs(z22 - z0) * w22 * e22 * w11));
    }
    // the capacitor alone as a one-port with another reference: Y exists
    double const z75 = 75.0;
    if(!c.analyze_net(w, {{&n_out, nullptr}}, &z75))
    {
        std::fprintf(stderr, "net_twoport: analyze_net (one port) failed: %s\n", c.last_error.c_str());
        return 1;
    }
    for(std::size_t k = 0; k < w.size(); ++k)
    {
        cplx const z = R / cplx{1.0, w[k] * R * C};
        double const e = 1e-9 + 1e-6 * std::abs(z), wm = 1.0 / std::abs(z + z75);
        expect("one-port Z", c.get_net(PE_HIP_NET_Z, k)[0], z, e);
        expect("one-port Y", c.get_net(PE_HIP_NET_Y, k)[0], 1.0 / z, 2.0 * e / std::norm(z));
        expect("one-port S", c.get_net(PE_HIP_NET_S, k)[0], (z - z75) / (z + z75), 2.0 * (e * wm + std::abs(z - z75) * wm * e * wm));
    }
    if(failures) return 1;
    std::printf("net_twoport: ok\n");
    return 0;
}
