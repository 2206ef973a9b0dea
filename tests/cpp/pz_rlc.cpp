// Pole-zero analysis through the plug-in API (circult::analyze_pz -> pe_hip_analyze_pz: shift-invert Arnoldi on one factorisation).
// Known answer: VDC - L - R - C in series, s = (-R +- sqrt(R^2 - 4 L / C)) / (2 L): two real poles at R = 100, a complex pair at R = 20;
// with ports (in: the node behind the inductor, out: the capacitor's node) the current divides between L (to the source, an AC short) and
// the R - C branch, so H = V(out) / I(in) = s L / (s^2 L C + s R C + 1): one finite zero, at s = 0.  Tolerance: both poles are simple with
// condition numbers below 10 at the shift j 1e4; 1e-9 relative to |s - s0| is five orders above the rounding of the iteration
// (tests/pz_common.py E) and far below any wrong answer.
// exit 0 = pass.
#include <cmath>
#include <complex>
#include <cstdio>

#include <phy_engine/circuits/circuit.h>
#include <phy_engine/model/models/linear/VDC.h>
#include <phy_engine/model/models/linear/capacitor.h>
#include <phy_engine/model/models/linear/inductor.h>
#include <phy_engine/model/models/linear/resistance.h>
#include <phy_engine/netlist/impl.h>

namespace pm = ::phy_engine::model;
using cplx = std::complex<double>;

static int failures = 0;
static void expect(char const* what, cplx got, cplx want, double tol)
{
    if(!(std::abs(got - want) <= tol))
    {
        std::fprintf(stderr, "pz_rlc: %s = %.15g%+.15gj, expected %.15g%+.15gj (tol %g)\n", what, got.real(), got.imag(), want.real(), want.imag(), tol);
        ++failures;
    }
}

static void run(double R)
{
    constexpr double L = 1e-3, C = 1e-6, w0 = 1e4;
    ::phy_engine::circult c{};
    c.set_analyze_type(::phy_engine::analyze_type::OP);
    auto& nl{c.get_netlist()};
    auto [src, p0]{add_model(nl, pm::VDC{.V = 1.0})};
    auto [l1, p1]{add_model(nl, pm::inductor{.m_kZimag = L})};
    auto [r1, p2]{add_model(nl, pm::resistance{.r = R})};
    auto [c1, p3]{add_model(nl, pm::capacitor{.m_kZimag = C})};
    auto& n1{create_node(nl)};
    auto& n2{create_node(nl)};
    auto& n3{create_node(nl)};
    auto& gnd{nl.ground_node};
    add_to_node(nl, *src, 0, n1);
    add_to_node(nl, *src, 1, gnd);
    add_to_node(nl, *l1, 0, n1);
    add_to_node(nl, *l1, 1, n2);
    add_to_node(nl, *r1, 0, n2);
    add_to_node(nl, *r1, 1, n3);
    add_to_node(nl, *c1, 0, n3);
    add_to_node(nl, *c1, 1, gnd);

    ::phy_engine::circult::net_port const in{&n2, nullptr}, out{&n3, nullptr};
    if(!c.analyze_pz(w0, 2, 32, &in, &out))
    {
        std::fprintf(stderr, "pz_rlc: analyze_pz failed: %s\n", c.last_error.c_str());
        ++failures;
        return;
    }
    auto const& st{c.last_pz_stats};
    if(st.n_factorisations != 1 || st.n_solves < st.n_steps || !c.pz_poles_complete || c.pz_poles.size() != 2 || c.pz_poles_converged != 2 || c.pz_zeros.size() != 1)
    {
        std::fprintf(stderr, "pz_rlc: R = %g: factorisations %d solves %d steps %d complete %d poles %zu converged %d zeros %zu\n", R, st.n_factorisations,
                     st.n_solves, st.n_steps, int(c.pz_poles_complete), c.pz_poles.size(), c.pz_poles_converged, c.pz_zeros.size());
        ++failures;
        return;
    }
    cplx const root = std::sqrt(cplx{R * R - 4.0 * L / C, 0.0});
    cplx a = (-R + root) / (2.0 * L), b = (-R - root) / (2.0 * L);
    cplx const s0{0.0, w0};
    if(std::abs(b - s0) < std::abs(a - s0)) std::swap(a, b);  // nearest to the shift first
    expect("pole 0", c.pz_poles[0], a, 1e-9 * std::abs(a - s0));
    expect("pole 1", c.pz_poles[1], b, 1e-9 * std::abs(b - s0));
    expect("zero", c.pz_zeros[0], cplx{0.0, 0.0}, 1e-9 * w0);
    // H(s0) = s0 L / (s0^2 L C + s0 R C + 1)
    cplx const h = s0 * L / (s0 * s0 * L * C + s0 * R * C + 1.0);
    expect("H(s0)", c.pz_gain, h, 1e-9 + 1e-6 * std::abs(h));
}

int main()
{
    run(100.0);
    run(20.0);
    if(failures) return 1;
    std::puts("pz_rlc: ok");
    return 0;
}
