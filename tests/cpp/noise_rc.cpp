// Noise analysis through the plug-in API (circult::analyze_noise -> pe_hip_analyze_noise, the adjoint sweep on the device).  Known answer:
// an R - C low pass behind an AC source, output at the capacitor: S_v(omega) = 4 k T R / (1 + (omega R C)^2) at every point, and the
// integrated noise is k T / C up to the quadrature error of the swept points, which is computed here from the closed form.
// R = 1 kOhm, C = 1 uF, 141 logarithmic points from 1 to 1e7 rad/s.  exit 0 = pass.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <vector>

#include <phy_engine/circuits/circuit.h>
#include <phy_engine/model/models/linear/VAC.h>
#include <phy_engine/model/models/linear/capacitor.h>
#include <phy_engine/model/models/linear/resistance.h>
#include <phy_engine/netlist/impl.h>

namespace pm = ::phy_engine::model;

static int failures = 0;
static void expect(char const* what, double got, double want, double tol)
{
    if(!(std::abs(got - want) <= tol))
    {
        std::fprintf(stderr, "noise_rc: %s = %.17g, expected %.17g (tol %g)\n", what, got, want, tol);
        ++failures;
    }
}

int main()
{
    constexpr double R = 1000.0, C = 1e-6, kB = 1.380650524e-23, T = 300.15;
    ::phy_engine::circult c{};
    c.set_analyze_type(::phy_engine::analyze_type::AC);
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

    std::vector<double> omegas;
    for(int i = 0; i <= 140; ++i) omegas.push_back(std::pow(10.0, 7.0 * i / 140.0));
    if(!c.analyze_noise(n_out, nullptr, omegas))
    {
        std::fprintf(stderr, "noise_rc: analyze_noise failed: %s\n", c.last_error.c_str());
        return 1;
    }
    auto closed = [&](double w) { return 4.0 * kB * T * R / (1.0 + (w * R * C) * (w * R * C)); };
    // the project's AC tolerance on the adjoint phasor y = R / (1 + j omega R C) (1e-9 + 1e-6 |y|, and 1e-9 on the row that reads 0),
    // propagated to S |y|^2
    auto tolerance = [&](double w)
    {
        double const y = R / std::sqrt(1.0 + (w * R * C) * (w * R * C)), e = 1e-9 + 1e-6 * y + 1e-9;
        return 4.0 * kB * T / R * ((y + e) * (y + e) - y * y);
    };
    auto const& res{c.get_noise_results()};
    expect("points", static_cast<double>(res.size()), 141.0, 0.0);
    double trap = 0.0, trap_bound = 0.0, prev_b = 0.0;
    constexpr double two_pi = 6.283185307179586476925286766559;
    for(std::size_t i = 0; i < res.size(); ++i)
    {
        double const w = res[i].omega, want = closed(w);
        expect("omega", w, omegas[i], 0.0);
        double const bound = tolerance(w);
        expect("density", res[i].psd, want, bound);
        if(i)
        {
            double const df = (w - res[i - 1].omega) / two_pi;
            trap += df * (want + closed(res[i - 1].omega)) / 2.0;
            trap_bound += df * (bound + prev_b) / 2.0;
        }
        prev_b = bound;
    }
    double const ktc = kB * T / C;
    // the integral the engine formed against the trapezoid of the closed form over the same points, and against kT/C with that
    // quadrature's own error
    expect("integrated noise vs the closed form's trapezoid", c.noise_integrated, trap, trap_bound);
    expect("integrated noise vs kT/C", c.noise_integrated, ktc, std::abs(trap - ktc) + trap_bound);
    expect("quadrature error of these points is the 1.5e-3 it was worked out to be", trap / ktc, 1.0015, 1e-4);
    auto const& st{c.last_noise_stats};
    expect("points in the statistics", st.n_points, 141.0, 0.0);
    expect("sources", st.n_sources, 1.0, 0.0);
    expect("retried points", st.n_retried_points, 0.0, 0.0);
    expect("analyses = bands (seven decades)", st.n_analyses, 7.0, 1.0);
    if(!(st.n_passes < 141))
    {
        std::fprintf(stderr, "noise_rc: %d passes for 141 points: not batched\n", st.n_passes);
        ++failures;
    }

    // a differential output across the resistor: the source is an AC short, so v_in - v_out = -v_out and the density is the same
    if(!c.analyze_noise(n_in, &n_out, {1e3, 1e5})) return 1;
    for(auto const& pt: c.get_noise_results())
    {
        double const want = closed(pt.omega);
        expect("density across the resistor", pt.psd, want, tolerance(pt.omega));
    }
    if(failures) std::fprintf(stderr, "noise_rc: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
