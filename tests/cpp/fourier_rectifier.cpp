// Fourier analysis of a transient through the plug-in API (circult::set_fourier / get_fourier -> pe_hip_set_fourier / pe_hip_get_fourier).
//   rectifier  VAC 2 V / 1 kHz - diode - (1 kOhm || 1 uF), g_min = 1e-12, 130 steps of a 64th of a period, H = 9, window [0, 2 ms]:
//              the THD of the output node against the value argv[1] with the bound argv[2] -- what the mpmath reference of
//              tests/fourier_common.py (cpp_expectations) gives for the same run of the same library.  Without arguments the THD is only
//              required to be a distorted wave's (0.5 .. 1).
//   pulse_src  PULSE 0 / 1 V, 1 kHz, edges of an eighth of a period, into 1 kOhm; the corners fall on steps, so the interpolant is the
//              trapezoid wave itself and a_k - j b_k = (2 / T) (-1 / w^2) sum (slope after - slope before) e^{-j w t_i} over its four
//              corners; compared to 1e-12 of the amplitude (the cap tests/fourier_common.py puts on a run's distance from the ideal wave).
// exit 0 = pass.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>

#include <phy_engine/circuits/circuit.h>
#include <phy_engine/model/models/generator/pulse.h>
#include <phy_engine/model/models/linear/VAC.h>
#include <phy_engine/model/models/linear/capacitor.h>
#include <phy_engine/model/models/linear/resistance.h>
#include <phy_engine/model/models/non-linear/PN_junction.h>
#include <phy_engine/netlist/impl.h>

namespace pm = ::phy_engine::model;

static int failures = 0;
static void expect(char const* what, double got, double want, double tol)
{
    if(!(std::abs(got - want) <= tol))
    {
        std::fprintf(stderr, "fourier_rectifier: %s = %.17g, expected %.17g (tol %g)\n", what, got, want, tol);
        ++failures;
    }
}

constexpr double f0 = 1e3, T = 1.0 / f0, pi = 3.14159265358979323846;

static bool run(::phy_engine::circult& c, ::phy_engine::model::node_t& probe, int H)
{
    c.set_analyze_type(::phy_engine::analyze_type::TR);
    c.get_analyze_setting().tr.t_step = T / 64;
    c.get_analyze_setting().tr.t_stop = 129.5 * (T / 64);  // 130 steps: two past the window's end
    if(!c.set_fourier(probe, f0, 0.0, 2, H))
    {
        std::fprintf(stderr, "fourier_rectifier: set_fourier failed: %s\n", c.last_error.c_str());
        return false;
    }
    if(!c.get_fourier() || !std::isnan(c.fourier_thd) || c.fourier_covered != 0.0)
    {
        std::fprintf(stderr, "fourier_rectifier: before the transient thd = %g, covered = %g\n", c.fourier_thd, c.fourier_covered);
        ++failures;
    }
    if(!c.analyze() || !c.get_fourier())
    {
        std::fprintf(stderr, "fourier_rectifier: transient or get_fourier failed: %s\n", c.last_error.c_str());
        return false;
    }
    expect("covered", c.fourier_covered, 2 * T, 1e-15);
    return true;
}

int main(int argc, char** argv)
{
    {
        ::phy_engine::circult c{};
        c.env.g_min = 1e-12;
        auto& nl{c.get_netlist()};
        auto [vac, p0]{add_model(nl, pm::VAC{.m_Vp = 2.0, .m_omega = 2.0 * pi * f0, .m_phase = 0.0})};
        auto [d, p1]{add_model(nl, pm::PN_junction{})};
        auto [r, p2]{add_model(nl, pm::resistance{.r = 1e3})};
        auto [cap, p3]{add_model(nl, pm::capacitor{.m_kZimag = 1e-6})};
        auto& a{create_node(nl)};
        auto& k{create_node(nl)};
        auto& gnd{nl.ground_node};
        add_to_node(nl, *vac, 0, a);
        add_to_node(nl, *vac, 1, gnd);
        add_to_node(nl, *d, 0, a);
        add_to_node(nl, *d, 1, k);
        add_to_node(nl, *r, 0, k);
        add_to_node(nl, *r, 1, gnd);
        add_to_node(nl, *cap, 0, k);
        add_to_node(nl, *cap, 1, gnd);
        if(!run(c, k, 9)) return 1;
        if(argc >= 3) expect("thd of the rectifier", c.fourier_thd, std::atof(argv[1]), std::atof(argv[2]));
        else if(!(c.fourier_thd > 0.5 && c.fourier_thd < 1.0))
        {
            std::fprintf(stderr, "fourier_rectifier: thd = %.17g\n", c.fourier_thd);
            ++failures;
        }
        double s2 = 0.0;
        for(int h = 2; h <= 9; ++h) s2 = std::fma(c.fourier_results[h].amp, c.fourier_results[h].amp, s2);
        expect("thd from the harmonics", c.fourier_thd, std::sqrt(s2) / c.fourier_results[1].amp, 0.0);
    }
    {
        ::phy_engine::circult c{};
        auto& nl{c.get_netlist()};
        auto [g, p0]{add_model(nl, pm::pulse_gen{.Vh = 1.0, .Vl = 0.0, .freq = f0, .duty = 0.5, .phase = 0.0, .tr = T / 8, .tf = T / 8})};
        auto [r, p1]{add_model(nl, pm::resistance{.r = 1e3})};
        auto& n{create_node(nl)};
        auto& gnd{nl.ground_node};
        add_to_node(nl, *g, 0, n);
        add_to_node(nl, *g, 1, gnd);
        add_to_node(nl, *r, 0, n);
        add_to_node(nl, *r, 1, gnd);
        constexpr int H = 21;
        if(!run(c, n, H)) return 1;
        expect("a_0 of the trapezoid", c.fourier_results[0].a, 0.375, 1e-12);
        double const corner[4] = {0.0, T / 8, 3 * T / 8, T / 2}, jump[4] = {8 / T, -8 / T, -8 / T, 8 / T};
        for(int h = 1; h <= H; ++h)
        {
            double const w = 2.0 * pi * f0 * h;
            std::complex<double> z{};
            for(int i = 0; i < 4; ++i) z += jump[i] * std::exp(std::complex<double>(0.0, -w * corner[i]));
            z *= 2.0 / T * (-1.0 / (w * w));
            char what[32];
            std::snprintf(what, sizeof what, "a_%d of the trapezoid", h);
            expect(what, c.fourier_results[h].a, z.real(), 1e-12);
            std::snprintf(what, sizeof what, "b_%d of the trapezoid", h);
            expect(what, c.fourier_results[h].b, -z.imag(), 1e-12);
        }
    }
    if(failures) std::fprintf(stderr, "fourier_rectifier: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
