// Frequency sweeps through the plug-in API (analyze_type::AC with sweep_type::log / linear): run_ac_analysis hands the whole omega list
// to pe_hip_analyze_ac_sweep, which solves the points as batches of instances on the device.  Known answer: a series R - L into a
// shunt C driven by 1 V, H = v_out / v_in = 1 / (1 - omega^2 L C + j omega R C) at every point (R = 1 kOhm, L = 1 mH, C = 1 uF: corner
// 1 / sqrt(L C) = 31.6 krad/s inside the swept range).  exit 0 = pass.
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdio>

#include <phy_engine/circuits/circuit.h>
#include <phy_engine/model/models/linear/VAC.h>
#include <phy_engine/model/models/linear/capacitor.h>
#include <phy_engine/model/models/linear/inductor.h>
#include <phy_engine/model/models/linear/resistance.h>
#include <phy_engine/netlist/impl.h>

namespace pm = ::phy_engine::model;

static int failures = 0;
static void expect(char const* what, double got, double want, double tol)
{
    if(!(std::abs(got - want) <= tol))
    {
        std::fprintf(stderr, "ac_sweep: %s = %.17g, expected %.17g (tol %g)\n", what, got, want, tol);
        ++failures;
    }
}

int main()
{
    constexpr double R = 1000.0, L = 1e-3, C = 1e-6;
    ::phy_engine::circult c{};
    c.set_analyze_type(::phy_engine::analyze_type::AC);
    auto& nl{c.get_netlist()};
    auto [vac, p0]{add_model(nl, pm::VAC{.m_Vp = 1.0, .m_omega = 1000.0})};
    auto [r1, p1]{add_model(nl, pm::resistance{.r = R})};
    auto [l1, p2]{add_model(nl, pm::inductor{.m_kZimag = L})};
    auto [c1, p3]{add_model(nl, pm::capacitor{.m_kZimag = C})};
    auto& n_in{create_node(nl)};
    auto& n_mid{create_node(nl)};
    auto& n_out{create_node(nl)};
    auto& gnd{nl.ground_node};
    add_to_node(nl, *vac, 0, n_in);
    add_to_node(nl, *vac, 1, gnd);
    add_to_node(nl, *r1, 0, n_in);
    add_to_node(nl, *r1, 1, n_mid);
    add_to_node(nl, *l1, 0, n_mid);
    add_to_node(nl, *l1, 1, n_out);
    add_to_node(nl, *c1, 0, n_out);
    add_to_node(nl, *c1, 1, gnd);
    auto H = [&](double w) { return 1.0 / std::complex<double>(1.0 - w * w * L * C, w * R * C); };

    // logarithmic sweep: 60 points over six decades (no point sits on a band boundary: ten points per decade-wide band)
    auto& ac{c.get_analyze_setting().ac};
    ac.sweep = ::phy_engine::analyzer::AC::sweep_type::log;
    ac.omega_start = 10.0;
    ac.omega_stop = 1e7;
    ac.points = 60;
    if(!c.analyze())
    {
        std::fprintf(stderr, "ac_sweep: log sweep failed: %s\n", c.last_error.c_str());
        return 1;
    }
    {
        auto const& res{c.get_ac_sweep_results()};
        expect("log sweep points", static_cast<double>(res.size()), 60.0, 0.0);
        // the omega list is formed as the reference forms it: start, then repeated multiplication by the ratio
        double const ratio = std::pow(1e7 / 10.0, 1.0 / 59.0);
        double w = 10.0;
        for(auto const& pt: res)
        {
            expect("log sweep omega", pt.omega, w, 0.0);
            expect("log sweep |H - v_out|", std::abs(pt.x[n_out.node_index] - H(pt.omega)), 0.0, 1e-12);
            expect("log sweep |v_in - 1|", std::abs(pt.x[n_in.node_index] - 1.0), 0.0, 1e-12);
            w *= ratio;
        }
        // nodes, branches and ac.omega hold the LAST point
        if(!res.empty())
        {
            auto const& last{res.back()};
            expect("omega left in the setting", ac.omega, last.omega, 0.0);
            expect("node voltage left behind (re)", n_out.node_information.an.voltage.real(), last.x[n_out.node_index].real(), 0.0);
            expect("node voltage left behind (im)", n_out.node_information.an.voltage.imag(), last.x[n_out.node_index].imag(), 0.0);
        }
        auto const& st{c.last_ac_sweep_stats};
        expect("points in the statistics", st.n_points, 60.0, 0.0);
        expect("fallback points", st.n_fallback_points, 0.0, 0.0);
        expect("analyses = bands (six decades, ten points each)", st.n_analyses, 6.0, 0.0);
        if(!(st.n_passes >= st.n_analyses && st.n_passes < 60))
        {
            std::fprintf(stderr, "ac_sweep: %d passes for 60 points in %d bands: not batched\n", st.n_passes, st.n_analyses);
            ++failures;
        }
    }

    // linear sweep across the corner: 25 points
    ac.sweep = ::phy_engine::analyzer::AC::sweep_type::linear;
    ac.omega_start = 1e3;
    ac.omega_stop = 1e5;
    ac.points = 25;
    if(!c.analyze())
    {
        std::fprintf(stderr, "ac_sweep: linear sweep failed: %s\n", c.last_error.c_str());
        return 1;
    }
    {
        auto const& res{c.get_ac_sweep_results()};
        expect("linear sweep points", static_cast<double>(res.size()), 25.0, 0.0);
        double const step = (1e5 - 1e3) / 24.0;
        for(std::size_t i = 0; i < res.size(); ++i)
        {
            expect("linear sweep omega", res[i].omega, 1e3 + step * static_cast<double>(i), 0.0);
            expect("linear sweep |H - v_out|", std::abs(res[i].x[n_out.node_index] - H(res[i].omega)), 0.0, 1e-12);
        }
        if(!res.empty()) expect("last point in the node", std::abs(n_out.node_information.an.voltage - res.back().x[n_out.node_index]), 0.0, 0.0);
    }

    // a single point afterwards still takes the single-point path and agrees with the sweep's value there
    ac.sweep = ::phy_engine::analyzer::AC::sweep_type::single;
    ac.omega = 1e4;
    if(!c.analyze()) return 1;
    expect("single point |H - v_out|", std::abs(n_out.node_information.an.voltage - H(1e4)), 0.0, 1e-12);

    if(failures) std::fprintf(stderr, "ac_sweep: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
