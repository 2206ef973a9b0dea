// Operating point with gmin / source stepping through the plug-in API (circult::analyze_op_stepping -> pe_hip_analyze_op_stepping).  The
// deck is the common-emitter stage of the goldens bjt_npn_ce_dc_fail / bjt_pnp_ce_op_fail: 5 V rail, 100 kOhm base resistor, 1 kOhm
// collector resistor, NPN with Is = 1e-16, BetaF = 100.  The model's exponential has no junction limiting, so the cold-start Newton
// iteration of analyze() overflows and fails, as it does in the reference; stepping reaches v(B) = 0.692889 V (the value the oracle's
// stepped solution gives, checked to 1e-6) with every method, and the base node obeys Ib = (5 - v(B)) / 100 kOhm = Is (exp(v(B) / Ut) - 1)
// to the Newton stop rule.  analyze() is unchanged by the feature: it never steps.  exit 0 = pass.
#include <cmath>
#include <cstdio>

#include <phy_engine/circuits/circuit.h>
#include <phy_engine/model/models/linear/VDC.h>
#include <phy_engine/model/models/linear/resistance.h>
#include <phy_engine/model/models/non-linear/BJT_NPN.h>
#include <phy_engine/netlist/impl.h>

namespace pm = ::phy_engine::model;

static int failures = 0;
static void expect(char const* what, double got, double want, double tol)
{
    if(!(std::abs(got - want) <= tol))
    {
        std::fprintf(stderr, "op_step_ce: %s = %.17g, expected %.17g (tol %g)\n", what, got, want, tol);
        ++failures;
    }
}

static int stage(int method)
{
    ::phy_engine::circult c{};
    c.set_analyze_type(::phy_engine::analyze_type::DC);
    auto& nl{c.get_netlist()};
    auto [vcc, p0]{add_model(nl, pm::VDC{.V = 5.0})};
    auto [rb, p1]{add_model(nl, pm::resistance{.r = 1e5})};
    auto [rc, p2]{add_model(nl, pm::resistance{.r = 1e3})};
    auto [q1, p3]{add_model(nl, pm::BJT_NPN{.Is = 1e-16, .N = 1.0, .BetaF = 100.0, .Temp = 27.0, .Area = 1.0})};
    auto& n_cc{create_node(nl)};
    auto& n_b{create_node(nl)};
    auto& n_c{create_node(nl)};
    auto& gnd{nl.ground_node};
    add_to_node(nl, *vcc, 0, n_cc);
    add_to_node(nl, *vcc, 1, gnd);
    add_to_node(nl, *rb, 0, n_cc);
    add_to_node(nl, *rb, 1, n_b);
    add_to_node(nl, *rc, 0, n_cc);
    add_to_node(nl, *rc, 1, n_c);
    add_to_node(nl, *q1, 0, n_b);
    add_to_node(nl, *q1, 1, n_c);
    add_to_node(nl, *q1, 2, gnd);

    if(c.analyze())
    {
        std::fprintf(stderr, "op_step_ce: analyze() converged on the cold common-emitter stage: it must fail like the reference\n");
        ++failures;
    }
    if(!c.analyze_op_stepping(::phy_engine::analyze_type::DC, method))
    {
        std::fprintf(stderr, "op_step_ce: analyze_op_stepping(method %d) failed: %s\n", method, c.last_error.c_str());
        return 1;
    }
    double const vb = n_b.node_information.an.voltage.real(), vc = n_c.node_information.an.voltage.real(), vcc_v = n_cc.node_information.an.voltage.real();
    double const Ut = 1.380650524e-23 * (27.0 + 273.15) / 1.6021765314e-19;
    double const ib = 1e-16 * (std::exp(vb / Ut) - 1.0);
    // (gmin stepping, which PE_HIP_STEP_AUTO tries first, ends on 0.6928886; source stepping arrives along another path and stops on
    //  0.6928907, as the oracle's source-stepped run does: both inside the Newton stop rule, compared under the project's non-linear
    //  tolerance 1e-6 + 1e-5 |v|)
    expect("v(B)", vb, 0.692889, method == PE_HIP_STEP_SOURCE ? 1e-6 + 1e-5 * 0.692889 : 1e-6);
    expect("v(CC)", vcc_v, 5.0, 1e-9);
    expect("base KCL", (5.0 - vb) / 1e5, ib, 1e-3 * ib + 1e-12);            // Newton stop rule: 1e-3 relative
    expect("collector KCL", (5.0 - vc) / 1e3, 100.0 * ib, 1e-3 * 100.0 * ib + 1e-9);
    auto const& st{c.last_op_step_stats};
    expect("instances solved directly", st.n_direct, 0.0, 0.0);
    expect("instances failed", st.n_failed, 0.0, 0.0);
    expect("instances solved in the expected phase", method == PE_HIP_STEP_SOURCE ? st.n_source : st.n_gmin, 1.0, 0.0);
    if(!(st.n_levels >= 2 && st.n_solves == st.n_levels + 1 && st.n_launches == st.n_levels + 2))
    {
        std::fprintf(stderr, "op_step_ce: levels %lld solves %d launches %d\n", st.n_levels, st.n_solves, st.n_launches);
        ++failures;
    }
    // analyze() itself never steps: from the zero state it fails as before ... (the engine keeps the stepped solution as its state, from
    // which the plain iteration converges: the second analyze() below is the check that a following analysis runs on the real sources)
    if(!c.analyze())
    {
        std::fprintf(stderr, "op_step_ce: analyze() from the stepped solution failed: %s\n", c.last_error.c_str());
        ++failures;
    }
    expect("v(B) after analyze() from the stepped solution", n_b.node_information.an.voltage.real(), 0.692889, 1e-6 + 1e-5 * 0.692889);
    return 0;
}

int main()
{
    for(int method: {PE_HIP_STEP_AUTO, PE_HIP_STEP_GMIN, PE_HIP_STEP_SOURCE})
        if(stage(method)) return 1;
    if(failures) std::fprintf(stderr, "op_step_ce: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
