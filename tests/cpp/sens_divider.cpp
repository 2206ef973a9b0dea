// DC sensitivity analysis through the plug-in API (circult::analyze_sens -> pe_hip_analyze_sens, the adjoint solve on the device).  Known
// answer: a resistive divider behind a DC source, V = 3 V over R1 = 10 Ohm (source node - output) and R2 = 20 Ohm (output - ground):
// v_out = V R2 / (R1 + R2), so d v_out / d R1 = -V R2 / (R1 + R2)^2, d v_out / d R2 = V R1 / (R1 + R2)^2, d v_out / d V = R2 / (R1 + R2).
// Tolerance: the project's AC tolerance on every adjoint entry (1e-9 + 1e-6 |y_r|) propagated through d f / d p, with the closed-form
// adjoint solution y(output node) = R1 || R2, y(source node) = 0, y(source branch) = R2 / (R1 + R2).  exit 0 = pass.
#include <cmath>
#include <cstddef>
#include <cstdio>

#include <phy_engine/circuits/circuit.h>
#include <phy_engine/model/models/linear/VDC.h>
#include <phy_engine/model/models/linear/resistance.h>
#include <phy_engine/netlist/impl.h>

namespace pm = ::phy_engine::model;

static int failures = 0;
static void expect(char const* what, double got, double want, double tol)
{
    if(!(std::abs(got - want) <= tol))
    {
        std::fprintf(stderr, "sens_divider: %s = %.17g, expected %.17g (tol %g)\n", what, got, want, tol);
        ++failures;
    }
}

int main()
{
    constexpr double V = 3.0, R1 = 10.0, R2 = 20.0;
    ::phy_engine::circult c{};
    c.set_analyze_type(::phy_engine::analyze_type::OP);
    auto& nl{c.get_netlist()};
    auto [r1, p0]{add_model(nl, pm::resistance{.r = R1})};
    auto [r2, p1]{add_model(nl, pm::resistance{.r = R2})};
    auto [vdc, p2]{add_model(nl, pm::VDC{.V = V})};
    auto& n_out{create_node(nl)};
    auto& n_src{create_node(nl)};
    auto& gnd{nl.ground_node};
    add_to_node(nl, *r1, 0, n_src);
    add_to_node(nl, *r1, 1, n_out);
    add_to_node(nl, *r2, 0, n_out);
    add_to_node(nl, *r2, 1, gnd);
    add_to_node(nl, *vdc, 0, n_src);
    add_to_node(nl, *vdc, 1, gnd);

    if(!c.analyze_sens(n_out, nullptr))
    {
        std::fprintf(stderr, "sens_divider: analyze_sens failed: %s\n", c.last_error.c_str());
        return 1;
    }
    double const sum = R1 + R2, y_out = R1 * R2 / sum, y_k = R2 / sum;
    double const e_out = 1e-9 + 1e-6 * y_out, e_src = 1e-9, e_k = 1e-9 + 1e-6 * y_k;
    double const i = V / sum;  // the divider's current
    // d f / d R1 = -+ i / R1 at the source node and at the output; d f / d R2 = - i / R2 at the output; d f / d V = -1 at the branch row
    double const want[3] = {-V * R2 / (sum * sum), V * R1 / (sum * sum), R2 / sum};
    double const tol[3] = {(e_out + e_src) * i / R1, e_out * i / R2, e_k};
    auto const& res{c.get_sens_results()};
    expect("parameters", static_cast<double>(res.size()), 3.0, 0.0);
    if(res.size() == 3)
    {
        char const* name[3] = {"d v_out / d R1", "d v_out / d R2", "d v_out / d V"};
        int const kind[3] = {PE_HIP_R, PE_HIP_R, PE_HIP_VDC}, index[3] = {0, 1, 0};
        for(std::size_t k = 0; k < 3; ++k)
        {
            expect("kind", res[k].kind, kind[k], 0.0);
            expect("index", res[k].index, index[k], 0.0);
            expect("column", res[k].column, 0.0, 0.0);
            expect(name[k], res[k].value, want[k], tol[k]);
        }
    }
    auto const& st{c.last_sens_stats};
    expect("outputs in the statistics", st.n_outputs, 1.0, 0.0);
    expect("parameters in the statistics", st.n_params, 3.0, 0.0);
    expect("retried outputs", st.n_retried_outputs, 0.0, 0.0);
    expect("analyses", st.n_analyses, 1.0, 0.0);

    // the voltage across R1, normalised: p d (v_src - v_out) / d p = (V R1 / sum) x {R2 / sum, -R2 / sum, 1}
    if(!c.analyze_sens(n_src, &n_out, true)) return 1;
    auto const& rn{c.get_sens_results()};
    if(rn.size() == 3)
    {
        double const v1 = V * R1 / sum;
        // (the output is v_src - v_out: the adjoint is the negative of the one above at the output node, 1 - y_k at the branch row)
        double const e_k2 = 1e-9 + 1e-6 * (1.0 - y_k);
        expect("R1 d v_R1 / d R1", rn[0].value, v1 * R2 / sum, R1 * (e_out + e_src) * i / R1);
        expect("R2 d v_R1 / d R2", rn[1].value, -v1 * R2 / sum, R2 * e_out * i / R2);
        expect("V d v_R1 / d V", rn[2].value, v1, V * e_k2);
    }
    else
        ++failures;
    if(failures) std::fprintf(stderr, "sens_divider: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
