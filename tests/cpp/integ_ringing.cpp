// Integration rule of the transient through the plug-in API (circult::set_tr_method -> pe_hip_set_tr_method): the L-stability case of
// tests/integ_common.py.  Series R = 1 Ohm, L = 1 nH (L / R = 1 ns) behind a square source that falls from 1 V to 0 at t = 250 ns, stepped
// at h = 100 ns from its operating point: the edge lies between steps 2 and 3.  The inductor voltage at the ten steps after the edge:
//   TRAP   alternates in sign on all ten and |v| at step 10 exceeds half of |v| at step 1 (the amplification factor tends to -1);
//   BE     |v| strictly decreasing;
//   BE and GEAR2   |v| at step 6 below 1e-4 of |v| at step 1.
// Also: an unknown method is refused and leaves the setting alone.  exit 0 = pass.
#include <cmath>
#include <cstdio>

#include <phy_engine/circuits/circuit.h>
#include <phy_engine/model/models/generator/square.h>
#include <phy_engine/model/models/linear/inductor.h>
#include <phy_engine/model/models/linear/resistance.h>
#include <phy_engine/netlist/impl.h>

namespace pm = ::phy_engine::model;

static int failures = 0;
static void check(bool ok, char const* what)
{
    if(!ok)
    {
        std::fprintf(stderr, "integ_ringing: %s\n", what);
        ++failures;
    }
}

constexpr double h = 1e-7;

// inductor voltage at steps 3 .. 12
static bool run(int method, double v[10])
{
    ::phy_engine::circult c{};
    auto& nl{c.get_netlist()};
    auto [g, p0]{add_model(nl, pm::square_gen{.Vh = 1.0, .Vl = 0.0, .freq = 1e5, .duty = 0.025, .phase = 0.0})};
    auto [r, p1]{add_model(nl, pm::resistance{.r = 1.0})};
    auto [l, p2]{add_model(nl, pm::inductor{.m_kZimag = 1e-9})};
    auto& a{create_node(nl)};
    auto& b{create_node(nl)};
    auto& gnd{nl.ground_node};
    add_to_node(nl, *g, 0, a);
    add_to_node(nl, *g, 1, gnd);
    add_to_node(nl, *r, 0, a);
    add_to_node(nl, *r, 1, b);
    add_to_node(nl, *l, 0, b);
    add_to_node(nl, *l, 1, gnd);
    if(c.set_tr_method(7) || c.tr_method_ != PE_HIP_TR_TRAP)
    {
        std::fprintf(stderr, "integ_ringing: an unknown method was accepted\n");
        return false;
    }
    if(!c.set_tr_method(method))
    {
        std::fprintf(stderr, "integ_ringing: set_tr_method(%d) failed: %s\n", method, c.last_error.c_str());
        return false;
    }
    c.get_analyze_setting().tr.t_step = h;
    c.get_analyze_setting().tr.t_stop = 0.5 * h;  // one step per analyze()
    for(int s = 1; s <= 12; ++s)
    {
        c.set_analyze_type(s == 1 ? ::phy_engine::analyze_type::TROP : ::phy_engine::analyze_type::TR);  // (the operating point, then step 1)
        if(!c.analyze())
        {
            std::fprintf(stderr, "integ_ringing: step %d under method %d failed: %s\n", s, method, c.last_error.c_str());
            return false;
        }
        if(s >= 3) v[s - 3] = b.node_information.an.voltage.real();
    }
    return true;
}

int main()
{
    double trap[10], be[10], gear[10];
    if(!run(PE_HIP_TR_TRAP, trap) || !run(PE_HIP_TR_BE, be) || !run(PE_HIP_TR_GEAR2, gear)) return 1;
    for(int k = 1; k < 10; ++k) check(trap[k] * trap[k - 1] < 0.0, "TRAP: the inductor voltage does not alternate in sign");
    check(std::abs(trap[9]) > 0.5 * std::abs(trap[0]), "TRAP: |v| at step 10 is not above half of |v| at step 1");
    for(int k = 1; k < 10; ++k) check(std::abs(be[k]) < std::abs(be[k - 1]), "BE: |v| is not strictly decreasing");
    check(std::abs(be[5]) < 1e-4 * std::abs(be[0]), "BE: |v| at step 6 is not below 1e-4 of |v| at step 1");
    check(std::abs(gear[5]) < 1e-4 * std::abs(gear[0]), "GEAR2: |v| at step 6 is not below 1e-4 of |v| at step 1");
    check(std::abs(trap[0]) > 1e-3 && std::abs(be[0]) > 1e-3 && std::abs(gear[0]) > 1e-3, "no edge seen at step 1");
    if(failures)
    {
        for(int k = 0; k < 10; ++k) std::fprintf(stderr, "  step %2d  TRAP %.6g  BE %.6g  GEAR2 %.6g\n", k + 1, trap[k], be[k], gear[k]);
        std::fprintf(stderr, "integ_ringing: %d failure(s)\n", failures);
    }
    return failures ? 1 : 0;
}
