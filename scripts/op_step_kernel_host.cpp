// op_step_kernel_host.cpp -- the kernel text of the stepped operating point (phy-engine_amd/csrc/pe_op_step.hpp: op_step_nonfinite,
// op_step_advance, op_step_apply through op_step_control_serial) run on the host with a one-thread team over a hand-made view: 3 instances
// that are in different phases at the same time (one solved by the direct attempt, one in gmin stepping, one whose gmin phase fails at
// lambda = 0 and goes on in source stepping, with a non-finite solution among its rejections), a ragged source list (3 of 9 value slots,
// not contiguous), a log shorter than the levels solved.  The "solves" between the controller launches are scripted: they write a status
// and a solution.  A program of its own for the sanitizers:
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iphy-engine_amd/csrc scripts/op_step_kernel_host.cpp -o op_step_kernel_host
// Every buffer is a std::vector of exactly the size the engine allocates, so an index one past any of them is reported.  exit 0 = the
// controller did what the rule says at every launch and every slot holds its real value at the end.
#include <cmath>
#include <cstdio>
#include <vector>

#include "pe_op_step.hpp"

namespace
{
    int failures = 0;
    void check(bool ok, char const* what, int round)
    {
        if(!ok)
        {
            std::fprintf(stderr, "op_step_kernel_host: %s (round %d)\n", what, round);
            ++failures;
        }
    }
}  // namespace

int main()
{
    using namespace pe;
    constexpr int B = 3, rows = 5, nD = 2, nRl = 1, dv_len = 9, n_src = 3, cap = 4;
    DevView V{};
    V.batch = B;
    V.rows = rows;
    V.nD = nD;
    V.nRl = nRl;
    V.dv_len = dv_len;
    std::vector<double> x(B * rows), ud(B * nD), gq(B * nD), dv(B * dv_len);
    std::vector<int> rl(B * nRl), status(B);
    std::vector<long long> n_iters(B);
    V.x = x.data();
    V.d_udlast = ud.data();
    V.d_geq = gq.data();
    V.rl_engaged = rl.data();
    V.dv = dv.data();
    V.status = status.data();
    V.n_iters = n_iters.data();

    OpStepView S{};
    std::vector<int> slot{3, 5, 8}, state(B), phase(B), first(B), have(B), fin(B), levels(B), rej(B), log_n(B), sr(B * nRl);
    std::vector<double> base(B * n_src), lambda(B), delta(B), cand(B), sx(B * rows), su(B * nD), sg(B * nD);
    std::vector<long long> iters(B), it_prev(B);
    std::vector<int> lp(B * cap), lo(B * cap), li(B * cap);
    std::vector<double> ll(B * cap), lv(B * cap);
    OpStepRecord rec{};
    S.method = OP_STEP_GMIN | OP_STEP_SOURCE;
    S.n_src = n_src;
    S.max_levels = 200;
    S.log_capacity = cap;
    S.attempt_cap = 6;
    S.direct_cap = 64;
    S.dl_init = 0.125;
    S.grow = 2.0;
    S.shrink = 0.25;
    S.dl_min = 0x1p-20;
    S.g_min = 1e-12;
    S.g_start = 1e-2;
    S.g_ratio = 1e-12 / 1e-2;
    S.src_slot = slot.data();
    S.src_base = base.data();
    S.state = state.data();
    S.phase = phase.data();
    S.first = first.data();
    S.have_shadow = have.data();
    S.lambda = lambda.data();
    S.delta = delta.data();
    S.cand = cand.data();
    S.final_status = fin.data();
    S.levels = levels.data();
    S.rejected = rej.data();
    S.iters = iters.data();
    S.it_prev = it_prev.data();
    S.sx = sx.data();
    S.su = su.data();
    S.sg = sg.data();
    S.sr = sr.data();
    S.log_phase = lp.data();
    S.log_outcome = lo.data();
    S.log_iters = li.data();
    S.log_n = log_n.data();
    S.log_lambda = ll.data();
    S.log_value = lv.data();
    S.rec = &rec;
    for(int b = 0; b < B; ++b)
    {
        for(int i = 0; i < dv_len; ++i) dv[b * dv_len + i] = 100.0 * b + i;  // (slots outside the list must keep these)
        dv[b * dv_len + DV_GMIN] = S.g_min;
        for(int j = 0; j < n_src; ++j) base[b * n_src + j] = dv[b * dv_len + slot[j]] = (b + 1) * (j + 2.5);
    }
    auto const dv0 = dv;

    // a scripted solve: status, a solution that tells the round, the junction state and the relay moved, iterations spent when converged
    auto solve = [&](int b, int st, int round, bool nan = false)
    {
        if(status[b] != 0) return;  // (parked)
        status[b] = st;
        for(int r = 0; r < rows; ++r) x[b * rows + r] = 10.0 * round + r + 0.25 * b;
        if(nan) x[b * rows + rows - 1] = NAN;  // (the last row: a loop one short would miss it)
        for(int i = 0; i < nD; ++i)
        {
            ud[b * nD + i] = round + 0.5 * i;
            gq[b * nD + i] = 2.0 * round + i;
        }
        rl[b * nRl] = round & 1;
        if(st == 0) n_iters[b] += 3;
    };
    auto launch = [&](int role)
    {
        rec = OpStepRecord{};
        op_step_control_serial(V, S, role);
    };

    // ---- the direct attempt: instance 0 converges, 1 does not, 2 "converges" to a non-finite solution
    for(int b = 0; b < B; ++b) it_prev[b] = n_iters[b];
    solve(0, 0, 0);
    solve(1, -4, 0);
    solve(2, 0, 0, true);
    auto const x_direct = std::vector<double>(x.begin(), x.begin() + rows);
    launch(OP_STEP_ROLE_BEGIN);
    check(rec.n_direct == 1 && rec.n_done == 1 && rec.n_active == 2 && rec.n_failed == 0 && rec.iters == 3 + 64, "record of the begin role", 0);
    check(status[0] == DC_SWEEP_PARKED && status[1] == 0 && status[2] == 0, "statuses after the begin role", 0);
    check(phase[1] == OP_STEP_GMIN && phase[2] == OP_STEP_GMIN && x[rows] == 0.0 && x[2 * rows + rows - 1] == 0.0 && rl[1] == 0, "first phase opened from zeros", 0);
    check(dv[1 * dv_len + DV_GMIN] == S.g_start && dv[DV_GMIN] == S.g_min, "DV_GMIN at lambda = 0", 0);

    // ---- levels.  Instance 1: gmin stepping, accept / accept / reject / accept ... to lambda = 1.  Instance 2: its gmin phase fails at
    // lambda = 0, source stepping: accept, non-finite, accept ...
    int round = 0, rejected1 = 0, rejected2 = 0;
    double shadow1 = -1.0;
    while(rec.n_active > 0 && round < 100)
    {
        ++round;
        bool const rej1 = round == 3, rej2 = round == 1 || round == 3 || round == 4;
        double const cand1 = cand[1], cand2 = cand[2], lam1 = lambda[1];
        int const ph2 = phase[2];
        bool const live1 = status[1] == 0, live2 = status[2] == 0;
        solve(1, rej1 ? -4 : 0, round);
        solve(2, round == 3 ? 0 : (rej2 ? -3 : 0), round, round == 3);
        if(live1 && !rej1) shadow1 = x[rows];
        launch(OP_STEP_ROLE_CONTROL);
        if(live1)
        {
            rejected1 += rej1;
            if(rej1) check(lambda[1] == lam1 && x[rows] == shadow1 && cand[1] < cand1, "rejection: state back from the shadow, a smaller step", round);
            else
                check(lambda[1] == cand1, "acceptance: lambda moves to the candidate", round);
            if(state[1] == OP_STEP_STEPPING) check(dv[1 * dv_len + DV_GMIN] == op_step_gmin(S, cand[1]) && dv[1 * dv_len + slot[1]] == base[1 * n_src + 1], "gmin level: DV_GMIN scaled, sources real", round);
        }
        if(live2)
        {
            rejected2 += rej2;
            if(round == 1) check(phase[2] == OP_STEP_SOURCE && cand[2] == 0.0 && x[2 * rows] == 0.0 && dv[2 * dv_len + slot[0]] == 0.0 && dv[2 * dv_len + DV_GMIN] == S.g_min, "gmin phase failed at lambda = 0: source phase opened from zeros", round);
            else if(state[2] == OP_STEP_STEPPING)
                check(dv[2 * dv_len + slot[2]] == cand[2] * base[2 * n_src + 2] && dv[2 * dv_len + DV_GMIN] == S.g_min && ph2 == OP_STEP_SOURCE, "source level: slots scaled by one multiply", round);
            (void)cand2;
        }
        for(int b = 0; b < B; ++b)
        {
            check((status[b] == 0) == (state[b] == OP_STEP_STEPPING) && (status[b] == 0 || status[b] == DC_SWEEP_PARKED), "finished instances parked, stepping ones open", round);
            for(int i = 0; i < dv_len; ++i)
                if(i != DV_GMIN && i != slot[0] && i != slot[1] && i != slot[2]) check(dv[b * dv_len + i] == dv0[b * dv_len + i], "a slot outside the list changed", round);
            if(state[b] != OP_STEP_STEPPING)
                for(int i = 0; i < dv_len; ++i) check(dv[b * dv_len + i] == dv0[b * dv_len + i], "a finished instance holds a scaled value", round);
        }
    }
    check(rec.n_active == 0 && state[1] == OP_STEP_SOLVED && state[2] == OP_STEP_SOLVED, "both stepping instances solved", round);
    check(phase[0] == 0 && phase[1] == OP_STEP_GMIN && phase[2] == OP_STEP_SOURCE, "phase each instance was solved in", round);
    check(rej[1] == rejected1 && rej[2] == rejected2 && levels[1] == log_n[1] && log_n[1] > cap, "counts; the log counts past its capacity", round);
    check(lp[1 * cap] == OP_STEP_GMIN && ll[1 * cap] == 0.0 && lo[1 * cap + 2] == 0 && lp[2 * cap] == OP_STEP_GMIN && lp[2 * cap + 1] == OP_STEP_SOURCE, "log entries", round);

    launch(OP_STEP_ROLE_FINISH);
    for(int b = 0; b < B; ++b)
    {
        check(status[b] == 0, "final status of a solved instance", round);
        for(int i = 0; i < dv_len; ++i) check(dv[b * dv_len + i] == dv0[b * dv_len + i], "real values after the finish role", round);
    }
    for(int r = 0; r < rows; ++r) check(x[r] == x_direct[r], "the directly solved instance was never touched", round);

    // ---- a call that gives up: max_levels 2, the last accepted level comes back
    S.max_levels = 2;
    for(int b = 0; b < B; ++b) status[b] = 0;
    solve(0, -4, 50);
    solve(1, -4, 50);
    solve(2, -4, 50);
    launch(OP_STEP_ROLE_BEGIN);
    solve(0, 0, 51);
    solve(1, -3, 51);
    solve(2, 0, 51);
    double const kept = x[0];
    launch(OP_STEP_ROLE_CONTROL);
    solve(0, -4, 52);
    solve(2, 0, 52);
    launch(OP_STEP_ROLE_CONTROL);
    check(rec.n_active == 0 && state[0] == OP_STEP_FAILED && state[1] == OP_STEP_STEPPING + OP_STEP_FAILED && state[2] == OP_STEP_FAILED, "max_levels spent", 52);
    launch(OP_STEP_ROLE_FINISH);
    check(status[0] == -4 && x[0] == kept && rl[0] == 1, "failed: status of the last failed attempt, state of the last accepted level", 52);
    check(status[1] == -3 && x[rows] == 0.0 && ud[nD] == 0.0, "failed without an accepted level: zeros", 52);
    check(status[2] == -4 && x[2 * rows] == 10.0 * 52 + 0.5, "failed after two accepted levels: the second one stays", 52);
    for(int b = 0; b < B; ++b)
        for(int i = 0; i < dv_len; ++i) check(dv[b * dv_len + i] == dv0[b * dv_len + i], "real values after a failed call", 52);

    if(failures) std::fprintf(stderr, "op_step_kernel_host: %d failure(s)\n", failures);
    else
        std::printf("op_step_kernel_host: ok (%d rounds)\n", round);
    return failures ? 1 : 0;
}
