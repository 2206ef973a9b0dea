// pe_op_step.hpp -- gmin and source stepping for operating points (pe_engine_newton.cpp pe_hip_analyze_op_stepping): the per-element code
// of the controller that runs between two DC solves, team-generic like pe_dc_sweep.hpp.  Every failing instance carries its own phase,
// lambda and Delta on the device; the solves in between are dc_solve's, untouched, with the finished instances parked
// (pe::DC_SWEEP_PARKED).  pe_kernels.hip runs this text with one 256-thread workgroup per instance (k_op_step_control); builds without
// HIP run it with a one-thread team (the serial launcher in pe_engine_newton.cpp, scripts/op_step_kernel_host.cpp).  Only tid() and
// size() of the team are used; the one decision per instance (op_step_advance) is taken by one thread and handed to the others by the caller.
#pragma once
#include "pe_dc_sweep.hpp"  // DC_SWEEP_PARKED, DC_SWEEP_NONFINITE
#include "pe_device.hpp"

#include <cmath>

#ifndef PE_DEV
    #if defined(__HIPCC__)
        #define PE_DEV __device__ __forceinline__
    #else
        #define PE_DEV inline
    #endif
#endif

namespace pe
{
    enum : int
    {
        OP_STEP_GMIN = 1,    // phases (PE_HIP_STEP_GMIN / _SOURCE; 0: solved by the direct attempt)
        OP_STEP_SOURCE = 2,
        OP_STEP_STEPPING = 0,  // states
        OP_STEP_SOLVED = 1,
        OP_STEP_FAILED = 2,
        OP_STEP_ROLE_BEGIN = 0,    // after the direct attempt: classify it, initialise the controller, zero the starting state
        OP_STEP_ROLE_CONTROL = 1,  // after the solve of a level
        OP_STEP_ROLE_FINISH = 2,   // slots back to their real values, final statuses, failed instances back to their shadow
        OP_STEP_ACT_SAVE = 1,      // what the team does after the decision: state -> shadow
        OP_STEP_ACT_RESTORE = 2,   // shadow -> state
        OP_STEP_ACT_ZERO = 4,      // state as pe_hip_reset leaves it
        OP_STEP_ACT_SLOTS = 8      // source slots and DV_GMIN of the next level (or the real values)
    };

    // what a controller launch leaves for the host: the only thing it reads per level
    struct OpStepRecord
    {
        int n_active;    // instances with a level to solve next
        int n_done;      // instances solved so far (direct attempt included)
        int n_failed;    // instances that have given up
        int n_accepted;  // levels accepted / rejected by this launch
        int n_rejected;
        int n_direct;    // instances the direct attempt solved (role BEGIN)
        long long iters;  // Newton iterations of the attempts classified by this launch (a non-converged attempt counts the cap)
    };

    // What the controller reads and writes besides the engine's view (kept out of DevView: its size is part of k_tr_steps' register
    // allocation).  All pointers are device memory; per-instance arrays are [batch].
    struct OpStepView
    {
        int method;               // OP_STEP_GMIN, OP_STEP_SOURCE, or both bits: gmin stepping first, then source stepping
        int n_src;                // independent static source slots per instance
        int max_levels;           // levels an instance may spend over all its phases
        int log_capacity;         // log entries kept per instance (0: none)
        int attempt_cap;          // iterations a non-converged attempt has spent (the cap of that solve; 1 for a linear circuit)
        int direct_cap;           // ... of the direct attempt
        double dl_init, grow, shrink, dl_min;
        double g_min;             // the engine's g_min: what DV_GMIN holds outside gmin stepping and at lambda = 1
        double g_start, g_ratio;  // gmin stepping: DV_GMIN = g_start * g_ratio^lambda below lambda = 1 (g_ratio = g_end / g_start)
        int const* src_slot;      // [n_src] index of each source slot in the device value vector
        double const* src_base;   // [batch][n_src] the real value of each slot
        // controller state
        int* state;               // OP_STEP_STEPPING / _SOLVED / _FAILED
        int* phase;               // phase in progress (the one it was solved in once solved; 0: direct)
        int* first;               // 1: the level being solved is lambda = 0 of its phase
        int* have_shadow;         // 1: the shadow holds an accepted level of the phase in progress
        double *lambda, *delta, *cand;  // last accepted lambda, Delta, the lambda of the level being solved
        int* final_status;        // status of the instance once the call returns (stepping: that of its last failed attempt)
        int *levels, *rejected;   // levels solved, levels rejected
        long long* iters;         // Newton iterations spent by this call
        long long* it_prev;       // n_iters of the engine at the last classification
        // the shadow: the arrays a DC solve reads (dc_sweep_seed)
        double *sx, *su, *sg;     // [batch][rows], [batch][nD], [batch][nD]
        int* sr;                  // [batch][nRl]
        // the log: [batch][log_capacity]
        int *log_phase, *log_outcome, *log_iters, *log_n;  // (log_n [batch]: entries written so far, may exceed the capacity)
        double *log_lambda, *log_value;
        OpStepRecord* rec;
    };

    // the decision of one instance, as its team needs it
    struct OpStepAct
    {
        int bits;     // OP_STEP_ACT_*
        int phase;    // phase of the level to write (0: the real values)
        double cand;  // its lambda
    };

    // this thread's share of the finiteness flag of instance b's solution (1: something is not finite): a flag, never a maximum
    template <class Team>
    PE_DEV int op_step_nonfinite(Team const& tm, DevView const& V, int b)
    {
        double const* x = V.x + static_cast<long long>(b) * V.rows;
        int bad = 0;
        for(int r = tm.tid(); r < V.rows; r += tm.size())
            if(!(fabs(x[r]) <= 1.7976931348623157e308)) bad = 1;
        return bad;
    }

    // what DV_GMIN holds at level lambda of gmin stepping
    PE_DEV double op_step_gmin(OpStepView const& S, double lambda) { return lambda < 1.0 ? S.g_start * pow(S.g_ratio, lambda) : S.g_min; }

    // first level of `phase`: lambda = 0 from the zero state
    PE_DEV OpStepAct op_step_open_phase(OpStepView const& S, int b, int phase)
    {
        S.phase[b] = phase;
        S.first[b] = 1;
        S.have_shadow[b] = 0;
        S.lambda[b] = 0.0;
        S.delta[b] = S.dl_init;
        S.cand[b] = 0.0;
        return OpStepAct{OP_STEP_ACT_ZERO | OP_STEP_ACT_SLOTS, phase, 0.0};
    }

    // The controller of instance b (one thread; `nonfinite` = the instance's combined flag).  Plain double arithmetic: +, *, min and
    // comparisons.  Adds to the caller's private record; returns what the team does next.
    PE_DEV OpStepAct op_step_advance(DevView const& V, OpStepView const& S, int b, int nonfinite, int role, OpStepRecord& R)
    {
        OpStepAct none{0, 0, 0.0};
        if(role == OP_STEP_ROLE_FINISH)
        {
            // (an instance still stepping here belongs to a call that returns early: it keeps the status of its last failed attempt)
            int const failed = S.state[b] != OP_STEP_SOLVED;
            V.status[b] = S.final_status[b];
            if(failed && S.phase[b] == 0) return OpStepAct{OP_STEP_ACT_SLOTS, 0, 1.0};  // (never opened a phase: the direct attempt's state stays)
            return OpStepAct{OP_STEP_ACT_SLOTS | (failed ? (S.have_shadow[b] ? OP_STEP_ACT_RESTORE : OP_STEP_ACT_ZERO) : 0), 0, 1.0};
        }
        if(role == OP_STEP_ROLE_CONTROL && S.state[b] != OP_STEP_STEPPING) return none;  // (parked: finished or failed earlier)
        int st = V.status[b];
        if(st == 0 && nonfinite) st = DC_SWEEP_NONFINITE;
        long long const now = V.n_iters[b];
        int const cap = role == OP_STEP_ROLE_BEGIN ? S.direct_cap : S.attempt_cap;
        long long const it = st == 0 ? now - S.it_prev[b] : (st == -4 ? cap : 0);  // (-4: PE_HIP_ERR_NO_CONVERGENCE)
        S.it_prev[b] = now;
        R.iters += it;
        if(role == OP_STEP_ROLE_BEGIN)
        {
            S.iters[b] = it;
            S.levels[b] = 0;
            S.rejected[b] = 0;
            S.log_n[b] = 0;
            S.final_status[b] = st;
            S.have_shadow[b] = 0;
            S.first[b] = 0;
            S.delta[b] = 0.0;
            S.cand[b] = 0.0;
            S.phase[b] = 0;
            if(st == 0)
            {
                S.state[b] = OP_STEP_SOLVED;
                S.lambda[b] = 1.0;
                V.status[b] = DC_SWEEP_PARKED;
                ++R.n_done;
                ++R.n_direct;
                return none;
            }
            S.lambda[b] = 0.0;
            if(S.max_levels < 1)
            {
                S.state[b] = OP_STEP_FAILED;
                V.status[b] = DC_SWEEP_PARKED;
                ++R.n_failed;
                return none;
            }
            S.state[b] = OP_STEP_STEPPING;
            V.status[b] = 0;
            ++R.n_active;
            return op_step_open_phase(S, b, (S.method & OP_STEP_GMIN) ? OP_STEP_GMIN : OP_STEP_SOURCE);
        }
        // ---- a level of the phase in progress has been solved
        S.iters[b] += it;
        int const phase = S.phase[b];
        double const t = S.cand[b];
        int const n_log = S.log_n[b];
        if(n_log < S.log_capacity)
        {
            long long const o = static_cast<long long>(b) * S.log_capacity + n_log;
            S.log_phase[o] = phase;
            S.log_lambda[o] = t;
            S.log_value[o] = phase == OP_STEP_GMIN ? op_step_gmin(S, t) : t;
            S.log_outcome[o] = st == 0 ? 1 : 0;
            S.log_iters[o] = static_cast<int>(it);
        }
        S.log_n[b] = n_log + 1;
        int const levels = ++S.levels[b];
        int bits = 0;
        bool phase_failed = false;
        if(st == 0)
        {
            ++R.n_accepted;
            bits |= OP_STEP_ACT_SAVE;
            S.have_shadow[b] = 1;
            S.lambda[b] = t;
            if(S.first[b]) S.first[b] = 0;
            else
                S.delta[b] *= S.grow;
            if(t >= 1.0)
            {
                S.state[b] = OP_STEP_SOLVED;
                S.final_status[b] = 0;
                V.status[b] = DC_SWEEP_PARKED;
                ++R.n_done;
                return OpStepAct{bits | OP_STEP_ACT_SLOTS, 0, 1.0};
            }
        }
        else
        {
            ++R.n_rejected;
            ++S.rejected[b];
            S.final_status[b] = st;
            if(S.first[b]) phase_failed = true;
            else
            {
                S.delta[b] *= S.shrink;
                if(S.delta[b] < S.dl_min) phase_failed = true;
            }
        }
        bool const spent = levels >= S.max_levels;
        if(spent || (phase_failed && !(phase == OP_STEP_GMIN && (S.method & OP_STEP_SOURCE))))
        {
            // gives up: FINISH puts the state of the last accepted level of this phase back (zeros if there is none)
            S.state[b] = OP_STEP_FAILED;
            V.status[b] = DC_SWEEP_PARKED;
            ++R.n_failed;
            return OpStepAct{bits | OP_STEP_ACT_SLOTS, 0, 1.0};
        }
        V.status[b] = 0;
        ++R.n_active;
        if(phase_failed) return op_step_open_phase(S, b, OP_STEP_SOURCE);
        if(st != 0) bits |= OP_STEP_ACT_RESTORE;
        double const next = fmin(1.0, S.lambda[b] + S.delta[b]);
        S.cand[b] = next;
        return OpStepAct{bits | OP_STEP_ACT_SLOTS, phase, next};
    }

    // the team's part: the copies between the state and the shadow, then the slots of the level to solve (phase 0: the real values)
    template <class Team>
    PE_DEV void op_step_apply(Team const& tm, DevView const& V, OpStepView const& S, int b, OpStepAct const& a)
    {
        long long const B = b;
        double* x = V.x + B * V.rows;
        double *ud = V.d_udlast + B * V.nD, *gq = V.d_geq + B * V.nD;
        int* rl = V.rl_engaged + B * V.nRl;
        double *sx = S.sx + B * V.rows, *su = S.su + B * V.nD, *sg = S.sg + B * V.nD;
        int* sr = S.sr + B * V.nRl;
        if(a.bits & OP_STEP_ACT_SAVE)
        {
            for(int r = tm.tid(); r < V.rows; r += tm.size()) sx[r] = x[r];
            for(int i = tm.tid(); i < V.nD; i += tm.size())
            {
                su[i] = ud[i];
                sg[i] = gq[i];
            }
            for(int i = tm.tid(); i < V.nRl; i += tm.size()) sr[i] = rl[i];
        }
        if(a.bits & OP_STEP_ACT_RESTORE)
        {
            for(int r = tm.tid(); r < V.rows; r += tm.size()) x[r] = sx[r];
            for(int i = tm.tid(); i < V.nD; i += tm.size())
            {
                ud[i] = su[i];
                gq[i] = sg[i];
            }
            for(int i = tm.tid(); i < V.nRl; i += tm.size()) rl[i] = sr[i];
        }
        if(a.bits & OP_STEP_ACT_ZERO)
        {
            for(int r = tm.tid(); r < V.rows; r += tm.size()) x[r] = 0.0;
            for(int i = tm.tid(); i < V.nD; i += tm.size())
            {
                ud[i] = 0.0;
                gq[i] = 0.0;
            }
            for(int i = tm.tid(); i < V.nRl; i += tm.size()) rl[i] = 0;
        }
        if(a.bits & OP_STEP_ACT_SLOTS)
        {
            double* dv = V.dv + B * V.dv_len;
            double const* base = S.src_base + B * S.n_src;
            bool const scale = a.phase == OP_STEP_SOURCE;
            for(int j = tm.tid(); j < S.n_src; j += tm.size()) dv[S.src_slot[j]] = scale ? a.cand * base[j] : base[j];
            if(tm.tid() == 0) dv[DV_GMIN] = a.phase == OP_STEP_GMIN ? op_step_gmin(S, a.cand) : S.g_min;
        }
    }

#if !defined(__HIPCC__)
    // the whole controller launch by one thread (builds without HIP; the device runs the same text, one workgroup per instance)
    inline void op_step_control_serial(DevView const& V, OpStepView const& S, int role)
    {
        struct One
        {
            int tid() const { return 0; }
            int size() const { return 1; }
        };
        OpStepRecord R{};
        for(int b = 0; b < V.batch; ++b)
        {
            int const bad = role == OP_STEP_ROLE_FINISH ? 0 : op_step_nonfinite(One{}, V, b);
            OpStepAct const a = op_step_advance(V, S, b, bad, role, R);
            op_step_apply(One{}, V, S, b, a);
        }
        S.rec->n_active += R.n_active;
        S.rec->n_done += R.n_done;
        S.rec->n_failed += R.n_failed;
        S.rec->n_accepted += R.n_accepted;
        S.rec->n_rejected += R.n_rejected;
        S.rec->n_direct += R.n_direct;
        S.rec->iters += R.iters;
    }
#endif
}  // namespace pe
