// pe_dc_sweep.hpp -- DC sweep with the points of a pass as extra instances (pe_engine_newton.cpp pe_hip_analyze_dc_sweep): the per-element
// code of the sweep's kernels, team-generic like pe_ac_sweep.hpp.  Sweep-engine instance q = b * P + p is circuit instance b at slot p of
// the pass; the slots of a pass hold a contiguous run of the SORTED values.  pe_kernels.hip runs this text with a grid team (k_dc_sweep_fill
// / _seed / _gather) and with one workgroup per circuit instance (k_dc_sweep_classify, whose scans live there); builds without HIP run it
// with a one-thread team (the serial launchers in pe_engine_newton.cpp).  Only tid() and size() of the team are used.
#pragma once
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
    // status of an instance neither schedule may touch: not OK (the resident kernel and the split schedule's mask skip it), not one of the
    // statuses the residual safety net retries, not the marker run_m2_dc parks its own subsets with
    constexpr int DC_SWEEP_PARKED = -2000;
    constexpr int DC_SWEEP_NONFINITE = -3;  // PE_HIP_ERR_SINGULAR: what the solvers report for a non-finite solution

    // what a classification leaves for the host: the only thing it reads per round
    struct DcSweepRecord
    {
        int n_failing;          // valid pairs whose last attempt failed
        int n_newly_converged;  // ... that were solved since the last classification and converged
        int n_reseeded;         // failing pairs given a seed for the next round
        int pad;
        long long iters;        // Newton iterations of the attempts classified (a non-converged attempt counts the cap)
    };

    // What the sweep's kernels read and write besides the sweep engine's view (kept out of DevView: its size is part of k_tr_steps' register
    // allocation).  All pointers are device memory.
    struct DcSweepView
    {
        int P;                    // slots per pass: the sweep engine's batch is (circuit batch) x P
        int n_inst;               // circuit batch
        int n_valid;              // slots of this pass that hold a point (the rest repeat the last one: solved once, never gathered or used as seeds)
        int slot;                 // index of the swept value in the device value vector, -1: the device has an unconnected pin
        int trace;                // 1: TRACE layout, P == 2 -- slot 0 is the working copy, slot 1 the shadow of the last converged state
        int attempt_cap;          // iterations a non-converged attempt has spent (max_newton; 1 for a linear circuit)
        double const* value;      // [P] what the swept slot holds at each slot of the pass (PE_HIP_R: 1 / r, divided on the host)
        int const* point;         // [P] the caller's index of each slot's point, -1: unused slot
        int const* rank;          // [P] dense rank of the slot's value inside the pass: equal values share a rank (distance 0)
        // the main engine's state of circuit instance b: source of round 0 (read only)
        double const *m_x, *m_udlast, *m_geq, *m_dv, *m_t_now, *m_last_step;
        int const* m_rl;
        int* seed_of;             // [n_inst * P] source instance of the next seed launch, -1: none
        unsigned long long* scan; // [n_inst * P] scratch of the classification (nearest converged slot to the left)
        int* pair_status;         // [n_inst * P] status of the pair's last attempt (0: converged)
        int* pair_iters;          // [n_inst * P] Newton iterations of that attempt when it converged
        int* pair_seed;           // [n_inst * P] the caller's index of the point its last attempt was seeded from, -1: the main engine's state
        DcSweepRecord* rec;
        int n_keep;               // kept rows per point (no selection: every row)
        int const* keep;          // [n_keep] rows of x, or null: all rows
        double* res;              // [n_points][n_inst][n_keep] results in the caller's order, NaN where the pair failed
        int *res_status, *res_iters, *res_seed;  // [n_points][n_inst]
    };

    // the swept slot of sweep-engine instance q
    template <class Team>
    PE_DEV void dc_sweep_fill(Team const& tm, DevView const& V, DcSweepView const& S)
    {
        if(S.slot < 0) return;
        for(int q = tm.tid(); q < V.batch; q += tm.size()) V.dv[static_cast<long long>(q) * V.dv_len + S.slot] = S.value[q % S.P];
    }

    // state of destination q from source S.seed_of[q]: the arrays a DC solve reads.  from_main: the source is a circuit instance of the main
    // engine (round 0: its device value vector and time too, and the iteration counter starts at 0); else a converged instance of the sweep
    // engine itself -- sources are converged, destinations failed (TRACE: working copy and shadow), so the two sets are disjoint.
    template <class Team>
    PE_DEV void dc_sweep_seed(Team const& tm, DevView const& V, DcSweepView const& S, int q, bool from_main)
    {
        int const src = S.seed_of[q];
        if(src < 0) return;
        long long const d = q, s = src;
        double const* sx = (from_main ? S.m_x : V.x) + s * V.rows;
        double const* su = (from_main ? S.m_udlast : V.d_udlast) + s * V.nD;
        double const* sg = (from_main ? S.m_geq : V.d_geq) + s * V.nD;
        int const* sr = (from_main ? S.m_rl : V.rl_engaged) + s * V.nRl;
        for(int r = tm.tid(); r < V.rows; r += tm.size()) V.x[d * V.rows + r] = sx[r];
        for(int i = tm.tid(); i < V.nD; i += tm.size())
        {
            V.d_udlast[d * V.nD + i] = su[i];
            V.d_geq[d * V.nD + i] = sg[i];
        }
        for(int i = tm.tid(); i < V.nRl; i += tm.size()) V.rl_engaged[d * V.nRl + i] = sr[i];
        if(from_main)
            for(int i = tm.tid(); i < V.dv_len; i += tm.size()) V.dv[d * V.dv_len + i] = S.m_dv[s * V.dv_len + i];
        if(tm.tid() == 0)
        {
            if(from_main)
            {
                V.t_now[q] = S.m_t_now[src];
                V.last_step[q] = S.m_last_step[src];
                V.n_iters[q] = 0;
                S.pair_seed[q] = -1;
            }
            else if(!S.trace)
                S.pair_seed[q] = S.point[src % S.P];
        }
    }

    // this thread's share of the finiteness flag of instance q's solution (1: something is not finite)
    template <class Team>
    PE_DEV int dc_sweep_nonfinite(Team const& tm, DevView const& V, int q)
    {
        double const* x = V.x + static_cast<long long>(q) * V.rows;
        int bad = 0;
        for(int r = tm.tid(); r < V.rows; r += tm.size())
            if(!(fabs(x[r]) <= 1.7976931348623157e308)) bad = 1;
        return bad;
    }

    // Bookkeeping of pair q after a solve (one thread, `nonfinite` = the instance's reduced flag).  A pair that was parked during the solve
    // keeps what it has.  Returns 1 when the pair's last attempt converged; adds to the caller's private counters.
    PE_DEV int dc_sweep_book(DevView const& V, DcSweepView const& S, int q, int nonfinite, int& n_newly, long long& iters)
    {
        int st = V.status[q];
        if(st != DC_SWEEP_PARKED)
        {
            if(st == 0 && nonfinite) st = DC_SWEEP_NONFINITE;
            long long const it = V.n_iters[q];
            V.n_iters[q] = 0;
            S.pair_status[q] = st;
            S.pair_iters[q] = st == 0 ? static_cast<int>(it) : 0;
            iters += st == 0 ? it : (st == -4 ? S.attempt_cap : 0);  // (-4: PE_HIP_ERR_NO_CONVERGENCE)
            if(st == 0) ++n_newly;
        }
        return S.pair_status[q] == 0 ? 1 : 0;
    }

    // The nearest-converged rule over scan keys.  Left candidates: the key of a converged slot p is (rank << 32) | (2^32 - 1 - p) and the
    // scan takes the MAXIMUM (highest rank, then lowest slot), 0 = none.  Right candidates: (rank << 32) | p, scan takes the MINIMUM
    // (lowest rank, then lowest slot), all ones = none.
    PE_DEV unsigned long long dc_sweep_key_left(int conv, int rank, int p)
    {
        return conv ? (static_cast<unsigned long long>(static_cast<unsigned>(rank)) << 32) | (0xFFFFFFFFull - static_cast<unsigned>(p)) : 0ull;
    }
    PE_DEV unsigned long long dc_sweep_key_right(int conv, int rank, int p)
    {
        return conv ? (static_cast<unsigned long long>(static_cast<unsigned>(rank)) << 32) | static_cast<unsigned>(p) : ~0ull;
    }
    // slot of the seed of a failing slot of rank `rank`, -1: no converged slot.  Distance = difference of ranks; a tie goes to the lower slot,
    // which is the left candidate (it sits below the failing slot, the right one above).
    PE_DEV int dc_sweep_choose(unsigned long long left, unsigned long long right, int rank)
    {
        bool const has_l = left != 0ull, has_r = right != ~0ull;
        if(!has_l && !has_r) return -1;
        int const pl = static_cast<int>(0xFFFFFFFFull - (left & 0xFFFFFFFFull)), pr = static_cast<int>(right & 0xFFFFFFFFull);
        if(!has_r) return pl;
        if(!has_l) return pr;
        long long const dl = rank - static_cast<long long>(left >> 32), dr = static_cast<long long>(right >> 32) - rank;
        return dl <= dr ? pl : pr;
    }
    // what the classification leaves for slot p of circuit instance b: its seed (or none) and its status for the next round -- reseeded -> OK,
    // everything else parked.  Returns 1 when the pair was reseeded.
    PE_DEV int dc_sweep_decide(DevView const& V, DcSweepView const& S, int b, int p, int conv, int seed_slot, bool reseed)
    {
        int const q = b * S.P + p;
        bool const take = reseed && p < S.n_valid && !conv && seed_slot >= 0;
        S.seed_of[q] = take ? b * S.P + seed_slot : -1;
        V.status[q] = take ? 0 : DC_SWEEP_PARKED;
        return take ? 1 : 0;
    }

    // TRACE (P == 2), one thread per circuit instance after the point's solve: a converged working copy becomes the shadow, a failed one is
    // restored from it; the working copy is open for the next point either way.  pair_seed of the shadow = the point its state belongs to.
    PE_DEV void dc_sweep_trace_decide(DevView const& V, DcSweepView const& S, int b, int conv)
    {
        int const w = 2 * b, s = 2 * b + 1;
        S.pair_seed[w] = S.pair_seed[s];
        if(conv) S.pair_seed[s] = S.point[0];
        S.seed_of[w] = conv ? -1 : s;
        S.seed_of[s] = conv ? w : -1;
        V.status[w] = 0;
        V.status[s] = DC_SWEEP_PARKED;
    }

    // the kept rows of instance q into the result at the caller's index of its point, NaN for a failed pair; its bookkeeping beside them
    template <class Team>
    PE_DEV void dc_sweep_gather(Team const& tm, DevView const& V, DcSweepView const& S, int q)
    {
        int const b = q / S.P, p = q - b * S.P;
        if(p >= S.n_valid || (S.trace && p != 0)) return;
        int const pt = S.point[p];
        if(pt < 0) return;
        bool const ok = S.pair_status[q] == 0;
        double const* x = V.x + static_cast<long long>(q) * V.rows;
        long long const o = static_cast<long long>(pt) * S.n_inst + b;
        for(int k = tm.tid(); k < S.n_keep; k += tm.size()) S.res[o * S.n_keep + k] = ok ? x[S.keep ? S.keep[k] : k] : NAN;
        if(tm.tid() == 0)
        {
            S.res_status[o] = S.pair_status[q];
            S.res_iters[o] = S.pair_iters[q];
            S.res_seed[o] = S.pair_seed[q];
        }
    }

#if !defined(__HIPCC__)
    // the whole classification by one thread (builds without HIP; the device runs the same helpers under wavefront scans)
    inline void dc_sweep_classify_serial(DevView const& V, DcSweepView const& S, bool reseed)
    {
        struct One
        {
            int tid() const { return 0; }
            int size() const { return 1; }
        };
        for(int b = 0; b < S.n_inst; ++b)
        {
            int n_newly = 0, n_failing = 0, n_reseeded = 0;
            long long iters = 0;
            if(S.trace)
            {
                int const conv = dc_sweep_book(V, S, 2 * b, dc_sweep_nonfinite(One{}, V, 2 * b), n_newly, iters);
                dc_sweep_trace_decide(V, S, b, conv);
                n_failing = conv ? 0 : 1;
            }
            else
            {
                for(int p = 0; p < S.n_valid; ++p)
                {
                    int const q = b * S.P + p;
                    if(!dc_sweep_book(V, S, q, dc_sweep_nonfinite(One{}, V, q), n_newly, iters)) ++n_failing;
                }
                unsigned long long run = 0ull;
                for(int p = 0; p < S.n_valid; ++p)
                {
                    unsigned long long const k = dc_sweep_key_left(S.pair_status[b * S.P + p] == 0, S.rank[p], p);
                    run = k > run ? k : run;
                    S.scan[b * S.P + p] = run;
                }
                run = ~0ull;
                for(int p = S.P - 1; p >= 0; --p)
                {
                    int const q = b * S.P + p;
                    int const conv = p < S.n_valid && S.pair_status[q] == 0;
                    if(p < S.n_valid)
                    {
                        unsigned long long const k = dc_sweep_key_right(conv, S.rank[p], p);
                        run = k < run ? k : run;
                    }
                    int const seed = p < S.n_valid && !conv ? dc_sweep_choose(S.scan[q], run, S.rank[p]) : -1;
                    n_reseeded += dc_sweep_decide(V, S, b, p, conv, seed, reseed);
                }
            }
            S.rec->n_failing += n_failing;
            S.rec->n_newly_converged += n_newly;
            S.rec->n_reseeded += n_reseeded;
            S.rec->iters += iters;
        }
    }
#endif
}  // namespace pe
