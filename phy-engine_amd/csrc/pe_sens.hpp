// pe_sens.hpp -- DC sensitivity analysis (pe_engine_ac.cpp pe_hip_analyze_sens): the per-element code of its kernels, team-generic like
// pe_noise.hpp.  With the residual f(x, p) = A(x; p) x - b(x; p) of the resident operating point and J^T y = e_out (the adjoint
// small-signal system of pe_ac.hpp at omega = 0, one instance of the sweep's engine per output), d out / d p_k = -y^T d f / d p_k.
//
// Every parameter reaches f through value slots of the main engine's value vector dv, and the contribution lists of pe_circuit.cpp say
// where a slot is stamped: an A entry (row r, column c, sign) adds +-dv_j x[c] to f_r, a right-hand-side entry (row r, sign) takes
// +-dv_j from it.  Those lists, transposed to "by slot" (SensView::sl_ptr / sl_ent, host-built once per circuit from the lists the stamp
// kernel gathers from, after their '=' cells were resolved), give g_j = -y^T d f / d dv_j with every sign taken from the stamp itself:
// sens_slot.  A parameter is then a handful of operations: s_k = sum_j g_j d dv_j / d p_k at the resident x.  For a non-linear device the
// companion pair (g, Ieq = I - g V) moves with p such that d g / d p drops out of f: only d I / d p at fixed x through the slot of Ieq
// remains, evaluated on the arm of the model that eval_devices (pe_front.hpp) takes at x, with the chain rule through the derived
// columns of pe_circuit.cpp (diode_derive, gen_derive) from the raw columns, which the host uploads once per call.
// pe_kernels.hip runs this text with a grid team (k_sens_rhs) and a workgroup team (k_sens_accumulate), builds without HIP with a
// one-thread team (the serial launchers at the end of pe_engine_ac.cpp).  Only tid() and size() of the team are used.
#pragma once
#include "pe_ac_sweep.hpp"
#include "pe_device.hpp"

#include <cmath>

namespace pe
{
    // how s_k follows from the slot sensitivities
    enum SensType : int
    {
        SENS_NONE = 0,   // a device with an unconnected pin (no stamp): enumerated, reads 0
        SENS_R = 1,      // aux: slot of g = 1 / R            d g / d R = -g^2
        SENS_UNIT = 2,   // aux: slot that holds the parameter itself (VDC, IDC, controlled-source gains, transformer ratio)
        SENS_XCT = 3,    // aux: slot of 1 / (2 n_total)      d / d n_total = -2 slot^2; n_total = 0 (slot 0): reads 0
        SENS_DIODE = 4,  // idx: junction, col: raw column (PE_HIP_DIODE columns 0-6, 8), aux: slot of its Ieq
        SENS_MOS = 5,    // idx: n3 device, col: Kp, lambda, Vth
        SENS_BJT = 6     // idx: n3 device, col: Is, N, BetaF, Temp, Area; aux: offset of its raw columns in one instance's block of g_raw
    };
    struct alignas(16) SensParam
    {
        int type, idx, col, aux;
    };
    // one stamp of a value slot: rs = (row << 1) | negated, c = column of an A entry or -1 for a right-hand-side entry
    struct alignas(8) SensEnt
    {
        int rs, c;
    };

    constexpr int SENS_THREADS = 256;                // workgroup of k_sens_accumulate
    constexpr int SENS_CHUNK = SENS_THREADS * 8;     // parameters per workgroup: the summation order depends on n_par and these two only
    constexpr int SENS_DIODE_NRAW = 11;              // PE_HIP_DIODE_NPARAM (checked against the C header in pe_engine_ac.cpp)
    constexpr int SENS_KIND_NMOS = 18;               // PE_HIP_NMOS, PE_HIP_BJT_NPN in DevView::n3_kind (checked likewise)
    constexpr int SENS_KIND_BJT_NPN = 20;
    // the constants of the models' thermal voltage (pe_circuit.cpp)
    constexpr double SENS_K_BOLTZMANN = 1.380650524e-23;
    constexpr double SENS_Q_ELEMENT = 1.6021765314e-19;
    constexpr double SENS_KELVIN = -273.15;

    // What the sensitivity kernels read and write (kept out of DevView like NoiseView).  All pointers are device memory.
    struct SensView
    {
        int n_par;               // parameters of the circuit
        int n_chunks;            // ceil(n_par / SENS_CHUNK), at least 1
        int n_inst;              // circuit batch
        int P;                   // outputs per pass of the adjoint engine: its instance q = b * P + p
        int n_half;              // N: rows of the system (the real half of the adjoint engine's 2N)
        int gen_par_len;         // doubles of one instance's block of g_raw
        int normalized;          // 1: s_k is p_k d out / d p_k (0 where p_k == 0)
        int rhs0;                // first of the 2N right-hand-side slots of the adjoint engine's value vector
        SensParam const* par;    // [n_par] the parameter table (host-built once per circuit)
        int const* sl_ptr;       // [dv_len + 1] stamps of every value slot of the main engine ...
        SensEnt const* sl_ent;   // ... in the order of the contribution lists
        double const* d_raw;     // [n_inst][nD][SENS_DIODE_NRAW] raw junction columns of this call
        double const* g_raw;     // [n_inst][gen_par_len] raw columns of the generic devices of this call
        double const* weight;    // null, or [n_par]
        int const* out_pos;      // [n_outputs] rows of every output (-1: ground)
        int const* out_neg;
        double const* xacc;      // [n_inst * P][2N] refined solution of the adjoint system (AcSweepView::xacc)
        int const* point;        // [P] the caller's output index of each slot of this pass, -1: unused
        double* partial;         // [n_inst * P][n_chunks] chunk sums of a pass (weight and n_chunks > 1 only)
        double* rss;             // null (no weight), or [n_outputs][n_inst]
        double* s;               // null (not kept), or [n_outputs][n_inst][n_par]
    };

    // right-hand side of adjoint-engine instance q: the selector of its slot's own output in the real half, zero elsewhere (an unused slot
    // solves a zero right-hand side).  Runs after ac_sweep_fill, before the solve that the refinement takes its copy b0 from.
    template <class Team>
    PE_DEV void sens_rhs(Team const& tm, DevView const& V, SensView const& Z, int q)
    {
        int const b = q / Z.P;
        int const pt = Z.point[q - b * Z.P];
        int const pos = pt >= 0 ? Z.out_pos[pt] : -1, neg = pt >= 0 ? Z.out_neg[pt] : -1;
        double* rhs = V.dv + static_cast<long long>(q) * V.dv_len + Z.rhs0;
        for(int r = tm.tid(); r < V.rows; r += tm.size()) rhs[r] = (r == pos ? 1.0 : 0.0) - (r == neg ? 1.0 : 0.0);
    }

    // limexp of pe_front.hpp with its derivative (the linear continuation above 50 has the constant slope exp(50))
    PE_DEV double sens_limexp(double x, double& d)
    {
        if(x > 50.0)
        {
            d = exp(50.0);
            return d * (1.0 + (x - 50.0));
        }
        if(x < -50.0)
        {
            d = 0.0;
            return exp(-50.0);
        }
        d = exp(x);
        return d;
    }
    PE_DEV double sens_row(double const* x, int r) { return r >= 0 ? x[r] : 0.0; }

    // g_j = -y^T d f / d dv_j of value slot j of the main engine
    PE_DEV double sens_slot(SensView const& Z, double const* x, double const* y, int j)
    {
        double acc = 0.0;
        int const e1 = Z.sl_ptr[j + 1];
        for(int e = Z.sl_ptr[j]; e < e1; ++e)
        {
            SensEnt const s = Z.sl_ent[e];
            double const yr = y[s.rs >> 1];
            double const t = s.c >= 0 ? yr * x[s.c] : -yr;
            acc = (s.rs & 1) ? acc + t : acc - t;
        }
        return acc;
    }

    // d out / d p_k of circuit instance b against the adjoint solution y; pval: the parameter's value
    PE_DEV double sens_param(DevView const& V, SensView const& Z, int b, int k, double const* y, double& pval)
    {
        SensParam const s = Z.par[k];
        double const* dv = V.dv + static_cast<long long>(b) * V.dv_len;
        double const* x = V.x + static_cast<long long>(b) * V.rows;
        pval = 0.0;
        switch(s.type)
        {
            case SENS_R:
            {
                double const g = dv[s.aux];
                pval = 1.0 / g;
                return -(g * g) * sens_slot(Z, x, y, s.aux);
            }
            case SENS_UNIT: pval = dv[s.aux]; return sens_slot(Z, x, y, s.aux);
            case SENS_XCT:
            {
                double const v = dv[s.aux];
                if(v == 0.0) return 0.0;
                pval = 0.5 / v;
                return -2.0 * v * v * sens_slot(Z, x, y, s.aux);
            }
            case SENS_DIODE:
            {
                long long const o = static_cast<long long>(b) * V.nD + s.idx;
                double const* raw = Z.d_raw + o * SENS_DIODE_NRAW;
                double const* p = V.d_par + o * DP_NCOL;
                double const Is = raw[0], N = raw[1], Isr = raw[2], Nr = raw[3], Temp = raw[4], Ibv = raw[5], Area = raw[8];
                pval = raw[s.col];
                double const c_t = SENS_K_BOLTZMANN / SENS_Q_ELEMENT;
                double const Ut = SENS_K_BOLTZMANN * (Temp - SENS_KELVIN) / SENS_Q_ELEMENT;
                double const Is_eff = p[DP_IS_EFF], Isr_eff = p[DP_ISR_EFF], Ute = p[DP_UTE], Uter = p[DP_UTER], Bv_eff = p[DP_BV_EFF];
                bool const Bv_set = p[DP_BV_SET] != 0.0;
                double const Ud = sens_row(x, V.d_a[s.idx]) - sens_row(x, V.d_c[s.idx]);
                // d Id / d (Is_eff, Isr_eff, Ute, Uter, Bv_eff at fixed Is_eff) on the arm eval_devices takes at Ud
                double dIs, dIsr = 0.0, dUte, dUter = 0.0, dBv = 0.0;
                if(Bv_set && Ud < -Bv_eff)
                {
                    double const z = -(Bv_eff + Ud) / Ute;
                    double e1;
                    double const e = sens_limexp(z, e1);
                    // (Is_eff also moves Bv_eff, by N Ut / Is_eff: taken together here, -e + e1, which is exactly 0 below the linear
                    // continuation -- the breakdown current -Ibv exp(-(Bv + Ud) / Ute) does not depend on Is)
                    dIs = e1 - e;
                    dUte = Is_eff * e1 * z / Ute;
                    dBv = Is_eff * e1 / Ute;
                }
                else
                {
                    double const z = Ud / Ute, zr = Ud / Uter;
                    double e1, er1;
                    dIs = sens_limexp(z, e1) - 1.0;
                    dIsr = sens_limexp(zr, er1) - 1.0;
                    dUte = -Is_eff * e1 * z / Ute;
                    dUter = -Isr_eff * er1 * zr / Uter;
                }
                // Bv_eff = Bv - N Ut ln(Ibv / Is_eff) when Bv is set (diode_derive); on the other arm dBv is 0 and none of this is evaluated
                double const L = dBv != 0.0 ? log(Ibv / Is_eff) : 0.0;
                double d = 0.0;
                switch(s.col)
                {
                    case 0: d = dIs * Area; break;
                    case 1: d = dUte * Ut - dBv * Ut * L; break;
                    case 2: d = dIsr * Area; break;
                    case 3: d = dUter * Ut; break;
                    case 4: d = dUte * N * c_t + dUter * Nr * c_t - dBv * N * c_t * L; break;
                    case 5: d = dBv != 0.0 ? -dBv * Ute / Ibv : 0.0; break;
                    case 6: d = dBv; break;
                    case 8: d = dIs * Is + dIsr * Isr; break;
                    default: break;
                }
                return d * sens_slot(Z, x, y, s.aux);
            }
            case SENS_MOS:
            {
                // Shichman-Hodges level 1 as eval_devices writes it; the drain current enters f through the slot of Ieq (n3_dv + 2)
                double const* p = V.n3_par + (static_cast<long long>(b) * V.nN3 + s.idx) * 3;
                int const* n = V.n3_n + 3 * s.idx;  // D, G, S
                double const v0 = sens_row(x, n[0]), v1 = sens_row(x, n[1]), v2 = sens_row(x, n[2]);
                double const Kp = p[0], lambda = p[1], Vth = p[2];
                pval = p[s.col];
                bool const nmos = V.n3_kind[s.idx] == SENS_KIND_NMOS;
                double const Vc = nmos ? v1 - v2 : v2 - v1;
                double const Vds = v0 - v2;
                double const Vx = nmos ? Vds : -Vds;
                double const Vov = Vc - Vth;
                double d = 0.0;
                if(Vov <= 0.0) {}
                else if(Vx < Vov)
                {
                    double const B = Vov * Vx - 0.5 * Vx * Vx;
                    d = s.col == 0 ? B * (1.0 + lambda * Vx) : s.col == 1 ? Kp * B * Vx : -Kp * Vx * (1.0 + lambda * Vx);
                }
                else
                    d = s.col == 0 ? 0.5 * Vov * Vov * (1.0 + lambda * Vx) : s.col == 1 ? 0.5 * Kp * Vov * Vov * Vx : -Kp * Vov * (1.0 + lambda * Vx);
                if(d == 0.0) return 0.0;
                return (nmos ? d : -d) * sens_slot(Z, x, y, V.n3_dv[s.idx] + 2);
            }
            case SENS_BJT:
            {
                // forward-active Ebers-Moll as eval_devices writes it: Ij through the slot of Ieq_be (n3_dv + 1), BetaF Ij through Ieq_c (+ 3)
                double const* p = V.n3_par + (static_cast<long long>(b) * V.nN3 + s.idx) * 3;
                double const* raw = Z.g_raw + static_cast<long long>(b) * Z.gen_par_len + s.aux;  // Is, N, BetaF, Temp, Area
                int const* n = V.n3_n + 3 * s.idx;  // B, C, E
                pval = raw[s.col];
                double const Is_eff = p[0], Ute = p[1], BetaF = p[2];
                double const vbe = sens_row(x, n[0]) - sens_row(x, n[2]);
                double const Vj = V.n3_kind[s.idx] == SENS_KIND_BJT_NPN ? vbe : -vbe;
                double const e = exp(Vj / Ute);
                double const dIs = e - 1.0, dUte = -Is_eff * e * Vj / (Ute * Ute);
                double const Ut = SENS_K_BOLTZMANN * (raw[3] - SENS_KELVIN) / SENS_Q_ELEMENT;
                int const o = V.n3_dv[s.idx];
                if(s.col == 2) return Is_eff * dIs * sens_slot(Z, x, y, o + 3);
                double const dIj = s.col == 0   ? dIs * raw[4]
                                   : s.col == 1 ? dUte * Ut
                                   : s.col == 3 ? dUte * raw[1] * (SENS_K_BOLTZMANN / SENS_Q_ELEMENT)
                                                : dIs * raw[0];
                return dIj * (sens_slot(Z, x, y, o + 1) + BetaF * sens_slot(Z, x, y, o + 3));
            }
            default: return 0.0;
        }
    }

    // This thread's share of chunk c of adjoint-engine instance q: the parameters c * SENS_CHUNK + tid, + size, ... in ascending order.
    // Streams the table, gathers the rows of y, stores s when kept; returns the thread's sum of (w_k s_k)^2 (0 without weights), formed as
    // acc = fma(t, t, acc) with t = w_k s_k.  An unused pass slot does nothing (the caller skips its stores too: see sens_slot_rss).
    template <class Team>
    PE_DEV double sens_accumulate_chunk(Team const& tm, DevView const& V, SensView const& Z, int rows2, int q, int c)
    {
        int const b = q / Z.P;
        int const pt = Z.point[q - b * Z.P];
        if(pt < 0) return 0.0;
        double const* y = Z.xacc + static_cast<long long>(q) * rows2;
        double* out = Z.s ? Z.s + (static_cast<long long>(pt) * Z.n_inst + b) * Z.n_par : nullptr;
        int const k1 = (c + 1) * SENS_CHUNK < Z.n_par ? (c + 1) * SENS_CHUNK : Z.n_par;
        double acc = 0.0;
        for(int k = c * SENS_CHUNK + tm.tid(); k < k1; k += tm.size())
        {
            double pval;
            double sk = sens_param(V, Z, b, k, y, pval);
            if(Z.normalized) sk = pval == 0.0 ? 0.0 : pval * sk;
            if(out) out[k] = sk;
            if(Z.weight)
            {
                double const t = Z.weight[k] * sk;
                acc = fma(t, t, acc);  // (spelled out: the same operation on the device and in the builds without HIP)
            }
        }
        return acc;
    }
    // where the sum of instance q goes: rss[output][b], or nowhere for an unused slot or a call without weights
    PE_DEV double* sens_slot_rss(SensView const& Z, int q)
    {
        int const b = q / Z.P;
        int const pt = Z.point[q - b * Z.P];
        return (pt < 0 || !Z.rss) ? nullptr : Z.rss + static_cast<long long>(pt) * Z.n_inst + b;
    }
    // second stage (n_chunks > 1): the chunk sums of instance q in ascending chunk order
    PE_DEV void sens_finish(SensView const& Z, int q)
    {
        double* dst = sens_slot_rss(Z, q);
        if(!dst) return;
        double const* p = Z.partial + static_cast<long long>(q) * Z.n_chunks;
        double acc = 0.0;
        for(int c = 0; c < Z.n_chunks; ++c) acc += p[c];
        *dst = acc;
    }
}  // namespace pe
