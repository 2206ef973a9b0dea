// pe_noise.hpp -- small-signal noise analysis (pe_engine_ac.cpp pe_hip_analyze_noise): the per-element code of its kernels, team-generic
// like pe_ac_sweep.hpp.  The adjoint system (pe_ac.hpp AcAdjoint) is solved once per frequency point as an instance of the sweep's AC
// engine; its solution y gives every source's transfer to the output at once: a white current source of one-sided density S_k [A^2/Hz]
// between rows a, b contributes S_k |y_b - y_a|^2 to the output density.  pe_kernels.hip runs this text with a grid team
// (k_noise_sources / k_noise_accumulate / k_noise_finish), builds without HIP with a one-thread team (the serial launchers at the end of
// pe_engine_ac.cpp).  Only tid() and size() of the team are used.
#pragma once
#include "pe_ac_sweep.hpp"
#include "pe_device.hpp"

#include <cmath>

namespace pe
{
    // the constants of the models (pe_circuit.cpp)
    constexpr double NOISE_K_BOLTZMANN = 1.380650524e-23;
    constexpr double NOISE_Q_ELEMENT = 1.6021765314e-19;
    constexpr double NOISE_TEMP_DEFAULT = 300.15;  // the models' default Temp of 27 degrees C
    constexpr int NOISE_KIND_BJT_NPN = 20;         // PE_HIP_BJT_NPN in DevView::n3_kind (checked against the enum in pe_engine_ac.cpp)

    // how the density of a source follows from the resident operating point
    enum NoiseSourceType : int
    {
        NOISE_NONE = 0,    // a device whose AC stamp is skipped (unconnected pin): enumerated, S = 0
        NOISE_R = 1,       // resistor idx:   4 k T |g|,  g = dv[dv_r + idx] (kept equal to the host's r_g that AcSlot::R_G is filled from)
        NOISE_DIODE = 2,   // junction idx:   2 q |geq V_d(x) + Ieq|, conduction current of the last linearisation
        NOISE_MOS = 3,     // n3 device idx:  (8/3) k T |gm|
        NOISE_BJT_B = 4,   // n3 device idx:  2 q |geq V_j(x) + Ieq_be|
        NOISE_BJT_C = 5    // n3 device idx:  2 q |gm V_j(x) + Ieq_c|
    };
    struct alignas(16) NoiseSource
    {
        int type, idx, a, b;  // NoiseSourceType, index in its device array, the two rows (-1: ground)
    };
    struct alignas(8) NoiseRows
    {
        int a, b;
    };

    constexpr int NOISE_THREADS = 256;                  // workgroup of k_noise_accumulate
    constexpr int NOISE_CHUNK = NOISE_THREADS * 8;      // sources per workgroup: the summation order depends on n_src and these two only

    // What the noise kernels read and write (kept out of DevView like AcSweepView).  All pointers are device memory.
    struct NoiseView
    {
        int n_src;               // sources of the circuit
        int n_chunks;            // ceil(n_src / NOISE_CHUNK)
        int n_inst;              // circuit batch
        int P;                   // points per pass of the adjoint engine: its instance q = b * P + p
        int n_half;              // N: rows of the complex system
        double temp_k;           // circuit temperature of the thermal sources
        NoiseSource const* src;  // [n_src] the source table (host-built once per circuit)
        NoiseRows* rows;         // [n_src] the two rows of every source, shared by the instances (k_noise_sources fills it)
        double* S;               // [n_inst][n_src] densities of this call, A^2/Hz
        double const* xacc;      // [n_inst * P][2N] refined solution of the adjoint system (AcSweepView::xacc)
        int const* point;        // [P] the caller's index of each point of this pass, -1: unused
        double* partial;         // [n_inst * P][n_chunks] chunk sums of a pass (n_chunks > 1 only)
        double* psd;             // [n_points][n_inst] output density in the caller's point order
        double* contrib;         // null, or [n_points][n_inst][n_src]: S_k |y_b - y_a|^2 of every source
    };

    PE_DEV double noise_row(double const* x, int r) { return r >= 0 ? x[r] : 0.0; }

    // density of source k of circuit instance b from the main engine's resident state
    PE_DEV double noise_density(DevView const& V, NoiseView const& Z, int b, int k)
    {
        NoiseSource const s = Z.src[k];
        double const* dv = V.dv + static_cast<long long>(b) * V.dv_len;
        double const* x = V.x + static_cast<long long>(b) * V.rows;
        switch(s.type)
        {
            case NOISE_R: return 4.0 * NOISE_K_BOLTZMANN * Z.temp_k * fabs(dv[V.dv_r + s.idx]);
            case NOISE_DIODE:
            {
                long long const o = static_cast<long long>(b) * V.nD + s.idx;
                double const geq = V.d_geq[o];
                double ieq = dv[V.dv_di + s.idx];
                // a transient stamp folds the diffusion-capacitance companion into the two slots (pe_front.hpp: g = geq + prevg,
                // ie = Ieq + hist); only the conduction current is a shot-noise current
                if(dv[V.dv_dg + s.idx] != geq) ieq -= V.d_hist[o];
                double const vd = noise_row(x, V.d_a[s.idx]) - noise_row(x, V.d_c[s.idx]);
                return 2.0 * NOISE_Q_ELEMENT * fabs(geq * vd + ieq);
            }
            case NOISE_MOS: return (8.0 / 3.0) * NOISE_K_BOLTZMANN * Z.temp_k * fabs(dv[V.n3_dv[s.idx] + 1]);
            case NOISE_BJT_B:
            case NOISE_BJT_C:
            {
                int const* n = V.n3_n + 3 * s.idx;  // B, C, E
                double const vbe = noise_row(x, n[0]) - noise_row(x, n[2]);
                double const vj = V.n3_kind[s.idx] == NOISE_KIND_BJT_NPN ? vbe : -vbe;  // NPN: Vbe | PNP: Veb (pe_front.hpp)
                double const* d = dv + V.n3_dv[s.idx];  // geq, Ieq_be, gm, Ieq_c
                return 2.0 * NOISE_Q_ELEMENT * fabs(s.type == NOISE_BJT_B ? d[0] * vj + d[1] : d[2] * vj + d[3]);
            }
            default: return 0.0;
        }
    }

    // S[b][.] of circuit instance b; instance 0 also writes the shared row pairs.  Consecutive threads store consecutive doubles.
    template <class Team>
    PE_DEV void noise_sources(Team const& tm, DevView const& V, NoiseView const& Z, int b)
    {
        double* S = Z.S + static_cast<long long>(b) * Z.n_src;
        for(int k = tm.tid(); k < Z.n_src; k += tm.size())
        {
            S[k] = noise_density(V, Z, b, k);
            if(b == 0) Z.rows[k] = NoiseRows{Z.src[k].a, Z.src[k].b};
        }
    }

    // This thread's share of chunk c of adjoint-engine instance q: the sources c * NOISE_CHUNK + tid, + size, ... in ascending order.
    // Streams S and the row pairs, gathers the four doubles of y, stores the contributions when they are kept.  An unused pass slot
    // does nothing (the caller skips its stores too: see noise_slot_point).
    template <class Team>
    PE_DEV double noise_accumulate_chunk(Team const& tm, NoiseView const& Z, int rows2, int q, int c)
    {
        int const b = q / Z.P;
        int const pt = Z.point[q - b * Z.P];
        if(pt < 0) return 0.0;
        double const* y = Z.xacc + static_cast<long long>(q) * rows2;
        double const* S = Z.S + static_cast<long long>(b) * Z.n_src;
        double* out = Z.contrib ? Z.contrib + (static_cast<long long>(pt) * Z.n_inst + b) * Z.n_src : nullptr;
        int const k1 = (c + 1) * NOISE_CHUNK < Z.n_src ? (c + 1) * NOISE_CHUNK : Z.n_src;
        double acc = 0.0;
        for(int k = c * NOISE_CHUNK + tm.tid(); k < k1; k += tm.size())
        {
            NoiseRows const r = Z.rows[k];
            double const dre = noise_row(y, r.b) - noise_row(y, r.a);
            double const dim = (r.b >= 0 ? y[Z.n_half + r.b] : 0.0) - (r.a >= 0 ? y[Z.n_half + r.a] : 0.0);
            double const ck = S[k] * (dre * dre + dim * dim);
            if(out) out[k] = ck;
            acc += ck;
        }
        return acc;
    }
    // where the sum of instance q goes: psd[point][b], or nowhere for an unused slot
    PE_DEV double* noise_slot_psd(NoiseView const& Z, int q)
    {
        int const b = q / Z.P;
        int const pt = Z.point[q - b * Z.P];
        return pt < 0 ? nullptr : Z.psd + static_cast<long long>(pt) * Z.n_inst + b;
    }
    // second stage (n_chunks > 1): the chunk sums of instance q in ascending chunk order
    PE_DEV void noise_finish(NoiseView const& Z, int q)
    {
        double* dst = noise_slot_psd(Z, q);
        if(!dst) return;
        double const* p = Z.partial + static_cast<long long>(q) * Z.n_chunks;
        double acc = 0.0;
        for(int c = 0; c < Z.n_chunks; ++c) acc += p[c];
        *dst = acc;
    }
}  // namespace pe
