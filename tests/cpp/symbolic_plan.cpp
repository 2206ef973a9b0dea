// symbolic_plan.cpp -- pins the plans of the symbolic analysis (pe_symbolic.hpp) bit for bit.
//
// A Symbolic is a bag of integer vectors and a few scalars; every plan the kernels walk comes out of pe::analyze and
// pe::build_assembly_lists.  This program builds a corpus of patterns in memory, analyses each under the option sets the engine's policy
// uses, and prints one line per case: the outcome, a few scalars, and an FNV-1a-64 hash per GROUP of fields, so that a difference says
// where it is.  tests/test_symbolic_plan.py compares the lines with tests/golden/symbolic_plans.json.
//
// The program itself checks that every case takes the path it is there for (exit 2 otherwise): the pin cannot go vacuous.
// Corpus values come from integer arithmetic only (an LCG; no <random> distributions, whose output differs between standard libraries).
// Built from csrc/pe_symbolic.cpp alone (tests/cpp/Makefile, targets symplan / symplan_san); exit 0 = every case ran and every check held.
#include "pe_symbolic.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace
{
    struct Rng  // Knuth's 64-bit LCG, the high bits
    {
        std::uint64_t x;
        unsigned next()
        {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            return static_cast<unsigned>(x >> 33);
        }
        int below(int k) { return static_cast<int>(next() % static_cast<unsigned>(k)); }
        double unit() { return (1 + below(1000)) / 1000.0; }  // 0.001 .. 1.000
    };

    struct Matrix
    {
        int n{};
        std::vector<std::map<int, double>> rows;
        std::vector<int> rp, ci;
        std::vector<double> v;
        explicit Matrix(int n_) : n(n_), rows(static_cast<size_t>(n_)) {}
        void set(int i, int j, double a) { rows[static_cast<size_t>(i)][j] = a; }
        void finish()
        {
            rp.assign(1, 0);
            ci.clear();
            v.clear();
            for(auto const& r: rows)
            {
                for(auto const& [c, a]: r)
                {
                    ci.push_back(c);
                    v.push_back(a);
                }
                rp.push_back(static_cast<int>(ci.size()));
            }
        }
    };

    // undirected graph -> diagonally dominant matrix on its pattern (values not symmetric)
    Matrix from_edges(int n, std::vector<std::pair<int, int>> const& edges, std::uint64_t seed, int extra = 0)
    {
        Matrix M(n + extra);
        Rng g{seed};
        std::vector<double> sum(static_cast<size_t>(n), 0.0);
        for(auto const& [a, b]: edges)
        {
            if(a == b) continue;
            double const w1 = g.unit(), w2 = g.unit();
            M.set(a, b, -w1);
            M.set(b, a, -w2);
        }
        for(int i = 0; i < n; ++i)
        {
            double s = 1.0;
            for(auto const& [c, a]: M.rows[static_cast<size_t>(i)]) s += -a;
            M.set(i, i, s);
        }
        return M;
    }
    std::vector<std::pair<int, int>> mesh_edges(int k)
    {
        std::vector<std::pair<int, int>> e;
        for(int y = 0; y < k; ++y)
            for(int x = 0; x < k; ++x)
            {
                if(x + 1 < k) e.push_back({y * k + x, y * k + x + 1});
                if(y + 1 < k) e.push_back({y * k + x, (y + 1) * k + x});
            }
        return e;
    }
    Matrix mesh(int k, std::uint64_t seed)
    {
        Matrix M = from_edges(k * k, mesh_edges(k), seed);
        M.finish();
        return M;
    }

    // ---- FNV-1a-64 over the bytes of the fields of a group (every vector preceded by its length)
    struct Hash
    {
        std::uint64_t h{1469598103934665603ull};
        void bytes(void const* p, size_t n)
        {
            auto const* b = static_cast<unsigned char const*>(p);
            for(size_t i = 0; i < n; ++i)
            {
                h ^= b[i];
                h *= 1099511628211ull;
            }
        }
        template<class T>
        Hash& s(T const& x)
        {
            std::uint64_t const w = static_cast<std::uint64_t>(static_cast<long long>(x));
            bytes(&w, sizeof w);
            return *this;
        }
        Hash& d(double x)
        {
            std::uint64_t w;
            std::memcpy(&w, &x, sizeof w);
            bytes(&w, sizeof w);
            return *this;
        }
        template<class T>
        Hash& v(std::vector<T> const& x)
        {
            s(x.size());
            if(!x.empty()) bytes(x.data(), x.size() * sizeof(T));
            return *this;
        }
    };

    [[noreturn]] void fail(std::string const& name, char const* what)
    {
        std::fprintf(stderr, "symbolic_plan: case %s: %s\n", name.c_str(), what);
        std::exit(2);
    }
    void require(bool ok, std::string const& name, char const* what)
    {
        if(!ok) fail(name, what);
    }

    constexpr long long whole_cu = 163840 / 8 - 160 - 8;  // LDS doubles of a CU a workgroup may use (pe_engine_policy.cpp)

    // analyse + assembly lists (with the caps the launch geometry of the option set implies) + the line of the case
    bool run(std::string const& name, Matrix const& M, pe::SymbolicOptions const& opt, pe::Symbolic& S)
    {
        bool const ok = pe::analyze(M.n, M.rp.data(), M.ci.data(), M.v.empty() ? nullptr : M.v.data(), opt, S);
        bool asm_ok = false;
        if(ok)
        {
            long long const cap_wave = opt.wave_slot > 0 ? opt.wave_slot : (pe::pe_ld(opt.wave_m) + 1LL) * opt.wave_m;
            long long const cap_team = opt.panel_doubles + opt.panel_reserve - 2;
            // top levels: wide (1) on a single-circuit geometry, 2 where a front was formed against a CU's LDS (pe_engine_policy.cpp)
            std::vector<int> wide(S.top_ptr.size(), opt.shared_cu ? 0 : 1);
            for(size_t l = 0; l + 1 < S.top_ptr.size(); ++l)
                for(int k = S.top_ptr[l]; k < S.top_ptr[l + 1]; ++k)
                {
                    int const s = S.top_list[static_cast<size_t>(k)], p = S.f_p[static_cast<size_t>(s)], u = S.f_u[static_cast<size_t>(s)];
                    if(p > opt.max_pivots || static_cast<long long>(pe::pe_ld(p + u)) * p + static_cast<long long>(pe::pe_ld(p)) * u > opt.panel_doubles) wide[l] = 2;
                }
            asm_ok = pe::build_assembly_lists(S, cap_wave, cap_team, opt.n_parts > 1 ? wide.data() : nullptr, whole_cu - 2, whole_cu / 2 - 2);
        }
        Hash perm, fronts, own, stat, sched, store, cmap, quad, lists;
        perm.v(S.row_src).v(S.col_src);
        fronts.s(S.n).s(S.nnzA).s(S.nfronts).v(S.f_col0).v(S.f_p).v(S.f_u).v(S.f_parent).v(S.f_rows_ptr).v(S.f_rows).v(S.f_child_ptr).v(S.f_child);
        fronts.v(S.f_rel_ptr).v(S.f_rel).s(S.max_m).s(S.max_u).s(S.tree_depth).s(S.nnz_LU).s(S.nnz_LU_stored).d(S.flops);
        own.v(S.f_asm_ptr).v(S.asm_slot).v(S.asm_pos);
        stat.v(S.f_static).s(S.n_static_quad).s(S.static_root_doubles).v(S.row_keep);
        sched.v(S.f_kind).v(S.f_quad).v(S.f_wstack).v(S.f_wpar).s(S.wave_stack).s(S.n_parts).v(S.wave_ptr).v(S.wave_list).v(S.coop_ptr).v(S.coop_list).v(S.top_ptr).v(S.top_list);
        store.v(S.f_lptr).v(S.f_uptr).v(S.f_sptr).s(S.factor_doubles).s(S.arena_doubles).s(S.q_zero_off).s(S.wave_panel_doubles);
        cmap.v(S.f_inv_off).v(S.f_cnp).v(S.f_inv).v(S.f_bmask);
        quad.s(S.quad).s(S.q_lds_doubles).s(S.q_lds_kept).s(S.q_lds_total).v(S.q_prog).v(S.q_lists).v(S.q_lane).v(S.q_bprog);
        quad.v(S.q2_prog).v(S.q2_lists).v(S.q2_lane).s(S.n_mid).v(S.q_prog_dyn).v(S.q_lists_dyn);
        lists.s(asm_ok).v(S.f_mode).v(S.f_keep).v(S.gl_ptr).v(S.gl_rptr).v(S.gl_sptr).v(S.gl_dst).v(S.gl_cnt).v(S.gl_src);
        auto x = [](Hash const& h) { return static_cast<unsigned long long>(h.h); };
        std::printf("%s ok=%d singular=%d error=\"%s\" nfronts=%d max_m=%d nnz_LU=%lld n_row_swaps=%d perm=%016llx fronts=%016llx own=%016llx static=%016llx "
                    "schedule=%016llx storage=%016llx childmaps=%016llx quad=%016llx lists=%016llx\n",
                    name.c_str(), ok ? 1 : 0, S.structurally_singular ? 1 : 0, S.error.c_str(), S.nfronts, S.max_m, S.nnz_LU, S.n_row_swaps, x(perm), x(fronts), x(own),
                    x(stat), x(sched), x(store), x(cmap), x(quad), x(lists));
        return ok;
    }

    pe::SymbolicOptions sweep_geometry()  // a large sweep: four 4-wavefront workgroups per CU, lane-group kernel
    {
        pe::SymbolicOptions o{};
        o.n_waves = 4;
        o.wave_m = 45;
        o.wave_slot = (pe::pe_ld(35) + 1) * 35;
        o.wave_p = 16;
        o.absorb_m = 32;
        o.relax_small = 4;
        o.max_pivots = 32;
        o.n_parts = 4;
        o.part_cut = 1.0;
        o.nd_leaf = 10;
        o.quad = 1;
        o.shared_cu = 1;
        o.panel_doubles = 4688;
        return o;
    }
    pe::SymbolicOptions single_geometry()  // one large circuit: one 8-wavefront workgroup per CU, 48 parts
    {
        pe::SymbolicOptions o{};
        o.n_waves = 8;
        o.wave_m = 56;
        o.wave_p = 20;
        o.max_pivots = 48;
        o.n_parts = 48;
        o.part_cut = 1.0;
        o.nd_leaf = 10;
        return o;
    }
    int count(std::vector<int> const& v, int what) { return static_cast<int>(std::count(v.begin(), v.end(), what)); }
}  // namespace

int main()
{
    pe::Symbolic S;
    pe::SymbolicOptions const def{};

    {
        Matrix M(0);
        M.finish();
        require(run("empty", M, def, S) && S.nfronts == 0, "empty", "n == 0 must succeed with no fronts");
    }
    {
        Matrix M(1);
        M.set(0, 0, 2.0);
        M.finish();
        require(run("one", M, def, S) && S.nfronts == 1 && S.max_m == 1, "one", "n == 1 must give one front of order 1");
    }
    {
        // unknowns 1 and 2 appear in equation 0 only
        Matrix M(3);
        M.set(0, 0, 1.0), M.set(0, 1, 1.0), M.set(0, 2, 1.0), M.set(1, 0, 1.0), M.set(2, 0, 1.0);
        M.finish();
        require(!run("singular", M, def, S) && S.structurally_singular, "singular", "must be reported structurally singular");
    }

    Matrix const m12 = mesh(12, 1);
    std::vector<int> plain_rows;
    {
        require(run("mesh12", m12, def, S) && S.n_row_swaps == 0, "mesh12", "a diagonally dominant mesh keeps its diagonal");
        plain_rows = S.row_src;
    }
    {
        // branch rows (voltage sources between two nodes): zero diagonal, the matched entry is off the diagonal
        int const n0 = 144, nb = 10;
        Matrix M = from_edges(n0, mesh_edges(12), 1, nb);
        Rng g{2};
        for(int b = 0; b < nb; ++b)
        {
            int const a = g.below(n0), c = (a + 1 + g.below(n0 - 1)) % n0;
            M.set(a, n0 + b, 1.0), M.set(n0 + b, a, 1.0), M.set(c, n0 + b, -1.0), M.set(n0 + b, c, -1.0);
        }
        M.finish();
        require(run("mesh12_branches", M, def, S) && S.n_row_swaps > 0, "mesh12_branches", "branch rows must swap rows");
    }
    {
        // weak diagonal at node 0: the greedy search reaches unknown 0 through equation 1's entry of 1e-6, the weighted matching
        // through equation 12's of 0.5
        Matrix M = from_edges(144, mesh_edges(12), 1);
        M.set(0, 0, 1e-12), M.set(0, 1, 1.0), M.set(0, 12, 0.5);
        M.set(1, 0, 1e-6), M.set(1, 1, 1.0), M.set(1, 2, 1e-9), M.set(1, 13, 1e-9);
        M.set(12, 0, 0.5), M.set(12, 12, 1.0);
        M.finish();
        pe::SymbolicOptions greedy{};
        greedy.match_greedy = true;
        pe::Symbolic G;
        require(run("weak_diag_weighted", M, def, S), "weak_diag_weighted", "must succeed");
        require(run("weak_diag_greedy", M, greedy, G), "weak_diag_greedy", "must succeed");
        require(S.row_src != G.row_src, "weak_diag_greedy", "greedy and weighted matching must choose different rows");
    }
    {
        // real-equivalent form of a complex 8 x 8 mesh: conductances between the nodes, capacitors to ground at every third node
        int const h = 64;
        Matrix C = mesh(8, 3);
        Matrix M(2 * h);
        for(int i = 0; i < h; ++i)
            for(auto const& [c, a]: C.rows[static_cast<size_t>(i)])
            {
                double const re = (c == i && i % 3 == 0) ? 1e-3 : a, im = (c == i && i % 3 == 0) ? 40.0 : (c == i ? 0.25 : 0.0);
                M.set(i, c, re), M.set(i, c + h, -im), M.set(h + i, c, im), M.set(h + i, c + h, re);
            }
        M.finish();
        pe::SymbolicOptions o{};
        o.match_pairs = true;
        require(run("paired", M, o, S), "paired", "must succeed");
        int imag = 0;
        for(int k = 0; k < 2 * h; ++k) imag += S.col_src[static_cast<size_t>(k)] < h && S.row_src[static_cast<size_t>(k)] >= h;
        require(imag > 0, "paired", "a pivot must be entered through its imaginary half");
        pe::SymbolicOptions o2{};
        pe::Symbolic U;
        require(run("paired_unpaired", M, o2, U) && U.row_src != S.row_src, "paired_unpaired", "matching by pairs must differ from the plain matching");
    }

    Matrix const m100 = mesh(100, 4);
    {
        pe::SymbolicOptions const o = sweep_geometry();
        require(run("mesh100_sweep", m100, o, S), "mesh100_sweep", "must succeed");
        require(S.top_ptr.size() > 1 && !S.top_list.empty(), "mesh100_sweep", "must have top levels");
        require(count(S.f_quad, 1) > 0 && count(S.f_kind, 0) > count(S.f_quad, 1) && count(S.f_kind, 1) > 0, "mesh100_sweep", "must have quad, other wave and cooperative fronts");
        int const all_fronts = S.nfronts;
        size_t const prog = S.q_prog.size();

        // the first three lines of the mesh depend on x
        std::vector<char> rows(static_cast<size_t>(m100.n), 0), slots(m100.ci.size(), 0);
        for(int i = 0; i < m100.n; ++i)
        {
            rows[static_cast<size_t>(i)] = i < 300;
            for(int e = m100.rp[static_cast<size_t>(i)]; e < m100.rp[static_cast<size_t>(i) + 1]; ++e) slots[static_cast<size_t>(e)] = i < 300 || m100.ci[static_cast<size_t>(e)] < 300;
        }
        pe::SymbolicOptions d = o;
        d.dyn_slots = &slots;
        d.dyn_rows = &rows;
        require(run("mesh100_sweep_static", m100, d, S) && S.nfronts == all_fronts, "mesh100_sweep_static", "must succeed with the same fronts");
        require(S.n_static_quad > 0 && S.static_root_doubles > 0 && S.q_prog_dyn.size() < prog && S.q_prog.size() == prog, "mesh100_sweep_static",
                "must have static quad fronts, persistent static roots and a shorter dynamic program");

        // the retired classes: MID fronts and the LDS stack of the lane-group kernel
        pe::SymbolicOptions r = o;
        r.quad_mid = 1;
        r.quad_lds_doubles = 600;
        require(run("mesh100_sweep_mid", m100, r, S) && S.n_mid > 0 && S.q_lds_kept > 0 && count(S.f_kind, 3) == S.n_mid, "mesh100_sweep_mid", "must have MID fronts and update matrices kept in LDS");
    }
    {
        pe::SymbolicOptions o = single_geometry();
        require(run("mesh100_single", m100, o, S), "mesh100_single", "must succeed");
        require(S.top_ptr.size() > 1 && count(S.f_kind, 0) > 0 && count(S.f_kind, 1) > 0, "mesh100_single", "must have top, cooperative and wave fronts");
        int const first_pass = S.nfronts;
        // second pass: the unknowns of the top fronts may form fronts against a CU's whole LDS
        std::vector<char> big(static_cast<size_t>(m100.n), 0);
        for(int s: S.top_list)
            for(int c = S.f_col0[static_cast<size_t>(s)]; c < S.f_col0[static_cast<size_t>(s)] + S.f_p[static_cast<size_t>(s)]; ++c) big[static_cast<size_t>(S.col_src[static_cast<size_t>(c)])] = 1;
        o.big_unknowns = &big;
        o.max_pivots_top = 64;
        o.panel_doubles_top = whole_cu - 2 - std::max<long long>(o.panel_reserve, S.max_m + 8 + 512);
        require(run("mesh100_single_wide_top", m100, o, S) && S.nfronts < first_pass, "mesh100_single_wide_top", "the second pass must give fewer fronts");
        require(*std::max_element(S.f_p.begin(), S.f_p.end()) > 48, "mesh100_single_wide_top", "a top front must take more than max_pivots pivots");
    }
    {
        // a chain of 5 000 nodes with 500 random links: non-planar, fronts beyond what the LDS panels take in one piece
        int const n = 5000;
        std::vector<std::pair<int, int>> e;
        for(int i = 0; i + 1 < n; ++i) e.push_back({i, i + 1});
        Rng g{5};
        for(int k = 0; k < 500; ++k)
        {
            int const a = g.below(n), b = g.below(n);
            e.push_back({a, b});
        }
        Matrix M = from_edges(n, e, 6);
        M.finish();
        require(run("chain5000", M, def, S) && S.max_m > 400, "chain5000", "must have a front of order > 400");
        int links = 0;  // a group cut against the panel budget: a front continued by the next one, fewer pivots than the limit
        for(int s = 0; s + 1 < S.nfronts; ++s)
        {
            size_t const a = static_cast<size_t>(s);
            links += S.f_p[a] + S.f_u[a] > 64 && S.f_p[a] < def.max_pivots && S.f_parent[a] == s + 1 && S.f_col0[a + 1] == S.f_col0[a] + S.f_p[a] && S.f_u[a] == S.f_p[a + 1] + S.f_u[a + 1];
        }
        require(links > 0, "chain5000", "a group must be split against the panel budget");
    }
    {
        pe::SymbolicOptions o{};
        o.wave_m = 8;
        o.panel_doubles = 10;
        require(!run("mesh12_tiny_panels", m12, o, S) && !S.structurally_singular && S.error == "front too large for the LDS panels", "mesh12_tiny_panels", "must fail on the panel budget");
    }
    return 0;
}
