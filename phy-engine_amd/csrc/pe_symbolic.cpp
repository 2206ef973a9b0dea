// pe_symbolic.cpp -- see pe_symbolic.hpp.
//
// Index conventions.  A is the n x n MNA matrix in CSR.  The factorisation works on
//     A''[k][l] = A[ row_src[k] ][ col_src[l] ]
// i.e. permuted equation k is original equation row_src[k] and permuted unknown l is original unknown
// col_src[l].  row_src = rmatch o q and col_src = q, where rmatch is the row matching (equation chosen as
// pivot row for each unknown) and q the fill-reducing symmetric ordering of pattern(A' + A'^T),
// A'[j][:] = A[rmatch[j]][:].
#include "pe_symbolic.hpp"

#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>
#include <numeric>
#include <queue>
#include <utility>

namespace pe
{
    namespace
    {
        using ivec = std::vector<int>;

        // ------------------------------------------------------------------------------------
        // 1. row matching: unknown j <- equation rmatch[j]
        //
        // The numeric factorisation never searches for a pivot, so the matching IS the pivot choice, and a matching that is merely
        // zero-free is not enough: on a circuit with many branch rows (inductors, controlled sources, transformers) a greedy choice
        // strings pivots of 1e-3 beside entries of 1 into chains whose multipliers multiply up -- errors of 1e9 tolerance units on
        // matrices of condition 6e7 that partial pivoting solves to 1e-8.
        //
        // (a) weighted_matching: the matching of maximum PRODUCT of the magnitudes (equivalently minimum sum of cost = log(max|row|) -
        //     log|a|), by shortest augmenting paths on reduced costs (Dijkstra with row / column potentials u, v: the sparse assignment
        //     algorithm of Duff & Koster's MC64).  On return cost - u - v >= 0 for every entry and = 0 for the matched ones: with the
        //     rows scaled by exp(u) / max|row| and the columns by exp(v) every entry of A is <= 1 in magnitude and every matched one is
        //     1.  A factorisation without pivot search is invariant under such a scaling, so the scaling is never applied: it is the
        //     yardstick in which a pivot's size is judged.
        // (b) match_plain: the own diagonal is kept wherever it is >= tau_diag in that scaling -- a symmetric pattern fills less, a
        //     node-voltage matrix keeps the identity, and the diagonal of an MNA matrix is a sound pivot well below the entries beside it:
        //     a conductance of 1e-3 beside susceptances of 1e3 whose own block [[1, -1], [-1, 1]] is singular (two nodes joined by a
        //     capacitor in the real-equivalent AC system) is the pivot that works, the larger entries are the ones that cancel.  The other
        //     equations are matched by augmenting paths over entries >= tau only, largest scaled magnitude first: an off-diagonal pivot has
        //     nothing structural to recommend it, so it has to be large -- threshold pivoting with threshold tau, decided once.  A path
        //     always exists: the matching of (a) is a perfect matching among those entries.
        // ------------------------------------------------------------------------------------
        // red[e]: reduced cost of entry e (-log of its scaled magnitude; +inf for an explicit zero).  False: structurally singular.
        bool weighted_matching(int n, int const* rp, int const* ci, double const* vals, std::vector<double>& red, ivec& rmatch)
        {
            double const inf = std::numeric_limits<double>::infinity();
            int const nnz = rp[n];
            red.assign(nnz, 0.0);
            std::vector<double> u(n, 0.0), v(n, 0.0);
            if(vals)
            {
                for(int i = 0; i < n; ++i)
                {
                    double mx = 0.0;
                    // (an infinite entry is a usable pivot, the largest there is; a NaN is none)
                    double const big = std::numeric_limits<double>::max();
                    for(int e = rp[i]; e < rp[i + 1]; ++e)
                        if(double const w = std::min(std::fabs(vals[e]), big); w > mx) mx = w;
                    for(int e = rp[i]; e < rp[i + 1]; ++e)
                    {
                        double const w = std::min(std::fabs(vals[e]), big);
                        red[e] = w > 0.0 ? std::log(mx) - std::log(w) : inf;
                    }
                }
                // starting potentials: v = column minimum, u = row minimum of what is left
                v.assign(n, inf);
                for(int e = 0; e < nnz; ++e) v[ci[e]] = std::min(v[ci[e]], red[e]);
                for(int j = 0; j < n; ++j)
                    if(v[j] == inf) return false;
                for(int i = 0; i < n; ++i)
                {
                    u[i] = inf;
                    for(int e = rp[i]; e < rp[i + 1]; ++e)
                        if(red[e] < inf) u[i] = std::min(u[i], red[e] - v[ci[e]]);
                    if(u[i] == inf) return false;
                }
            }
            rmatch.assign(n, -1);
            ivec colof(n, -1);
            // tight entries first (the diagonal before the others)
            for(int pass = 0; pass < 2; ++pass)
                for(int i = 0; i < n; ++i)
                    for(int e = rp[i]; e < rp[i + 1] && colof[i] < 0; ++e)
                    {
                        int const c = ci[e];
                        if((pass == 0 && c != i) || rmatch[c] >= 0 || !(red[e] - u[i] - v[c] <= 0.0)) continue;
                        rmatch[c] = i;
                        colof[i] = c;
                    }
            // shortest augmenting path from every equation still free
            std::vector<double> d(n, inf), lrow(n, 0.0);
            ivec pred(n, -1), seen(n, -1), done(n, -1), tree_rows, done_cols;
            using item = std::pair<double, int>;
            std::priority_queue<item, std::vector<item>, std::greater<item>> heap;
            for(int r0 = 0; r0 < n; ++r0)
            {
                if(colof[r0] >= 0) continue;
                heap = {};
                tree_rows.assign(1, r0);
                done_cols.clear();
                lrow[r0] = 0.0;
                int i = r0, jend = -1;
                double lsp = 0.0;
                for(;;)
                {
                    for(int e = rp[i]; e < rp[i + 1]; ++e)
                    {
                        int const c = ci[e];
                        if(red[e] == inf || done[c] == r0) continue;
                        double const nd = lrow[i] + std::max(0.0, red[e] - u[i] - v[c]);
                        if(seen[c] != r0 || nd < d[c])
                        {
                            seen[c] = r0;
                            d[c] = nd;
                            pred[c] = i;
                            heap.push({nd, c});
                        }
                    }
                    int c = -1;
                    while(!heap.empty())
                    {
                        auto const [dd, cc] = heap.top();
                        heap.pop();
                        if(done[cc] == r0 || dd > d[cc]) continue;
                        c = cc;
                        break;
                    }
                    if(c < 0) return false;  // no zero-free diagonal exists
                    done[c] = r0;
                    if(rmatch[c] < 0)
                    {
                        jend = c;
                        lsp = d[c];
                        break;
                    }
                    done_cols.push_back(c);
                    i = rmatch[c];
                    lrow[i] = d[c];
                    tree_rows.push_back(i);
                }
                for(int c: done_cols) v[c] += d[c] - lsp;
                for(int r: tree_rows) u[r] += lsp - lrow[r];
                for(int c = jend;;)
                {
                    int const r = pred[c], prev = colof[r];
                    rmatch[c] = r;
                    colof[r] = c;
                    if(r == r0) break;
                    c = prev;
                }
            }
            for(int i = 0; i < n; ++i)
                for(int e = rp[i]; e < rp[i + 1]; ++e)
                    if(red[e] < inf) red[e] = std::max(0.0, red[e] - u[i] - v[ci[e]]);
            return true;
        }

        // Keep the diagonal of the equations with diag_ok, then augmenting paths by depth-first search for the others: the candidates of an
        // equation are its entries with key < inf, smallest key first (ties: lowest column).  False: no perfect matching among them.
        bool dfs_matching(int n, int const* rp, int const* ci, std::vector<double> const& key, std::vector<char> const& diag_ok, ivec& rmatch)
        {
            double const inf = std::numeric_limits<double>::infinity();
            rmatch.assign(n, -1);
            ivec colof(n, -1);  // equation i -> unknown it pivots
            for(int i = 0; i < n; ++i)
                if(diag_ok[i])
                {
                    rmatch[i] = i;
                    colof[i] = i;
                }
            std::vector<ivec> cand(n);
            auto build_cand = [&](int i)
            {
                if(!cand[i].empty()) return;
                std::vector<std::pair<double, int>> t;
                for(int e = rp[i]; e < rp[i + 1]; ++e)
                    if(key[e] < inf) t.push_back({key[e], ci[e]});
                std::sort(t.begin(), t.end());
                for(auto const& [w, c]: t) cand[i].push_back(c);
            };
            ivec visited(n, -1), it(n, 0), stack_row, stack_col;
            for(int r0 = 0; r0 < n; ++r0)
            {
                if(colof[r0] >= 0) continue;
                // iterative DFS over alternating paths: equation -> candidate unknown -> equation currently holding it
                stack_row.assign(1, r0);
                stack_col.clear();
                build_cand(r0);
                it[r0] = 0;
                bool found = false;
                while(!stack_row.empty())
                {
                    int const i = stack_row.back();
                    if(it[i] >= static_cast<int>(cand[i].size()))
                    {
                        stack_row.pop_back();
                        if(!stack_col.empty()) stack_col.pop_back();
                        continue;
                    }
                    int const c = cand[i][it[i]++];
                    if(visited[c] == r0) continue;
                    visited[c] = r0;
                    stack_col.push_back(c);
                    if(rmatch[c] < 0)
                    {
                        found = true;
                        break;
                    }
                    int const nxt = rmatch[c];
                    build_cand(nxt);
                    it[nxt] = 0;
                    stack_row.push_back(nxt);
                }
                if(!found) return false;
                // flip along the path: stack_row[t] takes stack_col[t]
                for(size_t t = 0; t < stack_row.size(); ++t)
                {
                    rmatch[stack_col[t]] = stack_row[t];
                    colof[stack_row[t]] = stack_col[t];
                }
            }
            return true;
        }

        // The greedy matching: the diagonal wherever it is >= diag_rel of its row, every non-zero entry a candidate of the others, heaviest
        // first.  Cheap, and on node-voltage matrices the choice the goldens were recorded with -- but it looks at no pivot's size beyond the
        // order of the search: match_plain judges the result.
        bool greedy_matching(int n, int const* rp, int const* ci, double const* vals, double diag_rel, ivec& rmatch)
        {
            std::vector<double> key(rp[n]);
            std::vector<char> diag_ok(n, 0);
            for(int i = 0; i < n; ++i)
            {
                double rowmax = 0.0;
                for(int e = rp[i]; e < rp[i + 1]; ++e) rowmax = std::max(rowmax, vals ? std::fabs(vals[e]) : 1.0);
                for(int e = rp[i]; e < rp[i + 1]; ++e)
                {
                    double const w = vals ? std::fabs(vals[e]) : 1.0;
                    key[e] = w > 0.0 ? -w : std::numeric_limits<double>::infinity();
                    if(ci[e] == i && w > 0.0 && w >= diag_rel * rowmax) diag_ok[i] = 1;
                }
            }
            return dfs_matching(n, rp, ci, key, diag_ok, rmatch);
        }

        bool match_plain(int n, int const* rp, int const* ci, double const* vals, double tau, double tau_diag, bool greedy_only, ivec& rmatch)
        {
            if(greedy_only) return greedy_matching(n, rp, ci, vals, tau_diag, rmatch);
            std::vector<double> red;
            ivec best;
            if(!weighted_matching(n, rp, ci, vals, red, best)) return false;
            // an entry qualifies as a pivot when its scaled magnitude is >= tau (the slack: the matched entries of (a) are 1 up to rounding)
            double const limit = -std::log(std::min(1.0, std::max(tau, 1e-300))) + 1e-9;
            double const limit_diag = std::max(limit, -std::log(std::min(1.0, std::max(tau_diag, 1e-300))));
            // the greedy matching first: taken when it meets the same two thresholds
            if(greedy_matching(n, rp, ci, vals, tau_diag, rmatch))
            {
                bool ok = true;
                for(int i = 0; i < n && ok; ++i)
                    for(int e = rp[i]; e < rp[i + 1]; ++e)
                        if(rmatch[ci[e]] == i) ok = ok && red[e] <= (ci[e] == i ? limit_diag : limit);
                if(ok) return true;
            }
            std::vector<double> key(rp[n]);
            std::vector<char> diag_ok(n, 0);
            for(int i = 0; i < n; ++i)
                for(int e = rp[i]; e < rp[i + 1]; ++e)
                {
                    key[e] = red[e] <= limit ? red[e] : std::numeric_limits<double>::infinity();
                    if(ci[e] == i && red[e] <= limit_diag) diag_ok[i] = 1;
                }
            // (a failure is unreachable but for rounding at the limit: the matching of (a) lies among the qualifying entries)
            if(!dfs_matching(n, rp, ci, key, diag_ok, rmatch)) rmatch = best;
            return true;
        }

        // (c) The real-equivalent form [[Ar, -Ai], [Ai, Ar]] of a complex system of order h = n / 2, rows laid out as pe_engine_seam.cpp
        //     real_equivalent_pattern lays them out (row i = [columns of complex row i | the same + h], row h + i likewise).  Rows i and
        //     h + i carry the two halves of the same complex entries, equal in magnitude, and a matching on magnitudes is free to take the
        //     halves of a complex pivot from two different entries: on AC stamps of circuits it then ends on blocks that cancel exactly
        //     (a zero pivot).  So the COMPLEX matrix is matched, on the moduli |a + j b| of its entries, by (a) and (b) above, and a matched
        //     entry (i, j) becomes the pivot block of rows i, h + i and columns j, h + j, entered through its larger half: a on the
        //     diagonal of the block when |a| >= |b|, otherwise b (equation i takes unknown h + j and equation h + i unknown j).
        //     False when the pattern is not of that layout.
        bool paired_layout(int n, int const* rp, int const* ci)
        {
            int const h = n / 2;
            if(n % 2) return false;
            for(int i = 0; i < h; ++i)
            {
                int const len = rp[i + 1] - rp[i], half = len / 2;
                if(len % 2 || rp[h + i + 1] - rp[h + i] != len) return false;
                for(int k = 0; k < half; ++k)
                {
                    int const c = ci[rp[i] + k];
                    if(c >= h || ci[rp[i] + half + k] != c + h || ci[rp[h + i] + k] != c || ci[rp[h + i] + half + k] != c + h) return false;
                }
            }
            return true;
        }
        bool match_paired(int n, int const* rp, int const* ci, double const* vals, double tau, double tau_diag, bool greedy_only, ivec& rmatch)
        {
            int const h = n / 2;
            ivec rp1(h + 1, 0), ci1, rm1;
            std::vector<double> mod;
            for(int i = 0; i < h; ++i)
            {
                int const half = (rp[i + 1] - rp[i]) / 2;
                for(int k = 0; k < half; ++k)
                {
                    ci1.push_back(ci[rp[i] + k]);
                    mod.push_back(std::hypot(vals[rp[i] + k], vals[rp[i] + half + k]));
                }
                rp1[i + 1] = static_cast<int>(ci1.size());
            }
            if(!match_plain(h, rp1.data(), ci1.data(), mod.data(), tau, tau_diag, greedy_only, rm1)) return false;
            rmatch.assign(n, -1);
            for(int i = 0; i < h; ++i)
            {
                int const half = (rp[i + 1] - rp[i]) / 2;
                for(int k = 0; k < half; ++k)
                {
                    int const j = ci[rp[i] + k];
                    if(rm1[j] != i) continue;
                    bool const real_half = std::fabs(vals[rp[i] + k]) >= std::fabs(vals[rp[i] + half + k]);
                    rmatch[j] = real_half ? i : h + i;
                    rmatch[h + j] = real_half ? h + i : i;
                }
            }
            return true;
        }

        bool match_rows(int n, int const* rp, int const* ci, double const* vals, SymbolicOptions const& opt, ivec& rmatch, int& swaps)
        {
            bool const paired = opt.match_pairs && vals && paired_layout(n, rp, ci);
            if(!(paired ? match_paired : match_plain)(n, rp, ci, vals, opt.match_tau, opt.match_diag_tau, opt.match_greedy, rmatch)) return false;
            swaps = 0;
            for(int j = 0; j < n; ++j) swaps += rmatch[j] != j;
            return true;
        }

        // ------------------------------------------------------------------------------------
        // 2. adjacency of pattern(A' + A'^T), no diagonal
        // ------------------------------------------------------------------------------------
        void sym_graph(int n, int const* rp, int const* ci, ivec const& rmatch, ivec& gp, ivec& gi)
        {
            std::vector<ivec> adj(n);
            for(int j = 0; j < n; ++j)
            {
                int const r = rmatch[j];
                for(int e = rp[r]; e < rp[r + 1]; ++e)
                {
                    int const c = ci[e];
                    if(c == j) continue;
                    adj[j].push_back(c);
                    adj[c].push_back(j);
                }
            }
            gp.assign(n + 1, 0);
            for(int v = 0; v < n; ++v)
            {
                std::sort(adj[v].begin(), adj[v].end());
                adj[v].erase(std::unique(adj[v].begin(), adj[v].end()), adj[v].end());
                gp[v + 1] = gp[v] + static_cast<int>(adj[v].size());
            }
            gi.resize(gp[n]);
            for(int v = 0; v < n; ++v) std::copy(adj[v].begin(), adj[v].end(), gi.begin() + gp[v]);
        }

        // ------------------------------------------------------------------------------------
        // 3. nested dissection by BFS level sets, minimum degree on the leaves
        // ------------------------------------------------------------------------------------
        struct Dissector
        {
            int n;
            ivec const& gp;
            ivec const& gi;
            int leaf;
            ivec tag, level, order;
            int next_tag{1};

            Dissector(int n_, ivec const& gp_, ivec const& gi_, int leaf_) : n(n_), gp(gp_), gi(gi_), leaf(leaf_), tag(n_, 0), level(n_, 0) { order.reserve(n_); }

            // exact minimum degree on the induced subgraph of V (|V| small)
            void md_leaf(ivec const& V)
            {
                int const k = static_cast<int>(V.size());
                if(k == 0) return;
                int const t = next_tag++;
                ivec local(k);
                for(int a = 0; a < k; ++a)
                {
                    tag[V[a]] = t;
                    level[V[a]] = a;  // reuse as local id
                }
                std::vector<std::vector<char>> adj(k, std::vector<char>(k, 0));
                for(int a = 0; a < k; ++a)
                    for(int e = gp[V[a]]; e < gp[V[a] + 1]; ++e)
                        if(tag[gi[e]] == t) adj[a][level[gi[e]]] = 1;
                std::vector<char> gone(k, 0);
                for(int step = 0; step < k; ++step)
                {
                    int best = -1, bestd = 1 << 30;
                    for(int a = 0; a < k; ++a)
                    {
                        if(gone[a]) continue;
                        int d = 0;
                        for(int b = 0; b < k; ++b) d += (!gone[b] && adj[a][b]);
                        if(d < bestd)
                        {
                            bestd = d;
                            best = a;
                        }
                    }
                    gone[best] = 1;
                    order.push_back(V[best]);
                    for(int a = 0; a < k; ++a)
                    {
                        if(gone[a] || !adj[best][a]) continue;
                        for(int b = 0; b < k; ++b)
                            if(!gone[b] && b != a && adj[best][b]) adj[a][b] = 1;
                    }
                }
            }

            // BFS inside the tagged set from `start`; fills `out` (visit order) and level[]; returns eccentricity
            int bfs(int start, int t, int mark, ivec& out, ivec& seen)
            {
                out.clear();
                out.push_back(start);
                seen[start] = mark;
                level[start] = 0;
                size_t head = 0;
                int ecc = 0;
                while(head < out.size())
                {
                    int const v = out[head++];
                    for(int e = gp[v]; e < gp[v + 1]; ++e)
                    {
                        int const w = gi[e];
                        if(tag[w] != t || seen[w] == mark) continue;
                        seen[w] = mark;
                        level[w] = level[v] + 1;
                        ecc = level[w];
                        out.push_back(w);
                    }
                }
                return ecc;
            }

            ivec seen;
            int next_mark{1};

            void run(ivec V)
            {
                if(seen.empty()) seen.assign(n, 0);
                if(static_cast<int>(V.size()) <= leaf)
                {
                    md_leaf(V);
                    return;
                }
                int const t = next_tag++;
                for(int v: V) tag[v] = t;
                ivec reach;
                int ecc = bfs(V[0], t, next_mark++, reach, seen);
                if(reach.size() < V.size())
                {
                    // disconnected: dissect the components independently
                    int const mk = next_mark - 1;
                    ivec rest;
                    for(int v: V)
                        if(seen[v] != mk) rest.push_back(v);
                    ivec comp = reach;
                    run(std::move(comp));
                    run(std::move(rest));
                    return;
                }
                // pseudo-peripheral start: restart from a minimum-degree vertex of the last level while the depth grows
                for(int rounds = 0; rounds < 6; ++rounds)
                {
                    int far = reach.back(), fard = 1 << 30;
                    for(size_t a = reach.size(); a-- > 0 && level[reach[a]] == ecc;)
                    {
                        int const d = gp[reach[a] + 1] - gp[reach[a]];
                        if(d < fard)
                        {
                            fard = d;
                            far = reach[a];
                        }
                    }
                    ivec r2;
                    int const e2 = bfs(far, t, next_mark++, r2, seen);
                    if(e2 > ecc)
                    {
                        ecc = e2;
                        reach.swap(r2);
                    }
                    else
                    {
                        // keep the deeper (current `reach`) structure: recompute its levels (bfs overwrote level[])
                        int const s0 = reach[0];
                        ecc = bfs(s0, t, next_mark++, reach, seen);
                        break;
                    }
                }
                if(ecc < 2)
                {
                    md_leaf(V);
                    return;
                }
                // level sizes -> most balanced interior level
                ivec cnt(ecc + 1, 0);
                for(int v: reach) ++cnt[level[v]];
                long long below = cnt[0];
                long long const total = static_cast<long long>(reach.size());
                int best_m = 1;
                double best_cost = 1e300;
                for(int m = 1; m < ecc; ++m)
                {
                    long long const above = total - below - cnt[m];
                    double const cost = static_cast<double>(std::max(below, above)) + 0.5 * cnt[m];
                    if(cost < best_cost)
                    {
                        best_cost = cost;
                        best_m = m;
                    }
                    below += cnt[m];
                }
                ivec A, B, S;
                for(int v: reach)
                {
                    if(level[v] < best_m) A.push_back(v);
                    else if(level[v] > best_m) B.push_back(v);
                    else
                    {
                        bool touches = false;
                        for(int e = gp[v]; e < gp[v + 1] && !touches; ++e)
                            touches = tag[gi[e]] == t && level[gi[e]] == best_m + 1;
                        (touches ? S : A).push_back(v);
                    }
                }
                run(std::move(A));
                run(std::move(B));
                for(int v: S) order.push_back(v);
            }
        };

        // ------------------------------------------------------------------------------------
        // 4. elimination tree / postorder / column structures
        // ------------------------------------------------------------------------------------
        void etree_of(int n, std::vector<ivec> const& lower /* lower[i] = {k < i : B[i][k] != 0} */, ivec& parent)
        {
            parent.assign(n, -1);
            ivec anc(n, -1);
            for(int i = 0; i < n; ++i)
            {
                for(int k0: lower[i])
                {
                    int k = k0;
                    while(k != -1 && k < i)
                    {
                        int const nxt = anc[k];
                        anc[k] = i;
                        if(nxt == -1)
                        {
                            parent[k] = i;
                            break;
                        }
                        k = nxt;
                    }
                }
            }
        }

        void col_structs(int n, std::vector<ivec> const& upper /* upper[j] = {i > j : B[i][j] != 0} sorted */, ivec const& parent, std::vector<ivec>& st)
        {
            st.assign(n, {});
            std::vector<ivec> kids(n);
            for(int j = 0; j < n; ++j)
                if(parent[j] >= 0) kids[parent[j]].push_back(j);
            ivec mark(n, -1);
            for(int j = 0; j < n; ++j)
            {
                ivec& s = st[j];
                for(int i: upper[j])
                    if(mark[i] != j)
                    {
                        mark[i] = j;
                        s.push_back(i);
                    }
                for(int c: kids[j])
                    for(int i: st[c])
                        if(i != j && mark[i] != j)
                        {
                            mark[i] = j;
                            s.push_back(i);
                        }
                std::sort(s.begin(), s.end());
            }
        }

        // postorder of a forest (children before parents): the roots in the given order, the children of a node in the order of kids[]
        ivec postorder(std::vector<ivec> const& kids, ivec const& roots)
        {
            ivec post, stack, next(kids.size(), 0);
            post.reserve(kids.size());
            for(int r: roots)
            {
                stack.push_back(r);
                while(!stack.empty())
                {
                    int const v = stack.back();
                    if(next[v] < static_cast<int>(kids[v].size())) stack.push_back(kids[v][next[v]++]);
                    else
                    {
                        post.push_back(v);
                        stack.pop_back();
                    }
                }
            }
            return post;
        }

        // ====================================================================================
        // The phases of analyze(), in the order they run (numbered as in pe_symbolic.hpp).  A phase takes what it reads by const reference
        // and returns what it makes; the tables of the plan go straight into the Symbolic.  One that can fail leaves its message in
        // `error`, or in S.error where it fills the Symbolic.
        // ====================================================================================

        // cost model of a front, for the cuts and balances of the schedule: fixed work + the dense elimination
        double front_cost(int p, int u)
        {
            double const m = p + u;
            return 400.0 + m * m * (2.0 + p);
        }
        // arena doubles of a front's slot: the u x u update matrix followed by the u-vector of the forward substitution
        long long slot_doubles(int u) { return static_cast<long long>(u) * (u + 1); }

        // ---------------- phase 1: row matching, graph, nested dissection.  (The seam of the ordering: another fill-reducing ordering, or a
        // choice between several, changes this function only.)
        struct Ordering
        {
            ivec rmatch;  // unknown j <- equation rmatch[j]
            ivec gp, gi;  // adjacency of pattern(A' + A'^T)
            ivec q;       // fill-reducing symmetric ordering: position k holds unknown q[k]
            int swaps{};
            bool singular{};
        };
        Ordering fill_reducing_order(int n, int const* rp, int const* ci, double const* vals, SymbolicOptions const& opt, std::string& error)
        {
            Ordering o;
            if(!match_rows(n, rp, ci, vals, opt, o.rmatch, o.swaps))
            {
                o.singular = true;
                error = "structurally singular matrix (no zero-free diagonal exists)";
                return o;
            }
            sym_graph(n, rp, ci, o.rmatch, o.gp, o.gi);
            Dissector D(n, o.gp, o.gi, std::max(2, opt.nd_leaf));
            ivec all(n);
            std::iota(all.begin(), all.end(), 0);
            D.run(std::move(all));
            o.q = std::move(D.order);
            if(static_cast<int>(o.q.size()) != n) error = "internal: ordering lost vertices";
            return o;
        }

        // ---------------- phase 2: elimination tree + column structures of an ordering.  `repostorder`: q is then replaced by a postorder
        // of its tree, children sorted by structure size ascending (largest last => mergeable with the parent), and the tree is that of the new q
        struct Tree
        {
            ivec parent;           // elimination tree, -1 for roots
            std::vector<ivec> st;  // per column: its rows below the diagonal, ascending
        };
        Tree column_tree(ivec const& gp, ivec const& gi, ivec& q, bool repostorder)
        {
            int const n = static_cast<int>(q.size());
            Tree t;
            for(int pass = 0; pass < 2; ++pass)
            {
                ivec qinv(n);
                for(int k = 0; k < n; ++k) qinv[q[k]] = k;
                std::vector<ivec> lower(n), upper(n);
                for(int k = 0; k < n; ++k)
                {
                    int const v = q[k];
                    for(int e = gp[v]; e < gp[v + 1]; ++e)
                    {
                        int const l = qinv[gi[e]];
                        if(l < k) lower[k].push_back(l);
                        else upper[k].push_back(l);
                    }
                    std::sort(upper[k].begin(), upper[k].end());
                }
                etree_of(n, lower, t.parent);
                col_structs(n, upper, t.parent, t.st);
                if(pass == 1 || !repostorder) break;
                std::vector<ivec> kids(n);
                ivec roots;
                for(int j = 0; j < n; ++j) (t.parent[j] >= 0 ? kids[t.parent[j]] : roots).push_back(j);
                auto by_size = [&t](int a, int b) { return t.st[a].size() != t.st[b].size() ? t.st[a].size() < t.st[b].size() : a < b; };
                for(auto& kv: kids) std::sort(kv.begin(), kv.end(), by_size);
                ivec const post = postorder(kids, roots);
                ivec q2(n);
                for(int k = 0; k < n; ++k) q2[k] = q[post[k]];
                q.swap(q2);
            }
            return t;
        }

        // The top class of a run of columns (second pass: SymbolicOptions::big_unknowns; q maps a column to its unknown): a run made of
        // marked unknowns only forms fronts that own a CU's LDS -- more pivots, a larger panel budget, never a wave front
        struct TopClass
        {
            SymbolicOptions const& opt;
            ivec const& q;
            bool has_big;
            TopClass(SymbolicOptions const& opt_, ivec const& q_)
                : opt(opt_), q(q_), has_big(opt_.big_unknowns && opt_.big_unknowns->size() == q_.size() && opt_.panel_doubles_top > 0)
            {
            }
            int of(int c0, int c1) const  // 0: ordinary, 1: a CU's whole LDS, 2: half of it (the smallest share among its unknowns)
            {
                if(!has_big) return 0;
                int cls = 1;
                for(int c = c0; c < c1; ++c)
                {
                    int const k = (*opt.big_unknowns)[q[c]];
                    if(k == 0) return 0;
                    cls = std::max(cls, k);
                }
                return cls;
            }
            bool big(int c0, int c1) const { return of(c0, c1) != 0; }
            int pivots_max(int cls) const { return cls != 0 ? std::max(opt.max_pivots, opt.max_pivots_top) : opt.max_pivots; }
            long long panel_budget(int cls) const { return std::max(opt.panel_doubles, cls == 1 ? opt.panel_doubles_top : (cls == 2 ? opt.panel_doubles_mid : 0)); }
        };

        // ---------------- phase 3: supernodes: fundamental runs, then relaxed merging of last children
        struct SN
        {
            int c0, c1;       // columns [c0, c1)
            long long zeros;  // explicit zeros in the L panel (same count in U)
        };
        // P swallows the supernodes at the end of sn while they are its last children and the explicit zeros stay within the relaxation
        void merge_last_children(std::vector<SN>& sn, SN& P, Tree const& t, TopClass const& top, SymbolicOptions const& opt)
        {
            auto u_of = [&t](SN const& s) { return static_cast<int>(t.st[s.c1 - 1].size()); };
            while(!sn.empty())
            {
                SN const& C = sn.back();
                if(C.c1 != P.c0) break;
                int const pc = t.parent[C.c1 - 1];
                if(pc < P.c0 || pc >= P.c1) break;  // not a child of P
                int const pC = C.c1 - C.c0, uC = u_of(C);
                int const pP = P.c1 - P.c0, mP = pP + u_of(P);
                int const np = pC + pP;
                if(np > top.pivots_max(top.of(C.c0, P.c1))) break;
                long long const z = C.zeros + P.zeros + static_cast<long long>(pC) * (mP - uC);
                double const panel = static_cast<double>(np) * (np + u_of(P)) - 0.5 * np * (np - 1);
                if(np > opt.relax_small && static_cast<double>(z) > opt.relax_zero_frac * panel) break;
                P.c0 = C.c0;
                P.zeros = z;
                sn.pop_back();
            }
        }
        std::vector<SN> supernodes(Tree const& t, ivec const& q, SymbolicOptions const& opt)
        {
            int const n = static_cast<int>(q.size());
            TopClass const top(opt, q);
            std::vector<SN> sn;
            for(int j = 0; j < n;)
            {
                SN P{j, j + 1, 0};
                // (second pass: a fundamental run of the top stays ONE group, cut into equal links by split_into_fronts)
                while(P.c1 < n && t.parent[P.c1 - 1] == P.c1 && t.st[P.c1 - 1].size() == t.st[P.c1].size() + 1 && (top.big(P.c0, P.c1 + 1) || (P.c1 - P.c0) < opt.max_pivots)) ++P.c1;
                j = P.c1;
                merge_last_children(sn, P, t, top, opt);
                sn.push_back(P);
            }
            return sn;
        }

        // ---------------- phase 4: generalised absorption: a parent swallows ANY of its children while the merged front stays
        // small enough for one wavefront (m <= absorb_m).  The absorbed columns are treated as dense (explicit zeros),
        // which removes the tiny fronts whose cost on a GPU is pure latency.  Needs a re-permutation of q so that the
        // merged columns are contiguous; fill is unchanged (same elimination tree order within every subtree).
        // Returns the forced partition [c0, c1) of the columns in the NEW order.
        using Groups = std::vector<std::pair<int, int>>;
        Groups absorb_children(Tree const& t, std::vector<SN> const& sn, ivec& q, SymbolicOptions const& opt, std::string& error)
        {
            int const n = static_cast<int>(q.size()), ns = static_cast<int>(sn.size());
            ivec col2sn(n);
            for(int i = 0; i < ns; ++i)
                for(int c = sn[i].c0; c < sn[i].c1; ++c) col2sn[c] = i;
            ivec par(ns, -1), gp_(ns), gu(ns);
            std::vector<ivec> kids(ns), members(ns);
            for(int i = 0; i < ns; ++i)
            {
                auto const& r = t.st[sn[i].c1 - 1];
                if(!r.empty()) par[i] = col2sn[r[0]];
                gp_[i] = sn[i].c1 - sn[i].c0;
                gu[i] = static_cast<int>(r.size());
                members[i] = {i};
            }
            for(int i = 0; i < ns; ++i)
                if(par[i] >= 0) kids[par[i]].push_back(i);
            std::vector<char> absorbed(ns, 0);
            for(int P = 0; P < ns; ++P)
            {
                bool again = true;
                while(again)
                {
                    again = false;
                    ivec cand = kids[P];
                    std::sort(cand.begin(), cand.end(), [&gp_](int a, int b) { return gp_[a] != gp_[b] ? gp_[a] < gp_[b] : a < b; });
                    for(int C: cand)
                    {
                        if(gp_[P] + gp_[C] + gu[P] > opt.absorb_m || gp_[P] + gp_[C] > opt.wave_p) continue;
                        absorbed[C] = 1;
                        gp_[P] += gp_[C];
                        members[P].insert(members[P].end(), members[C].begin(), members[C].end());
                        auto& kp = kids[P];
                        kp.erase(std::find(kp.begin(), kp.end(), C));
                        for(int g: kids[C])
                        {
                            kp.push_back(g);
                            par[g] = P;
                        }
                        kids[C].clear();
                        again = true;  // grandchildren may now fit as well
                        break;
                    }
                }
            }
            // new column order: postorder of the merged tree, children ascending; a node emits its member supernodes in ascending order
            ivec roots;
            for(int r = 0; r < ns; ++r)
                if(par[r] < 0 && !absorbed[r]) roots.push_back(r);
            for(auto& k: kids) std::sort(k.begin(), k.end());
            Groups groups;
            ivec q2;
            q2.reserve(n);
            for(int v: postorder(kids, roots))
            {
                std::sort(members[v].begin(), members[v].end());
                int const c0 = static_cast<int>(q2.size());
                for(int mbr: members[v])
                    for(int c = sn[mbr].c0; c < sn[mbr].c1; ++c) q2.push_back(q[c]);
                groups.push_back({c0, static_cast<int>(q2.size())});
            }
            if(static_cast<int>(q2.size()) != n) error = "internal: absorption lost columns";
            else
                q.swap(q2);
            return groups;
        }

        // ---------------- phase 5: fronts = forced groups, split to respect the wave / LDS-panel limits
        struct FR
        {
            int c0, c1, g1;  // pivots [c0, c1); the group ends at g1 (rows = [c1, g1) + structure of column g1-1)
        };
        std::vector<FR> split_into_fronts(Tree const& t, Groups const& groups, ivec const& q, SymbolicOptions const& opt, std::string& error)
        {
            TopClass const top(opt, q);
            std::vector<FR> fr;
            for(auto const& [c0, c1]: groups)
            {
                int const ug = static_cast<int>(t.st[c1 - 1].size());
                int const cls = top.of(c0, c1);  // (second pass: a front of the top that owns a CU's LDS, or half of it)
                bool const big = cls != 0;
                for(int a = c0; a < c1;)
                {
                    int const rest = c1 - a;
                    int const mfull = rest + ug;
                    int b;
                    if(mfull <= opt.wave_m && !big) b = a + std::min(rest, opt.wave_p);  // (a front of the top is never a wave front)
                    else if(opt.quad_mid && mfull <= 64)
                        b = a + std::min(rest, 16);  // a candidate MID front of the lane-group kernels: <= 16 pivots (one row set)
                    else
                    {
                        long long const budget = top.panel_budget(cls);
                        int pbest = 0;
                        for(int pp = std::min(rest, top.pivots_max(cls)); pp >= 1; --pp)
                        {
                            long long const uch = (rest - pp) + ug, mch = pp + uch;
                            if(static_cast<long long>(pe_ld(static_cast<int>(mch))) * pp + static_cast<long long>(pe_ld(pp)) * uch <= budget)
                            {
                                pbest = pp;
                                break;
                            }
                        }
                        if(pbest == 0)
                        {
                            error = "front too large for the LDS panels";
                            return fr;
                        }
                        // (links of equal length instead of full ones + a remnant of two or three pivots: the panel need grows with the
                        //  pivots of a link, so the shorter link fits where the longest did)
                        if(big) pbest = (rest + (rest + pbest - 1) / pbest - 1) / ((rest + pbest - 1) / pbest);
                        b = a + pbest;
                    }
                    fr.push_back({a, b, c1});
                    a = b;
                }
            }
            return fr;
        }

        // local index of permuted row / column t in front s (pivots first, then the update rows), -1 if it is not there
        int local_of(Symbolic const& S, int s, int t)
        {
            int const c0 = S.f_col0[s], p = S.f_p[s];
            if(t < c0 + p) return t - c0;
            auto b = S.f_rows.begin() + S.f_rows_ptr[s], e = S.f_rows.begin() + S.f_rows_ptr[s + 1];
            auto it = std::lower_bound(b, e, t);
            if(it == e || *it != t) return -1;
            return p + static_cast<int>(it - b);
        }

        // ---------------- phase 6: the front tables: pivots, update rows, parents, children, relative maps, depth, statistics
        struct FrontMaps
        {
            ivec col2front;  // permuted column -> the front it is a pivot of
            ivec depth;      // of a front in the assembly tree, roots 1
        };
        FrontMaps fill_front_tables(Symbolic& S, Tree const& t, std::vector<FR> const& fr)
        {
            int const nf = static_cast<int>(fr.size());
            FrontMaps fm{ivec(t.st.size()), ivec(nf, 1)};
            S.nfronts = nf;
            S.f_col0.resize(nf);
            S.f_p.resize(nf);
            S.f_u.resize(nf);
            S.f_parent.assign(nf, -1);
            S.f_rows_ptr.assign(nf + 1, 0);
            for(int s = 0; s < nf; ++s)
            {
                S.f_col0[s] = fr[s].c0;
                S.f_p[s] = fr[s].c1 - fr[s].c0;
                S.f_u[s] = (fr[s].g1 - fr[s].c1) + static_cast<int>(t.st[fr[s].g1 - 1].size());
                S.f_rows_ptr[s + 1] = S.f_rows_ptr[s] + S.f_u[s];
                for(int c = fr[s].c0; c < fr[s].c1; ++c) fm.col2front[c] = s;
                S.nnz_LU_stored += 2LL * S.f_p[s] * S.f_u[s] + static_cast<long long>(S.f_p[s]) * S.f_p[s];
            }
            S.f_rows.resize(S.f_rows_ptr[nf]);
            for(int s = 0; s < nf; ++s)
            {
                int* dst = S.f_rows.data() + S.f_rows_ptr[s];
                for(int c = fr[s].c1; c < fr[s].g1; ++c) *dst++ = c;
                auto const& r = t.st[fr[s].g1 - 1];
                std::copy(r.begin(), r.end(), dst);
                if(S.f_u[s] > 0) S.f_parent[s] = fm.col2front[S.f_rows[S.f_rows_ptr[s]]];
                int const m = S.f_p[s] + S.f_u[s];
                S.max_m = std::max(S.max_m, m);
                S.max_u = std::max(S.max_u, S.f_u[s]);
                for(int k = 0; k < S.f_p[s]; ++k)
                {
                    double const r1 = m - k - 1;
                    S.flops += 2.0 * r1 * r1 + r1;
                }
            }
            if(S.max_m >= 65536)
            {
                S.error = "front order exceeds 65535";
                return fm;
            }
            // children, relative indices, depth
            S.f_child_ptr.assign(nf + 1, 0);
            for(int s = 0; s < nf; ++s)
                if(S.f_parent[s] >= 0) ++S.f_child_ptr[S.f_parent[s] + 1];
            for(int s = 0; s < nf; ++s) S.f_child_ptr[s + 1] += S.f_child_ptr[s];
            S.f_child.resize(S.f_child_ptr[nf]);
            ivec fill(S.f_child_ptr.begin(), S.f_child_ptr.end() - 1);
            for(int s = 0; s < nf; ++s)
                if(S.f_parent[s] >= 0) S.f_child[fill[S.f_parent[s]]++] = s;
            S.f_rel_ptr = S.f_rows_ptr;
            S.f_rel.assign(S.f_rows.size(), -1);
            for(int s = nf - 1; s >= 0; --s)
            {
                int const P = S.f_parent[s];
                if(P >= 0)
                {
                    fm.depth[s] = fm.depth[P] + 1;
                    if(P <= s)
                    {
                        S.error = "internal: front tree is not in postorder";
                        return fm;
                    }
                    for(int a = S.f_rows_ptr[s]; a < S.f_rows_ptr[s + 1]; ++a)
                    {
                        int const l = local_of(S, P, S.f_rows[a]);
                        if(l < 0)
                        {
                            S.error = "internal: child update row missing from parent front";
                            return fm;
                        }
                        S.f_rel[a] = l;
                    }
                }
                S.tree_depth = std::max(S.tree_depth, fm.depth[s]);
            }
            return fm;
        }

        // ---------------- phase 7: the own entries of every front: A slot e = (i_old, j_old) -> permuted (k, l) -> owner front = front of min(k, l)
        void own_entries(Symbolic& S, int const* rp, int const* ci, ivec const& col2front)
        {
            int const n = S.n, nf = S.nfronts, nnz = rp[n];
            ivec qinv(n), eq2k(n);
            for(int k = 0; k < n; ++k) qinv[S.col_src[k]] = k;
            for(int k = 0; k < n; ++k) eq2k[S.row_src[k]] = k;
            S.f_asm_ptr.assign(nf + 1, 0);
            ivec owner(nnz), pos(nnz);
            for(int i = 0; i < n; ++i)
            {
                int const k = eq2k[i];
                for(int e = rp[i]; e < rp[i + 1]; ++e)
                {
                    int const l = qinv[ci[e]];
                    int const s = col2front[std::min(k, l)];
                    int const r = local_of(S, s, k), c = local_of(S, s, l);
                    if(r < 0 || c < 0)
                    {
                        S.error = "internal: matrix entry outside its front";
                        return;
                    }
                    owner[e] = s;
                    pos[e] = (r << 16) | c;
                    ++S.f_asm_ptr[s + 1];
                }
            }
            for(int s = 0; s < nf; ++s) S.f_asm_ptr[s + 1] += S.f_asm_ptr[s];
            S.asm_slot.resize(nnz);
            S.asm_pos.resize(nnz);
            ivec fill(S.f_asm_ptr.begin(), S.f_asm_ptr.end() - 1);
            for(int e = 0; e < nnz; ++e)
            {
                int const d = fill[owner[e]]++;
                S.asm_slot[d] = e;
                S.asm_pos[d] = pos[e];
            }
        }

        // ---------------- phase 8: static fronts (pe_symbolic.hpp): own x-dependent entry / pivot row, or a dynamic child (postorder: children come first)
        void classify_static(Symbolic& S, SymbolicOptions const& opt, int nnz)
        {
            int const nf = S.nfronts;
            S.f_static.assign(nf, 0);
            if(!(opt.dyn_slots && opt.dyn_rows && static_cast<int>(opt.dyn_slots->size()) == nnz && static_cast<int>(opt.dyn_rows->size()) == S.n)) return;
            std::vector<char> dynamic(nf, 0);
            for(int s = 0; s < nf; ++s)
            {
                for(int e = S.f_asm_ptr[s]; e < S.f_asm_ptr[s + 1] && !dynamic[s]; ++e) dynamic[s] = (*opt.dyn_slots)[S.asm_slot[e]] != 0;
                for(int k = S.f_col0[s]; k < S.f_col0[s] + S.f_p[s] && !dynamic[s]; ++k) dynamic[s] = (*opt.dyn_rows)[S.row_src[k]] != 0;
                S.f_static[s] = dynamic[s] ? 0 : 1;
                if(dynamic[s] && S.f_parent[s] >= 0) dynamic[S.f_parent[s]] = 1;
            }
        }

        // ---------------- phase 9: the schedule.
        // Two nested proportional cuts of the assembly tree (from the roots downwards):
        //   level 1 (only when n_parts > 1, the multi-workgroup mode for one or few instances): subtrees costing at most
        //           total / (n_parts * part_cut) become PART subtrees, spread over n_parts workgroups; what stays above is
        //           the TOP, processed one tree level per kernel launch with one workgroup per front;
        //   level 2 (inside every part): subtrees that fit one wavefront's LDS slot and cost at most
        //           part_total / (W * cut_factor) become WAVE subtrees, spread over the W wavefronts of the workgroup;
        //           the rest of the part is COOPERATIVE (whole workgroup).
        // Near a root there is no tree parallelism left, so the upper fronts are always handled by the wider executor.
        struct SubtreeCosts
        {
            std::vector<double> cost, sub;           // of a front (front_cost) / of its whole subtree
            std::vector<char> fits, fits_mid, fits_quad;  // the whole subtree of a front satisfies the limits of the wave / MID / quad class
            double total{};
        };
        SubtreeCosts subtree_costs(Symbolic const& S, SymbolicOptions const& opt)
        {
            int const nf = S.nfronts;
            SubtreeCosts c{std::vector<double>(nf, 0.0), std::vector<double>(nf, 0.0), std::vector<char>(nf, 1), std::vector<char>(nf, opt.quad_mid ? 1 : 0),
                           std::vector<char>(nf, opt.quad ? 1 : 0), 0.0};
            for(int s = 0; s < nf; ++s)
            {
                int const p = S.f_p[s], u = S.f_u[s], m = p + u;
                c.cost[s] = front_cost(p, u);
                c.total += c.cost[s];
                c.fits[s] = c.fits[s] && m <= opt.wave_m && p <= opt.wave_p;
                // lane-group kernel (pe_quad.hpp): two row sets of 16, pivots in the first, one-byte entry indices -- a wave front is a QUAD front
                // when its whole subtree satisfies this; the other wave fronts stay with the per-instance wave phase of factor_part
                bool const lane_group = p <= 16 && S.f_asm_ptr[s + 1] - S.f_asm_ptr[s] <= 255 && S.f_child_ptr[s + 1] - S.f_child_ptr[s] <= 16;
                c.fits_quad[s] = c.fits_quad[s] && m <= 32 && lane_group;
                if(c.fits[s] && opt.wave_slot > 0)
                {
                    // (the slot also holds the right-hand-side column: m doubles behind the image / the panels)
                    long long const whole = (pe_ld(m) + 1LL) * m, panel = static_cast<long long>(pe_ld(m)) * p + static_cast<long long>(pe_ld(p)) * u + m;
                    if(whole > opt.wave_slot && panel > opt.wave_slot) c.fits[s] = 0;
                }
                // MID class of the lane-group kernels: order <= 64 (four row sets), otherwise the wave fronts' limits, whole subtree
                c.fits_mid[s] = c.fits_mid[s] && m <= 64 && lane_group;
                c.sub[s] += c.cost[s];
                int const P = S.f_parent[s];
                if(P >= 0)
                {
                    c.sub[P] += c.sub[s];
                    if(!c.fits[s]) c.fits[P] = 0;
                    if(!c.fits_mid[s]) c.fits_mid[P] = 0;
                    if(!c.fits_quad[s]) c.fits_quad[P] = 0;
                }
            }
            return c;
        }

        // level 1: part_of[s] = part of front s (-1: top), parts numbered in descending cost; part_total[q] = cost of part q
        struct Parts
        {
            ivec part_of;
            std::vector<double> part_total;
        };
        Parts cut_parts(Symbolic const& S, SymbolicOptions const& opt, SubtreeCosts const& c, int K)
        {
            int const nf = S.nfronts;
            Parts P{ivec(nf, K > 1 ? -1 : 0), std::vector<double>(K, 0.0)};
            if(K == 1)
            {
                P.part_total[0] = c.total;
                return P;
            }
            double const limit1 = c.total / (static_cast<double>(K) * opt.part_cut);
            ivec stack, sroots;
            for(int s = 0; s < nf; ++s)
                if(S.f_parent[s] < 0) stack.push_back(s);
            while(!stack.empty())
            {
                int const s = stack.back();
                stack.pop_back();
                if(c.sub[s] <= limit1) sroots.push_back(s);
                else
                    for(int a = S.f_child_ptr[s]; a < S.f_child_ptr[s + 1]; ++a) stack.push_back(S.f_child[a]);
            }
            std::sort(sroots.begin(), sroots.end(), [&c](int a, int b) { return c.sub[a] != c.sub[b] ? c.sub[a] > c.sub[b] : a < b; });
            for(int r: sroots)
            {
                int const pidx = static_cast<int>(std::min_element(P.part_total.begin(), P.part_total.end()) - P.part_total.begin());
                P.part_total[pidx] += c.sub[r];
                for(ivec todo{r}; !todo.empty();)  // the whole subtree of r
                {
                    int const t = todo.back();
                    todo.pop_back();
                    P.part_of[t] = pidx;
                    for(int a = S.f_child_ptr[t]; a < S.f_child_ptr[t + 1]; ++a) todo.push_back(S.f_child[a]);
                }
            }
            // parts in descending cost: the launch dispatches workgroups part by part, the cheapest last (shortest tail)
            ivec order(K), rank(K);
            for(int q = 0; q < K; ++q) order[q] = q;
            std::stable_sort(order.begin(), order.end(), [&P](int a, int b) { return P.part_total[a] > P.part_total[b]; });
            std::vector<double> sorted_total(K);
            for(int q = 0; q < K; ++q)
            {
                rank[order[q]] = q;
                sorted_total[q] = P.part_total[order[q]];
            }
            P.part_total = sorted_total;
            for(int t = 0; t < nf; ++t)
                if(P.part_of[t] >= 0) P.part_of[t] = rank[P.part_of[t]];
            return P;
        }

        // executors: wave w of part q -> q * (W + 1) + w ; cooperative phase of part q -> q * (W + 1) + W ; top fronts: none (-1).
        // Also lays out the wavefronts' backward stacks (f_wstack, f_wpar, wave_stack).
        ivec assign_executors(Symbolic& S, ivec const& part_of, SubtreeCosts const& c, int K, int W)
        {
            int const nf = S.nfronts;
            ivec exec_of(nf, -1), wroot_of(nf, -1);
            S.f_wstack.assign(nf, 0);
            S.f_wpar.assign(nf, -1);
            S.wave_stack = 1;
            // wave subtree roots per part, LPT over the W wavefronts
            std::vector<ivec> wroots(K);
            for(int s = nf - 1; s >= 0; --s)
            {
                if(S.f_kind[s] != 0) continue;
                int const P = S.f_parent[s];
                bool const inner = P >= 0 && part_of[P] == part_of[s] && S.f_kind[P] == 0;
                wroot_of[s] = inner ? wroot_of[P] : s;
                S.f_wpar[s] = inner ? S.f_wstack[P] : -1;
                S.f_wstack[s] = inner ? S.f_wstack[P] + S.f_p[P] + S.f_u[P] : 0;
                S.wave_stack = std::max(S.wave_stack, S.f_wstack[s] + S.f_p[s] + S.f_u[s]);
                if(!inner) wroots[part_of[s]].push_back(s);
            }
            // With the lane-group kernel the quad fronts of a list cost the part's workgroup nothing (they were factored by the launch
            // before, one wavefront per (quad, list), dynamically scheduled: the balance BETWEEN lists hardly matters there), so the W
            // wavefronts of a part are balanced on what they really walk -- the non-quad fronts (measured before: 140..230 us per
            // wavefront of a part with the lists balanced on all fronts) -- and the pure-quad subtrees even out the quad lists after that.
            std::vector<double> sub_nq(nf, 0.0);
            for(int s = 0; s < nf; ++s)
            {
                if(S.f_kind[s] != 0) continue;
                if(!S.f_quad[s]) sub_nq[s] += c.cost[s];
                int const P = S.f_parent[s];
                if(P >= 0 && S.f_kind[P] == 0 && part_of[P] == part_of[s]) sub_nq[P] += sub_nq[s];
            }
            for(int q = 0; q < K; ++q)
            {
                auto& r = wroots[q];
                std::sort(r.begin(), r.end(),
                          [&](int a, int b)
                          {
                              if(sub_nq[a] != sub_nq[b]) return sub_nq[a] > sub_nq[b];
                              return c.sub[a] != c.sub[b] ? c.sub[a] > c.sub[b] : a < b;
                          });
                std::vector<double> load(W, 0.0), load_q(W, 0.0);
                for(int root: r)
                {
                    int w = 0;
                    for(int k = 1; k < W; ++k)
                    {
                        bool const better = sub_nq[root] > 0.0 ? (load[k] < load[w] || (load[k] == load[w] && load_q[k] < load_q[w])) : load_q[k] < load_q[w];
                        if(better) w = k;
                    }
                    load[w] += sub_nq[root];
                    load_q[w] += c.sub[root] - sub_nq[root];
                    exec_of[root] = q * (W + 1) + w;
                }
            }
            for(int s = 0; s < nf; ++s)
            {
                if(S.f_kind[s] == 0) exec_of[s] = exec_of[wroot_of[s]];
                else if(S.f_kind[s] == 1 || S.f_kind[s] == 3)
                    exec_of[s] = part_of[s] * (W + 1) + W;
            }
            return exec_of;
        }

        // the lists of every executor (ascending front index = postorder inside every executor) -> wave_* / coop_*, and the top levels
        // (height above the parts) -> top_*
        std::vector<ivec> executor_lists(Symbolic& S, ivec const& exec_of, int K, int W)
        {
            int const nf = S.nfronts;
            std::vector<ivec> lists(static_cast<size_t>(K) * (W + 1));
            for(int s = 0; s < nf; ++s)
                if(exec_of[s] >= 0) lists[exec_of[s]].push_back(s);
            S.wave_ptr.assign(static_cast<size_t>(K) * (W + 1) + 1, 0);  // per part: W wave lists (entry W of a part is empty, keeps the stride)
            S.wave_list.clear();
            S.coop_ptr.assign(K + 1, 0);
            S.coop_list.clear();
            for(int q = 0; q < K; ++q)
            {
                for(int w = 0; w <= W; ++w)
                {
                    size_t const e = static_cast<size_t>(q) * (W + 1) + w;
                    if(w < W) S.wave_list.insert(S.wave_list.end(), lists[e].begin(), lists[e].end());
                    S.wave_ptr[e + 1] = static_cast<int>(S.wave_list.size());
                }
                auto const& cl = lists[static_cast<size_t>(q) * (W + 1) + W];
                S.coop_list.insert(S.coop_list.end(), cl.begin(), cl.end());
                S.coop_ptr[q + 1] = static_cast<int>(S.coop_list.size());
            }
            ivec h(nf, 0);
            int maxh = 0;
            for(int s = 0; s < nf; ++s)
            {
                if(S.f_kind[s] != 2) continue;
                int hh = 1;
                for(int a = S.f_child_ptr[s]; a < S.f_child_ptr[s + 1]; ++a)
                    if(S.f_kind[S.f_child[a]] == 2) hh = std::max(hh, h[S.f_child[a]] + 1);
                h[s] = hh;
                maxh = std::max(maxh, hh);
            }
            S.top_ptr.assign(maxh + 1, 0);
            S.top_list.clear();
            for(int lev = 1; lev <= maxh; ++lev)
            {
                for(int s = 0; s < nf; ++s)
                    if(S.f_kind[s] == 2 && h[s] == lev) S.top_list.push_back(s);
                S.top_ptr[lev] = static_cast<int>(S.top_list.size());
            }
            return lists;
        }

        struct Schedule
        {
            ivec exec_of;              // executor of a front (assign_executors), -1 for a top front
            std::vector<ivec> lists;   // fronts of every executor, in postorder
        };
        Schedule schedule(Symbolic& S, SymbolicOptions const& opt)
        {
            int const nf = S.nfronts, W = std::max(1, opt.n_waves), K = std::max(1, opt.n_parts);
            S.n_parts = K;
            SubtreeCosts const c = subtree_costs(S, opt);
            Parts const parts = cut_parts(S, opt, c, K);
            // level 2
            S.f_kind.assign(nf, 1);
            for(int s = nf - 1; s >= 0; --s)
            {
                if(parts.part_of[s] < 0)
                {
                    S.f_kind[s] = 2;
                    continue;
                }
                int const P = S.f_parent[s];
                bool const parent_is_wave = P >= 0 && parts.part_of[P] == parts.part_of[s] && S.f_kind[P] == 0;
                if(parent_is_wave) S.f_kind[s] = 0;  // inside a wave subtree
                else
                {
                    double const limit2 = parts.part_total[parts.part_of[s]] / (opt.cut_factor * W);
                    S.f_kind[s] = (c.fits[s] && c.sub[s] <= limit2) ? 0 : (c.fits_mid[s] ? 3 : 1);
                }
            }
            S.f_quad.assign(nf, 0);
            for(int s = 0; s < nf; ++s) S.f_quad[s] = (opt.quad && S.f_kind[s] == 0 && c.fits_quad[s]) ? 1 : 0;
            Schedule sch;
            sch.exec_of = assign_executors(S, parts.part_of, c, K, W);
            sch.lists = executor_lists(S, sch.exec_of, K, W);
            return sch;
        }

        // ---------------- phase 10: storage offsets: the factor panels, then the update-matrix arena
        void place_storage(Symbolic& S, Schedule const& sch, ivec const& depth, SymbolicOptions const& opt)
        {
            int const nf = S.nfronts;
            S.f_lptr.resize(nf);
            S.f_uptr.resize(nf);
            S.f_sptr.assign(nf, 0);
            long long fo = 0;
            for(int s = 0; s < nf; ++s)
            {
                long long const p = S.f_p[s], u = S.f_u[s], m = p + u;
                S.f_lptr[s] = fo;
                fo += m * p;
                S.f_uptr[s] = fo;
                fo += p * u;
            }
            S.factor_doubles = fo;
            // update-matrix arena; a slot holds the u x u update matrix followed by the u-vector of the forward substitution
            // (the right-hand side rides through the factorisation as one more column, pe_front.hpp).  A front whose parent runs on a different executor (or is a top front) keeps its update
            // matrix in a persistent slot; inside one executor the matrices live on TWO LIFO stacks chosen by the parity of
            // the tree depth: a front writes its Schur tiles while later tiles still gather from its children's, so a parent
            // must never overlap its children -- children always sit on the other stack.
            std::vector<char> persistent(nf);
            S.static_root_doubles = 0;
            for(int s = 0; s < nf; ++s)
            {
                int const P = S.f_parent[s];
                // (a MID front is factored by its own launch, before and in another order than the cooperative list it belongs to:
                //  its update matrix cannot live on that executor's LIFO stacks; likewise a QUAD front under a wave front of the per-instance path)
                bool const on_stacks = !(sch.exec_of[s] < 0 || P < 0 || sch.exec_of[P] != sch.exec_of[s] || S.f_kind[s] == 3 || (S.f_quad[s] && !S.f_quad[P]));
                // a static root of the lane-group kernel: the launches that skip the static fronts still assemble its update matrix + vector into
                // the (dynamic) parent -- on the LIFO stacks a later front of the same launch would have overwritten them
                bool const static_quad_root = S.f_quad[s] && S.f_static[s] && P >= 0 && !S.f_static[P];
                if(on_stacks && static_quad_root) S.static_root_doubles += slot_doubles(S.f_u[s]);
                persistent[s] = !on_stacks || static_quad_root;
            }
            long long base = 0;
            for(int s = 0; s < nf; ++s)
                if(persistent[s])
                {
                    S.f_sptr[s] = base;
                    base += slot_doubles(S.f_u[s]);
                }
            for(auto const& lst: sch.lists)
            {
                long long sp[2] = {0, 0}, peak[2] = {0, 0};
                std::vector<long long> rel_off(lst.size(), 0);
                for(size_t qi = 0; qi < lst.size(); ++qi)
                {
                    int const s = lst[qi];
                    for(int a = S.f_child_ptr[s]; a < S.f_child_ptr[s + 1]; ++a)
                    {
                        int const c = S.f_child[a];
                        if(!persistent[c]) sp[depth[c] & 1] -= slot_doubles(S.f_u[c]);
                    }
                    if(persistent[s]) continue;
                    int const q = depth[s] & 1;
                    rel_off[qi] = sp[q];
                    sp[q] += slot_doubles(S.f_u[s]);
                    peak[q] = std::max(peak[q], sp[q]);
                }
                if(sp[0] != 0 || sp[1] != 0)
                {
                    S.error = "internal: executor stacks not empty at the end";
                    return;
                }
                for(size_t qi = 0; qi < lst.size(); ++qi)
                {
                    int const s = lst[qi];
                    if(!persistent[s]) S.f_sptr[s] = base + ((depth[s] & 1) ? peak[0] : 0) + rel_off[qi];
                }
                base += peak[0] + peak[1];
            }
            if(opt.quad)
            {
                S.q_zero_off = base;  // never written: lanes of the lane-group kernel without a contribution read their zeros here
                base += Symbolic::Q_ZERO;
            }
            S.arena_doubles = base;
        }

        // ---------------- phase 11: inverse relative maps of every parent front (per child edge), the largest panel need of a wave front
        void child_maps(Symbolic& S)
        {
            S.f_inv_off.assign(S.f_child.size(), -1);
            S.f_cnp.assign(S.f_child.size(), 0);
            S.f_bmask.assign(S.f_child.size(), 0u);
            S.f_inv.clear();
            S.wave_panel_doubles = 1;
            for(int s = 0; s < S.nfronts; ++s)
            {
                int const m = S.f_p[s] + S.f_u[s];
                if(S.f_kind[s] == 0) S.wave_panel_doubles = std::max<long long>(S.wave_panel_doubles, static_cast<long long>(pe_ld(m)) * S.f_p[s] + static_cast<long long>(pe_ld(S.f_p[s])) * S.f_u[s]);
                for(int a = S.f_child_ptr[s]; a < S.f_child_ptr[s + 1]; ++a)
                {
                    int const c = S.f_child[a];
                    S.f_inv_off[a] = static_cast<long long>(S.f_inv.size());
                    S.f_inv.resize(S.f_inv.size() + m, -1);
                    int* inv = S.f_inv.data() + S.f_inv_off[a];
                    for(int i = 0; i < S.f_u[c]; ++i)
                    {
                        int const l = S.f_rel[S.f_rows_ptr[c] + i];
                        inv[l] = i;
                        if(l >= S.f_p[s]) S.f_bmask[a] |= 1u << std::min((l - S.f_p[s]) >> 4, 31);
                    }
                    int np = 0;
                    while(np < S.f_u[c] && S.f_rel[S.f_rows_ptr[c] + np] < S.f_p[s]) ++np;
                    S.f_cnp[a] = np;
                }
            }
        }
    }  // namespace

    void build_quad_plan(Symbolic& S, int lds_doubles);  // phase 12, below

    bool analyze(int n, int const* rp, int const* ci, double const* vals, SymbolicOptions const& opt, Symbolic& S)
    {
        S = Symbolic{};
        S.n = n;
        S.nnzA = rp[n];
        if(n == 0) return true;

        Ordering ord = fill_reducing_order(n, rp, ci, vals, opt, S.error);
        S.structurally_singular = ord.singular;
        S.n_row_swaps = ord.swaps;
        if(!S.error.empty()) return false;
        ivec& q = ord.q;  // re-permuted twice on the way down: by the postorder of its tree, and by the absorption

        Tree tree = column_tree(ord.gp, ord.gi, q, true);
        for(int j = 0; j < n; ++j) S.nnz_LU += 2LL * static_cast<long long>(tree.st[j].size()) + 1;
        std::vector<SN> const sn = supernodes(tree, q, opt);
        Groups const groups = absorb_children(tree, sn, q, opt, S.error);
        if(!S.error.empty()) return false;
        tree = column_tree(ord.gp, ord.gi, q, false);  // (of the final order)

        std::vector<FR> const fronts = split_into_fronts(tree, groups, q, opt, S.error);
        if(!S.error.empty()) return false;
        FrontMaps const maps = fill_front_tables(S, tree, fronts);
        if(!S.error.empty()) return false;

        S.col_src = q;
        S.row_src.resize(n);
        for(int k = 0; k < n; ++k) S.row_src[k] = ord.rmatch[q[k]];
        own_entries(S, rp, ci, maps.col2front);
        if(!S.error.empty()) return false;
        classify_static(S, opt, rp[n]);

        Schedule const sch = schedule(S, opt);
        place_storage(S, sch, maps.depth, opt);
        if(!S.error.empty()) return false;
        child_maps(S);
        if(opt.quad) build_quad_plan(S, opt.quad_lds_doubles);
        return true;
    }

    // index program of the lane-group kernels (pe_symbolic.hpp "quad plan") for the given lists of fronts (each in postorder).  Every
    // front has <= 16 pivots, <= 255 own entries and <= 16 children (the schedule's `fits` / `fits_mid`); order <= 32 for the wave
    // fronts, <= 64 for the MID fronts; and so has every child (whole subtrees).
    static void build_quad_program(Symbolic& S, std::vector<std::vector<int>> const& lists, int lds_doubles, std::vector<int>& prog, std::vector<int>& lptr,
                                   std::vector<unsigned char>& lane)
    {
        prog.clear();
        lane.clear();
        lptr.assign(2 * lists.size(), 0);
        std::vector<int> lds_off(S.nfronts, -1);
        for(size_t L = 0; L < lists.size(); ++L)
        {
            auto const& lst = lists[L];
            lptr[2 * L] = static_cast<int>(prog.size());
            lptr[2 * L + 1] = static_cast<int>(lst.size());
            size_t prev_hdr = 0;
            int top = 0;  // LDS stack pointer of this list (doubles per instance)
            for(size_t i = 0; i < lst.size(); ++i)
            {
                int const s = lst[i];
                int const p = S.f_p[s], u = S.f_u[s], m = p + u, rs = (m + 15) / 16, M = 16 * rs, rec = M + 16;
                int const ch0 = S.f_child_ptr[s], nch = S.f_child_ptr[s + 1] - ch0;
                size_t const h = prog.size();
                prog.resize(h + Symbolic::Q_HDR + static_cast<size_t>(nch) * Symbolic::Q_CHILD, 0);
                int* q = prog.data() + h;
                size_t const l0 = lane.size();
                lane.resize(l0 + static_cast<size_t>(M) * rec, 0);
                q[0] = m;
                q[1] = p;
                q[2] = S.f_col0[s];
                q[3] = S.f_asm_ptr[s];
                q[4] = nch;
                q[5] = rs;
                q[6] = static_cast<int>(S.f_lptr[s] & 0xffffffffll);
                q[7] = static_cast<int>(S.f_lptr[s] >> 32);
                q[8] = static_cast<int>(S.f_sptr[s] & 0xffffffffll);
                q[9] = static_cast<int>(S.f_sptr[s] >> 32);
                q[10] = static_cast<int>(l0);
                {
                    // this front consumes its children (the top of the stack, postorder), then parks its own update matrix if its
                    // parent belongs to the same list and the stack has room
                    for(int a = nch - 1; a >= 0; --a)
                    {
                        int const c = S.f_child[ch0 + a];
                        if(lds_off[c] >= 0) top = lds_off[c];
                    }
                    int const need = u * (u + 1), P = S.f_parent[s];
                    bool const same_list = P >= 0 && std::find(lst.begin(), lst.end(), P) != lst.end();
                    if(lds_doubles > 0) S.q_lds_total += need;
                    if(same_list && need > 0 && top + need <= lds_doubles)
                    {
                        lds_off[s] = top;
                        top += need;
                        S.q_lds_kept += need;
                    }
                    q[13] = lds_off[s];
                }
                if(i > 0)
                {
                    prog[prev_hdr + 11] = rs;
                    prog[prev_hdr + 12] = static_cast<int>(l0);
                }
                prev_hdr = h;
                for(int e = S.f_asm_ptr[s]; e < S.f_asm_ptr[s + 1]; ++e)
                {
                    int const r = S.asm_pos[e] >> 16, c = S.asm_pos[e] & 0xffff;
                    lane[l0 + static_cast<size_t>(r) * rec + c] = static_cast<unsigned char>(1 + (e - S.f_asm_ptr[s]));
                }
                for(int a = 0; a < nch; ++a)
                {
                    int const c = S.f_child[ch0 + a];
                    int* cb = q + Symbolic::Q_HDR + a * Symbolic::Q_CHILD;
                    cb[0] = static_cast<int>(S.f_sptr[c]);
                    cb[1] = S.f_u[c];
                    cb[18] = lds_off[c];
                    unsigned char* cm = reinterpret_cast<unsigned char*>(cb + 2);
                    for(int k = 0; k < S.f_u[c]; ++k)
                    {
                        int const l = S.f_rel[S.f_rows_ptr[c] + k];
                        cm[l] = static_cast<unsigned char>(1 + k);
                        lane[l0 + static_cast<size_t>(l) * rec + M + a] = static_cast<unsigned char>(1 + k);
                    }
                }
            }
        }
        lane.resize(lane.size() + 64, 0);  // (slack: the prefetch of a row record reads whole 16-byte pieces)
    }

    void build_quad_plan(Symbolic& S, int lds_doubles)
    {
        S.quad = 1;
        S.q_lds_doubles = std::max(0, lds_doubles);
        S.q_lds_kept = S.q_lds_total = 0;
        int const K = std::max(1, S.n_parts), W = static_cast<int>((S.wave_ptr.size() - 1) / K) - 1;
        std::vector<std::vector<int>> lists(static_cast<size_t>(K) * W);
        for(int part = 0; part < K; ++part)
            for(int w = 0; w < W; ++w)
                for(int i = S.wave_ptr[part * (W + 1) + w]; i < S.wave_ptr[part * (W + 1) + w + 1]; ++i)
                    if(S.f_quad[S.wave_list[i]]) lists[static_cast<size_t>(part) * W + w].push_back(S.wave_list[i]);
        build_quad_program(S, lists, S.q_lds_doubles, S.q_prog, S.q_lists, S.q_lane);
        // the same program without the static fronts (pe_symbolic.hpp "static fronts"): the blocks of the dynamic fronts copied list by
        // list -- a child block keeps pointing at its child's arena slot, persistent for a static root --, the look-ahead of a block
        // (row sets and per-lane data of the NEXT front of the list) rebuilt for the shortened list
        S.n_static_quad = 0;
        S.q_prog_dyn.clear();
        S.q_lists_dyn.assign(2 * lists.size(), 0);
        S.row_keep.assign(static_cast<size_t>(S.n), 0);
        for(size_t L = 0; L < lists.size(); ++L)
        {
            S.q_lists_dyn[2 * L] = static_cast<int>(S.q_prog_dyn.size());
            size_t h = static_cast<size_t>(S.q_lists[2 * L]), prev = 0;
            int kept = 0;
            for(int const s: lists[L])
            {
                size_t const len = Symbolic::Q_HDR + static_cast<size_t>(S.q_prog[h + 4]) * Symbolic::Q_CHILD;
                if(S.f_static[s])
                {
                    ++S.n_static_quad;
                    for(int k = S.f_col0[s]; k < S.f_col0[s] + S.f_p[s]; ++k) S.row_keep[static_cast<size_t>(k)] = 1;
                }
                else
                {
                    size_t const d = S.q_prog_dyn.size();
                    S.q_prog_dyn.insert(S.q_prog_dyn.end(), S.q_prog.begin() + static_cast<long>(h), S.q_prog.begin() + static_cast<long>(h + len));
                    S.q_prog_dyn[d + 11] = S.q_prog_dyn[d + 12] = 0;
                    if(kept > 0)
                    {
                        S.q_prog_dyn[prev + 11] = S.q_prog_dyn[d + 5];
                        S.q_prog_dyn[prev + 12] = S.q_prog_dyn[d + 10];
                    }
                    prev = d;
                    ++kept;
                }
                h += len;
            }
            S.q_lists_dyn[2 * L + 1] = kept;
        }
        if(S.q_prog_dyn.empty()) S.q_prog_dyn.push_back(0);
        S.q_bprog.clear();
        // owner front of every pivot column: a front of the backward walk reads the unknowns of its update rows, i.e. of the fronts that
        // own those columns.  It needs the wavefront's fence only if one of them was written by this wavefront since its last fence
        // (the front right before it in the walk, typically its parent); unknowns from earlier launches or from behind an earlier fence
        // are in memory already -- q[6] tells (half of the fronts of M10k: a first child right behind its parent yes, its siblings no).
        std::vector<int> col_owner(static_cast<size_t>(S.n), -1);
        for(int s = 0; s < S.nfronts; ++s)
            for(int c = 0; c < S.f_p[s]; ++c) col_owner[static_cast<size_t>(S.f_col0[s] + c)] = s;
        std::vector<char> pending(static_cast<size_t>(S.nfronts), 0);
        for(auto const& lst: lists)  // (q_lists[2 L + 1] fronts of list L, stored back to back in list order: block index = fronts before it)
        {
            std::vector<int> since_fence;
            for(auto it = lst.rbegin(); it != lst.rend(); ++it)
            {
                int const s = *it;
                bool need = it == lst.rbegin();
                for(int j = 0; j < S.f_u[s] && !need; ++j)
                {
                    int const o = col_owner[static_cast<size_t>(S.f_rows[S.f_rows_ptr[s] + j])];
                    need = o >= 0 && pending[static_cast<size_t>(o)];
                }
                if(need)
                {
                    for(int t: since_fence) pending[static_cast<size_t>(t)] = 0;
                    since_fence.clear();
                }
                pending[static_cast<size_t>(s)] = 1;
                since_fence.push_back(s);
                size_t const h = S.q_bprog.size();
                S.q_bprog.resize(h + Symbolic::Q_BACK, 0);
                int* q = S.q_bprog.data() + h;
                q[0] = S.f_p[s] + S.f_u[s];
                q[1] = S.f_p[s];
                q[2] = S.f_col0[s];
                q[3] = S.f_u[s];
                q[4] = static_cast<int>(S.f_lptr[s] & 0xffffffffll);
                q[5] = static_cast<int>(S.f_lptr[s] >> 32);
                q[6] = need ? 1 : 0;
                for(int j = 0; j < S.f_u[s]; ++j) q[8 + j] = S.f_rows[S.f_rows_ptr[s] + j];
            }
            for(int t: since_fence) pending[static_cast<size_t>(t)] = 0;
        }
        // MID fronts: the subtrees of kind-3 fronts inside a part's cooperative list, dealt out to W lists per part (longest first)
        S.n_mid = 0;
        std::vector<std::vector<int>> mlists(static_cast<size_t>(K) * W);
        for(int part = 0; part < K; ++part)
        {
            std::vector<int> roots, root_of(S.nfronts, -1);
            std::vector<double> cost(S.nfronts, 0.0);
            for(int i = S.coop_ptr[part + 1] - 1; i >= S.coop_ptr[part]; --i)  // parents before children
            {
                int const s = S.coop_list[i];
                if(S.f_kind[s] != 3) continue;
                ++S.n_mid;
                int const P = S.f_parent[s];
                root_of[s] = (P >= 0 && S.f_kind[P] == 3) ? root_of[P] : s;
                if(root_of[s] == s) roots.push_back(s);
                cost[root_of[s]] += front_cost(S.f_p[s], S.f_u[s]);
            }
            std::sort(roots.begin(), roots.end(), [&](int a, int b) { return cost[a] != cost[b] ? cost[a] > cost[b] : a < b; });
            std::vector<double> load(W, 0.0);
            std::vector<int> list_of(S.nfronts, -1);
            for(int r: roots)
            {
                int const w = static_cast<int>(std::min_element(load.begin(), load.end()) - load.begin());
                load[w] += cost[r];
                list_of[r] = w;
            }
            for(int i = S.coop_ptr[part]; i < S.coop_ptr[part + 1]; ++i)  // (ascending = postorder)
            {
                int const s = S.coop_list[i];
                if(S.f_kind[s] == 3) mlists[static_cast<size_t>(part) * W + list_of[root_of[s]]].push_back(s);
            }
        }
        build_quad_program(S, mlists, 0, S.q2_prog, S.q2_lists, S.q2_lane);
    }

    bool build_assembly_lists(Symbolic& S, long long cap_wave, long long cap_team, int const* top_wide, long long cap_top, long long cap_mid)
    {
        int const nf = S.nfronts;
        S.f_mode.assign(nf, 0);
        S.f_keep.assign(nf, 0);
        // top fronts of a level that runs one wide workgroup per front own a CU's LDS: larger cap, and a chain link that follows its
        // child in the same run of single-front levels (same workgroup, one after the other) finds its front already in LDS
        std::vector<int> wide_level(nf, -1);  // level of a top front at a wide level, else -1
        if(top_wide && cap_top > 0)
            for(size_t l = 0; l + 1 < S.top_ptr.size(); ++l)
                // (single-front levels only: measured at 128 instances, the levels with two fronts run 3..5 us SLOWER in the whole-front
                //  layout of the larger cap -- 27 -> 30, 31 -> 36 us -- while the run of single-front levels gains 12 us, 178 -> 166)
                //  (top_wide 2: a level with fronts formed against the larger cap -- every front of it is laid out against that cap)
                if(top_wide[l] == 2 || (top_wide[l] == 1 && S.top_ptr[l + 1] - S.top_ptr[l] == 1))
                    for(int k = S.top_ptr[l]; k < S.top_ptr[l + 1]; ++k) wide_level[S.top_list[k]] = static_cast<int>(l);
        std::vector<char> mid_level(nf, 0);  // a top front at a level of the 8-wavefront launch with half a CU's LDS (top_wide 3)
        if(top_wide && cap_mid > 0)
            for(size_t l = 0; l + 1 < S.top_ptr.size(); ++l)
                if(top_wide[l] == 3)
                    for(int k = S.top_ptr[l]; k < S.top_ptr[l + 1]; ++k) mid_level[S.top_list[k]] = 1;
        S.gl_ptr.assign(nf + 1, 0);
        S.gl_rptr.assign(nf + 1, 0);
        S.gl_sptr.assign(nf + 1, 0);
        S.gl_dst.clear();
        S.gl_cnt.clear();
        S.gl_src.clear();
        if(S.arena_doubles >= (1ll << 31))
        {
            S.error = "update-matrix arena exceeds 2^31 doubles per instance";
            return false;
        }
        std::vector<int> first, next, srcv, cells, cnt;  // per LDS cell: chained list of sources (append order = children's order)
        std::vector<int> last;
        for(int s = 0; s < nf; ++s)
        {
            long long const p = S.f_p[s], u = S.f_u[s], m = p + u;
            long long const cap = S.f_kind[s] == 0 ? cap_wave : (wide_level[s] >= 0 ? std::max(cap_team, cap_top) : (mid_level[s] ? std::max(cap_team, cap_mid) : cap_team));
            int const ch0 = S.f_child_ptr[s], ch1 = S.f_child_ptr[s + 1];
            long long const ldl = pe_ld(static_cast<int>(m)), ldp = pe_ld(static_cast<int>(p));  // odd LDS leading dimensions (pe_device.hpp)
            bool const full = ldl * m + m <= cap;
            bool const link = ch1 - ch0 == 1 && S.f_u[S.f_child[ch0]] == m;
            bool const chain = !full && link;
            S.f_mode[s] = full ? 0 : (chain ? 2 : 1);
            if(link && wide_level[s] >= 1)
            {
                // continued in LDS: the child is the only front of the level below, ran in the whole-front layout (its Schur block sits
                // in its image) in the same workgroup right before this front
                int const c = S.f_child[ch0], l = wide_level[s];
                bool const same_run = wide_level[c] == l - 1 && S.top_ptr[l + 1] - S.top_ptr[l] == 1 && S.top_ptr[l] - S.top_ptr[l - 1] == 1;
                if(same_run && (S.f_mode[c] == 0 || S.f_mode[c] == 3))
                {
                    S.f_mode[s] = 3;
                    S.f_keep[c] = 1;
                }
            }
            if(S.f_mode[s] != 3 && !chain && ch1 > ch0)
            {
                long long const nlds = full ? ldl * m : ldl * p + ldp * u;
                if(nlds + m > 65535)
                {
                    S.error = "front image exceeds the 16-bit cell index of the assembly lists";
                    return false;
                }
                first.assign(static_cast<size_t>(nlds + m), -1);
                last.assign(static_cast<size_t>(nlds + m), -1);
                next.clear();
                srcv.clear();
                auto add = [&](long long d, long long src)
                {
                    int const e = static_cast<int>(srcv.size());
                    srcv.push_back(static_cast<int>(src));
                    next.push_back(-1);
                    if(first[d] < 0) first[d] = e;
                    else
                        next[last[d]] = e;
                    last[d] = e;
                };
                for(int a = ch0; a < ch1; ++a)
                {
                    int const c = S.f_child[a];
                    long long const uc = S.f_u[c], sp = S.f_sptr[c];
                    int const* rel = S.f_rel.data() + S.f_rows_ptr[c];
                    if(full)
                    {
                        for(long long j = 0; j < uc; ++j)
                            for(long long i = 0; i < uc; ++i) add(rel[i] + rel[j] * ldl, sp + i + j * uc);
                    }
                    else
                    {
                        long long np = 0;  // the child's leading update rows that are pivots of this front (f_rel ascends)
                        while(np < uc && rel[np] < p) ++np;
                        for(long long j = 0; j < np; ++j)
                            for(long long i = 0; i < uc; ++i) add(rel[i] + rel[j] * ldl, sp + i + j * uc);          // L panel (columns < p)
                        for(long long j = np; j < uc; ++j)
                            for(long long i = 0; i < np; ++i) add(ldl * p + rel[i] + (rel[j] - p) * ldp, sp + i + j * uc);  // U panel (rows < p)
                    }
                    for(long long i = 0; i < uc; ++i) add(nlds + rel[i], sp + uc * uc + i);  // update vector -> right-hand-side column
                }
                cells.clear();
                cnt.assign(first.size(), 0);
                for(size_t d = 0; d < first.size(); ++d)
                    if(first[d] >= 0)
                    {
                        cells.push_back(static_cast<int>(d));
                        for(int e = first[d]; e >= 0; e = next[e]) ++cnt[d];
                    }
                std::sort(cells.begin(), cells.end(),
                          [&](int a, int b)
                          {
                              if(cnt[a] != cnt[b]) return cnt[a] > cnt[b];
                              return srcv[first[a]] < srcv[first[b]];
                          });
                int const rounds = cells.empty() ? 0 : cnt[cells[0]];
                for(int d: cells) S.gl_dst.push_back(static_cast<unsigned short>(d));
                std::vector<int> cur(cells.size());
                for(size_t k = 0; k < cells.size(); ++k) cur[k] = first[cells[k]];
                for(int r = 0; r < rounds; ++r)
                {
                    int n_r = 0;
                    for(size_t k = 0; k < cells.size() && cnt[cells[k]] > r; ++k)
                    {
                        S.gl_src.push_back(srcv[cur[k]]);
                        cur[k] = next[cur[k]];
                        ++n_r;
                    }
                    S.gl_cnt.push_back(n_r);
                }
            }
            S.gl_ptr[s + 1] = static_cast<int>(S.gl_dst.size());
            S.gl_rptr[s + 1] = static_cast<int>(S.gl_cnt.size());
            S.gl_sptr[s + 1] = static_cast<long long>(S.gl_src.size());
        }
        return true;
    }
}  // namespace pe
