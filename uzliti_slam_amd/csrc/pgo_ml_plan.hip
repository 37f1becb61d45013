// pgo_ml_plan.hip — ml_plan (pgo_ml_plan.hpp): the class of a block system's aggregation hierarchy and its index arrays.  Host code only.
#include "uzl_common.hpp"
#include "pgo_ml_plan.hpp"

#include <algorithm>
#include <utility>

namespace uzl {
namespace {
// Level f + 1 of the hierarchy from level f (F: col and srow of its slots): the pairs of aggregates joined by a fine slot, sorted by
// column within a row, and the Galerkin product's work list.  nf / nc entities below / above, fan_c children per aggregate.
void coarsen(const MlPlan::Level& F, int nf, int nc, int fan_c, MlPlan::Level& C)
{
    const int ns = (int)F.col.size();
    struct Off { int32_t A, C, s; };
    std::vector<Off> off; std::vector<std::pair<int32_t, int32_t>> dg;
    for (int s = 0; s < ns; s++) {
        const int c = F.col[s];
        if (c < 0) continue;
        const int A = F.srow[s] / fan_c, Cc = c / fan_c;
        if (A != Cc) off.push_back({A, Cc, s}); else dg.push_back({A, s});
    }
    // order by (A, C, s) / (A, s).  The slots come in ascending s and a coarse row holds a few dozen of them: a stable counting pass by A,
    // then a small sort inside every row (one std::sort over all of level 0's 100k slots was most of the 4 ms this function took at 10k / 50k)
    {
        std::vector<int32_t> cnt((size_t)nc + 1, 0);
        for (const Off& o : off) cnt[o.A + 1]++;
        for (int a = 0; a < nc; a++) cnt[a + 1] += cnt[a];
        std::vector<Off> tmp(off.size());
        std::vector<int32_t> pos(cnt.begin(), cnt.end() - 1);
        for (const Off& o : off) tmp[pos[o.A]++] = o;
        off.swap(tmp);
        for (int a = 0; a < nc; a++)
            std::sort(off.begin() + cnt[a], off.begin() + cnt[a + 1], [](const Off& x, const Off& y) { return x.C != y.C ? x.C < y.C : x.s < y.s; });
        std::fill(cnt.begin(), cnt.end(), 0);
        for (const auto& d : dg) cnt[d.first + 1]++;
        for (int a = 0; a < nc; a++) cnt[a + 1] += cnt[a];
        std::vector<std::pair<int32_t, int32_t>> dt(dg.size());
        pos.assign(cnt.begin(), cnt.end() - 1);
        for (const auto& d : dg) dt[pos[d.first]++] = d;                  // (s ascending within A already)
        dg.swap(dt);
    }
    C.row_ptr.assign((size_t)nc + 1, 0);
    for (size_t k = 0; k < off.size(); k++) {
        if (k == 0 || off[k].A != off[k - 1].A || off[k].C != off[k - 1].C) {
            C.srow.push_back(off[k].A); C.col.push_back(off[k].C); C.off_ptr.push_back((int32_t)k);
            C.row_ptr[off[k].A + 1]++;
        }
    }
    C.off_ptr.push_back((int32_t)off.size());
    for (int a = 0; a < nc; a++) C.row_ptr[a + 1] += C.row_ptr[a];
    C.n_off = (int32_t)off.size();
    C.diag_ptr.assign((size_t)nc + 1, 0);
    for (size_t k = 0; k < dg.size(); k++) C.diag_ptr[dg[k].first + 1]++;
    for (int a = 0; a < nc; a++) C.diag_ptr[a + 1] += C.diag_ptr[a];
    // The Galerkin product as a GATHER (ml_galerkin_kernel): contribution q comes from fine slot cslot[q]; a workgroup takes a chunk of
    // consecutive output blocks whose contributions (<= kGalItems) it transforms into LDS and sums in order.  chunk = {kind (0: off-
    // diagonal blocks, 1: diagonal blocks), first output, outputs, first contribution, contributions}.
    C.cslot.resize(off.size() + dg.size());
    for (size_t k = 0; k < off.size(); k++) C.cslot[k] = off[k].s;
    for (size_t k = 0; k < dg.size(); k++) C.cslot[off.size() + k] = dg[k].second;
    const int nso = (int)C.col.size();
    for (int b = 0; b < nso;) {                                      // off-diagonal outputs
        int e = b, items = 0;
        while (e < nso && (e == b || items + (C.off_ptr[e + 1] - C.off_ptr[e]) <= kGalItems) && e - b < kGalOutputs) { items += C.off_ptr[e + 1] - C.off_ptr[e]; e++; }
        const int32_t c5[5] = {0, b, e - b, C.off_ptr[b], items};
        C.chunk.insert(C.chunk.end(), c5, c5 + 5);
        b = e;
    }
    for (int a = 0; a < nc;) {                                       // diagonal outputs: + two items (G, M) per child
        int e = a, items = 0;
        auto cost = [&](int A) { return (C.diag_ptr[A + 1] - C.diag_ptr[A]) + 2 * (std::min(nf, (A + 1) * fan_c) - A * fan_c); };
        while (e < nc && (e == a || items + cost(e) <= kGalItems) && e - a < kGalOutputs) { items += cost(e); e++; }
        const int32_t c5[5] = {1, a, e - a, C.n_off + C.diag_ptr[a], C.diag_ptr[e] - C.diag_ptr[a]};
        C.chunk.insert(C.chunk.end(), c5, c5 + 5);
        a = e;
    }
}
}  // namespace

MlPlan ml_plan(const MlPlanIn& in, const std::vector<int32_t>& row_ptr0, const std::vector<int32_t>& col0)
{
    const int nb = in.nb, nslots = in.nslots;
    MlPlan P;
    P.n.assign(1, nb); P.nslots.assign(1, nslots); P.chunks.assign(1, 0); P.fan.assign(1, 1);
    if (!in.precond_on || nb <= kMlTopMax) return P;
    // Up to here the level-1 dense operator applies (6 n_1 <= kMlComp1Max: ml_cg_comp_lm_kernel<16, ...>); above, AGG = 4 with the level-2 one.  Its
    // rebuild (Newton-Schulz GEMMs, n^3) outgrows what the exact level-1 solve saves in PCG iterations between 3000 and 4000 vertices on
    // loopy graphs (>= 3 edges per vertex: 3000/12000 20.6 -> 18.3 ms, 4000/16000 24.5 -> 26.3 ms) and later on sparse ones - the shape of a
    // Schur-reduced online graph (4000/6000 26.0 -> 17.2 ms; config 5's last solve 2328 -> 1288 PCG iterations).
    const bool loopy = nslots >= 6 * nb;
    const int agg1_max = loopy ? kMlAgg1MaxLoopy : kMlAgg1MaxSparse;
    P.agg = (nb <= agg1_max && !in.strong_blocks) ? 1 : 4;           // (strong aggregates in blocks of 4 x 8 rows are laid out for AGG = 4)
    // The dense operator of a hierarchy of `lvl` levels, the ONE statement of where it exists:
    //   level 1 - composite path: one aggregate per workgroup, at least two coarse levels, 6 n_1 <= kMlComp1Max;
    //   level 2 - large graphs (AGG = 4, gather level 2): the same construction one level up - the hierarchy above level 2 as one dense
    // operator that ml_cg_lm_kernel<4, true, ...> applies instead of its LDS walk (measured 733 -> 332 ms at 20k / 100k, the rebuild's
    // Newton-Schulz GEMMs take 7 ms there).  6 n_2 <= kMlComp4Max = 18432 - the cap was 4096 (21.8k vertices)
    // until round 5, and a 30k / 150k graph took 2.39 s (11.9 k PCG iterations on the walked hierarchy) where it takes 0.32 s with the
    // operator (1.8 k), 40k / 200k 5.13 -> 0.62 s, 50k / 250k 10.9 -> 1.56 s (tests/diag/big_graphs.py; at n = 7500 a GEMM is 10 ms, half of
    // that solve), 64k / 320k ~11 -> 2.3 s, 90k / 450k 29.3 -> 6.3 s.  The path ends where ml_cg's gather-level vector no longer fits the LDS
    // (95k vertices: 6 n_2 = 17.9k, 2.6 GB per matrix, a GEMM 136 ms); kMaxPartials ml_spmv workgroups admit 131k.
    // comp4_off: the walked hierarchy instead (tests/test_ab_paths_gpu.py)
    auto dense_level = [&](int lvl) {
        if (P.agg == 1) return (lvl >= 2 && 6 * P.n[1] <= kMlComp1Max) ? 1 : 0;
        return (!in.comp4_off && lvl >= 3 && 6 * P.n[2] <= kMlComp4Max) ? 2 : 0;
    };
    // A level above the composite one may be the top with up to kMlTopWide aggregates: config 2 (1000 vertices: 125 / 16 / 2) loses its
    // 2-aggregate level and with it ten launches per rebuild (the cycle around it and four Newton-Schulz steps of the 96-row level)
    int L = 0;
    while (P.n.back() > (dense_level(L) ? kMlTopWide : kMlTopMax) && L < kMlMaxLevels) {
        const int fan = (L == 1 && P.agg == 4) ? kMlFanout2 : kMlFanout;     // large graphs: level 2 = 4 level-1 aggregates
        P.fan.push_back(fan);
        P.n.push_back((P.n.back() + fan - 1) / fan);
        L++;
    }
    const int cl = dense_level(L);
    // the PCG kernels' LDS: with the dense level-2 operator ml_cg stages nothing but the gather-level vector (ml_cg_variant); the walked
    // hierarchy needs every level above the gather level.  Beyond either limit (and beyond kMaxPartials ml_spmv workgroups = 131k
    // vertices): block-Jacobi - with agg as chosen above, which nothing reads then
    const bool fits = cl == 2 ? ml_comp4_fits(nb, P.n[2]) : ml_fits_lds(P.n.data(), L, P.agg);
    if (!fits) { P.n.assign(1, nb); P.fan.assign(1, 1); return P; }
    P.levels = L;
    P.cl = cl;
    P.gather_level = ml_gather_level(P.agg, L);
    P.lds = cl == 2 ? ml_comp4_lds(P.n[2]) : ml_cg_lds_bytes(P.n.data(), L, P.agg);      // what the variant in use asks for: never above kMlLdsLimit
    // A handle whose graphs made the multiplicative operator break down (chain-like graphs: few loop closures per vertex, the
    // shape of an online run) keeps the additive operator for its later structures instead of failing once per add_graph.
    P.mult = cl > 0 && !in.mult_banned;
    // Newton-Schulz steps of the composite operator per rebuild: 2; 4 on large loopy graphs (AGG = 4, >= 6 slots per row), where two
    // more GEMM pairs per rebuild buy a quarter of the PCG iterations (10k/50k 1882 -> 1455 per solve, 107.7 -> 94.1 ms; 5k/25k 68.6 ->
    // 62.3; 20k/100k 242 -> 224) - on chain-like graphs of that size they cost more than they save (20k/21.7k: 209 -> 261 ms), on
    // small graphs the count barely moves (config 2: 538 -> 511 for +0.3 ms)
    P.ns_steps = P.mult ? ((P.agg == 4 && loopy) ? 4 : 2) : 0;
    // per-level index arrays
    P.lv.resize((size_t)L + 1);
    P.lv[0].col = col0;
    P.lv[0].srow.resize(col0.size());
    for (int a = 0; a < nb; a++) for (int s = row_ptr0[a]; s < row_ptr0[a + 1]; s++) P.lv[0].srow[s] = a;
    for (int f = 0; f < L; f++) {
        MlPlan::Level& C = P.lv[f + 1];
        coarsen(P.lv[f], P.n[f], P.n[f + 1], P.fan[f + 1], C);
        P.nslots.push_back((int32_t)C.col.size());
        P.chunks.push_back((int32_t)(C.chunk.size() / 5));
        P.inner_aggs += P.n[f + 1];                               // one sibling block per aggregate of every coarse level
    }
    // slot ranges by parent aggregate, for every level the multiplicative cycle is built at (cl .. L-1): [n_l*n_{l+1}] begin | end
    if (P.mult) {
        for (int l = cl; l < L; l++) {
            const int n1 = P.n[l], n2 = P.n[l + 1], fan2 = P.fan[l + 1];
            MlPlan::Level& X = P.lv[l];
            X.grp.assign((size_t)2 * n1 * n2, 0);
            for (int i = 0; i < n1; i++) {
                int s = X.row_ptr[i];
                const int send = X.row_ptr[i + 1];
                for (int p = 0; p < n2; p++) {
                    X.grp[(size_t)i * n2 + p] = s;
                    while (s < send && X.col[s] / fan2 == p) s++;
                    X.grp[(size_t)n1 * n2 + (size_t)i * n2 + p] = s;
                }
            }
        }
    }
    return P;
}
}  // namespace uzl

#ifdef UZL_DIAG
// ml_plan without a handle or a device (tests/test_ml_plan.py).  flags: 1 preconditioner on, 2 strong blocks, 4 multiplicative operator
// banned, 8 dense level-2 operator switched off.  Two kinds of call, as uzl_debug_pgo_hierarchy:
//   what < 0:  info[64] = {levels, cl, agg, mult, 0.., [12] Newton-Schulz steps of the structure, [14] gather level, [15] LDS bytes;
//              [16 + l] n_l; [32 + l] fan_l; [48 + l] nslots_l}
//   what >= 0: one array of level `level` (0 row_ptr [n_l + 1], 1 col [nslots_l]; i32).  *nbytes: in = the room at `out` (ignored when out
//              is null), out = the array's size in bytes.
// Stateless: the plan is recomputed per call.
extern "C" UZL_DIAG_EXPORT int uzl_debug_ml_plan(int32_t nb, const int32_t* row_ptr, const int32_t* col, int32_t flags, int32_t level, int32_t what,
                                                 int32_t* info, void* out, int64_t* nbytes)
{
    if (nb < 0 || !row_ptr || (row_ptr[nb] > 0 && !col)) return UZL_ERR_BAD_ARG;
    try {
        const std::vector<int32_t> rp(row_ptr, row_ptr + nb + 1), cc(col, col + rp[nb]);
        uzl::MlPlanIn in;
        in.nb = nb; in.nslots = rp[nb];
        in.precond_on = flags & 1; in.strong_blocks = flags & 2; in.mult_banned = flags & 4; in.comp4_off = flags & 8;
        const uzl::MlPlan P = uzl::ml_plan(in, rp, cc);
        if (what < 0) {
            if (!info) return UZL_ERR_BAD_ARG;
            for (int i = 0; i < 64; i++) info[i] = 0;
            info[0] = P.levels; info[1] = P.cl; info[2] = P.agg; info[3] = P.mult ? 1 : 0; info[12] = P.ns_steps;
            info[14] = P.gather_level; info[15] = (int32_t)P.lds;
            for (int l = 0; l <= P.levels; l++) { info[16 + l] = P.n[l]; info[32 + l] = P.fan[l]; info[48 + l] = P.nslots[l]; }
            return UZL_OK;
        }
        if (!nbytes || P.levels == 0 || level < 0 || level > P.levels || what > 1) return UZL_ERR_BAD_ARG;
        const std::vector<int32_t>& v = what == 1 ? P.lv[level].col : (level == 0 ? rp : P.lv[level].row_ptr);
        const int64_t bytes = (int64_t)v.size() * 4;
        if (out && bytes) {
            if (*nbytes < bytes) return UZL_ERR_BAD_ARG;
            memcpy(out, v.data(), (size_t)bytes);
        }
        *nbytes = bytes;
        return UZL_OK;
    } catch (const std::bad_alloc&) {
        return UZL_ERR_OOM;
    }
}
#endif
