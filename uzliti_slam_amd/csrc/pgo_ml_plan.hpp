// pgo_ml_plan.hpp — the symbolic aggregation hierarchy of the multilevel preconditioner as a host-side value: which class a block system
// gets (aggregates per PCG workgroup, levels, fan-outs, dense level, gather level, multiplicative or additive, Newton-Schulz steps, LDS
// demand - or block-Jacobi) and every level's index arrays.  Pure integer work: no handle, no HIP call, no environment.  A structure is
// made in three steps, each plan -> upload -> bind (uzl_pgo.hip: build_structure): system_plan (pgo_structure.hpp) -> schur_plan
// (pgo_schur.hpp) -> ml_plan, uploaded by upload_ml (arena layout and descriptors).
// tests/test_ml_plan.py holds the class boundaries on the CPU through uzl_debug_ml_plan.
#pragma once
#include "pgo_types.hpp"

#include <vector>

namespace uzl {
// launch geometry and LDS demand of the PCG kernels (pgo_ml_kernels.hip)
int g_ml_rows(int nb, int agg);
int g_ml_spmv(int nb, int agg);
size_t ml_cg_lds_bytes(const int* n, int levels, int agg);
bool ml_fits_lds(const int* n_per_level, int levels, int agg);
// The ONE statement of the PCG kernels' LDS budget and of what ml_cg stages when the dense level-2 operator is present (the gather-level
// vector and nothing else): ml_plan's admission test, ml_cg_variant and ml_fits_lds all read these (tests/test_ml_admission.py
// holds the boundaries through uzl_debug_ml_admission)
// (kMlLdsLimit, ml_comp4_lds: pgo_types.hpp)
bool ml_comp4_fits(int nb, int n2);          // LDS of the comp4 variant and ml_spmv's partial count

struct MlPlanIn {
    int nb = 0, nslots = 0;        // the block system the PCG solves: the full one or the Schur-reduced one
    bool precond_on = true;        // uzl_pgo_cfg::preconditioner != 0
    bool strong_blocks = false;    // a reduced system numbered by strong aggregates in blocks of 4 x 8 rows (SchurPlan)
    bool mult_banned = false;      // the multiplicative operator broke down on an earlier graph of the handle
    bool comp4_off = false;        // diagnostic switch UZL_ML_NO_COMP4: the walked hierarchy instead of the dense level-2 operator
};

struct MlPlan {
    int levels = 0;                // 0: block-Jacobi
    int agg = 4;                   // level-1 aggregates per PCG workgroup (1: small graphs, 4: large)
    int cl = 0;                    // level of the dense operator (1: small graphs, 2: AGG = 4), 0 = none
    int gather_level = 0;          // level whose residual the PCG kernels gather (ml_gather_level); 0 without a hierarchy
    bool mult = false;             // the dense operator is built by the multiplicative cycle (pgo_ml_kernels.hip); false: additive
    int ns_steps = 0;              // Newton-Schulz refinements of the dense operator per rebuild
    size_t lds = 0;                // dynamic LDS the ml_cg variant in use asks for: never above kMlLdsLimit
    int inner_aggs = 0;            // aggregates of all coarse levels: one sibling block each
    std::vector<int32_t> n, fan, nslots, chunks;       // per level: entities, children per aggregate, off-diagonal blocks, work chunks of ml_galerkin_kernel
    // index arrays per level (MlLevel, pgo_types.hpp); cslot / chunk: ml_galerkin_kernel's work list; grp: slot ranges by parent aggregate
    // [n_l * n_{l+1}] begin | end, for every level the multiplicative cycle is built at (cl .. L-1, when mult).  Level 0: col and srow only.
    struct Level { std::vector<int32_t> row_ptr, col, srow, off_ptr, diag_ptr, cslot, chunk, grp; int32_t n_off = 0; };
    std::vector<Level> lv;
    void release_indices() { std::vector<Level>().swap(lv); }      // once uploaded: the scalars and per-level sizes stay
};

// deterministic; row_ptr [nb + 1] / col [nslots] (-1: fixed neighbour) of the block system
MlPlan ml_plan(const MlPlanIn& in, const std::vector<int32_t>& row_ptr, const std::vector<int32_t>& col);
}  // namespace uzl
