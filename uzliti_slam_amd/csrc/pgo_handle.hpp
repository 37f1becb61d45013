// pgo_handle.hpp — the pose-graph handle (struct uzl_pgo), the kernel launchers and the host-side pieces shared by the translation
// units behind uzl_pgo_*: uzl_pgo.hip (C ABI, structure uploads, the host-driven Levenberg-Marquardt loop), uzl_pgo_lm.hip (the device-resident
// loop: captured passes over slot twins), uzl_pgo_debug.hip (the stage hooks of the diagnostic library).  Private to csrc/: the product surface is include/uzl_mi355x.h.
#pragma once
#include "uzl_common.hpp"
#include "pgo_types.hpp"
#include "pgo_schur.hpp"
#include "pgo_ml_plan.hpp"
#include "pgo_structure.hpp"
#include "pgo_lm.hpp"
#include "pgo_lm_pass.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <functional>
#include <limits>
#include <new>
#include <numeric>

namespace uzl {
void k_prepare_nodes(const uzl_node* nodes, int n, int xy, double* pose, hipStream_t s);
void k_prepare_flat_nodes(const double* poses12, int n, double* pose, hipStream_t s);
void k_prepare_edges(const uzl_edge* edges, const int32_t* src, int e, const double* sensors, int ns, int xy, int odom_params,
                     double* zinv, double* info, hipStream_t s);
void k_prepare_flat_edges(const double* meas12, const double* info36, int e, double* zinv, double* info, hipStream_t s);
int k_chi2(const PgoDev& D, const double* pose, double delta, hipStream_t s);
int k_chi2_trial(const PgoDev& D, const double* pose, double delta, hipStream_t s);
hipError_t k_hessian(const PgoDev& D, const double* pose, double delta, int* g_edges, int* g_rows, hipStream_t s, bool with_chi2 = true, hipEvent_t ev_a = nullptr,
                     hipEvent_t ev_b = nullptr);
void k_finalize(const PgoDev& D, int na, int nb_, int nc, int what, hipStream_t s);
int k_diagmax(const PgoDev& D, hipStream_t s);
void k_precond(const PgoDev& D, hipStream_t s);
void k_publish(const PgoDev& D, PgoHostScal* out_dev, uint32_t seq, hipStream_t s);
void k_set_scalar(double* dst, double v, hipStream_t s);
void k_set_scalar2(double* dst_a, double va, double* dst_b, double vb, hipStream_t s);
void k_residual_guard(const PgoDev& D, hipStream_t s);
void k_pcg_progress(const PgoDev& D, hipStream_t s);
void k_set_trial(double* scal, double lambda, double tol_f2, double eps_t, double eps_r, hipStream_t s);
int k_pcg_init(const PgoDev& D, double* p0, double* p1, hipStream_t s);
int k_pcg_spmv(const PgoDev& D, const double* p_old, double* p_new, int n_part, double tol2, hipStream_t s);
int k_pcg_update(const PgoDev& D, const double* p, int n_part, hipStream_t s);
int g_pcg_spmv(int nb);
int g_pcg_update(int nb);
// (g_ml_rows, g_ml_spmv, ml_cg_lds_bytes, ml_fits_lds, ml_comp4_fits: pgo_ml_plan.hpp)
int k_oplus(const PgoDev& D, const double* pose_in, double* pose_out, hipStream_t s);
int g_edges_for(int e);
void k_slot_records(const double* zinv, const double* info, int e, const int32_t* slot_edge, int nslots, double* srec, hipStream_t s);
int g_oplus_for(int n);
void k_edge_error(const PgoDev& D, const double* pose, double* err, hipStream_t s);
void k_poses_out(const double* pose, int n, double* out12, hipStream_t s);
void k_schur_gather(const PgoDev& D, const SchurDev& S, hipStream_t s);
// slot twins of the device-resident LM loop (pgo_types.hpp: LmSlot / LmDev / LmShape)
void k_lm_head(const LmSlot* slots, int nslots, int pass_flags, hipStream_t s);
void k_lm_tail(const LmSlot* slots, int nslots, hipStream_t s);
hipError_t kl_linearize(const LmSlot* sl, int nslots, int g_edges, int g_asm, hipStream_t s);
void kl_eval(const LmSlot* sl, int nslots, int g_edges, int g_oplus, hipStream_t s);
// The Schur reduction and the hierarchy set-up, for both loops: a slot table (`which`: the segment of a pass, pgo_ml_kernels.hip) or the
// host-driven loop's HostSlot (timer, may be null: the profiled solve's records).  ns_steps: Newton-Schulz steps of the composite level.
// level1_done (may be empty) runs once level 1's Galerkin product is enqueued: a sharded solve all-reduces it there.
void kl_schur_reduce(const LmSlot* sl, const LmShape& sh, hipStream_t s);
void kl_schur_backsub(const LmSlot* sl, const LmShape& sh, hipStream_t s);
void kl_schur_reduce(const HostSlot& hs, const LmShape& sh, hipStream_t s, KernelTimer* timer);
void kl_schur_backsub(const HostSlot& hs, const LmShape& sh, hipStream_t s, KernelTimer* timer);
void kl_ml_numeric(const LmSlot* sl, const LmShape& sh, int which, hipStream_t s);
void kl_ml_trial(const LmSlot* sl, const LmShape& sh, int which, int ns_steps, hipStream_t s);
void kl_ml_numeric(const HostSlot& hs, const LmShape& sh, hipStream_t s, KernelTimer* timer, const std::function<void()>& level1_done);
void kl_ml_trial(const HostSlot& hs, const LmShape& sh, int ns_steps, hipStream_t s, KernelTimer* timer);
void ml_cg_variant(const MlHot& ml, int agg, size_t lds_full, int32_t* variant, int32_t* comp_u, uint64_t* lds);
hipError_t kl_ml_init(const LmSlot* sl, const LmSlot* by_value, const LmShape& sh, int ix, bool in_head, hipStream_t s);
// a one-graph pass of the small-graph class may send its PCG init as further workgroups of the head's launch (lm_init_rides, pgo_lm_pass.hpp)
bool lm_init_rides_shape(const LmSlot* by_value, const LmShape& sh);
void kl_lm_head_init(const LmSlot* sl, const LmSlot* by_value, int pass_flags, int ix, hipStream_t s);
hipError_t kl_ml_pcg_its(const LmSlot* sl, const LmSlot* by_value, const LmShape& sh, int ix, double tol2, int first, int n, hipStream_t s, hipEvent_t* ev = nullptr);
// the same PCG kernels for the host-driven loop (pgo_types.hpp: HostSlot): init, and the two launches of iteration `parity` one by one
void kl_ml_pcg_init(const HostSlot& hs, const LmShape& sh, hipStream_t s);
void kl_ml_spmv(const HostSlot& hs, const LmShape& sh, int parity, hipStream_t s, hipEvent_t ev_a = nullptr, hipEvent_t ev_b = nullptr);
hipError_t kl_ml_cg(const HostSlot& hs, const LmShape& sh, int parity, int init, hipStream_t s, hipEvent_t ev_a = nullptr, hipEvent_t ev_b = nullptr);
}  // namespace uzl



namespace uzl { struct LmRun; }
using namespace uzl;      // (private header of the uzl_pgo_* translation units; the handle itself is the C ABI's global-namespace type)

// The device buffers of one block system the PCG can run on: the full system over the free vertices, or the Schur-reduced one over the
// separators (uzl_pgo::Reduced).  build_structure sizes, fills and binds either with the same calls.
struct SysBufs {
    DevBuf<int32_t> row_ptr, col, rowhdr, b2v;
    DevBuf<double> blk, hdiag, minv, x, xs, r, z, p, p2, ap;
    // sizes for nb rows, then copies the index arrays and the row headers (row_headers, pgo_structure.hpp): keep the arguments until the
    // stream has been synchronised
    void upload(int nb, const std::vector<int32_t>& h_row_ptr, const std::vector<int32_t>& h_col, const std::vector<int32_t>& h_b2v, const std::vector<int32_t>& h_rowhdr,
                hipStream_t s)
    {
        const int nslots = h_row_ptr[nb];
        const size_t nbz = std::max(nb, 1), nsz = std::max(nslots, 1);
        b2v.reserve(nbz); row_ptr.reserve(nbz + 1); col.reserve(nsz); rowhdr.reserve(nbz * kRowHdr);
        blk.reserve(nsz * 36);
        hdiag.reserve(nbz * 42); minv.reserve(nbz * 36);               // [H_aa | b] contiguous: one all-reduce when sharded
        x.reserve(nbz * 6); xs.reserve(nbz * 6); r.reserve(nbz * 6); z.reserve(nbz * 6); p.reserve(nbz * 6); p2.reserve(nbz * 6);
        ap.reserve(nbz * 12 + kMaxPartials);                           // [A p | restricted A p | partials]
        if (nb > 0) UZL_HIP(hipMemcpyAsync(b2v.p, h_b2v.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice, s));
        UZL_HIP(hipMemcpyAsync(row_ptr.p, h_row_ptr.data(), sizeof(int32_t) * (nb + 1), hipMemcpyHostToDevice, s));
        if (nslots > 0) UZL_HIP(hipMemcpyAsync(col.p, h_col.data(), sizeof(int32_t) * nslots, hipMemcpyHostToDevice, s));
        UZL_HIP(hipMemcpyAsync(rowhdr.p, h_rowhdr.data(), sizeof(int32_t) * h_rowhdr.size(), hipMemcpyHostToDevice, s));
    }
    void bind(PgoDev& D, int nb, int nslots) const
    {
        D.nb = nb; D.nslots = nslots;
        D.b2v = b2v.p; D.row_ptr = row_ptr.p; D.col = col.p; D.rowhdr = rowhdr.p;
        D.blk = blk.p; D.hdiag = hdiag.p; D.minv = minv.p; D.b = hdiag.p + (size_t)nb * 36;
        D.x = x.p; D.xs = xs.p; D.r = r.p; D.z = z.p; D.p = p.p; D.ap = ap.p; D.part_a = ap.p + (size_t)std::max(nb, 1) * 12;
    }
};

struct uzl_pgo : uzl::HandleBase {
    uzl_pgo_cfg cfg;
    hipStream_t stream = nullptr;
    // ---- host-side structure of the current problem
    int32_t n = 0, e_in = 0, e = 0, nb = 0, nslots = 0;
    std::vector<uint8_t> fixed_in, fixed_eff;
    std::vector<int32_t> ij;       // system edges, 2 per edge
    std::vector<int32_t> src;      // system edge -> input edge
    std::vector<InEdge> in_edges;  // the input edges of uzl_pgo_add_graph (pgo_structure.hpp), kept so that uzl_pgo_append_graph can grow the graph in place
    bool in_ready = false;         // in_edges / d_edges describe the current graph (add_graph or append_graph, not set_graph)
    int32_t n_sensors_in = 0;
    std::vector<uint8_t> robust;
    std::vector<double> edge_w;    // trace of each system edge's information matrix: the coupling strength the aggregation order follows
    bool have_graph = false, structure_ready = false;
    int32_t n_gauge = 0;
    // ---- device
    DevBuf<double> pose_a, pose_b, pose_init;
    double* cur = nullptr;
    double* trial = nullptr;
    DevBuf<int32_t> d_v2b, d_ei, d_ej, d_src, d_flags;
    SysBufs sys;                               // the full system over the free vertices
    DevBuf<int32_t> d_slot_edge, d_rb_ptr;
    DevBuf<double> d_srec;                     // slot records (pgo_kernels.hip: slot_records_kernel): values of the edges in the order of the structure's slots
    DevBuf<int4> d_smeta;
    bool srec_stale = true;                    // edges' values or the structure changed since d_srec was written
    DevBuf<double> d_zinv, d_info;
    DevBuf<double> d_part_a, d_part_b, d_part_c, d_scal, d_err, d_out12, d_stage;
    DevBuf<uint8_t> d_robust;
    DevBuf<uzl_node> d_nodes;
    DevBuf<uzl_edge> d_edges;
    // uzl_pgo_rewrite_graph: the edge buffer the surviving records are compacted into (then swapped with d_edges), the plan's index
    // arrays [records 4 e | new_to_old_edge e | node sources n], and [xf 12 n_xf | the placed poses 8 n_pose]
    DevBuf<uzl_edge> d_edges_spare;
    DevBuf<int32_t> d_rw_idx;
    DevBuf<double> d_rw_val;
    PinBuf<PgoHostScal> h_scal;     // pinned + coherent: written by publish_kernel, polled by the host
    PgoHostScal* d_pub = nullptr;    // its device-side address
    uint32_t pub_seq = 0;
    PinBuf<double> h_lambda;
    PgoDev D;
    // The system the PCG (and its preconditioner) sees: D itself, or - when chain interiors are Schur-eliminated (pgo_schur.hpp) - the
    // reduced system over the separator vertices.  scal / flags / part_b / part_c are shared with D.
    PgoDev Dp;
    double* pbuf[2] = {nullptr, nullptr};      // PCG direction, ping-pong (of the Dp system)
    struct Reduced {
        bool on = false, strong = false, strong_blocks = false;      // strong: numbered by strong aggregates, with empty rows (SchurPlan); _blocks: in blocks of 4 groups
        int32_t n_int = 0, n_runs = 0, longest_run = 0, n_sep = 0;
        DevBuf<int32_t> run_ptr, run_rows, slotP, slotN, endL, endR, sep_rows, rsrc, inc_ptr, inc;
        DevBuf<double> elim, runout, runblk;
        SysBufs sys;                           // the reduced system over the separators
        SchurDev S;
    } red;
    int prev_pcg_iters = 0;
    double num_its[2] = {-1., -1.};            // PCG iterations per LM trial of the last solve with the reduced system in row order / by strong aggregates
    int num_last = -1;                         // numbering of that solve (-1: none yet); see reduced_numbering (pgo_structure.hpp)
    // multilevel preconditioner: the class and per-level sizes of this structure's hierarchy as ml_plan decided them (its index arrays
    // released once uploaded); levels = 0: block-Jacobi
    MlPlan mlp;
    // STATE, not plan: initialised from mlp.mult / mlp.ns_steps with every multilevel structure, then changed for the life of the
    // structure by the additive fallback (do_optimize_host).  Everything else about the class is read from mlp.
    bool ml_mult = false;            // the dense operator in use is the multiplicative cycle's (pgo_ml_kernels.hip)
    int ml_ns_steps = 0;             // Newton-Schulz refinements of the dense operator per rebuild
    // Two complete copies of the preconditioner's numeric state (arena, device descriptor, kernel-argument block, PCG graph): the
    // solver applies copy `ml_ix` while a rebuild for the next LM iteration runs on `stream2` into the other one.
    struct MlBuf {
        MlDev* dml = nullptr;                  // device copy of the descriptor
        MlHot hot;                             // hot subset, by-value kernel argument
        double* rg[2] = {nullptr, nullptr};    // double-buffered gather-level residual
        double* y1 = nullptr; double* nsT = nullptr; double* nsX = nullptr;
        double* l1_span_ptr = nullptr;         // level-1 Galerkin arrays (blk | G | M), all-reduced once per linearisation
        hipGraph_t graph = nullptr; hipGraphExec_t graph_exec = nullptr;        // 2 x kGraphPairs PCG iterations
        hipGraph_t graph_s = nullptr; hipGraphExec_t graph_exec_s = nullptr;    // 2 x kShortPairs: the solves of a converged LM iteration end after 2 - 4
    } mlb[2];
    double* ml_dense_ptr[2][kMlMaxLevels + 1] = {};   // host copy of MlDev::Ydense per hierarchy copy
    int ml_ix = 0;                             // = LmDev::ix of the host-driven loop's state (do_optimize_host keeps it in step; host_slot reads it)
    hipStream_t stream2 = nullptr;
    bool streams_borrowed = false;             // stream / stream2 are a batch's (uzl_pgo_batch_create): not this handle's to destroy
    hipEvent_t ev_lin = nullptr, ev_setup = nullptr;
    DevBuf<double> d_scal2;                    // lambda slot (scal[3]) for the kernels of an asynchronous rebuild
    DevBuf<uint8_t> ml_arena;
    size_t ml_copy_stride = 0;                 // bytes between the two hierarchy copies inside ml_arena
    DevBuf<MlDev> d_ml;
    bool no_graph = false;          // UZL_NO_GRAPH=1: eager launches (rocprofv3 --kernel-trace crashes on hipGraphLaunch here)
    // shard (BASELINE config 4)
    int32_t rank = 0, world = 1;
    uzl_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    void* rccl_comm = nullptr;       // ncclComm_t owned by the handle (uzl_pgo_set_shard_rccl); the exchange then needs no callback
    bool sharded = false;            // an exchange (callback or communicator) is set and the multilevel path is active for this structure
    DevBuf<double> d_red;
    int64_t iter_span = 0;           // doubles all-reduced per PCG iteration: [A p | restricted A p | p.Ap partials]
    int64_t l1_span = 0;
    // per-optimize accounting (uzl_pgo_stats)
    double structure_ms = 0., exchange_ms = 0.;
    int32_t exchange_calls = 0;
    bool structure_reused = false;
    double last_residual_ratio = 0.;
    int32_t guard_trips = 0;
    uint64_t structure_gen = 0;      // bumped by build_structure: batches rebuild their slots when it moves
    bool mult_banned = false;        // the multiplicative operator broke down on a graph of this handle: later structures start additive
    KernelTimer timer;
    uzl::LmRun* lm = nullptr;        // the device-resident LM loop's slot table and captured passes (uzl_pgo_lm.hip)
    // the host-driven loop's slot and launch geometry of the multilevel PCG kernels, for structure generation ml_slot_gen (uzl_pgo.hip: host_slot)
    LmSlot ml_slot{};
    LmShape ml_shape{};
    uint64_t ml_slot_gen = ~0ull;
    bool last_structure_reused = false;
    std::chrono::steady_clock::time_point t_start;      // start of the running uzl_pgo_optimize (solve_ms)
};

namespace uzl {
// ---- when a linear solve stops (uzl_pgo.hip "When a linear solve stops"; cfg.pcg_stop = 1: the plain relative test - no floor factor,
//      and a step accuracy of 0 switches the look off: progress_unit, pgo_device.hpp)
inline double pgo_tol_f2(const uzl_pgo_cfg& c) { return c.pcg_stop == 1 ? 1. : kTolFloor2; }
inline double pgo_eps_t(const uzl_pgo_cfg& c) { return c.pcg_stop == 1 ? 0. : kStepT * c.pcg_tol; }
inline double pgo_eps_r(const uzl_pgo_cfg& c) { return c.pcg_stop == 1 ? 0. : kStepR * c.pcg_tol; }
// ---- shared host-side pieces (uzl_pgo.hip)
void build_structure(uzl_pgo* h);                     // system plan, Schur plan, hierarchy plan (pgo_structure.hpp), each uploaded and bound; bumps structure_gen
void ensure_structure(uzl_pgo* h);                    // gauge + build_structure, unless the structure is ready
void destroy_pcg_graph(uzl_pgo* h);
bool ml_async_level(const uzl_pgo* h);
double ml_rate_drop(const uzl_pgo* h);
void prepare_optimize(uzl_pgo* h);                    // optimizeImpl's front part: gauge + structure (cached), t_start
void own_streams(uzl_pgo* h, bool drain_borrowed);               // a batch's handle takes streams of its own (uzl_pgo.hip)
int do_optimize_host(uzl_pgo* h, int32_t iterations, uzl_pgo_stats* st);      // the host-driven loop (sharded / block-Jacobi / profiled solves, anomaly fallback)
int do_optimize(uzl_pgo* h, int32_t iterations, uzl_pgo_stats* st);           // picks the loop
// ---- pieces of the host-driven loop the stage hooks drive one by one (uzl_pgo.hip; uzl_pgo_debug.hip)
HostSlot host_slot(uzl_pgo* h);                       // the slot twins' slot for this handle, the hierarchy copy in use, the current pose buffer
void set_lambda(uzl_pgo* h, double lambda, double tol_f2);
void ml_setup_numeric(uzl_pgo* h, const HostSlot& hs, hipStream_t s, KernelTimer* timer);
int pcg_solve(uzl_pgo* h, LmDev& lm);                 // one (H + lambda I) dx = b solve of the trial `lm` is in; returns lm_solve_verdict (0: converged)
inline double tol_factor2(const uzl_pgo_cfg& c) { return pgo_tol_f2(c); }
// ---- the device-resident loop (uzl_pgo_lm.hip)
struct LmRun;                                          // captured passes + slot table of one handle (or one batch)
void lm_run_destroy(LmRun* r);
bool lm_eligible(const uzl_pgo* h);
int do_optimize_lm(uzl_pgo* h, int32_t iterations, uzl_pgo_stats* st);
bool lm_batch_eligible(const std::vector<uzl_pgo*>& hs);
LmDev lm_initial_state(const uzl_pgo* h, int iterations, bool sync_rebuild);      // the state a graph starts its LM loop in (both loops)
void lm_stats(const LmDev& v, uzl_pgo_stats& S);                                   // ... and what its final state says in the stats
LmSlot make_slot(const uzl_pgo* h, LmDev* d_lm, LmHost* d_pub);
LmShape make_shape(const std::vector<uzl_pgo*>& hs, int nslots, bool batch_geometry);
int batch_optimize_lm(LmRun*& R, const std::vector<uzl_pgo*>& hs, int resident, hipStream_t s, hipStream_t s2, int32_t iterations, bool eager, bool verbose, KernelTimer* timer,
                      uzl_pgo_stats* stats, int* rc_all);
constexpr int kSchurStrongOneMax = 256;                // strong aggregates: up to this many groups as ONE level (level-1 path), beyond in blocks of 4 (pgo_schur.hpp)
extern const int kUpperNs;                            // Newton-Schulz steps of the dense levels above the composite level
// lazy refresh of the multilevel preconditioner (lm_refresh): rebuilt when the last step moved chi2 by more than kRefreshRel ... and,
// where the rebuild is synchronous (large loopy graphs: its GEMMs are 1.4 ms at 10k / 50k, 7 ms at 20k / 100k, in front of the solve),
// by the chi2 rule only while the problem still changes wholesale (kRefreshRelSync), the PCG-rate rule (kRateDrop, pgo_lm.hpp) from then on
constexpr double kRefreshRel = 1e-3;
constexpr double kRefreshRelSync = 3e-2;
// (kLambdaRetake, kGraphPairs, kShortPairs and ml_ns_steps_at: pgo_lm_pass.hpp, with the host's other predictions about a solve)

// The head of uzl_pgo_stats: what the structure of the solved graph says, the same for both loops
inline void stats_head(const uzl_pgo* h, uzl_pgo_stats& S)
{
    S.structure_reused = h->last_structure_reused ? 1 : 0;
    S.n_vertices = h->n; S.n_edges = h->e; S.n_gauge_fixed = h->n_gauge;
    S.n_eliminated = h->red.on ? h->red.n_int : 0; S.reduced_strong = (h->red.on && h->red.strong) ? 1 : 0;
}

// Diagnostic build, UZL_PHASES=1: GPU time between the marks a loop sets on the solver's stream (graph replays as in production), summed
// per mark over the solve and printed after it; UZL_PHASES_EACH=1: every stretch as well.  N marks per round (LM iteration or pass),
// named by the loop.
template <int N>
struct PhaseMarks {
    std::vector<hipEvent_t> ev;
    std::vector<int> tag;
    static bool on() { static const bool v = diag_flag("UZL_PHASES"); return v; }
    void mark(int t, hipStream_t s)
    {
        if (!on()) return;
        hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, s); ev.push_back(e); tag.push_back(t);
    }
    // after the stream has been synchronised: "<what> over <rounds> <unit>" and the sums
    void report(const char* what, int rounds, const char* unit, const char* const (&names)[N])
    {
        if (!on() || ev.size() <= 1) return;
        double acc[N] = {};
        static const bool each = diag_flag("UZL_PHASES_EACH");
        for (size_t i = 0; i + 1 < ev.size(); i++) {
            float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]); acc[tag[i] % N] += ms;
            if (each) fprintf(stderr, "%s%d:%.0f", tag[i] == 0 ? "\n[uzl_pgo]   " : " ", tag[i], 1e3 * ms);
        }
        if (each) fprintf(stderr, "\n");
        fprintf(stderr, "[uzl_pgo] %s over %d %s (GPU event time, ms):", what, rounds, unit);
        for (int k = 0; k < N; k++) fprintf(stderr, "  %s %.3f", names[k], acc[k]);
        fprintf(stderr, "\n");
    }
    ~PhaseMarks() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
};
}  // namespace uzl
