// uzl_pgo.hip — host side of the pose-graph half: the graph-entry calls, the structure's uploads (its plans are host-side values:
// pgo_structure.hpp, pgo_schur.hpp, pgo_ml_plan.hpp), the Levenberg-Marquardt driver and the C ABI (uzl_pgo_*, uzl_pgo_batch_*).
// Mirrors G2oOptimizer (graph_optimization/src/g2o_optimizer.cpp:55-349): add_graph = addGraphImpl,
// optimize = optimizeImpl (initializeOptimization + setFixedNodes + optimize(iterations)),
// store = storeImpl.  All arithmetic on poses, measurements and the normal equations runs in the HIP
// kernels of pgo_kernels.hip; the host only makes the integer/structural decisions and the scalar LM
// accept/reject logic of g2o's OptimizationAlgorithmLevenberg [EXT].
#include "merge_types.hpp"
#include "pgo_handle.hpp"
#include "pgo_lm.hpp"
#include "pgo_rewrite.hpp"
#include "scope_types.hpp"
#include "uzl_streams.hpp"

#include <array>

using namespace uzl;

// ---- RCCL through dlopen: the collective library is only loaded by processes that shard a graph -----------------------------
#include <dlfcn.h>
#include <exception>
#include <system_error>
#include <thread>
namespace {
struct RcclApi {
    typedef struct { char internal[UZL_RCCL_UNIQUE_ID_BYTES]; } UniqueId;     // ncclUniqueId (rccl.h:43)
    typedef void* Comm;                                                        // ncclComm_t
    int (*GetUniqueId)(UniqueId*) = nullptr;                                   // ncclResult_t: 0 = ncclSuccess
    int (*CommInitRank)(Comm*, int, UniqueId, int) = nullptr;
    int (*CommDestroy)(Comm) = nullptr;
    int (*CommCount)(Comm, int*) = nullptr;
    int (*AllReduce)(const void*, void*, size_t, int, int, Comm, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    static constexpr int kDouble = 8, kSum = 0;                                // ncclDouble (rccl.h:467), ncclSum (rccl.h:448)
    bool ok = false;
    std::string error;
};
RcclApi& rccl()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* so = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!so) so = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!so) { api.error = std::string("dlopen(librccl.so) failed: ") + dlerror(); return; }
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(so, "ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(so, "ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(so, "ncclCommDestroy"));
        api.CommCount = reinterpret_cast<decltype(api.CommCount)>(dlsym(so, "ncclCommCount"));
        api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(so, "ncclAllReduce"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(so, "ncclGetErrorString"));
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllReduce;
        if (!api.ok) api.error = "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllReduce";
    });
    return api;
}

struct Timed {
    uzl_pgo* h;
    Timed(uzl_pgo* h_, const char* name) : h(h_) { h->timer.begin(name, h->stream); }
    ~Timed() { h->timer.end(h->stream); }
};

// Device scalars -> host.  A one-workgroup kernel at the end of the queued work writes them straight into pinned
// coherent host memory and bumps a sequence word; the host spins on that word (bounded, then falls back to a stream
// synchronise so that a failed launch surfaces as an error instead of a hang).
void fetch_scal(uzl_pgo* h)
{
    const uint32_t seq = ++h->pub_seq;
    k_publish(h->D, h->d_pub, seq, h->stream);
    volatile PgoHostScal* pub = h->h_scal.p;
    const auto t0 = std::chrono::steady_clock::now();
    bool seen = false;
    for (int spin = 0; !seen; spin++) {
        seen = __atomic_load_n(&h->h_scal.p->seq, __ATOMIC_ACQUIRE) == seq;
        if (!seen && (spin & 1023) == 1023 &&
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > 50.0) break;
    }
    (void)pub;
    if (!seen || h->timer.on) {
        UZL_HIP(hipStreamSynchronize(h->stream));
        if (__atomic_load_n(&h->h_scal.p->seq, __ATOMIC_ACQUIRE) != seq) throw HipError{hipErrorUnknown, "publish_kernel did not run", __FILE__, __LINE__};
    }
    h->timer.resolve();
}

// When a linear solve stops.  What the parity bar constrains is the pose, i.e. the error e = dx - dx* of each LM step in metres and
// radians - not a residual norm: a relative residual test solves a 1e-7 m step of a converged LM iteration to the same twelve digits
// as the metre-sized first one (config 5's last solve spent 5000 of its 6660 PCG iterations on steps below 1e-6 m), and on badly
// conditioned graphs it still lets too much error through in the soft modes (round 2 carried two corrective heuristics for that:
// a 10x tighter tolerance while chi2 still moved, and a tolerance shrinking with the previous solve's iteration count).  Both are
// replaced by an a-posteriori estimate of e itself, taken every kProgressEvery iterations from how far x still moves (progress_decide_ml,
// pgo_device.hpp: inside the iteration kernels), against an absolute target derived from cfg.pcg_tol:
//     largest translation component of e  <=  kStepT * pcg_tol  [m]      (default 1e-5: 1e-5 m   = 1/100 of the 1e-3 m bar per LM step)
//     largest rotation component of e     <=  kStepR * pcg_tol  [q_xyz]  (default       1e-6     ~ 2e-6 rad = 1/50 of the 1e-4 rad bar)
// LM is self-correcting, so the per-step errors do not add up coherently; twenty of them stay an order of magnitude inside the bar.
// The relative test on r.M^-1 r remains as a floor two orders below pcg_tol (kTolFloor2 on its square): it ends solves whose target is
// below what the arithmetic can settle.
// (kStepT, kStepR, kTolFloor2: pgo_lm.hpp)
constexpr int kProgressEveryBJ = 8;           // block-Jacobi path: PCG iterations between two looks (a launch of their own; the multilevel path looks every
                                              // kProgressEvery iterations inside its kernels, pgo_types.hpp)
// How stale is a kept preconditioner?  Not the iteration count of the last solve (with an absolute stop test that follows the size of
// the LM step and lambda, not the operator): the CONTRACTION it delivers, nats of r.M^-1 r per PCG iteration.  rz_stop = scal[1] is
// pcg_tol^2 * tol_f2 * (r_0.M^-1 r_0).  A rebuild is due when the rate has fallen below kRateDrop of what the operator delivered when fresh.
// (kRateDrop and the rule: pgo_lm.hpp)
}  // namespace

void uzl::set_lambda(uzl_pgo* h, double lambda, double tol_f2)
{
    k_set_trial(h->D.scal, lambda, tol_f2, pgo_eps_t(h->cfg), pgo_eps_r(h->cfg), h->stream);
}

namespace {
// exchange step of the sharded solve: sum `count` doubles at dev_ptr over all ranks (caller-supplied RCCL all-reduce)
void shard_allreduce(uzl_pgo* h, double* ptr, int64_t count)
{
    if (!h->sharded || count <= 0) return;
    const auto t0 = std::chrono::steady_clock::now();
    // native: stream-ordered between the producing and the consuming kernel, the host does not wait
    const int rc = h->rccl_comm ? rccl().AllReduce(ptr, ptr, (size_t)count, RcclApi::kDouble, RcclApi::kSum, h->rccl_comm, h->stream)
                                : h->allreduce(ptr, count, (void*)h->stream, h->allreduce_user);
    h->exchange_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    h->exchange_calls++;
    if (rc != 0) throw HipError{hipErrorUnknown, h->rccl_comm ? "ncclAllReduce failed" : "all-reduce callback failed", __FILE__, __LINE__};
}
// chi2 is a sum over edges: partial per rank
void shard_allreduce_chi2(uzl_pgo* h)
{
    if (!h->sharded) return;
    h->d_red.reserve(2);
    UZL_HIP(hipMemcpyAsync(h->d_red.p, h->D.scal + 4, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    shard_allreduce(h, h->d_red.p, 1);
    UZL_HIP(hipMemcpyAsync(h->D.scal + 4, h->d_red.p, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
}

// allocate everything that depends on (n, e) only
void alloc_problem(uzl_pgo* h, bool keep_poses = false)
{
    const size_t n = std::max(h->n, 1), e = std::max(h->e, 1);
    const bool cur_b = keep_poses && h->cur != nullptr && h->cur == h->pose_b.p;       // (the estimate sits in whichever buffer the last solve left it)
    h->pose_a.reserve(n * 8, keep_poses, h->stream); h->pose_b.reserve(n * 8, keep_poses, h->stream); h->pose_init.reserve(n * 8);
    h->d_zinv.reserve(e * 7); h->d_info.reserve(e * 36); h->d_robust.reserve(e);
    h->d_ei.reserve(e); h->d_ej.reserve(e);
    h->d_v2b.reserve(n);
    h->d_part_a.reserve(kMaxPartials); h->d_part_b.reserve(kMaxPartials); h->d_part_c.reserve(2 * kMaxPartials);     // (part_c: two maxima per ml_cg workgroup at a look)
    h->d_scal.reserve(16); h->d_flags.reserve(4);
    h->h_scal.reserve(1, hipHostMallocMapped | hipHostMallocCoherent); h->h_lambda.reserve(1);
    memset(h->h_scal.p, 0, sizeof(PgoHostScal));
    UZL_HIP(hipHostGetDevicePointer((void**)&h->d_pub, h->h_scal.p, 0));
    h->cur = cur_b ? h->pose_b.p : h->pose_a.p; h->trial = cur_b ? h->pose_a.p : h->pose_b.p;
}

// the system edges of uzl_pgo::in_edges (flatten_edges, pgo_structure.hpp: the skip rules of addGraphImpl)
void flatten_edges(uzl_pgo* h)
{
    FlatEdges F = uzl::flatten_edges(h->n, h->in_edges, h->fixed_in);
    h->ij.swap(F.ij); h->src.swap(F.src); h->robust.swap(F.robust); h->edge_w.swap(F.edge_w);
    h->e = (int32_t)h->src.size();
}
InEdge in_edge_of(const uzl_edge& ed)
{
    double tr = 0.; for (int r = 0; r < 6; r++) tr += ed.information[r * 7];
    return {ed.from, ed.to, (uint8_t)(ed.type == UZL_EDGE_TYPE_2D_WHEEL_ODOMETRY ? 1 : 0), (uint8_t)(ed.valid ? 1 : 0), tr};
}

void upload_edges_common(uzl_pgo* h)
{
    hipStream_t s = h->stream;
    const int e = h->e;
    h->srec_stale = true;               // (values, not structure: the slot records follow in prepare_optimize, also when the structure is kept)
    if (e > 0) {
        std::vector<int32_t> ei((size_t)e), ej((size_t)e);
        for (int k = 0; k < e; k++) { ei[k] = h->ij[2 * k]; ej[k] = h->ij[2 * k + 1]; }
        UZL_HIP(hipMemcpyAsync(h->d_ei.p, ei.data(), sizeof(int32_t) * e, hipMemcpyHostToDevice, s));
        UZL_HIP(hipMemcpyAsync(h->d_ej.p, ej.data(), sizeof(int32_t) * e, hipMemcpyHostToDevice, s));
        UZL_HIP(hipMemcpyAsync(h->d_robust.p, h->robust.data(), (size_t)e, hipMemcpyHostToDevice, s));
        UZL_HIP(hipStreamSynchronize(s));   // ei/ej are stack vectors
    }
}

// The hierarchy a plan describes (pgo_ml_plan.hpp), on the device: one arena holding both hierarchy copies, the two MlDev / MlHot
// descriptors, one staged copy of the index arrays.  Reads the plan and decides nothing.
// (d_*: the block system the PCG solves - the full one or the Schur-reduced one)
void upload_ml(uzl_pgo* h, const MlPlan& P, const int32_t* d_row_ptr, const int32_t* d_col, double* d_blk, double* d_hdiag)
{
    const int L = P.levels, cl = P.cl;
    if (L == 0) return;
    const std::vector<MlPlan::Level>& lv = P.lv;
    // ---- one arena for everything: first the int arrays (staged on the host), then the doubles
    size_t bytes = 0;
    auto take = [&](size_t b) { size_t o = bytes; bytes = (bytes + b + 255) / 256 * 256; return o; };
    enum { iRowPtr, iCol, iSrow, iOffPtr, iDiagPtr, iCslot, iChunk, kIdx };
    static constexpr std::vector<int32_t> MlPlan::Level::* idx[kIdx] = {&MlPlan::Level::row_ptr, &MlPlan::Level::col, &MlPlan::Level::srow, &MlPlan::Level::off_ptr,
                                                                        &MlPlan::Level::diag_ptr, &MlPlan::Level::cslot, &MlPlan::Level::chunk};
    std::vector<std::array<size_t, kIdx>> io((size_t)L + 1);
    for (int l = 0; l <= L; l++) for (int k = 0; k < kIdx; k++) io[l][k] = take(std::max<size_t>((lv[l].*idx[k]).size(), 1) * 4);
    const size_t int_bytes = bytes;
    struct DblOff { size_t blk, G, M, Winv, geo, cen, r, y; };
    std::vector<DblOff> dof((size_t)L + 1);
    for (int l = 0; l <= L; l++) {
        const size_t n = (size_t)std::max(P.n[l], 1), ns = (size_t)std::max(P.nslots[l], 1);
        dof[l].blk = (l == 0) ? 0 : take(ns * 36 * 8);
        dof[l].G = (l == 0) ? 0 : take(n * 36 * 8);
        dof[l].M = (l == 0) ? 0 : take(n * 36 * 8);
        dof[l].Winv = (l < L) ? take((size_t)std::max(P.n[l + 1], 1) * (size_t)(36 * P.fan[l + 1] * P.fan[l + 1]) * 8) : 0;
        dof[l].geo = (l == 0) ? take(n * 12 * 8) : 0;          // levels >= 1: one contiguous blob (geo_blob below)
        dof[l].cen = take(n * 4 * 8);
        dof[l].r = take(n * 6 * 8);
        dof[l].y = take(n * 6 * 8);
    }
    size_t geo_blob_doubles = 0;
    std::vector<size_t> geo_sub((size_t)L + 1, 0);
    for (int l = 1; l <= L; l++) { geo_sub[l] = geo_blob_doubles; geo_blob_doubles += (size_t)std::max(P.n[l], 1) * 3; }
    const size_t o_geo_blob = take(geo_blob_doubles * 8 + 64);     // ml_cg copies levels g..L-1 with one linear loop
    std::vector<size_t> o_dense((size_t)L + 1, 0);
    if (cl) for (int l = cl; l < L; l++) o_dense[l] = take((size_t)(6 * P.n[l]) * (size_t)(6 * P.n[l]) * 8);
    const size_t n12 = P.mult ? (size_t)P.n[cl] * P.n[cl + 1] * 36 * 8 : 0;
    const size_t o_mQ = take(n12), o_mQY = take(n12);
    const size_t nsq = P.mult ? (size_t)(6 * P.n[cl]) * (size_t)(6 * P.n[cl]) * 8 : 0;     // also the scratch of the levels above cl
    const size_t o_nsT = take(nsq), o_nsX = take(nsq);
    const int c32_stride = cl ? ((6 * P.n[cl] + 3) & ~3) : 0;
    const size_t o_c32 = take(cl ? (size_t)(6 * P.n[cl]) * c32_stride * 4 + 16384 : 0);      // f32 copy of Y_cl: what the PCG kernels read (+ slack: ml_cg_lm_kernel<4, true, true, ...> prefetches 18 x 512 B per row unconditionally)
    std::vector<size_t> o_grp((size_t)L + 1, 0);
    if (P.mult) for (int l = cl; l < L; l++) o_grp[l] = take(lv[l].grp.size() * 4);
    const size_t o_top = take((size_t)(6 * kMlTopWide) * (6 * kMlTopWide) * 8);
    const size_t ngz = (size_t)std::max(P.n[P.gather_level], 1) * 6 * 8 * 2;          // (x 2: the gather-level-2 Sg holds two parts per entity)
    const size_t o_sg = take(ngz), o_rga = take(ngz), o_rgb = take(ngz), o_vg = take(ngz);
    const size_t buf_bytes = (bytes + 255) / 256 * 256;
    h->ml_arena.reserve(2 * buf_bytes);
    h->ml_copy_stride = buf_bytes;
    std::vector<uint8_t> stage(int_bytes, 0);
    for (int l = 0; l <= L; l++)
        for (int k = 0; k < kIdx; k++) { const std::vector<int32_t>& v = lv[l].*idx[k]; if (!v.empty()) memcpy(stage.data() + io[l][k], v.data(), v.size() * 4); }
    hipStream_t s = h->stream;
    h->d_ml.reserve(2);
    h->d_scal2.reserve(16);
    MlDev Mh[2];
    for (int bi = 0; bi < 2; bi++) {
        uint8_t* base = h->ml_arena.p + (size_t)bi * buf_bytes;
        UZL_HIP(hipMemsetAsync(base, 0, bytes, s));            // padding between arrays takes part in the sharded all-reduce
        UZL_HIP(hipMemcpyAsync(base, stage.data(), int_bytes, hipMemcpyHostToDevice, s));
        MlDev& M = Mh[bi];
        memset(&M, 0, sizeof(M));
        M.levels = L;
        for (int l = 0; l <= L; l++) {
            MlLevel& X = M.lv[l];
            X.n = P.n[l]; X.nslots = P.nslots[l];
            X.fan = P.fan[l];
            X.span = 1; for (int q = 1; q <= l; q++) X.span *= P.fan[q];
            auto ints = [&](int k) { return reinterpret_cast<const int32_t*>(base + io[l][k]); };
            X.row_ptr = (l == 0) ? d_row_ptr : ints(iRowPtr);
            X.col = (l == 0) ? d_col : ints(iCol);
            X.srow = ints(iSrow); X.off_ptr = ints(iOffPtr); X.diag_ptr = ints(iDiagPtr); X.cslot = ints(iCslot); X.chunk = ints(iChunk);
            X.n_off_contrib = lv[l].n_off;
            X.n_chunks = P.chunks[l];
            X.blk = (l == 0) ? d_blk : reinterpret_cast<double*>(base + dof[l].blk);
            X.G = (l == 0) ? d_hdiag : reinterpret_cast<double*>(base + dof[l].G);
            X.M = (l == 0) ? nullptr : reinterpret_cast<double*>(base + dof[l].M);
            X.Winv = (l < L) ? reinterpret_cast<double*>(base + dof[l].Winv) : nullptr;
            X.geo = (l == 0) ? reinterpret_cast<double*>(base + dof[l].geo) : reinterpret_cast<double*>(base + o_geo_blob) + geo_sub[l];
            X.cen = reinterpret_cast<double*>(base + dof[l].cen);
            X.r = reinterpret_cast<double*>(base + dof[l].r);
            X.y = reinterpret_cast<double*>(base + dof[l].y);
        }
        M.top_inv = reinterpret_cast<double*>(base + o_top);
        for (int l = 1; l < L; l++) M.Ydense[l] = (cl && l >= cl) ? reinterpret_cast<double*>(base + o_dense[l]) : nullptr;
        for (int l = 0; l <= kMlMaxLevels; l++) h->ml_dense_ptr[bi][l] = (l >= 1 && l < L) ? M.Ydense[l] : nullptr;
        M.comp_level = cl;
        if (P.mult) {
            for (int l = cl; l < L; l++) {
                UZL_HIP(hipMemcpyAsync(base + o_grp[l], lv[l].grp.data(), lv[l].grp.size() * 4, hipMemcpyHostToDevice, s));
                M.grp_beg[l] = reinterpret_cast<const int32_t*>(base + o_grp[l]);
                M.grp_end[l] = M.grp_beg[l] + (size_t)P.n[l] * P.n[l + 1];
            }
        }
        M.nsT = reinterpret_cast<double*>(base + o_nsT); M.nsX = reinterpret_cast<double*>(base + o_nsX);
        M.mQ = reinterpret_cast<double*>(base + o_mQ); M.mQY = reinterpret_cast<double*>(base + o_mQY);
        M.Sg = reinterpret_cast<double*>(base + o_sg);
        uzl_pgo::MlBuf& B = h->mlb[bi];
        B.dml = h->d_ml.p + bi;
        B.nsT = M.nsT; B.nsX = M.nsX; B.y1 = cl ? M.Ydense[cl] : nullptr;
        B.rg[0] = reinterpret_cast<double*>(base + o_rga);
        B.rg[1] = reinterpret_cast<double*>(base + o_rgb);
        MlHot& Hh = B.hot;
        memset(&Hh, 0, sizeof(Hh));
        Hh.levels = L;
        for (int l = 0; l <= L; l++) { Hh.n[l] = P.n[l]; Hh.fan[l] = P.fan[l]; Hh.geo[l] = M.lv[l].geo; Hh.Winv[l] = M.lv[l].Winv; }
        Hh.geo0 = M.lv[0].geo; Hh.top_inv = M.top_inv; Hh.Sg = M.Sg; Hh.Vg = reinterpret_cast<double*>(base + o_vg);
        Hh.Cmat = cl ? ((P.ns_steps & 1) ? M.nsX : M.Ydense[cl]) : nullptr;   // Newton-Schulz steps ping-pong Y_cl <-> nsX
        Hh.Cmat32 = cl ? reinterpret_cast<const float*>(base + o_c32) : nullptr;
        Hh.c32_stride = c32_stride;
        B.l1_span_ptr = M.lv[1].blk;
        h->l1_span = (int64_t)((M.lv[1].M + (size_t)std::max(P.n[1], 1) * 36) - M.lv[1].blk);
    }
    h->ml_ix = 0;
    UZL_HIP(hipMemcpyAsync(h->d_ml.p, Mh, sizeof(Mh), hipMemcpyHostToDevice, s));
    UZL_HIP(hipStreamSynchronize(s));      // stage / Mh are locals
}

}  // namespace

// the slot twins' slot for this handle: its slot (the handle's own flags; rebuilt with the structure - the additive fallback bumps
// structure_gen when it swaps hot.Cmat), the hierarchy copy in use, the pose buffer of the current estimate and pcg_tol^2.  Launch
// geometry: h->ml_shape
HostSlot uzl::host_slot(uzl_pgo* h)
{
    if (h->ml_slot_gen != h->structure_gen) {
        h->ml_slot = make_slot(h, nullptr, nullptr);
        h->ml_shape = make_shape({h}, 1, false);
        h->ml_slot_gen = h->structure_gen;
    }
    HostSlot hs;
    hs.S = h->ml_slot; hs.ix = h->ml_ix; hs.cur = h->cur == h->pose_b.p ? 1 : 0; hs.tol2 = h->cfg.pcg_tol * h->cfg.pcg_tol;
    return hs;
}
// numeric part of the set-up of hierarchy copy hs.ix; a sharded solve all-reduces level 1 on the way (levels >= 2 need no exchange)
void uzl::ml_setup_numeric(uzl_pgo* h, const HostSlot& hs, hipStream_t s, KernelTimer* timer)
{
    kl_ml_numeric(hs, h->ml_shape, s, timer, [&] { shard_allreduce(h, h->mlb[hs.ix].l1_span_ptr, h->l1_span); });
}

namespace {
// enqueue `pairs` x 2 PCG iterations (p0 -> p1 -> p0); kernels no-op once the device `done` flag is set
void enqueue_pcg_pairs(uzl_pgo* h, int pairs, bool timed)
{
    hipStream_t s = h->stream;
    const PgoDev& D = h->Dp;
    const double tol2 = h->cfg.pcg_tol * h->cfg.pcg_tol;
    const bool ml = h->mlp.levels > 0;
    const HostSlot hs = ml ? host_slot(h) : HostSlot{};
    const int ga = g_pcg_spmv(D.nb), gu = g_pcg_update(D.nb);                     // block-Jacobi: partials written by spmv / by update
    double* pb[2] = {h->pbuf[0], h->pbuf[1]};
    auto progress = [&]() {                                                         // how far is x from settled: the stop test (pgo_kernels.hip)
        if (timed) h->timer.begin("pcg_progress", s);
        k_pcg_progress(D, s);
        if (timed) h->timer.end(s);
    };
    for (int i = 0; i < 2 * pairs; i++) {
        if (!ml && i > 0 && i % kProgressEveryBJ == 0) progress();
        double* po = pb[i & 1];
        double* pn = pb[(i & 1) ^ 1];
        hipEvent_t ea = nullptr, eb = nullptr;
        if (ml) {
            if (timed) h->timer.pair("pcg_spmv", &ea, &eb);                      // dispatch timestamps: agree with rocprofv3
            kl_ml_spmv(hs, h->ml_shape, i & 1, s, ea, eb);
            shard_allreduce(h, D.ap, h->iter_span);                              // the one exchange per PCG iteration
            ea = eb = nullptr;
            if (timed) h->timer.pair("ml_cg", &ea, &eb);
            UZL_HIP(kl_ml_cg(hs, h->ml_shape, i & 1, 0, s, ea, eb));
        } else {
            if (timed) h->timer.begin("pcg_spmv", s);
            k_pcg_spmv(D, po, pn, gu, tol2, s);
            if (timed) h->timer.end(s);
            if (timed) h->timer.begin("pcg_update", s);
            k_pcg_update(D, pn, ga, s);
            if (timed) h->timer.end(s);
        }
    }
    if (!ml) progress();
}

// |r|^2 / |b|^2 a solve under the multiplicative operator must reach.  Deliberately loose: legitimate solves end at 1e-10 .. 1e-6 while
// the linearisation moves and at ~1e-3 once LM has converged and b itself is rounding noise (a 1e-4 guard tripped there and threw a
// healthy operator away); an operator that is not SPD leaves |r| of the order of |b| or above.
// (kResidualGuard = 0.25: pgo_lm.hpp)

// The launch-bound inner loop is captured once per problem structure and preconditioner copy: every kernel argument (pointers,
// partial counts, tolerance) is fixed, lambda and the CG scalars live in device memory.  Two lengths: 2 x kGraphPairs iterations,
// and 2 x kShortPairs for solves expected to end at once (a launch behind convergence is a no-op, but still ~1.2 us of stream time:
// a converged LM iteration's solve of 2 - 4 iterations used to pay for 28 of them).
void ensure_pcg_graph(uzl_pgo* h)
{
    uzl_pgo::MlBuf& B = h->mlb[h->ml_ix];
    if (B.graph_exec) return;
    const auto t0 = std::chrono::steady_clock::now();
    UZL_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    enqueue_pcg_pairs(h, kGraphPairs, false);
    UZL_HIP(hipStreamEndCapture(h->stream, &B.graph));
    UZL_HIP(hipGraphInstantiate(&B.graph_exec, B.graph, nullptr, nullptr, 0));
    UZL_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    enqueue_pcg_pairs(h, kShortPairs, false);
    UZL_HIP(hipStreamEndCapture(h->stream, &B.graph_s));
    UZL_HIP(hipGraphInstantiate(&B.graph_exec_s, B.graph_s, nullptr, nullptr, 0));
    if (h->cfg.verbose) fprintf(stderr, "[uzl_pgo] structure: %-28s %.3f ms\n", "PCG graphs of one copy", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    h->structure_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// One (H + lambda I) dx = b solve of the trial the host-driven loop's state `lm` is in: the trial part of the set-up of copy lm.ix first
// when the state stamps it for this pass (trial_pass == pass), PCG batches up to lm.max_it, the residual guard's ratio.  Leaves the
// PCG's done / iterations / breakdown words in lm.flags and returns lm_solve_verdict over them (pgo_lm.hpp; 0: converged).
int uzl::pcg_solve(uzl_pgo* h, LmDev& lm)
{
    hipStream_t s = h->stream;
    const PgoDev& D = h->Dp;
    lm.flags[0] = 1; lm.flags[1] = 0; lm.flags[2] = 0; lm.flags[3] = 0;
    if (D.nb == 0) { h->prev_pcg_iters = 0; h->last_residual_ratio = 0.; return kLmSolved; }     // every free vertex was Schur-eliminated: nothing left to iterate on
    const int max_it = lm.max_it;
    const bool timed = h->timer.on || h->no_graph || h->sharded;   // per-kernel events, rocprofv3 and the exchange callback need eager launches
    if (h->mlp.levels > 0) {
        const HostSlot hs = host_slot(h);
        if (lm.trial_pass == lm.pass) kl_ml_trial(hs, h->ml_shape, ml_ns_steps_at(h->ml_ns_steps, lm.it), s, &h->timer);
        { Timed t(h, "pcg_init"); kl_ml_pcg_init(hs, h->ml_shape, s); }
        { Timed t(h, "ml_cg"); UZL_HIP(kl_ml_cg(hs, h->ml_shape, 0, 1, s)); }
    } else {
        { Timed t(h, "precond"); k_precond(D, s); }
        Timed t(h, "pcg_init"); k_pcg_init(D, h->pbuf[0], h->pbuf[1], s);
    }
    if (!timed) ensure_pcg_graph(h);
    int launched = 0;
    // batches sized by lm_host_batch (pgo_lm_pass.hpp), a look after each; the kernels no-op once `done` is set
    for (int round = 0;; round++) {
        const int want = lm_host_batch(round, h->prev_pcg_iters, max_it, launched);
        if (timed) enqueue_pcg_pairs(h, want / 2, h->timer.on);
        else {
            for (int i = 0; i < want / kPcgLong; i++) UZL_HIP(hipGraphLaunch(h->mlb[h->ml_ix].graph_exec, s));
            for (int i = 0; i < (want % kPcgLong + kPcgStep - 1) / kPcgStep; i++) UZL_HIP(hipGraphLaunch(h->mlb[h->ml_ix].graph_exec_s, s));
        }
        launched += want;
        k_residual_guard(D, s);                                   // a no-op until `done` is set
        fetch_scal(h);
        if (h->h_scal.p->flags[0] || launched >= max_it) break;
    }
    UZL_HIP(hipGetLastError());
    for (int i = 0; i < 4; i++) lm.flags[i] = h->h_scal.p->flags[i];
    // The multiplicative cycle / Newton-Schulz operator is not SPD by construction (see the fallback in do_optimize_host).  The
    // recurrence residual r is the true residual of x whatever the preconditioner did, so a solve under that operator which
    // claims convergence in the M^-1 norm while |r| has not come down by kResidualGuard relative to |b| is refused (lm.guarded) and the
    // caller falls back to the additive operator (a sum of SPD terms, whose M^-1 norm is a norm).
    h->last_residual_ratio = h->h_scal.p->scal[7];
    const int verdict = lm_solve_verdict(&lm, h->last_residual_ratio);
    if (verdict == kLmAnomalyGuard) h->guard_trips++;
    h->prev_pcg_iters = lm.flags[1];
    return verdict;
}


namespace uzl {
const int kUpperNs = 4;                   // Newton-Schulz steps of the dense levels above the composite level (even: the result ends in Ydense[l])
// the rate rule where the rebuild is synchronous: with the dense operator of that class a rebuild pays as soon as the rate has fallen to
// 0.75 of the fresh one (0.6 elsewhere; -3 ... -8 % on eight of nine such shapes, the 30k / 150k graph - no dense operator - +14 %)
constexpr double kRateDropSyncDense = 0.75;
// (ml_ns_steps_at, the Newton-Schulz steps of a synchronous set-up at an LM iteration: pgo_lm_pass.hpp)
double ml_rate_drop(const uzl_pgo* h) { return (!ml_async_level(h) && h->mlp.cl > 0) ? kRateDropSyncDense : kRateDrop; }

// Asynchronous rebuild (second stream, second copy of the hierarchy) pays on the composite level-1 path, and for the reduced system of a
// chain-like graph on the level-2 path: there a rebuild (0.8 ms) is as long as the LM iteration it would otherwise hold up.  (Other
// level-2 graphs - config 4 - measured +9 % PCG iterations for no net gain.)
bool ml_async_level(const uzl_pgo* h)
{
    return h->mlp.cl == 1 || (h->mlp.cl == 2 && h->red.on && h->red.strong);
}

namespace {
void upload_i32(DevBuf<int32_t>& b, const std::vector<int32_t>& v, size_t n, hipStream_t s)      // the first n of v; the buffer holds at least one
{
    b.reserve(std::max<size_t>(n, 1));
    if (n > 0) UZL_HIP(hipMemcpyAsync(b.p, v.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
}
// step 1 of build_structure: the block system of a SystemPlan on the device (Y stays alive until the stream is synchronised), bound to h->D
void upload_system(uzl_pgo* h, const SystemPlan& Y)
{
    hipStream_t s = h->stream;
    const int n = h->n, nb = Y.nb, nslots = Y.nslots;
    const size_t nsz = std::max(nslots, 1);
    h->nb = nb; h->nslots = nslots;
    h->d_srec.reserve(nsz * 44); h->d_smeta.reserve(nsz);
    h->srec_stale = true;
    static_assert(sizeof(int4) == 4 * sizeof(int32_t), "SystemPlan::smeta is the kernels' int4 per slot");
    if (nslots > 0) UZL_HIP(hipMemcpyAsync(h->d_smeta.p, Y.smeta.data(), sizeof(int4) * nslots, hipMemcpyHostToDevice, s));
    if (n > 0) UZL_HIP(hipMemcpyAsync(h->d_v2b.p, Y.v2b.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    h->sys.upload(nb, Y.row_ptr, Y.col, Y.b2v, Y.rowhdr, s);
    upload_i32(h->d_slot_edge, Y.slot_edge, (size_t)nslots, s);
    upload_i32(h->d_rb_ptr, Y.rb_ptr, Y.rb_ptr.size(), s);
    // blocks of slots whose neighbour is fixed are never written: keep them defined
    if (nslots > 0) UZL_HIP(hipMemsetAsync(h->sys.blk.p, 0, sizeof(double) * 36 * (size_t)nslots, s));      // (and slots of edges other ranks own stay 0)
    UZL_HIP(hipStreamSynchronize(s));
    PgoDev& D = h->D;
    D.n = n; D.e = h->e;
    h->sys.bind(D, nb, nslots);
    D.pose = h->cur; D.pose_trial = h->trial;
    D.v2b = h->d_v2b.p; D.ei = h->d_ei.p; D.ej = h->d_ej.p;
    D.zinv = h->d_zinv.p; D.info = h->d_info.p; D.robust = h->d_robust.p;
    D.rb_ptr = h->d_rb_ptr.p; D.n_rb = (int32_t)Y.rb_ptr.size() - 1; D.pad_rb = 0; D.srec = h->d_srec.p; D.smeta = h->d_smeta.p;
    D.part_b = h->d_part_b.p; D.part_c = h->d_part_c.p;
    D.scal = h->d_scal.p; D.flags = h->d_flags.p;
    D.e_begin = 0; D.e_end = h->e; D.diag_owner = 1; D.sibling0 = 1;      // sibling0 finalised once the hierarchy is planned
}
// step 2: an adopted SchurPlan on the device, the reduced system bound to h->Dp (rb2v: its rows as vertices)
void upload_schur(uzl_pgo* h, const SchurPlan& P, const std::vector<int32_t>& rb2v, bool may_shard)
{
    hipStream_t s = h->stream;
    uzl_pgo::Reduced& Rd = h->red;
    Rd.on = true; Rd.n_int = P.n_int; Rd.n_runs = P.n_runs; Rd.longest_run = P.longest_run; Rd.strong = P.strong; Rd.strong_blocks = P.strong && P.n_strong2 > 0; Rd.n_sep = P.n_sep;
    const size_t ni = (size_t)P.n_int, nru = (size_t)P.n_runs;
    const std::pair<DevBuf<int32_t>*, const std::vector<int32_t>*> idx[] = {{&Rd.run_ptr, &P.run_ptr}, {&Rd.run_rows, &P.run_rows}, {&Rd.slotP, &P.slotP}, {&Rd.slotN, &P.slotN},
                                                                             {&Rd.endL, &P.endL}, {&Rd.endR, &P.endR}, {&Rd.sep_rows, &P.sep_rows}, {&Rd.rsrc, &P.rsrc},
                                                                             {&Rd.inc_ptr, &P.inc_ptr}, {&Rd.inc, &P.inc}};
    for (const auto& bv : idx) upload_i32(*bv.first, *bv.second, bv.second->size(), s);
    const std::vector<int32_t> rhdr = row_headers(P.nbr, P.row_ptr, P.col);
    Rd.sys.upload(P.nbr, P.row_ptr, P.col, rb2v, rhdr, s);
    Rd.elim.reserve(std::max<size_t>(ni, 1) * kSchurElim); Rd.runout.reserve(std::max<size_t>(nru, 1) * kSchurRunOut);
    UZL_HIP(hipStreamSynchronize(s));                                  // rhdr is a local
    SchurDev& S = Rd.S;
    S.n_runs = P.n_runs; S.n_int = P.n_int; S.nbr = P.nbr; S.nslots_r = P.nslots_r;
    S.run_ptr = Rd.run_ptr.p; S.run_rows = Rd.run_rows.p; S.slotP = Rd.slotP.p; S.slotN = Rd.slotN.p; S.endL = Rd.endL.p; S.endR = Rd.endR.p;
    S.sep_rows = Rd.sep_rows.p; S.rsrc = Rd.rsrc.p; S.inc_ptr = Rd.inc_ptr.p; S.inc = Rd.inc.p; S.elim = Rd.elim.p; S.runout = Rd.runout.p;
    // Sharded solve: a run is eliminated by EVERY rank (the reduced system's diagonal blocks and right-hand side are then complete
    // everywhere, like H_aa | b after its all-reduce), so each needs the run's chain blocks whole - one more all-reduce per
    // linearisation, [E_m per eliminated vertex | C_1 per run] gathered into a contiguous buffer.  Fill blocks enter A p on rank 0 only.
    S.runblk = nullptr;
    if (may_shard) { Rd.runblk.reserve((ni + nru) * 36); S.runblk = Rd.runblk.p; }
    h->Dp = h->D;
    Rd.sys.bind(h->Dp, P.nbr, P.nslots_r);
    h->Dp.smeta = nullptr; h->Dp.srec = nullptr;                      // the reduced system is assembled by schur_assemble_kernel
}
}  // namespace

// The structure of a graph in the three steps of DESIGN.md section 6, each "plan (a host-side value: pgo_structure.hpp, pgo_schur.hpp,
// pgo_ml_plan.hpp) -> upload -> bind": the block system over the free vertices, the Schur reduction of the chain interiors, the hierarchy
void build_structure(uzl_pgo* h)
{
    auto t_prev = std::chrono::steady_clock::now();
    auto tick = [&](const char* what) {                       // UZL_VERBOSE: where the host side of a new structure spends its time
        if (!h->cfg.verbose) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[uzl_pgo] structure: %-28s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - t_prev).count());
        t_prev = t;
    };
    destroy_pcg_graph(h);
    tick("drop the captured graphs");
    // ---- 1. the block system over the free vertices
    std::vector<int32_t> order = aggregation_order(h->n, h->ij, h->fixed_eff, h->edge_w);
    tick("aggregation order");
    const SystemPlan Y = system_plan(h->n, h->ij, h->robust, std::move(order));
    upload_system(h, Y);
    PgoDev& D = h->D;
    PgoDev& Dp = h->Dp;
    // ---- 2. Schur reduction of the chain interiors (pgo_schur.hpp): when a third or more of the free vertices carry nothing but their two
    //      chain edges, the PCG runs on the Schur complement over the others (sharded solves included: see SchurDev::runblk).
    uzl_pgo::Reduced& Rd = h->red;
    Rd.on = false; Rd.n_int = 0; Rd.n_runs = 0; Rd.longest_run = 0; Rd.strong = false; Rd.strong_blocks = false; Rd.n_sep = 0;
    // longest run: 24.  (Twelve for small graphs paid 3 - 8 % while one wave walked a whole run; with a run eliminated from both ends the
    // chain is twelve steps anyway, and stars of 20-vertex arms keep being eliminated completely: tests/test_schur_gpu.py.)
    constexpr int kSchurCap = 24;
    constexpr int kStrongThetaPct = 25;                                      // groups hang together by edges >= 0.25 x the stiffest at either end
    const bool may_shard = h->allreduce != nullptr || h->rccl_comm != nullptr;
    SchurPlan P;
    if (h->cfg.schur_reduce >= 0 && Y.nb > 0) {
        tick("block-CSR + uploads");
        const ReducedNumbering num = reduced_numbering(h->cfg.reduced_numbering, h->cfg.preconditioner, may_shard, h->num_its);
        const std::vector<double> slot_w = (num.strong_min > 0 && h->edge_w.size() == (size_t)h->e) ? slot_weights(Y, h->edge_w) : std::vector<double>();
        P = schur_plan(Y.nb, Y.row_ptr, Y.col, kSchurCap, slot_w.empty() ? nullptr : slot_w.data(), num.strong_min, 0.01 * kStrongThetaPct, num.max_contig, kSchurStrongOneMax,
                       schur_min_interiors(Y.nb));
        tick("Schur plan");
        if (schur_admitted(Y.nb, P.n_int)) upload_schur(h, P, reduced_b2v(P.sep_rows, Y.b2v), may_shard);
    }
    PgoDev& Dsys = Rd.on ? Dp : D;                                             // what the PCG kernels get
    const int nbp = Dsys.nb;
    const SysBufs& Bsys = Rd.on ? Rd.sys : h->sys;
    tick("reduced system uploads");
    // ---- 3. the hierarchy of the system the PCG solves
    {
        static const bool comp4_off = diag_flag("UZL_ML_NO_COMP4");          // the walked hierarchy instead (tests/test_ab_paths_gpu.py)
        MlPlanIn in;
        in.nb = nbp; in.nslots = Dsys.nslots;
        in.precond_on = h->cfg.preconditioner != 0; in.strong_blocks = Rd.strong_blocks; in.mult_banned = h->mult_banned; in.comp4_off = comp4_off;
        h->mlp = ml_plan(in, Rd.on ? P.row_ptr : Y.row_ptr, Rd.on ? P.col : Y.col);
        tick("hierarchy plan (host index arrays)");
        upload_ml(h, h->mlp, Dsys.row_ptr, Dsys.col, Dsys.blk, Dsys.hdiag);
        h->mlp.release_indices();
        // (a block-Jacobi structure leaves the two as the structure before it had them, as it always did: pcg_solve's residual guard reads them)
        if (h->mlp.levels > 0) { h->ml_mult = h->mlp.mult; h->ml_ns_steps = h->mlp.ns_steps; }
    }
    tick("hierarchy uploads");
    {   // per-iteration exchange buffer: [A p (6 nb) | restricted A p (6 n_g) | p.Ap partials]
        const ExchangeLayout X = exchange_layout(nbp, h->mlp);
        if (h->mlp.gather_level) { h->mlb[0].hot.Sg = Bsys.ap.p + X.sg; h->mlb[1].hot.Sg = h->mlb[0].hot.Sg; }
        Dsys.part_a = Bsys.ap.p + X.part_a;
        h->iter_span = X.iter_span;
    }
    Dsys.sibling0 = (h->mlp.levels > 0 && h->mlp.agg == 1) ? 1 : 0;     // large graphs keep the level-0 smoother block-diagonal
    D.sibling0 = Dsys.sibling0;
    // ---- sharded solve (BASELINE config 4): this rank linearises a contiguous range of the system edges
    // (a callback with world_size 1 still runs every exchange step: that is how the RCCL callback is tested on one GPU;
    //  graphs too small for the multilevel path are simply solved redundantly by every rank)
    h->sharded = h->mlp.levels > 0 && may_shard;
    if (h->sharded) {
        const ShardRange R = shard_range(h->e, h->rank, h->world);
        D.e_begin = R.e_begin; D.e_end = R.e_end; D.diag_owner = R.diag_owner;
        D.sibling0 = 0;
    }
    if (Rd.on) {                                                              // (Dp was copied from D before the rank's share was known)
        Dp.e_begin = D.e_begin; Dp.e_end = D.e_end; Dp.diag_owner = D.diag_owner; Dp.sibling0 = D.sibling0;
        Rd.S.runblk = h->sharded ? Rd.runblk.p : nullptr;
    }
    if (!Rd.on) Dp = D;
    h->pbuf[0] = Bsys.p.p; h->pbuf[1] = Bsys.p2.p;
    h->structure_ready = true;
    h->structure_gen++;
}


void destroy_pcg_graph(uzl_pgo* h)
{
    for (auto& B : h->mlb) {
        if (B.graph_exec) { (void)hipGraphExecDestroy(B.graph_exec); B.graph_exec = nullptr; }
        if (B.graph) { (void)hipGraphDestroy(B.graph); B.graph = nullptr; }
        if (B.graph_exec_s) { (void)hipGraphExecDestroy(B.graph_exec_s); B.graph_exec_s = nullptr; }
        if (B.graph_s) { (void)hipGraphDestroy(B.graph_s); B.graph_s = nullptr; }
    }
}

// initializeOptimization :139, setFixedNodes :144-146: the structure, cached until the next add_graph / set_graph
void ensure_structure(uzl_pgo* h)
{
    if (h->structure_ready) return;
    h->fixed_eff = h->fixed_in;
    h->n_gauge = gauge_fix(h->n, h->ij, h->fixed_eff);
    build_structure(h);
}
// optimizeImpl's front part
void prepare_optimize(uzl_pgo* h)
{
    h->t_start = std::chrono::steady_clock::now();
    h->structure_ms = 0.; h->exchange_ms = 0.; h->exchange_calls = 0;
    h->last_structure_reused = h->structure_ready;
    if (!h->structure_ready) {
        const auto ts = std::chrono::steady_clock::now();
        ensure_structure(h);
        h->structure_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
    }
    if (h->srec_stale) {                // the edges' values in slot order (new values on a kept structure, or a new structure)
        k_slot_records(h->d_zinv.p, h->d_info.p, h->e, h->d_slot_edge.p, h->nslots, h->d_srec.p, h->stream);
        h->srec_stale = false;
    }
}
int do_optimize(uzl_pgo* h, int32_t iterations, uzl_pgo_stats* st)
{
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "optimize before add_graph/set_graph");
    UZL_HIP(hipSetDevice(h->cfg.device));
    if (iterations <= 0) iterations = h->cfg.iterations;
    prepare_optimize(h);
    uzl_pgo_stats local;
    uzl_pgo_stats* sp = st ? st : &local;
    const int rc = lm_eligible(h) ? do_optimize_lm(h, iterations, sp) : do_optimize_host(h, iterations, sp);
    if (h->red.on && h->red.n_sep >= kSchurStrongMin && sp->lm_trials > 0 && (rc == UZL_OK || rc == UZL_ERR_NOT_CONVERGED)) {      // what the next structure's numbering goes by
        h->num_last = h->red.strong ? 1 : 0;
        h->num_its[h->num_last] = (h->red.strong_blocks ? 1.3 : 1.) * (double)sp->pcg_iterations / sp->lm_trials;      // an iteration on the padded AGG = 4 layout: 20 against 14 us, less the rebuilds it saves
    }
    return rc;
}
// The host-driven loop: the second driver of the LM state machine (pgo_lm.hpp; the first is the pair of decision kernels of
// uzl_pgo_lm.hip).  It keeps an LmDev and an image of the solve's scalars on the host, has lm_head_decide / lm_trial_decide take every
// decision on them, and reads what to launch from the state the way the slot twins do: schur_pass / numeric_pass / trial_pass /
// build_pass == pass, build_ix, scal2[3], ix, cur.  It can launch any segment at any time, so it offers the head both (kPassSetup |
// kPassRebuild) and never stalls.  Its own: the launches and round trips, the shard exchanges, the timer, the verbose lines, and the
// remedies the device-resident loop hands a graph over for.
// Called through do_optimize (structure prepared, device set), or by do_optimize_lm for a solve that met an anomaly.
int do_optimize_host(uzl_pgo* h, int32_t iterations, uzl_pgo_stats* st)
{
    const auto t0 = h->t_start;
    uzl_pgo_stats S;
    memset(&S, 0, sizeof(S));
    stats_head(h, S);
    hipStream_t s = h->stream;
    PgoDev& D = h->D;
    PgoDev& Dp = h->Dp;                       // the system the PCG solves: D, or the Schur complement over the separator vertices
    const bool red = h->red.on;
    const SchurDev& SD = h->red.S;
    const double delta = h->cfg.huber_delta;
    h->timer.reset();
    h->prev_pcg_iters = 0;
    int rc = UZL_OK;
    if (h->nb == 0 || h->e == 0) {
        // nothing to optimise: chi2 only
        if (h->e > 0) {
            int g;
            { Timed t(h, "chi2"); g = k_chi2(D, h->cur, delta, s); }
            k_finalize(D, g, 0, 0, 0, s);
            fetch_scal(h);
            S.chi2_initial = S.chi2_final = h->h_scal.p->scal[4];
        }
        S.solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (st) *st = S;
        return UZL_OK;
    }
    // optimizer_.optimize(iterations) (:148) -> OptimizationAlgorithmLevenberg::solve [EXT]
    // Asynchronous rebuild: from the second LM iteration on a wanted rebuild runs on stream2 into the OTHER copy of the
    // hierarchy while this iteration's PCG still uses the current one (any SPD preconditioner gives the same solution; one
    // that is one linearisation old costs a few iterations, a rebuild on the critical path costs ~0.4 ms).  The copy is
    // adopted at the start of the next iteration, which has to wait for it anyway before it overwrites H and the poses.
    static const bool async_off = diag_flag("UZL_ML_SYNC_REBUILD");             // diagnostic build: every rebuild synchronous (tests/test_ab_paths_gpu.py)
    // (small graphs only: at 10k vertices the rebuild's Newton-Schulz GEMMs take more from the overlapped PCG than they give back:
    // 113.2 -> 115.1 ms; config 2: 11.09 -> 10.67 ms with 540 instead of 517 PCG iterations)
    const bool async_ok = !async_off && h->mlp.levels > 0 && ml_async_level(h) && !h->sharded && !h->timer.on && h->stream2 != nullptr;
    const bool ml = h->mlp.levels > 0;
    LmDev L = lm_initial_state(h, iterations, !async_ok);
    L.cur = h->cur == h->pose_b.p ? 1 : 0;     // (the estimate sits in whichever buffer the last solve left it)
    double scal[16] = {};                      // the host's image of PgoDev::scal, as far as the decisions read and write it
    h->ml_ix = L.ix;
    struct DrainRebuild {                      // an exception must not leave a rebuild running on stream2 behind the handle's back
        uzl_pgo* h; LmDev& L;
        ~DrainRebuild() { if (L.pending) { (void)hipStreamSynchronize(h->stream2); L.pending = 0; } }
    } drain{h, L};
    PhaseMarks<4> phases;                      // diagnostic build, UZL_PHASES=1: GPU time between the marks of every LM iteration
    auto mark = [&](int tag) { phases.mark(tag, s); };
    // one solve of the trial in front of L, and what the state machine needs of it on the host: scal[0], scal[1]
    auto solve = [&]() {
        const int verdict = pcg_solve(h, L);                                      // _solver->solve()
        scal[0] = h->h_scal.p->scal[0]; scal[1] = h->h_scal.p->scal[1];
        return verdict;
    };
    // a solve that did not stand is solved again with the inverses of copy L.ix taken at this lambda; its PCG iterations stay counted
    auto solve_again = [&]() {
        L.st_pcg_iterations += L.flags[1];
        L.trial_pass = L.pass; L.lambda_setup[L.ix] = L.lambda;
        return solve();
    };
    while (L.phase != kLmDone && L.it < iterations) {
        const int phase = L.phase;                                               // kLmLin or kLmRetry: this driver never stalls, and remedies its anomalies itself
        double chi = 0., dmax = 0.;
        if (phase == kLmLin) {
            int gl, ga;
            mark(0);
            if (L.pending) UZL_HIP(hipStreamWaitEvent(s, h->ev_setup, 0));      // the copy built during the last iteration: the head adopts it
            D.pose = h->cur; D.pose_trial = h->trial;
            Dp.pose = h->cur; Dp.pose_trial = h->trial;
            // (computeActiveErrors: chi2 of the linearisation point is needed in the first iteration, and by every rank of a sharded solve,
            //  which exchanges it; later iterations carry the accepted trial's over - as lm_head_kernel does)
            {                                                                       // computeActiveErrors + buildSystem
                hipEvent_t ea = nullptr, eb = nullptr;
                h->timer.pair("linearize", &ea, &eb);                               // (profiling: dispatch timestamps, as rocprofv3 reports the kernel)
                UZL_HIP(k_hessian(D, h->cur, delta, &gl, &ga, s, L.it == 0 || h->sharded, ea, eb));
            }
            if (h->sharded) {                                                         // H_aa, b: sums over all ranks' edges
                shard_allreduce(h, h->sys.hdiag.p, (int64_t)h->nb * 42);
                ga = k_diagmax(D, s);
            }
            { Timed t(h, "finalize"); k_finalize(D, gl, 0, ga, 2, s); }
            shard_allreduce_chi2(h);
            if (red && h->sharded && SD.runblk) {           // the runs' chain blocks, summed over the ranks (once per linearisation)
                k_schur_gather(D, SD, s);
                shard_allreduce(h, SD.runblk, (int64_t)(SD.n_int + SD.n_runs) * 36);
            }
            if (L.it == 0 || h->sharded) {                  // later iterations carry chi2 over from the accepted trial: no round trip
                fetch_scal(h);
                chi = h->h_scal.p->scal[4]; dmax = h->h_scal.p->scal[6];
            }
        }
        // ---- the head: lambda_0, adoption, refresh, retake, fresh, the stamps of this trial's segments
        lm_head_decide(&L, scal, red ? 1 : 0, phase, chi, dmax, kPassSetup | kPassRebuild);
        h->ml_ix = L.ix;                                                          // (host_slot, the captured PCG graphs)
        if (phase == kLmLin && h->sharded) L.chi_cur = chi;                     // a sharded solve takes the all-reduced chi2 of every linearisation
        if (!ml) L.lambda_setup[L.ix] = 0.;                                     // block-Jacobi has no inverses to keep: every trial is fresh
        set_lambda(h, L.lambda, L.tol_f2);                                        // setLambda (+ this trial's PCG floor and step accuracy)
        if (L.schur_pass == L.pass) {                       // (H + lambda I) with the chain interiors eliminated: once per lambda (pgo_schur.hpp)
            if (phase == kLmRetry && L.pending) UZL_HIP(hipStreamWaitEvent(s, h->ev_setup, 0));   // (a rebuild running ahead on stream2 still reads the old one)
            kl_schur_reduce(host_slot(h), h->ml_shape, s, &h->timer);
        }
        if (ml && L.numeric_pass == L.pass) ml_setup_numeric(h, host_slot(h), s, &h->timer);
        if (L.build_pass == L.pass) {                       // a rebuild ahead, into the other copy, with this iteration's lambda
            UZL_HIP(hipEventRecord(h->ev_lin, s));                                // H, b and the poses of this linearisation are final
            UZL_HIP(hipStreamWaitEvent(h->stream2, h->ev_lin, 0));
            HostSlot hb = host_slot(h);
            hb.ix = L.build_ix; hb.cur = L.build_cur;
            hb.S.Dp.scal = h->d_scal2.p;                                          // the trials move scal[3] on the main stream
            k_set_scalar(hb.S.Dp.scal + 3, L.scal2[3], h->stream2);
            ml_setup_numeric(h, hb, h->stream2, nullptr);
            kl_ml_trial(hb, h->ml_shape, h->ml_ns_steps, h->stream2, nullptr);    // (a rebuild that runs ahead: the structure's steps)
            UZL_HIP(hipEventRecord(h->ev_setup, h->stream2));
        }
        if (phase == kLmLin) mark(1);
        // ---- the solve, and this driver's remedies for one that does not stand
        const int it = L.it, trial = L.qmax;
        const double lambda = L.lambda;
        int verdict = solve();
        if (verdict != kLmSolved && !L.fresh && ml) verdict = solve_again();      // stale hierarchy: retake the inverses once
        if (verdict != kLmSolved && L.guarded) {
            if (h->cfg.verbose)
                fprintf(stderr, "[uzl_pgo] it %d trial %d lambda %.3e: multiplicative operator refused (pcg %d, rz %.3e, breakdown %d, |r|2/|b|2 %.3e) -> additive\n",
                        it, trial, lambda, L.flags[1], scal[0], L.flags[2], h->last_residual_ratio);
            // The multiplicative cycle / its Newton-Schulz refinement is SPD only while the level-1 smoother contracts
            // (lambda_max(Y_1 A_1) < 2), which block-Jacobi does not guarantee on every graph: fall back, for the rest
            // of this handle's structure, to the additive operator (a sum of SPD terms) and solve again.
            if (L.pending) {                                                      // the copy being built on stream2 still holds the
                UZL_HIP(hipStreamSynchronize(h->stream2));                        // multiplicative operator: drop it and rebuild
                L.pending = 0; L.last_rel = 1e300;                                // at the next linearisation
            }
            h->ml_mult = false; h->ml_ns_steps = 0; h->mult_banned = true;       // (the additive operator takes no refinement steps)
            L.guarded = 0;
            for (auto& B : h->mlb) B.hot.Cmat = B.y1;
            destroy_pcg_graph(h);                                                 // MlHot is a by-value kernel argument
            h->structure_gen++;                                                   // (slot tables that carry it are rebuilt: uzl_pgo_lm.hip, batches)
            verdict = solve_again();
        }
        if (h->cfg.verbose)
            fprintf(stderr, "[uzl_pgo] it %d trial %d lambda %.3e pcg %d  rz_end %.3e  rz_stop %.3e  |r|2/|b|2 %.3e  conv %d  chi2 %.9g\n", it, trial, lambda, L.flags[1],
                    scal[0], scal[1], h->last_residual_ratio, (int)(verdict == kLmSolved), L.chi_cur);
        // not converged is no anomaly here: the trial is evaluated whatever the verdict, and the caller is told
        if (verdict != kLmSolved) { S.pcg_not_converged++; rc = UZL_ERR_NOT_CONVERGED; }
        mark(2);
        if (red) kl_schur_backsub(host_slot(h), h->ml_shape, s, &h->timer);      // dx of the eliminated vertices from the separators'
        int go, gc;
        { Timed t(h, "oplus"); go = k_oplus(D, h->cur, h->trial, s); }            // push + update
        { Timed t(h, "chi2"); gc = k_chi2_trial(D, h->cur, delta, s); }           // computeActiveErrors (at trial poses made on the fly: the arithmetic of the device-resident loop's eval_lm_kernel)
        { Timed t(h, "finalize"); k_finalize(D, gc, go, 0, 1, s); }
        shard_allreduce_chi2(h);
        fetch_scal(h);
        mark(3);
        // ---- the tail's decision over the evaluated trial: rho, lambda, accept / reject, what comes next
        lm_trial_decide(&L, scal, h->h_scal.p->scal[4], h->h_scal.p->scal[5]);
        h->cur = L.cur ? h->pose_b.p : h->pose_a.p; h->trial = L.cur ? h->pose_a.p : h->pose_b.p;      // an accepted step: discardTop (else pop)
    }
    lm_stats(L, S);
    if (L.pending) { UZL_HIP(hipStreamSynchronize(h->stream2)); L.pending = 0; }   // a rebuild nobody will use: let it drain
    UZL_HIP(hipStreamSynchronize(s));
    static const char* const kPhaseNames[4] = {"linearise+set-up (0->1)", "solve incl. init (1->2)", "evaluate+round trip (2->3)", "host decision / next (3->0)"};
    phases.report("phases", S.iterations_done, "LM iterations", kPhaseNames);
    S.solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    S.structure_ms = h->structure_ms; S.exchange_ms = h->exchange_ms; S.exchange_calls = h->exchange_calls;
    if (st) *st = S;
    if (rc != UZL_OK) h->last_error = "PCG hit pcg_max_iter in at least one LM trial";
    return rc;
}

// Read-only, for uzl_scope_poses_from_pgo (scope_types.hpp): the translations of the current estimates as SoA positions on stream s,
// under the solver's lock and behind whatever is still queued on the solver's stream.  Nothing of the solver changes.
int pgo_positions_to(uzl_pgo* h, int32_t device, int32_t n, double* x, double* y, double* z, hipStream_t s)
{
    std::lock_guard<std::mutex> lock(h->mu);
    if (!h->have_graph || !h->cur) return UZL_ERR_STATE;
    if (h->cfg.device != device || h->n != n) return UZL_ERR_BAD_ARG;
    if (h->stream) UZL_HIP(hipStreamSynchronize(h->stream));
    launch_scope_pgo_poses(h->cur, n, x, y, z, s);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    return UZL_OK;
}

// Read-only, for uzl_merge_poses_from_pgo (merge_types.hpp): the current estimates as n x 12 [R|t], written by the kernel uzl_pgo_store
// reads poses back with - so they are the bits a store would hand to the host - under the same lock and waits as above.
int pgo_poses12_to(uzl_pgo* h, int32_t device, int32_t n, double* out12, hipStream_t s)
{
    std::lock_guard<std::mutex> lock(h->mu);
    if (!h->have_graph || !h->cur) return UZL_ERR_STATE;
    if (h->cfg.device != device || h->n != n) return UZL_ERR_BAD_ARG;
    if (h->stream) UZL_HIP(hipStreamSynchronize(h->stream));
    k_poses_out(h->cur, n, out12, s);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    return UZL_OK;
}
}  // namespace uzl

// what the structure of a handle was built from (moved out before a new graph is read in, compared afterwards)
struct StructureKey {
    bool ready = false;
    int32_t n = 0;
    std::vector<uint8_t> fixed_in, robust;
    std::vector<int32_t> ij;
    std::vector<double> edge_w;
};
// Every graph-entry call (add_graph, append_graph, set_graph) begins here, with the node count of the graph it brings ...
// clear() (:57): the reference rebuilds everything.  Here the structure of the previous graph (gauge, block-CSR, aggregation order,
// hierarchy arrays, captured PCG graph) is kept when the new graph has the same vertices, fixed flags, system edges and edge
// weights - a timer-driven re-optimisation of an unchanged graph, or one whose poses / measurements only moved - and rebuilt
// otherwise; either way the solve is the one a fresh handle would run (same order, same operators).
static StructureKey begin_graph(uzl_pgo* h, int32_t n_new)
{
    StructureKey k;
    k.ready = h->structure_ready && h->have_graph;
    if (k.ready) {
        k.n = h->n;
        k.fixed_in.swap(h->fixed_in); k.robust.swap(h->robust); k.ij.swap(h->ij); k.edge_w.swap(h->edge_w);
    }
    // what the handle learned about the numbering of ITS reduced systems (num_its, reduced_numbering) belongs to the session it came from: a
    // graph that is not the previous one grown (fewer nodes than before) starts as on a fresh handle
    if (n_new < h->n) { h->num_its[0] = h->num_its[1] = -1.; h->num_last = -1; }
    h->have_graph = false; h->structure_ready = false;
    return k;
}
// ... and ends here, once n, fixed_in, ij, robust and edge_w describe the new graph and its values are enqueued: the start poses are
// kept for uzl_pgo_reset, the system edges' index arrays go up, the structure is kept if it is the key's, and the numbering history if the graph is the key's grown (graph_grown)
static void finish_graph(uzl_pgo* h, const StructureKey& k)
{
    if (h->n) UZL_HIP(hipMemcpyAsync(h->pose_init.p, h->cur, sizeof(double) * 8 * (size_t)h->n, hipMemcpyDeviceToDevice, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));                  // inputs are borrowed for the duration of the call only
    upload_edges_common(h);
    h->have_graph = true;
    h->structure_ready = k.ready && k.n == h->n && k.fixed_in == h->fixed_in && k.ij == h->ij && k.robust == h->robust && k.edge_w == h->edge_w;
    if (!k.ready || h->structure_ready) return;                     // nothing learned yet / the same structure again
    if (!graph_grown(k.n, k.fixed_in, k.ij, h->n, h->fixed_in, h->ij)) { h->num_its[0] = h->num_its[1] = -1.; h->num_last = -1; }
}


// A handle with a stream pair of its own from the device's pool (uzl_pgo_create), or - the graphs of a batch - on the batch's streams: a
// stream costs the runtime ~3.5 ms to make and ~2 ms to destroy (round 4's uzl_pgo_create 6.9 ms, measured: tests/diag/create_cost.py),
// which a batch of 64 graphs paid 128 times over although its solves never use its handles' streams.  A batch's handle takes a pair
// of its own the first time it is solved through uzl_pgo_optimize (own_streams).
static int pgo_create_on(const uzl_pgo_cfg* cfg, hipStream_t shared, hipStream_t shared2, uzl_pgo** out)
{
    if (!out) return UZL_ERR_BAD_ARG;
    *out = nullptr;
    uzl_pgo_cfg c;
    if (cfg) c = *cfg; else uzl_pgo_cfg_default(&c);
    if (check_device(c.device) != UZL_OK) return UZL_ERR_NO_DEVICE;
    uzl_pgo* h = new (std::nothrow) uzl_pgo();
    if (!h) return UZL_ERR_OOM;
    h->cfg = c;
    memset(&h->D, 0, sizeof(h->D));
    { const char* ng = getenv("UZL_NO_GRAPH"); h->no_graph = ng && ng[0] == '1'; }
    if (getenv("UZL_VERBOSE")) h->cfg.verbose = 1;                                    // diagnostic: per-trial PCG log on stderr
    bool ok = hipSetDevice(c.device) == hipSuccess;
    if (ok && shared) { h->stream = shared; h->stream2 = shared2; h->streams_borrowed = true; }
    else if (ok) {
        // The solver's stream and the stream its rebuilds run ahead on (at the higher priority: they overlap with the PCG they are for)
        // come from the device's pool too: a pair that shares a compute pipe costs a config-5 run a quarter of its solver time (two
        // OnlineSlam sessions in one process: 1.34 against 1.67 s of optimize, tests/diag/online_passes.py - the second session's handle
        // had taken its streams as they came).  Streams go back to the pool with the handle: making a handle no longer costs two
        // hipStreamCreates (7 ms) once the pool holds a pair.
        h->stream = stream_lease(c.device, 0, {}, false);
        h->stream2 = h->stream ? stream_lease(c.device, -1, {h->stream}, false) : nullptr;
        ok = h->stream && h->stream2;
    }
    ok = ok && hipEventCreateWithFlags(&h->ev_lin, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&h->ev_setup, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        if (!h->streams_borrowed) { stream_release(c.device, h->stream); stream_release(c.device, h->stream2); }
        if (h->ev_lin) (void)hipEventDestroy(h->ev_lin);
        if (h->ev_setup) (void)hipEventDestroy(h->ev_setup);
        delete h;
        return UZL_ERR_HIP;
    }
    *out = h;
    return UZL_OK;
}
// a batch's handle that is solved on its own: from now on with its own streams (captures and rebuild events of two such handles driven
// from two threads must not meet on one stream).  `drain_borrowed`: wait for the borrowed streams first - right for a handle that is
// taken out of an idle batch (uzl_pgo_optimize), WRONG from inside a running batch: every handle of a batch borrows launch sequence 0's
// streams, sequence 0 may be capturing on them on another thread (a synchronize fails with hipErrorStreamCaptureUnsupported and
// invalidates that capture), and the handle has no work of its own on them - its sequence has synchronized the stream it ran on.
void uzl::own_streams(uzl_pgo* h, bool drain_borrowed)
{
    if (!h->streams_borrowed) return;
    UZL_HIP(hipSetDevice(h->cfg.device));
    if (drain_borrowed) {
        UZL_HIP(hipStreamSynchronize(h->stream));
        if (h->stream2) UZL_HIP(hipStreamSynchronize(h->stream2));
    }
    hipStream_t a = stream_lease(h->cfg.device, 0, {}, false);
    hipStream_t b = a ? stream_lease(h->cfg.device, -1, {a}, false) : nullptr;
    if (!a || !b) { stream_release(h->cfg.device, a); throw HipError{hipErrorUnknown, "stream_lease", __FILE__, __LINE__}; }
    h->stream = a; h->stream2 = b; h->streams_borrowed = false;
}

extern "C" {

static_assert(sizeof(uzl_pgo_cfg) == 64, "uzl_pgo_cfg::pass_history occupies the former tail padding: the layout of ABI version 3 is unchanged");

void uzl_pgo_cfg_default(uzl_pgo_cfg* cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->iterations = 20;               // cfg/GraphOptimizer.cfg:10
    cfg->use_odometry_parameters = 0;   // :11
    cfg->optimize_xy_only = 0;          // :12
    cfg->device = 0;
    // relative M^-1-norm residual.  g2o's own LinearSolverPCG stops at 1e-6 on the SQUARED norm (1e-3 here) [EXT];
    // 1e-5 keeps the result within ~1e-5 m / 1e-6 rad of the direct (CSparse-like) solve at every LM iteration
    // count (measured deviation scales linearly with this value)
    cfg->pcg_tol = 1e-5;
    cfg->pcg_max_iter = 0;              // 0 = 6 * free vertices (system dimension)
    cfg->schur_reduce = 0;              // 0 = Schur-eliminate chain interiors when a third of the free vertices are (pgo_schur.hpp); -1 = never
    cfg->huber_delta = 1.0;             // g2o_optimizer.cpp:293
    cfg->verbose = 0;
    cfg->preconditioner = 1;            // additive multilevel (rigid-body-mode aggregation); 0 = block-Jacobi
    cfg->pcg_stop = 0;                  // step-error estimate; 1 = relative residual test only
    cfg->lm_loop = 0;                   // LM decisions on the device (captured passes); 1 = host-driven loop
    cfg->reduced_numbering = 0;         // the handle chooses between row order and strong aggregates (pgo_schur.hpp)
    cfg->pass_history = 0;              // pass sizes of a repeated optimize may come from the previous one's per-trial counts; 1 = never
}

int uzl_pgo_create(const uzl_pgo_cfg* cfg, uzl_pgo** out) { return pgo_create_on(cfg, nullptr, nullptr, out); }

void uzl_pgo_destroy(uzl_pgo* h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    destroy_pcg_graph(h);
    lm_run_destroy(h->lm); h->lm = nullptr;
    if (h->rccl_comm) { (void)rccl().CommDestroy(h->rccl_comm); h->rccl_comm = nullptr; }
    if (h->ev_lin) (void)hipEventDestroy(h->ev_lin);
    if (h->ev_setup) (void)hipEventDestroy(h->ev_setup);
    if (!h->streams_borrowed) { stream_release(h->cfg.device, h->stream2); stream_release(h->cfg.device, h->stream); }      // back to the pool, verdicts kept
    delete h;
}

int uzl_pgo_set_config(uzl_pgo* h, const uzl_pgo_cfg* cfg)
{
    if (!h || !cfg) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (cfg->device != h->cfg.device) return fail(h, UZL_ERR_BAD_ARG, "device cannot change after create");
    if (cfg->iterations < 1 || cfg->pcg_tol <= 0. || cfg->huber_delta <= 0.) return fail(h, UZL_ERR_BAD_ARG, "bad config value");
    if (cfg->pcg_tol != h->cfg.pcg_tol) destroy_pcg_graph(h);      // the tolerance is a captured kernel argument
    if (cfg->preconditioner != h->cfg.preconditioner || cfg->schur_reduce != h->cfg.schur_reduce || cfg->reduced_numbering != h->cfg.reduced_numbering) h->structure_ready = false;
    h->cfg = *cfg;
    return UZL_OK;
}

const char* uzl_pgo_last_error(uzl_pgo* h) { return last_error_of(h); }

int uzl_pgo_add_graph(uzl_pgo* h, int32_t n_nodes, const uzl_node* nodes, int32_t n_edges, const uzl_edge* edges,
                      int32_t n_sensors, const double* sensors)
{
    UZL_GUARD_BEGIN(h)
    if (n_nodes < 0 || n_edges < 0 || n_sensors < 0 || (n_nodes > 0 && !nodes) || (n_edges > 0 && !edges) ||
        (n_sensors > 0 && !sensors))
        return fail(h, UZL_ERR_BAD_ARG, "null or negative-size input");
    UZL_HIP(hipSetDevice(h->cfg.device));
    const StructureKey old_key = begin_graph(h, n_nodes);
    h->n = n_nodes; h->e_in = n_edges;
    h->fixed_in.assign((size_t)n_nodes, 0);
    for (int v = 0; v < n_nodes; v++) h->fixed_in[v] = nodes[v].fixed ? 1 : 0;
    h->in_edges.resize((size_t)n_edges);
    for (int k = 0; k < n_edges; k++) h->in_edges[k] = in_edge_of(edges[k]);
    h->in_ready = true; h->n_sensors_in = n_sensors;
    flatten_edges(h);
    alloc_problem(h);
    hipStream_t s = h->stream;
    h->d_nodes.reserve((size_t)std::max(n_nodes, 1));
    h->d_edges.reserve((size_t)std::max(n_edges, 1));
    h->d_src.reserve((size_t)std::max(h->e, 1));
    h->d_stage.reserve((size_t)std::max(n_sensors, 1) * 12);
    if (n_nodes) UZL_HIP(hipMemcpyAsync(h->d_nodes.p, nodes, sizeof(uzl_node) * (size_t)n_nodes, hipMemcpyHostToDevice, s));
    if (n_edges) UZL_HIP(hipMemcpyAsync(h->d_edges.p, edges, sizeof(uzl_edge) * (size_t)n_edges, hipMemcpyHostToDevice, s));
    if (n_sensors) UZL_HIP(hipMemcpyAsync(h->d_stage.p, sensors, sizeof(double) * 12 * (size_t)n_sensors, hipMemcpyHostToDevice, s));
    if (h->e) UZL_HIP(hipMemcpyAsync(h->d_src.p, h->src.data(), sizeof(int32_t) * (size_t)h->e, hipMemcpyHostToDevice, s));
    k_prepare_nodes(h->d_nodes.p, n_nodes, h->cfg.optimize_xy_only, h->cur, s);
    k_prepare_edges(h->d_edges.p, h->d_src.p, h->e, h->d_stage.p, n_sensors, h->cfg.optimize_xy_only, h->cfg.use_odometry_parameters,
                    h->d_zinv.p, h->d_info.p, s);
    UZL_HIP(hipGetLastError());
    finish_graph(h, old_key);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_pgo_append_graph(uzl_pgo* h, int32_t n_new_nodes, const uzl_node* new_nodes, int32_t n_new_edges, const uzl_edge* new_edges,
                         int32_t n_flags, const int32_t* edge_index, const uint8_t* edge_valid)
{
    UZL_GUARD_BEGIN(h)
    if (n_new_nodes < 0 || n_new_edges < 0 || n_flags < 0 || (n_new_nodes > 0 && !new_nodes) || (n_new_edges > 0 && !new_edges) ||
        (n_flags > 0 && (!edge_index || !edge_valid)))
        return fail(h, UZL_ERR_BAD_ARG, "null or negative-size input");
    if (!h->have_graph || !h->in_ready) return fail(h, UZL_ERR_BAD_ARG, "uzl_pgo_append_graph needs a graph from uzl_pgo_add_graph to grow");
    const int32_t n_old = h->n, e_old = h->e_in;
    for (int q = 0; q < n_flags; q++) if (edge_index[q] < 0 || edge_index[q] >= e_old) return fail(h, UZL_ERR_BAD_ARG, "edge index out of range");
    UZL_HIP(hipSetDevice(h->cfg.device));
    const StructureKey old_key = begin_graph(h, n_old + n_new_nodes);
    h->n = n_old + n_new_nodes; h->e_in = e_old + n_new_edges;
    if (old_key.ready) { h->fixed_in = old_key.fixed_in; }               // (the key took the vectors; the old flags are the first n_old of the new)
    for (int v = 0; v < n_new_nodes; v++) h->fixed_in.push_back(new_nodes[v].fixed ? 1 : 0);
    for (int q = 0; q < n_flags; q++) h->in_edges[edge_index[q]].valid = edge_valid[q] ? 1 : 0;
    for (int k = 0; k < n_new_edges; k++) h->in_edges.push_back(in_edge_of(new_edges[k]));
    flatten_edges(h);
    hipStream_t s = h->stream;
    alloc_problem(h, true);                                             // the estimates of the old nodes stay where the last solve left them
    h->d_nodes.reserve((size_t)std::max(n_new_nodes, 1));
    h->d_edges.reserve((size_t)std::max(h->e_in, 1), true, s);
    h->d_src.reserve((size_t)std::max(h->e, 1));
    if (n_new_nodes) UZL_HIP(hipMemcpyAsync(h->d_nodes.p, new_nodes, sizeof(uzl_node) * (size_t)n_new_nodes, hipMemcpyHostToDevice, s));
    if (n_new_edges) UZL_HIP(hipMemcpyAsync(h->d_edges.p + e_old, new_edges, sizeof(uzl_edge) * (size_t)n_new_edges, hipMemcpyHostToDevice, s));
    if (h->e) UZL_HIP(hipMemcpyAsync(h->d_src.p, h->src.data(), sizeof(int32_t) * (size_t)h->e, hipMemcpyHostToDevice, s));
    if (n_new_nodes) k_prepare_nodes(h->d_nodes.p, n_new_nodes, h->cfg.optimize_xy_only, h->cur + (size_t)n_old * 8, s);
    k_prepare_edges(h->d_edges.p, h->d_src.p, h->e, h->d_stage.p, h->n_sensors_in, h->cfg.optimize_xy_only, h->cfg.use_odometry_parameters,
                    h->d_zinv.p, h->d_info.p, s);
    UZL_HIP(hipGetLastError());
    finish_graph(h, old_key);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_pgo_rewrite_graph(uzl_pgo* h, const uzl_pgo_rewrite* rw, int32_t cap_nodes, int32_t* old_to_new_node, int32_t cap_edges, int32_t* old_to_new_edge)
{
    UZL_GUARD_BEGIN(h)
    if (!rw || rw->n_drop < 0 || rw->n_pose < 0 || rw->n_xf < 0 || rw->n_ops < 0 || (rw->n_drop > 0 && !rw->drop_nodes) ||
        (rw->n_pose > 0 && (!rw->pose_nodes || !rw->poses)) || (rw->n_xf > 0 && !rw->xf) || (rw->n_ops > 0 && !rw->ops))
        return fail(h, UZL_ERR_BAD_ARG, "null or negative-size input");
    if (!h->have_graph || !h->in_ready) return fail(h, UZL_ERR_BAD_ARG, "uzl_pgo_rewrite_graph needs a graph from uzl_pgo_add_graph to shrink");
    const int32_t n_old = h->n, e_old = h->e_in;
    if ((old_to_new_node && cap_nodes < n_old) || (old_to_new_edge && cap_edges < e_old)) return fail(h, UZL_ERR_BAD_ARG, "a map's capacity is below the old count");
    // ---- the plan (pgo_structure.hpp): a refused rewrite has changed nothing
    RewriteIn in;
    in.drop_nodes.assign(rw->drop_nodes, rw->drop_nodes + rw->n_drop);
    in.pose_nodes.assign(rw->pose_nodes, rw->pose_nodes + rw->n_pose);
    in.n_xf = rw->n_xf;
    in.ops.resize((size_t)rw->n_ops);
    for (int q = 0; q < rw->n_ops; q++) in.ops[q] = {rw->ops[q].edge, rw->ops[q].action, rw->ops[q].xf, rw->ops[q].node};
    RewritePlan P = rewrite_plan(n_old, h->in_edges, h->fixed_in, in);
    if (P.why) return fail(h, UZL_ERR_BAD_ARG, P.why);
    const int32_t n_new = (int32_t)P.new_to_old_node.size(), e_new = (int32_t)P.new_to_old_edge.size();
    UZL_HIP(hipSetDevice(h->cfg.device));
    const StructureKey old_key = begin_graph(h, n_new);
    hipStream_t s = h->stream;
    // ---- the plan on the device: [records | new_to_old_edge | node sources], [xf | placed poses]
    std::vector<int32_t> idx((size_t)5 * e_new + n_new);
    static_assert(sizeof(RewriteEdge) == 16, "rewrite_edges_kernel reads a record as one int4");
    if (e_new) {
        memcpy(idx.data(), P.rec.data(), sizeof(RewriteEdge) * (size_t)e_new);
        memcpy(idx.data() + (size_t)4 * e_new, P.new_to_old_edge.data(), sizeof(int32_t) * (size_t)e_new);
    }
    int32_t* node_src = idx.data() + (size_t)5 * e_new;
    for (int v = 0; v < n_new; v++) node_src[v] = P.new_to_old_node[v];
    for (int q = 0; q < rw->n_pose; q++) node_src[P.old_to_new_node[rw->pose_nodes[q]]] = ~q;
    std::vector<uzl_node> placed((size_t)rw->n_pose);
    for (int q = 0; q < rw->n_pose; q++) { memcpy(placed[q].pose, rw->poses + 12 * (size_t)q, sizeof(double) * 12); placed[q].fixed = 0; }
    h->d_rw_idx.reserve(std::max<size_t>(idx.size(), 1));
    h->d_rw_val.reserve(std::max<size_t>((size_t)12 * rw->n_xf + (size_t)8 * rw->n_pose, 1));
    h->d_edges_spare.reserve((size_t)std::max(e_new, 1));
    h->d_nodes.reserve((size_t)std::max(rw->n_pose, 1));
    double* d_xf = h->d_rw_val.p;
    double* d_placed = d_xf + (size_t)12 * rw->n_xf;
    if (!idx.empty()) UZL_HIP(hipMemcpyAsync(h->d_rw_idx.p, idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice, s));
    if (rw->n_xf) UZL_HIP(hipMemcpyAsync(d_xf, rw->xf, sizeof(double) * 12 * (size_t)rw->n_xf, hipMemcpyHostToDevice, s));
    if (rw->n_pose) UZL_HIP(hipMemcpyAsync(h->d_nodes.p, placed.data(), sizeof(uzl_node) * (size_t)rw->n_pose, hipMemcpyHostToDevice, s));
    // ---- the two compactions, out of place: the edge records into the spare buffer, the estimates into the other pose buffer
    //      (pose_nodes: prepared as add_graph prepares a node pose, by the same kernel, then placed by the gather)
    k_prepare_nodes(h->d_nodes.p, rw->n_pose, h->cfg.optimize_xy_only, d_placed, s);
    {
        hipEvent_t ea = nullptr, eb = nullptr;
        if (e_new > 0) h->timer.pair("rewrite_edges", &ea, &eb);
        k_rewrite_edges(h->d_edges.p, h->d_edges_spare.p, h->d_rw_idx.p + (size_t)4 * e_new, h->d_rw_idx.p, e_new, d_xf, s, ea, eb);
        ea = eb = nullptr;
        if (n_new > 0) h->timer.pair("rewrite_nodes", &ea, &eb);
        k_rewrite_nodes(h->cur, d_placed, h->d_rw_idx.p + (size_t)5 * e_new, n_new, h->trial, s, ea, eb);
    }
    std::swap(h->d_edges.p, h->d_edges_spare.p); std::swap(h->d_edges.cap, h->d_edges_spare.cap);
    std::swap(h->cur, h->trial);
    // ---- from here on as uzl_pgo_append_graph: the new graph's host side, its system edges, their values from the resident records
    h->n = n_new; h->e_in = e_new;
    h->fixed_in.swap(P.fixed_in);
    h->in_edges.swap(P.in_edges);
    flatten_edges(h);
    alloc_problem(h, true);
    h->d_src.reserve((size_t)std::max(h->e, 1));
    if (h->e) UZL_HIP(hipMemcpyAsync(h->d_src.p, h->src.data(), sizeof(int32_t) * (size_t)h->e, hipMemcpyHostToDevice, s));
    k_prepare_edges(h->d_edges.p, h->d_src.p, h->e, h->d_stage.p, h->n_sensors_in, h->cfg.optimize_xy_only, h->cfg.use_odometry_parameters,
                    h->d_zinv.p, h->d_info.p, s);
    UZL_HIP(hipGetLastError());
    finish_graph(h, old_key);                                            // (synchronises: idx / placed are locals)
    h->timer.resolve();
    if (old_to_new_node && n_old) memcpy(old_to_new_node, P.old_to_new_node.data(), sizeof(int32_t) * (size_t)n_old);
    if (old_to_new_edge && e_old) memcpy(old_to_new_edge, P.old_to_new_edge.data(), sizeof(int32_t) * (size_t)e_old);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_pgo_set_graph(uzl_pgo* h, int32_t n, const double* poses, const uint8_t* fixed, int32_t e,
                      const int32_t* ij, const double* meas, const double* info, const uint8_t* robust)
{
    UZL_GUARD_BEGIN(h)
    if (n < 0 || e < 0 || (n > 0 && (!poses || !fixed)) || (e > 0 && (!ij || !meas || !info || !robust)))
        return fail(h, UZL_ERR_BAD_ARG, "null or negative-size input");
    for (int k = 0; k < e; k++)
        if (ij[2 * k] < 0 || ij[2 * k] >= n || ij[2 * k + 1] < 0 || ij[2 * k + 1] >= n || ij[2 * k] == ij[2 * k + 1])
            return fail(h, UZL_ERR_BAD_ARG, "edge endpoint out of range");
    UZL_HIP(hipSetDevice(h->cfg.device));
    const StructureKey old_key = begin_graph(h, n);
    h->n = n; h->e_in = e; h->e = e;
    h->in_ready = false; h->in_edges.clear();                            // (d_stage, the sensors' place, is this call's staging area)
    h->fixed_in.assign(fixed, fixed + n);
    for (auto& f : h->fixed_in) f = f ? 1 : 0;
    h->ij.assign(ij, ij + 2 * (size_t)e);
    h->robust.assign(robust, robust + e);
    h->src.resize((size_t)e);
    std::iota(h->src.begin(), h->src.end(), 0);
    h->edge_w.resize((size_t)e);
    for (int k = 0; k < e; k++) { double tr = 0.; for (int r = 0; r < 6; r++) tr += info[36 * (size_t)k + r * 7]; h->edge_w[k] = tr; }
    alloc_problem(h);
    hipStream_t s = h->stream;
    const size_t stage = (size_t)std::max(n, 1) * 12 + (size_t)std::max(e, 1) * 48;
    h->d_stage.reserve(stage);
    double* d_p = h->d_stage.p;
    double* d_m = d_p + (size_t)std::max(n, 1) * 12;
    double* d_i = d_m + (size_t)std::max(e, 1) * 12;
    if (n) UZL_HIP(hipMemcpyAsync(d_p, poses, sizeof(double) * 12 * (size_t)n, hipMemcpyHostToDevice, s));
    if (e) {
        UZL_HIP(hipMemcpyAsync(d_m, meas, sizeof(double) * 12 * (size_t)e, hipMemcpyHostToDevice, s));
        UZL_HIP(hipMemcpyAsync(d_i, info, sizeof(double) * 36 * (size_t)e, hipMemcpyHostToDevice, s));
    }
    k_prepare_flat_nodes(d_p, n, h->cur, s);
    k_prepare_flat_edges(d_m, d_i, e, h->d_zinv.p, h->d_info.p, s);
    UZL_HIP(hipGetLastError());
    finish_graph(h, old_key);
    return UZL_OK;
    UZL_GUARD_END(h)
}


int uzl_pgo_reset(uzl_pgo* h)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "reset before add_graph/set_graph");
    UZL_HIP(hipSetDevice(h->cfg.device));
    if (h->n) UZL_HIP(hipMemcpyAsync(h->cur, h->pose_init.p, sizeof(double) * 8 * (size_t)h->n, hipMemcpyDeviceToDevice, h->stream));
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_pgo_optimize(uzl_pgo* h, int32_t iterations, uzl_pgo_stats* stats)
{
    UZL_GUARD_BEGIN(h)
    own_streams(h, true);
    return do_optimize(h, iterations, stats);
    UZL_GUARD_END(h)
}

int uzl_pgo_store(uzl_pgo* h, double* poses, double* edge_error, uint8_t* edge_in_system)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "store before add_graph/set_graph");
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    if (poses && h->n > 0) {
        h->d_out12.reserve((size_t)h->n * 12);
        k_poses_out(h->cur, h->n, h->d_out12.p, s);                                   // :110-117
        UZL_HIP(hipMemcpyAsync(poses, h->d_out12.p, sizeof(double) * 12 * (size_t)h->n, hipMemcpyDeviceToHost, s));
    }
    std::vector<double> err;
    if (edge_error && h->e > 0) {
        ensure_structure(h);    // store without optimize: same structure optimize would build
        h->d_err.reserve((size_t)h->e);
        k_edge_error(h->D, h->cur, h->d_err.p, s);                                    // :124-131
        err.resize((size_t)h->e);
        UZL_HIP(hipMemcpyAsync(err.data(), h->d_err.p, sizeof(double) * (size_t)h->e, hipMemcpyDeviceToHost, s));
    }
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    if (edge_error) {
        for (int k = 0; k < h->e_in; k++) edge_error[k] = std::numeric_limits<double>::quiet_NaN();
        for (int k = 0; k < h->e; k++) edge_error[h->src[k]] = err[k];
    }
    if (edge_in_system) {
        memset(edge_in_system, 0, (size_t)h->e_in);
        for (int k = 0; k < h->e; k++) edge_in_system[h->src[k]] = 1;
    }
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_pgo_get_fixed(uzl_pgo* h, uint8_t* fixed)
{
    if (!h || !fixed) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "no graph");
    const std::vector<uint8_t>& f = h->fixed_eff.size() == (size_t)h->n ? h->fixed_eff : h->fixed_in;
    if (h->n) memcpy(fixed, f.data(), (size_t)h->n);
    return UZL_OK;
}

int uzl_pgo_set_profiling(uzl_pgo* h, int32_t on)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->timer.on = on != 0;
    return UZL_OK;
}

int uzl_pgo_kernel_times(uzl_pgo* h, int32_t cap, const char** names, double* ms, int32_t* launches)
{
    if (!h || cap < 0 || (cap > 0 && (!names || !ms || !launches))) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return h->timer.report(cap, names, ms, launches);
}

int uzl_pgo_set_shard(uzl_pgo* h, int32_t rank, int32_t world_size, uzl_allreduce_fn allreduce, void* user)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (world_size < 1 || rank < 0 || rank >= world_size) return fail(h, UZL_ERR_BAD_ARG, "bad rank/world_size");
    if (world_size > 1 && !allreduce) return fail(h, UZL_ERR_BAD_ARG, "world_size > 1 needs an all-reduce callback");
    if (h->rccl_comm) { (void)hipStreamSynchronize(h->stream); (void)rccl().CommDestroy(h->rccl_comm); h->rccl_comm = nullptr; }
    h->rank = rank; h->world = world_size; h->allreduce = allreduce; h->allreduce_user = user;
    h->structure_ready = false;
    return UZL_OK;
}

int uzl_rccl_unique_id(void* id_out, int32_t cap)
{
    if (!id_out || cap < UZL_RCCL_UNIQUE_ID_BYTES) return UZL_ERR_BAD_ARG;
    RcclApi& R = rccl();
    if (!R.ok) return UZL_ERR_STATE;
    RcclApi::UniqueId id;
    if (R.GetUniqueId(&id) != 0) return UZL_ERR_HIP;
    memcpy(id_out, id.internal, UZL_RCCL_UNIQUE_ID_BYTES);
    return UZL_OK;
}

int uzl_pgo_set_shard_rccl(uzl_pgo* h, int32_t rank, int32_t world_size, const void* unique_id, int32_t id_bytes)
{
    UZL_GUARD_BEGIN(h)
    if (world_size < 1 || rank < 0 || rank >= world_size) return fail(h, UZL_ERR_BAD_ARG, "bad rank/world_size");
    if (!unique_id || id_bytes != UZL_RCCL_UNIQUE_ID_BYTES) return fail(h, UZL_ERR_BAD_ARG, "unique id must be UZL_RCCL_UNIQUE_ID_BYTES bytes");
    RcclApi& R = rccl();
    if (!R.ok) { h->last_error = R.error; return UZL_ERR_STATE; }
    UZL_HIP(hipSetDevice(h->cfg.device));
    UZL_HIP(hipStreamSynchronize(h->stream));
    if (h->rccl_comm) { (void)R.CommDestroy(h->rccl_comm); h->rccl_comm = nullptr; }
    RcclApi::UniqueId id;
    memcpy(id.internal, unique_id, UZL_RCCL_UNIQUE_ID_BYTES);
    RcclApi::Comm comm = nullptr;
    const int rc = R.CommInitRank(&comm, world_size, id, rank);               // collective over the ranks
    if (rc != 0 || !comm) {
        h->last_error = std::string("ncclCommInitRank failed: ") + (R.GetErrorString ? R.GetErrorString(rc) : "?");
        return UZL_ERR_HIP;
    }
    h->rccl_comm = comm;
    h->rank = rank; h->world = world_size; h->allreduce = nullptr; h->allreduce_user = nullptr;
    h->structure_ready = false;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_pgo_rccl_ranks(uzl_pgo* h)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    if (!h->rccl_comm) return 0;
    RcclApi& R = rccl();
    int n = 0;
    if (!R.CommCount || R.CommCount(h->rccl_comm, &n) != 0) return UZL_ERR_HIP;
    return n;
}

}  // extern "C"


// =====================================================================================================================
//  Batched solve: B independent graphs through ONE launch sequence (uzl_pgo_batch_*)
//
//  One config-2-sized graph leaves the chip ~97 % idle (125 workgroups per launch, two dependent launches per PCG iteration);
//  several handles on several streams do not recover it (tests/diag/multi_handle.py: 4 handles 1.9x, 16 handles 1.5x - the
//  launches serialise).  Here every kernel of the solve is launched once for all graphs (blockIdx.z = slot, arguments from a slot
//  table, each graph's Levenberg-Marquardt state on the device: uzl_pgo_lm.hip), so a PCG iteration of B graphs costs two launches,
//  like one graph's.  The kernels are the single-graph kernels' bodies and every graph's loop takes its own decisions from its own
//  state: poses, chi2 and iteration counts are bit-identical to a uzl_pgo_optimize of that graph alone.  Batched together are
//  graphs of the small-graph class (dense level-1 operator) with one hierarchy shape of the system the PCG solves - full or
//  Schur-reduced: chain-like graphs batch on their reduced systems; anything else - and any graph that meets an anomaly (PCG not
//  converged, breakdown) - is solved by the single-graph path, so results never depend on whether a graph was batched.
// =====================================================================================================================
struct uzl_pgo_batch : HandleBase {
    uzl_pgo_cfg cfg;
    std::vector<uzl_pgo*> h;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;        // rebuilds that run ahead (into the hierarchy copy the PCG does not use), beside this iteration's solves
    int32_t resident = 0;                 // graphs solved at a time (0 = all): uzl_pgo_batch_set_resident
    int32_t last_batched = 0;
    uzl::LmRun* lm = nullptr;             // slot table, LM states, captured segments (uzl_pgo_lm.hip)
    // second launch sequence (batches of >= kBatchLaneMin graphs): the second half of the graphs on streams of its own, driven by a second
    // host thread for the duration of the call - its kernels fill the tails of the first half's and a pass is as long as the longest solve
    // of eight graphs, not sixteen.  Only with four streams that do not stand in each other's way (uzl_pgo_batch_create).
    hipStream_t stream_b = nullptr, stream2_b = nullptr;
    uzl::LmRun* lm_b = nullptr;
    KernelTimer timer;                    // profiling (uzl_pgo_batch_set_profiling): the two PCG kernels, launched eagerly with event pairs
};

static int batch_optimize(uzl_pgo_batch* b, int32_t iterations, uzl_pgo_stats* stats, int32_t* n_batched)
{
    const int B = (int)b->h.size();
    if (n_batched) *n_batched = 0;
    for (uzl_pgo* h : b->h) if (!h->have_graph) return fail(b, UZL_ERR_STATE, "optimize before every graph of the batch has been set");
    UZL_HIP(hipSetDevice(b->cfg.device));
    // per graph: optimizeImpl's initializeOptimization + setFixedNodes (:139-146), structure
    for (int g = 0; g < B; g++) {
        uzl_pgo* h = b->h[g];
        if (iterations <= 0) iterations = h->cfg.iterations;
        prepare_optimize(h);
        UZL_HIP(hipStreamSynchronize(h->stream));
    }
    int rc_all = UZL_OK;
    if (!lm_batch_eligible(b->h)) {      // not one class / one shape: every graph through the single-graph path
        if (b->cfg.verbose)
            for (const uzl_pgo* h : b->h)
                fprintf(stderr, "[uzl_pgo_batch] not batched: levels %d agg %d mult %d cl %d sharded %d nb %d (pcg system %d) e %d timer %d n1 %d ns %d\n", h->mlp.levels,
                        h->mlp.agg, (int)h->ml_mult, h->mlp.cl, (int)h->sharded, h->nb, h->Dp.nb, h->e, (int)h->timer.on, h->mlp.n.size() > 1 ? h->mlp.n[1] : -1, h->ml_ns_steps);
        for (int g = 0; g < B; g++) {
            uzl_pgo* h = b->h[g];
            h->t_start = std::chrono::steady_clock::now();
            uzl_pgo_stats S;
            const int rc = lm_eligible(h) ? do_optimize_lm(h, iterations, &S) : do_optimize_host(h, iterations, &S);
            if (rc != UZL_OK && rc != UZL_ERR_NOT_CONVERGED) { b->last_error = h->last_error; return rc; }
            if (rc != UZL_OK) rc_all = rc;
            if (stats) stats[g] = S;
        }
        b->last_batched = 0;
        return rc_all;
    }
    static const bool one_lane = diag_int("UZL_BATCH_LANES", 2) < 2;          // diagnostic build, UZL_BATCH_LANES=1: one launch sequence
    const bool eager = b->h[0]->no_graph, verbose = b->cfg.verbose != 0;
    auto one_sequence = [&]() {
        const int done = batch_optimize_lm(b->lm, b->h, b->resident, b->stream, b->stream2, iterations, eager, verbose, &b->timer, stats, &rc_all);
        if (done < 0) { b->last_error = b->h[(size_t)(-1 - done)]->last_error; return rc_all; }
        b->last_batched = done;
        if (n_batched) *n_batched = done;
        return rc_all;
    };
    if (B < kBatchLaneMin || one_lane || b->resident == 1 || b->timer.on || !b->stream_b || !b->stream2_b) return one_sequence();
    // ---- L launch sequences: the graphs in L runs, the first from this thread, the others from helper threads.  The sequences share
    //      nothing but the device (every graph has its handle, every sequence its streams, slot table and captured segments), and a graph's
    //      result does not depend on its neighbours in the batch, so the split changes no bit of any result.
    constexpr int L = 2;
    struct Lane { uzl::LmRun** lm; hipStream_t s, s2; int first, count, resident, rc, done; std::exception_ptr ex; };
    std::vector<Lane> lanes((size_t)L);
    {
        uzl::LmRun** lms[L] = {&b->lm, &b->lm_b};
        hipStream_t ss[L] = {b->stream, b->stream_b};
        hipStream_t s2s[L] = {b->stream2, b->stream2_b};
        int first = 0, res_left = b->resident;
        for (int l = 0; l < L; l++) {
            const int count = (B - first + (L - l) - 1) / (L - l);
            const int res = b->resident > 0 ? (res_left + (L - l) - 1) / (L - l) : 0;
            lanes[(size_t)l] = Lane{lms[l], ss[l], s2s[l], first, count, res, UZL_OK, 0, nullptr};
            first += count; res_left -= res;
        }
    }
    auto run_lane = [&](Lane& ln) {
        try {
            UZL_HIP(hipSetDevice(b->cfg.device));
            const std::vector<uzl_pgo*> hs(b->h.begin() + ln.first, b->h.begin() + ln.first + ln.count);
            ln.done = batch_optimize_lm(*ln.lm, hs, ln.resident, ln.s, ln.s2, iterations, eager, verbose, nullptr, stats ? stats + ln.first : nullptr, &ln.rc);
        } catch (...) { ln.ex = std::current_exception(); }
    };
    std::vector<std::thread> helpers;
    try {
        for (int l = 1; l < L; l++) helpers.emplace_back([&, l] { run_lane(lanes[(size_t)l]); });
    } catch (const std::system_error&) {                                       // (no more threads to be had: the sequences not started run from this one)
        for (int l = (int)helpers.size() + 1; l < L; l++) run_lane(lanes[(size_t)l]);
    }
    run_lane(lanes[0]);
    for (std::thread& t : helpers) t.join();
    for (Lane& ln : lanes) if (ln.ex) std::rethrow_exception(ln.ex);
    int total = 0;
    for (Lane& ln : lanes) {
        if (ln.done < 0) { b->last_error = b->h[(size_t)(ln.first - 1 - ln.done)]->last_error; return ln.rc; }
        if (ln.rc != UZL_OK && rc_all == UZL_OK) rc_all = ln.rc;
        total += ln.done;
    }
    b->last_batched = total;
    if (n_batched) *n_batched = total;
    return rc_all;
}

extern "C" {

int uzl_pgo_batch_create(const uzl_pgo_cfg* cfg, int32_t n_graphs, uzl_pgo_batch** out)
{
    if (!out || n_graphs < 1 || n_graphs > kBatchMax) return UZL_ERR_BAD_ARG;
    *out = nullptr;
    uzl_pgo_cfg c;
    if (cfg) c = *cfg; else uzl_pgo_cfg_default(&c);
    if (check_device(c.device) != UZL_OK) return UZL_ERR_NO_DEVICE;
    uzl_pgo_batch* b = new (std::nothrow) uzl_pgo_batch();
    if (!b) return UZL_ERR_OOM;
    b->cfg = c;
    if (getenv("UZL_VERBOSE")) b->cfg.verbose = 1;
    // The batch's streams come from the device's pool (uzl_streams.hip): none in another's way.  Batches of kBatchLaneMin graphs and more
    // get a second launch sequence if four such streams can be had within the pool's budget - otherwise, and with UZL_STREAM_PROBE=0,
    // the batch runs as ONE launch sequence whatever streams it got; a rebuild stream that cannot be had apart from the solver's is
    // replaced by any stream (slower, not wrong).
    static const bool two_on = diag_int("UZL_BATCH_LANES", 2) >= 2;          // diagnostic build, UZL_BATCH_LANES=1: one launch sequence
    const int dev = c.device;
    b->stream = stream_lease(dev, 0, {}, false);
    bool ok = b->stream != nullptr;
    if (ok && two_on && n_graphs >= kBatchLaneMin) b->stream_b = stream_lease(dev, 0, {b->stream}, true);
    if (ok) {
        b->stream2 = stream_lease(dev, 0, {b->stream, b->stream_b}, false);
        ok = b->stream2 != nullptr;
    }
    if (ok && b->stream_b) {
        b->stream2_b = stream_lease(dev, 0, {b->stream, b->stream_b, b->stream2}, true);
        if (!b->stream2_b) { stream_release(dev, b->stream_b); b->stream_b = nullptr; }      // no fourth: one sequence
    }
    int rc_h = UZL_OK;
    for (int32_t g = 0; ok && g < n_graphs; g++) {              // the graphs' handles, on the batch's first launch sequence's streams
        uzl_pgo* h = nullptr;
        rc_h = pgo_create_on(&c, b->stream, b->stream2, &h);
        if (rc_h != UZL_OK) { ok = false; break; }
        b->h.push_back(h);
    }
    if (!ok) {
        for (uzl_pgo* x : b->h) uzl_pgo_destroy(x);
        for (hipStream_t q : {b->stream, b->stream2, b->stream_b, b->stream2_b}) stream_release(dev, q);
        delete b;
        return rc_h != UZL_OK ? rc_h : UZL_ERR_HIP;
    }
    *out = b;
    return UZL_OK;
}

void uzl_pgo_batch_destroy(uzl_pgo_batch* b)
{
    if (!b) return;
    (void)hipSetDevice(b->cfg.device);
    for (hipStream_t q : {b->stream2, b->stream, b->stream2_b, b->stream_b}) if (q) (void)hipStreamSynchronize(q);
    lm_run_destroy(b->lm); b->lm = nullptr;
    lm_run_destroy(b->lm_b); b->lm_b = nullptr;
    for (uzl_pgo* x : b->h) uzl_pgo_destroy(x);
    for (hipStream_t q : {b->stream, b->stream2, b->stream_b, b->stream2_b}) stream_release(b->cfg.device, q);      // back to the pool, verdicts kept
    delete b;
}

const char* uzl_pgo_batch_last_error(uzl_pgo_batch* b) { return last_error_of(b); }
int uzl_pgo_batch_size(uzl_pgo_batch* b) { return b ? (int)b->h.size() : UZL_ERR_BAD_ARG; }
uzl_pgo* uzl_pgo_batch_graph(uzl_pgo_batch* b, int32_t i) { return (b && i >= 0 && i < (int32_t)b->h.size()) ? b->h[(size_t)i] : nullptr; }

int uzl_pgo_batch_set_resident(uzl_pgo_batch* b, int32_t n_resident)
{
    if (!b || n_resident < 0) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(b->mu);
    b->resident = n_resident;
    return UZL_OK;
}

int uzl_pgo_batch_set_profiling(uzl_pgo_batch* b, int32_t on)
{
    if (!b) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(b->mu);
    b->timer.on = on != 0;
    return UZL_OK;
}

int uzl_pgo_batch_kernel_times(uzl_pgo_batch* b, int32_t cap, const char** names, double* ms, int32_t* launches)
{
    if (!b || cap < 0 || (cap > 0 && (!names || !ms || !launches))) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(b->mu);
    return b->timer.report(cap, names, ms, launches);
}

int uzl_pgo_batch_optimize(uzl_pgo_batch* b, int32_t iterations, uzl_pgo_stats* stats, int32_t* n_batched)
{
    UZL_GUARD_BEGIN(b)
    return batch_optimize(b, iterations, stats, n_batched);
    UZL_GUARD_END(b)
}

}  // extern "C"
