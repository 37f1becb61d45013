// laser_kernels.hip — point-to-line ICP of laser scan pairs on gfx950 (contract: include/uzl_mi355x.h, "Laser scan matching").
//
// laser_icp_kernel: one 256-thread workgroup per pair, the whole ICP inside it.  `from`'s Cartesian points are staged once into
// LDS (an invalid beam as NaN, so it never wins a comparison); lane t owns beams t, t + 256, ... of `to` and recomputes their
// points from the (cos, sin) table and the readings (two multiplies) instead of holding a second 64 KB array.  The nearest-
// neighbour loop reads `from` at a wave-uniform LDS address (broadcast).  Doubles: 64-bit integer min per j1 in LDS on the bit
// pattern of the squared distance.  Trim: the two order statistics by a rank count over the distances in LDS.  Sums: beam order
// within a lane's strip, a butterfly within the wave, then ((w0 + w1) + (w2 + w3)) - every lane ends with the same bits, so the
// closed-form step and every decision after it are computed redundantly by all lanes and never broadcast.
// Built with -ffp-contract=off: every operation rounds as the contract says.
#include "laser_types.hpp"

namespace uzl {

namespace {

constexpr int kNone = -1;
constexpr int kDroppedDouble = 1 << 24, kDroppedTrim = 1 << 25, kDropped = kDroppedDouble | kDroppedTrim;

struct Est { double tx, ty, c, s; };

struct Lds {
    double2* from;                 // [nf] point of beam j, (NaN, NaN) when the beam is invalid
    unsigned long long* best;      // [nf] bits of the smallest squared distance among the correspondences with this j1
    double* dist;                  // [nt] squared distance to j1, then the point-to-line distance (+inf: no correspondence)
    int32_t* corr;                 // [nt] j1 | j2 << 12 | flags, or kNone
    double (*red)[kIcpSums];       // [kIcpWaves]
    int32_t* cnt;                  // [0] after doubles, [1] after trim, [2] valid beams of `to`
    double* lim;                   // [0], [1]: the two order statistics
};

__device__ inline bool beam_valid(float r, const LaserScanRec& s) { return r >= s.range_min && r <= s.range_max; }

__device__ inline double wave_tree(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// contract steps 2-4 at estimate x; returns the number of correspondences left (the same in every lane)
__device__ int correspondences(const LaserIcpArgs& a, const LaserScanRec& F, const LaserScanRec& T, const Est& x, const Lds& l)
{
    const int tid = (int)threadIdx.x, nf = F.n, nt = T.n;
    for (int j = tid; j < nf; j += kIcpBlock) l.best[j] = ~0ull;
    if (tid < 2) l.cnt[tid] = 0;
    __syncthreads();
    // step 2
    for (int i = tid; i < nt; i += kIcpBlock) {
        const float r = a.values[T.values_off + i];
        int32_t packed = kNone;
        double keep = __longlong_as_double(0x7ff0000000000000ll);
        if (beam_valid(r, T)) {
            const double2 t = a.trig[T.trig_off + i];
            const double px = t.x * (double)r, py = t.y * (double)r;
            const double wx = (x.c * px - x.s * py) + x.tx, wy = (x.s * px + x.c * py) + x.ty;
            double bd = keep;
            int bj = -1;
            for (int j = 0; j < nf; j++) {
                const double2 q = l.from[j];
                const double dx = wx - q.x, dy = wy - q.y;
                const double d2 = dx * dx + dy * dy;
                if (d2 < bd) { bd = d2; bj = j; }
            }
            if (bj >= 0 && bd <= a.max_corr_sq) {
                int up = -1, down = -1;
                for (int j = bj + 1; j < nf; j++) if (l.from[j].x == l.from[j].x) { up = j; break; }
                for (int j = bj - 1; j >= 0; j--) if (l.from[j].x == l.from[j].x) { down = j; break; }
                int j2 = -1;
                if (up >= 0 && down >= 0) {
                    const double2 qu = l.from[up], qd = l.from[down];
                    const double ux = wx - qu.x, uy = wy - qu.y, ex = wx - qd.x, ey = wy - qd.y;
                    j2 = (ux * ux + uy * uy) <= (ex * ex + ey * ey) ? up : down;
                } else {
                    j2 = up >= 0 ? up : down;
                }
                if (j2 >= 0) {
                    const double2 q1 = l.from[bj], q2 = l.from[j2];
                    const double lx = q2.x - q1.x, ly = q2.y - q1.y;
                    if (lx * lx + ly * ly > 0.0) {
                        packed = bj | (j2 << 12);
                        keep = bd;
                        atomicMin(&l.best[bj], (unsigned long long)__double_as_longlong(bd));
                    }
                }
            }
        }
        l.corr[i] = packed;
        l.dist[i] = keep;
    }
    __syncthreads();
    // step 3, and step 4's distance of what is left
    for (int i = tid; i < nt; i += kIcpBlock) {
        const int32_t packed = l.corr[i];
        if (packed < 0) continue;
        const int j1 = packed & 0xfff, j2 = (packed >> 12) & 0xfff;
        if (l.best[j1] < (unsigned long long)__double_as_longlong(l.dist[i])) {
            l.corr[i] = packed | kDroppedDouble;
            l.dist[i] = __longlong_as_double(0x7ff0000000000000ll);
            continue;
        }
        const float r = a.values[T.values_off + i];
        const double2 t = a.trig[T.trig_off + i];
        const double px = t.x * (double)r, py = t.y * (double)r;
        const double wx = (x.c * px - x.s * py) + x.tx, wy = (x.s * px + x.c * py) + x.ty;
        const double2 q1 = l.from[j1], q2 = l.from[j2];
        const double lx = q2.x - q1.x, ly = q2.y - q1.y;
        const double len = sqrt(lx * lx + ly * ly);
        const double nx = -ly / len, ny = lx / len;
        l.dist[i] = fabs(nx * (wx - q1.x) + ny * (wy - q1.y));
        atomicAdd(&l.cnt[0], 1);
    }
    __syncthreads();
    const int k = l.cnt[0];
    if (k == 0) return 0;
    // step 4: the two order statistics by rank (ties by beam index: the value at a rank does not depend on them)
    int i1 = (int)floor((double)k * a.max_perc), i2 = (int)floor((double)k * a.adaptive_order);
    i1 = min(max(i1, 0), k - 1);
    i2 = min(max(i2, 0), k - 1);
    for (int i = tid; i < nt; i += kIcpBlock) {
        const int32_t packed = l.corr[i];
        if (packed < 0 || (packed & kDropped)) continue;
        const double d = l.dist[i];
        int rank = 0;
        for (int j = 0; j < nt; j++) {
            const double e = l.dist[j];
            rank += (e < d || (e == d && j < i)) ? 1 : 0;
        }
        if (rank == i1) l.lim[0] = d;
        if (rank == i2) l.lim[1] = d;
    }
    __syncthreads();
    const double limit = fmin(l.lim[0], a.adaptive_mult * l.lim[1]);
    for (int i = tid; i < nt; i += kIcpBlock) {
        const int32_t packed = l.corr[i];
        if (packed < 0 || (packed & kDropped)) continue;
        if (l.dist[i] > limit) l.corr[i] = packed | kDroppedTrim;
        else atomicAdd(&l.cnt[1], 1);
    }
    __syncthreads();
    return l.cnt[1];
}

// step 6's sums over the correspondences left, in the fixed order
__device__ void sums(const LaserIcpArgs& a, const LaserScanRec& T, const Lds& l, double* S)
{
    const int tid = (int)threadIdx.x, nt = T.n;
#pragma unroll
    for (int k = 0; k < kIcpSums; k++) S[k] = 0.0;
    for (int i = tid; i < nt; i += kIcpBlock) {
        const int32_t packed = l.corr[i];
        if (packed < 0 || (packed & kDropped)) continue;
        const int j1 = packed & 0xfff, j2 = (packed >> 12) & 0xfff;
        const double r = (double)a.values[T.values_off + i];
        const double2 t = a.trig[T.trig_off + i];
        const double px = t.x * r, py = t.y * r;
        const double2 q1 = l.from[j1], q2 = l.from[j2];
        const double lx = q2.x - q1.x, ly = q2.y - q1.y;
        const double len = sqrt(lx * lx + ly * ly);
        const double nx = -ly / len, ny = lx / len;
        const double w = 1.0 / (r * r);
        const double a2 = nx * px + ny * py, a3 = ny * px - nx * py, b = nx * q1.x + ny * q1.y;
        const double w0 = w * nx, w1 = w * ny, w2 = w * a2, w3 = w * a3, wb = w * b;
        S[0] += w0 * nx; S[1] += w0 * ny; S[2] += w0 * a2; S[3] += w0 * a3;
        S[4] += w1 * ny; S[5] += w1 * a2; S[6] += w1 * a3;
        S[7] += w2 * a2; S[8] += w2 * a3;
        S[9] += w3 * a3;
        S[10] += wb * nx; S[11] += wb * ny; S[12] += wb * a2; S[13] += wb * a3;
        S[14] += wb * b;
    }
    __syncthreads();                                        // the previous reduction's readers are done with red
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < kIcpSums; k++) {
        const double v = wave_tree(S[k]);
        if (lane == 0) l.red[wave][k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kIcpSums; k++) S[k] = (l.red[0][k] + l.red[1][k]) + (l.red[2][k] + l.red[3][k]);
}

// step 8's error: sum of squared point-to-line distances of the correspondences left, at estimate x, in the fixed order
__device__ double final_error(const LaserIcpArgs& a, const LaserScanRec& T, const Est& x, const Lds& l)
{
    const int tid = (int)threadIdx.x, nt = T.n;
    double acc = 0.0;
    for (int i = tid; i < nt; i += kIcpBlock) {
        const int32_t packed = l.corr[i];
        if (packed < 0 || (packed & kDropped)) continue;
        const int j1 = packed & 0xfff, j2 = (packed >> 12) & 0xfff;
        const double r = (double)a.values[T.values_off + i];
        const double2 t = a.trig[T.trig_off + i];
        const double px = t.x * r, py = t.y * r;
        const double wx = (x.c * px - x.s * py) + x.tx, wy = (x.s * px + x.c * py) + x.ty;
        const double2 q1 = l.from[j1], q2 = l.from[j2];
        const double lx = q2.x - q1.x, ly = q2.y - q1.y;
        const double len = sqrt(lx * lx + ly * ly);
        const double nx = -ly / len, ny = lx / len;
        const double e = nx * (wx - q1.x) + ny * (wy - q1.y);
        acc += e * e;
    }
    __syncthreads();                                        // the previous reduction's readers are done with red
    const double v = wave_tree(acc);
    if ((tid & 63) == 0) l.red[tid >> 6][0] = v;
    __syncthreads();
    return (l.red[0][0] + l.red[1][0]) + (l.red[2][0] + l.red[3][0]);
}

// step 6's closed form: false when the system is degenerate
__device__ bool solve(const double* S, Est* out)
{
    const double M00 = S[0], M01 = S[1], M02 = S[2], M03 = S[3], M11 = S[4], M12 = S[5], M13 = S[6], M22 = S[7], M23 = S[8], M33 = S[9];
    const double v0 = S[10], v1 = S[11], v2 = S[12], v3 = S[13];
    const double det_a = M00 * M11 - M01 * M01;
    if (!(det_a > 0.0)) return false;
    const double E00 = (M11 * M02 - M01 * M12) / det_a, E01 = (M11 * M03 - M01 * M13) / det_a;
    const double E10 = (M00 * M12 - M01 * M02) / det_a, E11 = (M00 * M13 - M01 * M03) / det_a;
    const double f0 = (M11 * v0 - M01 * v1) / det_a, f1 = (M00 * v1 - M01 * v0) / det_a;
    const double Q00 = M22 - (M02 * E00 + M12 * E10), Q01 = M23 - (M02 * E01 + M12 * E11), Q11 = M33 - (M03 * E01 + M13 * E11);
    const double h0 = -2.0 * (v2 - (M02 * f0 + M12 * f1)), h1 = -2.0 * (v3 - (M03 * f0 + M13 * f1));
    const double dq = Q00 - Q11;
    const double e_min = ((Q00 + Q11) - sqrt(dq * dq + 4.0 * (Q01 * Q01))) / 2.0;
    const double hn = sqrt(h0 * h0 + h1 * h1);
    if (!(hn > 0.0) || !(hn < 1.7e308) || !(e_min == e_min)) return false;
    double lo = -e_min, hi = lo + hn;
    for (int it = 0; it < kIcpBisections; it++) {
        const double mid = 0.5 * (lo + hi);
        const double p = Q00 + mid, q = Q11 + mid;
        const double det = p * q - Q01 * Q01;
        const double g0 = q * h0 - Q01 * h1, g1 = p * h1 - Q01 * h0;
        if (det * det - 0.25 * (g0 * g0 + g1 * g1) > 0.0) hi = mid; else lo = mid;
    }
    const double lam = 0.5 * (lo + hi);
    const double p = Q00 + lam, q = Q11 + lam;
    const double det = p * q - Q01 * Q01;
    const double g0 = q * h0 - Q01 * h1, g1 = p * h1 - Q01 * h0;
    double c = -g0 / (2.0 * det), s = -g1 / (2.0 * det);
    const double nrm = sqrt(c * c + s * s);
    if (!(nrm > 0.0) || !(nrm < 1.7e308)) return false;
    c = c / nrm;
    s = s / nrm;
    out->c = c; out->s = s;
    out->tx = f0 - (E00 * c + E01 * s);
    out->ty = f1 - (E10 * c + E11 * s);
    return out->tx == out->tx && out->ty == out->ty;
}

__global__ __launch_bounds__(kIcpBlock) void laser_icp_kernel(LaserIcpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ double s_red[kIcpWaves][kIcpSums];
    __shared__ double s_lim[2];
    __shared__ int32_t s_cnt[3];
    Lds l;
    l.from = reinterpret_cast<double2*>(lds);
    l.best = reinterpret_cast<unsigned long long*>(lds + (size_t)a.max_from * sizeof(double2));
    l.dist = reinterpret_cast<double*>(lds + (size_t)a.max_from * (sizeof(double2) + sizeof(unsigned long long)));
    l.corr = reinterpret_cast<int32_t*>(lds + (size_t)a.max_from * (sizeof(double2) + sizeof(unsigned long long)) + (size_t)a.max_to * sizeof(double));
    l.red = s_red; l.lim = s_lim; l.cnt = s_cnt;

    const int tid = (int)threadIdx.x;
    const LaserPairRec pr = a.pairs[blockIdx.x];
    const LaserScanRec F = a.scans[pr.from], T = a.scans[pr.to];
    if (F.n > a.max_from || T.n > a.max_to) return;         // (the host sizes both from the same pairs)
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // step 1
    if (tid == 0) s_cnt[2] = 0;
    for (int j = tid; j < F.n; j += kIcpBlock) {
        const float r = a.values[F.values_off + j];
        const double2 t = a.trig[F.trig_off + j];
        l.from[j] = beam_valid(r, F) ? make_double2(t.x * (double)r, t.y * (double)r) : make_double2(nan, nan);
    }
    __syncthreads();
    int my_valid = 0;
    for (int i = tid; i < T.n; i += kIcpBlock) my_valid += beam_valid(a.values[T.values_off + i], T) ? 1 : 0;
    if (my_valid) atomicAdd(&s_cnt[2], my_valid);

    Est x{pr.tx, pr.ty, pr.c, pr.s};
    if (a.stage) {
        correspondences(a, F, T, x, l);
        for (int i = tid; i < T.n; i += kIcpBlock) {
            const int32_t packed = l.corr[i];
            const bool any = packed >= 0;
            a.st_j1[i] = any ? (packed & 0xfff) : -1;
            a.st_j2[i] = any ? ((packed >> 12) & 0xfff) : -1;
            a.st_valid[i] = (any && !(packed & kDropped)) ? 1 : 0;
            a.st_dist[i] = (any && !(packed & kDroppedDouble)) ? l.dist[i] : 0.0;
        }
        return;
    }

    int status = UZL_LASER_OK, iterations = 0, left = 0;
    double S[kIcpSums];
    while (iterations < a.max_iterations) {
        left = correspondences(a, F, T, x, l);
        // step 5
        if (left == 0 || (double)left < a.fail_fraction * (double)T.n) { status = UZL_LASER_FEW_CORR; break; }
        sums(a, T, l, S);
        Est y;
        if (!solve(S, &y)) { status = UZL_LASER_DEGENERATE; break; }
        iterations++;
        // step 7
        const double dx = y.tx - x.tx, dy = y.ty - x.ty;
        const double cross = x.c * y.s - x.s * y.c, dot = x.c * y.c + x.s * y.s;
        const bool converged = (dx * dx + dy * dy < a.eps_xy_sq) && (fabs(cross) < a.sin_eps_theta) && (dot > 0.0);
        x = y;
        if (converged) break;
    }
    const double error = status == UZL_LASER_OK ? final_error(a, T, x, l) : 0.0;
    if (tid != 0) return;
    LaserPairOut o;
    o.tx = x.tx; o.ty = x.ty; o.c = x.c; o.s = x.s;
    for (int k = 0; k < 6; k++) o.H[k] = 0.0;
    o.error = 0.0;
    o.status = status; o.nvalid = 0; o.deg_count = 0; o.iterations = iterations; o._pad = 0;
    o.scan_valid = s_cnt[2];
    if (status == UZL_LASER_OK) {
        // step 8's walk in beam order
        int last_corr = -1, deg = 0;
        for (int i = 0; i < T.n; i++) {
            const int32_t packed = l.corr[i];
            if (packed < 0 || (packed & kDropped)) continue;
            const int j1 = packed & 0xfff;
            if (j1 > last_corr) deg++; else if (j1 < last_corr) deg--;
            last_corr = j1;
        }
        o.nvalid = left;
        o.deg_count = deg;
        o.error = error;
        // step 9: u = d(c, s)/dtheta = (-s, c)
        const double u0 = -x.s, u1 = x.c;
        o.H[0] = S[0]; o.H[1] = S[1]; o.H[2] = S[2] * u0 + S[3] * u1;
        o.H[3] = S[4]; o.H[4] = S[5] * u0 + S[6] * u1;
        o.H[5] = (S[7] * (u0 * u0) + 2.0 * (S[8] * (u0 * u1))) + S[9] * (u1 * u1);
    }
    a.out[blockIdx.x] = o;
}

}  // namespace

void laser_icp_prepare()
{
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(laser_icp_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)laser_icp_lds(kIcpMaxBeams, kIcpMaxBeams));
}

void launch_laser_icp(const LaserIcpArgs& a, int n_pairs, hipStream_t s)
{
    if (n_pairs > 0)
        hipLaunchKernelGGL(laser_icp_kernel, dim3(n_pairs), dim3(kIcpBlock), laser_icp_lds(a.max_from, a.max_to), s, a);
}

}  // namespace uzl
