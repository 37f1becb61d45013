// cloud_kernels.hip — colour point-cloud registration (GICP-6D): the device side of uzl_cloud_*.
//
// include/uzl_mi355x.h states the contract step by step; tests/cloud_reference.py restates it in NumPy.  Built with
// -ffp-contract=off: every product and sum below rounds on its own, in the order written.
//   cloud_lab_kernel     step 3: BGR8 -> CIELAB (f64 through the host's linearisation table, cube root by Halley steps)
//   cloud_cov_kernel     step 4: 20 nearest in 3-D (targets stream through LDS, a sorted list per lane in registers), covariance,
//                        normal by cyclic Jacobi, C = I - (1 - eps) n n^T
//   cloud_prepare_kernel step 5: the `to` cloud moved by the first guess, the pair's state
//   cloud_nn6_kernel     step 6: brute-force 6-D nearest neighbour, lanes own queries, the target read at a wave-uniform LDS address
//   cloud_step_kernel    steps 6-8: M_i, the damped Gauss-Newton steps with sums in a fixed order, the convergence test
#include "cloud_types.hpp"

namespace uzl {
namespace {

// ------------------------------------------------------------------------------------------------ step 3
__device__ inline double lab_f(double x)
{
    if (!(x > 0.008856)) return 7.787 * x + 16.0 / 116.0;
    double y = 0.35 + 0.7 * x;
#pragma unroll
    for (int s = 0; s < kCloudCbrtSteps; s++) {
        const double y3 = (y * y) * y;
        y = (y * (y3 + (x + x))) / ((y3 + y3) + x);
    }
    return y;
}

__global__ __launch_bounds__(256) void cloud_lab_kernel(const uint8_t* __restrict__ bgr, float* __restrict__ lab,
                                                        const double* __restrict__ table, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double B = table[bgr[3 * i]], G = table[bgr[3 * i + 1]], R = table[bgr[3 * i + 2]];
    double X = (R * 0.4124 + G * 0.3576) + B * 0.1805;
    double Y = (R * 0.2126 + G * 0.7152) + B * 0.0722;
    double Z = (R * 0.0193 + G * 0.1192) + B * 0.9505;
    X = X / 0.95047;
    Z = Z / 1.08883;
    X = lab_f(X); Y = lab_f(Y); Z = lab_f(Z);
    lab[3 * i] = (float)(116.0 * Y - 16.0);
    lab[3 * i + 1] = (float)(500.0 * (X - Y));
    lab[3 * i + 2] = (float)(200.0 * (Y - Z));
}

// ------------------------------------------------------------------------------------------------ step 4
// One Jacobi rotation of the symmetric 3x3 in the (p, q) plane; r is the third index, (vkp, vkq) the columns p and q of V.
__device__ inline void jacobi(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p,
                              double& v1q, double& v2p, double& v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp; arq = rq;
    double a, b;
    a = c * v0p - s * v0q; b = s * v0p + c * v0q; v0p = a; v0q = b;
    a = c * v1p - s * v1q; b = s * v1p + c * v1q; v1p = a; v1q = b;
    a = c * v2p - s * v2q; b = s * v2p + c * v2q; v2p = a; v2q = b;
}

__global__ __launch_bounds__(kCloudBlock) void cloud_cov_kernel(const CloudRec* __restrict__ recs, const float* __restrict__ xyz,
                                                                double* __restrict__ cov, int32_t k, double gicp_epsilon)
{
    __shared__ float4 tile[kCloudTile];
    const CloudRec rec = recs[blockIdx.y];
    const int n = rec.n;
    if (n < k || (int)blockIdx.x * kCloudBlock >= n) return;  // a cloud too small for step 4 keeps no covariances (an estimate refuses it)
    const float* P = xyz + 3 * rec.off;
    const int tid = threadIdx.x, i = blockIdx.x * kCloudBlock + tid;
    const bool live = i < n;
    const int ic = live ? i : n - 1;
    const float qx = P[3 * ic], qy = P[3 * ic + 1], qz = P[3 * ic + 2];
    float ld[kCloudK];
    int li[kCloudK];
#pragma unroll
    for (int r = 0; r < kCloudK; r++) { ld[r] = __builtin_inff(); li[r] = 0; }
    for (int base = 0; base < n; base += kCloudTile) {
        const int m = min(kCloudTile, n - base);
        __syncthreads();
        for (int j = tid; j < m; j += kCloudBlock) {
            const float* s = P + 3 * (size_t)(base + j);
            tile[j] = make_float4(s[0], s[1], s[2], 0.f);
        }
        __syncthreads();
        for (int jj = 0; jj < m; jj++) {
            const float4 t = tile[jj];
            const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
            const float d = (dx * dx + dy * dy) + dz * dz;
            if (d < ld[kCloudK - 1]) {
                ld[kCloudK - 1] = d; li[kCloudK - 1] = base + jj;
#pragma unroll
                for (int r = kCloudK - 1; r > 0; r--) {
                    const bool sw = ld[r] < ld[r - 1];
                    const float d0 = ld[r - 1], d1 = ld[r];
                    const int i0 = li[r - 1], i1 = li[r];
                    ld[r - 1] = sw ? d1 : d0; ld[r] = sw ? d0 : d1;
                    li[r - 1] = sw ? i1 : i0; li[r] = sw ? i0 : i1;
                }
            }
        }
    }
    if (!live) return;
    double sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
#pragma unroll
    for (int r = 0; r < kCloudK; r++) {
        if (r < k) {
            const float* s = P + 3 * (size_t)li[r];
            const double x = s[0], y = s[1], z = s[2];
            sx += x; sy += y; sz += z;
            sxx += x * x; sxy += x * y; sxz += x * z; syy += y * y; syz += y * z; szz += z * z;
        }
    }
    const double kk = (double)k;
    const double mx = sx / kk, my = sy / kk, mz = sz / kk;
    double a00 = sxx / kk - mx * mx, a01 = sxy / kk - mx * my, a02 = sxz / kk - mx * mz;
    double a11 = syy / kk - my * my, a12 = syz / kk - my * mz, a22 = szz / kk - mz * mz;
    double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
    for (int sweep = 0; sweep < UZL_CLOUD_JACOBI_SWEEPS; sweep++) {
        jacobi(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        jacobi(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        jacobi(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    double nx = v00, ny = v10, nz = v20, e = a00;
    if (a11 < e) { nx = v01; ny = v11; nz = v21; e = a11; }
    if (a22 < e) { nx = v02; ny = v12; nz = v22; }
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / len; ny = ny / len; nz = nz / len;
    const double w = 1.0 - gicp_epsilon;
    double* C = cov + 6 * (size_t)(rec.off + i);
    C[0] = 1.0 - (w * nx) * nx; C[1] = 0.0 - (w * nx) * ny; C[2] = 0.0 - (w * nx) * nz;
    C[3] = 1.0 - (w * ny) * ny; C[4] = 0.0 - (w * ny) * nz; C[5] = 1.0 - (w * nz) * nz;
}

// ------------------------------------------------------------------------------------------------ step 5
__global__ __launch_bounds__(kCloudBlock) void cloud_prepare_kernel(CloudIcpArgs a)
{
    const CloudPairRec& P = a.pairs[blockIdx.y];
    const CloudRec to = a.clouds[P.to];
    const int i = blockIdx.x * kCloudBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        CloudPairState& S = a.state[blockIdx.y];
        for (int k = 0; k < 12; k++) S.T[k] = P.T0[k];
        S.done = 0; S.iterations = 0; S.status = UZL_CLOUD_OK; S.num_corr = 0;
        for (int k = 0; k < UZL_CLOUD_MAX_ITERATIONS; k++) S.num_corr_iter[k] = 0;
    }
    if (i >= to.n) return;
    float g[12];
#pragma unroll
    for (int k = 0; k < 12; k++) g[k] = (float)P.G[k];
    const float* p = a.xyz + 3 * (size_t)(to.off + i);
    const float* c = a.lab + 3 * (size_t)(to.off + i);
    const float x = p[0], y = p[1], z = p[2];
    float4* out = reinterpret_cast<float4*>(a.tgt + 8 * (size_t)(P.tgt_off + i));
    out[0] = make_float4(((g[0] * x + g[1] * y) + g[2] * z) + g[3], ((g[4] * x + g[5] * y) + g[6] * z) + g[7],
                         ((g[8] * x + g[9] * y) + g[10] * z) + g[11], 0.f);
    out[1] = make_float4(a.lab_weight * c[0], a.lab_weight * c[1], a.lab_weight * c[2], 0.f);
}

// ------------------------------------------------------------------------------------------------ step 6: the search
__global__ __launch_bounds__(kCloudBlock) void cloud_nn6_kernel(CloudIcpArgs a)
{
    __shared__ float4 tile[2 * kCloudTile];
    const CloudPairState& S = a.state[blockIdx.y];
    if (S.done) return;
    const CloudPairRec& P = a.pairs[blockIdx.y];
    const CloudRec from = a.clouds[P.from];
    if ((int)blockIdx.x * kCloudBlock >= from.n) return;
    const int nt = a.clouds[P.to].n;
    const int tid = threadIdx.x, i = blockIdx.x * kCloudBlock + tid;
    const bool live = i < from.n;
    const int ic = live ? i : from.n - 1;
    float t[12];
#pragma unroll
    for (int k = 0; k < 12; k++) t[k] = (float)S.T[k];
    const float* p = a.xyz + 3 * (size_t)(from.off + ic);
    const float* c = a.lab + 3 * (size_t)(from.off + ic);
    const float x = p[0], y = p[1], z = p[2];
    const float qx = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
    const float qy = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
    const float qz = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
    const float qL = a.lab_weight * c[0], qa = a.lab_weight * c[1], qb = a.lab_weight * c[2];
    const float4* T = reinterpret_cast<const float4*>(a.tgt + 8 * (size_t)P.tgt_off);
    float best = __builtin_inff();
    int bj = 0;
    for (int base = 0; base < nt; base += kCloudTile) {
        const int m = min(kCloudTile, nt - base);
        __syncthreads();
        for (int j = tid; j < 2 * m; j += kCloudBlock) tile[j] = T[2 * (size_t)base + j];
        __syncthreads();
#pragma unroll 4
        for (int jj = 0; jj < m; jj++) {
            const float4 u = tile[2 * jj], v = tile[2 * jj + 1];
            const float dx = qx - u.x, dy = qy - u.y, dz = qz - u.z, dL = qL - v.x, da = qa - v.y, db = qb - v.z;
            const float d = ((((dx * dx + dy * dy) + dz * dz) + dL * dL) + da * da) + db * db;
            if (d < best) { best = d; bj = base + jj; }
        }
    }
    if (!live) return;
    a.nn_j[P.src_off + i] = bj;
    a.nn_d[P.src_off + i] = best;
}

// ------------------------------------------------------------------------------------------------ steps 6-8: the step
struct StepLds {
    double red[kCloudBlock / 64][kCloudSums];
    int cnt[kCloudBlock / 64];
};

__device__ inline double wave_tree(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// H, g and f at the pose (R, t) over the kept correspondences; every thread returns the same 28 sums.
__device__ void cloud_eval(const CloudIcpArgs& a, const CloudPairRec& P, const CloudRec& from, const double* T, StepLds& l, double* S)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < kCloudSums; k++) S[k] = 0.0;
    for (int i = tid; i < from.n; i += kCloudBlock) {
        if (!((double)a.nn_d[P.src_off + i] < a.max_corr_sq)) continue;
        const int j = a.nn_j[P.src_off + i];
        const float* p = a.xyz + 3 * (size_t)(from.off + i);
        const float* q = a.tgt + 8 * (size_t)(P.tgt_off + j);
        const double* M = a.M + 6 * (size_t)(P.src_off + i);
        const double x = p[0], y = p[1], z = p[2];
        const double ax = (T[0] * x + T[1] * y) + T[2] * z, ay = (T[4] * x + T[5] * y) + T[6] * z, az = (T[8] * x + T[9] * y) + T[10] * z;
        const double dx = (ax + T[3]) - (double)q[0], dy = (ay + T[7]) - (double)q[1], dz = (az + T[11]) - (double)q[2];
        const double m00 = M[0], m01 = M[1], m02 = M[2], m11 = M[3], m12 = M[4], m22 = M[5];
        const double ex = (m00 * dx + m01 * dy) + m02 * dz, ey = (m01 * dx + m11 * dy) + m12 * dz, ez = (m02 * dx + m12 * dy) + m22 * dz;
        // A = [a]x M, row r, column c = (a x M[:, c])[r]
        const double A00 = ay * m02 - az * m01, A01 = ay * m12 - az * m11, A02 = ay * m22 - az * m12;
        const double A10 = az * m00 - ax * m02, A11 = az * m01 - ax * m12, A12 = az * m02 - ax * m22;
        const double A20 = ax * m01 - ay * m00, A21 = ax * m11 - ay * m01, A22 = ax * m12 - ay * m02;
        // H_ww row r = a x A[r, :]
        S[0] += ay * A02 - az * A01; S[1] += az * A00 - ax * A02; S[2] += ax * A01 - ay * A00;
        S[3] += az * A10 - ax * A12; S[4] += ax * A11 - ay * A10;
        S[5] += ax * A21 - ay * A20;
        S[6] += A00; S[7] += A01; S[8] += A02; S[9] += A10; S[10] += A11; S[11] += A12; S[12] += A20; S[13] += A21; S[14] += A22;
        S[15] += m00; S[16] += m01; S[17] += m02; S[18] += m11; S[19] += m12; S[20] += m22;
        S[21] += ay * ez - az * ey; S[22] += az * ex - ax * ez; S[23] += ax * ey - ay * ex;
        S[24] += ex; S[25] += ey; S[26] += ez;
        S[27] += (dx * ex + dy * ey) + dz * ez;
    }
    __syncthreads();                                        // the previous reduction's readers are done with red
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < kCloudSums; k++) {
        const double v = wave_tree(S[k]);
        if (lane == 0) l.red[wave][k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCloudSums; k++) S[k] = (l.red[0][k] + l.red[1][k]) + (l.red[2][k] + l.red[3][k]);
}

// (H + mu diag H) delta = -g by a 6x6 Cholesky; false when a pivot is not positive.
__device__ inline bool cloud_solve(const double* S, double mu, double* delta)
{
    // upper triangle of H from the 21 sums: w = 0..2, v = 3..5
    double H[6][6];
    H[0][0] = S[0]; H[0][1] = S[1]; H[0][2] = S[2]; H[1][1] = S[3]; H[1][2] = S[4]; H[2][2] = S[5];
    H[0][3] = S[6]; H[0][4] = S[7]; H[0][5] = S[8]; H[1][3] = S[9]; H[1][4] = S[10]; H[1][5] = S[11];
    H[2][3] = S[12]; H[2][4] = S[13]; H[2][5] = S[14];
    H[3][3] = S[15]; H[3][4] = S[16]; H[3][5] = S[17]; H[4][4] = S[18]; H[4][5] = S[19]; H[5][5] = S[20];
    double L[6][6];
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double d = H[c][c] + mu * H[c][c];
#pragma unroll
        for (int k = 0; k < c; k++) d -= L[c][k] * L[c][k];
        if (!(d > 0.0)) ok = false;
        const double piv = sqrt(d);
        L[c][c] = piv;
#pragma unroll
        for (int r = c + 1; r < 6; r++) {
            double v = H[c][r];
#pragma unroll
            for (int k = 0; k < c; k++) v -= L[r][k] * L[c][k];
            L[r][c] = v / piv;
        }
    }
    double yv[6];
#pragma unroll
    for (int r = 0; r < 6; r++) {
        double v = 0.0 - S[21 + r];
#pragma unroll
        for (int k = 0; k < r; k++) v -= L[r][k] * yv[k];
        yv[r] = v / L[r][r];
    }
#pragma unroll
    for (int r = 5; r >= 0; r--) {
        double v = yv[r];
#pragma unroll
        for (int k = r + 1; k < 6; k++) v -= L[k][r] * delta[k];
        delta[r] = v / L[r][r];
    }
#pragma unroll
    for (int r = 0; r < 6; r++) if (!(fabs(delta[r]) <= 1.7976931348623157e308)) ok = false;
    return ok;
}

// T' = [dR(w) | v] applied on the left: R' = dR R, t' = t + v, dR the rotation of the unit quaternion (1, w / 2) / |.|
__device__ inline void cloud_apply(const double* T, const double* delta, double* Tn)
{
    const double hx = delta[0] / 2.0, hy = delta[1] / 2.0, hz = delta[2] / 2.0;
    const double nrm = sqrt(((1.0 + hx * hx) + hy * hy) + hz * hz);
    const double qw = 1.0 / nrm, qx = hx / nrm, qy = hy / nrm, qz = hz / nrm;
    const double D[9] = {1.0 - 2.0 * (qy * qy + qz * qz), 2.0 * (qx * qy - qw * qz), 2.0 * (qx * qz + qw * qy),
                         2.0 * (qx * qy + qw * qz), 1.0 - 2.0 * (qx * qx + qz * qz), 2.0 * (qy * qz - qw * qx),
                         2.0 * (qx * qz - qw * qy), 2.0 * (qy * qz + qw * qx), 1.0 - 2.0 * (qx * qx + qy * qy)};
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Tn[4 * r + c] = (D[3 * r] * T[c] + D[3 * r + 1] * T[4 + c]) + D[3 * r + 2] * T[8 + c];
        Tn[4 * r + 3] = T[4 * r + 3] + delta[3 + r];
    }
}

#ifdef UZL_DIAG
// Trial s of the launch into the diagnostic log: thread 0 writes (every thread holds the same values); delta == NULL: a refused trial.
__device__ inline void cloud_log_trial(const CloudIcpArgs& a, int s, double mu, int outcome, const double* delta, double f)
{
    if (!a.log || threadIdx.x != 0 || s >= kCloudLogTrials) return;
    double* e = a.log->trial[s];
    e[0] = mu; e[1] = (double)outcome;
    for (int k = 0; k < 6; k++) e[2 + k] = delta ? delta[k] : 0.0;
    e[8] = f;
    a.log->n_trials = s + 1;
}
#endif

__global__ __launch_bounds__(kCloudBlock) void cloud_step_kernel(CloudIcpArgs a)
{
    __shared__ StepLds l;
    CloudPairState& st = a.state[blockIdx.x];
    if (st.done) return;
    const CloudPairRec& P = a.pairs[blockIdx.x];
    const CloudRec from = a.clouds[P.from], to = a.clouds[P.to];
    const int tid = threadIdx.x;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; k++) T[k] = st.T[k];
    const int it = st.iterations;
    // M_i = (R C1_i R^T + R0 C2_j R0^T)^-1, upper triangle
    int cnt = 0;
    for (int i = tid; i < from.n; i += kCloudBlock) {
        if (!((double)a.nn_d[P.src_off + i] < a.max_corr_sq)) continue;
        cnt++;
        const int j = a.nn_j[P.src_off + i];
        double Sm[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const double* C = a.cov + 6 * (size_t)(half == 0 ? from.off + i : to.off + j);
            const double* R = half == 0 ? T : P.G;
            const double c[9] = {C[0], C[1], C[2], C[1], C[3], C[4], C[2], C[4], C[5]};
            double A[9];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int cc = 0; cc < 3; cc++) A[3 * r + cc] = (R[4 * r] * c[cc] + R[4 * r + 1] * c[3 + cc]) + R[4 * r + 2] * c[6 + cc];
            int o = 0;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int cc = r; cc < 3; cc++, o++)
                    Sm[o] = Sm[o] + ((A[3 * r] * R[4 * cc] + A[3 * r + 1] * R[4 * cc + 1]) + A[3 * r + 2] * R[4 * cc + 2]);
        }
        const double s00 = Sm[0], s01 = Sm[1], s02 = Sm[2], s11 = Sm[3], s12 = Sm[4], s22 = Sm[5];
        const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
        const double c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
        const double det = (s00 * c00 + s01 * c01) + s02 * c02;
        double* M = a.M + 6 * (size_t)(P.src_off + i);
        M[0] = c00 / det; M[1] = c01 / det; M[2] = c02 / det; M[3] = c11 / det; M[4] = c12 / det; M[5] = c22 / det;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((tid & 63) == 0) l.cnt[tid >> 6] = cnt;
    __syncthreads();                                        // also: every M is written before cloud_eval reads it (each lane reads its own)
    cnt = (l.cnt[0] + l.cnt[1]) + (l.cnt[2] + l.cnt[3]);
    if (cnt == 0) {
        if (tid == 0) { st.num_corr_iter[it] = 0; st.num_corr = 0; st.status = UZL_CLOUD_NO_CORR; st.done = 1; }
        return;
    }
    double S[kCloudSums], Sn[kCloudSums], Tn[12], delta[6];
    cloud_eval(a, P, from, T, l, S);
#ifdef UZL_DIAG
    if (a.log && tid == 0) for (int k = 0; k < kCloudSums; k++) a.log->sums[k] = S[k];
#endif
    double mu = UZL_CLOUD_MU0;
    for (int s = 0; s < a.inner_iterations; s++) {
        if (!cloud_solve(S, mu, delta)) {
#ifdef UZL_DIAG
            cloud_log_trial(a, s, mu, 0, nullptr, 0.0);
#endif
            mu = mu * 10.0;
            continue;
        }
        cloud_apply(T, delta, Tn);
        cloud_eval(a, P, from, Tn, l, Sn);
#ifdef UZL_DIAG
        cloud_log_trial(a, s, mu, Sn[27] <= S[27] ? 1 : 2, delta, Sn[27]);
#endif
        if (Sn[27] <= S[27]) {
#pragma unroll
            for (int k = 0; k < 12; k++) T[k] = Tn[k];
#pragma unroll
            for (int k = 0; k < kCloudSums; k++) S[k] = Sn[k];
            mu = fmax(mu / 10.0, UZL_CLOUD_MU_MIN);
        } else {
            mu = mu * 10.0;
        }
        double big = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) big = fmax(big, fabs(delta[k]));
        if (big < UZL_CLOUD_INNER_EPS) break;
    }
    // step 8
    double dmax = 0.0;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const double e = (k & 3) == 3 ? a.trans_eps : a.rot_eps;
        dmax = fmax(dmax, fabs(st.T[k] - T[k]) / e);
    }
    __syncthreads();                                        // every thread has read st.T
    if (tid == 0) {
        for (int k = 0; k < 12; k++) st.T[k] = T[k];
        st.num_corr_iter[it] = cnt; st.num_corr = cnt;
        st.iterations = it + 1;
        if (dmax < 1.0 || it + 1 >= a.max_iterations) st.done = 1;
    }
    (void)to;
}

}  // namespace

void launch_cloud_lab(const uint8_t* bgr, float* lab, const double* table, int64_t n, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(cloud_lab_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bgr, lab, table, n);
}

void launch_cloud_cov(const CloudRec* recs, int32_t n_clouds, int32_t max_n, const float* xyz, double* cov, int32_t k, double gicp_epsilon,
                      hipStream_t s)
{
    if (n_clouds > 0 && max_n > 0)
        hipLaunchKernelGGL(cloud_cov_kernel, dim3((max_n + kCloudBlock - 1) / kCloudBlock, n_clouds), dim3(kCloudBlock), 0, s, recs, xyz, cov,
                           k, gicp_epsilon);
}

void launch_cloud_prepare(const CloudIcpArgs& a, int32_t n_pairs, int32_t max_to, hipStream_t s)
{
    if (n_pairs > 0) hipLaunchKernelGGL(cloud_prepare_kernel, dim3((max_to + kCloudBlock - 1) / kCloudBlock, n_pairs), dim3(kCloudBlock), 0, s, a);
}

void launch_cloud_nn6(const CloudIcpArgs& a, int32_t n_pairs, int32_t max_from, hipStream_t s)
{
    if (n_pairs > 0) hipLaunchKernelGGL(cloud_nn6_kernel, dim3((max_from + kCloudBlock - 1) / kCloudBlock, n_pairs), dim3(kCloudBlock), 0, s, a);
}

void launch_cloud_step(const CloudIcpArgs& a, int32_t n_pairs, hipStream_t s)
{
    if (n_pairs > 0) hipLaunchKernelGGL(cloud_step_kernel, dim3(n_pairs), dim3(kCloudBlock), 0, s, a);
}

}  // namespace uzl
