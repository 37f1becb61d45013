// depthfilter_kernels.hip — depth refinement and keypoint lifting on gfx950 (contract: include/uzl_mi355x.h, "Depth refinement and
// 3-D keypoint lifting").
//
// depth_refine_kernel: one 256-thread workgroup per (64 x 32 output tile, image); gridDim.z = image, so many small images share one
// launch (a workgroup whose tile lies outside its image leaves at once).  With H = max(R, P):
//   load   the step-1 depth of the tile and an H-pixel halo, indices clamped to the image (BORDER_REPLICATE), as f32 into LDS, the
//          guide beside it as u8, and the two weight tables;
//   pass 1 step 3 for the tile's rows and R halo rows above and below, into LDS;
//   pass 2 step 4 in registers, then step 5 against the depth tile already in LDS.  Step 5 addresses the image by reflection
//          (BORDER_REFLECT_101), which is the clamp only inside the image: the reflected index is computed on its own and always
//          lies inside the image, at most P from the pixel - so inside the loaded tile, where the clamp was the identity.
// Each image is read once and written once; a pixel's value is a fixed sequence of operations on its own window, whatever the tile.
// The kernel exists twice: for the reference's own radii (R = 3, P = 2, the defaults) the taps are unrolled and each lane makes a run
// of 8 pixels along the pass's direction from one window held in registers (8 + 2R loads of depth and guide where 8 (2R + 1) would
// be needed), lanes side by side across the other direction; any other radii take one pixel per lane and loops.  The LDS pitches
// are odd, so lanes that walk down rows and lanes that walk along columns both spread over the banks.  Same operations in the same
// order either way.
// depth_lift_kernel: step 7, one lane per keypoint.
// Built with -ffp-contract=off and correctly rounded f32 divide: every operation rounds as the contract says.
#include "depthfilter_types.hpp"

#include <cfloat>

namespace uzl {

namespace {

// contract step 1
__device__ inline float depth_at(const uint8_t* row, int x, int encoding, double scale)
{
    float d = encoding == UZL_DEPTH_F32_M ? reinterpret_cast<const float*>(row)[x]
                                          : (float)((double)reinterpret_cast<const uint16_t*>(row)[x] * 0.001);
    if (scale != 1.0) d = (float)((double)d * scale);
    return d;
}

// BORDER_REFLECT_101: -1 -> 1, n -> n - 2, repeated while outside; everything -> 0 when n = 1
__device__ inline int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// Steps 3 / 4 for one pixel: the taps are `stride` apart in src and guide, centred on src[0] / guide[0].
__device__ inline float joint_pass(const float* src, int src_stride, const uint8_t* guide, int guide_stride, const float* cw, const float* sw,
                                   int R)
{
    const int g0 = (int)guide[0];
    float t = 0.f, ws = 0.f;
    for (int k = -R; k <= R; k++) {
        const int g = (int)guide[k * guide_stride];
        const float w = sw[k + R] * cw[abs(g - g0)];
        t = t + w * src[k * src_stride];
        ws = ws + w;
    }
    const float w = 0.0f * cw[0];                           // the reference's one tap too many: weight 0 at the centre
    t = t + w * src[0];
    ws = ws + w;
    return t / ws;
}

constexpr int kDepthRun = 8;              // pixels of one lane's run in the unrolled passes

// Step 3 or 4 for a run of kDepthRun pixels from its window (v, g: kDepthRun + 2R values, the first pixel's centre at index R).
template <int R>
__device__ inline void joint_run(const float (&v)[kDepthRun + 2 * R], const int (&g)[kDepthRun + 2 * R], const float* cw,
                                 const float (&sw)[2 * R + 1], float cw0, float (&out)[kDepthRun])
{
#pragma unroll
    for (int p = 0; p < kDepthRun; p++) {
        float t = 0.f, ws = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * R; k++) {
            const float w = sw[k] * cw[abs(g[p + k] - g[p + R])];
            t = t + w * v[p + k];
            ws = ws + w;
        }
        const float w = 0.0f * cw0;                         // the reference's one tap too many: weight 0 at the centre
        t = t + w * v[p + R];
        ws = ws + w;
        out[p] = t / ws;
    }
}

// RT, PT >= 0: the radii at compile time (the launch checks that they are the config's); RT < 0: the config's, in loops.
template <int RT, int PT>
__global__ __launch_bounds__(kDepthBlock) void depth_refine_kernel(DepthRefineArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const DepthImageRec& im = a.images[blockIdx.z];
    const int x0 = (int)blockIdx.x * kDepthTileW, y0 = (int)blockIdx.y * kDepthTileH;
    const int W = im.width, Hh = im.height;
    if (x0 >= W || y0 >= Hh) return;                        // the whole workgroup: this image has fewer tiles
    const int tw = min(kDepthTileW, W - x0), th = min(kDepthTileH, Hh - y0);
    const int tid = (int)threadIdx.x;
    const uint8_t* depth = a.pixels + im.depth_off;
    float* out = a.out + im.out_off;
    if (!a.filter) {                                        // contract step 6
        for (int idx = tid; idx < th * kDepthTileW; idx += kDepthBlock) {
            const int c = idx % kDepthTileW, y = y0 + idx / kDepthTileW;
            if (c < tw) out[(size_t)y * W + x0 + c] = depth_at(depth + (size_t)y * im.depth_step, x0 + c, im.encoding, a.depth_scale);
        }
        return;
    }
    const int R = RT >= 0 ? RT : a.radius, P = RT >= 0 ? PT : a.nearest, halo = max(R, P);
    const int dw = depth_pitch(R, P), dh = kDepthTileH + 2 * halo;                  // the LDS tile's pitch and rows
    float* sd = reinterpret_cast<float*>(lds);                                      // depth, dh x dw
    float* sh = sd + dw * dh;                                                       // pass 1, (kDepthTileH + 2R) x kDepthPitchH
    float* cw = sh + kDepthPitchH * (kDepthTileH + 2 * R);
    float* sw = cw + kDepthColours;
    uint8_t* sg = reinterpret_cast<uint8_t*>(sw + 2 * R + 1);                       // guide, dh x dw
    const uint8_t* guide = a.pixels + im.guide_off;

    for (int k = tid; k < kDepthColours + 2 * R + 1; k += kDepthBlock) cw[k] = a.tables[k];
    const int lw = tw + 2 * halo, lh = th + 2 * halo;       // the part of the LDS tile this workgroup's pixels reach
    for (int idx = tid; idx < lw * lh; idx += kDepthBlock) {
        const int r = idx / lw, c = idx - r * lw;
        const int y = min(max(y0 - halo + r, 0), Hh - 1), x = min(max(x0 - halo + c, 0), W - 1);
        sd[r * dw + c] = depth_at(depth + (size_t)y * im.depth_step, x, im.encoding, a.depth_scale);
        sg[r * dw + c] = guide[(size_t)y * im.guide_step + x];
    }
    __syncthreads();
    if constexpr (RT >= 0) {
        float swr[2 * RT + 1];
#pragma unroll
        for (int k = 0; k <= 2 * RT; k++) swr[k] = sw[k];
        const float cw0 = cw[0];
        // pass 1: lanes down the rows, each a run of columns
        const int nrows = th + 2 * RT;
        for (int item = tid; item < nrows * (kDepthTileW / kDepthRun); item += kDepthBlock) {
            const int r = item % nrows, c0 = item / nrows * kDepthRun;
            if (c0 >= tw) continue;
            const int at = (r + halo - RT) * dw + c0 + halo - RT;
            float v[kDepthRun + 2 * RT], f[kDepthRun];
            int g[kDepthRun + 2 * RT];
#pragma unroll
            for (int q = 0; q < kDepthRun + 2 * RT; q++) { v[q] = sd[at + q]; g[q] = (int)sg[at + q]; }
            joint_run<RT>(v, g, cw, swr, cw0, f);
#pragma unroll
            for (int p = 0; p < kDepthRun; p++)
                if (c0 + p < tw) sh[r * kDepthPitchH + c0 + p] = f[p];
        }
        __syncthreads();
        // pass 2 and the snap: lanes along the columns, each a run of rows
        for (int item = tid; item < kDepthTileW * (kDepthTileH / kDepthRun); item += kDepthBlock) {
            const int c = item % kDepthTileW, r0 = item / kDepthTileW * kDepthRun;
            if (c >= tw || r0 >= th) continue;
            float v[kDepthRun + 2 * RT], f[kDepthRun];
            int g[kDepthRun + 2 * RT];
#pragma unroll
            for (int q = 0; q < kDepthRun + 2 * RT; q++) {
                v[q] = sh[(r0 + q) * kDepthPitchH + c];
                g[q] = (int)sg[(r0 + halo - RT + q) * dw + c + halo];
            }
            joint_run<RT>(v, g, cw, swr, cw0, f);
            int col[2 * PT + 1];
#pragma unroll
            for (int j = 0; j <= 2 * PT; j++) col[j] = reflect101(x0 + c + j - PT, W) - x0 + halo;
#pragma unroll
            for (int p = 0; p < kDepthRun; p++) {
                const int y = y0 + r0 + p;
                if (y >= Hh) break;
                float minv = FLT_MAX, best = 0.0f;
#pragma unroll
                for (int i = -PT; i <= PT; i++) {
                    const int row = (reflect101(y + i, Hh) - y0 + halo) * dw;
#pragma unroll
                    for (int j = -PT; j <= PT; j++) {
                        if (i * i + j * j > PT * PT) continue;
                        const float b = sd[row + col[j + PT]];
                        const float d = fabsf(b - f[p]);
                        if (d < minv) { minv = d; best = b; }
                    }
                }
                out[(size_t)y * W + x0 + c] = best;
            }
        }
        return;
    }
    // pass 1: row r of sh is image row clamp(y0 - R + r), LDS row r + halo - R
    for (int idx = tid; idx < (th + 2 * R) * kDepthTileW; idx += kDepthBlock) {
        const int c = idx % kDepthTileW, r = idx / kDepthTileW;
        if (c >= tw) continue;
        const int at = (r + halo - R) * dw + c + halo;
        sh[r * kDepthPitchH + c] = joint_pass(sd + at, 1, sg + at, 1, cw, sw, R);
    }
    __syncthreads();
    // pass 2 and the snap
    for (int idx = tid; idx < th * kDepthTileW; idx += kDepthBlock) {
        const int c = idx % kDepthTileW, r = idx / kDepthTileW;
        if (c >= tw) continue;
        const int x = x0 + c, y = y0 + r;
        const float f = joint_pass(sh + (r + R) * kDepthPitchH + c, kDepthPitchH, sg + (r + halo) * dw + c + halo, dw, cw, sw, R);
        float minv = FLT_MAX, best = 0.0f;
        for (int i = -P; i <= P; i++) {
            const int row = (reflect101(y + i, Hh) - y0 + halo) * dw;
            for (int j = -P; j <= P; j++) {
                if (i * i + j * j > P * P) continue;        // sqrt(i i + j j) <= P
                const float b = sd[row + reflect101(x + j, W) - x0 + halo];
                const float d = fabsf(b - f);
                if (d < minv) { minv = d; best = b; }
            }
        }
        out[(size_t)y * W + x] = best;
    }
}

__global__ __launch_bounds__(kDepthLiftBlock) void depth_lift_kernel(DepthLiftArgs a)
{
    const int i = (int)(blockIdx.x * kDepthLiftBlock + threadIdx.x);
    if (i >= a.n) return;
    const int u = min(max(a.u[i], 0), a.width - 1), v = min(max(a.v[i], 0), a.height - 1);
    const double d = (double)a.image[(size_t)v * a.width + u];
    const bool valid = d != 0.0 && !isnan(d) && (a.max_depth == 0.0 || d <= a.max_depth);
    double x = 0.0, y = 0.0, z = -1.0;
    if (valid) {
        x = (((double)u - a.cx) * d) / a.fx;
        y = (((double)v - a.cy) * d) / a.fy;
        z = d;
    }
    a.pos[3 * (size_t)i] = x;
    a.pos[3 * (size_t)i + 1] = y;
    a.pos[3 * (size_t)i + 2] = z;
    a.valid[i] = valid ? 1 : 0;
}

}  // namespace

void launch_depth_refine(const DepthRefineArgs& a, int tiles_x, int tiles_y, int n_images, hipStream_t s)
{
    if (tiles_x <= 0 || tiles_y <= 0 || n_images <= 0) return;
    const dim3 grid(tiles_x, tiles_y, n_images);
    const size_t lds = depth_refine_lds(a.radius, a.nearest);
    if (a.radius == 3 && a.nearest == 2) hipLaunchKernelGGL((depth_refine_kernel<3, 2>), grid, dim3(kDepthBlock), lds, s, a);
    else hipLaunchKernelGGL((depth_refine_kernel<-1, -1>), grid, dim3(kDepthBlock), lds, s, a);
}

void launch_depth_lift(const DepthLiftArgs& a, hipStream_t s)
{
    if (a.n > 0) hipLaunchKernelGGL(depth_lift_kernel, dim3((a.n + kDepthLiftBlock - 1) / kDepthLiftBlock), dim3(kDepthLiftBlock), 0, s, a);
}

}  // namespace uzl
