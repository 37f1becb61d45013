// orb_kernels.hip — ORB keypoints, descriptors and binary GIST on gfx950 (contract: include/uzl_mi355x.h, "ORB keypoints,
// descriptors and binary GIST").
//
// A unit is one image as a detector sees it: a grid cell (steps 2-8) or the whole image (steps 9-10).  Every kernel indexes its grid
// by unit or image, level and tile, so a call's launch count does not depend on the number of images; a workgroup whose tile or
// candidate block lies outside its unit leaves at once, one whose unit has more tiles than the grid has rows strides over them.
//   orb_resize_kernel       step 3: level l of every unit, image and mask, from level l - 1 (one launch per level above 0)
//   orb_gist_resize_kernel  step 11: the whole image to 63 x 63, one workgroup per image
//   orb_fast_kernel         steps 4-5: one workgroup per 64 x 32 tile of the region the border leaves.  The u8 tile with a 4-pixel
//                           halo goes to LDS, the scores of the tile and one pixel around it (arc min / max form, in registers, for
//                           the pixels the compass test lets through; scores below the threshold are kept as 0) go to LDS, the 3 x 3 test and the mask follow; survivors are collected in LDS, one global atomic per
//                           workgroup reserves their place and an integer atomic per survivor counts its score's bin
//   orb_cut_kernel          steps 6 and 8: one workgroup per cell, one lane per bin; a suffix scan of the level's histogram gives
//                           the level's cut, of the survivors' joint histogram the cell's
//   orb_orient_kernel       step 7 and the coordinates of step 8: one wave per 64 candidates; the kept ones (ballot) are taken one
//                           after the other, all 64 lanes summing the patch's integer moments; one atomic per wave reserves their
//                           place in the image's list
//   orb_order_kernel        the order of step 8: each keypoint's rank is the number of smaller keys, the image's keys passing
//                           through LDS 256 at a time.  The key is total, so the arrival order leaves no trace
//   orb_blur_kernel         step 10 for every level of every whole image and the 63 x 63 image: tile with a 3-pixel reflected halo
//                           in LDS, rows then columns, each lane a run of 8 pixels from one window held in registers
//   orb_describe_kernel     step 9 and the descriptor of step 11: one wave per keypoint, 4 bits per lane
// The LDS pitches are odd in 32-bit words.  Integer sums and integer atomics only where order could matter: nothing depends on the
// schedule.  Built with -ffp-contract=off and correctly rounded f32 divide.
#include "orb_types.hpp"

#include <cfloat>

namespace uzl {

namespace {

// BORDER_REFLECT_101: -1 -> 1, n -> n - 2, repeated while outside; everything -> 0 when n = 1
__device__ inline int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;
    return p;
}

// cvRound of an f32: half to even
__device__ inline int rnd(float x) { return (int)rintf(x); }

__device__ inline int sat_s16(int v) { return min(max(v, -32768), 32767); }

// contract step 3, one axis: the left tap, the right tap and their weights
__device__ inline void resize_taps(int d, int dn, int sn, int* s0, int* s1, int* w0, int* w1)
{
    const double scale = 1.0 / ((double)dn / (double)sn);
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= sn - 1) { s = sn - 1; f = 0.f; }
    *s0 = s; *s1 = min(s + 1, sn - 1);
    *w0 = sat_s16(rnd((1.f - f) * 2048.f));
    *w1 = sat_s16(rnd(f * 2048.f));
}

// one pixel from its column taps (x0, x1, a0, a1) and its row taps
__device__ inline uint8_t resize_from_taps(const uint8_t* src, int sstep, int x0, int x1, int a0, int a1, int y0, int y1, int b0, int b1)
{
    const uint8_t* r0 = src + (size_t)y0 * sstep;
    const uint8_t* r1 = src + (size_t)y1 * sstep;
    const int h0 = (int)r0[x0] * a0 + (int)r0[x1] * a1, h1 = (int)r1[x0] * a0 + (int)r1[x1] * a1;
    return (uint8_t)min(max((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2, 0), 255);
}

__device__ inline uint8_t resize_pixel(const uint8_t* src, int sstep, int sw, int sh, int dw, int dh, int dx, int dy)
{
    int x0, x1, a0, a1, y0, y1, b0, b1;
    resize_taps(dx, dw, sw, &x0, &x1, &a0, &a1);
    resize_taps(dy, dh, sh, &y0, &y1, &b0, &b1);
    return resize_from_taps(src, sstep, x0, x1, a0, a1, y0, y1, b0, b1);
}

__global__ __launch_bounds__(kOrbBlock) void orb_resize_kernel(OrbArgs a, int level)
{
    const OrbUnit& un = a.units[blockIdx.x];
    const int plane = (int)blockIdx.z;                      // 0: image, 1: mask
    if (plane == 1 && !un.has_mask) return;
    const OrbLevel& d = un.lev[level];
    const OrbLevel& s = un.lev[level - 1];
    const uint8_t* src = (level == 1 ? a.pixels : a.pyr) + (plane ? s.mask_off : s.img_off);
    const int sstep = plane ? s.mask_step : s.step, dstep = plane ? d.mask_step : d.step;
    uint8_t* dst = a.pyr + (plane ? d.mask_off : d.img_off);
    const int tiles_x = (d.w + kOrbTileW - 1) / kOrbTileW, tiles = tiles_x * ((d.h + kOrbTileH - 1) / kOrbTileH);
    const int cx = (int)threadIdx.x % kOrbTileW, ry = (int)threadIdx.x / kOrbTileW;   // a lane keeps its column: the column taps once
    for (int t = (int)blockIdx.y; t < tiles; t += (int)gridDim.y) {
        const int x = t % tiles_x * kOrbTileW + cx, y0 = t / tiles_x * kOrbTileH;
        if (x >= d.w) continue;
        int sx0, sx1, a0, a1;
        resize_taps(x, d.w, s.w, &sx0, &sx1, &a0, &a1);
        for (int y = y0 + ry; y < min(y0 + kOrbTileH, d.h); y += kOrbBlock / kOrbTileW) {
            int sy0, sy1, b0, b1;
            resize_taps(y, d.h, s.h, &sy0, &sy1, &b0, &b1);
            dst[(size_t)y * dstep + x] = resize_from_taps(src, sstep, sx0, sx1, a0, a1, sy0, sy1, b0, b1);
        }
    }
}

__global__ __launch_bounds__(kOrbBlock) void orb_gist_resize_kernel(OrbArgs a)
{
    const OrbImage& im = a.images[blockIdx.x];
    if (im.width == 0) return;
    const OrbLevel& s = a.units[im.whole].lev[0];
    uint8_t* dst = a.pyr + im.gist_off;
    for (int idx = (int)threadIdx.x; idx < kOrbGist * kOrbGist; idx += kOrbBlock)
        dst[idx] = resize_pixel(a.pixels + s.img_off, s.step, s.w, s.h, kOrbGist, kOrbGist, idx % kOrbGist, idx / kOrbGist);
}

// contract step 4: the largest t at which 9 contiguous circle pixels are all brighter than p + t or all darker than p - t.  With
// e = sign * (I - p) an arc qualifies at every t < min(e), so one side's best is the largest of the 16 arc minima; arcs of 9 from
// arcs of 2, 4 and 8.
__device__ inline int fast_arcs(const int (&d)[16], int sign)
{
    int e[16], lo2[16], lo4[16], lo8[16];
#pragma unroll
    for (int k = 0; k < 16; k++) e[k] = sign * d[k];
#pragma unroll
    for (int k = 0; k < 16; k++) lo2[k] = min(e[k], e[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) lo4[k] = min(lo2[k], lo2[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) lo8[k] = min(lo4[k], lo4[(k + 4) & 15]);
    int best = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) best = max(best, min(lo8[k], e[(k + 8) & 15]));
    return best;
}

// brighter / darker: the sides on which an arc can exist at all (the caller's compass test); the score is the best arc's value less one
__device__ inline int fast_score(const uint8_t* c, int pitch, bool brighter, bool darker)
{
    const int p = (int)c[0];
    int d[16];
    d[0] = c[3 * pitch]; d[1] = c[3 * pitch + 1]; d[2] = c[2 * pitch + 2]; d[3] = c[pitch + 3];
    d[4] = c[3]; d[5] = c[-pitch + 3]; d[6] = c[-2 * pitch + 2]; d[7] = c[-3 * pitch + 1];
    d[8] = c[-3 * pitch]; d[9] = c[-3 * pitch - 1]; d[10] = c[-2 * pitch - 2]; d[11] = c[-pitch - 3];
    d[12] = c[-3]; d[13] = c[pitch - 3]; d[14] = c[2 * pitch - 2]; d[15] = c[3 * pitch - 1];
#pragma unroll
    for (int k = 0; k < 16; k++) d[k] -= p;
    int best = fast_arcs(d, brighter ? 1 : -1);             // one pass serves the lanes of either side
    if (brighter && darker) best = max(best, fast_arcs(d, -1));
    return max(best - 1, 0);
}

__global__ __launch_bounds__(kOrbBlock) void orb_fast_kernel(OrbArgs a)
{
    __shared__ __attribute__((aligned(4))) uint8_t sp[(kOrbTileH + 2 * kOrbFastHalo) * kOrbFastPitch];
    __shared__ __attribute__((aligned(4))) uint8_t ss[(kOrbTileH + 2) * kOrbScorePitch];
    __shared__ uint2 found_xy[kOrbTileW * kOrbTileH / 4];   // strict 3 x 3 maxima: at most one per 2 x 2 block
    __shared__ uint8_t found_score[kOrbTileW * kOrbTileH / 4];
    __shared__ uint32_t n_found, base;
    const OrbUnit& un = a.units[blockIdx.x];
    const int level = (int)blockIdx.z, job = (int)blockIdx.x * a.n_levels + level;
    const OrbLevel& lv = un.lev[level];
    const int e = a.edge, W = lv.w, H = lv.h, rw = W - 2 * e, rh = H - 2 * e;
    if (rw <= 0 || rh <= 0) return;                         // contract step 5: the level keeps nothing
    const uint8_t* img = (level == 0 ? a.pixels : a.pyr) + lv.img_off;
    const uint8_t* mask = un.has_mask ? (level == 0 ? a.pixels : a.pyr) + lv.mask_off : nullptr;
    const int tiles_x = (rw + kOrbTileW - 1) / kOrbTileW, tiles = tiles_x * ((rh + kOrbTileH - 1) / kOrbTileH);
    const int tid = (int)threadIdx.x;
    for (int t = (int)blockIdx.y; t < tiles; t += (int)gridDim.y) {
        const int x0 = e + t % tiles_x * kOrbTileW, y0 = e + t / tiles_x * kOrbTileH;     // e >= 19: the halo stays inside
        const int tw = min(kOrbTileW, W - e - x0), th = min(kOrbTileH, H - e - y0);
        if (tid == 0) n_found = 0;
        for (int idx = tid; idx < (kOrbTileH + 2 * kOrbFastHalo) * (kOrbTileW + 2 * kOrbFastHalo); idx += kOrbBlock) {
            const int r = idx / (kOrbTileW + 2 * kOrbFastHalo), c = idx - r * (kOrbTileW + 2 * kOrbFastHalo);
            const int y = min(y0 - kOrbFastHalo + r, H - 1), x = min(x0 - kOrbFastHalo + c, W - 1);   // past a cut tile: unused
            sp[r * kOrbFastPitch + c] = img[(size_t)y * lv.step + x];
        }
        __syncthreads();
        // scores of the tile and one pixel around it: rows y0 - 1 .. y0 + th, all within [3, H - 3)
        for (int idx = tid; idx < (kOrbTileH + 2) * (kOrbTileW + 2); idx += kOrbBlock) {
            const int r = idx / (kOrbTileW + 2), c = idx - r * (kOrbTileW + 2);
            int s = 0;
            if (r <= th + 1 && c <= tw + 1) {
                // An arc of 9 holds at least two of the four compass pixels.  Without two of them beyond the threshold on one side the
                // score is below it, and such a score is kept as 0: it neither makes a keypoint nor outranks one.
                const uint8_t* q = sp + (r + 3) * kOrbFastPitch + c + 3;
                const int p = (int)q[0], t = a.fast_threshold;                 // score >= t iff an arc lies beyond t
                const int d0 = (int)q[3 * kOrbFastPitch] - p, d1 = (int)q[3] - p, d2 = (int)q[-3 * kOrbFastPitch] - p, d3 = (int)q[-3] - p;
                const int up = (d0 > t) + (d1 > t) + (d2 > t) + (d3 > t), down = (d0 < -t) + (d1 < -t) + (d2 < -t) + (d3 < -t);
                if (up >= 2 || down >= 2) s = fast_score(q, kOrbFastPitch, up >= 2, down >= 2);
                if (s < a.fast_threshold) s = 0;
            }
            ss[r * kOrbScorePitch + c] = (uint8_t)s;
        }
        __syncthreads();
        for (int idx = tid; idx < kOrbTileW * kOrbTileH; idx += kOrbBlock) {
            const int r = idx / kOrbTileW, c = idx - r * kOrbTileW;
            if (r >= th || c >= tw) continue;
            const uint8_t* q = ss + (r + 1) * kOrbScorePitch + c + 1;
            const int s = (int)q[0];
            if (s < a.fast_threshold) continue;
            const int m = max(max(max((int)q[-kOrbScorePitch - 1], (int)q[-kOrbScorePitch]), max((int)q[-kOrbScorePitch + 1], (int)q[-1])),
                              max(max((int)q[1], (int)q[kOrbScorePitch - 1]), max((int)q[kOrbScorePitch], (int)q[kOrbScorePitch + 1])));
            if (s <= m) continue;
            const int x = x0 + c, y = y0 + r;
            if (mask && mask[(size_t)y * lv.mask_step + x] == 0) continue;
            const uint32_t k = atomicAdd(&n_found, 1u);
            found_xy[k] = make_uint2((uint32_t)x, (uint32_t)y);
            found_score[k] = (uint8_t)s;
        }
        __syncthreads();
        if (tid == 0 && n_found) base = atomicAdd(&a.n_cand[job], n_found);
        __syncthreads();
        for (uint32_t k = (uint32_t)tid; k < n_found; k += kOrbBlock) {
            if (base + k >= (uint32_t)lv.cand_cap) continue;   // cannot happen: cand_cap is the bound on strict maxima
            a.cand_xy[lv.cand_off + base + k] = found_xy[k];
            a.cand_score[lv.cand_off + base + k] = found_score[k];
            atomicAdd(&a.hist[(size_t)job * kOrbBins + found_score[k]], 1u);
        }
        __syncthreads();
    }
}

// The cut of steps 6 and 8 for the histogram in S (one bin per lane, replaced by its suffix sums): the smallest kept response.
__device__ inline uint32_t cut_of(uint32_t* S, uint32_t* found, uint32_t h, int n, int t)
{
    S[t] = h;
    __syncthreads();
    for (int off = 1; off < kOrbBins; off *= 2) {
        const uint32_t v = t + off < kOrbBins ? S[t + off] : 0u;
        __syncthreads();
        S[t] += v;
        __syncthreads();
    }
    const uint32_t total = S[0];
    uint32_t c = 0;
    if (total > (uint32_t)max(n, 0)) {
        if (n <= 0) c = kOrbBins;                           // nothing is kept
        else {
            if (S[t] >= (uint32_t)n && (t == kOrbBins - 1 || S[t + 1] < (uint32_t)n)) *found = (uint32_t)t;   // the n-th largest
            __syncthreads();
            c = *found;
        }
    }
    __syncthreads();
    return c;
}

__global__ __launch_bounds__(kOrbBins) void orb_cut_kernel(OrbArgs a)
{
    __shared__ uint32_t S[kOrbBins];
    __shared__ uint32_t found;
    const int t = (int)threadIdx.x, unit = (int)blockIdx.x;
    uint32_t cl[kOrbMaxLevels];
    uint32_t hc = 0;
    for (int l = 0; l < a.n_levels; l++) {
        const uint32_t h = a.hist[((size_t)unit * a.n_levels + l) * kOrbBins + t];
        cl[l] = cut_of(S, &found, h, a.n_per_level[l], t);
        if ((uint32_t)t >= cl[l]) hc += h;
    }
    const uint32_t c2 = cut_of(S, &found, hc, a.n_per_cell, t);
    if (t < a.n_levels) a.thr[(size_t)unit * a.n_levels + t] = max(cl[t], c2);
}

__device__ const int8_t kOrbUmax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

// contract step 7
__device__ inline float fast_atan2(float y, float x)
{
    const float scale = (float)(180.0 / 3.14159265358979323846);
    const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale, p5 = 0.1555786518463281f * scale,
                p7 = -0.04432655554792128f * scale;
    const float ax = fabsf(x), ay = fabsf(y);
    float r, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        r = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        r = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0.f) r = 180.f - r;
    if (y < 0.f) r = 360.f - r;
    return r;
}

__global__ __launch_bounds__(kOrbBlock) void orb_orient_kernel(OrbArgs a)
{
    const OrbUnit& un = a.units[blockIdx.x];
    const int level = (int)blockIdx.z, job = (int)blockIdx.x * a.n_levels + level;
    const OrbLevel& lv = un.lev[level];
    const OrbImage& im = a.images[un.image];
    const uint32_t nc = min(a.n_cand[job], (uint32_t)lv.cand_cap), thr = a.thr[job];
    const uint8_t* img = (level == 0 ? a.pixels : a.pyr) + lv.img_off;
    const float sf = a.level_scale[level];
    const int lane = (int)threadIdx.x & 63;
    for (uint32_t first = blockIdx.y * kOrbBlock; first < nc; first += gridDim.y * kOrbBlock) {
        const uint32_t i = first + threadIdx.x;
        int x = 0, y = 0, score = 0;
        float u = 0.f, v = 0.f;
        bool keep = false;
        if (i < nc) {
            const uint2 p = a.cand_xy[lv.cand_off + i];
            x = (int)p.x; y = (int)p.y;
            score = (int)a.cand_score[lv.cand_off + i];
            u = (float)x; v = (float)y;
            if (level != 0) { u = u * sf; v = v * sf; }
            u = u + (float)un.x0; v = v + (float)un.y0;
            const int ru = rnd(u), rv = rnd(v);             // step 9's border test on the whole image
            keep = (uint32_t)score >= thr && ru >= a.edge && ru < im.width - a.edge && rv >= a.edge && rv < im.height - a.edge;
        }
        const unsigned long long kept = __ballot(keep);
        if (!kept) continue;
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&a.count[im.slot], (uint32_t)__popcll(kept));
        at = __shfl(at, 0);
        for (unsigned long long rest = kept; rest; rest &= rest - 1) {
            const int src = __ffsll((long long)rest) - 1;
            const int cx = __shfl(x, src), cy = __shfl(y, src);
            int m01 = 0, m10 = 0;
            for (int idx = lane; idx < 31 * 31; idx += 64) {
                const int dy = idx / 31 - 15, dx = idx - (dy + 15) * 31 - 15;
                if (abs(dx) > kOrbUmax[abs(dy)]) continue;
                const int val = (int)img[(size_t)(cy + dy) * lv.step + cx + dx];
                m10 += dx * val;
                m01 += dy * val;
            }
            for (int off = 32; off; off >>= 1) { m01 += __shfl_xor(m01, off); m10 += __shfl_xor(m10, off); }
            if (lane == src) {
                const uint32_t k = at + (uint32_t)__popcll(kept & ((1ull << src) - 1));
                if (k < (uint32_t)im.kp_cap) {
                    OrbKp o;
                    o.u = u; o.v = v; o.response = (float)score; o.angle = fast_atan2((float)m01, (float)m10); o.octave = level;
                    a.kp_tmp[im.tmp_off + k] = o;
                }
            }
        }
    }
}

// the order of step 8 as three words compared in turn: (octave, 255 - response), v, u (non-negative floats order as their bits)
struct OrbKey { uint32_t k0, k1, k2; };

__device__ inline OrbKey key_of(const OrbKp& p)
{
    return OrbKey{((uint32_t)p.octave << 8) | (uint32_t)(255 - (int)p.response), __float_as_uint(p.v), __float_as_uint(p.u)};
}

__device__ inline bool key_less(const OrbKey& x, const OrbKey& y)
{
    return x.k0 != y.k0 ? x.k0 < y.k0 : x.k1 != y.k1 ? x.k1 < y.k1 : x.k2 < y.k2;
}

__global__ __launch_bounds__(kOrbBlock) void orb_order_kernel(OrbArgs a)
{
    __shared__ OrbKey keys[kOrbBlock];
    const OrbImage& im = a.images[blockIdx.y];
    const uint32_t n = min(a.count[im.slot], (uint32_t)im.kp_cap);
    const OrbKp* in = a.kp_tmp + im.tmp_off;
    for (uint32_t first = blockIdx.x * kOrbBlock; first < n; first += gridDim.x * kOrbBlock) {
        const uint32_t i = first + threadIdx.x;
        OrbKp mine = {};
        OrbKey key = {};
        if (i < n) { mine = in[i]; key = key_of(mine); }
        uint32_t rank = 0;
        for (uint32_t t0 = 0; t0 < n; t0 += kOrbBlock) {
            __syncthreads();
            if (t0 + threadIdx.x < n) keys[threadIdx.x] = key_of(in[t0 + threadIdx.x]);
            __syncthreads();
            const uint32_t m = min((uint32_t)kOrbBlock, n - t0);
            for (uint32_t j = 0; j < m; j++) rank += key_less(keys[j], key) ? 1u : 0u;
        }
        if (i < n) a.kp[im.kp_off + rank] = mine;
    }
}

constexpr int kOrbRun = 8;                // pixels of one lane's run in the blur's passes

// step 10 along one axis for a run of kOrbRun pixels from its window of kOrbRun + 6 values
__device__ inline void blur_run(const int (&v)[kOrbRun + 2 * kOrbBlurHalo], int (&out)[kOrbRun])
{
    constexpr int K[7] = {18, 34, 49, 55, 49, 34, 18};
#pragma unroll
    for (int p = 0; p < kOrbRun; p++) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) s += K[k] * v[p + k];
        out[p] = s;
    }
}

__global__ __launch_bounds__(kOrbBlock) void orb_blur_kernel(OrbArgs a)
{
    constexpr int PW = kOrbTileW + 2 * kOrbBlurHalo, PH = kOrbTileH + 2 * kOrbBlurHalo, PP = PW + 2;   // PP = 72: a run starts on 8 bytes
    __shared__ __attribute__((aligned(8))) uint8_t sp[PH * PP];
    __shared__ int sh[PH * kOrbBlurPitch];
    const OrbImage& im = a.images[blockIdx.x];
    const int level = (int)blockIdx.z;                      // n_levels: the 63 x 63 image
    const uint8_t* src;
    uint8_t* dst;
    int W, H, step;
    if (level == a.n_levels) {
        if (!a.do_gist || im.width == 0) return;
        src = a.pyr + im.gist_off; dst = a.blur + im.gist_blur_off; W = H = step = kOrbGist;
    } else {
        const OrbLevel& lv = a.units[im.whole].lev[level];
        src = (level == 0 ? a.pixels : a.pyr) + lv.img_off; dst = a.blur + lv.blur_off; W = lv.w; H = lv.h; step = lv.step;
    }
    if (W <= 0 || H <= 0) return;
    const int tiles_x = (W + kOrbTileW - 1) / kOrbTileW, tiles = tiles_x * ((H + kOrbTileH - 1) / kOrbTileH);
    const int tid = (int)threadIdx.x;
    for (int t = (int)blockIdx.y; t < tiles; t += (int)gridDim.y) {
        const int x0 = t % tiles_x * kOrbTileW, y0 = t / tiles_x * kOrbTileH;
        __syncthreads();
        // the tile and its reflected halo; past a cut tile the values are unused, the indices stay inside
        for (int idx = tid; idx < PH * PW; idx += kOrbBlock) {
            const int r = idx / PW, c = idx - r * PW;
            const int y = reflect101(min(y0 - kOrbBlurHalo + r, H + kOrbBlurHalo - 1), H);
            const int x = reflect101(min(x0 - kOrbBlurHalo + c, W + kOrbBlurHalo - 1), W);
            sp[r * PP + c] = src[(size_t)y * step + x];
        }
        __syncthreads();
        // rows: a lane makes a run of 8 columns from 16 bytes read as two 64-bit words
        for (int item = tid; item < PH * (kOrbTileW / kOrbRun); item += kOrbBlock) {
            const int r = item / (kOrbTileW / kOrbRun), c0 = item % (kOrbTileW / kOrbRun) * kOrbRun;
            const uint2 w0 = *reinterpret_cast<const uint2*>(sp + r * PP + c0), w1 = *reinterpret_cast<const uint2*>(sp + r * PP + c0 + 8);
            const uint32_t w[4] = {w0.x, w0.y, w1.x, w1.y};
            int v[kOrbRun + 2 * kOrbBlurHalo], o[kOrbRun];
#pragma unroll
            for (int q = 0; q < kOrbRun + 2 * kOrbBlurHalo; q++) v[q] = (int)((w[q >> 2] >> (8 * (q & 3))) & 255u);
            blur_run(v, o);
#pragma unroll
            for (int p = 0; p < kOrbRun; p++) sh[r * kOrbBlurPitch + c0 + p] = o[p];
        }
        __syncthreads();
        // columns: lanes side by side, each a run of 8 rows
        {
            const int c = tid % kOrbTileW, r0 = tid / kOrbTileW * kOrbRun;
            int v[kOrbRun + 2 * kOrbBlurHalo], o[kOrbRun];
#pragma unroll
            for (int q = 0; q < kOrbRun + 2 * kOrbBlurHalo; q++) v[q] = sh[(r0 + q) * kOrbBlurPitch + c];
            blur_run(v, o);
            if (x0 + c < W) {
#pragma unroll
                for (int p = 0; p < kOrbRun; p++)
                    if (y0 + r0 + p < H) dst[(size_t)(y0 + r0 + p) * W + x0 + c] = (uint8_t)min((o[p] + 32768) >> 16, 255);
            }
        }
    }
}

// contract step 9 for one keypoint by one wave: lane i makes bits 4i .. 4i + 3, even lanes store a byte
__device__ inline void describe(const uint8_t* blur, const uint8_t* raw, int raw_step, int W, int H, int cx, int cy, float angle,
                                const int8_t* pattern, uint8_t* out, int lane)
{
    const float rad = angle * (float)(3.14159265358979323846 / 180.0);
    double cd, sd;
    orb_cos_sin((double)rad, &cd, &sd);
    const float ca = (float)cd, sb = (float)sd;
    int nib = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        int val[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int pt = (lane * 4 + q) * 2 + e;
            const float px = (float)pattern[2 * pt], py = (float)pattern[2 * pt + 1];
            const int row = cy + rnd(px * sb + py * ca), col = cx + rnd(px * ca - py * sb);
            if ((unsigned)row < (unsigned)H && (unsigned)col < (unsigned)W) val[e] = (int)blur[(size_t)row * W + col];
            else val[e] = (int)raw[(size_t)reflect101(row, H) * raw_step + reflect101(col, W)];
        }
        nib |= (val[0] < val[1] ? 1 : 0) << q;
    }
    const int next = __shfl_down(nib, 1);
    if ((lane & 1) == 0) out[lane >> 1] = (uint8_t)(nib | (next << 4));
}

__global__ __launch_bounds__(kOrbBlock) void orb_describe_kernel(OrbArgs a)
{
    const OrbImage& im = a.images[blockIdx.y];
    const OrbUnit& un = a.units[im.whole];
    const int lane = (int)threadIdx.x & 63, wave = (int)(blockIdx.x * (kOrbBlock / 64) + threadIdx.x / 64);
    const uint32_t n = min(a.count[im.slot], (uint32_t)im.kp_cap);
    for (uint32_t k = (uint32_t)wave; k < n; k += kOrbWavesPerImage) {
        const OrbKp p = a.kp[im.kp_off + k];
        const OrbLevel& lv = un.lev[p.octave];
        const float s = 1.0f / a.level_scale[p.octave];
        describe(a.blur + lv.blur_off, (p.octave == 0 ? a.pixels : a.pyr) + lv.img_off, lv.step, lv.w, lv.h, rnd(p.u * s), rnd(p.v * s),
                 p.angle, a.pattern, a.desc + (size_t)(im.kp_off + k) * kOrbDescBytes, lane);
    }
    if (a.do_gist && wave == kOrbWavesPerImage - 1) {
        uint8_t* out = a.gist + (size_t)im.slot * kOrbDescBytes;
        if (im.width == 0) { if (lane < kOrbDescBytes) out[lane] = 0; }
        else describe(a.blur + im.gist_blur_off, a.pyr + im.gist_off, kOrbGist, kOrbGist, kOrbGist, kOrbGist / 2, kOrbGist / 2,
                      im.gist_angle, a.pattern, out, lane);
    }
}

// uzl_orb_lift: Feature.u / .v as the front end rounds them, half away from zero
__global__ __launch_bounds__(kOrbBlock) void orb_round_kernel(OrbRoundArgs a)
{
    const int i = (int)(blockIdx.x * kOrbBlock + threadIdx.x);
    if (i >= a.n) return;
    a.u[i] = (int)roundf(a.kp[i].u);
    a.v[i] = (int)roundf(a.kp[i].v);
}

inline int rows_for(int max_w, int max_h)
{
    const long long t = (long long)((max_w + kOrbTileW - 1) / kOrbTileW) * ((max_h + kOrbTileH - 1) / kOrbTileH);
    return (int)(t < 1 ? 1 : t > kOrbMaxTileBlocks ? kOrbMaxTileBlocks : t);
}

inline int blocks_for(int max_cap)
{
    const int b = (max_cap + kOrbBlock - 1) / kOrbBlock;
    return b < 1 ? 1 : b > kOrbMaxTileBlocks ? kOrbMaxTileBlocks : b;
}

}  // namespace

void launch_orb_resize(const OrbArgs& a, int level, int n_units, int max_w, int max_h, hipStream_t s)
{
    if (n_units > 0) hipLaunchKernelGGL(orb_resize_kernel, dim3(n_units, rows_for(max_w, max_h), 2), dim3(kOrbBlock), 0, s, a, level);
}

void launch_orb_gist_resize(const OrbArgs& a, hipStream_t s)
{
    if (a.n_images > 0) hipLaunchKernelGGL(orb_gist_resize_kernel, dim3(a.n_images), dim3(kOrbBlock), 0, s, a);
}

void launch_orb_fast(const OrbArgs& a, int max_w, int max_h, hipStream_t s)
{
    if (a.n_cell_units > 0) hipLaunchKernelGGL(orb_fast_kernel, dim3(a.n_cell_units, rows_for(max_w, max_h), a.n_levels), dim3(kOrbBlock), 0, s, a);
}

void launch_orb_cut(const OrbArgs& a, hipStream_t s)
{
    if (a.n_cell_units > 0) hipLaunchKernelGGL(orb_cut_kernel, dim3(a.n_cell_units), dim3(kOrbBins), 0, s, a);
}

void launch_orb_orient(const OrbArgs& a, int max_cap, hipStream_t s)
{
    if (a.n_cell_units > 0) hipLaunchKernelGGL(orb_orient_kernel, dim3(a.n_cell_units, blocks_for(max_cap), a.n_levels), dim3(kOrbBlock), 0, s, a);
}

void launch_orb_order(const OrbArgs& a, int max_cap, hipStream_t s)
{
    if (a.n_images > 0) hipLaunchKernelGGL(orb_order_kernel, dim3(blocks_for(max_cap), a.n_images), dim3(kOrbBlock), 0, s, a);
}

void launch_orb_blur(const OrbArgs& a, int max_w, int max_h, hipStream_t s)
{
    if (a.n_images > 0) hipLaunchKernelGGL(orb_blur_kernel, dim3(a.n_images, rows_for(max_w, max_h), a.n_levels + 1), dim3(kOrbBlock), 0, s, a);
}

void launch_orb_describe(const OrbArgs& a, hipStream_t s)
{
    if (a.n_images > 0) hipLaunchKernelGGL(orb_describe_kernel, dim3(kOrbWavesPerImage / (kOrbBlock / 64), a.n_images), dim3(kOrbBlock), 0, s, a);
}

void launch_orb_round(const OrbRoundArgs& a, hipStream_t s)
{
    if (a.n > 0) hipLaunchKernelGGL(orb_round_kernel, dim3((a.n + kOrbBlock - 1) / kOrbBlock), dim3(kOrbBlock), 0, s, a);
}

}  // namespace uzl
