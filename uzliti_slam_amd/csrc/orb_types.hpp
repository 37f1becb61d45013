// orb_types.hpp — POD shared by orb_kernels.hip and uzl_orb.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kOrbBlock = 256;            // every orb kernel: 256 threads, 4 waves
constexpr int kOrbMaxLevels = 8;          // contract: n_levels in [1, 8]
constexpr int kOrbTileW = 64;             // resize, blur and FAST tile: 64 x 32 pixels, 8 per lane
constexpr int kOrbTileH = 32;
constexpr int kOrbFastHalo = 4;           // FAST: 3 for the circle, 1 for the 3 x 3 suppression
constexpr int kOrbFastPitch = kOrbTileW + 2 * kOrbFastHalo + 4;   // 76 bytes = 19 words: odd in words, rows spread over the banks
constexpr int kOrbScorePitch = kOrbTileW + 2 + 2;                 // 68 bytes = 17 words
constexpr int kOrbBlurHalo = 3;           // 7 x 7
constexpr int kOrbBlurPitch = kOrbTileW + 2 * kOrbBlurHalo + 1;   // ints, odd
constexpr int kOrbBins = 256;             // a FAST score is an integer in [0, 255]
constexpr int kOrbPoints = 512;           // pattern points; pair 2k, 2k + 1 gives bit k
constexpr int kOrbDescBytes = 32;
constexpr int kOrbGist = 63;              // contract step 11
constexpr int kOrbWavesPerImage = 64;     // describe kernel: waves that share one image's keypoints
constexpr int kOrbMaxTileBlocks = 4096;   // grid rows over tiles / candidate blocks; a workgroup strides over the rest

// One level of a unit: where its pixels lie (level 0: in the chunk's pixel area; above: in the pyramid buffer).
struct OrbLevel {
    int64_t img_off, mask_off;    // first byte of row 0
    int64_t blur_off;             // whole-image units: the blurred level in the blur buffer (pitch = w)
    int64_t cand_off;             // cell units: first candidate of this level in the candidate arrays
    int32_t w, h, step, mask_step;
    int32_t cand_cap, _pad;
};

// A unit is one image seen as a detector sees it: a cell of the grid (steps 2-8) or the whole image (steps 9-10).
struct OrbUnit {
    int32_t image;                // index into the chunk's OrbImage records
    int32_t x0, y0;               // the cell's corner in the image
    int32_t has_mask;
    OrbLevel lev[kOrbMaxLevels];
};

struct OrbImage {
    int64_t kp_off;               // first keypoint of this image in the resident arrays
    int64_t tmp_off;              // ... in the chunk's arrival-order array
    int64_t gist_off, gist_blur_off;   // 63 x 63 images in the pyramid / blur buffer
    int32_t width, height;
    int32_t kp_cap, slot;         // slot: the image's index in the call (its count and its gist)
    int32_t whole;                // its whole-image unit
    float gist_angle;
};

// A keypoint as it lies in HBM, unsorted and sorted.
struct OrbKp {
    float u, v, response, angle;
    int32_t octave;
};

struct OrbArgs {
    const uint8_t* pixels;        // the chunk's pixel area: images and masks
    const OrbUnit* units;         // cell units first (n_cell_units), then one whole-image unit per image
    const OrbImage* images;
    uint8_t* pyr;                 // levels >= 1 of every unit, image and mask, and the gist images
    uint8_t* blur;
    uint2* cand_xy;               // candidates after FAST, mask and border: level position
    uint8_t* cand_score;
    uint32_t* hist;               // per (cell unit, level): 256 bins
    uint32_t* n_cand;             // per (cell unit, level)
    uint32_t* thr;                // per (cell unit, level): keep response >= thr
    uint32_t* count;              // per image of the call (slot): keypoints
    OrbKp* kp_tmp;                // in arrival order
    OrbKp* kp;                    // in the contract's order
    uint8_t* desc;                // 32 bytes per keypoint, beside kp
    uint8_t* gist;                // 32 bytes per image of the call
    const int8_t* pattern;        // 512 x (x, y)
    float level_scale[kOrbMaxLevels];     // (float)pow((double)scale_factor, l)
    int32_t n_per_level[kOrbMaxLevels];   // step 6
    int32_t n_per_cell;                   // step 8
    int32_t n_levels, edge, fast_threshold;
    int32_t n_cell_units, n_images, do_gist;
};

struct OrbRoundArgs {
    const OrbKp* kp;
    int32_t* u;
    int32_t* v;
    int32_t n;
};

// launches of one chunk, in order; `level` of launch_orb_resize = the level made (from level - 1)
void launch_orb_resize(const OrbArgs& a, int level, int n_units, int max_w, int max_h, hipStream_t s);
void launch_orb_gist_resize(const OrbArgs& a, hipStream_t s);
void launch_orb_fast(const OrbArgs& a, int max_w, int max_h, hipStream_t s);
void launch_orb_cut(const OrbArgs& a, hipStream_t s);
void launch_orb_orient(const OrbArgs& a, int max_cap, hipStream_t s);
void launch_orb_order(const OrbArgs& a, int max_cap, hipStream_t s);
void launch_orb_blur(const OrbArgs& a, int max_w, int max_h, hipStream_t s);
void launch_orb_describe(const OrbArgs& a, hipStream_t s);
void launch_orb_round(const OrbRoundArgs& a, hipStream_t s);

// The cos / sin of contract step 9 (arithmetic only, f64; shared with the restatement in tests/orb_reference.py).
__host__ __device__ inline void orb_cos_sin(double x, double* c, double* s)
{
    const double k = rint(x * 0.63661977236758138243);          // 2 / pi
    const double r = (x - k * 1.57079632673412561417) - k * 6.07710050650619224932e-11;   // pi / 2 in two parts, the first 33 bits
    const double z = r * r;
    const double sp = r + r * z * (-1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                      z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)))));
    const double cp = 1.0 - 0.5 * z + z * z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                      z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const int q = (int)(k - 4.0 * floor(k * 0.25));              // k mod 4, k is an integer below 2^31
    *c = q == 0 ? cp : q == 1 ? -sp : q == 2 ? -cp : sp;
    *s = q == 0 ? sp : q == 1 ? cp : q == 2 ? -sp : -cp;
}

}  // namespace uzl
