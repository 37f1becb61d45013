// depthfilter_types.hpp — POD shared by depthfilter_kernels.hip and uzl_depthfilter.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kDepthBlock = 256;          // refine kernel: one workgroup per (tile, image)
constexpr int kDepthTileW = 64;           // output tile: 64 x 32 pixels, 8 per lane
constexpr int kDepthTileH = 32;
constexpr int kDepthMaxRadius = 15;       // contract: R in [0, 15], P in [0, 7]
constexpr int kDepthMaxNearest = 7;
constexpr int kDepthColours = 256;        // contract step 2: cw has one entry per |g - g'|
constexpr int kDepthLiftBlock = 256;      // lift kernel: one lane per keypoint

// One image of a chunk as the refine kernel reads it.
struct DepthImageRec {
    int64_t depth_off;        // first byte of the depth image's row 0 in the chunk's pixel area
    int64_t guide_off;        // ... of the guide's
    int64_t out_off;          // first float of the refined image in the resident buffer
    int32_t width, height, depth_step, guide_step, encoding, _pad;
};

struct DepthRefineArgs {
    const uint8_t* pixels;
    const DepthImageRec* images;
    const float* tables;      // cw[0..255], then sw[-R..R]
    float* out;
    double depth_scale;
    int32_t radius, nearest, filter;
};

struct DepthLiftArgs {
    const float* image;
    const int32_t* u;
    const int32_t* v;
    double* pos;              // 3 per keypoint
    uint8_t* valid;
    double fx, fy, cx, cy, max_depth;
    int32_t width, height, n;
};

// The halo of the depth tile: the passes reach R, the snap P
__host__ __device__ inline int depth_halo(int radius, int nearest) { return radius > nearest ? radius : nearest; }

// LDS pitches, both odd: of the depth / guide tile with its halo, and of the horizontal-pass rows
__host__ __device__ inline int depth_pitch(int radius, int nearest) { return kDepthTileW + 2 * depth_halo(radius, nearest) + 1; }
constexpr int kDepthPitchH = kDepthTileW + 1;

// LDS of one refine workgroup: depth tile and halo (f32), horizontal-pass rows (f32), the two tables, guide tile and halo (u8)
inline size_t depth_refine_lds(int radius, int nearest)
{
    const size_t tile = (size_t)depth_pitch(radius, nearest) * (kDepthTileH + 2 * (size_t)depth_halo(radius, nearest));
    return (tile + (size_t)kDepthPitchH * (kDepthTileH + 2 * (size_t)radius) + kDepthColours + 2 * (size_t)radius + 1) * sizeof(float) + tile;
}

void launch_depth_refine(const DepthRefineArgs& a, int tiles_x, int tiles_y, int n_images, hipStream_t s);
void launch_depth_lift(const DepthLiftArgs& a, hipStream_t s);

// uzl_depthfilter_lift for keypoints that lie on `device` already (uzl_orb_lift): n int32 each, complete when the call is made.
// Takes the filter handle's lock; UZL_ERR_BAD_ARG for another device, else as uzl_depthfilter_lift.
int depthfilter_lift_device(uzl_depthfilter* h, int device, int32_t image, int32_t n, const int32_t* d_u, const int32_t* d_v,
                            double max_depth, double* pos_xyz, uint8_t* valid3d);

}  // namespace uzl
