// cloud_types.hpp — POD shared by cloud_kernels.hip and uzl_cloud.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kCloudBlock = 256;          // queries per workgroup of the search kernels; the step kernel's workgroup (lane t owns t, t + 256, ...)
constexpr int kCloudTile = 1024;          // target points per LDS tile (32 B each in the 6-D search, 16 B in the 3-D one)
constexpr int kCloudK = 20;               // length of the 3-D search's sorted list (cfg.k_neighbours <= it)
constexpr int kCloudMinPoints = 3;        // the least k_neighbours
constexpr int kCloudMaxPoints = UZL_CLOUD_MAX_POINTS;
constexpr int kCloudSums = 28;            // H (21: ww 6, wv 9, vv 6), g (6), f
constexpr int kCloudCbrtSteps = 6;        // contract step 3: Halley steps of the cube root

// One stored cloud: its points are [off, off + n) of the store's arrays (xyz 3 f32, bgr 3 u8, lab 3 f32, cov 6 f64 per point).
struct CloudRec {
    int64_t off;
    int32_t n;
    int32_t k;                            // the k_neighbours its covariances were made with; 0: none (fewer points than that)
};

// One pair as the kernels read it.
struct CloudPairRec {
    int32_t from, to;
    int64_t tgt_off, src_off;             // into the call's work arrays: moved target points; per-source-point j, distance, M
    double G[12];                         // T_diff, the first guess
    double T0[12];                        // the estimate to start from: the identity, or the stage entry's T
};

// The state of one pair between launches, and what the host reads at the end.
struct CloudPairState {
    double T[12];
    int32_t done, iterations, status, num_corr;
    int32_t num_corr_iter[UZL_CLOUD_MAX_ITERATIONS];
};

#ifdef UZL_DIAG
// What cloud_step_kernel's thread 0 records of one launch for uzl_debug_cloud_step (the diagnostic library only).
constexpr int kCloudLogTrials = 100;      // the most inner_iterations may be
struct CloudStepLog {
    double sums[kCloudSums];              // H, g and f at the pose the launch starts from
    double trial[kCloudLogTrials][9];     // mu as used, outcome (0 refused, 1 accepted, 2 rejected), delta (6), the trial pose's f
    int32_t n_trials, _pad;
};
#endif

struct CloudIcpArgs {
    const CloudRec* clouds;
    const float* xyz;
    const float* lab;
    const double* cov;
    const CloudPairRec* pairs;
    CloudPairState* state;
    float* tgt;                           // 8 f32 per moved target point: x y z 0 sL sa sb 0
    int32_t* nn_j;
    float* nn_d;
    double* M;                            // 6 f64 per source point: 00 01 02 11 12 22
    double max_corr_sq, rot_eps, trans_eps;
    float lab_weight;
    int32_t max_iterations, inner_iterations;
#ifdef UZL_DIAG
    CloudStepLog* log;                    // NULL in every launch but uzl_debug_cloud_step's (one pair)
#endif
};

// One image pair of an add: depth and colour pixels already on the device.
struct CloudImageRec {
    const uint8_t* depth;
    const uint8_t* color;
    int64_t pix_off;                      // the image's first pixel among the call's pixels
    int32_t width, height, depth_step, color_step, encoding, swap_rb;
    double fx, fy, cx, cy;
};

// Work of one voxelisation (steps 1-2), owned by the handle and reused.
struct CloudVoxelWork {
    uint32_t* bbox;                       // order-preserving codes: min x y z of every image, then max x y z of every image
    int32_t* info;                        // 2 per image: voxel count, 1 iff the grid overflows int32
    uint64_t* keys[2];                    // (image << 32 | key), before and after the sort
    uint32_t* vals[2];                    // pixel index among the call's pixels
    uint32_t* flag;                       // 1 at the first sorted position of a voxel
    uint32_t* rank;                       // exclusive scan of flag
    void* temp;
    size_t temp_bytes;
};

// bytes of rocPRIM scratch a voxelisation of n_pixels pixels needs
size_t cloud_voxel_temp_bytes(int64_t n_pixels, int32_t n_images);
// Steps 1-2 up to the voxel counts: bounding boxes, keys, the stable sort, heads and their ranks; info is complete when the stream
// has run.
void cloud_voxel_sort(const CloudImageRec* recs, int32_t n_images, int64_t n_pixels, int32_t max_pixels, float leaf, float z_min,
                      float z_max, const CloudVoxelWork& w, hipStream_t s);
// The voxel points: one thread per voxel sums its pixels in ascending pixel index; point r of the call goes to xyz / bgr[3 r ..].
void launch_cloud_voxel_points(const CloudImageRec* recs, int64_t n_pixels, float leaf, float z_min, float z_max, const CloudVoxelWork& w,
                               float* xyz, uint8_t* bgr, hipStream_t s);

void launch_cloud_lab(const uint8_t* bgr, float* lab, const double* table, int64_t n, hipStream_t s);
// covariances of n_clouds clouds (recs on the device, the largest of them max_n points) into cov
void launch_cloud_cov(const CloudRec* recs, int32_t n_clouds, int32_t max_n, const float* xyz, double* cov, int32_t k, double gicp_epsilon,
                      hipStream_t s);
void launch_cloud_prepare(const CloudIcpArgs& a, int32_t n_pairs, int32_t max_to, hipStream_t s);
void launch_cloud_nn6(const CloudIcpArgs& a, int32_t n_pairs, int32_t max_from, hipStream_t s);
void launch_cloud_step(const CloudIcpArgs& a, int32_t n_pairs, hipStream_t s);

// uzl_depthfilter_to_cloud's way into the store: steps 1-4 over n images whose f32 depth pixels d_depth[i] (row step 4 * width)
// already lie on `device` and are complete; geom[i] gives width, height and intrinsics (its data, step and encoding are not read),
// colors[i] the host's colour image.  Takes the handle's lock.
int cloud_add_device_images(uzl_cloud* h, int device, int32_t n, const uzl_depth_image* geom, const float* const* d_depth,
                            const uzl_color_image* colors, int32_t* first_cloud);

}  // namespace uzl
