// laserline_types.hpp — POD shared by laserline_kernels.hip and uzl_laserline.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kLaserBlock = 256;          // bin kernel: one workgroup per (band of rows, image)
constexpr int kLaserVec = 4;              // pixels per lane and row: one 16-byte load of f32, one 8-byte load of u16
constexpr int kLaserFinishBlock = 256;    // finish kernel: one workgroup per group
constexpr int kLaserMaxBeams = 4096;      // contract step 1
constexpr uint32_t kLaserInfBits = 0x7f800000u;   // +inf: the empty value of a bin's min s (its max s starts at 0)

// One image of a chunk as the bin kernel reads it.
struct LaserImageRec {
    int64_t data_off;         // first byte of row 0 in the chunk's pixel area (16-byte aligned)
    int32_t width, height, step, encoding;
    int32_t lanes;            // lanes across one row (<= kLaserBlock); kLaserBlock / lanes rows are walked side by side
    int32_t out;              // index of the image in the call: its bins are smin / smax[out * n ..]
    double fx, fy, cx, cy;
    float T[12];              // (float)camera_transform
};

struct LaserBinArgs {
    const uint8_t* pixels;
    const LaserImageRec* images;
    const double2* trig;      // (c_k, s_k), k = 0..n
    uint32_t* smin;           // per image and bin: bits of min s, max s
    uint32_t* smax;
    double min_height, max_height, depth_scale;
    float amin, inc;          // for the first guess of a bin only
    int32_t n, band_rows;
};

struct LaserFinishArgs {
    const uint32_t* smin;
    const uint32_t* smax;
    const int32_t* group_first;   // images group_first[g] .. group_first[g + 1] make scan g
    const double2* trig;
    float* ranges;
    float* intensities;
    double* centers;              // 3 per scan
    float lo, hi0;
    int32_t n;
};

// LDS of one bin workgroup: the table, then the bins' min and max
inline size_t laser_bin_lds(int32_t n) { return (size_t)(n + 1) * sizeof(double2) + 2 * (size_t)n * sizeof(uint32_t); }

void laser_prepare();             // on the current device: allows the bin kernel its largest LDS request (n = 4096: 96 KiB)
void launch_laser_bin(const LaserBinArgs& a, int max_bands, int n_images, hipStream_t s);
void launch_laser_finish(const LaserFinishArgs& a, int n_groups, hipStream_t s);

struct HandleBase;
// What uzl_laserline_extract refuses in its images (the header names the set); the message goes to h.  Shared with uzl_depthfilter_refine.
int depth_images_check(HandleBase* h, int32_t n, const uzl_depth_image* images);
// bytes of an image from its first to its last pixel
size_t depth_image_bytes(const uzl_depth_image& im);

// Steps 1-9 of the laser-line handle over n_images f32 images that already lie on its device (uzl_depthfilter_to_laserline):
// recs[i] has data_off = the byte offset of image i in d_pixels (16-byte aligned), step = 4 * width, encoding f32, the intrinsics
// and T; lanes and out are filled in here.  groups[i] as uzl_depth_image.group, already checked.  Takes the handle's lock; the
// handle's depth_scale must be 1 and its device `device` (else UZL_ERR_BAD_ARG).  The result is the handle's resident result,
// as after an extract of the same images from the host.
int laserline_extract_device(uzl_laserline* h, int device, int32_t n_images, LaserImageRec* recs, const int32_t* groups,
                             const uint8_t* d_pixels, int32_t* n_scans, int32_t* n_beams);

}  // namespace uzl
