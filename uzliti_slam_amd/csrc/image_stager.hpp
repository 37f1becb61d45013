// image_stager.hpp — how uzl_laserline and uzl_depthfilter move a call's images to the device: in chunks through two pinned
// staging halves, so that the host packs one half while the other half's copy and kernel run.  A chunk is one copy, its image
// records in front of its pixels; what a record is and what counts as an image's bytes is the module's business.
#pragma once
#include "uzl_common.hpp"

namespace uzl {

constexpr size_t kStageChunkBytes = (size_t)64 << 20;   // pixels of one staging half (an image larger than this gets a half of its own size)
constexpr int32_t kStageChunkImages = 8192;             // images of one chunk (a grid dimension of the kernels that take a chunk)

// Items 0..n in chunks, in order: chunk k is [first[k], first[k + 1]).  An item joins the open chunk while that has fewer than
// max_items (>= 1) items and the item is its first or the chunk's bytes stay within max_bytes.
template <typename ItemBytes>
std::vector<int32_t> plan_chunks(ItemBytes&& item_bytes, int32_t n, size_t max_bytes, int32_t max_items)
{
    std::vector<int32_t> first{0};
    for (int32_t i0 = 0; i0 < n; first.push_back(i0)) {
        int32_t i1 = i0;
        size_t bytes = 0;
        while (i1 < n && i1 - i0 < max_items) {
            const size_t nb = item_bytes(i1);
            if (i1 > i0 && bytes + nb > max_bytes) break;
            bytes += nb;
            i1++;
        }
        i0 = i1;
    }
    return first;
}

struct ImageStager {
    Event copied[2];             // the copy out of staging half i has finished
    PinBuf<uint8_t> h_chunk[2];
    DevBuf<uint8_t> d_chunk[2];

    void create() { for (Event& e : copied) e.create(); }

    // Waits for the half's last copy and makes room for `total` bytes on both sides: where the host packs them.
    uint8_t* open(int half, size_t total)
    {
        UZL_HIP(hipEventSynchronize(copied[half]));
        h_chunk[half].reserve(total);
        d_chunk[half].reserve(total);
        return h_chunk[half].p;
    }

    // Sends the half's first `total` bytes in one copy on `s` and marks the half: where they lie on the device.
    const uint8_t* send(int half, size_t total, hipStream_t s)
    {
        UZL_HIP(hipMemcpyAsync(d_chunk[half].p, h_chunk[half].p, total, hipMemcpyHostToDevice, s));
        UZL_HIP(hipEventRecord(copied[half], s));
        return d_chunk[half].p;
    }
};

}  // namespace uzl
