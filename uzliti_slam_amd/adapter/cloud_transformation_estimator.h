// cloud_transformation_estimator.h — host-side mirror of CloudTransformationEstimator
// (transformation_estimation/include/transformation_estimation/cloud_transformation_estimator.h,
//  src/cloud_transformation_estimator.cpp:40-161) with uzl_cloud_* in the place of the voxel grid and GICP-6D.
// Same contract as the feature mirror beside it: estimateEdge() enqueues, the worker delivers one callback per pair.  What
// changes: a node's depth images become clouds in HBM once (uzl_cloud_add_images) and are referenced by index afterwards, and
// the worker sends every queued pair, with every combination of the two nodes' depth sensors (:46-51), through ONE
// uzl_cloud_estimate call; per pair the first combination in the reference's loop order that passes the gates is the edge.
#pragma once
#include <unordered_map>

#include "transformation_estimator.h"

namespace uzl_adapter {

class Mi355xCloudTransformationEstimator : public TransformationEstimator {
public:
    explicit Mi355xCloudTransformationEstimator(uzl_adapter::function<void(SlamEdge)> callback, int device = 0);
    ~Mi355xCloudTransformationEstimator() override;
    bool estimateEdgeImpl(SlamNode& from, SlamNode& to, SlamEdge& edge) override;
    int lastStatus() const { return status_; }
    // the uzl_cloud_edge that decided the last pair of the last batch (status, iterations, num_corr per iteration, match_score)
    const uzl_cloud_edge& lastEdge() const { return last_; }

protected:
    void estimateBatch(std::vector<std::pair<SlamNode, SlamNode>>& pairs, std::vector<SlamEdge>& edges, std::vector<char>& ok) override;

private:
    int32_t cloudId(const DepthImageDataPtr& d);            // -1: the image gives no cloud that can be registered
    uzl_cloud* h_ = nullptr;
    std::unordered_map<const DepthImageData*, int32_t> cloud_ids_;      // DepthImageData are shared_ptr'd and immutable once created
    std::unordered_map<const DepthImageData*, DepthImageDataPtr> keep_alive_;
    int status_ = 0;
    uzl_cloud_edge last_{};
};

}  // namespace uzl_adapter
