// cloud_transformation_estimator.cpp — see the header
#include "cloud_transformation_estimator.h"

#include <cstring>

namespace uzl_adapter {
namespace {

Isometry3d mul(const Isometry3d& A, const Isometry3d& B)
{
    Isometry3d C;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 4; c++) C.m[4 * r + c] = A.m[4 * r] * B.m[c] + A.m[4 * r + 1] * B.m[4 + c] + A.m[4 * r + 2] * B.m[8 + c];
        C.m[4 * r + 3] += A.m[4 * r + 3];
    }
    return C;
}

Isometry3d inverse(const Isometry3d& A)                      // Isometry3d::inverse(): R^T, -R^T t
{
    Isometry3d B;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) B.m[4 * r + c] = A.m[4 * c + r];
        B.m[4 * r + 3] = -(A.m[r] * A.m[3] + A.m[4 + r] * A.m[7] + A.m[8 + r] * A.m[11]);
    }
    return B;
}

struct Combo { size_t pair; DepthImageDataPtr from, to; };

}  // namespace

Mi355xCloudTransformationEstimator::Mi355xCloudTransformationEstimator(uzl_adapter::function<void(SlamEdge)> callback, int device)
    : TransformationEstimator(callback)
{
    uzl_cloud_cfg c;
    uzl_cloud_cfg_default(&c);
    c.device = device;
    status_ = uzl_cloud_create(&c, &h_);
}

Mi355xCloudTransformationEstimator::~Mi355xCloudTransformationEstimator()
{
    stopThread();
    uzl_cloud_destroy(h_);
}

int32_t Mi355xCloudTransformationEstimator::cloudId(const DepthImageDataPtr& d)
{
    auto it = cloud_ids_.find(d.get());
    if (it != cloud_ids_.end()) return it->second;
    uzl_depth_image depth;
    std::memset(&depth, 0, sizeof(depth));
    depth.data = d->depth_image_.data(); depth.encoding = UZL_DEPTH_F32_M;
    depth.width = d->width; depth.height = d->height; depth.step = 4 * d->width;
    depth.fx = d->fx; depth.fy = d->fy; depth.cx = d->cx; depth.cy = d->cy;
    const Isometry3d I;
    std::memcpy(depth.camera_transform, I.m.data(), sizeof(depth.camera_transform));     // toPointCloudColor gets the identity (:60-61)
    uzl_color_image color{d->color_image_.data(), d->width, d->height, 3 * d->width, d->color_is_rgb ? UZL_COLOR_RGB8 : UZL_COLOR_BGR8};
    int32_t id = -1;
    status_ = uzl_cloud_add_images(h_, 1, &depth, &color, &id);
    if (status_ != UZL_OK) id = -1;
    cloud_ids_[d.get()] = id;
    keep_alive_[d.get()] = d;
    return id;
}

void Mi355xCloudTransformationEstimator::estimateBatch(std::vector<std::pair<SlamNode, SlamNode>>& pairs, std::vector<SlamEdge>& edges,
                                                       std::vector<char>& ok)
{
    std::vector<Combo> combos;
    std::vector<uzl_cloud_pair> jobs;
    for (size_t j = 0; j < pairs.size(); j++) {
        ok[j] = 0;
        SlamNode& from = pairs[j].first;
        SlamNode& to = pairs[j].second;
        edges[j].id_from_ = from.id_; edges[j].id_to_ = to.id_;
        if (!h_) continue;
        for (auto& sf : from.sensor_data_) {                                              // :46-51
            if (sf->type_ != SENSOR_TYPE_DEPTH_IMAGE) continue;
            for (auto& st : to.sensor_data_) {
                if (st->type_ != SENSOR_TYPE_DEPTH_IMAGE) continue;
                DepthImageDataPtr df = std::dynamic_pointer_cast<DepthImageData>(sf), dt = std::dynamic_pointer_cast<DepthImageData>(st);
                if (!df || !dt) continue;
                uzl_cloud_pair p;
                p.cloud_from = cloudId(df); p.cloud_to = cloudId(dt);
                if (p.cloud_from < 0 || p.cloud_to < 0) continue;
                const Isometry3d T_diff = mul(mul(mul(inverse(sensor_transforms_[df->sensor_frame_]), inverse(df->displacement_)),       // :54-58
                                                  mul(inverse(from.pose_), to.pose_)),
                                              mul(dt->displacement_, sensor_transforms_[dt->sensor_frame_]));
                std::memcpy(p.first_guess, T_diff.m.data(), sizeof(p.first_guess));
                jobs.push_back(p);
                combos.push_back(Combo{j, df, dt});
            }
        }
    }
    if (jobs.empty()) return;
    std::vector<uzl_cloud_edge> res(jobs.size());
    status_ = uzl_cloud_estimate(h_, (int32_t)jobs.size(), jobs.data(), res.data());
    if (status_ != UZL_OK) return;
    for (size_t k = 0; k < jobs.size(); k++) {
        const size_t j = combos[k].pair;
        if (ok[j]) continue;                                                              // the first success returns (:92-93)
        if (j + 1 == pairs.size()) last_ = res[k];                                        // of the last pair: the combination that decided it
        if (res[k].status != UZL_CLOUD_OK) continue;                                      // the gates of :66-70
        SlamEdge& e = edges[j];
        std::memcpy(e.transform_.m.data(), res[k].transform, sizeof(res[k].transform));   // :83
        std::memcpy(e.information_.data(), res[k].information, sizeof(res[k].information));   // :84
        e.type_ = TYPE_3D_FULL;                                                           // :85
        e.sensor_from_ = combos[k].from->sensor_frame_; e.sensor_to_ = combos[k].to->sensor_frame_;           // :86-87
        e.displacement_from_ = combos[k].from->displacement_; e.displacement_to_ = combos[k].to->displacement_;   // :88-89
        e.matching_score_ = res[k].matching_score;                                        // :90
        ok[j] = 1;
    }
}

bool Mi355xCloudTransformationEstimator::estimateEdgeImpl(SlamNode& from, SlamNode& to, SlamEdge& edge)
{
    std::vector<std::pair<SlamNode, SlamNode>> one(1, std::make_pair(from, to));
    std::vector<SlamEdge> e(1);
    std::vector<char> ok(1, 0);
    estimateBatch(one, e, ok);
    edge = e[0];
    return ok[0] != 0;
}

}  // namespace uzl_adapter
