// place_filters.hpp — what PlaceRecognizer does with an impl's result (place_recognizer.cpp:87-114, 157-180), shared by the
// recognizers behind it (uzl_gist.hip, uzl_gfr.hip).
#pragma once
#include <cmath>
#include <cstdint>
#include <unordered_set>
#include <vector>

namespace uzl {

// PlaceRecognizer::searchAndAddPlace / searchPlace after the impl: live, time gap, k cut, reported once.  stamp / alive = per place
// index the node's stamp and its membership of place_id_map_, checked = the (neighbour, query) pairs already reported (checked_);
// place_at(j), j < n = the impl's result, best first.  The k cut is tested after a neighbour is taken (:98), so k = 0 lets one through.
template <class PlaceAt>
void place_filters(const std::vector<int64_t>& stamp, const std::vector<uint8_t>& alive, std::unordered_set<uint64_t>& checked,
                   double min_time_gap, int32_t k, int32_t n, PlaceAt place_at, int64_t stamp_q, int32_t id_q, std::vector<int32_t>& res)
{
    int32_t pr = 0;
    for (int32_t j = 0; j < n; j++) {
        const int32_t nb = place_at(j);
        if (nb < 0 || nb >= (int32_t)alive.size() || !alive[nb]) continue;
        if (!(std::fabs((double)(stamp[nb] - stamp_q) * 1e-9) > min_time_gap)) continue;
        pr++;
        const uint64_t pair = ((uint64_t)(uint32_t)nb << 32) | (uint32_t)id_q;
        if (checked.insert(pair).second) res.push_back(nb);
        if (pr >= k) break;
    }
}

// the first `cap - at` of res to out[at ...]
inline void write_places(const std::vector<int32_t>& res, int64_t at, int64_t cap, int32_t* out)
{
    for (size_t j = 0; j < res.size(); j++)
        if (at + (int64_t)j < cap && out) out[at + j] = res[j];
}

}  // namespace uzl
