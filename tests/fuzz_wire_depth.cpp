// CPU-only sanitizer fuzz of the depth-image branch of the SensorData parser (tests/test_laserline_wire.py builds it with
// g++ -fsanitize=address,undefined together with csrc/uzl_wire.hip, which is plain host C++): mutated and truncated Node messages
// whose sensors carry depth images must never make uzl_wire_sensor_depth / uzl_wire_depth_image / the encoder read out of bounds
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <fstream>
#include <iterator>
#include "../include/uzl_mi355x.h"
static std::vector<uint8_t> rd(const char* p) { std::ifstream f(p, std::ios::binary); return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), {}); }
static uint32_t s = 1; static uint32_t rnd() { s = s * 1664525u + 1013904223u; return s >> 8; }
int main(int argc, char** argv)
{
    std::vector<std::vector<uint8_t>> seeds; for (int i = 1; i < argc; i++) seeds.push_back(rd(argv[i]));
    long ok[3] = {0, 0, 0}, n = 0;
    const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int it = 0; it < 100000; it++) {
        std::vector<uint8_t> m = seeds[rnd() % seeds.size()];
        const int muts = rnd() % 4;
        for (int k = 0; k < muts && !m.empty(); k++) {
            const size_t pos = rnd() % m.size();
            switch (rnd() % 4) { case 0: m[pos] = (uint8_t)rnd(); break; case 1: m[pos] ^= 1u << (rnd() % 8); break;
                case 2: { uint32_t v = (rnd() % 3 == 0) ? 0xffffffffu : rnd() % 100000; if (pos + 4 <= m.size()) memcpy(&m[pos], &v, 4); break; }
                case 3: m.resize(pos); break; }
        }
        // exact-size heap copy so that any overread trips the sanitizer
        uint8_t* b = (uint8_t*)malloc(m.size() ? m.size() : 1); memcpy(b, m.data(), m.size());
        uzl_wire_node nd; uzl_wire_sensor sens[4]; uzl_span eids[4]; int64_t st[4]; uint64_t used = 0;
        if (uzl_wire_node_decode(b, m.size(), &nd, 4, st, 4, eids, 4, sens, &used) == UZL_OK) {
            ok[0]++;
            for (int i = 0; i < nd.n_sensors && i < 4; i++) {
                volatile char acc = 0;
                uzl_wire_depth d;
                const int rc = uzl_wire_sensor_depth(&sens[i], &d);
                if (rc != UZL_OK && rc != UZL_ERR_UNSUPPORTED) continue;
                ok[1]++;
                if (d.data.n) acc += d.data.p[d.data.n - 1];
                if (d.color.n) acc += d.color.p[d.color.n - 1];
                if (d.encoding.n) acc += d.encoding.p[d.encoding.n - 1];
                if (d.frame_id.n) acc += d.frame_id.p[d.frame_id.n - 1];
                uzl_depth_image im;
                if (uzl_wire_depth_image(&d, I, 0, &im) == UZL_OK) {
                    ok[2]++;
                    if (im.height > 0) acc += ((const char*)im.data)[(size_t)im.height * (size_t)im.step - 1];
                }
                uzl_wire_scan sc;
                if (uzl_wire_sensor_scan(&sens[i], &sc) == UZL_OK && sc.ranges.n) acc += sc.ranges.p[sc.ranges.n - 1];
                std::vector<uint8_t> o(uzl_wire_depth_sensor_size(sens[i].sensor_frame, &d, sens[i].camera_info)); uint64_t w = 0;
                if (!o.empty()) uzl_wire_depth_sensor_encode(1, 2, sens[i].sensor_frame, I, &d, sens[i].camera_info, o.data(), o.size(), &w);
            }
        }
        free(b); n++;
    }
    printf("fuzz: %ld inputs, decoded ok: node %ld depth %ld image %ld\n", n, ok[0], ok[1], ok[2]);
    return 0;
}
