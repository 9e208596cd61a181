// tests/pc2_layout_san_main.cpp -- a stand-alone program (its own main, never loaded into Python) that tests/test_pc2_sanitizer.py compiles
// together with sr_livo_amd/csrc/srl_pc2_layout.cpp under -fsanitize=address,undefined and runs: srl_pc2_yaw_angles and the layout
// validation of srl_pc2_decode over buffers that are EXACTLY as long as the layout says (heap blocks: one byte read beyond the last point,
// or one misaligned typed access, is a report), with the layouts real drivers produce -- a RoboSense message with the double at offset 18
// and a message whose rows are padded.  It checks the values too, against atan2 called here.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sr_livo_amd/csrc/srl_pc2_layout.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); failures++; } } while (0)

// width x height points written at the layout's offsets into a heap block of exactly the needed size (+ slack bytes behind it)
static std::vector<unsigned char> *make_message(const srl_pc2_layout &l, int time_bytes, size_t slack, std::vector<float> &xs, std::vector<float> &ys) {
    const size_t n = (size_t)l.width * l.height;
    const size_t bytes = n ? (size_t)(l.height - 1) * l.row_step + (size_t)(l.width - 1) * l.point_step + l.point_step : 0;
    std::vector<unsigned char> *buf = new std::vector<unsigned char>(bytes + slack, (unsigned char)0xA5);
    xs.resize(n); ys.resize(n);
    for (size_t i = 0; i < n; i++) {
        unsigned char *p = buf->data() + srl_pc2_point_offset(l, i);
        const float x = (float)std::cos(0.37 * (double)i) * (1.0f + (float)i), y = (float)std::sin(0.37 * (double)i) * (1.0f + (float)i), z = 0.25f * (float)i;
        const double t = 1.7e9 + 1e-4 * (double)i;
        const float tf = (float)(1e-4 * (double)i);
        const uint16_t ring = (uint16_t)(i % 16);
        std::memcpy(p + l.off_x, &x, 4); std::memcpy(p + l.off_y, &y, 4); std::memcpy(p + l.off_z, &z, 4);
        if (time_bytes == 8) std::memcpy(p + l.off_time, &t, 8); else std::memcpy(p + l.off_time, &tf, 4);
        std::memcpy(p + l.off_ring, &ring, 2);
        xs[i] = x; ys[i] = y;
    }
    return buf;
}

static void run_layout(const srl_pc2_layout &l, int lidar_type) {
    std::vector<float> xs, ys;
    std::vector<unsigned char> *buf = make_message(l, srl_pc2_time_bytes(lidar_type), 0, xs, ys);
    const size_t n = xs.size();
    uint64_t count = 0;
    CHECK(srl_pc2_layout_check(&l, lidar_type, buf->size(), &count) == SRL_OK && count == n);
    CHECK(srl_pc2_layout_check(&l, lidar_type, buf->size() - 1, &count) == SRL_ERR_BAD_ARG && count == 0);      // one byte short of the last point
    std::vector<double> *yaw = new std::vector<double>(n);
    CHECK(srl_pc2_yaw_angles(buf->data(), buf->size(), &l, yaw->data()) == SRL_OK);
    for (size_t i = 0; i < n; i++) {
        const double want = std::atan2((double)ys[i], (double)xs[i]) * 57.2957;
        CHECK(std::memcmp(&want, &(*yaw)[i], 8) == 0);
    }
    CHECK(srl_pc2_yaw_angles(buf->data(), buf->size() - 1, &l, yaw->data()) == SRL_ERR_BAD_ARG);
    CHECK(srl_pc2_yaw_angles(nullptr, buf->size(), &l, yaw->data()) == SRL_ERR_BAD_ARG);
    CHECK(srl_pc2_yaw_angles(buf->data(), buf->size(), &l, nullptr) == SRL_ERR_BAD_ARG);
    // every field pushed one byte past point_step in turn, a negative offset, a big-endian message
    for (int f = 0; f < 5; f++) {
        srl_pc2_layout b = l;
        int32_t *off = f == 0 ? &b.off_x : f == 1 ? &b.off_y : f == 2 ? &b.off_z : f == 3 ? &b.off_time : &b.off_ring;
        const int size = f < 3 ? 4 : f == 3 ? srl_pc2_time_bytes(lidar_type) : srl_pc2_ring_bytes(lidar_type);
        *off = (int32_t)l.point_step - size + 1;
        CHECK(srl_pc2_layout_check(&b, lidar_type, buf->size(), &count) == SRL_ERR_BAD_ARG);
        *off = (int32_t)l.point_step - size;
        CHECK(srl_pc2_layout_check(&b, lidar_type, buf->size(), &count) == SRL_OK);                             // the last place it fits
        *off = -1;
        CHECK(srl_pc2_layout_check(&b, lidar_type, buf->size(), &count) == SRL_ERR_BAD_ARG);
    }
    srl_pc2_layout b = l;
    b.is_bigendian = 1;
    CHECK(srl_pc2_layout_check(&b, lidar_type, buf->size(), &count) == SRL_ERR_BAD_ARG);
    CHECK(srl_pc2_layout_check(&l, SRL_LIDAR_LIVOX, buf->size(), &count) == SRL_ERR_BAD_ARG);
    CHECK(srl_pc2_layout_check(&l, 7, buf->size(), &count) == SRL_ERR_BAD_ARG);
    CHECK(srl_pc2_layout_check(nullptr, lidar_type, buf->size(), &count) == SRL_ERR_BAD_ARG);
    delete yaw;
    delete buf;
}

int main() {
    // rslidar_sdk's XYZIRT: 26-byte points, the double at offset 18 -- nothing after x, y, z is aligned, and every second point is not either
    const srl_pc2_layout robo = {37, 1, 26, 37 * 26, 0, 4, 8, 18, 16, 0};
    run_layout(robo, SRL_LIDAR_ROBO);
    // the same with three rows and 5 bytes of padding behind each
    const srl_pc2_layout robo_rows = {13, 3, 26, 13 * 26 + 5, 0, 4, 8, 18, 16, 0};
    run_layout(robo_rows, SRL_LIDAR_ROBO);
    // velodyne_pointcloud's PointXYZIRT, 22 bytes, in rows padded to 64-byte multiples; an Ouster-sized point with odd offsets
    const srl_pc2_layout velo_rows = {10, 4, 22, 256, 0, 4, 8, 18, 16, 0};
    run_layout(velo_rows, SRL_LIDAR_VELO);
    const srl_pc2_layout oust_odd = {9, 2, 48, 9 * 48 + 1, 1, 5, 9, 21, 27, 0};
    run_layout(oust_odd, SRL_LIDAR_OUST);
    // no point at all: nothing is read, whatever the pointers
    const srl_pc2_layout empty = {0, 1, 26, 0, 0, 4, 8, 18, 16, 0};
    uint64_t count = 7;
    CHECK(srl_pc2_layout_check(&empty, SRL_LIDAR_ROBO, 0, &count) == SRL_OK && count == 0);
    CHECK(srl_pc2_yaw_angles(nullptr, 0, &empty, nullptr) == SRL_OK);
    // width * height beyond 32 bits does not wrap
    const srl_pc2_layout huge = {0xFFFFFFFFu, 0xFFFFFFFFu, 26, 0xFFFFFFFFu, 0, 4, 8, 18, 16, 0};
    CHECK(srl_pc2_layout_check(&huge, SRL_LIDAR_ROBO, (size_t)1 << 40, &count) == SRL_ERR_BAD_ARG);
    if (failures) return 1;
    std::printf("pc2 layout: ok\n");
    return 0;
}
