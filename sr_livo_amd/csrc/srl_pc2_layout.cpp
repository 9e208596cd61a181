// srl_pc2_layout.cpp -- layout validation of a PointCloud2 message and the yaw angles of srl_pc2_decode's fallback branch.  No HIP call.
// The yaw angle is the ONE step of the PointCloud2 decode that deliberately stays on the host: the reference's bits are
// atan2(double(y), double(x)) * 57.2957 of its libm (cloudProcessing.cpp:263, :372, :482), and a device atan2 is a different function.
#include "srl_pc2_layout.h"

#include <cmath>
#include <cstring>

int srl_pc2_time_bytes(int lidar_type) { return lidar_type == SRL_LIDAR_VELO || lidar_type == SRL_LIDAR_OUST ? 4 : lidar_type == SRL_LIDAR_ROBO ? 8 : 0; }
int srl_pc2_ring_bytes(int lidar_type) { return lidar_type == SRL_LIDAR_VELO || lidar_type == SRL_LIDAR_ROBO ? 2 : lidar_type == SRL_LIDAR_OUST ? 1 : 0; }

static bool field_fits(int32_t off, int bytes, uint32_t point_step) { return off >= 0 && (uint64_t)off + (uint64_t)bytes <= (uint64_t)point_step; }

int srl_pc2_layout_check(const srl_pc2_layout *l, int lidar_type, size_t data_bytes, uint64_t *n) {
    if (n) *n = 0;
    if (!l || l->is_bigendian != 0) return SRL_ERR_BAD_ARG;
    if (!field_fits(l->off_x, 4, l->point_step) || !field_fits(l->off_y, 4, l->point_step) || !field_fits(l->off_z, 4, l->point_step)) return SRL_ERR_BAD_ARG;
    if (lidar_type != 0) {
        const int tb = srl_pc2_time_bytes(lidar_type), rb = srl_pc2_ring_bytes(lidar_type);
        if (tb == 0 || !field_fits(l->off_time, tb, l->point_step) || !field_fits(l->off_ring, rb, l->point_step)) return SRL_ERR_BAD_ARG;
    }
    const uint64_t count = (uint64_t)l->width * (uint64_t)l->height;
    if (count > 0) {
        // the last point starts at the largest offset any point has, whatever row_step is
        // (three 32-bit factors pairwise: the sum can pass 2^64)
        const unsigned __int128 end = (unsigned __int128)(l->height - 1) * l->row_step + (unsigned __int128)(l->width - 1) * l->point_step + l->point_step;
        if ((unsigned __int128)data_bytes < end) return SRL_ERR_BAD_ARG;
    }
    if (n) *n = count;
    return SRL_OK;
}

extern "C" int srl_pc2_yaw_angles(const void *data, size_t data_bytes, const srl_pc2_layout *layout, double *yaw) {
    uint64_t n = 0;
    const int rc = srl_pc2_layout_check(layout, 0, data_bytes, &n);
    if (rc != SRL_OK) return rc;
    if (n > 0 && (!data || !yaw)) return SRL_ERR_BAD_ARG;
    const unsigned char *base = static_cast<const unsigned char *>(data);
    for (uint64_t i = 0; i < n; i++) {
        const unsigned char *p = base + srl_pc2_point_offset(*layout, i);
        float x, y;
        std::memcpy(&x, p + layout->off_x, 4);
        std::memcpy(&y, p + layout->off_y, 4);
        yaw[i] = std::atan2((double)y, (double)x) * 57.2957;
    }
    return SRL_OK;
}
