// srl_pc2_layout.h -- the host side of srl_pc2_decode that touches no device: what a srl_pc2_layout must satisfy before a byte of the message is
// read, and the yaw angles of the fallback branch (srl_pc2_yaw_angles, declared in srlivo_hip.h).  Plain C++ without a HIP call, so that it
// also builds into a stand-alone program under ASan / UBSan (tests/pc2_layout_san.cpp).
#pragma once
#include "../../include/srlivo_hip.h"

#include <cstddef>
#include <cstdint>

// cloudProcessing.h:25
enum { SRL_LIDAR_LIVOX = 1, SRL_LIDAR_VELO = 2, SRL_LIDAR_OUST = 3, SRL_LIDAR_ROBO = 4 };

// bytes of the time field / of the ring field of the registered point struct (cloudProcessing.h:50-114); 0: not a PointCloud2 LiDAR
int srl_pc2_time_bytes(int lidar_type);
int srl_pc2_ring_bytes(int lidar_type);
// SRL_OK iff every field the decode reads lies inside point_step, the message is little-endian and data_bytes covers the last point;
// *n = width * height.  lidar_type 0: the coordinates alone (srl_pc2_yaw_angles).  Reads no byte of the message.
int srl_pc2_layout_check(const srl_pc2_layout *layout, int lidar_type, size_t data_bytes, uint64_t *n);
// byte offset of point i
inline size_t srl_pc2_point_offset(const srl_pc2_layout &l, uint64_t i) { return (size_t)(i / l.width) * l.row_step + (size_t)(i % l.width) * l.point_step; }
