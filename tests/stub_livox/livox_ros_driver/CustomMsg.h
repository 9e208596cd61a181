// tests/stub_livox/livox_ros_driver/CustomMsg.h -- NOT the Livox driver.  A test-owned stand-in for livox_ros_driver::CustomMsg with the
// members cloudProcessing::livoxHandler reads (header.stamp, point_num, points[i].{offset_time, x, y, z, reflectivity, tag, line}), put
// ahead of oracle/ref_shim on the include path by tests/test_livox_checker_reference.py: the stand-in there is a header-only shell.
// CustomPoint is the driver's message layout: uint32 offset_time, float32 x y z, uint8 reflectivity tag line -- 20 bytes in memory, what
// include/srlivo_hip.h calls srl_livox_point.
#pragma once
#include <ros/ros.h>

#include <cstdint>
#include <memory>
#include <vector>

namespace livox_ros_driver {
struct CustomPoint {
    uint32_t offset_time;
    float x, y, z;
    uint8_t reflectivity, tag, line;
};
static_assert(sizeof(CustomPoint) == 20, "CustomPoint is 19 bytes of fields in a 20-byte record");
struct CustomMsg {
    typedef std::shared_ptr<const CustomMsg> ConstPtr;
    typedef std::shared_ptr<CustomMsg> Ptr;
    std_msgs::Header header;
    uint64_t timebase = 0;
    uint32_t point_num = 0;
    uint8_t lidar_id = 0;
    std::vector<CustomPoint> points;
};
}  // namespace livox_ros_driver
