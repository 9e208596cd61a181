// tests/stub_pc2/sensor_msgs/PointCloud2.h -- NOT ROS.  A test-owned stand-in for sensor_msgs::PointCloud2 with the members
// pcl::fromROSMsg reads of the real message: fields (name, offset, datatype, count), width, height, point_step, row_step, is_bigendian
// and the bytes themselves.  Put ahead of oracle/ref_shim (whose stand-in is a header-only shell) on the include path by
// tests/pc2_reader.py, so that the PointCloud2 handlers of src/cloudProcessing.cpp can be driven with real messages.
#pragma once
#include <ros/ros.h>

#include <cstdint>
#include <string>
#include <vector>

namespace sensor_msgs {
struct PointField {
    enum { INT8 = 1, UINT8 = 2, INT16 = 3, UINT16 = 4, INT32 = 5, UINT32 = 6, FLOAT32 = 7, FLOAT64 = 8 };
    std::string name;
    uint32_t offset = 0;
    uint8_t datatype = 0;
    uint32_t count = 1;
};
struct PointCloud2 {
    typedef std::shared_ptr<const PointCloud2> ConstPtr;
    typedef std::shared_ptr<PointCloud2> Ptr;
    std_msgs::Header header;
    uint32_t height = 0, width = 0;
    std::vector<PointField> fields;
    bool is_bigendian = false;
    uint32_t point_step = 0, row_step = 0;
    std::vector<uint8_t> data;
    bool is_dense = true;
};
typedef PointCloud2::ConstPtr PointCloud2ConstPtr;
struct Image { typedef std::shared_ptr<const Image> ConstPtr; std_msgs::Header header; };
typedef Image::ConstPtr ImageConstPtr;
struct CompressedImage { typedef std::shared_ptr<const CompressedImage> ConstPtr; std_msgs::Header header; std::string format; };
typedef CompressedImage::ConstPtr CompressedImageConstPtr;
namespace image_encodings { const std::string BGR8 = "bgr8"; }
}  // namespace sensor_msgs
