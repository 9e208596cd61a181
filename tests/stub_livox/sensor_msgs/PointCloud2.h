// tests/stub_livox/sensor_msgs/PointCloud2.h -- NOT ROS.  The stand-in of oracle/ref_shim with the one member more that
// src/cloudProcessing.cpp needs to be compiled where it lies (printfFieldName reads msg->fields).  The PointCloud2 handlers of that file
// are compiled and never called: tests/livox_ref_reader.cpp drives cloudProcessing::livoxHandler alone.
#pragma once
#include <ros/ros.h>
namespace sensor_msgs {
struct PointField { std::string name; };
struct PointCloud2 {
    typedef std::shared_ptr<const PointCloud2> ConstPtr;
    typedef std::shared_ptr<PointCloud2> Ptr;
    std_msgs::Header header;
    std::vector<PointField> fields;
};
typedef PointCloud2::ConstPtr PointCloud2ConstPtr;
struct Image { typedef std::shared_ptr<const Image> ConstPtr; std_msgs::Header header; };
typedef Image::ConstPtr ImageConstPtr;
struct CompressedImage { typedef std::shared_ptr<const CompressedImage> ConstPtr; std_msgs::Header header; std::string format; };
typedef CompressedImage::ConstPtr CompressedImageConstPtr;
namespace image_encodings { const std::string BGR8 = "bgr8"; }
}  // namespace sensor_msgs
