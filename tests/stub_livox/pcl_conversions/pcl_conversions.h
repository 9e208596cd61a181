// tests/stub_livox/pcl_conversions/pcl_conversions.h -- NOT PCL.  The stand-in of oracle/ref_shim plus an inert pcl::fromROSMsg, so that the
// PointCloud2 handlers of src/cloudProcessing.cpp compile beside livoxHandler (they are never called).
#pragma once
#include <pcl/point_types.h>
namespace pcl {
template <class M, class C> void fromROSMsg(const M &, C &) {}
}  // namespace pcl
