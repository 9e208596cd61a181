// tests/stub_pc2/pcl_conversions/pcl_conversions.h -- NOT PCL.  The stand-in of oracle/ref_shim plus a DECLARATION of pcl::fromROSMsg: the
// three handlers of src/cloudProcessing.cpp call it, and tests/pc2_ref_reader.cpp defines the three explicit specialisations they reach
// (a copy of the named fields into the reference's point structs: the test's stand-in for PCL's field mapping).
#pragma once
#include <pcl/point_types.h>
namespace pcl {
template <class M, class C> void fromROSMsg(const M &msg, C &cloud);
}  // namespace pcl
