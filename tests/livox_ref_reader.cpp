// tests/livox_ref_reader.cpp -- test-side driver of the reference's cloudProcessing::livoxHandler (src/cloudProcessing.cpp:125-214).
// tests/test_livox_checker_reference.py compiles the reference's src/cloudProcessing.cpp where it lies, TOGETHER with this file, into its
// temporary directory: the include path puts tests/stub_livox (a CustomMsg with real points, point_num and header) ahead of oracle/ref_shim,
// whose stand-in for that message is an empty shell.  oracle/_ref/libref_path.so supplies time_list (src/utility.cpp:16) and also exports an
// empty cloudProcessing::livoxHandler of the harness's own, so the reader is linked with -Wl,-Bsymbolic: the definitions of this shared
// object -- the reference's -- are the ones its calls reach.  Nothing is restated here: the function called is the reference's own, its
// std::sort and its point3D included; this file only fills the message and copies the queue out.
#include <cstdint>
#include <cstring>
#include <memory>
#include <queue>

#include "cloudProcessing.h"

namespace {
// cloudProcessing::last_end_time is private; this reads it without touching the reference's header (a member pointer handed out by an
// explicit instantiation, which may name private members)
template <class Tag, typename Tag::type M> struct Rob {
    friend typename Tag::type get(Tag) { return M; }
};
struct LastEnd {
    typedef double cloudProcessing::*type;
    friend type get(LastEnd);
};
template struct Rob<LastEnd, &cloudProcessing::last_end_time>;
}  // namespace

extern "C" {

// points: n records of 20 bytes.  out: capacity x 9 doubles per queued point (raw_point 3, point 3, relative_time, timestamp, alpha_time).
// Returns the number of points queued (they are all written when capacity suffices), *last_end_time as the class holds it afterwards.
int lrr_livox(const void *points, int n, double stamp, int n_scans, int time_unit, double blind, int point_filter_num, double *out, int capacity,
              double *last_end_time) {
    cloudProcessing cp;
    cp.setNumScans(n_scans);
    cp.setTimeUnit(time_unit);
    cp.setBlind(blind);
    cp.setPointFilterNum(point_filter_num);
    auto msg = std::make_shared<livox_ros_driver::CustomMsg>();
    msg->header.stamp.fromSec(stamp);
    msg->point_num = (uint32_t)n;
    msg->points.resize((size_t)n);
    static_assert(sizeof(livox_ros_driver::CustomPoint) == 20, "record size");
    if (n > 0) std::memcpy(msg->points.data(), points, (size_t)n * 20);
    std::queue<point3D> q;
    livox_ros_driver::CustomMsg::ConstPtr cmsg = msg;
    cp.livoxHandler(cmsg, q);
    *last_end_time = cp.*get(LastEnd());
    const int count = (int)q.size();
    for (int k = 0; k < count && k < capacity; k++) {
        const point3D &p = q.front();
        double *o = out + (size_t)k * 9;
        for (int d = 0; d < 3; d++) { o[d] = p.raw_point[d]; o[3 + d] = p.point[d]; }
        o[6] = p.relative_time; o[7] = p.timestamp; o[8] = p.alpha_time;
        q.pop();
    }
    return count;
}

}  // extern "C"
