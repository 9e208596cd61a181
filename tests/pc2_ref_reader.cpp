// tests/pc2_ref_reader.cpp -- test-side driver of the reference's cloudProcessing::process (src/cloudProcessing.cpp:100-123) and the three
// handlers behind it: velodyneHandler (:325-433), ousterHandler (:216-323), robosenseHandler (:435-542).
// tests/pc2_reader.py compiles the reference's src/cloudProcessing.cpp where it lies, TOGETHER with this file, into a temporary directory:
// the include path puts tests/stub_pc2 (a PointCloud2 with real data, width, height, point_step, row_step and fields; a pcl::fromROSMsg
// that is declared and not defined) ahead of tests/stub_livox and oracle/ref_shim.  oracle/_ref/libref_path.so supplies time_list,
// time_list_velodyne, time_list_ouster and time_list_robosense (src/utility.cpp:16-34); the reader is linked with -Wl,-Bsymbolic so that
// the definitions of this shared object -- the reference's handlers -- are the ones its calls reach.
// Nothing of the handlers is restated here: their loops, their std::sort, their point3D are the reference's own.  What IS the test's:
// the three explicit specialisations of pcl::fromROSMsg below.  They look the named fields up in msg.fields and copy them into the
// reference's registered point structs, point by point, with memcpy.  That copy is this test's stand-in for PCL's field mapping.
// One cloudProcessing object lives across a list of messages (pcr_new ... pcr_feed ... pcr_free), so last_end_time carries from message
// to message as it does in the node; each feed hands back what that message queued.
#include <cstdint>
#include <cstring>
#include <memory>
#include <queue>
#include <stdexcept>

#include "cloudProcessing.h"

namespace {
// private members of cloudProcessing, read without touching the reference's header (a member pointer handed out by an explicit
// instantiation, which may name private members)
template <class Tag, typename Tag::type M> struct Rob {
    friend typename Tag::type get(Tag) { return M; }
};
struct LastEnd {
    typedef double cloudProcessing::*type;
    friend type get(LastEnd);
};
template struct Rob<LastEnd, &cloudProcessing::last_end_time>;

uint32_t field_offset(const sensor_msgs::PointCloud2 &msg, const char *name, uint8_t datatype) {
    for (const sensor_msgs::PointField &f : msg.fields)
        if (f.name == name) {
            if (f.datatype != datatype) throw std::runtime_error(std::string("field of another datatype: ") + name);
            return f.offset;
        }
    throw std::runtime_error(std::string("field missing: ") + name);
}
const uint8_t *point_at(const sensor_msgs::PointCloud2 &msg, size_t i) {
    return msg.data.data() + (i / msg.width) * (size_t)msg.row_step + (i % msg.width) * (size_t)msg.point_step;
}
template <class T> T read_at(const uint8_t *p) { T v; std::memcpy(&v, p, sizeof v); return v; }
template <class P> void copy_xyz(const sensor_msgs::PointCloud2 &msg, std::vector<P> &pts) {
    typedef sensor_msgs::PointField F;
    const uint32_t ox = field_offset(msg, "x", F::FLOAT32), oy = field_offset(msg, "y", F::FLOAT32), oz = field_offset(msg, "z", F::FLOAT32);
    pts.resize((size_t)msg.width * msg.height);
    for (size_t i = 0; i < pts.size(); i++) {
        const uint8_t *p = point_at(msg, i);
        pts[i].x = read_at<float>(p + ox); pts[i].y = read_at<float>(p + oy); pts[i].z = read_at<float>(p + oz);
    }
}

struct Reader {
    cloudProcessing cp;
    std::queue<point3D> q;
};
}  // namespace

namespace pcl {
typedef sensor_msgs::PointField F;
template <> void fromROSMsg(const sensor_msgs::PointCloud2 &msg, PointCloud<velodyne_ros::Point> &cloud) {
    copy_xyz(msg, cloud.points);
    const uint32_t ot = field_offset(msg, "time", F::FLOAT32), orr = field_offset(msg, "ring", F::UINT16);
    for (size_t i = 0; i < cloud.points.size(); i++) {
        cloud.points[i].time = read_at<float>(point_at(msg, i) + ot);
        cloud.points[i].ring = read_at<uint16_t>(point_at(msg, i) + orr);
    }
}
template <> void fromROSMsg(const sensor_msgs::PointCloud2 &msg, PointCloud<ouster_ros::Point> &cloud) {
    copy_xyz(msg, cloud.points);
    const uint32_t ot = field_offset(msg, "t", F::UINT32), orr = field_offset(msg, "ring", F::UINT8);
    for (size_t i = 0; i < cloud.points.size(); i++) {
        cloud.points[i].t = read_at<uint32_t>(point_at(msg, i) + ot);
        cloud.points[i].ring = read_at<uint8_t>(point_at(msg, i) + orr);
    }
}
template <> void fromROSMsg(const sensor_msgs::PointCloud2 &msg, PointCloud<robosense_ros::Point> &cloud) {
    copy_xyz(msg, cloud.points);
    const uint32_t ot = field_offset(msg, "timestamp", F::FLOAT64), orr = field_offset(msg, "ring", F::UINT16);
    for (size_t i = 0; i < cloud.points.size(); i++) {
        cloud.points[i].timestamp = read_at<double>(point_at(msg, i) + ot);
        cloud.points[i].ring = read_at<uint16_t>(point_at(msg, i) + orr);
    }
}
}  // namespace pcl

extern "C" {

void *pcr_new(int lidar_type, int n_scans, int scan_rate, int time_unit, double blind, int point_filter_num) {
    Reader *r = new Reader();
    r->cp.setLidarType(lidar_type);
    r->cp.setNumScans(n_scans);
    r->cp.setScanRate(scan_rate);
    r->cp.setTimeUnit(time_unit);
    r->cp.setBlind(blind);
    r->cp.setPointFilterNum(point_filter_num);
    return r;
}

void pcr_free(void *h) { delete static_cast<Reader *>(h); }

// layout: width, height, point_step, row_step, off_x, off_y, off_z, off_time, off_ring (the first nine members of srl_pc2_layout).
// out: capacity x 9 doubles per point this message queued (raw_point 3, point 3, relative_time, timestamp, alpha_time).  Returns their
// number (-1: the field lookup failed); *last_end_time as the class holds it afterwards, *given = isPointTimeEnable().
int pcr_feed(void *h, int lidar_type, const void *data, size_t data_bytes, const int32_t *layout, double stamp, double *out, int capacity, double *last_end_time,
             int *given) {
    Reader *r = static_cast<Reader *>(h);
    typedef sensor_msgs::PointField F;
    auto msg = std::make_shared<sensor_msgs::PointCloud2>();
    msg->header.stamp.fromSec(stamp);
    msg->width = (uint32_t)layout[0]; msg->height = (uint32_t)layout[1]; msg->point_step = (uint32_t)layout[2]; msg->row_step = (uint32_t)layout[3];
    const char *time_name = lidar_type == VELO ? "time" : lidar_type == OUST ? "t" : "timestamp";
    const uint8_t time_type = lidar_type == VELO ? F::FLOAT32 : lidar_type == OUST ? F::UINT32 : F::FLOAT64;
    const uint8_t ring_type = lidar_type == OUST ? F::UINT8 : F::UINT16;
    const char *names[5] = {"x", "y", "z", time_name, "ring"};
    const uint8_t types[5] = {F::FLOAT32, F::FLOAT32, F::FLOAT32, time_type, ring_type};
    for (int k = 0; k < 5; k++) {
        F f; f.name = names[k]; f.offset = (uint32_t)layout[4 + k]; f.datatype = types[k];
        msg->fields.push_back(f);
    }
    msg->data.assign(static_cast<const uint8_t *>(data), static_cast<const uint8_t *>(data) + data_bytes);
    sensor_msgs::PointCloud2::ConstPtr cmsg = msg;
    try {
        r->cp.process(cmsg, r->q);
    } catch (const std::exception &) { return -1; }
    *last_end_time = r->cp.*get(LastEnd());
    *given = msg->data.empty() || msg->width * msg->height == 0 ? -1 : (r->cp.isPointTimeEnable() ? 1 : 0);      // an empty message assigns neither
    const int count = (int)r->q.size();
    for (int k = 0; k < count; k++) {
        const point3D &p = r->q.front();
        if (k < capacity) {
            double *o = out + (size_t)k * 9;
            for (int d = 0; d < 3; d++) { o[d] = p.raw_point[d]; o[3 + d] = p.point[d]; }
            o[6] = p.relative_time; o[7] = p.timestamp; o[8] = p.alpha_time;
        }
        r->q.pop();
    }
    return count;
}

}  // extern "C"
