// cameraState.h (host mirror) -- the camera members of class state (include/state.h:24-36) that imageProcessing::vioEsikf and
// vioPhotometric read and write, beside the pose they are chained to.  Kept apart from state.h: the LIO path does not carry them.
#pragma once
#include "srl_la.h"

namespace srlivo {

struct cameraState {
    double time_td = 0.0;
    srl::Mat3 R_imu_camera = srl::Mat3::Identity();
    srl::Vec3 t_imu_camera = srl::Vec3::Zero();
    double fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0;
    srl::Quat q_world_camera;
    srl::Vec3 t_world_camera = srl::Vec3::Zero();
    srl::Quat rotation;                                  // state::rotation, translation: the IMU pose the camera pose follows
    srl::Vec3 translation = srl::Vec3::Zero();
};
enum { SRL_CAMERA_STATE_DOUBLES = 31 };                  // time_td, R (9, row-major), t (3), fx fy cx cy, q_wc (w x y z), t_wc (3), rotation (w x y z), translation (3)

}  // namespace srlivo
