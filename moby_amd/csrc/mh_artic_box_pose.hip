// mh_artic_box_pose.hip -- the box kernels of mh_artic_box.hip in pose coordinates (include/moby_hip_artic.h: MH_ARTIC_BASE_POSE): the same
// bodies compiled with MH_ARTIC_BOX_TU and MH_ARTIC_POSE_TU, a code object of their own because the pose switch changes the kinematics of the
// whole translation unit.  Launcher: artic_box_pose_launch.
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_POSE_TU 1
#define MH_ARTIC_GEOM box
#include "mh_artic_dev.h"
