// mh_artic_pair_pose.hip -- the pair kernels of mh_artic_pair.hip in pose coordinates (include/moby_hip_artic.h: MH_ARTIC_BASE_POSE): the same
// bodies compiled with MH_ARTIC_BOX_TU, MH_ARTIC_PAIR_TU and MH_ARTIC_POSE_TU, a code object of their own because the pose switch changes the
// kinematics of the whole translation unit.  Launcher: artic_pair_pose_launch.
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_POSE_TU 1
#define MH_ARTIC_GEOM pair
#include "mh_artic_dev.h"
