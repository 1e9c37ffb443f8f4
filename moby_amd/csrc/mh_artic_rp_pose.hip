// mh_artic_rp_pose.hip -- the report kernels of mh_artic_rp.hip in pose coordinates (include/moby_hip_artic.h: MH_ARTIC_BASE_POSE): the same
// bodies compiled with MH_ARTIC_BOX_TU, MH_ARTIC_PAIR_TU, MH_ARTIC_BSP_TU, MH_ARTIC_REPORT_TU and MH_ARTIC_POSE_TU, a code object of their own
// because the pose switch changes the kinematics of the whole translation unit.  Launcher: artic_rp_pose_launch; image size: artic_rp_pose_lds_bytes.
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_BSP_TU 1
#define MH_ARTIC_REPORT_TU 1
#define MH_ARTIC_POSE_TU 1
#define MH_ARTIC_GEOM rp
#include "mh_artic_dev.h"
