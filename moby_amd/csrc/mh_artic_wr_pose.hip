// mh_artic_wr_pose.hip -- the link-wrench kernels of mh_artic_wr.hip in pose coordinates (include/moby_hip_artic.h: MH_ARTIC_BASE_POSE): the same
// bodies compiled with MH_ARTIC_POSE_TU too, a code object of their own because the pose switch changes the kinematics of the whole translation
// unit.  Launcher: artic_wr_pose_launch; image size: artic_wr_pose_lds_bytes.
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_BSP_TU 1
#define MH_ARTIC_REPORT_TU 1
#define MH_ARTIC_PARAMS_TU 1
#define MH_ARTIC_WRENCH_TU 1
#define MH_ARTIC_POSE_TU 1
#define MH_ARTIC_GEOM wr
#include "mh_artic_dev.h"
