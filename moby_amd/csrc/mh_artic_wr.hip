// mh_artic_wr.hip -- the articulated step with link wrenches and link damping (include/moby_hip_artic.h, "Link wrenches").
//
// The per-world-parameters kernels of mh_artic_pw.hip with MH_ARTIC_WRENCH_TU, under which the step's own forward-dynamics call evaluates the
// launch's mh_artic_wrench right after kin_inertia (mh_artic_dev.h: link_wrench) and adds the resulting generalized force to the tau the drive
// wrote.  Every line of it sits under the switch, and this is a code object of its own, so that the thirteen older articulated code objects keep
// their code.  Here the plain and the stabilising step in angle coordinates, each undriven and driven (k_artic_step_wr...), with the rows or NULL
// as the report kernels take them and the wrench by value behind them (terms 0 = none), their launcher artic_wr_launch and image size
// artic_wr_lds_bytes.  Pose forms: mh_artic_wr_pose.hip.  The forward dynamics / link poses / Jacobian queries and the record scatter of such a
// batch stay those of mh_artic_pw.hip.  The router (mh_artic.hip: artic_geom_step) sends every batch of mh_artic_batch_create_wrench here, and
// every batch that would take the per-world-parameters kernels created under mh_debug_set(21, 1).
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_BSP_TU 1
#define MH_ARTIC_REPORT_TU 1
#define MH_ARTIC_PARAMS_TU 1
#define MH_ARTIC_WRENCH_TU 1
#define MH_ARTIC_GEOM wr
#include "mh_artic_dev.h"
