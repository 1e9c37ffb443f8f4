// mh_artic_bsp.hip -- the articulated step for bodies with box-sphere contacts between links or static boxes (include/moby_hip_artic.h:
// mh_artic_model.pair_kind, box_link = -1).
//
// The pair kernels of mh_artic_pair.hip with the box-sphere work of mh_artic_contacts.inc switched in by MH_ARTIC_BSP_TU (the closed-form
// box-sphere contact and signed distance; a pair of either kind per pair slot; a static box has no plane work, no Jacobian term and
// calc_max_dist = 0), compiled as a code object of their own so that the seven older articulated code objects keep their code.  The contact list,
// the stabiliser vectors and the LDS image are the pair kernels' (62 520 bytes at 16 joints).  Here the plain and the stabilising step in angle
// coordinates, each undriven and driven (k_artic_step_bsp...), and their launcher artic_bsp_launch, both stamped by the header from the family
// token; their pose forms are mh_artic_bsp_pose.hip.  The router (mh_artic.hip: artic_geom_step) sends every batch with a box-sphere pair or a
// static box here, and every batch with geometry created under mh_debug_set(14, 1).
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_BSP_TU 1
#define MH_ARTIC_GEOM bsp
#include "mh_artic_dev.h"
