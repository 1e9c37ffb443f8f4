// mh_artic_pair.hip -- the articulated step for bodies with sphere contacts between links (include/moby_hip_artic.h: mh_artic_model.npairs,
// sphere_no_plane).
//
// The box kernels of mh_artic_box.hip with the pair work of mh_artic_contacts.inc switched in by MH_ARTIC_PAIR_TU (a contact names two links; six
// more entries in the contact list; calc_max_dist adds the base's velocity only below joint 0), compiled as a code object of their own so that
// the five older articulated code objects keep their code byte for byte.  Here the plain and the stabilising step in angle coordinates, each
// undriven and driven (k_artic_step_pair...), and their launcher artic_pair_launch, both stamped by the header from the family token; their pose
// forms are mh_artic_pair_pose.hip.  This code object also exports artic_pair_lds_bytes, the size of the pair layout's LDS image.  The router
// (mh_artic.hip: artic_geom_step) sends every batch with pairs or a plane mask here, and every batch with geometry created under
// mh_debug_set(13, 1).
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_GEOM pair
#include "mh_artic_dev.h"
