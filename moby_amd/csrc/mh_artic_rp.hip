// mh_artic_rp.hip -- the articulated step with the per-slot contact impulse report (include/moby_hip_artic.h, "Contact report").
//
// The box-sphere kernels of mh_artic_bsp.hip with the report switched in by MH_ARTIC_REPORT_TU: per contact an accumulator of the impulses the
// impact handler applied (LayC::racc, added to by every `apply`), the contact's slot (LayC::rslot, written where the contact list is built), and
// report_fold at the end of do_mini_step, which adds a mini-step's contacts to the step's rows in global memory.  Every line of that sits under
// the switch in mh_artic_contacts.inc, and this is a code object of its own, so that the nine older articulated code objects keep their code.
// The LDS image is the pair layout's plus 3 MH_NOSLIP_MAX doubles and the slot table (63 200 bytes at 16 joints); this file exports its size,
// artic_rp_lds_bytes.  Here the plain and the stabilising step in angle coordinates, each undriven and driven (k_artic_step_rp...), with one
// trailing argument, the rows or NULL, and their launcher artic_rp_launch; their pose forms are mh_artic_rp_pose.hip.  The router (mh_artic.hip:
// artic_geom_step) sends every batch of mh_artic_batch_create_report here, whatever its geometry, and every batch that would take the box-sphere
// kernels created under mh_debug_set(19, 1).
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_BSP_TU 1
#define MH_ARTIC_REPORT_TU 1
#define MH_ARTIC_GEOM rp
#include "mh_artic_dev.h"
