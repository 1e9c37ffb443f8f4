// mh_artic_box.hip -- the articulated step for bodies with box primitives on their links (include/moby_hip_artic.h: mh_artic_model.nboxes).
//
// The contact kernels of mh_artic_dev.h / mh_artic_contacts.inc with the box work switched in by MH_ARTIC_BOX_TU, compiled as a code object of their
// own, as mh_artic_drive.hip and mh_artic_pose.hip do for drives and pose coordinates: the kernels of those three code objects keep their code
// byte for byte.  Here the plain and the stabilising contact step in angle coordinates, each undriven and driven (k_artic_step_box...; the drive
// is a pointer, NULL = undriven, as in mh_artic_pose.hip), and their launcher artic_box_launch, both stamped by the header from the family token;
// their pose forms are mh_artic_box_pose.hip.  The router (mh_artic.hip: artic_geom_step) sends every step of a batch whose model has boxes
// here, and that of a sphere-only batch under mh_debug_set(12, 1).
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_GEOM box
#include "mh_artic_dev.h"
