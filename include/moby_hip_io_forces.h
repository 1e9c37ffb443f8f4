/* moby_hip_io_forces.h -- mh_io_load_xml with the scene's recurrent forces (C ABI, libmoby_hip_io.so).
 *
 * mh_io_load_xml (moby_hip_io.h) takes gravity as the one recurrent force and refuses a scene that lists any other; it stays exactly so.
 * This entry reads what it reads, plus the two drag elements of the reference:
 *
 *   <StokesDragForce id drag-b drag-b-ang>                       src/StokesDragForce.cpp:68-85
 *   <DampingForce id> <Gains body-id klinear kangular klinear-sq kangular-sq> ...   src/DampingForce.cpp:115-175
 *
 * referenced by <RecurrentForce recurrent-force-id> children of the simulator, which pushes each onto every body (src/Simulator.cpp:921-951).  A
 * body without a <Gains> child has zero gains and still carries the damping term, as in the reference.  The result is the mh_world_forces record of
 * include/moby_hip.h, for mh_world_batch_set_forces.
 *
 * Refused with a message, never reordered: a simulator list in any order other than gravity, Stokes drag, damping (the order the stepper
 * accumulates in: the reference accumulates in list order); more than one force of a kind; a <Gains> child that names an unknown or a
 * disabled body.  <RecurrentForce> children of a <RigidBody> are not read.
 */
#ifndef MOBY_HIP_IO_FORCES_H
#define MOBY_HIP_IO_FORCES_H
#include "moby_hip_io.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0 on success (*forces: terms == 0 when the scene lists none); nonzero on failure, mh_io_last_error() says why */
int mh_io_load_xml_forces(const char* path, mh_io_scene* out, mh_world_forces* forces);

#ifdef __cplusplus
}
#endif
#endif
