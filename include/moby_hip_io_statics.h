/* moby_hip_io_statics.h -- mh_io_load_xml with several static bodies (C ABI, libmoby_hip_io.so).
 *
 * mh_io_load_xml and mh_io_load_xml_forces (moby_hip_io.h, moby_hip_io_forces.h) take ONE disabled body, which must carry a <Plane>, as the scene's
 * ground, and refuse anything else; they stay exactly so.  This entry reads what mh_io_load_xml_forces reads, and makes EVERY disabled <RigidBody> of
 * the simulator a static body of the mh_world_statics record (include/moby_hip.h, "Static bodies"), in ascending id order:
 *
 *   a <Plane>   keeps the pose rules the ground has: the body's pose or the primitive's may rotate, not both; the plane's +Y is its normal
 *   a <Box>     takes the body's position and orientation (box centre, box axes) and the primitive's xlen / ylen / zlen; a box primitive with a pose
 *               of its own is refused
 *
 * Any other primitive on a disabled body is refused by name.  out->scene.has_ground = 0: the statics are bodies nb .. nb + n - 1, body_id[nb + k] holds
 * the id of static k, and <ContactParameters> / <DisabledPair> that name a static land in the scene's triangular pair slots over nb + n bodies.
 * nb + n must not exceed MH_MAX_BODIES + 1.
 */
#ifndef MOBY_HIP_IO_STATICS_H
#define MOBY_HIP_IO_STATICS_H
#include "moby_hip_io.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0 on success (*forces: terms == 0 when the scene lists none; forces may be NULL: then any force but gravity is refused, as mh_io_load_xml does);
 * nonzero on failure, mh_io_last_error() says why */
int mh_io_load_xml_statics(const char* path, mh_io_scene* out, mh_world_forces* forces, mh_world_statics* statics);

#ifdef __cplusplus
}
#endif
#endif
