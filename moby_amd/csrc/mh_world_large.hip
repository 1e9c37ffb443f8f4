// The "large" variant of the many-worlds kernel (mh_world_wave.inc): <= 8 bodies, <= 36 pairs, <= 40 contacts, <= 24 rows per island, every feature.
// One translation unit per variant: the LDS image, occupancy and feature set differ, and the three compile in parallel.
#include <hip/hip_runtime.h>
#include "../../include/moby_hip.h"
#include "mh_host.h"
// mh_world_large_prof.hip (MH_PROFILE_BUILD) is the same kernel with the s_memtime stamps compiled in (mh_world_batch_profile), mh_world_large_forces.hip
// (MH_FORCES_BUILD) the one with recurrent forces and the caller's wrench in its forward dynamics (MHW_FORCES): mh_world_wave.inc derives their names.
#define MHW_BASE large
#define MHW_NOSLIP 1
#define MHW_BOX 1
#define MHW_NB MH_MAX_BODIES
#define MHW_MAX_PAIRS MH_MAX_PAIRS
#define MHW_MAX_CONTACTS 40   /* the stabiliser lists one contact per candidate pair (up to 36), a box adds up to 8 */
#define MHW_MAX_ROWS 24
#define MHW_MAX_GROWS 24
#define MHW_WAVES_PER_SIMD 2
#include "mh_world_wave.inc"
