// The "large" variant of the many-worlds kernel (mh_world_wave.inc) with static bodies beside the free ones (MHW_STATICS, on top of MHW_BSP): what a batch
// created with a non-empty mh_world_statics launches, or one that would take the box-sphere build under mh_debug_set(16, 1).  The constants are
// mh_world_large.hip's: <= 8 bodies, <= 36 pairs over <= 9 bodies and statics, <= 40 contacts, <= 24 rows per island, every feature.  A translation unit of
// its own, so that the other large kernels stay the code objects they were.
#include <hip/hip_runtime.h>
#include "../../include/moby_hip.h"
#include "mh_host.h"
#define MHW_BASE large_st      /* mh_world_large_st_forces.hip (MH_FORCES_BUILD): the same kernel with recurrent forces and the caller's wrench in its forward dynamics */
#define MHW_STATICS 1
#define MHW_BSP 1
#define MHW_NOSLIP 1
#define MHW_BOX 1
#define MHW_NB MH_MAX_BODIES
#define MHW_MAX_PAIRS MH_MAX_PAIRS
#define MHW_MAX_CONTACTS 40   /* the stabiliser lists one contact per candidate pair (up to 36), a box adds up to 8 */
#define MHW_MAX_ROWS 24
#define MHW_MAX_GROWS 24
#define MHW_WAVES_PER_SIMD 2
#include "mh_world_wave.inc"
