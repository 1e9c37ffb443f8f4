// The "large" variant of the many-worlds kernel (mh_world_wave.inc) with box-sphere contacts between free bodies (MHW_BSP): what a batch launches when its
// scene enables at least one box-sphere pair, or under mh_debug_set(15, 1).  The constants are mh_world_large.hip's: <= 8 bodies, <= 36 pairs, <= 40 contacts,
// <= 24 rows per island, every feature.  A translation unit of its own, so that the plain large kernels stay the code objects they were.
#include <hip/hip_runtime.h>
#include "../../include/moby_hip.h"
#include "mh_host.h"
#define MHW_BASE large_bsp     /* mh_world_large_bsp_forces.hip (MH_FORCES_BUILD): the same kernel with recurrent forces and the caller's wrench in its forward dynamics */
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
