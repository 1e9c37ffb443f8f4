// The "large" variant of the many-worlds kernel (mh_world_wave.inc) with per-world parameters (MHW_PARAMS, on top of MHW_STATICS): what a batch created
// with mh_world_params records launches, whatever its scene, or one that would take the statics build under mh_debug_set(17, 1).  The cache fill of the
// kernel entry reads every value from the world's own record behind the statics record; nothing after the fill differs from mh_world_large_st.hip, whose
// constants these are: <= 8 bodies, <= 36 pairs over <= 9 bodies and statics, <= 40 contacts, <= 24 rows per island, every feature.  A translation unit of
// its own, so that the other large kernels stay the code objects they were.
#include <hip/hip_runtime.h>
#include "../../include/moby_hip.h"
#include "mh_host.h"
#define MHW_BASE large_pw      /* mh_world_large_pw_forces.hip (MH_FORCES_BUILD): the same kernel with recurrent forces and the caller's wrench in its forward dynamics */
#define MHW_PARAMS 1
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
