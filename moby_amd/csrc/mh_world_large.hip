// The "large" variant of the many-worlds kernel (mh_world_wave.inc): <= 8 bodies, <= 36 pairs, <= 40 contacts, <= 24 rows per island, every feature.
// One translation unit per variant: the LDS image, occupancy and feature set differ, and the three compile in parallel.
#include <hip/hip_runtime.h>
#include "../../include/moby_hip.h"
#include "mh_host.h"
#ifdef MH_PROFILE_BUILD      /* mh_world_large_prof.hip: the same kernel with the s_memtime stamps compiled in (mh_world_batch_profile) */
#define MHW_NS large_prof
#define MHW_VARIANT_GETTER mh_world_variant_large_prof
#elif defined(MH_FORCES_BUILD) /* mh_world_large_forces.hip: the same kernel with recurrent forces and the caller's wrench in its forward dynamics (MHW_FORCES) */
#define MHW_NS large_forces
#define MHW_VARIANT_GETTER mh_world_variant_large_forces
#define MHW_VARIANT_T mh_world_forced_variant
#define MHW_FORCES 1
#else
#define MHW_NS large
#define MHW_VARIANT_GETTER mh_world_variant_large
#endif
#define MHW_NOSLIP 1
#define MHW_BOX 1
#define MHW_NB MH_MAX_BODIES
#define MHW_MAX_PAIRS MH_MAX_PAIRS
#define MHW_MAX_CONTACTS 40   /* the stabiliser lists one contact per candidate pair (up to 36), a box adds up to 8 */
#define MHW_MAX_ROWS 24
#define MHW_MAX_GROWS 24
#define MHW_WAVES_PER_SIMD 2
#include "mh_world_wave.inc"
