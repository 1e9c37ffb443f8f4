// The "wheel" variant of the many-worlds kernel (mh_world_wave.inc): <= 2 bodies, <= 3 pairs, <= 4 contacts, + spokes geometry and the no-slip model (rimless wheel).
// One translation unit per variant: the LDS image, occupancy and feature set differ, and the three compile in parallel.
#include <hip/hip_runtime.h>
#include "../../include/moby_hip.h"
#include "mh_host.h"
#ifdef MH_PROFILE_BUILD      /* mh_world_wheel_prof.hip: the same kernel with the s_memtime stamps compiled in (mh_world_batch_profile) */
#define MHW_NS wheel_prof
#define MHW_VARIANT_GETTER mh_world_variant_wheel_prof
#elif defined(MH_FORCES_BUILD) /* mh_world_wheel_forces.hip: the same kernel with recurrent forces and the caller's wrench in its forward dynamics (MHW_FORCES) */
#define MHW_NS wheel_forces
#define MHW_VARIANT_GETTER mh_world_variant_wheel_forces
#define MHW_VARIANT_T mh_world_forced_variant
#define MHW_FORCES 1
#else
#define MHW_NS wheel
#define MHW_VARIANT_GETTER mh_world_variant_wheel
#endif
#define MHW_NOSLIP 1
#define MHW_BOX 0
#define MHW_NB 2
#define MHW_MAX_PAIRS 3
#define MHW_MAX_CONTACTS 4
#define MHW_MAX_ROWS 12
#define MHW_MAX_GROWS 12
#define MHW_WAVES_PER_SIMD 2
#include "mh_world_wave.inc"
