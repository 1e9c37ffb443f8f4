// The "wheel" variant of the many-worlds kernel (mh_world_wave.inc): <= 2 bodies, <= 3 pairs, <= 4 contacts, + spokes geometry and the no-slip model (rimless wheel).
// One translation unit per variant: the LDS image, occupancy and feature set differ, and the three compile in parallel.
#include <hip/hip_runtime.h>
#include "../../include/moby_hip.h"
#include "mh_host.h"
// mh_world_wheel_prof.hip (MH_PROFILE_BUILD) is the same kernel with the s_memtime stamps compiled in (mh_world_batch_profile), mh_world_wheel_forces.hip
// (MH_FORCES_BUILD) the one with recurrent forces and the caller's wrench in its forward dynamics (MHW_FORCES): mh_world_wave.inc derives their names.
#define MHW_BASE wheel
#define MHW_NOSLIP 1
#define MHW_BOX 0
#define MHW_NB 2
#define MHW_MAX_PAIRS 3
#define MHW_MAX_CONTACTS 4
#define MHW_MAX_ROWS 12
#define MHW_MAX_GROWS 12
#define MHW_WAVES_PER_SIMD 2
#include "mh_world_wave.inc"
