// The "large" variant of the many-worlds kernel (mh_world_wave.inc) with the per-pair contact impulse report (MHW_REPORT, on top of MHW_PARAMS): what a
// batch created with mh_world_batch_create_report launches, whatever its scene, or one that would take the per-world-parameters build under
// mh_debug_set(18, 1).  The kernel takes one more argument, the report rows (NULL: nothing is written, the steps are the same); beside that it is
// mh_world_large_pw.hip, whose constants these are, plus 3 MHW_MAX_CONTACTS doubles of accumulated (cn, cs, ct) and the fold of each mini-step's contacts
// into the step's rows.  A translation unit of its own, so that the other large kernels stay the code objects they were.
#include <hip/hip_runtime.h>
#include "../../include/moby_hip.h"
#include "mh_host.h"
#define MHW_BASE large_rp      /* mh_world_large_rp_forces.hip (MH_FORCES_BUILD): the same kernel with recurrent forces and the caller's wrench in its forward dynamics */
#define MHW_REPORT 1
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
