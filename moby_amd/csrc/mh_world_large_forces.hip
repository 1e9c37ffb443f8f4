// The "large" variant of the many-worlds kernel with the scene's recurrent forces (Stokes drag, damping) and the caller's per-world body wrench in its forward
// dynamics: what a batch launches once forces are stored or a wrench is passed (mh_world_batch_set_forces / mh_world_batch_step_wrench).  The plain kernel of
// mh_world_large.hip carries none of it.  Same launch bounds, same LDS image plus 12 MHW_NB doubles.
#define MH_FORCES_BUILD 1
#include "mh_world_large.hip"
