// The contact-report build of the "large" variant (mh_world_large_rp.hip) with the scene's recurrent forces and the caller's per-world body wrench in its
// forward dynamics: what a batch created for the report launches once forces are stored or a wrench is passed.
#define MH_FORCES_BUILD 1
#include "mh_world_large_rp.hip"
