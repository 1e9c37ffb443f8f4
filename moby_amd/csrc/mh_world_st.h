// The statics build of the large world variant (mh_world_large_st.hip, mh_world_large_st_forces.hip: mh_world_wave.inc with MHW_STATICS) as the host side
// sees it.  A header of its own, included by the statics translation units, mh_world.hip and mh_capi.hip only: the other world code objects include what
// they included and compile from the text they had.
#ifndef MH_WORLD_ST_H
#define MH_WORLD_ST_H
#include "mh_host.h"
extern "C" {   // (as in mh_host.h: C linkage so that the definitions may sit inside the extern "C" blocks of the ABI files)
MH_HIDDEN const mh_world_variant* mh_world_variant_large_st();
MH_HIDDEN const mh_world_forced_variant* mh_world_variant_large_st_forces();
extern MH_HIDDEN int mh_g_debug_world_st;            // mh_debug_set(16, v): batches that would take the box-sphere build through the statics build
}  // extern "C"
#endif
