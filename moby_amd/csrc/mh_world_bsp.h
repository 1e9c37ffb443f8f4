// The box-sphere build of the large world variant (mh_world_large_bsp.hip, mh_world_large_bsp_forces.hip: mh_world_wave.inc with MHW_BSP) as the host
// side sees it.  A header of its own, included by the box-sphere translation units, mh_world.hip and mh_capi.hip only: the other world code objects
// include mh_host.h alone and compile from the text they had.
#ifndef MH_WORLD_BSP_H
#define MH_WORLD_BSP_H
#include "mh_host.h"
extern "C" {   // (as in mh_host.h: C linkage so that the definitions may sit inside the extern "C" blocks of the ABI files)
MH_HIDDEN const mh_world_variant* mh_world_variant_large_bsp();
MH_HIDDEN const mh_world_forced_variant* mh_world_variant_large_bsp_forces();
extern MH_HIDDEN int mh_g_debug_world_bsp;           // mh_debug_set(15, v): batches that would take the large world variant through its box-sphere build
}  // extern "C"
#endif
