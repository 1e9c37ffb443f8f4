// mh_artic_box.hip -- the articulated step for bodies with box primitives on their links (include/moby_hip_artic.h: mh_artic_model.nboxes).
//
// The contact kernels of mh_artic.hip / mh_artic_contacts.inc with the box work switched in by MH_ARTIC_BOX_TU, compiled as a code object of their
// own, as mh_artic_drive.hip and mh_artic_pose.hip do for drives and pose coordinates: the kernels of those three code objects keep their code
// byte for byte.  Here the plain and the stabilising contact step in angle coordinates, each undriven and driven (the drive is a pointer, NULL =
// undriven, as in mh_artic_pose.hip); their pose forms are mh_artic_box_pose.hip.  The host side routes every step of a batch whose model has boxes
// here, and that of a sphere-only batch under mh_debug_set(12, 1).
#define MH_ARTIC_BOX_TU 1
#include "mh_artic.hip"

// this code object's copy of the regularisation ladder's powers of ten (mh_artic_batch_create fills mh_artic.hip's), once per device
static int init_pow10()
{
  static std::mutex mu; static std::vector<char> done;
  std::lock_guard<std::mutex> lk(mu);
  int dev = 0; MH_HIP(hipGetDevice(&dev));
  if ((int)done.size() <= dev) done.resize(dev + 1, 0);
  if (!done[dev]) {
    mh::Pow10Table p10; for (int i = 0; i < 64; i++) p10.v[i] = std::pow(10.0, (double)(i - 32));   // LCP.cpp:285
    MH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mh::artic::c_pow10a), &p10, sizeof(p10)));
    done[dev] = 1;
  }
  return MH_OK;
}

int artic_box_step(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D)
{
  namespace ar = mh::artic;
  if (ab->use_bsp) return artic_bsp_step(ab, stream, dt, nsteps, D);     // a box-sphere pair, a static box, or a batch created under mh_debug_set(14, 1)
  if (ab->use_pair) return artic_pair_step(ab, stream, dt, nsteps, D);   // sphere pairs, a plane mask, or a batch created under mh_debug_set(13, 1)
  if (ab->d_ws && ab->ws_stride < ar::WS_BOX)                  // a sphere batch created before mh_debug_set(12, 1): its workspace has the sphere kernels' layout
    return fail(MH_ERR_INVALID_ARG, "mh_debug_set(12, 1) applies to batches created after it (their workspace is sized for the box kernels at create)");
  if (ab->base_coords == MH_ARTIC_BASE_POSE) return artic_box_pose_launch(ab, stream, dt, nsteps, D);
  if (init_pow10() != MH_OK) return MH_ERR_HIP;
  const ar::Model* M = ab->d_model;
  const size_t lds = ar::lds_bytes_contacts(ab->nj);
  const hipStream_t st = (hipStream_t)stream;
  if (D && D->terms != 0) hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_box_stab_drive : ar::k_artic_step_box_drive, dim3(ab->B), dim3(64), lds, st,
                                             M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws, *D);
  else hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_box_stab : ar::k_artic_step_box, dim3(ab->B), dim3(64), lds, st,
                          M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws);
  MH_HIP(hipGetLastError());
  return MH_OK;
}
