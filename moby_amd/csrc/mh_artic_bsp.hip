// mh_artic_bsp.hip -- the articulated step for bodies with box-sphere contacts between links or static boxes (include/moby_hip_artic.h:
// mh_artic_model.pair_kind, box_link = -1).
//
// The pair kernels of mh_artic_pair.hip with the box-sphere work of mh_artic_contacts.inc switched in by MH_ARTIC_BSP_TU (the closed-form
// box-sphere contact and signed distance; a pair of either kind per pair slot; a static box has no plane work, no Jacobian term and
// calc_max_dist = 0), compiled as a code object of their own so that the seven older articulated code objects keep their code.  The contact list,
// the stabiliser vectors and the LDS image are the pair kernels' (62 520 bytes at 16 joints).  Here the plain and the stabilising step in angle
// coordinates, each undriven and driven; their pose forms are mh_artic_bsp_pose.hip.  artic_box_step hands every batch with a box-sphere pair
// or a static box on to artic_bsp_step, and every batch with geometry created under mh_debug_set(14, 1).
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_BSP_TU 1
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

int artic_bsp_step(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D)
{
  namespace ar = mh::artic;
  if (ab->d_ws && ab->ws_stride < ar::WS_PAIR) return fail(MH_ERR_INVALID_ARG, "the batch's workspace is not sized for the box-sphere kernels");
  const size_t lds = ar::lds_bytes_contacts(ab->nj);
  if (lds > 65536) return fail(MH_ERR_INVALID_ARG, "the box-sphere kernels' LDS image (%zu bytes) exceeds a workgroup's 64 KB", lds);
  if (ab->base_coords == MH_ARTIC_BASE_POSE) return artic_bsp_pose_launch(ab, stream, dt, nsteps, D);
  if (init_pow10() != MH_OK) return MH_ERR_HIP;
  const ar::Model* M = ab->d_model;
  const hipStream_t st = (hipStream_t)stream;
  if (D && D->terms != 0) hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_bsp_stab_drive : ar::k_artic_step_bsp_drive, dim3(ab->B), dim3(64), lds, st,
                                             M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws, *D);
  else hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_bsp_stab : ar::k_artic_step_bsp, dim3(ab->B), dim3(64), lds, st,
                          M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws);
  MH_HIP(hipGetLastError());
  return MH_OK;
}
