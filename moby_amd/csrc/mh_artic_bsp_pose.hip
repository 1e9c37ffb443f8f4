// mh_artic_bsp_pose.hip -- the box-sphere kernels of mh_artic_bsp.hip in pose coordinates (include/moby_hip_artic.h: MH_ARTIC_BASE_POSE): the
// same bodies compiled with MH_ARTIC_BOX_TU, MH_ARTIC_PAIR_TU, MH_ARTIC_BSP_TU and MH_ARTIC_POSE_TU, a code object of their own because the
// pose switch changes the kinematics of the whole translation unit.
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_BSP_TU 1
#define MH_ARTIC_POSE_TU 1
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

int artic_bsp_pose_launch(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D)
{
  namespace ar = mh::artic;
  if (init_pow10() != MH_OK) return MH_ERR_HIP;
  const ar::Model* M = ab->d_model;
  const size_t lds = ar::lds_bytes_contacts(ab->nj);
  const hipStream_t st = (hipStream_t)stream;
  if (D && D->terms != 0) hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_bsp_stab_pose_drive : ar::k_artic_step_bsp_pose_drive, dim3(ab->B), dim3(64), lds, st,
                                             M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws, ab->d_pose, *D);
  else hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_bsp_stab_pose : ar::k_artic_step_bsp_pose, dim3(ab->B), dim3(64), lds, st,
                          M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws, ab->d_pose);
  MH_HIP(hipGetLastError());
  return MH_OK;
}
