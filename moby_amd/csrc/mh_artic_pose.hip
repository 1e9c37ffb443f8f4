// mh_artic_pose.hip -- the articulated step in pose coordinates (include/moby_hip_artic.h: MH_ARTIC_BASE_POSE, mh_artic_batch_set_base_coords).
//
// The kernels of mh_artic_dev.h / mh_artic_contacts.inc with the floating base's pose switched in by MH_ARTIC_POSE_TU, compiled as a code object of
// their own, as mh_artic_drive.hip does for drives: the angle-coordinate kernels of mh_artic.hip and mh_artic_drive.hip keep their code byte for
// byte.  Here: the step at the default four-waves budget, the stabilising step and both contact steps, each undriven and driven; the forward
// dynamics / link poses and Jacobian kernels; the fold of the switch from angles; and the pose entry points of the C ABI.
#define MH_ARTIC_POSE_TU 1
#include "mh_artic_dev.h"

int artic_pose_step(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D)
{
  namespace ar = mh::artic;
  if (init_pow10() != MH_OK) return MH_ERR_HIP;
  const ar::Model* M = ab->d_model;
  const bool drv = D && D->terms != 0;
  const hipStream_t st = (hipStream_t)stream;
  if (ab->nspheres > 0) {
    const size_t lds = ar::lds_bytes_contacts(ab->nj);
    if (drv) hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_contacts_stab_pose_drive : ar::k_artic_step_contacts_pose_drive, dim3(ab->B), dim3(64), lds, st,
                                M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws, ab->d_pose, *D);
    else hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_contacts_stab_pose : ar::k_artic_step_contacts_pose, dim3(ab->B), dim3(64), lds, st,
                            M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws, ab->d_pose);
  } else if (ab->cstab) {
    const size_t lds = ar::lds_bytes(ab->nj, ar::NLSTAB);
    if (drv) hipLaunchKernelGGL(ar::k_artic_step_stab_pose_drive, dim3(ab->B), dim3(64), lds, st, M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_pose, *D);
    else hipLaunchKernelGGL(ar::k_artic_step_stab_pose, dim3(ab->B), dim3(64), lds, st, M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_pose);
  } else {                                                     // (MH_ARTIC_WAVES, MH_ARTIC_PACK / key 9: not in pose coordinates)
    const size_t lds = ar::lds_bytes(ab->nj);
    if (drv) hipLaunchKernelGGL(ar::k_artic_step_w4_pose_drive, dim3(ab->B), dim3(64), lds, st, M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_pose, *D);
    else hipLaunchKernelGGL(ar::k_artic_step_w4_pose, dim3(ab->B), dim3(64), lds, st, M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_pose);
  }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

hipError_t artic_pose_fwd_dyn_launch(mh_artic_batch* ab, void* stream, const double* d_tau, double* d_qdd, double* d_H, double* d_poses, int* d_ok)
{
  namespace ar = mh::artic;
  hipLaunchKernelGGL(ar::k_artic_fwd_dyn_pose, dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)stream,
                     (const ar::Model*)ab->d_model, ab->B, (const double*)ab->d_q, (const double*)ab->d_qd, d_tau, d_qdd, d_H, d_poses, d_ok, (const double*)ab->d_pose);
  return hipGetLastError();
}

hipError_t artic_pose_jacobian_launch(mh_artic_batch* ab, int link, const double* d_p, double* d_J)
{
  namespace ar = mh::artic;
  hipLaunchKernelGGL(ar::k_artic_jacobian_pose, dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)nullptr,
                     (const ar::Model*)ab->d_model, ab->B, (const double*)ab->d_q, link, d_p, d_J, (const double*)ab->d_pose);
  return hipGetLastError();
}

// the unit quaternion (w, x, y, z) of a rotation matrix (row-major), Shepperd's method: the largest of 4 w^2, 4 x^2, 4 y^2, 4 z^2 picks the branch
static void quat_of_R(const double* R, double* Q)
{
  const double tr = R[0] + R[4] + R[8];
  if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + tr);
    Q[0] = 0.25 * s; Q[1] = (R[7] - R[5]) / s; Q[2] = (R[2] - R[6]) / s; Q[3] = (R[3] - R[1]) / s;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]);
    Q[0] = (R[7] - R[5]) / s; Q[1] = 0.25 * s; Q[2] = (R[1] + R[3]) / s; Q[3] = (R[2] + R[6]) / s;
  } else if (R[4] >= R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]);
    Q[0] = (R[2] - R[6]) / s; Q[1] = (R[1] + R[3]) / s; Q[2] = 0.25 * s; Q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]);
    Q[0] = (R[3] - R[1]) / s; Q[1] = (R[2] + R[6]) / s; Q[2] = (R[5] + R[7]) / s; Q[3] = 0.25 * s;
  }
  const double n = std::sqrt(((Q[0] * Q[0] + Q[1] * Q[1]) + Q[2] * Q[2]) + Q[3] * Q[3]);
  for (int k = 0; k < 4; k++) Q[k] = Q[k] / n;
}

extern "C" {

int mh_artic_batch_set_base_coords(mh_artic_batch* ab, int coords)
{
  namespace ar = mh::artic;
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  if (coords != MH_ARTIC_BASE_ANGLES && coords != MH_ARTIC_BASE_POSE) return fail(MH_ERR_INVALID_ARG, "base coordinates %d: MH_ARTIC_BASE_ANGLES or MH_ARTIC_BASE_POSE", coords);
  if (coords == ab->base_coords) return MH_OK;
  if (coords == MH_ARTIC_BASE_ANGLES) return fail(MH_ERR_INVALID_ARG, "a batch in pose coordinates does not go back to angles (the model's pose is no longer its origin)");
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());                              // a step may be in flight on a caller's non-blocking stream
  ar::Model hm;
  MH_HIP(hipMemcpy(&hm, ab->d_model, sizeof(hm), hipMemcpyDeviceToHost));
  const mh_artic_model& m = hm.m;
  if (!m.floating_base) return fail(MH_ERR_INVALID_ARG, "pose coordinates need a floating base");
  const double INF_ = 1.7976931348623157e308;
  for (int v = 0; v < 6; v++)
    if (m.hilimit[v] < INF_ || m.lolimit[v] > -INF_) return fail(MH_ERR_INVALID_ARG, "joint %d: a finite limit on a virtual joint has no meaning in pose coordinates", v);
  double P0[7];
  for (int k = 0; k < 3; k++) P0[k] = m.trel[0][k];
  quat_of_R(m.Rrel[3], P0 + 3);
  const size_t B = (size_t)ab->B;
  std::vector<double> h(7 * B);
  for (size_t b = 0; b < B; b++) for (int k = 0; k < 7; k++) h[7 * b + k] = P0[k];
  if (ab->params) {                                            // per-world parameters: every world's pose from its own image (the topology checked above is shared)
    std::vector<ar::Model> images(B);
    MH_HIP(hipMemcpy(images.data(), ab->d_model, B * sizeof(ar::Model), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; b++) { for (int k = 0; k < 3; k++) h[7 * b + k] = images[b].m.trel[0][k]; quat_of_R(images[b].m.Rrel[3], h.data() + 7 * b + 3); }
  }
  double* d = nullptr;
  MH_HIP(hipMalloc((void**)&d, 7 * B * sizeof(double)));
  hipError_t e = hipMemcpy(d, h.data(), 7 * B * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(ar::k_artic_pose_fold, dim3((ab->B + 63) / 64), dim3(64), 0, (hipStream_t)nullptr, ab->B, ab->nj, ab->d_q, ab->d_qd, (const mh_world_aux*)ab->d_aux, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { (void)hipFree(d); return fail(MH_ERR_HIP, "switch to pose coordinates failed: %s", hipGetErrorString(e)); }
  ab->d_pose = d; ab->base_coords = MH_ARTIC_BASE_POSE;
  return MH_OK;
}

int mh_artic_batch_base_coords(const mh_artic_batch* ab, int* coords)
{
  if (!ab || !coords) return fail(MH_ERR_INVALID_ARG, "null batch / out");
  *coords = ab->base_coords;
  return MH_OK;
}

int mh_artic_batch_base_pose(mh_artic_batch* ab, double* pose)
{
  if (!ab || !pose) return fail(MH_ERR_INVALID_ARG, "null batch / buffer");
  if (ab->base_coords != MH_ARTIC_BASE_POSE) return fail(MH_ERR_INVALID_ARG, "the batch is in angle coordinates: no base pose");
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());
  MH_HIP(hipMemcpy(pose, ab->d_pose, (size_t)ab->B * 7 * sizeof(double), hipMemcpyDeviceToHost));
  return MH_OK;
}

int mh_artic_batch_set_base_pose(mh_artic_batch* ab, const double* pose)
{
  if (!ab || !pose) return fail(MH_ERR_INVALID_ARG, "null batch / buffer");
  if (ab->base_coords != MH_ARTIC_BASE_POSE) return fail(MH_ERR_INVALID_ARG, "the batch is in angle coordinates: no base pose");
  const size_t B = (size_t)ab->B;
  std::vector<double> h(pose, pose + 7 * B);
  for (size_t b = 0; b < B; b++) {
    double* P = h.data() + 7 * b;
    for (int k = 0; k < 7; k++) if (!std::isfinite(P[k])) return fail(MH_ERR_INVALID_ARG, "world %zu: a non-finite base pose", b);
    const double n = std::sqrt(((P[3] * P[3] + P[4] * P[4]) + P[5] * P[5]) + P[6] * P[6]);
    if (!(n > 0.0) || !std::isfinite(n)) return fail(MH_ERR_INVALID_ARG, "world %zu: the base quaternion has no direction", b);
    for (int k = 3; k < 7; k++) P[k] = P[k] / n;
  }
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());                              // a step may be reading the poses on a caller's stream
  MH_HIP(hipMemcpy(ab->d_pose, h.data(), 7 * B * sizeof(double), hipMemcpyHostToDevice));
  return MH_OK;
}

int mh_artic_batch_base_pose_dev(mh_artic_batch* ab, void* stream, double* dst)
{
  if (!ab || !dst) return fail(MH_ERR_INVALID_ARG, "null batch / buffer");
  if (ab->base_coords != MH_ARTIC_BASE_POSE) return fail(MH_ERR_INVALID_ARG, "the batch is in angle coordinates: no base pose");
  MH_ON_DEVICE(ab);
  MH_HIP(hipMemcpyAsync(dst, ab->d_pose, (size_t)ab->B * 7 * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MH_OK;
}

} // extern "C"
