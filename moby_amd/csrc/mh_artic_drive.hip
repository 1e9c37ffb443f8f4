// mh_artic_drive.hip -- the driven articulated step (include/moby_hip_artic.h: mh_artic_drive, mh_artic_batch_step_driven).
//
// The step kernels of mh_artic_dev.h with the drive switched in by MH_ARTIC_DRIVE_TU, compiled as a code object of their own: mh_artic.hip
// (MH_ARTIC_DRIVE_TU unset) holds the undriven kernels and every other entry point, this file the driven kernels and their launcher.  The
// preprocessor, not a template parameter, keeps the undriven kernels' source exactly what it was before drives existed, and with it their
// code (byte-identical ISA): a DRIVE template parameter, dead in the undriven instantiations, changed the register allocation of
// k_artic_step_w3 / w5 / contacts_stab (w5: six more spilled SGPRs).
#define MH_ARTIC_DRIVE_TU 1
#include "mh_artic_dev.h"

extern "C" {

int mh_artic_batch_step_driven(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* drive)
{
  namespace ar = mh::artic;
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  const mh_artic_drive& D = drive ? *drive : ab->drive;
  if (D.terms == 0) return mh_artic_batch_step(ab, stream, dt, nsteps);
  MH_ON_DEVICE(ab);
  if (nsteps < 0) return fail(MH_ERR_INVALID_ARG, "negative step count");
  const int rc = check_drive(&D, nsteps);
  if (rc != MH_OK) return rc;
  if (nsteps == 0) return MH_OK;
  if (!(dt > 0.0)) return fail(MH_ERR_INVALID_ARG, "dt must be > 0");
  if (artic_geom_family(ab) != MH_ARTIC_FAM_NONE) return artic_geom_step(ab, stream, dt, nsteps, &D);
  if (ab->base_coords == MH_ARTIC_BASE_POSE) return artic_pose_step(ab, stream, dt, nsteps, &D);
  if (init_pow10() != MH_OK) return MH_ERR_HIP;
  const ar::Model* M = ab->d_model;
  if (ab->nspheres > 0) {
    hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_contacts_stab_drive : ar::k_artic_step_contacts_drive, dim3(ab->B), dim3(64), ar::lds_bytes_contacts(ab->nj), (hipStream_t)stream,
                       M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws, D);
  } else if (ab->cstab) {
    hipLaunchKernelGGL(ar::k_artic_step_stab_drive, dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj, ar::NLSTAB), (hipStream_t)stream,
                       M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, D);
  } else {                                                     // (no two-worlds-per-wave form: key 9 / MH_ARTIC_PACK do not apply)
    static const int waves = [] { const char* e = std::getenv("MH_ARTIC_WAVES"); const int w = e ? std::atoi(e) : 4; return (w == 2 || w == 3 || w == 5) ? w : 4; }();
    hipLaunchKernelGGL(waves == 5 ? ar::k_artic_step_w5_drive : waves == 4 ? ar::k_artic_step_w4_drive : (waves == 2 ? ar::k_artic_step_w2_drive : ar::k_artic_step_w3_drive),
                       dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)stream, M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, D);
  }
  MH_HIP(hipGetLastError());
  return MH_OK;
}

} // extern "C"
