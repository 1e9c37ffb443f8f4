// TEST INFRASTRUCTURE: the articulated step in pose coordinates the GPU kernels are held to (include/moby_hip_artic.h, MH_ARTIC_BASE_POSE).
//
// Pose coordinates change two numbers of the model per world: trel[0] = p and Rrel[3] = R(Q).  So a world here is a COPY of the model with those
// two replaced, stepped by the driven reference (artic_drive_ref.cpp: oracle::Artic::step with the drive), one step at a time with that step's
// drive row; after a step that ran to its end (aux.steps counted it) the virtual joints are folded into (p, Q).  Nothing of the oracle is
// restated but the fold, whose operation order the device (mh_artic.hip, pose_fold) follows bit for bit.
// Built by the tests with g++ and oracle/Makefile's CXXFLAGS (-ffp-contract=off), linked with artic_drive_ref.cpp into one library.
#include <cmath>
#include <cstring>
#include "lcp.hpp"
#include "world.hpp"
#include "artic.hpp"

extern "C" void artic_drive_ref_step(const mh_artic_model* m, int B, double dt, int nsteps, double* q, double* qd, mh_world_aux* aux, const mh_artic_drive* drive);

namespace {

// Hamilton product o = a (x) b, quaternions stored w, x, y, z
void quat_mul(const double* a, const double* b, double* o)
{
  o[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
  o[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
  o[2] = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
  o[3] = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
}

// R(Q), row-major, for a unit Q
void quat_R(const double* Q, double* R)
{
  const double w = Q[0], x = Q[1], y = Q[2], z = Q[3];
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz);       R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = 1.0 - 2.0 * (xx + yy);
}

// THE fold (one world; q, qd its joint arrays, P its pose p, Q):
//   p += q[0..2]                                                   -- the sum kinematics forms for the base COM (sliders along global axes, Rrel = I)
//   Q = normalize(Q (x) Qx(q3) (x) Qy(q4) (x) Qz(q5))              -- half-angle sin / cos from sincos_kernel
//   qd[3..5] = Rz(q5)' (Ry(q4)' (e_x qd3 + e_y qd4) + e_z qd5)     -- = Rh' (e_x qd3 + Rx e_y qd4 + Rx Ry e_z qd5), Rh = Rx Ry Rz; full-angle
//                                                                     sin / cos by the double-angle formulas from the half angles
//   q[0..5] = 0; qd[0..2] and the body's own joints unchanged
void fold(double* q, double* qd, double* P)
{
  double* p = P; double* Q = P + 3;
  for (int k = 0; k < 3; k++) p[k] = p[k] + q[k];
  double s3, c3, s4, c4, s5, c5;
  oracle::sincos_kernel(0.5 * q[3], s3, c3); oracle::sincos_kernel(0.5 * q[4], s4, c4); oracle::sincos_kernel(0.5 * q[5], s5, c5);
  const double qx[4] = { c3, s3, 0.0, 0.0 }, qy[4] = { c4, 0.0, s4, 0.0 }, qz[4] = { c5, 0.0, 0.0, s5 };
  double t1[4], t2[4], t3[4];
  quat_mul(Q, qx, t1); quat_mul(t1, qy, t2); quat_mul(t2, qz, t3);
  const double n = std::sqrt(((t3[0] * t3[0] + t3[1] * t3[1]) + t3[2] * t3[2]) + t3[3] * t3[3]);
  for (int k = 0; k < 4; k++) Q[k] = t3[k] / n;
  const double S4 = 2.0 * (s4 * c4), C4 = c4 * c4 - s4 * s4, S5 = 2.0 * (s5 * c5), C5 = c5 * c5 - s5 * s5;
  const double u0 = C4 * qd[3], u1 = qd[4], u2 = S4 * qd[3] + qd[5];
  qd[3] = C5 * u0 + S5 * u1; qd[4] = C5 * u1 - S5 * u0; qd[5] = u2;
  for (int k = 0; k < 6; k++) q[k] = 0.0;
}

void world_model(const mh_artic_model* m, const double* P, mh_artic_model* out)
{
  std::memcpy(out, m, sizeof(*m));
  for (int k = 0; k < 3; k++) out->trel[0][k] = P[k];
  quat_R(P + 3, out->Rrel[3]);
}

}  // namespace

extern "C" {

// the fold of every world (B x nj q, qd; B x 7 poses), in place
void artic_pose_ref_fold(int B, int nj, double* q, double* qd, double* pose)
{
  for (int b = 0; b < B; b++) fold(q + (size_t)b * nj, qd + (size_t)b * nj, pose + 7 * (size_t)b);
}

// world b's model: m with trel[0] = p, Rrel[3] = R(Q)
void artic_pose_ref_model(const mh_artic_model* m, const double* pose, mh_artic_model* out) { world_model(m, pose, out); }

// B worlds x nsteps in pose coordinates, in place (drive: HOST arrays laid out as mh_artic_drive states; NULL or terms == 0 = undriven)
void artic_pose_ref_step(const mh_artic_model* m, int B, double dt, int nsteps, double* q, double* qd, mh_world_aux* aux, double* pose,
                         const mh_artic_drive* drive)
{
  const int nj = m->nj;
  const bool driven = drive && drive->terms != 0;
  for (int b = 0; b < B; b++) {
    double* qb = q + (size_t)b * nj; double* qdb = qd + (size_t)b * nj; double* P = pose + 7 * (size_t)b;
    for (int s = 0; s < nsteps; s++) {
      mh_artic_model mb; world_model(m, P, &mb);
      mh_artic_drive row; std::memset(&row, 0, sizeof(row));
      if (driven) {                                              // step s's row of world b, as a one-world, one-row drive
        const size_t o = (size_t)b * nj, r = (size_t)(drive->rows == 1 ? 0 : s) * (size_t)B * nj + o;
        row.terms = drive->terms; row.rows = 1;
        if (drive->kp) row.kp = drive->kp + o;
        if (drive->kv) row.kv = drive->kv + o;
        if (drive->q_des) row.q_des = drive->q_des + r;
        if (drive->qd_des) row.qd_des = drive->qd_des + r;
        if (drive->tau_ff) row.tau_ff = drive->tau_ff + r;
      }
      const unsigned long long done = aux[b].steps;
      artic_drive_ref_step(&mb, 1, dt, 1, qb, qdb, aux + b, driven ? &row : nullptr);
      if (aux[b].steps != done) fold(qb, qdb, P);
    }
  }
}

}  // extern "C"
