// TEST INFRASTRUCTURE: the driven articulated step the GPU kernels are held to (include/moby_hip_artic.h, mh_artic_drive).
//
// oracle::Artic::step / do_mini_step (oracle/artic.hpp) call the forward dynamics with tau = NULL, and oracle/ is not edited for a feature; so this
// file restates THOSE TWO FUNCTIONS ONLY, with the drive evaluated where the reference calls its controller -- once per mini-step, after the
// position update and before calc_fwd_dyn (precalc_fwd_dyn: TimeSteppingSimulator.cpp:173 -> Simulator.cpp:319-350, ArticulatedBody.cpp:95-115).
// Everything else is the oracle's own: kinematics, fwd_dyn / fwd_dyn_aba (with tau), CA_step, find_contact, handle_impacts, handle_limits, stabilize.
// Two pins keep the restatement honest (tests/test_artic_drive.py): with terms = 0 it equals oracle_artic_step bit for bit, and one driven step of
// a chain without limits or spheres equals the composition of the oracle's own forward dynamics.
// Built by the tests with g++ and oracle/Makefile's CXXFLAGS (-ffp-contract=off: no FMA in tau either).
#include <cstring>
#include <ctime>
#include "lcp.hpp"
#include "world.hpp"
#include "artic.hpp"

using namespace oracle;

namespace {

// tau_j = (kp_j (q_des_j - q_j) + kv_j (qd_des_j - qd_j)) + tau_ff_j, absent terms left out; false: undriven
bool drive_tau(const mh_artic_drive* D, int B, int b, int s, int nj, const double* q, const double* qd, double* tau)
{
  if (!D || D->terms == 0) return false;
  const size_t row = (size_t)(D->rows == 1 ? 0 : s) * (size_t)B * nj;
  for (int j = 0; j < nj; j++) {
    const size_t o = (size_t)b * nj + j, r = row + o;
    double t = 0.0;
    if (D->terms & MH_DRIVE_PD) {
      const double ep = D->q_des[r] - q[j], ev = D->qd_des[r] - qd[j];
      const double tp = D->kp[o] * ep, tv = D->kv[o] * ev;
      t = tp + tv;
      if (D->terms & MH_DRIVE_FORCE) t = t + D->tau_ff[r];
    } else t = D->tau_ff[r];
    tau[j] = t;
  }
  return true;
}

bool fwd(Artic& w, const double* tau, double* qdd)
{
  return (w.m->algorithm == MH_ARTIC_FSAB) ? w.fwd_dyn_aba(tau, qdd) : w.fwd_dyn(tau, qdd);
}

// Artic::do_mini_step with the drive
double do_mini_step(Artic& w, double dt, const mh_artic_drive* D, int B, int b, int s)
{
  const mh_artic_model* m = w.m; const int nj = w.nj;
  double qsave[Artic::NJ], V[Artic::NJ][6];
  for (int i = 0; i < nj; i++) qsave[i] = w.q[i];
  double h = 0.0;
  unsigned long guard = 0;
  while (h < dt) {
    if (++guard > MH_CA_HARD_CAP) { w.aux->status |= MH_WORLD_STALLED; break; }
    w.kinematics(); w.link_velocities(V);
    double CA = Artic::A_INF;
    for (int k = 0; k < m->nspheres; k++) { const double e = w.CA_step(k, V); CA = (e < CA) ? e : CA; }
    if (CA <= 0.0) break;
    double tc = (m->min_step_size > CA) ? m->min_step_size : CA;
    tc = ((dt - h) < tc) ? (dt - h) : tc;
    for (int i = 0; i < nj; i++) { double qn = w.qd[i] * (h + tc); qn = qn + qsave[i]; w.q[i] = qn; }
    h += tc;
  }
  double qdd[Artic::NJ], tau[Artic::NJ];
  const bool driven = drive_tau(D, B, b, s, nj, w.q, w.qd, tau);
  if (!fwd(w, driven ? tau : nullptr, qdd)) { w.aux->status |= MH_WORLD_LCP_FAILED; return h; }
  for (int i = 0; i < nj; i++) w.qd[i] = w.qd[i] + qdd[i] * h;
  std::vector<Artic::AContact> cs;
  for (int k = 0; k < m->nspheres; k++) {
    double ctr[3], cp[3]; w.sphere_center(k, ctr); w.to_plane(ctr, cp);
    const double dist = cp[1] + (-1.0 * m->sphere_radius[k]);
    Artic::AContact c;
    if (dist < m->contact_dist_thresh && w.find_contact(k, m->contact_dist_thresh, c)) cs.push_back(c);
  }
  w.handle_impacts(cs);
  if (w.aux->status & MH_WORLD_LCP_FAILED) return h;
  w.aux->time += h; w.aux->mini_steps++;
  return h;
}

// Artic::step with the drive (step s of the launch)
void step(Artic& w, double dt, const mh_artic_drive* D, int B, int b, int s)
{
  const mh_artic_model* m = w.m; const int nj = w.nj;
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  if (m->nspheres > 0) {
    const int FROZEN = MH_WORLD_UNSUPPORTED | MH_WORLD_STALLED;
    if (w.aux->status & FROZEN) return;
    double h = 0.0; unsigned guard = 0;
    while (h < dt) {
      h += do_mini_step(w, dt - h, D, B, b, s);
      if (w.aux->status & MH_WORLD_LCP_FAILED) return;
      if (w.aux->status & FROZEN) break;
      if (++guard > 100000u) { w.aux->status |= MH_WORLD_STALLED; break; }
    }
    w.stabilize();
    if (w.aux->status & MH_WORLD_LCP_FAILED) return;
    w.aux->steps++;
    return;
  }
  for (int i = 0; i < nj; i++) { double qn = w.qd[i] * dt; qn = qn + w.q[i]; w.q[i] = qn; }
  double qdd[Artic::NJ], tau[Artic::NJ];
  const bool driven = drive_tau(D, B, b, s, nj, w.q, w.qd, tau);
  if (!fwd(w, driven ? tau : nullptr, qdd)) { w.aux->status |= MH_WORLD_LCP_FAILED; return; }
  for (int i = 0; i < nj; i++) w.qd[i] = w.qd[i] + qdd[i] * dt;
  w.handle_limits();
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  w.aux->time += dt; w.aux->mini_steps++;
  w.stabilize();
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  w.aux->steps++;
}

}  // namespace

extern "C" {

// B worlds x nsteps driven steps, in place (drive: HOST arrays laid out as mh_artic_drive states; NULL or terms == 0 = undriven)
void artic_drive_ref_step(const mh_artic_model* m, int B, double dt, int nsteps, double* q, double* qd, mh_world_aux* aux, const mh_artic_drive* drive)
{
  for (int b = 0; b < B; b++) {
    Artic w(m, q + (size_t)b * m->nj, qd + (size_t)b * m->nj, aux + b);
    for (int s = 0; s < nsteps; s++) step(w, dt, drive, B, b, s);
  }
}

}  // extern "C"
