// TEST INFRASTRUCTURE: the forced world step the GPU kernels are held to (include/moby_hip.h, mh_world_forces / mh_world_batch_step_wrench).
//
// oracle::World::fwd_dyn (oracle/world.hpp) knows gravity alone, and oracle/ is not edited for a feature; World is all-public, so this file restates
// World::fwd_dyn, the joint-free branch of fwd_dyn_and_integrate, do_mini_step and step ONLY, with the forces evaluated where the reference runs its
// recurrent forces and controllers -- once per mini-step, after the position update and before calc_fwd_dyn (precalc_fwd_dyn:
// TimeSteppingSimulator.cpp:173 -> Simulator.cpp:319-350; StokesDragForce.cpp:39-44, DampingForce.cpp:32-51).  Everything else is the oracle's own:
// broad_phase, calc_pairwise_distances, next_CA_step, find_contacts, handle_impacts, stabilize.
// Pins (tests/test_world_forces.py): with no terms it equals oracle_world_step_batch bit for bit; a lone body under Stokes drag and a wrench follows the
// recurrence written out in numpy, operation by operation.
// Built by the tests with g++ and oracle/Makefile's CXXFLAGS (-ffp-contract=off: every operation rounds on its own).
#include <cstring>
#include <ctime>
#include "lcp.hpp"
#include "world.hpp"

using namespace oracle;

namespace {

struct Forcing {
  const mh_world_forces* F;    // stored terms, or NULL
  const double* wrench;        // rows x B x nb x 6, or NULL
  int rows, B, world, step;
};

// World::fwd_dyn with the terms in their canonical order: gravity, Stokes drag, damping, the caller's wrench; an absent term is left out
void fwd_dyn(const World& w, const Forcing& fo, int b, V3& xdd, V3& wd)
{
  const SceneView* sc = w.sc;
  const double m = sc->mass[b];
  V3 F = v3(sc->gravity[0] * m, sc->gravity[1] * m, sc->gravity[2] * m);
  V3 T = v3(0.0, 0.0, 0.0);
  bool has_t = false;
  const V3 v = w.Vl(b), om = w.Wa(b);
  const int terms = fo.F ? fo.F->terms : 0;
  if (terms & MH_FORCE_STOKES) {
    F = F + v * (-fo.F->stokes_b[b]);
    T = om * (-fo.F->stokes_b_ang[b]); has_t = true;
  }
  if (terms & MH_FORCE_DAMPING) {
    double R[9]; w.rot(b, R);
    const V3 vi = v3((R[0]*v.x + R[3]*v.y) + R[6]*v.z, (R[1]*v.x + R[4]*v.y) + R[7]*v.z, (R[2]*v.x + R[5]*v.y) + R[8]*v.z);
    const V3 wi = v3((R[0]*om.x + R[3]*om.y) + R[6]*om.z, (R[1]*om.x + R[4]*om.y) + R[7]*om.z, (R[2]*om.x + R[5]*om.y) + R[8]*om.z);
    const V3 fb = vi * (-(fo.F->damp_kl[b] + norm(vi) * fo.F->damp_klsq[b]));
    const V3 tb = wi * (-(fo.F->damp_ka[b] + norm(wi) * fo.F->damp_kasq[b]));
    const V3 fw = v3((R[0]*fb.x + R[1]*fb.y) + R[2]*fb.z, (R[3]*fb.x + R[4]*fb.y) + R[5]*fb.z, (R[6]*fb.x + R[7]*fb.y) + R[8]*fb.z);
    const V3 tw = v3((R[0]*tb.x + R[1]*tb.y) + R[2]*tb.z, (R[3]*tb.x + R[4]*tb.y) + R[5]*tb.z, (R[6]*tb.x + R[7]*tb.y) + R[8]*tb.z);
    F = F + fw;
    T = has_t ? T + tw : tw; has_t = true;
  }
  if (fo.wrench) {
    const double* r = fo.wrench + (((size_t)(fo.rows == 1 ? 0 : fo.step) * fo.B + fo.world) * sc->nb + b) * 6;
    F = F + v3(r[0], r[1], r[2]);
    const V3 tq = v3(r[3], r[4], r[5]);
    T = has_t ? T + tq : tq; has_t = true;
  }
  xdd = F / m;
  double Jw[9]; w.inertia_world(b, Jw);
  const V3 Jww = v3((Jw[0]*om.x + Jw[1]*om.y) + Jw[2]*om.z, (Jw[3]*om.x + Jw[4]*om.y) + Jw[5]*om.z, (Jw[6]*om.x + Jw[7]*om.y) + Jw[8]*om.z);
  const V3 tau = has_t ? T - cross(om, Jww) : -cross(om, Jww);
  double im, Ji[9]; w.inv_inertia(b, im, Ji);
  wd = v3((Ji[0]*tau.x + Ji[1]*tau.y) + Ji[2]*tau.z, (Ji[3]*tau.x + Ji[4]*tau.y) + Ji[5]*tau.z, (Ji[6]*tau.x + Ji[7]*tau.y) + Ji[8]*tau.z);
}

// World::do_mini_step with the forces (the scenes of the many-worlds stepper have no joints: the joint-free branch of fwd_dyn_and_integrate)
double do_mini_step(World& w, const Forcing& fo, double dt)
{
  const SceneView* sc = w.sc;
  const int nb = sc->nb;
  std::vector<double> qsave_v(7 * (size_t)nb);
  double (*qsave)[7] = reinterpret_cast<double (*)[7]>(qsave_v.data());
  for (int b = 0; b < nb; b++) w.get_coords(b, qsave[b]);
  double h = 0.0;
  unsigned long ca_guard = 0;
  while (h < dt) {
    g_ca_iters++;
    if (++ca_guard > MH_CA_HARD_CAP) { w.aux->status |= MH_WORLD_STALLED; break; }
    w.broad_phase(dt - h, w.pairs_to_check);
    w.calc_pairwise_distances(w.pairs_to_check, w.pairwise);
    const double CA = w.next_CA_step();
    if (CA <= 0.0) break;
    double tc = (sc->min_step_size > CA) ? sc->min_step_size : CA;
    tc = ((dt - h) < tc) ? (dt - h) : tc;
    for (int b = 0; b < nb; b++) {
      w.set_coords(b, qsave[b]);
      double qd[7]; w.euler_vel(b, qd);
      double q[7];
      for (int i = 0; i < 7; i++) { q[i] = qd[i] * (h + tc); q[i] = q[i] + qsave[b][i]; }
      w.set_coords(b, q);
    }
    h += tc;
  }
  for (int b = 0; b < nb; b++) { V3 xdd, wd; fwd_dyn(w, fo, b, xdd, wd); w.setV(b, w.Vl(b) + xdd * h); w.setW(b, w.Wa(b) + wd * h); }
  w.calc_pairwise_distances(w.pairs_to_check, w.pairwise);
  std::vector<Contact> cs;
  for (const PairDist& d : w.pairwise) if (d.dist < sc->contact_dist_thresh) w.find_contacts(d.pair, sc->contact_dist_thresh, cs);
  w.handle_impacts(cs);
  if (w.thrown_) return h;
  w.aux->time += h;
  w.aux->mini_steps++;
  return h;
}

// World::step with the forces (step `fo.step` of the launch)
void step(World& w, const Forcing& fo, double dt)
{
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  w.broad_phase(dt, w.pairs_to_check);
  w.calc_pairwise_distances(w.pairs_to_check, w.pairwise);
  double h = 0.0;
  unsigned guard = 0;
  while (h < dt) {
    h += do_mini_step(w, fo, dt - h);
    if (w.thrown_) return;
    if (++guard > 100000u) { w.aux->status |= MH_WORLD_STALLED; break; }
  }
  w.stabilize();
  w.aux->steps++;
}

}  // namespace

extern "C" {

// B worlds x nsteps forced steps, in place.  forces: NULL or terms == 0 = none; wrench: HOST array rows x B x nb x 6 or NULL; traj: B x nsteps x nb x 7 or NULL
void world_force_ref_step(const mh_scene* sc, int B, double dt, int nsteps, double* state, mh_world_aux* aux,
                          const mh_world_forces* forces, const double* wrench, int rows, double* traj)
{
  for (int b = 0; b < B; b++) {
    double* st = state + (size_t)b * sc->nb * MH_BODY_STATE;
    World w(sc, st, aux + b);
    for (int s = 0; s < nsteps; s++) {
      const Forcing fo = { forces, wrench, rows, B, b, s };
      step(w, fo, dt);
      if (traj) for (int k = 0; k < sc->nb; k++) for (int i = 0; i < 7; i++) traj[(((size_t)b * nsteps + s) * sc->nb + k) * 7 + i] = st[13*k + i];
    }
  }
}

}  // extern "C"
