// TEST INFRASTRUCTURE: the world step with the per-pair contact impulse report (include/moby_hip.h, "Contact report"), which the GPU kernels
// mh_world_large_rp*.hip are held to.
//
// The report adds no physics: it is what ConstraintSimulator::constraint_post_callback_fn (ConstraintSimulator.cpp:353) would see -- the mini-step's contact
// constraints with the contact_impulse that update_from_stacked accumulated (ImpactConstraintHandler.cpp:298-327) -- summed per pair.  The oracle already
// carries that quantity: Contact::imp (oracle/world.hpp:65), zeroed when the contact is made, added to by World::apply_impulses.  So this file includes
// tests/native/world_statics_ref.cpp for its geometry and restates ONLY
//   * the mini-step, whose tail (contact list -> handle_impacts -> fold) needs the contact list that world_statics_ref's do_mini_step keeps to itself; its
//     head (conservative advancement, forward dynamics) is repeated statement for statement;
//   * the step loop and the entry point, which hand the step's rows down.
// Pin (tests/test_world_report.py): state, trajectory and the complete aux record equal world_statics_ref_step's bit for bit.
// Built by the tests with g++ and oracle/Makefile's CXXFLAGS (-ffp-contract=off: every operation rounds on its own).
#include "world_statics_ref.cpp"

namespace {

// what a step's contacts were like, for the conditions the tests assert on their inputs (per world and step, 6 ints):
//   [0] mini-steps folded with at least one contact; [1] most contacts of one pair in one mini-step; [2] most pairs with cn > 0 in one mini-step;
//   [3] contacts with epsilon > 0 whose restitution pass added a second impulse; [4] contacts counted with zero impulse; [5] contacts with sign = -1
enum { SH_MINI = 0, SH_PAIR_CONTACTS, SH_PAIRS_LOADED, SH_RESTITUTION, SH_ZERO, SH_NEG_SIGN, SH_COUNT };

// rows: npt x MH_REPORT_PAIR of this step; the contacts in constraint-list order
void fold(const World& w, const std::vector<Contact>& cs, double* rows, int* shape)
{
  const int npt = w.sc->npairs;
  std::vector<int> per_pair(npt, 0); std::vector<double> cn_pair(npt, 0.0);
  for (const Contact& c : cs) {
    int i, j; w.pair_bodies(c.pair, i, j);                           // i < j
    const double cn = c.imp[0], cs_ = c.imp[1], ct = c.imp[2];
    const double sign = (c.g1 == i) ? 1.0 : -1.0;
    const V3 jv = (c.n * cn + c.s * cs_) + c.t * ct;
    double* r = rows + (size_t)MH_REPORT_PAIR * c.pair;
    r[0] += 1.0;
    r[1] += cn;
    r[2] += sign * jv.x; r[3] += sign * jv.y; r[4] += sign * jv.z;
    r[5] += c.p.x * cn; r[6] += c.p.y * cn; r[7] += c.p.z * cn;
    if (!shape) continue;
    per_pair[c.pair]++; cn_pair[c.pair] += cn;
    // the restitution pass (ICH:470-491, 581) adds eps * cn to every contact of an island once one of them has eps * cn > NEAR_ZERO.  Without it
    // imp[0] = cn and eps * cn <= NEAR_ZERO, so imp[0] eps / (1 + eps) > NEAR_ZERO can only be seen after a second impulse
    if (c.eps > 0.0 && cn * c.eps / (1.0 + c.eps) > NEAR_ZERO) shape[SH_RESTITUTION]++;
    if (cn == 0.0 && cs_ == 0.0 && ct == 0.0) shape[SH_ZERO]++;
    if (sign < 0.0) shape[SH_NEG_SIGN]++;
  }
  if (!shape) return;
  if (!cs.empty()) shape[SH_MINI]++;
  int loaded = 0;
  for (int p = 0; p < npt; p++) { if (per_pair[p] > shape[SH_PAIR_CONTACTS]) shape[SH_PAIR_CONTACTS] = per_pair[p]; if (cn_pair[p] > 0.0) loaded++; }
  if (loaded > shape[SH_PAIRS_LOADED]) shape[SH_PAIRS_LOADED] = loaded;
}

// do_mini_step of world_statics_ref.cpp with the fold behind handle_impacts
double do_mini_step_report(World& w, double dt, const Forcing* fo, double* rows, int* shape)
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
    broad_phase(w, dt - h, w.pairs_to_check);
    calc_pairwise_distances(w, w.pairs_to_check, w.pairwise);
    const double CA = next_CA_step(w);
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
  if (fo) for (int b = 0; b < nb; b++) { V3 xdd, wd; fwd_dyn(w, *fo, b, xdd, wd); w.setV(b, w.Vl(b) + xdd * h); w.setW(b, w.Wa(b) + wd * h); }
  else w.fwd_dyn_and_integrate(h);
  calc_pairwise_distances(w, w.pairs_to_check, w.pairwise);
  std::vector<Contact> cs;
  for (const PairDist& d : w.pairwise) if (d.dist < sc->contact_dist_thresh) find_contacts(w, d.pair, sc->contact_dist_thresh, cs);
  w.handle_impacts(cs);
  if (w.thrown_) return h;                                           // (the exception leaves before CSim:353: nothing is folded)
  if (rows) fold(w, cs, rows, shape);                                // constraint_post_callback_fn (CSim:353)
  w.aux->time += h;
  w.aux->mini_steps++;
  return h;
}

void step_report(World& w, double dt, const Forcing* fo, double* rows, int* shape)
{
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;                   // passed over: the rows stay zero
  broad_phase(w, dt, w.pairs_to_check);
  calc_pairwise_distances(w, w.pairs_to_check, w.pairwise);
  double h = 0.0;
  unsigned guard = 0;
  while (h < dt) {
    h += do_mini_step_report(w, dt - h, fo, rows, shape);
    if (w.thrown_) return;
    if (++guard > 100000u) { w.aux->status |= MH_WORLD_STALLED; break; }
  }
  stabilize(w);
  w.aux->steps++;
}

}  // namespace

extern "C" {

// world_statics_ref_step with the report: report B x nsteps x npt x MH_REPORT_PAIR (written whole: zero rows first) or NULL; shape B x nsteps x 6 ints
// (zeroed here) or NULL
void world_report_ref_step(const mh_scene* sc, const mh_world_statics* statics, int B, double dt, int nsteps, double* state, mh_world_aux* aux, double* traj,
                           const mh_world_forces* forces, const double* wrench, int rows, double* report, int* shape)
{
  g_st = statics ? statics : &g_none; g_hg = sc->has_ground ? 1 : 0;
  const View view(sc, g_st);
  const int npt = view.v.npairs;
  const bool forced = (forces && forces->terms) || wrench;
  if (report) for (size_t i = 0; i < (size_t)B * nsteps * npt * MH_REPORT_PAIR; i++) report[i] = 0.0;
  if (shape) for (size_t i = 0; i < (size_t)B * nsteps * SH_COUNT; i++) shape[i] = 0;
  for (int b = 0; b < B; b++) {
    double* st = state + (size_t)b * sc->nb * MH_BODY_STATE;
    World w(view.v, st, aux + b, aux[b].zlast, aux[b].zbuf, MH_LCP_MAX_N_WAVE);
    for (int s = 0; s < nsteps; s++) {
      const Forcing fo = { forces, wrench, rows, B, b, s };
      step_report(w, dt, forced ? &fo : nullptr, report ? report + ((size_t)b * nsteps + s) * npt * MH_REPORT_PAIR : nullptr,
                  shape ? shape + ((size_t)b * nsteps + s) * SH_COUNT : nullptr);
      if (traj) for (int k = 0; k < sc->nb; k++) for (int i = 0; i < 7; i++) traj[(((size_t)b * nsteps + s) * sc->nb + k) * 7 + i] = st[13*k + i];
    }
  }
}

}  // extern "C"
