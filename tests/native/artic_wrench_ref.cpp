// TEST INFRASTRUCTURE: the articulated step with link wrenches and link damping the GPU kernels of mh_artic_wr.hip are held to
// (include/moby_hip_artic.h, "Link wrenches").
//
// tests/native/artic_report_ref.cpp is included as it stands; only its do_mini_step_r / step_r are restated below, with the wrench folded into tau
// after kinematics() -- where the link frames of the mini-step's q exist -- by the rules of the header.  kinematics, link_velocities, fwd_dyn /
// fwd_dyn_aba and everything else are the oracle's, called as they are: the wrench reaches them as a richer tau (the Jacobian-transpose form).
// Host arrays take the place of the device arrays of mh_artic_wrench.  Pins (tests/test_artic_wrench.py): with terms = 0 and with a NULL wrench it
// equals artic_report_ref_step bit for bit.  Built by the tests as artic_report_ref.cpp is, as a library of its own.
#include "artic_report_ref.cpp"

namespace {

// tau_x of world b, schedule row s, from the link frames and q / qd of w (kinematics() has run); false: no term
bool wrench_tau(const ArticR& w, const mh_artic_wrench* W, int B, int b, int s, double* tau_x)
{
  using namespace artic;
  if (!W || W->terms == 0) return false;
  const mh_artic_model* m = w.m; const int nj = w.nj;
  double V[Artic::NJ][6], F6[Artic::NJ][6];
  w.link_velocities(V);
  const size_t r = (size_t)(W->rows == 1 ? 0 : s);
  for (int i = 0; i < nj; i++) {
    const double* R = w.R[i];
    double rc[3], c[3], F[3], T[3];
    mat3vec(R, m->com[i], rc);
    for (int k = 0; k < 3; k++) c[k] = w.x[i][k] + rc[k];
    const bool damp = (W->terms & MH_LINK_DAMPING) != 0;
    if (damp) {                                                    // add_damping on link i
      const size_t o = (size_t)b * nj + i;
      const double* om = V[i]; const double* v = V[i] + 3;
      double wxc[3], vc[3], vi[3], wi[3], fb[3], tb[3];
      cross3(om, c, wxc);
      for (int k = 0; k < 3; k++) vc[k] = v[k] + wxc[k];
      for (int k = 0; k < 3; k++) { vi[k] = (R[k] * vc[0] + R[3 + k] * vc[1]) + R[6 + k] * vc[2]; wi[k] = (R[k] * om[0] + R[3 + k] * om[1]) + R[6 + k] * om[2]; }
      const double nv = std::sqrt((vi[0] * vi[0] + vi[1] * vi[1]) + vi[2] * vi[2]), nw = std::sqrt((wi[0] * wi[0] + wi[1] * wi[1]) + wi[2] * wi[2]);
      const double cl = -(W->kl[o] + nv * W->klsq[o]), ca = -(W->ka[o] + nw * W->kasq[o]);
      for (int k = 0; k < 3; k++) { fb[k] = vi[k] * cl; tb[k] = wi[k] * ca; }
      mat3vec(R, fb, F); mat3vec(R, tb, T);
    }
    if (W->terms & MH_LINK_WRENCH) {
      const double* e = W->w + ((r * B + b) * nj + i) * 6;
      double f[3] = { e[0], e[1], e[2] }, n[3] = { e[3], e[4], e[5] };
      if (W->terms & MH_LINK_WRENCH_LINK_AXES) { double t[3]; mat3vec(R, f, t); for (int k = 0; k < 3; k++) f[k] = t[k]; mat3vec(R, n, t); for (int k = 0; k < 3; k++) n[k] = t[k]; }
      for (int k = 0; k < 3; k++) { F[k] = damp ? F[k] + f[k] : f[k]; T[k] = damp ? T[k] + n[k] : n[k]; }
    }
    double cxF[3]; cross3(c, F, cxF);
    for (int k = 0; k < 3; k++) { F6[i][k] = T[k] + cxF[k]; F6[i][3 + k] = F[k]; }
  }
  for (int j = 0; j < nj; j++) {
    double acc = 0.0;
    for (int i = 0; i < nj; i++) {
      bool on = false;
      for (int a = i; a >= 0; a = m->parent[a]) if (a == j) on = true;
      if (on) acc = acc + dot6(w.S[j], F6[i]);
    }
    tau_x[j] = acc;
  }
  return true;
}

// do_mini_step_r of artic_report_ref.cpp with the wrench between the drive and the forward dynamics
double do_mini_step_w(ArticR& w, double dt, const mh_artic_drive* D, const mh_artic_wrench* W, int B, int b, int s, double* rep)
{
  const mh_artic_model* m = w.m; const int nj = w.nj;
  double qsave[Artic::NJ], V[Artic::NJ][6];
  for (int i = 0; i < nj; i++) qsave[i] = w.q[i];
  double h = 0.0;
  unsigned long guard = 0;
  while (h < dt) {
    if (++guard > MH_CA_HARD_CAP) { w.aux->status |= MH_WORLD_STALLED; break; }
    w.kinematics(); w.link_velocities(V);
    double CA = INF_;
    for (int k = 0; k < m->nspheres; k++) { if (w.masked(k)) continue; const double e = w.CA_sphere(k, V); CA = (e < CA) ? e : CA; }
    for (int k = 0; k < m->nboxes; k++) { if (m->box_link[k] < 0) continue; const double e = CA_box(w, k, V); CA = (e < CA) ? e : CA; }
    for (int k = 0; k < m->npairs; k++) { const double e = w.is_bsp(k) ? w.CA_bsp(k, V) : w.CA_pair(k, V); CA = (e < CA) ? e : CA; }
    if (CA <= 0.0) break;
    double tc = (m->min_step_size > CA) ? m->min_step_size : CA;
    tc = ((dt - h) < tc) ? (dt - h) : tc;
    for (int i = 0; i < nj; i++) { double qn = w.qd[i] * (h + tc); qn = qn + qsave[i]; w.q[i] = qn; }
    h += tc;
  }
  double qdd[Artic::NJ], tau[Artic::NJ], tau_x[Artic::NJ];
  bool driven = drive_tau(D, B, b, s, nj, w.q, w.qd, tau);
  w.kinematics();                                                  // the link frames of this mini-step's q (the forward dynamics forms the same ones again)
  if (wrench_tau(w, W, B, b, s, tau_x)) {
    for (int j = 0; j < nj; j++) tau[j] = driven ? tau[j] + tau_x[j] : tau_x[j];
    driven = true;
  }
  const bool ok = (m->algorithm == MH_ARTIC_FSAB) ? w.fwd_dyn_aba(driven ? tau : nullptr, qdd) : w.fwd_dyn(driven ? tau : nullptr, qdd);
  if (!ok) { w.aux->status |= MH_WORLD_LCP_FAILED; return h; }       // thrown before the contacts exist: nothing to fold
  for (int i = 0; i < nj; i++) w.qd[i] = w.qd[i] + qdd[i] * h;
  std::vector<PC> cs; std::vector<int> slot;           // spheres, then every box's vertices within the threshold, then the pairs
  for (int k = 0; k < m->nspheres; k++) {
    if (w.masked(k)) continue;
    double ctr[3], cp[3]; w.sphere_center(k, ctr); w.to_plane(ctr, cp);
    const double dist = cp[1] + (-1.0 * m->sphere_radius[k]);
    Artic::AContact c;
    if (dist < m->contact_dist_thresh && w.find_contact(k, m->contact_dist_thresh, c)) { cs.push_back(c); slot.push_back(k); }
  }
  for (int k = 0; k < m->nboxes; k++) {
    double pa[3], pp[3];
    if (m->box_link[k] < 0) continue;                  // a static box never meets the plane
    if (!(box_dist(w, k, pa, pp) < m->contact_dist_thresh)) continue;
    for (int i = 0; i < 8; i++) { double v[3], q[3]; box_vertex(w, k, i, v); w.to_plane(v, q); if (q[1] <= m->contact_dist_thresh) { cs.push_back(vertex_contact(w, k, v, q[1])); slot.push_back(m->nspheres + k); } }
  }
  for (int k = 0; k < m->npairs; k++) {
    PC c;
    if (w.is_bsp(k)) { if (w.any_dist(k) < m->contact_dist_thresh && w.bsp_contact(k, m->contact_dist_thresh, c)) { cs.push_back(c); slot.push_back(m->nspheres + m->nboxes + k); } }
    else if (w.pair_contact(k, m->contact_dist_thresh, c) && c.dist < m->contact_dist_thresh) { cs.push_back(c); slot.push_back(m->nspheres + m->nboxes + k); }
  }
  std::vector<double> acc(3 * cs.size() + 1, 0.0);     // a new constraint list: no contact has received an impulse yet
  w.handle_impacts_r(cs, acc);
  if (w.aux->status & MH_WORLD_LCP_FAILED) return h;   // the handler threw: the callback of CSim:353 is not reached
  if (rep) for (size_t c = 0; c < cs.size(); c++) {    // the fold, in constraint-list order
    const bool has = c < (size_t)MH_NOSLIP_MAX;        // the handler holds no more contacts than that: one beyond them has no impulse
    const double cn = has ? acc[3*c] : 0.0, csi = has ? acc[3*c + 1] : 0.0, cti = has ? acc[3*c + 2] : 0.0;
    double* row = rep + (size_t)RP * slot[c];
    row[0] = row[0] + 1.0;
    row[1] = row[1] + cn;
    for (int k = 0; k < 3; k++) { const double jv = (cs[c].n[k] * cn + cs[c].sv[k] * csi) + cs[c].tv[k] * cti; row[2 + k] = row[2 + k] + jv; }
    for (int k = 0; k < 3; k++) row[5 + k] = row[5 + k] + cs[c].p[k] * cn;
  }
  w.aux->time += h; w.aux->mini_steps++; w.folds++;
  return h;
}

void step_w(ArticR& w, double dt, const mh_artic_drive* D, const mh_artic_wrench* W, int B, int b, int s, double* rep)
{
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  const int FROZEN = MH_WORLD_UNSUPPORTED | MH_WORLD_STALLED;
  if (w.aux->status & FROZEN) return;
  double h = 0.0; unsigned guard = 0;
  while (h < dt) {
    h += do_mini_step_w(w, dt - h, D, W, B, b, s, rep);
    if (w.aux->status & MH_WORLD_LCP_FAILED) return;
    if (w.aux->status & FROZEN) break;
    if (++guard > 100000u) { w.aux->status |= MH_WORLD_STALLED; break; }
  }
  stabilize(w);                                        // (never reads the wrench: it moves positions)
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  w.aux->steps++;
}

}  // namespace

extern "C" {

// artic_report_ref_step with a wrench: HOST arrays where mh_artic_wrench names device arrays; NULL or terms 0: no force
void artic_wrench_ref_step(const mh_artic_model* m, int B, double dt, int nsteps, double* q, double* qd, mh_world_aux* aux, double* pose,
                           const mh_artic_drive* drive, const mh_artic_wrench* wrench, double* report, double* diag)
{
  const int nj = m->nj, nslots = m->nspheres + m->nboxes + m->npairs;
  if (report) for (size_t e = 0; e < (size_t)B * nsteps * nslots * RP; e++) report[e] = 0.0;
  for (int b = 0; b < B; b++) {
    double* qb = q + (size_t)b * nj; double* qdb = qd + (size_t)b * nj;
    for (int s = 0; s < nsteps; s++) {
      mh_artic_model mb;
      if (pose) artic_pose_ref_model(m, pose + 7 * (size_t)b, &mb); else std::memcpy(&mb, m, sizeof(mb));
      ArticR w(&mb, qb, qdb, aux + b);
      const unsigned long long done = aux[b].steps;
      step_w(w, dt, drive, wrench, B, b, s, report ? report + ((size_t)b * nsteps + s) * nslots * RP : nullptr);
      if (pose && aux[b].steps != done) artic_pose_ref_fold(1, nj, qb, qdb, pose + 7 * (size_t)b);
      if (diag) { diag[((size_t)b * nsteps + s) * 2] = (double)w.folds; diag[((size_t)b * nsteps + s) * 2 + 1] = w.first_cn; }
    }
  }
}

}  // extern "C"
