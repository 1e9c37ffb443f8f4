// TEST INFRASTRUCTURE: the articulated step with box primitives on links the GPU box kernels are held to (include/moby_hip_artic.h, mh_artic_model.nboxes).
//
// oracle/ is not edited for a feature, so this file restates only what boxes change, in the device's operation order (mh_artic_contacts.inc under
// MH_ARTIC_BOX_TU): the box geometry (vertices, signed distance, rmax), the box's conservative advancement (calc_CA_Euler_step_generic with the
// rest rule and the polyhedron-plane step), the contact list of do_mini_step (spheres, then every box's vertices), and the stabiliser (Artic::stabilize
// with the boxes' rows, its eval and its line search).  Kinematics, the dynamics and handle_impacts(std::vector<AContact>) are the oracle's own.  The
// drive is artic_drive_ref.cpp's, evaluated the same way (restated: its helper is file-local there); pose coordinates use artic_pose_ref.cpp's model
// copy and fold.  Pins (tests/test_artic_box.py): with nboxes = 0 it equals oracle_artic_step, artic_drive_ref_step and artic_pose_ref_step bit for bit.
// Built by the tests with g++ and oracle/Makefile's CXXFLAGS (-ffp-contract=off), linked with artic_drive_ref.cpp and artic_pose_ref.cpp.
#include <cmath>
#include <cstring>
#include <vector>
#include "lcp.hpp"
#include "world.hpp"
#include "artic.hpp"

using namespace oracle;

extern "C" void artic_pose_ref_fold(int B, int nj, double* q, double* qd, double* pose);
extern "C" void artic_pose_ref_model(const mh_artic_model* m, const double* pose, mh_artic_model* out);

namespace {

const double NZ = A_NEAR_ZERO;
constexpr double INF_ = Artic::A_INF;

// vertex i of box k, model frame (get_vertices order)
void box_vertex(const Artic& w, int k, int i, double v[3])
{
  const mh_artic_model* m = w.m; const int l = m->box_link[k];
  const double hx = m->box_len[k][0] * 0.5, hy = m->box_len[k][1] * 0.5, hz = m->box_len[k][2] * 0.5;
  const double px = (i & 4) ? -hx : hx, py = (i & 2) ? -hy : hy, pz = (i & 1) ? -hz : hz;
  const double* Rb = m->box_R[k];
  const double lp[3] = { m->box_center[k][0] + ((Rb[0]*px + Rb[1]*py) + Rb[2]*pz), m->box_center[k][1] + ((Rb[3]*px + Rb[4]*py) + Rb[5]*pz),
                         m->box_center[k][2] + ((Rb[6]*px + Rb[7]*py) + Rb[8]*pz) };
  double rc[3]; artic::mat3vec(w.R[l], lp, rc);
  for (int c = 0; c < 3; c++) v[c] = w.x[l][c] + rc[c];
}
// signed distance: the lowest vertex's plane-frame height, first wins ties; pa the vertex, pp it in the plane frame
double box_dist(const Artic& w, int k, double pa[3], double pp[3])
{
  double mn = INF_;
  for (int i = 0; i < 8; i++) {
    double v[3], q[3]; box_vertex(w, k, i, v); w.to_plane(v, q);
    if (q[1] < mn) { mn = q[1]; for (int c = 0; c < 3; c++) { pa[c] = v[c]; pp[c] = q[c]; } }
  }
  return mn;
}
double rmax_box(const Artic& w, int k)
{
  const mh_artic_model* m = w.m; const int l = m->box_link[k];
  const double d[3] = { m->box_center[k][0] - m->com[l][0], m->box_center[k][1] - m->com[l][1], m->box_center[k][2] - m->com[l][2] };
  const double x = m->box_len[k][0], y = m->box_len[k][1], z = m->box_len[k][2];
  return std::sqrt((x*x + y*y) + z*z) + std::sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
}
bool rel_equal(double x, double y) { return std::fabs(x - y) <= NZ * std::max(std::fabs(x), std::max(std::fabs(y), 1.0)); }
bool collinear(const double* a, const double* b, const double* c)
{
  return rel_equal((c[2]-a[2])*(b[1]-a[1]), (b[2]-a[2])*(c[1]-a[1])) && rel_equal((b[2]-a[2])*(c[0]-a[0]), (b[0]-a[0])*(c[2]-a[2])) &&
         rel_equal((b[0]-a[0])*(c[1]-a[1]), (b[1]-a[1])*(c[0]-a[0]));
}
// calc_CA_Euler_step_generic for (box k, plane)
double CA_box(const Artic& w, int k, const double V[][6])
{
  const mh_artic_model* m = w.m; const int link = m->box_link[k];
  double pa[3], pp[3];
  const double dist = box_dist(w, k, pa, pp);
  double n[3]; w.plane_n(n);
  const double* V6 = V[link];
  if (dist <= 0.0) {                                              // calc_next_CA_Euler_step_generic
    std::vector<std::vector<double>> cs;
    for (int i = 0; i < 8; i++) { double v[3], q[3]; box_vertex(w, k, i, v); w.to_plane(v, q); if (q[1] <= NZ) cs.push_back({ v[0], v[1], v[2] }); }
    if (cs.empty()) return INF_;
    for (const auto& c : cs) if (Artic::point_vel_dir(V6, c.data(), n) < -NZ) return 0.0;
    if (cs.size() >= 3 && !collinear(cs[0].data(), cs[1].data(), cs[2].data())) return INF_;
    const double offset0 = artic::dot3(n, cs[0].data());          // calc_next_CA_Euler_step_polyhedron_plane
    double Rbg[9]; artic::mat3mul(w.R[link], m->box_R[k], Rbg);
    double cb[3]; { double rc[3]; artic::mat3vec(w.R[link], m->box_center[k], rc); for (int c = 0; c < 3; c++) cb[c] = w.x[link][c] + rc[c]; }
    auto to_box = [&](const double* v, double* o) {
      o[0] = (Rbg[0]*v[0] + Rbg[3]*v[1]) + Rbg[6]*v[2]; o[1] = (Rbg[1]*v[0] + Rbg[4]*v[1]) + Rbg[7]*v[2]; o[2] = (Rbg[2]*v[0] + Rbg[5]*v[1]) + Rbg[8]*v[2];
    };
    double nP[3]; to_box(n, nP);
    const double d0[3] = { n[0] * offset0 - cb[0], n[1] * offset0 - cb[1], n[2] * offset0 - cb[2] };
    double t[3]; to_box(d0, t);
    const double offset = artic::dot3(nP, t);
    double wxc[3]; artic::cross3(V6, cb, wxc);
    const double vrel[3] = { V6[3] + wxc[0], V6[4] + wxc[1], V6[5] + wxc[2] };
    double wb[3], vb[3]; to_box(V6, wb); to_box(vrel, vb);
    const double av_norm = std::sqrt(artic::dot3(wb, wb));
    const double lv_dot_n = -artic::dot3(nP, vb);
    const double hx = m->box_len[k][0] * 0.5, hy = m->box_len[k][1] * 0.5, hz = m->box_len[k][2] * 0.5;
    double max_step = INF_;
    for (int i = 0; i < 8; i++) {
      const double vtx[3] = { (i & 4) ? -hx : hx, (i & 2) ? -hy : hy, (i & 1) ? -hz : hz };
      const double r = std::sqrt(artic::dot3(vtx, vtx));
      const double dv = artic::dot3(nP, vtx) - offset;
      if (dv < NZ) continue;
      const double sp = lv_dot_n + av_norm * r;
      const double speed = (0.0 > sp) ? 0.0 : sp;
      const double cand = dv / speed;
      max_step = (cand < max_step) ? cand : max_step;
    }
    return max_step;
  }
  double pb[3]; w.from_plane(pp[0], 0.0, pp[2], pb);
  const double d0[3] = { pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2] };
  const double len = std::sqrt(artic::dot3(d0, d0));
  const double mn0[3] = { -(d0[0] / len), -(d0[1] / len), -(d0[2] / len) };
  const double tA = w.calc_max_dist(link, mn0, rmax_box(w, k));
  double total = tA + 0.0;
  if (total < 0.0) total = 0.0;
  const double cand = dist / total;
  return (cand < INF_) ? cand : INF_;
}
Artic::AContact vertex_contact(const Artic& w, int k, const double v[3], double dist)
{
  Artic::AContact c; c.s = -1; c.link = w.m->box_link[k]; c.dist = dist;
  for (int j = 0; j < 3; j++) c.p[j] = v[j];
  w.plane_n(c.n); Artic::orthonormal_basis(c.n, c.sv, c.tv);
  return c;
}

// artic_drive_ref.cpp's drive_tau
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

// Artic::do_mini_step with the boxes (and the drive)
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
    double CA = INF_;
    for (int k = 0; k < m->nspheres; k++) { const double e = w.CA_step(k, V); CA = (e < CA) ? e : CA; }
    for (int k = 0; k < m->nboxes; k++) { const double e = CA_box(w, k, V); CA = (e < CA) ? e : CA; }
    if (CA <= 0.0) break;
    double tc = (m->min_step_size > CA) ? m->min_step_size : CA;
    tc = ((dt - h) < tc) ? (dt - h) : tc;
    for (int i = 0; i < nj; i++) { double qn = w.qd[i] * (h + tc); qn = qn + qsave[i]; w.q[i] = qn; }
    h += tc;
  }
  double qdd[Artic::NJ], tau[Artic::NJ];
  const bool driven = drive_tau(D, B, b, s, nj, w.q, w.qd, tau);
  const bool ok = (m->algorithm == MH_ARTIC_FSAB) ? w.fwd_dyn_aba(driven ? tau : nullptr, qdd) : w.fwd_dyn(driven ? tau : nullptr, qdd);
  if (!ok) { w.aux->status |= MH_WORLD_LCP_FAILED; return h; }
  for (int i = 0; i < nj; i++) w.qd[i] = w.qd[i] + qdd[i] * h;
  std::vector<Artic::AContact> cs;                                 // spheres, then every box's vertices within the threshold
  for (int k = 0; k < m->nspheres; k++) {
    double ctr[3], cp[3]; w.sphere_center(k, ctr); w.to_plane(ctr, cp);
    const double dist = cp[1] + (-1.0 * m->sphere_radius[k]);
    Artic::AContact c;
    if (dist < m->contact_dist_thresh && w.find_contact(k, m->contact_dist_thresh, c)) cs.push_back(c);
  }
  for (int k = 0; k < m->nboxes; k++) {
    double pa[3], pp[3];
    if (!(box_dist(w, k, pa, pp) < m->contact_dist_thresh)) continue;
    for (int i = 0; i < 8; i++) { double v[3], q[3]; box_vertex(w, k, i, v); w.to_plane(v, q); if (q[1] <= m->contact_dist_thresh) cs.push_back(vertex_contact(w, k, v, q[1])); }
  }
  w.handle_impacts(cs);
  if (w.aux->status & MH_WORLD_LCP_FAILED) return h;
  w.aux->time += h; w.aux->mini_steps++;
  return h;
}

// ---- the stabiliser (Artic::stabilize, CStab:88-131, 306-345, 1056-1216) with the boxes' rows ----
double cstab_eval(Artic& w, std::vector<double>& uC)
{
  const mh_artic_model* m = w.m; const int nj = w.nj;
  double vio = INF_;
  uC.clear();
  w.kinematics();
  for (int s = 0; s < m->nspheres; s++) {
    double ctr[3], cp[3]; w.sphere_center(s, ctr); w.to_plane(ctr, cp);
    uC.push_back(cp[1] + (-1.0 * m->sphere_radius[s])); vio = (uC.back() < vio) ? uC.back() : vio;
  }
  for (int k = 0; k < m->nboxes; k++) { double pa[3], pp[3]; uC.push_back(box_dist(w, k, pa, pp)); vio = (uC.back() < vio) ? uC.back() : vio; }
  for (int j = 0; j < nj; j++) {
    uC.push_back((m->hilimit[0] - w.q[0]) - 0.0); vio = (uC.back() < vio) ? uC.back() : vio;
    uC.push_back((w.q[0] + 0.0) - m->lolimit[0]); vio = (uC.back() < vio) ? uC.back() : vio;
  }
  return vio;
}
double cstab_eval_at(Artic& w, double t, unsigned i, const double* dq, const double* qv)
{
  std::vector<double> uC;
  for (int k = 0; k < w.nj; k++) { double v = dq[k] * t; v = v + qv[k]; w.q[k] = v; }
  cstab_eval(w, uC);
  return uC[i];
}
double sign2(double x, double y) { return (y > 0.0) ? std::fabs(x) : -std::fabs(x); }
double cstab_ridders(Artic& w, double x1, double x2, double fl, double fh, unsigned idx, const double* dq, const double* qv)
{
  const double TOL = 1e-4;
  double ans = INF_, fm, fnew, s2, xh, xl, xm, xnew;
  if ((fl > 0.0 && fh < 0.0) || (fl < 0.0 && fh > 0.0)) {
    xl = x1; xh = x2;
    for (unsigned j = 0; j < 25; j++) {
      xm = 0.5 * (xl + xh);
      fm = cstab_eval_at(w, xm, idx, dq, qv);
      s2 = std::sqrt(fm * fm - fl * fh);
      if (s2 == 0.0) return ans;
      xnew = xm + (xm - xl) * ((fl >= fh ? 1.0 : -1.0) * fm / s2);
      ans = xnew;
      fnew = cstab_eval_at(w, ans, idx, dq, qv);
      if (std::fabs(fnew) < TOL && fnew >= 0.0) return xnew;
      if (sign2(fm, fnew) != fm) { xl = xm; fl = fm; xh = ans; fh = fnew; }
      else if (sign2(fl, fnew) != fl) { xh = ans; fh = fnew; }
      else if (sign2(fh, fnew) != fh) { xl = ans; fl = fnew; }
    }
  } else {
    if (fl == 0.0) return x1;
    if (fh == 0.0) return x2;
  }
  return 0.0;
}
bool cstab_update_q(Artic& w, const double* dq, double* qv)
{
  const int nj = w.nj;
  std::vector<double> uC, uC_old;
  cstab_eval(w, uC_old);
  for (int k = 0; k < nj; k++) { double v = dq[k]; v = v + qv[k]; w.q[k] = v; }
  cstab_eval(w, uC);
  std::vector<char> br(uC.size(), 0);
  for (size_t i = 0; i < uC.size(); i++) br[i] = ((uC_old[i] < 0.0 && uC[i] > 0.0) || (uC_old[i] > 0.0 && uC[i] < 0.0)) ? 1 : 0;
  double t = 1.0;
  for (size_t i = 0; i < br.size(); i++) {
    if (!br[i]) continue;
    const double root = cstab_ridders(w, 0, t, uC_old[i], uC[i], (unsigned)i, dq, qv);
    if (root > 0.0 && root < 1.0) t = (root < t) ? root : t;
  }
  for (int k = 0; k < nj; k++) { double v = dq[k] * t; v = v + qv[k]; w.q[k] = v; }
  cstab_eval(w, uC);
  while (true) {
    bool stop = true;
    for (size_t i = 0; i < br.size(); i++) if (!br[i] && uC[i] < 0.0 && uC_old[i] > uC[i]) { stop = false; break; }
    if (stop) break;
    t *= 0.6;
    if (t < NZ) return false;
    for (int k = 0; k < nj; k++) { double v = dq[k] * t; v = v + qv[k]; w.q[k] = v; }
    cstab_eval(w, uC);
  }
  for (int k = 0; k < nj; k++) qv[k] = w.q[k];
  return true;
}
void stabilize(Artic& w)
{
  const mh_artic_model* m = w.m; const int nj = w.nj; mh_world_aux* aux = w.aux;
  if (m->cstab_max_iterations == 0) return;
  double qd_save[Artic::NJ], qv[Artic::NJ], dq[Artic::NJ];
  for (int i = 0; i < nj; i++) { qd_save[i] = w.qd[i]; qv[i] = w.q[i]; }
  std::vector<double> uC;
  double max_uvio = cstab_eval(w, uC);
  unsigned iterations = 0;
  while (max_uvio < m->cstab_eps) {
    if (iterations == (unsigned)m->cstab_max_iterations) break;
    if (iterations == MH_CSTAB_HARD_CAP) { aux->status |= MH_WORLD_STALLED; break; }
    for (int i = 0; i < nj; i++) { w.qd[i] = 0.0; dq[i] = 0.0; }
    std::vector<Artic::AContact> cs;
    w.kinematics();
    for (int s = 0; s < m->nspheres; s++) {
      double ctr[3], cp[3]; w.sphere_center(s, ctr); w.to_plane(ctr, cp);
      const double low = cp[1] + (-1.0 * m->sphere_radius[s]);
      Artic::AContact c;
      if (low >= NZ) {
        double on_plane[3]; w.from_plane(cp[0], 0.0, cp[2], on_plane); w.from_plane(cp[0], low, cp[2], c.p);
        const double d[3] = { on_plane[0] - c.p[0], on_plane[1] - c.p[1], on_plane[2] - c.p[2] };
        const double len = std::sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
        for (int k = 0; k < 3; k++) c.n[k] = d[k] / len;
        c.s = s; c.link = m->sphere_link[s]; c.dist = low;
        Artic::orthonormal_basis(c.n, c.sv, c.tv);
        cs.push_back(c);
      } else if (w.find_contact(s, NZ, c)) cs.push_back(c);
    }
    for (int k = 0; k < m->nboxes; k++) {                          // CStab:306-345 for (box, plane)
      double pa[3], pp[3];
      const double low = box_dist(w, k, pa, pp);
      if (low >= NZ) {
        double pb[3]; w.from_plane(pp[0], 0.0, pp[2], pb);
        const double d[3] = { pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2] };
        const double len = std::sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
        Artic::AContact c; c.s = -1; c.link = m->box_link[k]; c.dist = low;
        for (int j = 0; j < 3; j++) { c.p[j] = pa[j]; c.n[j] = d[j] / len; }
        Artic::orthonormal_basis(c.n, c.sv, c.tv);
        cs.push_back(c);
      } else {
        for (int i = 0; i < 8; i++) { double v[3], q[3]; box_vertex(w, k, i, v); w.to_plane(v, q); if (q[1] <= NZ) cs.push_back(vertex_contact(w, k, v, q[1])); }
      }
    }
    const int nc = (int)cs.size();
    int idx[2 * Artic::NJ]; bool upper[2 * Artic::NJ]; double viol[2 * Artic::NJ]; int nl = 0;
    for (int i = 0; i < nj; i++) {
      if (m->hilimit[i] < INF_) { idx[nl] = i; upper[nl] = true; viol[nl] = (m->hilimit[i] - w.q[i]) - 0.0; nl++; }
      if (m->lolimit[i] > -INF_) { idx[nl] = i; upper[nl] = false; viol[nl] = (w.q[i] + 0.0) - m->lolimit[i]; nl++; }
    }
    if (nc + nl > 0) {
      const int n = nc + nl;
      if (n > MH_LCP_MAX_N_WAVE) { aux->status |= MH_WORLD_UNSUPPORTED; break; }
      w.kinematics(); w.crba();
      std::vector<double> X(w.H, w.H + nj * nj);
      if (!inverse_spd(nj, X.data(), nj)) { aux->status |= MH_WORLD_LCP_FAILED; break; }
      std::vector<double> C((size_t)nc * nj, 0.0), XC((size_t)nc * nj, 0.0);
      for (int i = 0; i < nc; i++) {
        const int l = cs[i].link;
        double rc[3], com[3], r[3], J[6 * Artic::NJ], wr[6];
        artic::mat3vec(w.R[l], m->com[l], rc);
        for (int k = 0; k < 3; k++) { com[k] = w.x[l][k] + rc[k]; r[k] = cs[i].p[k] - com[k]; }
        w.jacobian(l, com, J);
        artic::cross3(r, cs[i].n, wr + 3);
        for (int k = 0; k < 3; k++) wr[k] = cs[i].n[k];
        for (int j = 0; j < nj; j++) { double acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + wr[k] * J[k * nj + j]; C[(size_t)i * nj + j] = acc; }
      }
      for (int i = 0; i < nc; i++) for (int c = 0; c < nj; c++) {
        double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[(size_t)i * nj + k] * X[k * nj + c];
        XC[(size_t)i * nj + c] = acc;
      }
      std::vector<double> MM((size_t)n * n), Lv(n);
      for (int i = 0; i < nc; i++) for (int j = 0; j < nc; j++) { double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[(size_t)i * nj + k] * XC[(size_t)j * nj + k]; MM[i + (size_t)n * j] = acc; }
      for (int i = 0; i < nc; i++) for (int k2 = 0; k2 < nl; k2++) {
        double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[(size_t)i * nj + k] * X[idx[k2] * nj + k];
        MM[i + (size_t)n * (nc + k2)] = acc; MM[(nc + k2) + (size_t)n * i] = acc;
      }
      for (int a = 0; a < nl; a++) for (int b = a; b < nl; b++) { const double e = X[idx[a] * nj + idx[b]]; MM[(nc + a) + (size_t)n * (nc + b)] = e; MM[(nc + b) + (size_t)n * (nc + a)] = e; }
      for (int i = 0; i < nc; i++) Lv[i] = (cs[i].dist - std::fabs(m->cstab_eps)) - NZ;
      for (int k = 0; k < nl; k++) Lv[nc + k] = (viol[k] - std::fabs(m->cstab_eps)) - NZ;
      Vec z;
      oracle_rand_t rs; std::memcpy(&rs, aux->rng, sizeof(rs));
      LCP lcp; lcp.rng = &rs;
      Trace tr; tr.buf = nullptr; tr.cap = 0;
      lcp.trace = &tr;
      unsigned piv = 0;
      bool ok = lcp.lcp_fast(n, MM.data(), n, Lv.data(), z, -1.0);
      piv += lcp.pivots;
      if (!ok) { ok = lcp.lcp_lemke_regularized(n, MM.data(), n, Lv.data(), z); piv += lcp.pivots; }
      std::memcpy(aux->rng, &rs, sizeof(rs));
      w.lcp_account(n, piv); aux->stab_rows += (unsigned long long)n;
      std::vector<double> dv(nj, 0.0);
      if (nc > 0) for (int r = 0; r < nj; r++) { double acc = 0.0; for (int i = 0; i < nc; i++) { const double ci = (i < (int)z.size()) ? z[i] : 0.0; acc = acc + XC[(size_t)i * nj + r] * ci; } dv[r] = acc; }
      { std::vector<double> t2(nj, 0.0);
        for (int k = 0; k < nl; k++) { const double lk = (nc + k < (int)z.size()) ? z[nc + k] : 0.0; const double ls = upper[k] ? -lk : lk; for (int r = 0; r < nj; r++) t2[r] = t2[r] + ls * X[idx[k] * nj + r]; }
        for (int r = 0; r < nj; r++) dv[r] = (nc > 0) ? dv[r] + t2[r] : t2[r]; }
      for (int r = 0; r < nj; r++) { w.qd[r] = w.qd[r] + dv[r]; dq[r] = w.qd[r]; }
    }
    if (!cstab_update_q(w, dq, qv)) { aux->status |= MH_WORLD_STAB_FAILED; break; }
    max_uvio = cstab_eval(w, uC);
    iterations++;
    aux->stab_iters++;
  }
  for (int i = 0; i < nj; i++) { w.qd[i] = qd_save[i]; w.q[i] = qv[i]; }
}

// Artic::step for a body with contact geometry (the box kernels' artic_contacts_body)
void step(Artic& w, double dt, const mh_artic_drive* D, int B, int b, int s)
{
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  const int FROZEN = MH_WORLD_UNSUPPORTED | MH_WORLD_STALLED;
  if (w.aux->status & FROZEN) return;
  double h = 0.0; unsigned guard = 0;
  while (h < dt) {
    h += do_mini_step(w, dt - h, D, B, b, s);
    if (w.aux->status & MH_WORLD_LCP_FAILED) return;
    if (w.aux->status & FROZEN) break;
    if (++guard > 100000u) { w.aux->status |= MH_WORLD_STALLED; break; }
  }
  stabilize(w);
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  w.aux->steps++;
}

}  // namespace

extern "C" {

// B worlds x nsteps through the box kernels' step, in place.  pose: NULL = angle coordinates, else B x 7 base poses (pose coordinates: each
// step on the world's model copy, folded after a step that ran to its end).  drive: HOST arrays laid out as mh_artic_drive states; NULL or
// terms == 0 = undriven.
void artic_box_ref_step(const mh_artic_model* m, int B, double dt, int nsteps, double* q, double* qd, mh_world_aux* aux, double* pose,
                        const mh_artic_drive* drive)
{
  const int nj = m->nj;
  for (int b = 0; b < B; b++) {
    double* qb = q + (size_t)b * nj; double* qdb = qd + (size_t)b * nj;
    for (int s = 0; s < nsteps; s++) {
      mh_artic_model mb;
      if (pose) artic_pose_ref_model(m, pose + 7 * (size_t)b, &mb); else std::memcpy(&mb, m, sizeof(mb));
      Artic w(&mb, qb, qdb, aux + b);
      const unsigned long long done = aux[b].steps;
      step(w, dt, drive, B, b, s);
      if (pose && aux[b].steps != done) artic_pose_ref_fold(1, nj, qb, qdb, pose + 7 * (size_t)b);
    }
  }
}

}  // extern "C"
