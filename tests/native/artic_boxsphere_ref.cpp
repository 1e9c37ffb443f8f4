// TEST INFRASTRUCTURE: the articulated step with box-sphere contacts between links and static boxes the GPU kernels of mh_artic_bsp.hip are
// held to (include/moby_hip_artic.h, mh_artic_model.pair_kind, box_link = -1).
//
// tests/native/artic_pair_ref.cpp restated (its helpers are file-local and existing files are not edited for a feature) with: the closed-form
// box-sphere geometry of the reference (find_contacts_box_sphere, CCD.inl:1208-1259, over BoxPrimitive::calc_closest_points,
// BoxPrimitive.cpp:183-254, whose projected-gradient QP is replaced by its fixed point, the componentwise clamp; BoxPrimitive::calc_signed_dist,
// BoxPrimitive.cpp:256-276 and 788-836, for conservative advancement and the stabiliser), pairs of both kinds in one list, and static boxes: no
// plane work, no Jacobian term, calc_max_dist = 0.  All pair geometry is computed in the box's frame and carried to the model frame by the box's
// pose.  Operation order = the device's (mh_artic_contacts.inc under MH_ARTIC_BSP_TU).  Pins (tests/test_artic_boxsphere.py): without a
// box-sphere pair or a static box it equals artic_boxsphere_ref_step bit for bit.  Built by the tests with g++ and oracle/Makefile's CXXFLAGS
// (-ffp-contract=off), linked with artic_box_ref.cpp, artic_drive_ref.cpp, artic_pose_ref.cpp and artic_pair_ref.cpp.
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

// a contact between two links: the oracle's record + the reference's geometry B's link (-1 = the plane)
struct PC : Artic::AContact {
  int linkB = -1;                                  // (link = -1 with linkB >= 0: geometry A is a static box)
  PC() {}
  PC(const Artic::AContact& c) : Artic::AContact(c), linkB(-1) {}
};

struct ArticP : Artic {
  using Artic::Artic;
  bool masked(int s) const { return ((m->sphere_no_plane >> s) & 1) != 0; }
  bool below(int link, int j) const { for (int k = link; k >= 0; k = m->parent[k]) if (k == j) return true; return false; }   // joint j is an ancestor of link (itself included)
  // the constraint velocity: A's point velocity along d minus B's; a plane contact keeps its single term
  double cvel(const double V[][6], const PC& c, const double* d = nullptr) const {
    const double* dir = d ? d : c.n;
    double v = 0.0;
    if (c.link >= 0) v = point_vel_dir(V[c.link], c.p, dir);
    if (c.linkB >= 0) { const double vb = point_vel_dir(V[c.linkB], c.p, dir); v = (c.link >= 0) ? v - vb : -vb; }   // a static A has no term
    return v;
  }
  // one link's share of a contact row: [dir, (p - com) x dir] . column j of calc_jacobian(link) at its COM (handle_impacts' expression)
  double row_term(int l, int j, const double* p, const double* dir) const {
    using namespace artic;
    double rc[3], com[3], r[3], J[6 * NJ], w[6];
    mat3vec(R[l], m->com[l], rc);
    for (int k = 0; k < 3; k++) { com[k] = x[l][k] + rc[k]; r[k] = p[k] - com[k]; }
    jacobian(l, com, J);
    cross3(r, dir, w + 3);
    for (int k = 0; k < 3; k++) w[k] = dir[k];
    double acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + w[k] * J[k * nj + j];
    return acc;
  }
  // A's term with dir plus B's with -dir, A's first; a joint that is an ancestor of only one link gets that term alone, of neither 0.0
  double contact_row(const PC& c, int j, const double* dir) const {
    const bool inA = c.link >= 0 && below(c.link, j), inB = c.linkB >= 0 && below(c.linkB, j);
    double val = 0.0;
    if (inA) val = row_term(c.link, j, c.p, dir);
    if (inB) { const double nd[3] = { -dir[0], -dir[1], -dir[2] }; const double tb = row_term(c.linkB, j, c.p, nd); val = inA ? val + tb : tb; }
    return val;
  }
  // the articulated CCD::calc_max_dist (Artic::calc_max_dist) with the floating base's linear velocity only for links that descend from joint 0
  double max_dist(int link, const double n[3], double rmax) const {
    double mv = 0.0;
    if (m->floating_base && below(link, 0)) mv = (n[0] * qd[0] + n[1] * qd[1]) + n[2] * qd[2];
    int inner = link;
    mv = mv + (2.0 * rmax) * std::fabs(qd[inner]);
    while (m->parent[inner] >= 0) {
      const int nxt = m->parent[inner];
      const double d[3] = { x[nxt][0] - x[inner][0], x[nxt][1] - x[inner][1], x[nxt][2] - x[inner][2] };
      mv = mv + std::fabs(qd[nxt]) * std::sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
      inner = nxt;
    }
    return mv;
  }
  // Artic::CA_step with that calc_max_dist
  double CA_sphere(int s, const double V[][6]) const {
    double ctr[3], cp[3]; sphere_center(s, ctr); to_plane(ctr, cp);
    const double dist = cp[1] + (-1.0 * m->sphere_radius[s]);
    AContact c;
    if (!(dist > A_NEAR_ZERO)) {
      const bool has = find_contact(s, A_NEAR_ZERO, c);
      if (has && std::fabs(point_vel_dir(V[c.link], c.p, c.n)) < A_NEAR_ZERO * 10) return A_INF;
    }
    if (dist <= 0.0) {
      if (!find_contact(s, A_NEAR_ZERO, c)) return A_INF;
      if (point_vel_dir(V[c.link], c.p, c.n) < -A_NEAR_ZERO) return 0.0;
      return A_INF;
    }
    double pn[3]; plane_n(pn);
    const double mn[3] = { -pn[0], -pn[1], -pn[2] };
    const double tA = max_dist(m->sphere_link[s], mn, rmax_of(s));
    double total = tA + 0.0;
    if (total < 0.0) total = 0.0;
    const double cand = dist / total;
    return (cand < A_INF) ? cand : A_INF;
  }
  // find_contacts_sphere_sphere (CCD.inl:1163-1206): d = cA - cB, dist = (|d| - rA) - rB, n = d / |d| (from b to a)
  double pair_dist(int k, double cA[3], double cB[3], double n[3]) const {
    const int a = m->pair_a[k], b = m->pair_b[k];
    sphere_center(a, cA); sphere_center(b, cB);
    const double d[3] = { cA[0] - cB[0], cA[1] - cB[1], cA[2] - cB[2] };
    const double len = std::sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
    for (int c = 0; c < 3; c++) n[c] = d[c] / len;
    return (len - m->sphere_radius[a]) - m->sphere_radius[b];
  }
  bool pair_contact(int k, double TOL, PC& c) const {
    double cA[3], cB[3];
    c.dist = pair_dist(k, cA, cB, c.n);
    if (c.dist > TOL) return false;
    const double rA = m->sphere_radius[m->pair_a[k]], rB = m->sphere_radius[m->pair_b[k]];
    for (int j = 0; j < 3; j++) c.p[j] = ((cA[j] - c.n[j] * rA) + (cB[j] + c.n[j] * rB)) * 0.5;
    c.s = -1; c.link = m->sphere_link[m->pair_a[k]]; c.linkB = m->sphere_link[m->pair_b[k]];
    orthonormal_basis(c.n, c.sv, c.tv);
    return true;
  }
  // the sphere rule of conservative advancement for pair k (CCD.cpp:138-235), both bodies' calc_max_dist
  double CA_pair(int k, const double V[][6]) const {
    double cA[3], cB[3], n[3];
    const double dist = pair_dist(k, cA, cB, n);
    PC c;
    if (!(dist > A_NEAR_ZERO)) {
      const bool has = pair_contact(k, A_NEAR_ZERO, c);
      if (has && std::fabs(cvel(V, c)) < A_NEAR_ZERO * 10) return A_INF;
    }
    if (dist <= 0.0) {
      if (!pair_contact(k, A_NEAR_ZERO, c)) return A_INF;
      if (cvel(V, c) < -A_NEAR_ZERO) return 0.0;
      return A_INF;
    }
    const int sa = m->pair_a[k], sb = m->pair_b[k];
    const double mn[3] = { -n[0], -n[1], -n[2] };
    const double tA = max_dist(m->sphere_link[sa], mn, rmax_of(sa));
    const double tB = max_dist(m->sphere_link[sb], n, rmax_of(sb));
    double total = tA + tB;
    if (total < 0.0) total = 0.0;
    const double cand = dist / total;
    return (cand < A_INF) ? cand : A_INF;
  }

  // ---- box-sphere pairs (mh_artic_model.pair_kind = MH_ARTIC_PAIR_BOX_SPHERE): pair_a indexes the box list, pair_b the sphere list ----
  bool is_bsp(int k) const { return m->pair_kind[k] == MH_ARTIC_PAIR_BOX_SPHERE; }
  // box b's pose in the model frame: its axes Rbg (row-major) and centre cb; a static box's is the model's own
  void box_pose(int b, double Rbg[9], double cb[3]) const {
    const int l = m->box_link[b];
    if (l < 0) { for (int c = 0; c < 9; c++) Rbg[c] = m->box_R[b][c]; for (int c = 0; c < 3; c++) cb[c] = m->box_center[b][c]; return; }
    artic::mat3mul(R[l], m->box_R[b], Rbg);
    double rc[3]; artic::mat3vec(R[l], m->box_center[b], rc);
    for (int c = 0; c < 3; c++) cb[c] = x[l][c] + rc[c];
  }
  // the sphere's centre cS (model frame) and c, the same point in the box's frame; h = the half lengths
  void bsp_frame(int k, double Rbg[9], double cb[3], double cS[3], double c[3], double h[3]) const {
    const int b = m->pair_a[k];
    box_pose(b, Rbg, cb); sphere_center(m->pair_b[k], cS);
    const double d[3] = { cS[0] - cb[0], cS[1] - cb[1], cS[2] - cb[2] };
    c[0] = (Rbg[0]*d[0] + Rbg[3]*d[1]) + Rbg[6]*d[2]; c[1] = (Rbg[1]*d[0] + Rbg[4]*d[1]) + Rbg[7]*d[2]; c[2] = (Rbg[2]*d[0] + Rbg[5]*d[1]) + Rbg[8]*d[2];
    for (int i = 0; i < 3; i++) h[i] = m->box_len[b][i] * 0.5;
  }
  // BoxPrimitive::calc_closest_points + find_contacts_box_sphere.  region (optional): 0 face, 1 edge, 2 vertex, 3 the centre inside the box
  // (the count of coordinates of p at their extent: 1, 2, 3, 0)
  bool bsp_contact(int k, double TOL, PC& ct, int* region = nullptr) const {
    double Rbg[9], cb[3], cS[3], c[3], h[3]; bsp_frame(k, Rbg, cb, cS, c, h);
    const double Rs = m->sphere_radius[m->pair_b[k]];
    double p[3], u[3];
    for (int i = 0; i < 3; i++) { p[i] = (c[i] < -h[i]) ? -h[i] : ((c[i] > h[i]) ? h[i] : c[i]); u[i] = p[i] - c[i]; }
    const double nrm = std::sqrt((u[0]*u[0] + u[1]*u[1]) + u[2]*u[2]);
    if (region) { int at = 0; for (int i = 0; i < 3; i++) if (!(std::fabs(p[i]) < h[i])) at++; *region = (at == 0) ? 3 : at - 1; }
    double dist;
    if (std::fabs(p[0]) < h[0] || std::fabs(p[1]) < h[1] || std::fabs(p[2]) < h[2] || nrm < Rs) {
      const double bd = std::min(h[0] - std::fabs(p[0]), std::min(h[1] - std::fabs(p[1]), h[2] - std::fabs(p[2])));
      dist = -std::min(bd, Rs - nrm);
    } else {
      const double sc = Rs / nrm;
      for (int i = 0; i < 3; i++) u[i] = u[i] * sc;
      const double e[3] = { (c[0] + u[0]) - p[0], (c[1] + u[1]) - p[1], (c[2] + u[2]) - p[2] };
      dist = std::sqrt((e[0]*e[0] + e[1]*e[1]) + e[2]*e[2]);
    }
    ct.dist = dist;
    if (dist > TOL) return false;
    double ug[3], pr[3]; artic::mat3vec(Rbg, u, ug); artic::mat3vec(Rbg, p, pr);
    const double sg[3] = { cS[0] + ug[0], cS[1] + ug[1], cS[2] + ug[2] };           // the sphere point, model frame
    const double ulen = std::sqrt((ug[0]*ug[0] + ug[1]*ug[1]) + ug[2]*ug[2]);
    bool own = false;
    if (dist > 0.0) {
      const double pg[3] = { cb[0] + pr[0], cb[1] + pr[1], cb[2] + pr[2] };         // the box point
      const double nd[3] = { pg[0] - sg[0], pg[1] - sg[1], pg[2] - sg[2] };
      const double nl = std::sqrt((nd[0]*nd[0] + nd[1]*nd[1]) + nd[2]*nd[2]);
      for (int i = 0; i < 3; i++) ct.p[i] = (sg[i] + pg[i]) * 0.5;
      if (nl > NZ) { for (int i = 0; i < 3; i++) ct.n[i] = nd[i] / nl; own = true; }
    } else for (int i = 0; i < 3; i++) ct.p[i] = sg[i];
    if (!own) for (int i = 0; i < 3; i++) ct.n[i] = ug[i] / ulen;
    ct.s = -1; ct.link = m->box_link[m->pair_a[k]]; ct.linkB = m->sphere_link[m->pair_b[k]];
    orthonormal_basis(ct.n, ct.sv, ct.tv);
    return true;
  }
  // BoxPrimitive::calc_signed_dist for a sphere: pA the box point, pB the sphere point (model frame)
  double bsp_sdist(int k, double pA[3], double pB[3]) const {
    double Rbg[9], cb[3], cS[3], c[3], h[3]; bsp_frame(k, Rbg, cb, cS, c, h);
    const double Rs = m->sphere_radius[m->pair_b[k]];
    double cl[3] = { c[0], c[1], c[2] };
    bool inside = true; double sq = 0.0, in = -INF_;
    for (int i = 0; i < 3; i++) {
      if (c[i] < -h[i]) { const double dl = c[i] + h[i]; cl[i] = -h[i]; sq += dl * dl; inside = false; }
      else if (c[i] > h[i]) { const double dl = c[i] - h[i]; cl[i] = h[i]; sq += dl * dl; inside = false; }
      else if (inside) { const double dd = -std::min(std::fabs(h[i] - c[i]), std::fabs(c[i] + h[i])); in = std::max(in, dd); }
    }
    const double dist = (inside ? in : std::sqrt(sq)) - Rs;
    const double v[3] = { cl[0] - c[0], cl[1] - c[1], cl[2] - c[2] };
    const double vn = std::sqrt((v[0]*v[0] + v[1]*v[1]) + v[2]*v[2]);
    double pr[3]; artic::mat3vec(Rbg, cl, pr);
    for (int i = 0; i < 3; i++) pA[i] = cb[i] + pr[i];
    if (vn == 0.0) { for (int i = 0; i < 3; i++) pB[i] = cS[i]; }
    else {
      double vg[3]; artic::mat3vec(Rbg, v, vg);
      const double sc = (Rs + std::min(dist, 0.0)) / vn;
      for (int i = 0; i < 3; i++) pB[i] = cS[i] + vg[i] * sc;
    }
    return dist;
  }
  double any_dist(int k) const {
    double a[3], b[3], n[3];
    return is_bsp(k) ? bsp_sdist(k, a, b) : pair_dist(k, a, b, n);
  }
  // the contact of pair k of either kind; the threshold test of do_mini_step reads the signed-distance function first (pdi.dist)
  bool any_contact(int k, double TOL, PC& c) const { return is_bsp(k) ? bsp_contact(k, TOL, c) : pair_contact(k, TOL, c); }
  // the sphere rule of conservative advancement for a box-sphere pair (CCD.cpp:138-235)
  double CA_bsp(int k, const double V[][6]) const {
    double pA[3], pB[3];
    const double dist = bsp_sdist(k, pA, pB);
    PC c;
    if (!(dist > A_NEAR_ZERO)) {
      const bool has = bsp_contact(k, A_NEAR_ZERO, c);
      if (has && std::fabs(cvel(V, c)) < A_NEAR_ZERO * 10) return A_INF;
    }
    if (dist <= 0.0) {
      if (!bsp_contact(k, A_NEAR_ZERO, c)) return A_INF;
      if (cvel(V, c) < -A_NEAR_ZERO) return 0.0;
      return A_INF;
    }
    const double d0[3] = { pA[0] - pB[0], pA[1] - pB[1], pA[2] - pB[2] };
    const double len = std::sqrt((d0[0]*d0[0] + d0[1]*d0[1]) + d0[2]*d0[2]);
    const double n[3] = { d0[0] / len, d0[1] / len, d0[2] / len };
    const double mn[3] = { -n[0], -n[1], -n[2] };
    const int b = m->pair_a[k], sb = m->pair_b[k];
    const double tA = (m->box_link[b] >= 0) ? max_dist(m->box_link[b], mn, rmax_box_of(b)) : 0.0;   // a disabled body (CCD.cpp:589-590)
    const double tB = max_dist(m->sphere_link[sb], n, rmax_of(sb));
    double total = tA + tB;
    if (total < 0.0) total = 0.0;
    const double cand = dist / total;
    return (cand < A_INF) ? cand : A_INF;
  }
  double rmax_box_of(int k) const {
    const int l = m->box_link[k];
    const double d[3] = { m->box_center[k][0] - m->com[l][0], m->box_center[k][1] - m->com[l][1], m->box_center[k][2] - m->com[l][2] };
    const double bx = m->box_len[k][0], by = m->box_len[k][1], bz = m->box_len[k][2];
    return std::sqrt((bx*bx + by*by) + bz*bz) + std::sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
  }

  // Artic::handle_impacts (oracle/artic.hpp) restated for contacts that name two links: the impacting test, the contact rows and the tolerance
  // test after the impact use both links; everything else is the oracle's text
  void handle_impacts2(const std::vector<PC>& cs) {
    using namespace artic;
    const int nc = (int)cs.size();
    int idx[2 * NJ]; bool upper[2 * NJ]; int nl = 0;
    for (int i = 0; i < nj; i++) {                                   // ArticulatedBody.inl:9-43 (q_tare = 0)
      if (q[i] >= m->hilimit[i]) { idx[nl] = i; upper[nl] = true; nl++; }
      if (q[i] <= m->lolimit[i]) { idx[nl] = i; upper[nl] = false; nl++; }
    }
    if (nc + nl == 0) return;
    double V[NJ][6]; link_velocities(V);
    bool impacting = false;                                          // CSim:313-323
    for (int i = 0; i < nc; i++) if (cvel(V, cs[i]) < -A_NEAR_ZERO) impacting = true;       // A's point velocity along n minus B's
    for (int k = 0; k < nl; k++) { const double v = upper[k] ? -qd[idx[k]] : qd[idx[k]]; if (v < -A_NEAR_ZERO) impacting = true; }
    if (!impacting) return;
    // ICH:123-146: the no-slip model when every CONTACT has mu_coulomb >= 100 (limits do not count: an island of limits alone
    // takes it too), otherwise the Drumwright-Shell QP
    const bool noslip = (nc == 0) || (m->cp_mu_coulomb >= 1e2);
    const int n = nc + nl;
    const int nk = (m->cp_nk > 0) ? m->cp_nk : 4, kh = nk / 2;
    const int nvars = 5 * nc + nl, N = nvars + nc + nl + nc * kh;    // ICH-QP:97-112
    // capacities of the build: the no-slip LCP's warm start _v holds MH_NOSLIP_MAX rows, the wave solver MH_LCP_MAX_N_WAVE, the limit tables MH_NOSLIP_MAX limits
    if (noslip ? (n > MH_NOSLIP_MAX) : (N > MH_LCP_MAX_N_WAVE || nl > MH_NOSLIP_MAX)) { aux->status |= MH_WORLD_UNSUPPORTED; return; }
    if (m->algorithm == MH_ARTIC_FSAB) crba();                       // get_generalized_inertia (ICH:1600-1607)
    std::vector<double> X(H, H + nj * nj);
    if (!inverse_spd(nj, X.data(), nj)) { aux->status |= MH_WORLD_LCP_FAILED; return; }
    // contact rows (ICH:1847-1895): wrench [d, r x d] about the link's COM times calc_jacobian at the COM (rows: linear, angular)
    std::vector<double> C[3], XC[3];                                 // C[d]: nc x nj; XC[d] = C[d] X (rows of X_CdT')
    for (int d = 0; d < 3; d++) { C[d].assign((size_t)nc * nj, 0.0); XC[d].assign((size_t)nc * nj, 0.0); }
    for (int i = 0; i < nc; i++) {                                    // two add_contact_dir_to_Jacobian blocks, A's first (contact_row)
      const double* dirs[3] = { cs[i].n, cs[i].sv, cs[i].tv };
      for (int d = 0; d < 3; d++) for (int j = 0; j < nj; j++) C[d][(size_t)i * nj + j] = contact_row(cs[i], j, dirs[d]);
    }
    for (int d = 0; d < 3; d++) for (int i = 0; i < nc; i++) for (int c = 0; c < nj; c++) {
      double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[d][(size_t)i * nj + k] * X[k * nj + c];
      XC[d][(size_t)i * nj + c] = acc;
    }
    // the cross blocks (ICH:2127-2147) and vectors (:2153-2156); compute_limit_components (ICH:1755-1781), signs as there
    std::vector<double> G[3][3], CL[3], Cv[3];
    for (int a = 0; a < 3; a++) for (int b = a; b < 3; b++) {
      G[a][b].assign((size_t)nc * nc, 0.0);
      for (int i = 0; i < nc; i++) for (int j = 0; j < nc; j++) { double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[a][(size_t)i * nj + k] * XC[b][(size_t)j * nj + k]; G[a][b][(size_t)i * nc + j] = acc; }
    }
    for (int d = 0; d < 3; d++) {
      CL[d].assign((size_t)nc * (nl > 0 ? nl : 1), 0.0); Cv[d].assign(nc, 0.0);
      for (int i = 0; i < nc; i++) {
        for (int k2 = 0; k2 < nl; k2++) { double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[d][(size_t)i * nj + k] * X[idx[k2] * nj + k]; CL[d][(size_t)i * nl + k2] = acc; }
        double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[d][(size_t)i * nj + k] * qd[k];
        Cv[d][i] = acc;
      }
    }
    std::vector<double> LL((size_t)nl * nl + 1), Lv(nl + 1);
    for (int a = 0; a < nl; a++) for (int b = a; b < nl; b++) { const double e = X[idx[a] * nj + idx[b]]; LL[a + (size_t)nl * b] = e; LL[b + (size_t)nl * a] = e; }
    for (int k = 0; k < nl; k++) { Lv[k] = qd[idx[k]]; if (upper[k]) Lv[k] = -Lv[k]; }

    std::vector<double> cn(nc, 0.0), csv(nc, 0.0), ctv(nc, 0.0), l(nl, 0.0);
    // dv = X_CnT cn + X_CsT cs + X_CtT ct + X_LT sl (ICH:1365-1373, 345-352): four products, added in this order
    auto apply = [&]() {
      std::vector<double> dv(nj, 0.0), t(nj);
      const std::vector<double>* imp[3] = { &cn, &csv, &ctv };
      for (int d = 0; d < 3; d++) {
        for (int r = 0; r < nj; r++) { double acc = 0.0; for (int i = 0; i < nc; i++) acc = acc + XC[d][(size_t)i * nj + r] * (*imp[d])[i]; t[r] = acc; }
        for (int r = 0; r < nj; r++) dv[r] = (d == 0) ? t[r] : dv[r] + t[r];
      }
      for (int r = 0; r < nj; r++) { double acc = 0.0; for (int k = 0; k < nl; k++) { const double ls = upper[k] ? -l[k] : l[k]; acc = acc + ls * X[idx[k] * nj + r]; } t[r] = acc; }
      for (int r = 0; r < nj; r++) dv[r] = dv[r] + t[r];
      for (int r = 0; r < nj; r++) qd[r] = qd[r] + dv[r];
    };
    // update_constraint_velocities_from_impulses (ICH:427-464)
    auto Gs = [&](int a, int b, int i, int j) -> double { return (a <= b) ? G[a][b][(size_t)i * nc + j] : G[b][a][(size_t)j * nc + i]; };
    auto update_vels = [&]() {
      const std::vector<double>* imp[3] = { &cn, &csv, &ctv };
      for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) {
          std::vector<double> t(nc, 0.0);
          for (int i = 0; i < nc; i++) { double acc = 0.0; for (int j = 0; j < nc; j++) acc = acc + Gs(a, b, i, j) * (*imp[b])[j]; t[i] = acc; }
          for (int i = 0; i < nc; i++) Cv[a][i] = Cv[a][i] + t[i];
        }
        for (int i = 0; i < nc; i++) { double acc = 0.0; for (int k = 0; k < nl; k++) acc = acc + CL[a][(size_t)i * nl + k] * l[k]; Cv[a][i] = Cv[a][i] + acc; }
      }
      const std::vector<double>* imp2[3] = { &cn, &csv, &ctv };
      for (int d = 0; d < 3; d++) for (int k = 0; k < nl; k++) { double acc = 0.0; for (int i = 0; i < nc; i++) acc = acc + CL[d][(size_t)i * nl + k] * (*imp2[d])[i]; Lv[k] = Lv[k] + acc; }
      std::vector<double> t(nl + 1, 0.0);
      for (int r = 0; r < nl; r++) { double acc = 0.0; for (int k = 0; k < nl; k++) acc = acc + LL[r + (size_t)nl * k] * l[k]; t[r] = acc; }
      for (int r = 0; r < nl; r++) Lv[r] = Lv[r] + t[r];
    };
    auto minv_of = [&]() {                                           // calc_min_constraint_velocity (ICH:413-424)
      double mn = A_INF;
      for (int i = 0; i < nc; i++) mn = (i == 0 || Cv[0][i] < mn) ? Cv[0][i] : mn;
      if (nl > 0) { double ml = Lv[0]; for (int k = 1; k < nl; k++) ml = (Lv[k] < ml) ? Lv[k] : ml; mn = (ml < mn) ? ml : mn; }
      return mn;
    };
    auto solve_noslip = [&]() -> bool {
    // apply_no_slip_model (ICH:1009-1417)
    std::vector<int> Sx, Tx; std::vector<double> Y;
    auto build_Y = [&](bool skew) -> int {
      const int ns = (int)Sx.size(), nt = (int)Tx.size(), mm = ns + nt;
      Y.assign((size_t)mm * mm + 1, 0.0);
      for (int a = 0; a < ns; a++) for (int b = 0; b < ns; b++) Y[a + (size_t)mm * b] = G[1][1][(size_t)Sx[a] * nc + Sx[b]];
      for (int a = 0; a < nt; a++) for (int b = 0; b < nt; b++) Y[(ns + a) + (size_t)mm * (ns + b)] = G[2][2][(size_t)Tx[a] * nc + Tx[b]];
      for (int a = 0; a < ns; a++) for (int b = 0; b < nt; b++) { const double g = G[1][2][(size_t)Sx[a] * nc + Tx[b]]; Y[a + (size_t)mm * (ns + b)] = g; Y[(ns + b) + (size_t)mm * a] = g; }
      if (skew) for (int j = 0; j < mm; j++) Y[j + (size_t)mm * j] = Y[j + (size_t)mm * j] - A_NEAR_ZERO;
      return mm;
    };
    for (int i = 0; i < nc; i++) {                                   // greedy largest non-singular tangent set (ICH:1087-1145)
      Sx.push_back(i); int mm = build_Y(true); if (!chol_factor(mm, Y.data(), mm)) Sx.pop_back();
      Tx.push_back(i); mm = build_Y(true);     if (!chol_factor(mm, Y.data(), mm)) Tx.pop_back();
    }
    const int ns = (int)Sx.size(), nt = (int)Tx.size();
    const int mm = build_Y(false);
    if (mm > 0 && !chol_factor(mm, Y.data(), mm)) { aux->status |= MH_WORLD_LCP_FAILED; return false; }   // assert(success)
    // Q X X' (n x mm): contact rows [Cn X Cs'(:,S)  Cn X Ct'(:,T)], limit rows [Cs X L'(S,:)'  Ct X L'(T,:)'] (ICH:1198-1207)
    std::vector<double> QX((size_t)n * mm + 1);
    for (int i = 0; i < nc; i++) {
      for (int a = 0; a < ns; a++) QX[(size_t)i * mm + a] = G[0][1][(size_t)i * nc + Sx[a]];
      for (int a = 0; a < nt; a++) QX[(size_t)i * mm + ns + a] = G[0][2][(size_t)i * nc + Tx[a]];
    }
    for (int k = 0; k < nl; k++) {
      for (int a = 0; a < ns; a++) QX[(size_t)(nc + k) * mm + a] = CL[1][(size_t)Sx[a] * nl + k];
      for (int a = 0; a < nt; a++) QX[(size_t)(nc + k) * mm + ns + a] = CL[2][(size_t)Tx[a] * nl + k];
    }
    std::vector<double> W((size_t)mm * n + 1), col(mm + 1);
    for (int j = 0; j < n; j++) {
      for (int a = 0; a < mm; a++) col[a] = QX[(size_t)j * mm + a];
      if (mm > 0) chol_solve(mm, Y.data(), mm, col.data());
      for (int a = 0; a < mm; a++) W[a + (size_t)mm * j] = col[a];
    }
    std::vector<double> MM((size_t)n * n), qq(n);
    auto QMQ = [&](int i, int j) -> double {                         // Q inv(M) Q' (ICH:1190-1196)
      if (i < nc && j < nc) return G[0][0][(size_t)i * nc + j];
      if (i < nc) return CL[0][(size_t)i * nl + (j - nc)];
      if (j < nc) return CL[0][(size_t)j * nl + (i - nc)];
      return LL[(i - nc) + (size_t)nl * (j - nc)];
    };
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
      double acc = 0.0; for (int a = 0; a < mm; a++) acc = acc + QX[(size_t)i * mm + a] * W[a + (size_t)mm * j];
      MM[i + (size_t)n * j] = QMQ(i, j) - acc;
    }
    std::vector<double> YXv(mm + 1);
    for (int a = 0; a < ns; a++) YXv[a] = Cv[1][Sx[a]];
    for (int a = 0; a < nt; a++) YXv[ns + a] = Cv[2][Tx[a]];
    if (mm > 0) chol_solve(mm, Y.data(), mm, YXv.data());
    for (int i = 0; i < n; i++) {
      double acc = 0.0; for (int a = 0; a < mm; a++) acc = acc + QX[(size_t)i * mm + a] * YXv[a];
      qq[i] = ((i < nc) ? Cv[0][i] : Lv[i - nc]) - acc;
    }
    Vec z; z.d.assign(aux->vns, aux->vns + MH_NOSLIP_MAX); z.len = (unsigned)aux->vns_size;
    oracle_rand_t rs; std::memcpy(&rs, aux->rng, sizeof(rs));
    LCP lcp; lcp.rng = &rs;
    Trace tr; tr.buf = trace ? trace + trace_len : nullptr; tr.cap = trace ? ((trace_cap - trace_len > 0) ? trace_cap - trace_len : 0) : 0;
    lcp.trace = &tr;
    unsigned piv = 0;
    bool ok = lcp.lcp_fast(n, MM.data(), n, qq.data(), z, -1.0);
    piv += lcp.pivots;
    if (!ok) { ok = lcp.lcp_lemke_regularized(n, MM.data(), n, qq.data(), z); piv += lcp.pivots; }
    trace_len += tr.len;
    std::memcpy(aux->rng, &rs, sizeof(rs));
    lcp_account(n, piv);
    if (!ok) { aux->status |= MH_WORLD_LCP_FAILED; return false; }
    for (int k = 0; k < n; k++) aux->vns[k] = z[k];
    aux->vns_size = n;
    std::vector<double> t2(mm + 1);                                  // [cs; ct] = -(Y^-1 X v + Y^-1 (QX)' z) (ICH:1293-1298)
    for (int a = 0; a < mm; a++) { double acc = 0.0; for (int i = 0; i < n; i++) acc = acc + QX[(size_t)i * mm + a] * z[i]; t2[a] = acc; }
    if (mm > 0) chol_solve(mm, Y.data(), mm, t2.data());
    for (int i = 0; i < nc; i++) cn[i] = z[i];
    for (int k = 0; k < nl; k++) l[k] = z[nc + k];
    for (int a = 0; a < ns; a++) csv[Sx[a]] = -(YXv[a] + t2[a]);
    for (int a = 0; a < nt; a++) ctv[Tx[a]] = -(YXv[ns + a] + t2[ns + a]);
      return true;
    };
    // ---- Drumwright-Shell QP -> LCP with contact and limit variables (ICH-QP:94-497) on the persistent _z / _zlast -------
    // variables [cn cs ct ncs nct l], inequality rows [Cn v+ >= 0 (NC); L v+ >= 0 (NL); friction polygons (NC nk/2)]
    auto solve_qp = [&]() -> bool {
      std::vector<double> MM((size_t)N * N, 0.0), qq(N, 0.0);
      auto at = [&](int r, int c2) -> double& { return MM[(size_t)r + (size_t)N * c2]; };
      const int dirs[5] = { 0, 1, 2, 1, 2 }; const double sgn[5] = { 1, 1, 1, -1, -1 };
      for (int a2 = 0; a2 < 5; a2++) {
        for (int b2 = 0; b2 < 5; b2++) for (int i = 0; i < nc; i++) for (int j = 0; j < nc; j++) {
          double g = Gs(dirs[a2], dirs[b2], i, j);
          if (sgn[a2] * sgn[b2] < 0) g = -g;
          at(a2 * nc + i, b2 * nc + j) = g;
        }
        for (int i = 0; i < nc; i++) for (int k = 0; k < nl; k++) {      // Cd X L' and its transpose (ICH-QP:411-434)
          double g = CL[dirs[a2]][(size_t)i * nl + k];
          if (sgn[a2] < 0) g = -g;
          at(a2 * nc + i, 5 * nc + k) = g; at(5 * nc + k, a2 * nc + i) = g;
        }
      }
      for (int a2 = 0; a2 < nl; a2++) for (int b2 = 0; b2 < nl; b2++) at(5 * nc + a2, 5 * nc + b2) = LL[a2 + (size_t)nl * b2];
      for (int i = 0; i < nc; i++) at(i, i) = at(i, i) + m->cp_compliance;                          // ICH-QP:438-440
      for (int i = 0; i < nc; i++) { qq[i] = Cv[0][i]; qq[nc + i] = Cv[1][i]; qq[2*nc + i] = Cv[2][i]; qq[3*nc + i] = -Cv[1][i]; qq[4*nc + i] = -Cv[2][i]; }
      for (int k = 0; k < nl; k++) qq[5 * nc + k] = Lv[k];
      for (int i = 0; i < nc; i++) { for (int c2 = 0; c2 < nvars; c2++) at(nvars + i, c2) = at(i, c2); qq[nvars + i] = Cv[0][i]; }
      for (int k = 0; k < nl; k++) { for (int c2 = 0; c2 < nvars; c2++) at(nvars + nc + k, c2) = at(5 * nc + k, c2); qq[nvars + nc + k] = Lv[k]; }
      int row = nvars + nc + nl;
      for (int i = 0; i < nc; i++) {
        const double vel = std::sqrt(Cv[1][i] * Cv[1][i] + Cv[2][i] * Cv[2][i]);
        for (int j = 0; j < kh; j++) {
          const double theta = (double)j / (kh - 1) * M_PI_2;
          const double ct = std::cos(theta), st_ = std::sin(theta);
          at(row, i) = m->cp_mu_coulomb;
          at(row, nc + i) = -ct; at(row, 3*nc + i) = -ct;
          at(row, 2*nc + i) = -st_; at(row, 4*nc + i) = -st_;
          qq[row] = m->cp_mu_viscous * vel;
          row++;
        }
      }
      for (int r = nvars; r < N; r++) for (int c2 = 0; c2 < nvars; c2++) at(c2, r) = -at(r, c2);
      // solve_qp_work's chain (ICH-QP:157-233)
      Vec z; z.d.assign(aux->zbuf, aux->zbuf + aux->zbuf_cap); z.len = (unsigned)aux->zbuf_size;
      z.resize((unsigned)N);
      if ((int)z.size() == aux->zlast_size) for (int i = 0; i < N; i++) z[i] = aux->zlast[i];
      oracle_rand_t rs; std::memcpy(&rs, aux->rng, sizeof(rs));
      LCP lcp; lcp.rng = &rs;
      Trace tr; tr.buf = trace ? trace + trace_len : nullptr; tr.cap = trace ? ((trace_cap - trace_len > 0) ? trace_cap - trace_len : 0) : 0;
      lcp.trace = &tr;
      unsigned piv = 0;
      std::vector<double> z_in(z.d.begin(), z.d.begin() + N); const oracle_rand_t rs_in = rs;
      bool ok = lcp.lcp_fast_regularized(N, MM.data(), N, qq.data(), z, -20, 4, -8);
      piv += lcp.pivots;
      const unsigned piv_fast = lcp.pivots; const bool ok_fast = ok; unsigned piv_lemke = 0;
      if (!ok) { z.set_zero(); ok = lcp.lcp_lemke_regularized(N, MM.data(), N, qq.data(), z); piv += lcp.pivots; piv_lemke = lcp.pivots; }
      if (g_lcp_dump) {                                                // diagnostic (oracle_dbg_lcp_dump), same record as world.hpp's
        const int hdr[5] = { N, ok_fast ? 1 : 0, (int)piv_fast, (int)piv_lemke, ok ? 1 : 0 };
        std::fwrite(hdr, sizeof(int), 5, g_lcp_dump); std::fwrite(&rs_in, sizeof(rs_in), 1, g_lcp_dump);
        std::fwrite(MM.data(), 8, (size_t)N * N, g_lcp_dump); std::fwrite(qq.data(), 8, N, g_lcp_dump); std::fwrite(z_in.data(), 8, N, g_lcp_dump);
        std::fflush(g_lcp_dump);
      }
      trace_len += tr.len;
      std::memcpy(aux->rng, &rs, sizeof(rs));
      lcp_account(N, piv);
      if (!ok) { aux->status |= MH_WORLD_LCP_FAILED; return false; }   // LCPSolverException
      aux->zlast_size = N;
      for (int i = 0; i < N; i++) { aux->zlast[i] = z[i]; aux->zbuf[i] = z[i]; }
      if (aux->zbuf_cap < N) aux->zbuf_cap = N;
      aux->zbuf_size = nvars;                                          // z repacked to the epd layout = its first N_VARS entries (ICH-QP:236-250)
      return true;
    };
    auto from_stacked = [&]() {                                        // update_from_stacked(q, z) (UCPD:218-228)
      for (int i = 0; i < nc; i++) {
        cn[i] = aux->zbuf[i];
        double sv2 = aux->zbuf[nc + i];   sv2 = sv2 - aux->zbuf[3*nc + i]; csv[i] = sv2;
        double tv2 = aux->zbuf[2*nc + i]; tv2 = tv2 - aux->zbuf[4*nc + i]; ctv[i] = tv2;
      }
      for (int k = 0; k < nl; k++) l[k] = aux->zbuf[5 * nc + k];
    };
    if (noslip) {
      if (!solve_noslip()) return;
      apply(); update_vels();
      const double minv = minv_of();
      bool changed = false;                                            // apply_restitution(q) (ICH:497-525)
      for (int i = 0; i < nc; i++) { cn[i] = cn[i] * m->cp_epsilon; if (!changed && cn[i] > A_NEAR_ZERO) changed = true; }
      for (int k = 0; k < nl; k++) { l[k] = l[k] * m->limit_restitution[idx[k]]; if (!changed && l[k] > A_NEAR_ZERO) changed = true; }
      if (changed) {
        for (int i = 0; i < nc; i++) { csv[i] = 0.0; ctv[i] = 0.0; }
        apply(); update_vels();
        const double minv_plus = minv_of();
        // ICH:284-291 would re-solve and then read the Drumwright-Shell solver's _z, which this path never sized
        if (minv_plus < 0.0 && minv_plus < minv - A_NEAR_ZERO) aux->status |= MH_WORLD_UNSUPPORTED;
      }
    } else {                                                           // apply_model_to_connected_constraints (ICH:530-626)
      if (!solve_qp()) return;
      from_stacked(); apply(); update_vels();
      const double minv = minv_of();
      bool changed = false;                                            // apply_restitution(q, z) (ICH:470-491): cn and l entries of z only
      for (int i = 0; i < nc; i++) { aux->zbuf[i] = aux->zbuf[i] * m->cp_epsilon; if (!changed && aux->zbuf[i] > A_NEAR_ZERO) changed = true; }
      for (int k = 0; k < nl; k++) { double& zl = aux->zbuf[5 * nc + k]; zl = zl * m->limit_restitution[idx[k]]; if (!changed && zl > A_NEAR_ZERO) changed = true; }
      if (changed) {
        from_stacked(); apply(); update_vels();                        // the tangential impulses are applied again in full, as the reference does
        const double minv_plus = minv_of();
        if (minv_plus < 0.0 && minv_plus < minv - A_NEAR_ZERO) {       // ICH:591-600: second solve on the updated C v vectors
          if (!solve_qp()) return;
          from_stacked(); apply();
        }
      }
    }
    link_velocities(V);                                              // ICH:157-167
    for (int i = 0; i < nc; i++) if (cvel(V, cs[i]) < -A_NEAR_ZERO) aux->status |= MH_WORLD_IMPACT_TOL;
    for (int k = 0; k < nl; k++) { const double v = upper[k] ? -qd[idx[k]] : qd[idx[k]]; if (v < -A_NEAR_ZERO) aux->status |= MH_WORLD_IMPACT_TOL; }
  }
};

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
double CA_box(const ArticP& w, int k, const double V[][6])
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
  const double tA = w.max_dist(link, mn0, rmax_box(w, k));
  double total = tA + 0.0;
  if (total < 0.0) total = 0.0;
  const double cand = dist / total;
  return (cand < INF_) ? cand : INF_;
}
PC vertex_contact(const Artic& w, int k, const double v[3], double dist)
{
  PC c; c.s = -1; c.link = w.m->box_link[k]; c.dist = dist;
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

// Artic::do_mini_step with the boxes, the pairs (and the drive)
double do_mini_step(ArticP& w, double dt, const mh_artic_drive* D, int B, int b, int s)
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
  double qdd[Artic::NJ], tau[Artic::NJ];
  const bool driven = drive_tau(D, B, b, s, nj, w.q, w.qd, tau);
  const bool ok = (m->algorithm == MH_ARTIC_FSAB) ? w.fwd_dyn_aba(driven ? tau : nullptr, qdd) : w.fwd_dyn(driven ? tau : nullptr, qdd);
  if (!ok) { w.aux->status |= MH_WORLD_LCP_FAILED; return h; }
  for (int i = 0; i < nj; i++) w.qd[i] = w.qd[i] + qdd[i] * h;
  std::vector<PC> cs;                                 // spheres, then every box's vertices within the threshold
  for (int k = 0; k < m->nspheres; k++) {
    if (w.masked(k)) continue;
    double ctr[3], cp[3]; w.sphere_center(k, ctr); w.to_plane(ctr, cp);
    const double dist = cp[1] + (-1.0 * m->sphere_radius[k]);
    Artic::AContact c;
    if (dist < m->contact_dist_thresh && w.find_contact(k, m->contact_dist_thresh, c)) cs.push_back(c);
  }
  for (int k = 0; k < m->nboxes; k++) {
    double pa[3], pp[3];
    if (m->box_link[k] < 0) continue;                  // a static box never meets the plane
    if (!(box_dist(w, k, pa, pp) < m->contact_dist_thresh)) continue;
    for (int i = 0; i < 8; i++) { double v[3], q[3]; box_vertex(w, k, i, v); w.to_plane(v, q); if (q[1] <= m->contact_dist_thresh) cs.push_back(vertex_contact(w, k, v, q[1])); }
  }
  for (int k = 0; k < m->npairs; k++) {
    PC c;
    if (w.is_bsp(k)) { if (w.any_dist(k) < m->contact_dist_thresh && w.bsp_contact(k, m->contact_dist_thresh, c)) cs.push_back(c); }
    else if (w.pair_contact(k, m->contact_dist_thresh, c) && c.dist < m->contact_dist_thresh) cs.push_back(c);
  }
  w.handle_impacts2(cs);
  if (w.aux->status & MH_WORLD_LCP_FAILED) return h;
  w.aux->time += h; w.aux->mini_steps++;
  return h;
}

// ---- the stabiliser (Artic::stabilize, CStab:88-131, 306-345, 1056-1216) with the boxes' and the pairs' rows ----
double cstab_eval(ArticP& w, std::vector<double>& uC)
{
  const mh_artic_model* m = w.m; const int nj = w.nj;
  double vio = INF_;
  uC.clear();
  w.kinematics();
  for (int s = 0; s < m->nspheres; s++) {
    if (w.masked(s)) continue;
    double ctr[3], cp[3]; w.sphere_center(s, ctr); w.to_plane(ctr, cp);
    uC.push_back(cp[1] + (-1.0 * m->sphere_radius[s])); vio = (uC.back() < vio) ? uC.back() : vio;
  }
  for (int k = 0; k < m->nboxes; k++) { if (m->box_link[k] < 0) continue; double pa[3], pp[3]; uC.push_back(box_dist(w, k, pa, pp)); vio = (uC.back() < vio) ? uC.back() : vio; }
  for (int k = 0; k < m->npairs; k++) { uC.push_back(w.any_dist(k)); vio = (uC.back() < vio) ? uC.back() : vio; }
  for (int j = 0; j < nj; j++) {
    uC.push_back((m->hilimit[0] - w.q[0]) - 0.0); vio = (uC.back() < vio) ? uC.back() : vio;
    uC.push_back((w.q[0] + 0.0) - m->lolimit[0]); vio = (uC.back() < vio) ? uC.back() : vio;
  }
  return vio;
}
double cstab_eval_at(ArticP& w, double t, unsigned i, const double* dq, const double* qv)
{
  std::vector<double> uC;
  for (int k = 0; k < w.nj; k++) { double v = dq[k] * t; v = v + qv[k]; w.q[k] = v; }
  cstab_eval(w, uC);
  return uC[i];
}
double sign2(double x, double y) { return (y > 0.0) ? std::fabs(x) : -std::fabs(x); }
double cstab_ridders(ArticP& w, double x1, double x2, double fl, double fh, unsigned idx, const double* dq, const double* qv)
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
bool cstab_update_q(ArticP& w, const double* dq, double* qv)
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
void stabilize(ArticP& w)
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
    std::vector<PC> cs;
    w.kinematics();
    for (int s = 0; s < m->nspheres; s++) {
      if (w.masked(s)) continue;
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
      if (m->box_link[k] < 0) continue;
      const double low = box_dist(w, k, pa, pp);
      if (low >= NZ) {
        double pb[3]; w.from_plane(pp[0], 0.0, pp[2], pb);
        const double d[3] = { pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2] };
        const double len = std::sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
        PC c; c.s = -1; c.link = m->box_link[k]; c.dist = low;
        for (int j = 0; j < 3; j++) { c.p[j] = pa[j]; c.n[j] = d[j] / len; }
        Artic::orthonormal_basis(c.n, c.sv, c.tv);
        cs.push_back(c);
      } else {
        for (int i = 0; i < 8; i++) { double v[3], q[3]; box_vertex(w, k, i, v); w.to_plane(v, q); if (q[1] <= NZ) cs.push_back(vertex_contact(w, k, v, q[1])); }
      }
    }
    for (int k = 0; k < m->npairs; k++) {                          // CStab:306-345 for a sphere pair: the synthetic contact on A's surface, or find_contacts'
      double cA[3], cB[3], n[3];
      if (w.is_bsp(k)) {                                           // ... for a box-sphere pair: A's closest point of the signed-distance function, normal B to A
        const double low = w.bsp_sdist(k, cA, cB);
        PC c;
        if (low >= NZ) {
          const double d[3] = { cA[0] - cB[0], cA[1] - cB[1], cA[2] - cB[2] };
          const double len = std::sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
          for (int j = 0; j < 3; j++) { c.p[j] = cA[j]; c.n[j] = d[j] / len; }
          c.s = -1; c.link = m->box_link[m->pair_a[k]]; c.linkB = m->sphere_link[m->pair_b[k]]; c.dist = low;
          Artic::orthonormal_basis(c.n, c.sv, c.tv);
          cs.push_back(c);
        } else if (w.bsp_contact(k, NZ, c)) cs.push_back(c);                 // (signed_violation = the contact's own distance)
        continue;
      }
      const double low = w.pair_dist(k, cA, cB, n);
      PC c;
      if (low >= NZ) {
        const double rA = m->sphere_radius[m->pair_a[k]];
        for (int j = 0; j < 3; j++) { c.p[j] = cA[j] - n[j] * rA; c.n[j] = n[j]; }
        c.s = -1; c.link = m->sphere_link[m->pair_a[k]]; c.linkB = m->sphere_link[m->pair_b[k]]; c.dist = low;
        Artic::orthonormal_basis(c.n, c.sv, c.tv);
        cs.push_back(c);
      } else if (w.pair_contact(k, NZ, c)) cs.push_back(c);
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
      for (int i = 0; i < nc; i++) for (int j = 0; j < nj; j++) C[(size_t)i * nj + j] = w.contact_row(cs[i], j, cs[i].n);   // two-link rows, normal direction
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

// Artic::step for a body with contact geometry (the pair kernels' artic_contacts_body)
void step(ArticP& w, double dt, const mh_artic_drive* D, int B, int b, int s)
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

// B worlds x nsteps through the pair kernels' step, in place.  pose: NULL = angle coordinates, else B x 7 base poses (pose coordinates: each
// step on the world's model copy, folded after a step that ran to its end).  drive: HOST arrays laid out as mh_artic_drive states; NULL or
// terms == 0 = undriven.
void artic_boxsphere_ref_step(const mh_artic_model* m, int B, double dt, int nsteps, double* q, double* qd, mh_world_aux* aux, double* pose,
                        const mh_artic_drive* drive)
{
  const int nj = m->nj;
  for (int b = 0; b < B; b++) {
    double* qb = q + (size_t)b * nj; double* qdb = qd + (size_t)b * nj;
    for (int s = 0; s < nsteps; s++) {
      mh_artic_model mb;
      if (pose) artic_pose_ref_model(m, pose + 7 * (size_t)b, &mb); else std::memcpy(&mb, m, sizeof(mb));
      ArticP w(&mb, qb, qdb, aux + b);
      const unsigned long long done = aux[b].steps;
      step(w, dt, drive, B, b, s);
      if (pose && aux[b].steps != done) artic_pose_ref_fold(1, nj, qb, qdb, pose + 7 * (size_t)b);
    }
  }
}

// the conservative-advancement bounds of one state, in the order the step takes them: every sphere that meets the plane, the boxes, the pairs
// (DBL_MAX = no bound); returns how many were written
int artic_boxsphere_ref_ca(const mh_artic_model* m, double* q, double* qd, double* out)
{
  mh_world_aux aux; std::memset(&aux, 0, sizeof(aux));
  ArticP w(m, q, qd, &aux);
  double V[Artic::NJ][6];
  w.kinematics(); w.link_velocities(V);
  int n = 0;
  for (int k = 0; k < m->nspheres; k++) { if (w.masked(k)) continue; out[n++] = w.CA_sphere(k, V); }
  for (int k = 0; k < m->nboxes; k++) if (m->box_link[k] >= 0) out[n++] = CA_box(w, k, V);
  for (int k = 0; k < m->npairs; k++) out[n++] = w.is_bsp(k) ? w.CA_bsp(k, V) : w.CA_pair(k, V);
  return n;
}

// the pairs' signed distances of one state
int artic_boxsphere_ref_dist(const mh_artic_model* m, double* q, double* qd, double* out)
{
  mh_world_aux aux; std::memset(&aux, 0, sizeof(aux));
  ArticP w(m, q, qd, &aux);
  w.kinematics();
  for (int k = 0; k < m->npairs; k++) out[k] = w.any_dist(k);
  return m->npairs;
}

// the contact of pair k at one state through the reference's contact entry (find_contacts with tolerance TOL): out = point (3), normal (3),
// distance, region (0 face, 1 edge, 2 vertex, 3 the sphere's centre inside the box; sphere pairs: -1).  Returns 1 if there is a contact,
// 0 if not (out[6] and out[7] are still written for a box-sphere pair).
int artic_boxsphere_ref_contact(const mh_artic_model* m, double* q, double* qd, int k, double TOL, double* out)
{
  mh_world_aux aux; std::memset(&aux, 0, sizeof(aux));
  ArticP w(m, q, qd, &aux);
  w.kinematics();
  PC c; int region = -1;
  const bool has = w.is_bsp(k) ? w.bsp_contact(k, TOL, c, &region) : w.pair_contact(k, TOL, c);
  out[6] = c.dist; out[7] = (double)region;
  if (!has) return 0;
  for (int j = 0; j < 3; j++) { out[j] = c.p[j]; out[3 + j] = c.n[j]; }
  return 1;
}

// the regions the box-sphere pairs of B states are in, and their signed distances: region[b * npairs + k] (as above; -1 for a sphere pair),
// dist[b * npairs + k].  What the tests choose their initial states with and assert their coverage from.
void artic_boxsphere_ref_regions(const mh_artic_model* m, int B, const double* q, const double* pose, int* region, double* dist)
{
  const int nj = m->nj;
  for (int b = 0; b < B; b++) {
    mh_artic_model mb;
    if (pose) artic_pose_ref_model(m, pose + 7 * (size_t)b, &mb); else std::memcpy(&mb, m, sizeof(mb));
    double qb[Artic::NJ], qdb[Artic::NJ];
    for (int j = 0; j < nj; j++) { qb[j] = q[(size_t)b * nj + j]; qdb[j] = 0.0; }
    mh_world_aux aux; std::memset(&aux, 0, sizeof(aux));
    ArticP w(&mb, qb, qdb, &aux);
    w.kinematics();
    for (int k = 0; k < m->npairs; k++) {
      int r = -1; PC c;
      if (w.is_bsp(k)) w.bsp_contact(k, -INF_, c, &r);
      region[(size_t)b * m->npairs + k] = r; dist[(size_t)b * m->npairs + k] = w.any_dist(k);
    }
  }
}

}  // extern "C"
