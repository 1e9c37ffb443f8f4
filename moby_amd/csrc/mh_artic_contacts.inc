// mh_artic_contacts.inc -- included by mh_artic_dev.h inside namespace mh::artic.
//
// The articulated stepper for bodies whose links carry sphere primitives (mh_artic_model.nspheres > 0) against one static plane:
// TimeSteppingSimulator::step in full (TSS:52-222) -- conservative advancement over the (sphere, plane) pairs with the ARTICULATED
// CCD::calc_max_dist (CCD.cpp:138-405, 545-583), mini-steps, find_contacts_sphere_plane (CCD.inl:804-847), contact rows
// [d, r x d] . calc_jacobian(link) (ICH:1847-1895), compute_problem_data's blocks (ICH:2110-2160), the no-slip model with contact
// AND limit rows (ICH:236-295, 1009-1417) for mu_coulomb >= 100, the Drumwright-Shell QP -> LCP with contact and limit variables
// (ICH:530-626, ICH-QP:94-497) below that.  Operation order = oracle/artic.hpp (handle_impacts, do_mini_step), bit for bit.
//
// A kernel of its own (k_artic_step_contacts): config 5's kernel keeps its 10 KB LDS image and its register budget.  One
// wavefront per world; the link quantities of mh_artic_dev.h's Lay first, then the contact work area below (8 KB at 10 joints + three arrays inside the dead forward-dynamics arrays).
// Element-wise products run one output per lane with the oracle's inner loop; the greedy tangent set (<= 8 Cholesky
// factorisations of <= 8 x 8) and the Schur-complement assembly run on lane 0 out of LDS -- no private arrays, no barriers
// under divergent control flow.

#ifdef MH_ARTIC_PAIR_TU
// the pair kernels (mh_artic_pair.hip): the box kernels' sizes with room for the sphere pairs between links in the contact list.  The box-sphere
// kernels (mh_artic_bsp.hip, MH_ARTIC_BSP_TU on top of the two switches) keep these sizes: a pair slot holds a pair of either kind
constexpr int NS = MH_NOSLIP_MAX;
constexpr int NCL = MH_ARTIC_MAX_SPHERES + 8 * MH_ARTIC_MAX_BOXES + MH_ARTIC_MAX_PAIRS;
#elif defined(MH_ARTIC_BOX_TU)
// the box kernels (mh_artic_box.hip): the impact handler holds MH_NOSLIP_MAX contacts (four box feet flat on the ground under the no-slip
// model); the contact list holds every sphere and every box vertex, so that the impacting test and the stabiliser see all of them
constexpr int NS = MH_NOSLIP_MAX;
constexpr int NCL = MH_ARTIC_MAX_SPHERES + 8 * MH_ARTIC_MAX_BOXES;
#else
constexpr int NS = MH_ARTIC_MAX_SPHERES;
constexpr int NCL = NS;
#endif
constexpr int NR = MH_NOSLIP_MAX;
constexpr int MT = 2 * NS;                                  // largest tangent set
constexpr int LOFF = (3 * NS <= 32) ? 32 : 3 * NS;          // first lane of the limit rows where lanes < 3 nc hold the contact rows
constexpr double A_INF_ = 1.7976931348623157e308;

#ifdef MH_ARTIC_PAIR_TU
constexpr int NINTS = (16 + 2 * NCL + 2 * NS + 2 + 1) / 2;  // the ints below, in doubles
#elif defined(MH_ARTIC_BOX_TU)
constexpr int NINTS = (16 + NCL + 2 * NS + 2 + 1) / 2;      // the ints below, in doubles
#else
constexpr int NINTS = 24;
#endif
struct LayC {
  int qsave, V, cp, C, XC, G, CL, Cv, Lv, MM, qq, QX, W, Yy, YXv, t2, imp, l, A, art, ints, total;
#ifdef MH_ARTIC_REPORT_TU
  int racc, rslot;      // the contact report (mh_artic_rp.hip): the contacts' accumulated (cn, cs, ct), laid out as imp; the contacts' slots, NCL ints beside clink
#endif
  // The arrays that live across calls (qsave, V, the contact list, ints) and most temporaries sit behind the config-5 image; the
  // three largest temporaries (MM, the LU scratch A, the C X C' blocks G) go into the forward-dynamics arrays that are dead while
  // the impact handler runs (I6 .. Iv of mh_artic_dev.h's Lay: composite inertias, RNEA velocities / accelerations / forces --
  // rebuilt by the next dynamics call; R, x, S, H, L, X are NOT in there) when they fit: 18 KB instead of 25 KB at 10 joints.
  __host__ __device__ LayC(int base, int n, int arena, int arena_size) {
    int o = base, a = arena;
    const int a_end = arena + arena_size;
    qsave = o; o += n; V = o; o += 6 * n; cp = o; o += 12 * NCL;
    C = o; o += 3 * NS * n; XC = o; o += 3 * NS * n; CL = o; o += 3 * NS * NR; Cv = o; o += 3 * NS;
    Lv = o; o += NR; qq = o; o += NR;
    QX = o; o += NR * MT; W = o; o += MT * NR; Yy = o; o += MT * MT; YXv = o; o += MT; t2 = o; o += MT;
    imp = o; o += 3 * NS; l = o; o += NR; art = o; o += MH_LCP_MAX_N_WAVE /* Lemke's artificial column: up to 64 rows in the Drumwright-Shell LCP */; ints = o; o += NINTS;
#ifdef MH_ARTIC_REPORT_TU
    racc = o; o += 3 * NS; rslot = o; o += (NCL + 1) / 2;           // (in front of the rule below that moves G to the workspace: it counts them)
#endif
    if (a + NR * NR <= a_end) { MM = a; a += NR * NR; } else { MM = o; o += NR * NR; }
    if (a + NR * NR <= a_end) { A = a; a += NR * NR; } else { A = o; o += NR * NR; }
#ifdef MH_ARTIC_PAIR_TU
    // the pair kernels' image must fit a workgroup's 64 KB up to MH_ARTIC_MAX_JOINTS: where G would push it over (from 12 joints on), G goes to
    // the world's HBM workspace instead (G = -1; handle_impacts picks the pointer)
    if (a + 6 * NS * NS <= a_end) { G = a; a += 6 * NS * NS; } else if (sizeof(double) * (size_t)(o + 6 * NS * NS) > 65536) G = -1; else { G = o; o += 6 * NS * NS; }
#else
    if (a + 6 * NS * NS <= a_end) { G = a; a += 6 * NS * NS; } else { G = o; o += 6 * NS * NS; }
#endif
    total = o;
  }
};
// ints: idx[16] (joint | upper << 8), clink[NCL], Sx[NS], Tx[NS], ns, nt
#ifdef MH_ARTIC_PAIR_TU
// ... and a second link table beside clink: clinkB[NCL], the contact's other link (the reference's geometry B), -1 = the plane
constexpr int I_IDX = 0, I_LINK = 16, I_LINKB = I_LINK + NCL, I_SX = I_LINKB + NCL, I_TX = I_SX + NS, I_NS = I_TX + NS, I_NT = I_NS + 1;
#define MH_SET_LINKB(i, v) ints[I_LINKB + (i)] = (v);
#define MH_BASE_PARAM , bool on_base
#define MH_BASE_ARG(M_, link_) , ((M_).anc[link_] & 1u) != 0u
#define MH_ON_BASE && on_base
#define MH_SKIP_MASKED(M_, s_) if (((M_).pr.no_plane >> (s_)) & 1) continue;
#ifdef MH_ARTIC_BSP_TU
// the box-sphere kernels (mh_artic_bsp.hip): a static box (link -1) has no plane work
#define MH_SKIP_STATIC(M_, k_) if ((M_).bx.link[k_] < 0) continue;
#else
#define MH_SKIP_STATIC(M_, k_)
#endif
#else
constexpr int I_IDX = 0, I_LINK = 16, I_SX = I_LINK + NCL, I_TX = I_SX + NS, I_NS = I_TX + NS, I_NT = I_NS + 1;
#define MH_SET_LINKB(i, v)
#define MH_BASE_PARAM
#define MH_BASE_ARG(M_, link_)
#define MH_ON_BASE
#define MH_SKIP_MASKED(M_, s_)
#define MH_SKIP_STATIC(M_, k_)
#endif
// the per-world HBM workspace: _MM and the Lemke LU workspace of the Drumwright-Shell / stabiliser LCP (2 x 64 x 64); the box kernels' stabiliser
// adds Cn and Cn X for up to 64 contacts and the distances of the whole contact list behind them
constexpr size_t WS_C = 2 * MH_LCP_MAX_N_WAVE * MH_LCP_MAX_N_WAVE, WS_XC = WS_C + MH_LCP_MAX_N_WAVE * NJ, WS_DIST = WS_XC + MH_LCP_MAX_N_WAVE * NJ;
constexpr size_t WS_BOX = WS_DIST + MH_ARTIC_MAX_SPHERES + 8 * MH_ARTIC_MAX_BOXES;
constexpr size_t WS_PAIR_G = WS_BOX + MH_ARTIC_MAX_PAIRS + 2;   // the pair kernels: the pairs' distances behind the boxes', then the C X C' blocks of a
constexpr size_t WS_PAIR = WS_PAIR_G + 6 * MH_NOSLIP_MAX * MH_NOSLIP_MAX;   // model whose LDS image has no room for them (LayC::G < 0)
#ifdef MH_ARTIC_PAIR_TU
constexpr size_t WS_WORLD = WS_PAIR;
constexpr int USTRIDE = 56;                                  // the stabiliser's uC vectors: 4 + 8 + 6 distances + 32 slacks
#elif defined(MH_ARTIC_BOX_TU)
constexpr size_t WS_WORLD = WS_BOX;
constexpr int USTRIDE = 48;
#endif
// the arena = Lay's I6, v, a, f, F, Iv (contiguous, 60 nj + 12 doubles); its offset from the layout itself on the device, by the
// same arithmetic on the host (q qd qdd C: 4 nj; H L X: 3 nj^2; R x S: 18 nj -- Rl, tl share v and a since round 5)
static size_t lds_bytes_contacts(int nj) {
  const LayC z((int)(lds_bytes(nj) / sizeof(double)), nj, 4 * nj + 3 * nj * nj + 18 * nj, 60 * nj + 12);
  return sizeof(double) * (size_t)z.total;
}

MH_DEV void plane_n(const mh_artic_model& m, double n[3]) { n[0] = m.plane_R[1]; n[1] = m.plane_R[4]; n[2] = m.plane_R[7]; }
MH_DEV void to_plane(const mh_artic_model& m, const double p[3], double o[3]) {
  const double* Rp = m.plane_R; const double d[3] = { p[0] - m.plane_o[0], p[1] - m.plane_o[1], p[2] - m.plane_o[2] };
  o[0] = (Rp[0]*d[0] + Rp[3]*d[1]) + Rp[6]*d[2]; o[1] = (Rp[1]*d[0] + Rp[4]*d[1]) + Rp[7]*d[2]; o[2] = (Rp[2]*d[0] + Rp[5]*d[1]) + Rp[8]*d[2];
}
MH_DEV void from_plane(const mh_artic_model& m, double px, double py, double pz, double o[3]) {
  const double* Rp = m.plane_R;
  o[0] = m.plane_o[0] + ((Rp[0]*px + Rp[1]*py) + Rp[2]*pz); o[1] = m.plane_o[1] + ((Rp[3]*px + Rp[4]*py) + Rp[5]*pz); o[2] = m.plane_o[2] + ((Rp[6]*px + Rp[7]*py) + Rp[8]*pz);
}
// sphere s's centre in the plane frame, from the link frames in LDS (every lane computes the same numbers)
MH_DEV void sphere_in_plane(const mh_artic_model& m, const Lay& Y, const double* g, int s, double cp[3]) {
  const int l = m.sphere_link[s];
  double rc[3], c[3]; mat3vec(g + Y.R + 9 * l, m.sphere_center[s], rc);
  for (int k = 0; k < 3; k++) c[k] = g[Y.x + 3 * l + k] + rc[k];
  to_plane(m, c, cp);
}
MH_DEV double point_vel_dir(const double* V6, const double* p, const double* d) {
  double wxp[3]; cross3(V6, p, wxp);
  const double v[3] = { V6[3] + wxp[0], V6[4] + wxp[1], V6[5] + wxp[2] };
  return dot3(d, v);
}
MH_DEV void orthonormal_basis(const double n[3], double s[3], double t[3]) {
  const double ax = fabs(n[0]), ay = fabs(n[1]), az = fabs(n[2]);
  double e[3] = { 0.0, 0.0, 0.0 };
  if (ax <= ay && ax <= az) e[0] = 1.0; else if (ay <= az) e[1] = 1.0; else e[2] = 1.0;
  cross3(n, e, s);
  const double len = sqrt((s[0]*s[0] + s[1]*s[1]) + s[2]*s[2]);
  for (int k = 0; k < 3; k++) s[k] = s[k] / len;
  cross3(n, s, t);
}
// find_contacts_sphere_plane (CCD.inl:804-847): the contact point, or false
MH_DEV bool find_contact(const mh_artic_model& m, const Lay& Y, const double* g, int s, double TOL, double p[3]) {
  double cp[3]; sphere_in_plane(m, Y, g, s, cp);
  const double r = m.sphere_radius[s];
  const double dist = cp[1] - r;
  if (dist > TOL) return false;
  from_plane(m, cp[0], 0.5 * (cp[1] - r), cp[2], p);
  return true;
}
// spatial velocity of every link about the world origin: V_i = V_parent + S_i qd_i, summed from the base outward (ancestors have
// smaller indices: joints are listed parents first)
MH_DEV void link_velocities(const Model& M, const Lay& Y, const LayC& Z, double* g) {
  const int nj = Y.nj, lane = lane_id();
  for (int e = lane; e < 6 * nj; e += 64) {
    const int i = e / 6, k = e - 6 * i;
    double acc = 0.0; bool first = true;
    for (int j = 0; j <= i; j++) if ((M.anc[i] >> j) & 1u) { const double vj = g[Y.S + 6 * j + k] * g[Y.qd + j]; acc = first ? vj : acc + vj; first = false; }
    g[Z.V + e] = acc;
  }
  wave_sync();
}
// the articulated CCD::calc_max_dist (CCD.cpp:545-583); n: the direction of approach (a floating base adds its linear velocity along it: the three virtual sliders' rates)
MH_DEV double calc_max_dist(const mh_artic_model& m, const Lay& Y, const double* g, int link, const double* n, double rmax MH_BASE_PARAM) {
  double mv = 0.0;
  if (m.floating_base MH_ON_BASE) mv = (n[0] * g[Y.qd] + n[1] * g[Y.qd + 1]) + n[2] * g[Y.qd + 2];
  int inner = link;
  mv = mv + (2.0 * rmax) * fabs(g[Y.qd + inner]);
  while (m.parent[inner] >= 0) {
    const int nxt = m.parent[inner];
    const double d[3] = { g[Y.x + 3*nxt] - g[Y.x + 3*inner], g[Y.x + 3*nxt + 1] - g[Y.x + 3*inner + 1], g[Y.x + 3*nxt + 2] - g[Y.x + 3*inner + 2] };
    mv = mv + fabs(g[Y.qd + nxt]) * sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
    inner = nxt;
  }
  return mv;
}
MH_DEV double rmax_of(const mh_artic_model& m, int s) {
  const int l = m.sphere_link[s];
  const double d[3] = { m.sphere_center[s][0] - m.com[l][0], m.sphere_center[s][1] - m.com[l][1], m.sphere_center[s][2] - m.com[l][2] };
  return m.sphere_radius[s] + sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
}
// CCD::calc_CA_Euler_step_sphere -> _generic -> calc_next_CA_Euler_step_generic (CCD.cpp:138-405); uniform
MH_DEV double CA_step(const mh_artic_model& m, const Lay& Y, const LayC& Z, const double* g, int s MH_BASE_PARAM) {
  double cp[3]; sphere_in_plane(m, Y, g, s, cp);
  const double dist = cp[1] + (-1.0 * m.sphere_radius[s]);
  const int link = m.sphere_link[s];
  double n[3]; plane_n(m, n);
  double p[3];
  if (!(dist > NEAR_ZERO_)) {
    const bool has = find_contact(m, Y, g, s, NEAR_ZERO_, p);
    if (has && fabs(point_vel_dir(g + Z.V + 6 * link, p, n)) < NEAR_ZERO_ * 10) return A_INF_;
  }
  if (dist <= 0.0) {
    if (!find_contact(m, Y, g, s, NEAR_ZERO_, p)) return A_INF_;
    if (point_vel_dir(g + Z.V + 6 * link, p, n) < -NEAR_ZERO_) return 0.0;
    return A_INF_;
  }
  const double mn[3] = { -n[0], -n[1], -n[2] };
#ifdef MH_ARTIC_PAIR_TU
  const double tA = calc_max_dist(m, Y, g, link, mn, rmax_of(m, s), on_base);
#else
  const double tA = calc_max_dist(m, Y, g, link, mn, rmax_of(m, s));
#endif
  double total = tA + 0.0;
  if (total < 0.0) total = 0.0;
  const double cand = dist / total;
  return (cand < A_INF_) ? cand : A_INF_;
}

#ifdef MH_ARTIC_BOX_TU
// ---- box primitives on links (mh_artic_model.nboxes; the model's box block is read from M.bx).  Every lane computes the same numbers. ----
// vertex i of box k in the model frame, BoxPrimitive::get_vertices order (BoxPrimitive.cpp:358-365): the link frame's centre + Rb (+-x/2, +-y/2, +-z/2)
MH_DEV void box_vertex(const Model& M, const Lay& Y, const double* g, int k, int i, double v[3]) {
  const Boxes& X = M.bx; const int l = X.link[k];
  const double hx = X.len[k][0] * 0.5, hy = X.len[k][1] * 0.5, hz = X.len[k][2] * 0.5;
  const double px = (i & 4) ? -hx : hx, py = (i & 2) ? -hy : hy, pz = (i & 1) ? -hz : hz;
  const double* Rb = X.R[k];
  const double lp[3] = { X.center[k][0] + ((Rb[0]*px + Rb[1]*py) + Rb[2]*pz), X.center[k][1] + ((Rb[3]*px + Rb[4]*py) + Rb[5]*pz),
                         X.center[k][2] + ((Rb[6]*px + Rb[7]*py) + Rb[8]*pz) };
  double rc[3]; mat3vec(g + Y.R + 9 * l, lp, rc);
  for (int c = 0; c < 3; c++) v[c] = g[Y.x + 3 * l + c] + rc[c];
}
// BoxPrimitive::calc_signed_dist -> PlanePrimitive (PlanePrimitive.cpp:338-376): the lowest vertex's plane-frame height, the first vertex wins
// ties; pa = that vertex, pp = it in the plane frame
MH_DEV double box_dist(const Model& M, const Lay& Y, const double* g, int k, double pa[3], double pp[3]) {
  double mn = A_INF_;
  for (int i = 0; i < 8; i++) {
    double v[3], q[3]; box_vertex(M, Y, g, k, i, v); to_plane(M.m, v, q);
    if (q[1] < mn) { mn = q[1]; for (int c = 0; c < 3; c++) { pa[c] = v[c]; pp[c] = q[c]; } }
  }
  return mn;
}
// CollisionGeometry::get_farthest_point_distance (CollisionGeometry.cpp:52-68): BoxPrimitive's bounding radius (the FULL diagonal) + the
// centre's offset from the link COM
MH_DEV double rmax_box(const Model& M, int k) {
  const Boxes& X = M.bx; const int l = X.link[k];
  const double d[3] = { X.center[k][0] - M.m.com[l][0], X.center[k][1] - M.m.com[l][1], X.center[k][2] - M.m.com[l][2] };
  const double x = X.len[k][0], y = X.len[k][1], z = X.len[k][2];
  return sqrt((x*x + y*y) + z*z) + sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
}
// CompGeom::rel_equal / collinear (CompGeom.cpp:1923-1931, CompGeom.h:110)
MH_DEV bool rel_equal_(double x, double y) {
  const double ax = fabs(x), ay = fabs(y);
  const double m1 = (ay < 1.0) ? 1.0 : ay, mm = (ax < m1) ? m1 : ax;
  return fabs(x - y) <= NEAR_ZERO_ * mm;
}
MH_DEV bool collinear_(const double* a, const double* b, const double* c) {
  return rel_equal_((c[2]-a[2])*(b[1]-a[1]), (b[2]-a[2])*(c[1]-a[1])) && rel_equal_((b[2]-a[2])*(c[0]-a[0]), (b[0]-a[0])*(c[2]-a[2])) &&
         rel_equal_((b[0]-a[0])*(c[1]-a[1]), (b[1]-a[1])*(c[0]-a[0]));
}
// box k against the plane: CCD::calc_CA_Euler_step_generic (CCD.cpp:169-235) -> calc_next_CA_Euler_step_generic (:238-405, the rest rule :285-323)
// -> calc_next_CA_Euler_step_polyhedron_plane (:405-468); uniform
MH_DEV double CA_box(const Model& M, const Lay& Y, const LayC& Z, const double* g, int k) {
  const mh_artic_model& m = M.m;
  const int link = M.bx.link[k];
  double pa[3], pp[3];
  const double dist = box_dist(M, Y, g, k, pa, pp);
  double n[3]; plane_n(m, n);
  const double* V6 = g + Z.V + 6 * link;
  if (dist <= 0.0) {
    int cnt = 0; double c0[3], c1[3], c2[3];
    bool approach = false;
    for (int i = 0; i < 8; i++) {                                    // find_contacts(NEAR_ZERO): the vertices within it, in order
      double v[3], q[3]; box_vertex(M, Y, g, k, i, v); to_plane(m, v, q);
      if (!(q[1] <= NEAR_ZERO_)) continue;
      if (point_vel_dir(V6, v, n) < -NEAR_ZERO_) approach = true;
      double* dst = (cnt == 0) ? c0 : ((cnt == 1) ? c1 : c2);
      if (cnt < 3) for (int c = 0; c < 3; c++) dst[c] = v[c];
      cnt++;
    }
    if (cnt == 0) return A_INF_;
    if (approach) return 0.0;
    if (cnt >= 3 && !collinear_(c0, c1, c2)) return A_INF_;
    // the polyhedron-plane step: normal = the plane's, offset0 = <n, first contact>; velocities at the box's pose, in box axes
    const double offset0 = dot3(n, c0);
    double Rbg[9]; mat3mul(g + Y.R + 9 * link, M.bx.R[k], Rbg);
    double cb[3]; { double rc[3]; mat3vec(g + Y.R + 9 * link, M.bx.center[k], rc); for (int c = 0; c < 3; c++) cb[c] = g[Y.x + 3 * link + c] + rc[c]; }
    auto to_box = [&](const double* v, double* o) {
      o[0] = (Rbg[0]*v[0] + Rbg[3]*v[1]) + Rbg[6]*v[2]; o[1] = (Rbg[1]*v[0] + Rbg[4]*v[1]) + Rbg[7]*v[2]; o[2] = (Rbg[2]*v[0] + Rbg[5]*v[1]) + Rbg[8]*v[2];
    };
    double nP[3]; to_box(n, nP);
    const double d0[3] = { n[0] * offset0 - cb[0], n[1] * offset0 - cb[1], n[2] * offset0 - cb[2] };
    double t[3]; to_box(d0, t);
    const double offset = dot3(nP, t);
    double wxc[3]; cross3(V6, cb, wxc);
    const double vrel[3] = { V6[3] + wxc[0], V6[4] + wxc[1], V6[5] + wxc[2] };
    double wb[3], vb[3]; to_box(V6, wb); to_box(vrel, vb);
    const double av_norm = sqrt(dot3(wb, wb));
    const double lv_dot_n = -dot3(nP, vb);
    const double hx = M.bx.len[k][0] * 0.5, hy = M.bx.len[k][1] * 0.5, hz = M.bx.len[k][2] * 0.5;
    double max_step = A_INF_;
    for (int i = 0; i < 8; i++) {
      const double vtx[3] = { (i & 4) ? -hx : hx, (i & 2) ? -hy : hy, (i & 1) ? -hz : hz };
      const double r = sqrt(dot3(vtx, vtx));
      const double dv = dot3(nP, vtx) - offset;
      if (dv < NEAR_ZERO_) continue;
      const double sp = lv_dot_n + av_norm * r;
      const double speed = (0.0 > sp) ? 0.0 : sp;
      const double cand = dv / speed;
      max_step = (cand < max_step) ? cand : max_step;
    }
    return max_step;
  }
  double pb[3]; from_plane(m, pp[0], 0.0, pp[2], pb);
  const double d0[3] = { pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2] };
  const double len = sqrt(dot3(d0, d0));
  const double mn0[3] = { -(d0[0] / len), -(d0[1] / len), -(d0[2] / len) };
  const double tA = calc_max_dist(m, Y, g, link, mn0, rmax_box(M, k) MH_BASE_ARG(M, link));
  double total = tA + 0.0;
  if (total < 0.0) total = 0.0;
  const double cand = dist / total;
  return (cand < A_INF_) ? cand : A_INF_;
}
#endif

#ifdef MH_ARTIC_PAIR_TU
// ---- sphere pairs between links (mh_artic_model.npairs; the model's pair block is read from M.pr).  Every lane computes the same numbers. ----
MH_DEV void sphere_centre(const mh_artic_model& m, const Lay& Y, const double* g, int s, double c[3]) {
  const int l = m.sphere_link[s];
  double rc[3]; mat3vec(g + Y.R + 9 * l, m.sphere_center[s], rc);
  for (int k = 0; k < 3; k++) c[k] = g[Y.x + 3 * l + k] + rc[k];
}
// find_contacts_sphere_sphere's distance (CCD.inl:1189-1190): d = cA - cB, dist = (|d| - rA) - rB, n = d / |d| (from b to a)
MH_DEV double pair_dist(const Model& M, const Lay& Y, const double* g, int k, double cA[3], double cB[3], double n[3]) {
  const mh_artic_model& m = M.m;
  const int a = M.pr.a[k], b = M.pr.b[k];
  sphere_centre(m, Y, g, a, cA); sphere_centre(m, Y, g, b, cB);
  const double d[3] = { cA[0] - cB[0], cA[1] - cB[1], cA[2] - cB[2] };
  const double len = sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
  for (int c = 0; c < 3; c++) n[c] = d[c] / len;
  return (len - m.sphere_radius[a]) - m.sphere_radius[b];
}
// the contact point halfway between the closest points (CCD.inl:1195-1200), or false
MH_DEV bool pair_contact(const Model& M, const Lay& Y, const double* g, int k, double TOL, double p[3], double n[3], double& dist) {
  double cA[3], cB[3];
  dist = pair_dist(M, Y, g, k, cA, cB, n);
  if (dist > TOL) return false;
  const double rA = M.m.sphere_radius[M.pr.a[k]], rB = M.m.sphere_radius[M.pr.b[k]];
  for (int c = 0; c < 3; c++) p[c] = ((cA[c] - n[c] * rA) + (cB[c] + n[c] * rB)) * 0.5;
  return true;
}
// the constraint velocity of a contact between links la and lb (lb < 0: the plane): A's point velocity along d minus B's
MH_DEV double pair_vel(const LayC& Z, const double* g, int la, int lb, const double* p, const double* d) {
#ifdef MH_ARTIC_BSP_TU
  if (la < 0) return -point_vel_dir(g + Z.V + 6 * lb, p, d);        // A is a static box: no term of its own
#endif
  double v = point_vel_dir(g + Z.V + 6 * la, p, d);
  if (lb >= 0) v = v - point_vel_dir(g + Z.V + 6 * lb, p, d);
  return v;
}
// the sphere rule of conservative advancement for pair k (CCD.cpp:138-235), the ladder CA_step walks for the plane; uniform
MH_DEV double CA_pair(const Model& M, const Lay& Y, const LayC& Z, const double* g, int k) {
  const mh_artic_model& m = M.m;
  const int sa = M.pr.a[k], sb = M.pr.b[k], la = m.sphere_link[sa], lb = m.sphere_link[sb];
  double cA[3], cB[3], n[3], p[3], nn[3], d2;
  const double dist = pair_dist(M, Y, g, k, cA, cB, n);
  if (!(dist > NEAR_ZERO_)) {
    const bool has = pair_contact(M, Y, g, k, NEAR_ZERO_, p, nn, d2);
    if (has && fabs(pair_vel(Z, g, la, lb, p, nn)) < NEAR_ZERO_ * 10) return A_INF_;
  }
  if (dist <= 0.0) {
    if (!pair_contact(M, Y, g, k, NEAR_ZERO_, p, nn, d2)) return A_INF_;
    if (pair_vel(Z, g, la, lb, p, nn) < -NEAR_ZERO_) return 0.0;
    return A_INF_;
  }
  const double mn[3] = { -n[0], -n[1], -n[2] };
  const double tA = calc_max_dist(m, Y, g, la, mn, rmax_of(m, sa), (M.anc[la] & 1u) != 0u);
  const double tB = calc_max_dist(m, Y, g, lb, n, rmax_of(m, sb), (M.anc[lb] & 1u) != 0u);
  double total = tA + tB;
  if (total < 0.0) total = 0.0;
  const double cand = dist / total;
  return (cand < A_INF_) ? cand : A_INF_;
}
// one link's share of a contact row: the wrench [dir, (p - com) x dir] about link l's COM times column j of calc_jacobian at that COM
MH_DEV double row_term(const mh_artic_model& m, const Lay& Y, const double* g, int l, int j, const double* p, const double* dir) {
  double rc[3], com[3], r[3], w[6];
  mat3vec(g + Y.R + 9 * l, m.com[l], rc);
  for (int k = 0; k < 3; k++) { com[k] = g[Y.x + 3 * l + k] + rc[k]; r[k] = p[k] - com[k]; }
  cross3(r, dir, w + 3);
  for (int k = 0; k < 3; k++) w[k] = dir[k];
  const double* Sj = g + Y.S + 6 * j;
  double acc = 0.0;
  for (int k = 0; k < 6; k++) {
    double Jk;
    if (k >= 3) Jk = Sj[k - 3];
    else { const int k1 = (k + 1) % 3, k2 = (k + 2) % 3; Jk = Sj[3 + k] + (Sj[k1] * com[k2] - Sj[k2] * com[k1]); }
    acc = acc + w[k] * Jk;
  }
  return acc;
}
// entry j of the row of a contact between links la and lb (lb < 0: the plane) at p along dir: A's term with dir plus B's with -dir, A's first;
// a joint that is an ancestor of only one link gets that term alone, of neither 0.0 (ICH:1817-1895)
MH_DEV double contact_row(const Model& M, const Lay& Y, const double* g, int la, int lb, int j, const double* p, const double* dir) {
#ifdef MH_ARTIC_BSP_TU
  const bool inA = la >= 0 && ((M.anc[la] >> j) & 1u) != 0u, inB = lb >= 0 && ((M.anc[lb] >> j) & 1u) != 0u;   // (a static box: B's term alone)
#else
  const bool inA = ((M.anc[la] >> j) & 1u) != 0u, inB = lb >= 0 && ((M.anc[lb] >> j) & 1u) != 0u;
#endif
  double val = 0.0;
  if (inA) val = row_term(M.m, Y, g, la, j, p, dir);
  if (inB) {
    const double nd[3] = { -dir[0], -dir[1], -dir[2] };
    const double tb = row_term(M.m, Y, g, lb, j, p, nd);
    val = inA ? val + tb : tb;
  }
  return val;
}
#endif

#ifdef MH_ARTIC_BSP_TU
// ---- box-sphere pairs between links and static boxes (mh_artic_model.pair_kind; M.pr.kind[k] != 0: M.pr.a[k] indexes the box list, M.pr.b[k]
// the sphere list; the box is the reference's geometry A).  Every lane computes the same numbers.  Operation order =
// tests/native/artic_boxsphere_ref.cpp. ----
// box b's pose in the model frame; a static box's is constant and read from the model
MH_DEV void box_pose(const Model& M, const Lay& Y, const double* g, int b, double Rbg[9], double cb[3]) {
  const Boxes& X = M.bx; const int l = X.link[b];
  if (l < 0) { for (int c = 0; c < 9; c++) Rbg[c] = X.R[b][c]; for (int c = 0; c < 3; c++) cb[c] = X.center[b][c]; return; }
  mat3mul(g + Y.R + 9 * l, X.R[b], Rbg);
  double rc[3]; mat3vec(g + Y.R + 9 * l, X.center[b], rc);
  for (int c = 0; c < 3; c++) cb[c] = g[Y.x + 3 * l + c] + rc[c];
}
// the sphere's centre cS (model frame), the same point c in the box's frame, the half lengths h
MH_DEV void bsp_frame(const Model& M, const Lay& Y, const double* g, int k, double Rbg[9], double cb[3], double cS[3], double c[3], double h[3]) {
  const int b = M.pr.a[k];
  box_pose(M, Y, g, b, Rbg, cb); sphere_centre(M.m, Y, g, M.pr.b[k], cS);
  const double d[3] = { cS[0] - cb[0], cS[1] - cb[1], cS[2] - cb[2] };
  c[0] = (Rbg[0]*d[0] + Rbg[3]*d[1]) + Rbg[6]*d[2]; c[1] = (Rbg[1]*d[0] + Rbg[4]*d[1]) + Rbg[7]*d[2]; c[2] = (Rbg[2]*d[0] + Rbg[5]*d[1]) + Rbg[8]*d[2];
  for (int i = 0; i < 3; i++) h[i] = M.bx.len[b][i] * 0.5;
}
// BoxPrimitive::calc_closest_points (BoxPrimitive.cpp:183-254; the QP's fixed point is the clamp) + find_contacts_box_sphere (CCD.inl:1208-1259)
MH_DEV bool bsp_contact(const Model& M, const Lay& Y, const double* g, int k, double TOL, double pt[3], double n[3], double& dist) {
  double Rbg[9], cb[3], cS[3], c[3], h[3]; bsp_frame(M, Y, g, k, Rbg, cb, cS, c, h);
  const double Rs = M.m.sphere_radius[M.pr.b[k]];
  double p[3], u[3];
  for (int i = 0; i < 3; i++) { p[i] = (c[i] < -h[i]) ? -h[i] : ((c[i] > h[i]) ? h[i] : c[i]); u[i] = p[i] - c[i]; }
  const double nrm = sqrt((u[0]*u[0] + u[1]*u[1]) + u[2]*u[2]);
  if (fabs(p[0]) < h[0] || fabs(p[1]) < h[1] || fabs(p[2]) < h[2] || nrm < Rs) {     // an OR: every face and edge region, and every penetration
    const double b1 = h[1] - fabs(p[1]), b2 = h[2] - fabs(p[2]);
    const double b12 = (b2 < b1) ? b2 : b1, b0 = h[0] - fabs(p[0]);
    const double bd = (b12 < b0) ? b12 : b0;
    const double rn = Rs - nrm;
    dist = -((rn < bd) ? rn : bd);
  } else {                                                                             // a vertex region: the sphere point goes to the surface
    const double sc = Rs / nrm;
    for (int i = 0; i < 3; i++) u[i] = u[i] * sc;
    const double e[3] = { (c[0] + u[0]) - p[0], (c[1] + u[1]) - p[1], (c[2] + u[2]) - p[2] };
    dist = sqrt((e[0]*e[0] + e[1]*e[1]) + e[2]*e[2]);
  }
  if (dist > TOL) return false;
  double ug[3], pr[3]; mat3vec(Rbg, u, ug); mat3vec(Rbg, p, pr);
  const double sg[3] = { cS[0] + ug[0], cS[1] + ug[1], cS[2] + ug[2] };
  const double ulen = sqrt((ug[0]*ug[0] + ug[1]*ug[1]) + ug[2]*ug[2]);
  bool own = false;
  if (dist > 0.0) {
    const double pg[3] = { cb[0] + pr[0], cb[1] + pr[1], cb[2] + pr[2] };
    const double nd[3] = { pg[0] - sg[0], pg[1] - sg[1], pg[2] - sg[2] };
    const double nl = sqrt((nd[0]*nd[0] + nd[1]*nd[1]) + nd[2]*nd[2]);
    for (int i = 0; i < 3; i++) pt[i] = (sg[i] + pg[i]) * 0.5;
    if (nl > NEAR_ZERO_) { for (int i = 0; i < 3; i++) n[i] = nd[i] / nl; own = true; }
  } else for (int i = 0; i < 3; i++) pt[i] = sg[i];
  if (!own) for (int i = 0; i < 3; i++) n[i] = ug[i] / ulen;      // (a centre inside the box: 0 / 0, as in the reference)
  return true;
}
// BoxPrimitive::calc_signed_dist for a sphere (BoxPrimitive.cpp:256-276, 788-836): pA the box point, pB the sphere point, model frame
MH_DEV double bsp_sdist(const Model& M, const Lay& Y, const double* g, int k, double pA[3], double pB[3]) {
  double Rbg[9], cb[3], cS[3], c[3], h[3]; bsp_frame(M, Y, g, k, Rbg, cb, cS, c, h);
  const double Rs = M.m.sphere_radius[M.pr.b[k]];
  double cl[3] = { c[0], c[1], c[2] };
  bool inside = true; double sq = 0.0, in = -A_INF_;
  for (int i = 0; i < 3; i++) {
    if (c[i] < -h[i]) { const double dl = c[i] + h[i]; cl[i] = -h[i]; sq = sq + dl * dl; inside = false; }
    else if (c[i] > h[i]) { const double dl = c[i] - h[i]; cl[i] = h[i]; sq = sq + dl * dl; inside = false; }
    else if (inside) { const double f1 = fabs(h[i] - c[i]), f2 = fabs(c[i] + h[i]); const double dd = -((f2 < f1) ? f2 : f1); in = (in < dd) ? dd : in; }
  }
  const double dist = (inside ? in : sqrt(sq)) - Rs;
  const double v[3] = { cl[0] - c[0], cl[1] - c[1], cl[2] - c[2] };
  const double vn = sqrt((v[0]*v[0] + v[1]*v[1]) + v[2]*v[2]);
  double pr[3]; mat3vec(Rbg, cl, pr);
  for (int i = 0; i < 3; i++) pA[i] = cb[i] + pr[i];
  if (vn == 0.0) { for (int i = 0; i < 3; i++) pB[i] = cS[i]; }
  else {
    double vg[3]; mat3vec(Rbg, v, vg);
    const double sc = (Rs + ((0.0 < dist) ? 0.0 : dist)) / vn;
    for (int i = 0; i < 3; i++) pB[i] = cS[i] + vg[i] * sc;
  }
  return dist;
}
// pair k's signed distance, either kind
MH_DEV double any_dist(const Model& M, const Lay& Y, const double* g, int k) {
  double a[3], b[3], n[3];
  return M.pr.kind[k] ? bsp_sdist(M, Y, g, k, a, b) : pair_dist(M, Y, g, k, a, b, n);
}
// the sphere rule of conservative advancement for a box-sphere pair (CCD.cpp:138-235); a static box is a disabled body: calc_max_dist = 0 (CCD.cpp:589-590)
MH_DEV double CA_bsp(const Model& M, const Lay& Y, const LayC& Z, const double* g, int k) {
  const mh_artic_model& m = M.m;
  const int bx = M.pr.a[k], sb = M.pr.b[k], la = M.bx.link[bx], lb = m.sphere_link[sb];
  double pA[3], pB[3], p[3], nn[3], d2;
  const double dist = bsp_sdist(M, Y, g, k, pA, pB);
  if (!(dist > NEAR_ZERO_)) {
    const bool has = bsp_contact(M, Y, g, k, NEAR_ZERO_, p, nn, d2);
    if (has && fabs(pair_vel(Z, g, la, lb, p, nn)) < NEAR_ZERO_ * 10) return A_INF_;
  }
  if (dist <= 0.0) {
    if (!bsp_contact(M, Y, g, k, NEAR_ZERO_, p, nn, d2)) return A_INF_;
    if (pair_vel(Z, g, la, lb, p, nn) < -NEAR_ZERO_) return 0.0;
    return A_INF_;
  }
  const double d0[3] = { pA[0] - pB[0], pA[1] - pB[1], pA[2] - pB[2] };
  const double len = sqrt((d0[0]*d0[0] + d0[1]*d0[1]) + d0[2]*d0[2]);
  const double n[3] = { d0[0] / len, d0[1] / len, d0[2] / len };
  const double mn[3] = { -n[0], -n[1], -n[2] };
  const double tA = (la >= 0) ? calc_max_dist(m, Y, g, la, mn, rmax_box(M, bx), (M.anc[la] & 1u) != 0u) : 0.0;
  const double tB = calc_max_dist(m, Y, g, lb, n, rmax_of(m, sb), (M.anc[lb] & 1u) != 0u);
  double total = tA + tB;
  if (total < 0.0) total = 0.0;
  const double cand = dist / total;
  return (cand < A_INF_) ? cand : A_INF_;
}
#endif

// lane 0, LDS: dpotf2('L') / dpotrs of linalg.hpp (chol_factor, chol_solve), column-major with leading dimension ld
MH_DEV bool chol_factor_s(int n, double* A, int ld) {
  for (int j = 0; j < n; j++) {
    double ajj = A[j + ld * j];
    for (int k = 0; k < j; k++) ajj = ajj - A[j + ld * k] * A[j + ld * k];
    if (!(ajj > 0.0)) return false;
    ajj = sqrt(ajj);
    A[j + ld * j] = ajj;
    for (int i = j + 1; i < n; i++) {
      double s = A[i + ld * j];
      for (int k = 0; k < j; k++) s = s - A[i + ld * k] * A[j + ld * k];
      A[i + ld * j] = s / ajj;
    }
  }
  return true;
}
MH_DEV void chol_solve_s(int n, const double* L, int ld, double* b) {
  for (int k = 0; k < n; k++) {
    b[k] = b[k] / L[k + ld * k];
    const double bk = b[k];
    for (int i = k + 1; i < n; i++) b[i] = b[i] - bk * L[i + ld * k];
  }
  for (int k = n - 1; k >= 0; k--) {
    double s = b[k];
    for (int i = k + 1; i < n; i++) s = s - L[i + ld * k] * b[i];
    b[k] = s / L[k + ld * k];
  }
}

// G block (a, b), a <= b, of contact rows i, j: order 00 01 02 11 12 22
MH_DEV int gblk(int a, int b) { return (a == 0) ? b : ((a == 1) ? 2 + b : 5); }

// calc_impacting_unilateral_constraint_forces -> process_constraints -> apply_no_slip_model_to_connected_constraints for the nc
// contacts stored in Z.cp / ints[I_LINK..] plus the limits of the current q (oracle Artic::handle_impacts)
MH_DEV void handle_impacts(const Model& M, const Lay& Y, const LayC& Z, double* g, double* ws, mh_world_aux* aux, WaveRand& rng, int nc, int& status,
                           unsigned long long& solves, unsigned long long& rows, unsigned long long& pivs, unsigned long long& bytes)
{
  const mh_artic_model& m = M.m;
  const int nj = Y.nj, lane = lane_id();
  int* ints = reinterpret_cast<int*>(g + Z.ints);
  const double qi0 = (lane < nj) ? g[Y.q + lane] : 0.0;
  const bool up = lane < nj && qi0 >= m.hilimit[lane], lo = lane < nj && qi0 <= m.lolimit[lane];
  const uint64_t mu = ballot(up), ml = ballot(lo);
  const int nl = popc(mu) + popc(ml);
  if (nc + nl == 0) return;
  link_velocities(M, Y, Z, g);
  const double qdi = (lane < nj) ? g[Y.qd + lane] : 0.0;
  bool imp_c = false;
#ifdef MH_ARTIC_PAIR_TU
  for (int i = lane; i < nc; i += 64) imp_c = imp_c || pair_vel(Z, g, ints[I_LINK + i], ints[I_LINKB + i], g + Z.cp + 12 * i, g + Z.cp + 12 * i + 3) < -NEAR_ZERO_;
#elif defined(MH_ARTIC_BOX_TU)
  for (int i = lane; i < nc; i += 64) imp_c = imp_c || point_vel_dir(g + Z.V + 6 * ints[I_LINK + i], g + Z.cp + 12 * i, g + Z.cp + 12 * i + 3) < -NEAR_ZERO_;
#else
  if (lane < nc) imp_c = point_vel_dir(g + Z.V + 6 * ints[I_LINK + lane], g + Z.cp + 12 * lane, g + Z.cp + 12 * lane + 3) < -NEAR_ZERO_;
#endif
  const bool impacting = ballot(imp_c || (up && -qdi < -NEAR_ZERO_) || (lo && qdi < -NEAR_ZERO_)) != 0ull;   // CSim:313-323
  if (!impacting) return;
  // ICH:123-146: the no-slip model when every CONTACT has mu_coulomb >= 100 (an island of limits alone takes it too), else the
  // Drumwright-Shell QP -> LCP over [cn cs ct ncs nct l] (ICH-QP:94-497)
  const bool noslip = (nc == 0) || (m.cp_mu_coulomb >= 1e2);
  const int n = nc + nl;
  const int kh = ((m.cp_nk > 0) ? m.cp_nk : 4) / 2;
  const int nvars = 5 * nc + nl, N = nvars + nc + nl + nc * kh;
  if (noslip ? (n > NR) : (N > MH_LCP_MAX_N_WAVE || nl > NR)) { status |= MH_WORLD_UNSUPPORTED; return; }   // the limit tables (idx, Lv, l, C X L') hold NR limits
  if (m.algorithm == MH_ARTIC_FSAB) { wave_sync(); if (!dynamics(M, Y, g, nullptr)) { status |= MH_WORLD_LCP_FAILED; return; } }
  if (lane < nj) {
    const int base = popc(mu & lanes_below(lane)) + popc(ml & lanes_below(lane));
    if (up) ints[I_IDX + base] = lane | 256;
    if (lo) ints[I_IDX + base + (up ? 1 : 0)] = lane;
  }
  wave_sync();
  inverse_from_factor(Y, g);                                     // compute_X (ICH:1607)
  const double* X = g + Y.X;
  const int* idx = ints + I_IDX;
  // contact rows: wrench [d, r x d] about the link's COM times calc_jacobian at the COM; lane = (direction, contact, joint)
  double* C = g + Z.C; double* XC = g + Z.XC;
  for (int e = lane; e < 3 * nc * nj; e += 64) {
    const int d = e / (nc * nj), i = (e - d * nc * nj) / nj, j = e - d * nc * nj - i * nj;
    const int l = ints[I_LINK + i];
    double val = 0.0;
#ifdef MH_ARTIC_PAIR_TU
    val = contact_row(M, Y, g, l, ints[I_LINKB + i], j, g + Z.cp + 12 * i, g + Z.cp + 12 * i + 3 + 3 * d);
#else
    if ((M.anc[l] >> j) & 1u) {
      double rc[3], com[3], r[3], w[6];
      mat3vec(g + Y.R + 9 * l, m.com[l], rc);
      const double* p = g + Z.cp + 12 * i; const double* dir = p + 3 + 3 * d;
      for (int k = 0; k < 3; k++) { com[k] = g[Y.x + 3 * l + k] + rc[k]; r[k] = p[k] - com[k]; }
      cross3(r, dir, w + 3);
      for (int k = 0; k < 3; k++) w[k] = dir[k];
      const double* Sj = g + Y.S + 6 * j;
      double acc = 0.0;
      for (int k = 0; k < 6; k++) {
        double Jk;
        if (k >= 3) Jk = Sj[k - 3];
        else { const int k1 = (k + 1) % 3, k2 = (k + 2) % 3; Jk = Sj[3 + k] + (Sj[k1] * com[k2] - Sj[k2] * com[k1]); }
        acc = acc + w[k] * Jk;
      }
      val = acc;
    }
#endif
    C[e] = val;
  }
  wave_sync();
  for (int e = lane; e < 3 * nc * nj; e += 64) {                  // XC[d][i][c] = C[d][i][:] X[:, c]
    const int di = e / nj, c = e - di * nj;
    double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[di * nj + k] * X[k * nj + c];
    XC[e] = acc;
  }
  wave_sync();
#ifdef MH_ARTIC_PAIR_TU
  if (Z.G < 0 && !ws) { status |= MH_WORLD_UNSUPPORTED; return; }   // (the host allocates the workspace for every pair batch)
  double* G = (Z.G < 0) ? ws + WS_PAIR_G : g + Z.G;
  double* CL = g + Z.CL; double* Cv = g + Z.Cv; double* Lv = g + Z.Lv;
#else
  double* G = g + Z.G; double* CL = g + Z.CL; double* Cv = g + Z.Cv; double* Lv = g + Z.Lv;
#endif
  for (int e = lane; e < 6 * nc * nc; e += 64) {                  // the cross blocks (ICH:2127-2147)
    const int blk = e / (nc * nc), ij = e - blk * nc * nc, i = ij / nc, j = ij - i * nc;
    const int a = (blk < 3) ? 0 : ((blk < 5) ? 1 : 2), b = (blk < 3) ? blk : ((blk < 5) ? blk - 2 : 2);
    double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[(a * nc + i) * nj + k] * XC[(b * nc + j) * nj + k];
    G[blk * NS * NS + i * nc + j] = acc;
  }
  for (int e = lane; e < 3 * nc * nl; e += 64) {                  // Cd X L' without the limits' signs (ICH:1755-1762, 2130-2145)
    const int di = e / nl, k2 = e - di * nl;
    const int ik = idx[k2] & 255;
    double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[di * nj + k] * X[ik * nj + k];
    CL[(di / nc) * NS * NR + (di % nc) * nl + k2] = acc;
  }
  for (int e = lane; e < 3 * nc; e += 64) {
    double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[e * nj + k] * g[Y.qd + k];
    Cv[(e / nc) * NS + (e % nc)] = acc;
  }
  // L X L'(a, b) = X(idx_a, idx_b) (compute_limit_components, ICH:1764-1772; X is mirrored exactly, so either triangle): read in place
  if (lane < nl) { double v = g[Y.qd + (idx[lane] & 255)]; if (idx[lane] & 256) v = -v; Lv[lane] = v; }
  wave_sync();
  double* imp = g + Z.imp; double* ll = g + Z.l;
  auto solve_noslip = [&]() -> bool {
  // apply_no_slip_model (ICH:1009-1417): the greedy tangent set, Y, Q X X', the Schur complement -- lane 0, out of LDS
  double* Yy = g + Z.Yy; double* QX = g + Z.QX; double* W = g + Z.W; double* MM = g + Z.MM; double* qq = g + Z.qq;
  double* YXv = g + Z.YXv; double* t2 = g + Z.t2;
  int okflag = 1;
  if (lane == 0) {
    int* Sx = ints + I_SX; int* Tx = ints + I_TX;
    int ns = 0, nt = 0;
    auto build_Y = [&](bool skew) -> int {
      const int mm = ns + nt;
      for (int a = 0; a < ns; a++) for (int b = 0; b < ns; b++) Yy[a + mm * b] = G[gblk(1, 1) * NS * NS + Sx[a] * nc + Sx[b]];
      for (int a = 0; a < nt; a++) for (int b = 0; b < nt; b++) Yy[(ns + a) + mm * (ns + b)] = G[gblk(2, 2) * NS * NS + Tx[a] * nc + Tx[b]];
      for (int a = 0; a < ns; a++) for (int b = 0; b < nt; b++) { const double gv = G[gblk(1, 2) * NS * NS + Sx[a] * nc + Tx[b]]; Yy[a + mm * (ns + b)] = gv; Yy[(ns + b) + mm * a] = gv; }
      if (skew) for (int j = 0; j < mm; j++) Yy[j + mm * j] = Yy[j + mm * j] - NEAR_ZERO_;
      return mm;
    };
    for (int i = 0; i < nc; i++) {                                // ICH:1087-1145
      Sx[ns++] = i; int mm = build_Y(true); if (!chol_factor_s(mm, Yy, mm)) ns--;
      Tx[nt++] = i; mm = build_Y(true);     if (!chol_factor_s(mm, Yy, mm)) nt--;
    }
    ints[I_NS] = ns; ints[I_NT] = nt;
    const int mm = build_Y(false);
    if (mm > 0 && !chol_factor_s(mm, Yy, mm)) okflag = 0;        // assert(success)
    if (okflag) {
      for (int i = 0; i < nc; i++) {
        for (int a = 0; a < ns; a++) QX[i * mm + a] = G[gblk(0, 1) * NS * NS + i * nc + Sx[a]];
        for (int a = 0; a < nt; a++) QX[i * mm + ns + a] = G[gblk(0, 2) * NS * NS + i * nc + Tx[a]];
      }
      for (int k = 0; k < nl; k++) {
        for (int a = 0; a < ns; a++) QX[(nc + k) * mm + a] = CL[1 * NS * NR + Sx[a] * nl + k];
        for (int a = 0; a < nt; a++) QX[(nc + k) * mm + ns + a] = CL[2 * NS * NR + Tx[a] * nl + k];
      }
      for (int j = 0; j < n; j++) {                               // W = Y^-1 (Q X X')' (ICH:1210-1211); t2 as the column buffer
        for (int a = 0; a < mm; a++) t2[a] = QX[j * mm + a];
        if (mm > 0) chol_solve_s(mm, Yy, mm, t2);
        for (int a = 0; a < mm; a++) W[a + mm * j] = t2[a];
      }
      for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {   // MM = Q inv(M) Q' - QX W (ICH:1190-1215)
        double acc = 0.0; for (int a = 0; a < mm; a++) acc = acc + QX[i * mm + a] * W[a + mm * j];
        double qmq;
        if (i < nc && j < nc) qmq = G[i * nc + j];
        else if (i < nc) qmq = CL[i * nl + (j - nc)];
        else if (j < nc) qmq = CL[j * nl + (i - nc)];
        else qmq = X[(idx[i - nc] & 255) * nj + (idx[j - nc] & 255)];
        MM[i + n * j] = qmq - acc;
      }
      for (int a = 0; a < ns; a++) YXv[a] = Cv[1 * NS + Sx[a]];
      for (int a = 0; a < nt; a++) YXv[ns + a] = Cv[2 * NS + Tx[a]];
      if (mm > 0) chol_solve_s(mm, Yy, mm, YXv);
      for (int i = 0; i < n; i++) {                               // qq = [Cn v; L v] - QX Y^-1 X v (ICH:1217-1236)
        double acc = 0.0; for (int a = 0; a < mm; a++) acc = acc + QX[i * mm + a] * YXv[a];
        qq[i] = ((i < nc) ? Cv[i] : Lv[i - nc]) - acc;
      }
    }
  }
  wave_sync();
  okflag = uni(okflag);
  if (!okflag) { status |= MH_WORLD_LCP_FAILED; return false; }
  const int ns = ints[I_NS], nt = ints[I_NT], mm = ns + nt;
  // lcp_fast on the persistent _v, then the Lemke ladder (ICH:1239, 1281)
  const bool valid = lane < n;
  double nrm0 = 0.0;
  for (int e = lane; e < n * n; e += 64) { const double a = fabs(MM[e]); nrm0 = (a > nrm0) ? a : nrm0; }
  nrm0 = wave_max(nrm0);
  const double dii = valid ? MM[lane + n * lane] : 0.0;
  const double qi = valid ? qq[lane] : 0.0;
  int zsize = uni(aux->vns_size);
  double zi = (valid && zsize == n) ? aux->vns[lane] : 0.0;
  DenseLds Md; Md.M = MM; Md.n = n;
  LuScratch S; S.small = g + Z.A; S.ka = n; S.big = g + Z.A;
  Trace tr; tr.buf = nullptr; tr.cap = 0; tr.len = 0;
  LcpParams P; P.kind = MH_LCP_FAST; P.min_exp = -20; P.step_exp = 1u; P.max_exp = 1; P.piv_tol = -1.0; P.zero_tol = -1.0;
  unsigned piv = 0, total = 0;
  bool ok = lcp_solve_wave(P, c_pow10a, n, Md, S, g + Z.art, nrm0, dii, qi, zi, zsize, rng, piv, tr);
  total += piv;
  if (!ok) {
    P.kind = MH_LCP_LEMKE_REG;
    ok = lcp_solve_wave(P, c_pow10a, n, Md, S, g + Z.art, nrm0, dii, qi, zi, zsize, rng, piv, tr);
    total += piv;
  }
  solves += 1ull; rows += (unsigned long long)n; pivs += total; bytes += 8ull * ((unsigned long long)n * n + 2ull * n);
  if (!ok) { status |= MH_WORLD_LCP_FAILED; return false; }
  if (valid) aux->vns[lane] = zi;
  if (lane == 0) aux->vns_size = n;
  // impulses: cn = z[:nc], l = z[nc:], [cs; ct] = -(Y^-1 X v + Y^-1 (QX)' z) (ICH:1293-1308)
  if (valid) qq[lane] = zi;                                       // z, read by lane 0 below (qq is dead)
  wave_sync();
  if (lane == 0) {
    const int* Sx = ints + I_SX; const int* Tx = ints + I_TX;
    for (int a = 0; a < mm; a++) { double acc = 0.0; for (int i = 0; i < n; i++) acc = acc + QX[i * mm + a] * qq[i]; t2[a] = acc; }
    if (mm > 0) chol_solve_s(mm, Yy, mm, t2);
    for (int i = 0; i < nc; i++) { imp[i] = qq[i]; imp[NS + i] = 0.0; imp[2 * NS + i] = 0.0; }
    for (int k = 0; k < nl; k++) ll[k] = qq[nc + k];
    for (int a = 0; a < ns; a++) imp[NS + Sx[a]] = -(YXv[a] + t2[a]);
    for (int a = 0; a < nt; a++) imp[2 * NS + Tx[a]] = -(YXv[ns + a] + t2[ns + a]);
  }
  wave_sync();
  return true;
  };
  // dv = X_CnT cn + X_CsT cs + X_CtT ct + X_LT sl (ICH:1365-1373, 345-352); update_constraint_velocities_from_impulses (ICH:427-464)
  auto apply = [&]() {
    if (lane < nj) {
      double dv = 0.0;
      for (int d = 0; d < 3; d++) {
        double acc = 0.0; for (int i = 0; i < nc; i++) acc = acc + XC[(d * nc + i) * nj + lane] * imp[d * NS + i];
        dv = (d == 0) ? acc : dv + acc;
      }
      double acc = 0.0;
      for (int k = 0; k < nl; k++) { const int c = idx[k]; const double ls = (c & 256) ? -ll[k] : ll[k]; acc = acc + ls * X[(c & 255) * nj + lane]; }
      dv = dv + acc;
      g[Y.qd + lane] = g[Y.qd + lane] + dv;
    }
    if (lane < 3 * nc) {                                          // Cd_v rows
      const int a = lane / nc, i = lane - a * nc;
      double cv = Cv[a * NS + i];
      for (int b = 0; b < 3; b++) {
        double acc = 0.0;
        for (int j = 0; j < nc; j++) { const double gv = (a <= b) ? G[gblk(a, b) * NS * NS + i * nc + j] : G[gblk(b, a) * NS * NS + j * nc + i]; acc = acc + gv * imp[b * NS + j]; }
        cv = cv + acc;
      }
      double acc = 0.0; for (int k = 0; k < nl; k++) acc = acc + CL[a * NS * NR + i * nl + k] * ll[k];
      cv = cv + acc;
      g[Z.W + lane] = cv;                                         // staged: W is dead
#ifdef MH_ARTIC_REPORT_TU
      g[Z.racc + a * NS + i] = g[Z.racc + a * NS + i] + imp[a * NS + i];   // contact_impulse += (cn, cs, ct) (ICH:298-327): every application adds what it applied
#endif
    }
    if (lane >= LOFF && lane < LOFF + nl) {                           // L_v rows
      const int k = lane - LOFF;
      double lv = Lv[k];
      for (int d = 0; d < 3; d++) { double acc = 0.0; for (int i = 0; i < nc; i++) acc = acc + CL[d * NS * NR + i * nl + k] * imp[d * NS + i]; lv = lv + acc; }
      double acc = 0.0; for (int k2 = 0; k2 < nl; k2++) acc = acc + X[(idx[k] & 255) * nj + (idx[k2] & 255)] * ll[k2];
      lv = lv + acc;
      g[Z.W + LOFF + k] = lv;
    }
    wave_sync();
    if (lane < 3 * nc) Cv[(lane / nc) * NS + (lane % nc)] = g[Z.W + lane];
    if (lane >= LOFF && lane < LOFF + nl) Lv[lane - LOFF] = g[Z.W + lane];
    wave_sync();
  };
  auto minv_of = [&]() -> double {                               // calc_min_constraint_velocity (ICH:413-424); uniform
    double mn = A_INF_;
    for (int i = 0; i < nc; i++) mn = (i == 0 || Cv[i] < mn) ? Cv[i] : mn;
    if (nl > 0) { double mlv = Lv[0]; for (int k = 1; k < nl; k++) mlv = (Lv[k] < mlv) ? Lv[k] : mlv; mn = (mlv < mn) ? mlv : mn; }
    return mn;
  };
  if (noslip) {
  if (!solve_noslip()) return;
  apply();
  const double minv = minv_of();
  wave_sync();
  bool ch = false;                                                // apply_restitution(q) (ICH:497-525)
  if (lane < nc) { const double v = imp[lane] * m.cp_epsilon; imp[lane] = v; ch = v > NEAR_ZERO_; }
  if (lane >= LOFF && lane < LOFF + nl) { const int k = lane - LOFF; const double v = ll[k] * m.limit_restitution[idx[k] & 255]; ll[k] = v; ch = v > NEAR_ZERO_; }
  const bool changed = ballot(ch) != 0ull;
  wave_sync();
  if (changed) {
    if (lane < nc) { imp[NS + lane] = 0.0; imp[2 * NS + lane] = 0.0; }
    wave_sync();
    apply();
    const double minv_plus = minv_of();
    if (minv_plus < 0.0 && minv_plus < minv - NEAR_ZERO_) status |= MH_WORLD_UNSUPPORTED;   // ICH:284-291 reads an unsized _z
  }
  } else {
  // ---- Drumwright-Shell: _MM = [H -M'; M 0] dense in this world's HBM workspace (N <= 64: one lane per row in the wave solver) ----
  double* WM = ws; double* WLU = ws + MH_LCP_MAX_N_WAVE * MH_LCP_MAX_N_WAVE;
  auto ds_H = [&](int r, int c) -> double {                       // H(r, c) over [cn cs ct ncs nct l] (ICH-QP:283-440)
    if (r < 5 * nc && c < 5 * nc) {
      const int a = r / nc, i = r - a * nc, b2 = c / nc, j = c - b2 * nc;
      const int da = (a == 0) ? 0 : ((a == 1 || a == 3) ? 1 : 2), db = (b2 == 0) ? 0 : ((b2 == 1 || b2 == 3) ? 1 : 2);
      double gv = (da <= db) ? G[gblk(da, db) * NS * NS + i * nc + j] : G[gblk(db, da) * NS * NS + j * nc + i];
      if ((a >= 3) != (b2 >= 3)) gv = -gv;
      if (r == c && r < nc) gv = gv + m.cp_compliance;
      return gv;
    }
    if (r < 5 * nc || c < 5 * nc) {
      const int rr = (r < 5 * nc) ? r : c, k = ((r < 5 * nc) ? c : r) - 5 * nc;
      const int a = rr / nc, i = rr - a * nc, da = (a == 0) ? 0 : ((a == 1 || a == 3) ? 1 : 2);
      double gv = CL[da * NS * NR + i * nl + k];
      if (a >= 3) gv = -gv;
      return gv;
    }
    return X[(idx[r - 5 * nc] & 255) * nj + (idx[c - 5 * nc] & 255)];
  };
  auto ds_M = [&](int rr, int c) -> double {                      // inequality row rr: normal rows, limit rows, friction polygons
    if (rr < nc) return ds_H(rr, c);
    if (rr < nc + nl) return ds_H(5 * nc + (rr - nc), c);
    const int f = rr - nc - nl, i = f / kh, j = f - i * kh;
    if (c == i) return m.cp_mu_coulomb;
    if (c == nc + i || c == 3 * nc + i) return -M.fcos[j];
    if (c == 2 * nc + i || c == 4 * nc + i) return -M.fsin[j];
    return 0.0;
  };
  auto solve_qp = [&]() -> bool {                                 // solve_qp_work (ICH-QP:94-263) on the persistent _z / _zlast
    double nrm0 = 0.0;
    for (int e = lane; e < N * N; e += 64) {
      const int r = e % N, c = e / N;
      double v;
      if (c < nvars) v = (r < nvars) ? ds_H(r, c) : ds_M(r - nvars, c);
      else v = (r < nvars) ? -ds_M(c - nvars, r) : 0.0;
      WM[e] = v;
      const double a = fabs(v); nrm0 = (a > nrm0) ? a : nrm0;
    }
    nrm0 = wave_max(nrm0);
    double qi = 0.0;
    if (lane < N) {
      const int r = lane;
      if (r < 5 * nc) { const int a = r / nc, i = r - a * nc; const double v = Cv[((a == 0) ? 0 : ((a == 1 || a == 3) ? 1 : 2)) * NS + i]; qi = (a >= 3) ? -v : v; }
      else if (r < nvars) qi = Lv[r - 5 * nc];
      else if (r < nvars + nc) qi = Cv[r - nvars];
      else if (r < nvars + nc + nl) qi = Lv[r - nvars - nc];
      else { const int i = (r - nvars - nc - nl) / kh; const double cs1 = Cv[NS + i], ct1 = Cv[2 * NS + i]; const double vel = sqrt(cs1 * cs1 + ct1 * ct1); qi = m.cp_mu_viscous * vel; }
    }
    wave_sync();
    const double dii = (lane < N) ? WM[lane + N * lane] : 0.0;
    // z.resize(N) on _z's storage; warm start from _zlast when the sizes match (ICH-QP:158-162)
    const int zbuf_cap = uni(aux->zbuf_cap), zlast_size = uni(aux->zlast_size);
    double zi = (N > zbuf_cap) ? 0.0 : aux->zbuf[lane];
    if (lane >= N) zi = 0.0;
    if (N == zlast_size) zi = (lane < N) ? aux->zlast[lane] : 0.0;
    int zsize = N;
    DenseLds Md; Md.M = WM; Md.n = N;
    LuScratch S; S.small = g + Z.A; S.ka = NR; S.big = WLU;
    Trace tr; tr.buf = nullptr; tr.cap = 0; tr.len = 0;
    LcpParams P; P.piv_tol = -1.0; P.zero_tol = -1.0; P.min_exp = -20; P.kind = MH_LCP_FAST_REG; P.step_exp = 4u; P.max_exp = -8;
    unsigned piv = 0, total = 0;
    bool ok = lcp_solve_wave(P, c_pow10a, N, Md, S, g + Z.art, nrm0, dii, qi, zi, zsize, rng, piv, tr);
    total += piv;
    if (!ok) {
      zi = 0.0;                                                   // z.set_zero() keeps the size (ICH-QP:222)
      P.kind = MH_LCP_LEMKE_REG; P.step_exp = 1u; P.max_exp = 1;
      ok = lcp_solve_wave(P, c_pow10a, N, Md, S, g + Z.art, nrm0, dii, qi, zi, zsize, rng, piv, tr);
      total += piv;
    }
    solves += 1ull; rows += (unsigned long long)N; pivs += total; bytes += 8ull * ((unsigned long long)N * N + 2ull * N);
    if (!ok) { status |= MH_WORLD_LCP_FAILED; return false; }     // LCPSolverException
    wave_sync();
    if (lane < N) { aux->zlast[lane] = zi; aux->zbuf[lane] = zi; }
    if (lane == 0) { aux->zlast_size = N; if (zbuf_cap < N) aux->zbuf_cap = N; aux->zbuf_size = nvars; }
    wave_sync();
    return true;
  };
  auto from_stacked = [&]() {                                     // update_from_stacked(q, z) (UCPD:218-228)
    if (lane < nc) {
      imp[lane] = aux->zbuf[lane];
      double sv = aux->zbuf[nc + lane];     sv = sv - aux->zbuf[3 * nc + lane]; imp[NS + lane] = sv;
      double tv = aux->zbuf[2 * nc + lane]; tv = tv - aux->zbuf[4 * nc + lane]; imp[2 * NS + lane] = tv;
    }
    if (lane >= LOFF && lane < LOFF + nl) ll[lane - LOFF] = aux->zbuf[5 * nc + lane - LOFF];
    wave_sync();
  };
  if (!solve_qp()) return;
  from_stacked(); apply();
  const double minv = minv_of();
  wave_sync();
  bool ch = false;                                                // apply_restitution(q, z) (ICH:470-491): the cn and l entries of z
  if (lane < nc) { const double v = aux->zbuf[lane] * m.cp_epsilon; aux->zbuf[lane] = v; ch = v > NEAR_ZERO_; }
  if (lane >= LOFF && lane < LOFF + nl) { const int k = lane - LOFF; const double v = aux->zbuf[5 * nc + k] * m.limit_restitution[idx[k] & 255]; aux->zbuf[5 * nc + k] = v; ch = v > NEAR_ZERO_; }
  const bool changed = ballot(ch) != 0ull;
  wave_sync();
  if (changed) {
    from_stacked(); apply();                                      // the tangential impulses go in again in full, as in the reference
    const double minv_plus = minv_of();
    wave_sync();
    if (minv_plus < 0.0 && minv_plus < minv - NEAR_ZERO_) {       // ICH:591-600: second solve on the updated C v vectors
      if (!solve_qp()) return;
      from_stacked(); apply();                                     // (its C v update is not read any more)
    }
  }
  }
  link_velocities(M, Y, Z, g);                                    // ICH:157-167
  bool tol = false;
#ifdef MH_ARTIC_PAIR_TU
  if (lane < nc) tol = pair_vel(Z, g, ints[I_LINK + lane], ints[I_LINKB + lane], g + Z.cp + 12 * lane, g + Z.cp + 12 * lane + 3) < -NEAR_ZERO_;
#else
  if (lane < nc) tol = point_vel_dir(g + Z.V + 6 * ints[I_LINK + lane], g + Z.cp + 12 * lane, g + Z.cp + 12 * lane + 3) < -NEAR_ZERO_;
#endif
  if (lane >= LOFF && lane < LOFF + nl) { const int c = idx[lane - LOFF]; const double v = g[Y.qd + (c & 255)]; tol = ((c & 256) ? -v : v) < -NEAR_ZERO_; }
  if (ballot(tol) != 0ull) status |= MH_WORLD_IMPACT_TOL;
}

#ifdef MH_ARTIC_REPORT_TU
// The contact report (include/moby_hip_artic.h, "Contact report").  Folds the mini-step's contacts into the step's rows, where
// ConstraintSimulator::constraint_post_callback_fn sees them (CSim:353): after handle_impacts returned without a throw, also when it returned early
// (the contacts then count with zero impulse).  Lane k owns slot k (sphere, box or pair: at most 18) and walks the contact list in its order, so the
// order of a row's additions is fixed and no lane reads what another wrote; the rows stay in global memory.  A contact the handler has no room for
// (list index >= NS) has no accumulator and folds with zero impulse.
MH_DEV void report_fold(const Model& M, const LayC& Z, const double* g, int nc, double* rep)
{
  const int lane = lane_id();
  if (!rep || lane >= M.m.nspheres + M.bx.n + M.pr.n) return;
  const int* rslot = reinterpret_cast<const int*>(g + Z.rslot);
  const double* racc = g + Z.racc;
  double* row = rep + MH_REPORT_PAIR * lane;
  for (int c = 0; c < nc; c++) {
    if (rslot[c] != lane) continue;
    const bool has = c < NS;
    const double cn = has ? racc[c] : 0.0, cs = has ? racc[NS + c] : 0.0, ct = has ? racc[2 * NS + c] : 0.0;
    const double* p = g + Z.cp + 12 * c;
    row[0] = row[0] + 1.0;
    row[1] = row[1] + cn;
    for (int k = 0; k < 3; k++) { const double jv = (p[3 + k] * cn + p[6 + k] * cs) + p[9 + k] * ct; row[2 + k] = row[2 + k] + jv; }
    for (int k = 0; k < 3; k++) row[5 + k] = row[5 + k] + p[k] * cn;
  }
}
#endif

// TimeSteppingSimulator::do_mini_step (TSS:114-222); returns h (uniform).  MH_ARTIC_DRIVE_TU: the drive's row of step s (world b of B) is
// evaluated after the position update, before the forward dynamics (precalc_fwd_dyn, Simulator.cpp:319-350)
MH_DEV double do_mini_step(const Model& M, const Lay& Y, const LayC& Z, double* g, double* ws, mh_world_aux* aux, WaveRand& rng, double dt, bool& kin_ok, int& status,
                           unsigned long long& solves, unsigned long long& rows, unsigned long long& pivs, unsigned long long& bytes
#ifdef MH_ARTIC_DRIVE_TU
                           , const mh_artic_drive& D, int B, int b, int s
#endif
#if defined(MH_ARTIC_POSE_TU) || defined(MH_ARTIC_BOX_TU)
                           , const mh_artic_drive* Dp, int B, int b, int s
#endif
#ifdef MH_ARTIC_REPORT_TU
                           , double* rep                        // this world's rows of step s in the caller's report, or NULL
#endif
#ifdef MH_ARTIC_WRENCH_TU
                           , const mh_artic_wrench* Wp          // the link wrench (mh_artic_wr.hip), or NULL: evaluated inside the forward dynamics, after kin_inertia
#endif
                           )
{
  const mh_artic_model& m = M.m;
  const int nj = Y.nj, lane = lane_id();
  if (lane < nj) g[Z.qsave + lane] = g[Y.q + lane];
  wave_sync();
  double h = 0.0;
  unsigned long guard = 0;
  while (h < dt) {
    if (++guard > MH_CA_HARD_CAP) { status |= MH_WORLD_STALLED; break; }
    // the link frames of the current q are still in LDS from the forward dynamics of the previous mini-step (nothing since then
    // moved q; R, x, S are not touched by the composite-inertia / articulated-inertia passes): only a q this loop moved needs a new pass
    if (!kin_ok) kin_inertia(M, Y, g);
    kin_ok = false;
    link_velocities(M, Y, Z, g);
    double CA = A_INF_;
    for (int s = 0; s < m.nspheres; s++) { MH_SKIP_MASKED(M, s) const double e = CA_step(m, Y, Z, g, s MH_BASE_ARG(M, m.sphere_link[s])); CA = (e < CA) ? e : CA; }
#ifdef MH_ARTIC_BOX_TU
    for (int k = 0; k < M.bx.n; k++) { MH_SKIP_STATIC(M, k) const double e = CA_box(M, Y, Z, g, k); CA = (e < CA) ? e : CA; }
#endif
#ifdef MH_ARTIC_BSP_TU
    for (int k = 0; k < M.pr.n; k++) { const double e = M.pr.kind[k] ? CA_bsp(M, Y, Z, g, k) : CA_pair(M, Y, Z, g, k); CA = (e < CA) ? e : CA; }
#elif defined(MH_ARTIC_PAIR_TU)
    for (int k = 0; k < M.pr.n; k++) { const double e = CA_pair(M, Y, Z, g, k); CA = (e < CA) ? e : CA; }
#endif
    CA = uni(CA);
    if (CA <= 0.0) { kin_ok = true; break; }
    double tc = (m.min_step_size > CA) ? m.min_step_size : CA;
    tc = ((dt - h) < tc) ? (dt - h) : tc;
    wave_sync();
    if (lane < nj) { double qn = g[Y.qd + lane] * (h + tc); qn = qn + g[Z.qsave + lane]; g[Y.q + lane] = qn; }
    h += tc;
    wave_sync();
  }
  wave_sync();
#ifdef MH_ARTIC_DRIVE_TU
  drive_tau(D, B, b, s, Y, g);                                    // (read by the dynamics after kin_inertia's barriers)
  const bool ok = (m.algorithm == MH_ARTIC_FSAB) ? dynamics_aba(M, Y, g, g + Y.qdd) : dynamics(M, Y, g, g + Y.qdd);
#elif defined(MH_ARTIC_POSE_TU) || defined(MH_ARTIC_BOX_TU)
  if (Dp) drive_tau(*Dp, B, b, s, Y, g);
  const double* tw = Dp ? g + Y.qdd : nullptr;
#ifdef MH_ARTIC_WRENCH_TU
  const bool ok = (m.algorithm == MH_ARTIC_FSAB) ? dynamics_aba(M, Y, g, tw, Wp, B, b, s) : dynamics(M, Y, g, tw, Wp, B, b, s);
#else
  const bool ok = (m.algorithm == MH_ARTIC_FSAB) ? dynamics_aba(M, Y, g, tw) : dynamics(M, Y, g, tw);
#endif
#else
  const bool ok = (m.algorithm == MH_ARTIC_FSAB) ? dynamics_aba(M, Y, g, nullptr) : dynamics(M, Y, g, nullptr);
#endif
  kin_ok = true;                                                  // kin_inertia ran first thing in there, whatever came after
  if (!ok) { status |= MH_WORLD_LCP_FAILED; wave_sync(); return h; }   // an exception ends the run (oracle Artic::do_mini_step): nothing below happens
  if (lane < nj) g[Y.qd + lane] = g[Y.qd + lane] + g[Y.qdd + lane] * h;   // TSS:182-192
  wave_sync();
  // find_unilateral_constraints (CSim:488-537): R, x, S of the current q are in LDS (kin_inertia inside the dynamics call)
  int* ints = reinterpret_cast<int*>(g + Z.ints);
  int nc = 0;
#ifdef MH_ARTIC_REPORT_TU
  int* rslot = reinterpret_cast<int*>(g + Z.rslot);
  for (int e = lane; e < 3 * NS; e += 64) g[Z.racc + e] = 0.0;     // a new constraint list: no contact has received an impulse yet
#endif
  for (int s = 0; s < m.nspheres; s++) {
    MH_SKIP_MASKED(M, s)
    double cp[3]; sphere_in_plane(m, Y, g, s, cp);
    const double dist = cp[1] + (-1.0 * m.sphere_radius[s]);
    double p[3];
    if (dist < m.contact_dist_thresh && find_contact(m, Y, g, s, m.contact_dist_thresh, p)) {
      if (lane == 0) {
        double* c = g + Z.cp + 12 * nc;
        double n[3], sv[3], tv[3]; plane_n(m, n); orthonormal_basis(n, sv, tv);
        for (int k = 0; k < 3; k++) { c[k] = p[k]; c[3 + k] = n[k]; c[6 + k] = sv[k]; c[9 + k] = tv[k]; }
        ints[I_LINK + nc] = m.sphere_link[s];
        MH_SET_LINKB(nc, -1)
#ifdef MH_ARTIC_REPORT_TU
        rslot[nc] = s;
#endif
      }
      nc++;
    }
  }
#ifdef MH_ARTIC_BOX_TU
  for (int k = 0; k < M.bx.n; k++) {                               // find_contacts_plane_generic: a contact at every vertex within the threshold
    double pa[3], pp[3];
    MH_SKIP_STATIC(M, k)
    if (!(box_dist(M, Y, g, k, pa, pp) < m.contact_dist_thresh)) continue;
    for (int i = 0; i < 8; i++) {
      double v[3], q[3]; box_vertex(M, Y, g, k, i, v); to_plane(m, v, q);
      if (!(q[1] <= m.contact_dist_thresh)) continue;
      if (lane == 0) {
        double* c = g + Z.cp + 12 * nc;
        double n[3], sv[3], tv[3]; plane_n(m, n); orthonormal_basis(n, sv, tv);
        for (int c2 = 0; c2 < 3; c2++) { c[c2] = v[c2]; c[3 + c2] = n[c2]; c[6 + c2] = sv[c2]; c[9 + c2] = tv[c2]; }
        ints[I_LINK + nc] = M.bx.link[k];
        MH_SET_LINKB(nc, -1)
#ifdef MH_ARTIC_REPORT_TU
        rslot[nc] = m.nspheres + k;
#endif
      }
      nc++;
    }
  }
#endif
#ifdef MH_ARTIC_PAIR_TU
  for (int k = 0; k < M.pr.n; k++) {                               // find_contacts_sphere_sphere: at most one contact per pair
    double p[3], n[3], dist;
#ifdef MH_ARTIC_BSP_TU
    const bool bsp = M.pr.kind[k] != 0;                            // find_contacts_box_sphere behind the signed-distance test (pdi.dist)
    if (bsp) { if (!(any_dist(M, Y, g, k) < m.contact_dist_thresh) || !bsp_contact(M, Y, g, k, m.contact_dist_thresh, p, n, dist)) continue; }
    else
#endif
    if (!pair_contact(M, Y, g, k, m.contact_dist_thresh, p, n, dist) || !(dist < m.contact_dist_thresh)) continue;
    if (lane == 0) {
      double* c = g + Z.cp + 12 * nc;
      double sv[3], tv[3]; orthonormal_basis(n, sv, tv);
      for (int c2 = 0; c2 < 3; c2++) { c[c2] = p[c2]; c[3 + c2] = n[c2]; c[6 + c2] = sv[c2]; c[9 + c2] = tv[c2]; }
#ifdef MH_ARTIC_BSP_TU
      ints[I_LINK + nc] = bsp ? M.bx.link[M.pr.a[k]] : m.sphere_link[M.pr.a[k]];
#else
      ints[I_LINK + nc] = m.sphere_link[M.pr.a[k]];
#endif
      ints[I_LINKB + nc] = m.sphere_link[M.pr.b[k]];
#ifdef MH_ARTIC_REPORT_TU
      rslot[nc] = m.nspheres + M.bx.n + k;
#endif
    }
    nc++;
  }
#endif
  nc = uni(nc);
  wave_sync();
  handle_impacts(M, Y, Z, g, ws, aux, rng, nc, status, solves, rows, pivs, bytes);
  wave_sync();
#ifdef MH_ARTIC_REPORT_TU
  if (!(status & MH_WORLD_LCP_FAILED)) report_fold(M, Z, g, nc, rep);   // a handler that threw leaves the step's rows as the earlier mini-steps left them
#endif
  return h;
}

// ConstraintStabilization::stabilize for a body with link spheres: contact rows AND joint-limit rows (oracle Artic::stabilize; CStab:167-254,
// 257-345, 431-441, 705-904, 932-970, 1056-1216, 1322-1379).  Per iteration: one contact per (sphere, plane) pair -- the synthetic
// contact "between separated bodies" (point on the sphere, normal from it towards the plane) when the signed distance is at least
// NEAR_ZERO, the contact of find_contacts otherwise -- and a row for every finite limit; MM = [Cn X Cn'  Cn X L'; .  L X L'] in this
// world's HBM workspace, cold lcp_fast then the Lemke ladder, dv = X Cn' cn + X L' ls.  update_q's line search evaluates the sphere
// distances by a kinematics pass per trial q; the limit slacks it looks at are joint 0's (CStab:117, as stabilize_limits).
// LDS: the contact list in Z.cp, Cn / Cn X in Z.C / Z.XC, the three uC vectors in Z.W, the row table (up to 2 nj ints) in Z.QX.
__device__ __noinline__ void stabilize_contacts(const Model& M, const Lay& Y, const LayC& Z, double* g, double* ws, WaveRand& rng, int& status,
                                                unsigned long long& solves, unsigned long long& rows, unsigned long long& pivs, unsigned long long& bytes,
                                                unsigned long long& stab_iters, unsigned long long& stab_rows)
{
  const mh_artic_model& m = M.m;
  const unsigned maxit = (unsigned)m.cstab_max_iterations;
  if (maxit == 0) return;
#ifdef MH_ARTIC_BOX_TU
  if (!ws) { status |= MH_WORLD_UNSUPPORTED; return; }              // (the host allocates it for every stabilising batch)
#endif
#ifdef MH_ARTIC_BOX_TU
  // the boxes' distances follow the spheres' in uC; up to NCL contacts: their distances and Cn / Cn X live in the HBM workspace behind the LCP
#ifdef MH_ARTIC_PAIR_TU
  // ... and the pairs' follow the boxes'; a sphere masked off the plane has no entry
#ifdef MH_ARTIC_BSP_TU
  const int nj = Y.nj, lane = lane_id(), nsph = m.nspheres, ngeo = (nsph - popc((uint64_t)(unsigned)M.pr.no_plane)) + (M.bx.n - M.pr.nstatic) + M.pr.n;   // (a static box has no entry)
#else
  const int nj = Y.nj, lane = lane_id(), nsph = m.nspheres, ngeo = (nsph - popc((uint64_t)(unsigned)M.pr.no_plane)) + M.bx.n + M.pr.n;
#endif
#else
  const int nj = Y.nj, lane = lane_id(), nsph = m.nspheres, ngeo = nsph + M.bx.n;
#endif
  const int nu = ngeo + 2 * nj;
  double* uO = g + Z.W; double* uN = uO + USTRIDE; double* uT = uN + USTRIDE;   // (nu <= 12 + 32, with pairs 18 + 32)
  int* idx = reinterpret_cast<int*>(g + Z.QX);
  int* ints = reinterpret_cast<int*>(g + Z.ints);
  double* dist = ws + WS_DIST;
#else
  const int nj = Y.nj, lane = lane_id(), nsph = m.nspheres;
  const int nu = nsph + 2 * nj;                                    // entries of uC: the pairwise distances, then joint 0's two slacks nj times
  double* uO = g + Z.W; double* uN = uO + 40; double* uT = uN + 40;   // uC at q, at q + dq, at the trial q (nu <= 4 + 32)
  int* idx = reinterpret_cast<int*>(g + Z.QX);                    // idx[k] = joint | (upper << 8), a row for every finite limit
  int* ints = reinterpret_cast<int*>(g + Z.ints);
  double* dist = g + Z.Cv;                                         // the contacts' signed distances
#endif
  const double hi0 = m.hilimit[0], lo0 = m.lolimit[0];
  // evaluate_unilateral_constraints at the q in LDS into `out`; returns the most negative entry (uniform)
  auto eval = [&](double* out) -> double {
    wave_sync();
    kin_inertia(M, Y, g);
    double vio = A_INF_;
#ifdef MH_ARTIC_PAIR_TU
    int o = 0;
    for (int s2 = 0; s2 < nsph; s2++) { MH_SKIP_MASKED(M, s2) double cp[3]; sphere_in_plane(m, Y, g, s2, cp); const double d = cp[1] + (-1.0 * m.sphere_radius[s2]); if (lane == 0) out[o] = d; o++; vio = (d < vio) ? d : vio; }
    for (int k = 0; k < M.bx.n; k++) { MH_SKIP_STATIC(M, k) double pa[3], pp[3]; const double d = box_dist(M, Y, g, k, pa, pp); if (lane == 0) out[o] = d; o++; vio = (d < vio) ? d : vio; }
#ifdef MH_ARTIC_BSP_TU
    for (int k = 0; k < M.pr.n; k++) { const double d = any_dist(M, Y, g, k); if (lane == 0) out[o] = d; o++; vio = (d < vio) ? d : vio; }
#else
    for (int k = 0; k < M.pr.n; k++) { double cA[3], cB[3], n[3]; const double d = pair_dist(M, Y, g, k, cA, cB, n); if (lane == 0) out[o] = d; o++; vio = (d < vio) ? d : vio; }
#endif
    const double q0 = g[Y.q];
    const double a = (hi0 - q0) - 0.0, b2 = (q0 + 0.0) - lo0;
    if (lane < nj) { out[ngeo + 2 * lane] = a; out[ngeo + 2 * lane + 1] = b2; }
#elif defined(MH_ARTIC_BOX_TU)
    for (int s2 = 0; s2 < nsph; s2++) { double cp[3]; sphere_in_plane(m, Y, g, s2, cp); const double d = cp[1] + (-1.0 * m.sphere_radius[s2]); if (lane == 0) out[s2] = d; vio = (d < vio) ? d : vio; }
    for (int k = 0; k < M.bx.n; k++) { double pa[3], pp[3]; const double d = box_dist(M, Y, g, k, pa, pp); if (lane == 0) out[nsph + k] = d; vio = (d < vio) ? d : vio; }
    const double q0 = g[Y.q];
    const double a = (hi0 - q0) - 0.0, b2 = (q0 + 0.0) - lo0;
    if (lane < nj) { out[ngeo + 2 * lane] = a; out[ngeo + 2 * lane + 1] = b2; }
#else
    for (int s2 = 0; s2 < nsph; s2++) { double cp[3]; sphere_in_plane(m, Y, g, s2, cp); const double d = cp[1] + (-1.0 * m.sphere_radius[s2]); if (lane == 0) out[s2] = d; vio = (d < vio) ? d : vio; }
    const double q0 = g[Y.q];
    const double a = (hi0 - q0) - 0.0, b2 = (q0 + 0.0) - lo0;
    if (lane < nj) { out[nsph + 2 * lane] = a; out[nsph + 2 * lane + 1] = b2; }
#endif
    vio = (a < vio) ? a : vio; vio = (b2 < vio) ? b2 : vio;
    wave_sync();
    return uni(vio);
  };
  const double qd_save = (lane < nj) ? g[Y.qd + lane] : 0.0;
  double qv = (lane < nj) ? g[Y.q + lane] : 0.0;                   // the stabiliser's q (CStab:183)
  double max_uvio = eval(uO);
  unsigned iterations = 0;
  const bool hfin = lane < nj && m.hilimit[lane] < A_INF_, lfin = lane < nj && m.lolimit[lane] > -A_INF_;
  const uint64_t mu = ballot(hfin), ml = ballot(lfin);
  const int nl = popc(mu) + popc(ml);
  double* WM = ws; double* WLU = ws + MH_LCP_MAX_N_WAVE * MH_LCP_MAX_N_WAVE;
  while (max_uvio < m.cstab_eps) {
    if (iterations == maxit) break;
    if (iterations == MH_CSTAB_HARD_CAP) { status |= MH_WORLD_STALLED; break; }
    wave_sync();
    if (lane < nj) g[Y.qd + lane] = 0.0;
    double dq = 0.0;
    wave_sync();
    // the contact list (the link frames of the current q are in LDS: eval ran at it)
    int nc = 0;
    for (int s2 = 0; s2 < nsph; s2++) {
      MH_SKIP_MASKED(M, s2)
      double cp[3]; sphere_in_plane(m, Y, g, s2, cp);
      const double low = cp[1] + (-1.0 * m.sphere_radius[s2]);
      double p[3], nn[3];
      bool have = true;
      if (low >= NEAR_ZERO_) {
        double on_plane[3]; from_plane(m, cp[0], 0.0, cp[2], on_plane); from_plane(m, cp[0], low, cp[2], p);
        const double d[3] = { on_plane[0] - p[0], on_plane[1] - p[1], on_plane[2] - p[2] };
        const double len = sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
        for (int k = 0; k < 3; k++) nn[k] = d[k] / len;
      } else { have = find_contact(m, Y, g, s2, NEAR_ZERO_, p); plane_n(m, nn); }
      if (have) {
        if (lane == 0) { double* c = g + Z.cp + 12 * nc; for (int k = 0; k < 3; k++) { c[k] = p[k]; c[3 + k] = nn[k]; } ints[I_LINK + nc] = m.sphere_link[s2]; MH_SET_LINKB(nc, -1) dist[nc] = low; }
        nc++;
      }
    }
#ifdef MH_ARTIC_BOX_TU
    for (int k = 0; k < M.bx.n; k++) {                             // CStab:306-345 for (box, plane): one synthetic contact, or the vertices within NEAR_ZERO
      double pa[3], pp[3];
      MH_SKIP_STATIC(M, k)
      const double low = box_dist(M, Y, g, k, pa, pp);
      if (low >= NEAR_ZERO_) {
        double pb[3]; from_plane(m, pp[0], 0.0, pp[2], pb);
        const double d[3] = { pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2] };
        const double len = sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
        if (lane == 0) { double* c = g + Z.cp + 12 * nc; for (int c2 = 0; c2 < 3; c2++) { c[c2] = pa[c2]; c[3 + c2] = d[c2] / len; } ints[I_LINK + nc] = M.bx.link[k]; MH_SET_LINKB(nc, -1) dist[nc] = low; }
        nc++;
      } else {
        for (int i = 0; i < 8; i++) {
          double v[3], q[3]; box_vertex(M, Y, g, k, i, v); to_plane(m, v, q);
          if (!(q[1] <= NEAR_ZERO_)) continue;
          if (lane == 0) { double* c = g + Z.cp + 12 * nc; double nn[3]; plane_n(m, nn); for (int c2 = 0; c2 < 3; c2++) { c[c2] = v[c2]; c[3 + c2] = nn[c2]; } ints[I_LINK + nc] = M.bx.link[k]; MH_SET_LINKB(nc, -1) dist[nc] = q[1]; }
          nc++;
        }
      }
    }
#endif
#ifdef MH_ARTIC_PAIR_TU
    for (int k = 0; k < M.pr.n; k++) {                             // CStab:306-345 for a sphere pair: the synthetic contact on A's surface, or find_contacts'
      double cA[3], cB[3], n[3], p[3];
#ifdef MH_ARTIC_BSP_TU
      if (M.pr.kind[k]) {                                          // ... for a box-sphere pair: A's closest point of the signed-distance function, normal B to A
        double low = bsp_sdist(M, Y, g, k, cA, cB);
        bool have = true;
        if (low >= NEAR_ZERO_) {
          const double d[3] = { cA[0] - cB[0], cA[1] - cB[1], cA[2] - cB[2] };
          const double len = sqrt((d[0]*d[0] + d[1]*d[1]) + d[2]*d[2]);
          for (int c2 = 0; c2 < 3; c2++) { p[c2] = cA[c2]; n[c2] = d[c2] / len; }
        } else have = bsp_contact(M, Y, g, k, NEAR_ZERO_, p, n, low);   // (signed_violation = the contact's own distance)
        if (have) {
          if (lane == 0) { double* c = g + Z.cp + 12 * nc; for (int c2 = 0; c2 < 3; c2++) { c[c2] = p[c2]; c[3 + c2] = n[c2]; }
                           ints[I_LINK + nc] = M.bx.link[M.pr.a[k]]; ints[I_LINKB + nc] = m.sphere_link[M.pr.b[k]]; dist[nc] = low; }
          nc++;
        }
        continue;
      }
#endif
      const double low = pair_dist(M, Y, g, k, cA, cB, n);
      const double rA = m.sphere_radius[M.pr.a[k]], rB = m.sphere_radius[M.pr.b[k]];
      if (low >= NEAR_ZERO_) { for (int c2 = 0; c2 < 3; c2++) p[c2] = cA[c2] - n[c2] * rA; }
      else { for (int c2 = 0; c2 < 3; c2++) p[c2] = ((cA[c2] - n[c2] * rA) + (cB[c2] + n[c2] * rB)) * 0.5; }
      if (lane == 0) { double* c = g + Z.cp + 12 * nc; for (int c2 = 0; c2 < 3; c2++) { c[c2] = p[c2]; c[3 + c2] = n[c2]; }
                       ints[I_LINK + nc] = m.sphere_link[M.pr.a[k]]; ints[I_LINKB + nc] = m.sphere_link[M.pr.b[k]]; dist[nc] = low; }
      nc++;
    }
#endif
    nc = uni(nc);
    const int n = nc + nl;
    wave_sync();
    if (n > 0) {
      if (n > MH_LCP_MAX_N_WAVE || nl > 2 * NJ || !ws) { status |= MH_WORLD_UNSUPPORTED; break; }
      if (!dynamics(M, Y, g, nullptr)) { status |= MH_WORLD_LCP_FAILED; break; }      // compute_X at the CURRENT configuration (ICH:1600-1607)
      if (lane < nj) {
        const int base = popc(mu & lanes_below(lane)) + popc(ml & lanes_below(lane));
        if (hfin) idx[base] = lane | 256;
        if (lfin) idx[base + (hfin ? 1 : 0)] = lane;
      }
      wave_sync();
      inverse_from_factor(Y, g);
      const double* X = g + Y.X;
#ifdef MH_ARTIC_BOX_TU
      double* C = ws + WS_C; double* XC = ws + WS_XC;
#else
      double* C = g + Z.C; double* XC = g + Z.XC;
#endif
      for (int e = lane; e < nc * nj; e += 64) {                   // Cn rows: [n, r x n] . calc_jacobian(link) at the link's COM (handle_impacts' rows, normal direction)
        const int i = e / nj, j = e - i * nj;
        const int l = ints[I_LINK + i];
        double val = 0.0;
#ifdef MH_ARTIC_PAIR_TU
        val = contact_row(M, Y, g, l, ints[I_LINKB + i], j, g + Z.cp + 12 * i, g + Z.cp + 12 * i + 3);
#else
        if ((M.anc[l] >> j) & 1u) {
          double rc[3], com[3], r[3], w[6];
          mat3vec(g + Y.R + 9 * l, m.com[l], rc);
          const double* p = g + Z.cp + 12 * i; const double* dir = p + 3;
          for (int k = 0; k < 3; k++) { com[k] = g[Y.x + 3 * l + k] + rc[k]; r[k] = p[k] - com[k]; }
          cross3(r, dir, w + 3);
          for (int k = 0; k < 3; k++) w[k] = dir[k];
          const double* Sj = g + Y.S + 6 * j;
          double acc = 0.0;
          for (int k = 0; k < 6; k++) {
            double Jk;
            if (k >= 3) Jk = Sj[k - 3];
            else { const int k1 = (k + 1) % 3, k2 = (k + 2) % 3; Jk = Sj[3 + k] + (Sj[k1] * com[k2] - Sj[k2] * com[k1]); }
            acc = acc + w[k] * Jk;
          }
          val = acc;
        }
#endif
        C[e] = val;
      }
      wave_sync();
      for (int e = lane; e < nc * nj; e += 64) {                   // XC[i][c] = C[i][:] X[:, c]
        const int i = e / nj, c = e - i * nj;
        double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[i * nj + k] * X[k * nj + c];
        XC[e] = acc;
      }
      wave_sync();
      double nrm0 = 0.0;
      for (int e = lane; e < n * n; e += 64) {                     // determine_dq (CStab:932-970): MM = [Cn_X_CnT  Cn_X_LT; Cn_X_LT'  L_X_LT], column-major
        const int r = e % n, c = e / n;
        double v;
        if (r < nc && c < nc) { double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[r * nj + k] * XC[c * nj + k]; v = acc; }
        else if (r < nc || c < nc) {
          const int i = (r < nc) ? r : c, k2 = ((r < nc) ? c : r) - nc;
          const int ik = idx[k2] & 255;
          double acc = 0.0; for (int k = 0; k < nj; k++) acc = acc + C[i * nj + k] * X[ik * nj + k];
          v = acc;
        } else { const int a = r - nc, b2 = c - nc; const int ia = idx[a] & 255, ib = idx[b2] & 255; v = (b2 >= a) ? X[ia * nj + ib] : X[ib * nj + ia]; }
        WM[e] = v;
        const double av = fabs(v); nrm0 = (av > nrm0) ? av : nrm0;
      }
      nrm0 = wave_max(nrm0);
      double qi = 0.0;
      if (lane < nc) qi = (dist[lane] - fabs(m.cstab_eps)) - NEAR_ZERO_;                                   // CStab:431
      else if (lane < n) { const int my = idx[lane - nc]; const int myj = my & 255; const double qj = g[Y.q + myj];
                           const double viol = (my & 256) ? (m.hilimit[myj] - qj) - 0.0 : (qj + 0.0) - m.lolimit[myj];
                           qi = (viol - fabs(m.cstab_eps)) - NEAR_ZERO_; }                                 // CStab:434-441
      wave_sync();
      const double dii = (lane < n) ? WM[lane + n * lane] : 0.0;
      int zsize = 0;                                               // determine_dq's local z: cold lcp_fast, then the Lemke ladder (CStab:954-955)
      double zi = 0.0;
      DenseLds Md; Md.M = WM; Md.n = n;
      LuScratch S; S.small = g + Z.A; S.ka = NR; S.big = WLU;
      Trace tr; tr.buf = nullptr; tr.cap = 0; tr.len = 0;
      LcpParams P; P.kind = MH_LCP_FAST; P.min_exp = -20; P.step_exp = 1u; P.max_exp = 1; P.piv_tol = -1.0; P.zero_tol = -1.0;
      unsigned piv = 0, total = 0;
      bool ok = lcp_solve_wave(P, c_pow10a, n, Md, S, g + Z.art, nrm0, dii, qi, zi, zsize, rng, piv, tr);
      total += piv;
      if (!ok) {
        P.kind = MH_LCP_LEMKE_REG;
        ok = lcp_solve_wave(P, c_pow10a, n, Md, S, g + Z.art, nrm0, dii, qi, zi, zsize, rng, piv, tr);
        total += piv;
      }
      solves += 1ull; rows += (unsigned long long)n; pivs += total; bytes += 8ull * ((unsigned long long)n * n + 2ull * n);
      stab_rows += (unsigned long long)n;
      // update_from_stacked(pd, z): cn, l = z whatever it holds; dv = X_CnT cn + X_LT ls; v += dv; dq = the joint velocities
      double* zz = uT;                                             // (free until the line search)
      wave_sync();
      if (lane < n) zz[lane] = (lane < uni(zsize)) ? zi : 0.0;
      wave_sync();
      if (lane < nj) {
        double dv = 0.0;
        if (nc > 0) { double acc = 0.0; for (int i = 0; i < nc; i++) acc = acc + XC[i * nj + lane] * zz[i]; dv = acc; }
        double t2 = 0.0;
        for (int k = 0; k < nl; k++) { const int c = idx[k]; const double lk = zz[nc + k]; const double ls = (c & 256) ? -lk : lk; t2 = t2 + ls * X[(c & 255) * nj + lane]; }
        dv = (nc > 0) ? dv + t2 : t2;
        const double v = g[Y.qd + lane] + dv;
        g[Y.qd + lane] = v; dq = v;
      }
      wave_sync();
    }
    // update_q (CStab:1056-1216)
    { auto set_q = [&](double t, bool plain) { wave_sync(); if (lane < nj) { double v = plain ? dq : dq * t; v = v + qv; g[Y.q + lane] = v; } };
      auto eval_at = [&](double t, unsigned i) -> double { set_q(t, false); eval(uT); const double v = uT[i]; wave_sync(); return v; };   // CStab:1281-1298
      set_q(0.0, false);                                           // (q = qv: dq * 0 + qv is qv for finite dq)
      if (lane < nj) g[Y.q + lane] = qv;
      eval(uO);
      set_q(1.0, true);
      eval(uN);
      double t = 1.0;
      for (int i = 0; i < nu; i++) {
        const double fo = uO[i], fn = uN[i];
        if (!((fo < 0.0 && fn > 0.0) || (fo > 0.0 && fn < 0.0))) continue;
        // Ridders (CStab:1322-1379)
        double root = 0.0;
        { const double TOL = 1e-4;
          double ans = A_INF_, fm, fnew, s2, xh, xl, xm, xnew, fl = fo, fh = fn;
          xl = 0.0; xh = t;
          bool done = false;
          for (unsigned j = 0; j < 25 && !done; j++) {
            xm = 0.5 * (xl + xh);
            fm = eval_at(xm, (unsigned)i);
            s2 = sqrt(fm * fm - fl * fh);
            if (s2 == 0.0) { root = ans; done = true; break; }
            xnew = xm + (xm - xl) * ((fl >= fh ? 1.0 : -1.0) * fm / s2);
            ans = xnew;
            fnew = eval_at(ans, (unsigned)i);
            if (fabs(fnew) < TOL && fnew >= 0.0) { root = xnew; done = true; break; }
            if (stab_sign2(fm, fnew) != fm) { xl = xm; fl = fm; xh = ans; fh = fnew; }
            else if (stab_sign2(fl, fnew) != fl) { xh = ans; fh = fnew; }
            else if (stab_sign2(fh, fnew) != fh) { xl = ans; fl = fnew; }
          }
          if (!done) root = 0.0; }
        if (root > 0.0 && root < 1.0) t = (root < t) ? root : t;
      }
      set_q(t, false);
      eval(uT);
      bool failed = false;
      while (true) {
        bool stop = true;
        for (int i = 0; i < nu; i++) {
          const double fo = uO[i], fn1 = uN[i], fc = uT[i];
          const bool br = (fo < 0.0 && fn1 > 0.0) || (fo > 0.0 && fn1 < 0.0);
          if (!br && fc < 0.0 && fo > fc) { stop = false; break; }
        }
        if (stop) break;
        t *= 0.6;
        if (t < NEAR_ZERO_) { failed = true; break; }
        set_q(t, false);
        eval(uT);
      }
      if (failed) { status |= MH_WORLD_STAB_FAILED; break; }
      wave_sync();
      if (lane < nj) qv = g[Y.q + lane];
      wave_sync();
    }
    max_uvio = eval(uO);
    iterations++;
    stab_iters += 1ull;
  }
  wave_sync();
  if (lane < nj) { g[Y.qd + lane] = qd_save; g[Y.q + lane] = qv; }
  wave_sync();
}

// STAB: ConstraintStabilization::stabilize after every step (its own kernel below: the out-of-line stabiliser costs the caller's register
// allocation 187 spilled registers and half its speed -- 116 ms against 60 on the ur10 with link spheres -- even when it never runs)
template <bool STAB>
MH_DEV void artic_contacts_body(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                mh_world_aux* __restrict__ auxg, double* __restrict__ wsg
#ifdef MH_ARTIC_DRIVE_TU
                                , const mh_artic_drive& D
#endif
#if defined(MH_ARTIC_POSE_TU) || defined(MH_ARTIC_BOX_TU)
                                , const mh_artic_drive* Dp
#endif
#ifdef MH_ARTIC_POSE_TU
                                , double* __restrict__ poseg
#endif
#ifdef MH_ARTIC_REPORT_TU
                                , double* __restrict__ report   // B x nsteps x nslots x MH_REPORT_PAIR rows, or NULL: nothing is written, the steps are the same
#endif
#ifdef MH_ARTIC_WRENCH_TU
                                , const mh_artic_wrench* Wp     // the link wrench of the launch, or NULL: no force, the steps of the per-world-parameters kernels
#endif
                                )
{
  extern __shared__ double g[];
  const int b = blockIdx.x;
  if (b >= B) return;
#ifdef MH_ARTIC_PARAMS_TU
  const Model& M = Mg[b];                                          // per-world parameters: world b's own image of B
#else
  const Model& M = *Mg;
#endif
  const int nj = M.m.nj, lane = lane_id();
  const Lay Y(nj);
  const LayC Z(Y.total, nj, Y.I6, 60 * nj + 12);
  mh_world_aux* aux = auxg + b;
#ifdef MH_ARTIC_BOX_TU
  double* ws = wsg ? wsg + (size_t)b * WS_WORLD : nullptr;
#else
  double* ws = wsg ? wsg + (size_t)b * 2 * MH_LCP_MAX_N_WAVE * MH_LCP_MAX_N_WAVE : nullptr;   // Drumwright-Shell: _MM and the Lemke LU workspace
#endif
  if (lane < nj) { g[Y.q + lane] = qg[(size_t)b * nj + lane]; g[Y.qd + lane] = qdg[(size_t)b * nj + lane]; }
#ifdef MH_ARTIC_POSE_TU
  pose_load(Y, g, poseg + 7 * (size_t)b);
#endif
  WaveRand rng; rng.load(aux->rng);
  if (lane == 0) g_lcp_prof_on = 0;
  int status = uni(aux->status);
  double tm = uni(aux->time);
  unsigned long long solves = 0, rows = 0, pivs = 0, bytes = 0, minis = 0, steps = 0, stab_iters = 0, stab_rows = 0;
  const int FROZEN = MH_WORLD_UNSUPPORTED | MH_WORLD_STALLED;
  bool kin_ok = false;
  wave_sync();
#ifdef MH_ARTIC_REPORT_TU
  // this world's rows: lane k owns slot k's row of every step and zeroes it before the step folds into it; the rows of steps that a world passed over
  // or frozen never reaches are zeroed behind the loop
  const int nslots = M.m.nspheres + M.bx.n + M.pr.n;
  double* const rep0 = report ? report + (size_t)b * nsteps * nslots * MH_REPORT_PAIR : nullptr;
  auto rep_zero = [&](int s) { if (rep0 && lane < nslots) for (int k = 0; k < MH_REPORT_PAIR; k++) rep0[((size_t)s * nslots + lane) * MH_REPORT_PAIR + k] = 0.0; };
  int rep_done = 0;
#endif
  for (int s = 0; s < nsteps; s++) {
#ifdef MH_ARTIC_REPORT_TU
    rep_zero(s); rep_done = s + 1;
    double* const rep = rep0 ? rep0 + (size_t)s * nslots * MH_REPORT_PAIR : nullptr;
#endif
    if (status & (FROZEN | MH_WORLD_LCP_FAILED)) break;           // as in the oracle: the reference would have thrown out of step() / never returned from it
    double h = 0.0; unsigned guard = 0;
    while (h < dt) {
#ifdef MH_ARTIC_DRIVE_TU
      const double hh = uni(do_mini_step(M, Y, Z, g, ws, aux, rng, dt - h, kin_ok, status, solves, rows, pivs, bytes, D, B, b, s));
#elif defined(MH_ARTIC_POSE_TU) || defined(MH_ARTIC_BOX_TU)
#ifdef MH_ARTIC_WRENCH_TU
      const double hh = uni(do_mini_step(M, Y, Z, g, ws, aux, rng, dt - h, kin_ok, status, solves, rows, pivs, bytes, Dp, B, b, s, rep, Wp));
#elif defined(MH_ARTIC_REPORT_TU)
      const double hh = uni(do_mini_step(M, Y, Z, g, ws, aux, rng, dt - h, kin_ok, status, solves, rows, pivs, bytes, Dp, B, b, s, rep));
#else
      const double hh = uni(do_mini_step(M, Y, Z, g, ws, aux, rng, dt - h, kin_ok, status, solves, rows, pivs, bytes, Dp, B, b, s));
#endif
#else
      const double hh = uni(do_mini_step(M, Y, Z, g, ws, aux, rng, dt - h, kin_ok, status, solves, rows, pivs, bytes));
#endif
      if (status & MH_WORLD_LCP_FAILED) break;                    // thrown out of the mini-step: current_time += h (TSS:215) is not reached, the mini-step not counted
      h += hh; tm += hh; minis++;
      if (status & FROZEN) break;
      if (++guard > 100000u) { status |= MH_WORLD_STALLED; break; }
    }
    if (status & MH_WORLD_LCP_FAILED) break;                      // ... and out of step(): no stabilisation, the step is not counted
    if (STAB && M.m.cstab_max_iterations != 0) {                  // TSS:97
      wave_sync();
      // (copies in and out: the stabiliser is an out-of-line function, and a variable whose address it takes would live in scratch
      //  memory for the whole kernel -- the mini-step loop above reads and writes these all the time)
      WaveRand r2 = rng; int st2 = status;
      unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
      stabilize_contacts(M, Y, Z, g, ws, r2, st2, c0, c1, c2, c3, c4, c5);
      rng = r2; status = st2; solves += c0; rows += c1; pivs += c2; bytes += c3; stab_iters += c4; stab_rows += c5;
      kin_ok = false;
      if (status & MH_WORLD_LCP_FAILED) break;                    // compute_X threw inside the stabiliser
    }
    steps++;
#ifdef MH_ARTIC_POSE_TU
    pose_fold_lds(Y, g);                                          // new coordinates: the link frames in LDS are the same only to round-off
    kin_ok = false;
#endif
  }
#ifdef MH_ARTIC_REPORT_TU
  for (int s = rep_done; s < nsteps; s++) rep_zero(s);
#endif
  if (lane < nj) { qg[(size_t)b * nj + lane] = g[Y.q + lane]; qdg[(size_t)b * nj + lane] = g[Y.qd + lane]; }
#ifdef MH_ARTIC_POSE_TU
  pose_store(Y, g, poseg + 7 * (size_t)b);
#endif
  rng.store(aux->rng);
  if (lane == 0) {
    aux->time = tm; aux->status = status;
    aux->steps += steps; aux->mini_steps += minis;
    aux->lcp_solves += solves; aux->lcp_rows += rows; aux->lcp_pivots += pivs; aux->lcp_alg_bytes += bytes;
    aux->stab_iters += stab_iters; aux->stab_rows += stab_rows;
  }
}

#ifdef MH_ARTIC_BOX_TU
// the geometry kernels, four per code object: k_artic_step_<fam>[_stab][_pose][_drive], {plain, stab} x {undriven, driven}, <fam> the file's
// family token MH_ARTIC_GEOM (box, pair, bsp) and _pose (with the B x 7 poses as one more argument) under MH_ARTIC_POSE_TU.  The drive is a
// pointer in the body, NULL = undriven.  One world per workgroup; the LDS image holds one world per SIMD or two (DESIGN 4.4), so no
// waves-per-EU bound
#ifndef MH_ARTIC_GEOM
#error "a geometry translation unit (MH_ARTIC_BOX_TU) names its family: #define MH_ARTIC_GEOM box | pair | bsp"
#endif
#ifdef MH_ARTIC_POSE_TU
#define MH_GEOM_KERNEL_(fam, stab, drive) k_artic_step_##fam##stab##_pose##drive
#define MH_GEOM_POSE_PARAM , double* __restrict__ poseg
#define MH_GEOM_POSE_ARG , poseg
#else
#define MH_GEOM_KERNEL_(fam, stab, drive) k_artic_step_##fam##stab##drive
#define MH_GEOM_POSE_PARAM
#define MH_GEOM_POSE_ARG
#endif
#ifdef MH_ARTIC_WRENCH_TU
// (the wrench travels by value behind the rows, as the drive does; terms 0 = the body's NULL)
#define MH_GEOM_REPORT_PARAM , double* __restrict__ report, mh_artic_wrench W
#define MH_GEOM_REPORT_ARG , report, (W.terms != 0 ? &W : nullptr)
#elif defined(MH_ARTIC_REPORT_TU)
#define MH_GEOM_REPORT_PARAM , double* __restrict__ report
#define MH_GEOM_REPORT_ARG , report
#else
#define MH_GEOM_REPORT_PARAM
#define MH_GEOM_REPORT_ARG
#endif
#define MH_GEOM_KERNEL_X(fam, stab, drive) MH_GEOM_KERNEL_(fam, stab, drive)      // (the token is expanded before it is pasted)
#define MH_GEOM_KERNEL(stab, drive) MH_GEOM_KERNEL_X(MH_ARTIC_GEOM, stab, drive)
#define MH_GEOM_STAMP(STAB, stab) \
__global__ __launch_bounds__(64) \
void MH_GEOM_KERNEL(stab, )(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg, \
                            mh_world_aux* __restrict__ auxg, double* __restrict__ wsg MH_GEOM_POSE_PARAM MH_GEOM_REPORT_PARAM) \
{ artic_contacts_body<STAB>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg, nullptr MH_GEOM_POSE_ARG MH_GEOM_REPORT_ARG); } \
__global__ __launch_bounds__(64) \
void MH_GEOM_KERNEL(stab, _drive)(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg, \
                                  mh_world_aux* __restrict__ auxg, double* __restrict__ wsg MH_GEOM_POSE_PARAM, mh_artic_drive D MH_GEOM_REPORT_PARAM) \
{ artic_contacts_body<STAB>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg, &D MH_GEOM_POSE_ARG MH_GEOM_REPORT_ARG); }
MH_GEOM_STAMP(false, )
MH_GEOM_STAMP(true, _stab)
#elif !defined(MH_ARTIC_DRIVE_TU) && !defined(MH_ARTIC_POSE_TU)
// 2 waves per SIMD = the 8 worlds per CU the 18 KB LDS image allows
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_contacts(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                           mh_world_aux* __restrict__ auxg, double* __restrict__ wsg) { artic_contacts_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg); }
// the same step followed by the stabiliser with contact and limit rows (stabilize_contacts)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_contacts_stab(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                mh_world_aux* __restrict__ auxg, double* __restrict__ wsg) { artic_contacts_body<true>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg); }
#elif defined(MH_ARTIC_DRIVE_TU)
// the same two with a drive (mh_artic_batch_step_driven)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_contacts_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                 mh_world_aux* __restrict__ auxg, double* __restrict__ wsg, mh_artic_drive D) { artic_contacts_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg, D); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_contacts_stab_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                      mh_world_aux* __restrict__ auxg, double* __restrict__ wsg, mh_artic_drive D) { artic_contacts_body<true>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg, D); }
#else
// the two in pose coordinates, undriven and driven (mh_artic_pose.hip)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_contacts_pose(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                mh_world_aux* __restrict__ auxg, double* __restrict__ wsg, double* __restrict__ poseg) { artic_contacts_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg, nullptr, poseg); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_contacts_pose_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                      mh_world_aux* __restrict__ auxg, double* __restrict__ wsg, double* __restrict__ poseg, mh_artic_drive D) { artic_contacts_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg, &D, poseg); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_contacts_stab_pose(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                     mh_world_aux* __restrict__ auxg, double* __restrict__ wsg, double* __restrict__ poseg) { artic_contacts_body<true>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg, nullptr, poseg); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_contacts_stab_pose_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                           mh_world_aux* __restrict__ auxg, double* __restrict__ wsg, double* __restrict__ poseg, mh_artic_drive D) { artic_contacts_body<true>(Mg, B, dt, nsteps, qg, qdg, auxg, wsg, &D, poseg); }
#endif
