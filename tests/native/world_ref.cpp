// TEST INFRASTRUCTURE: the one statement of the free-body world step beyond the oracle, which the GPU world kernels are held to bit for bit
// (include/moby_hip.h: "Box-sphere pairs", "Static bodies", mh_world_forces / mh_world_batch_step_wrench, "Contact report").
//
// oracle::World (oracle/world.hpp) knows one static object (the scene's plane), gravity alone, and refuses an enabled box-sphere pair in its broad phase.
// World is all-public and does not care about the index of a body that is not enabled (islands, problem data, impulses and point velocities only ask
// enabled(b)), so this file restates ONLY what those features change, each function once:
//   * the scene view: the pair arrays run triangularly over ntot = nb + has_ground + n bodies (an explicit pair list handed to World; with no statics
//     that is the scene's own numbering);
//   * the plane frame: to_plane / from_plane / plane_n take the plane's body index (the scene's ground is nb, static k is nb + has_ground + k), and with
//     them the plane cases of signed_dist and find_contacts (PlanePrimitive.cpp:338-411, CCD.inl:804-886) and the box-plane rule of conservative
//     advancement (CCD.cpp:238-468), whose polyhedron-plane tail is World's own;
//   * box-sphere pairs, the box a body (centre = COM, axes = World::rot) or a static (its record): signed_dist is BoxPrimitive::calc_signed_dist for a
//     sphere (BoxPrimitive.cpp:256-276, 788-836; with the sphere as A, SpherePrimitive.cpp:282-290 forwards with the point arguments swapped: the points
//     stay with their bodies); find_contacts is BoxPrimitive::calc_closest_points as its clamp fixed point + find_contacts_box_sphere
//     (CCD.inl:1208-1259), created as (box, sphere); the sphere rule of conservative advancement (CCD.cpp:121-235) gets calc_max_dist = 0 for a static
//     box from World (CCD.cpp:585-609).  The geometry is the text of tests/native/artic_boxsphere_ref.cpp (bsp_contact / bsp_sdist); three-term sums as
//     (a + b) + c;
//   * broad_phase: the refusal names box-box alone (a box body against a static box included), a box-sphere pair takes the swept-bounds test; a static
//     box's bounding sphere (centre, half diagonal) does not move (CCD.cpp:735-768), a plane's bound is infinite, pairs of two disabled bodies are
//     dropped (CCD.cpp:864-866);
//   * forcing: World::fwd_dyn and the joint-free branch of fwd_dyn_and_integrate with the terms evaluated where the reference runs its recurrent forces
//     and controllers -- once per mini-step, after the position update and before calc_fwd_dyn (precalc_fwd_dyn: TimeSteppingSimulator.cpp:173 ->
//     Simulator.cpp:319-350; StokesDragForce.cpp:39-44, DampingForce.cpp:32-51).  Taken whenever the caller hands over forces (even with no terms) or a
//     wrench; with neither the step runs the oracle's own fwd_dyn_and_integrate;
//   * the callers that reach those through non-virtual calls: calc_pairwise_distances, CA_step / next_CA_step, do_mini_step, the stabiliser
//     (eval_unilateral, eval_at, ridders, update_q, stabilize -- the joint-free statements: the scenes of the many-worlds stepper have no joints), step;
//   * the contact report, which adds no physics: it is what ConstraintSimulator::constraint_post_callback_fn (ConstraintSimulator.cpp:353) would see --
//     the mini-step's contact constraints with the contact_impulse that update_from_stacked accumulated (ImpactConstraintHandler.cpp:298-327) -- summed
//     per pair.  The oracle carries that quantity: Contact::imp (oracle/world.hpp:65), zeroed when the contact is made, added to by
//     World::apply_impulses; do_mini_step folds it behind handle_impacts when it is given a sink.
// Everything else is the oracle's own: sphere pairs, spokes (scene ground only), islands, the impact handler, the LCP chain, the dynamics.
// Pins: with forces of no terms, and with none at all, it equals oracle_world_step_batch bit for bit, and so it does with every coefficient zero
// (tests/test_world_forces.py, on the stack, wheel, box and ball scenes); a lone body under Stokes drag and a wrench follows the recurrence written out
// in numpy (same file); with no box-sphere pair enabled it equals the oracle (tests/test_world_boxsphere.py); a scene with has_ground = 1 and no
// statics, and the same scene with has_ground = 0 and one static plane carrying plane_R / plane_o, both equal the oracle, and statics = NULL equals an
// empty record (tests/test_world_statics.py); the box geometry equals numpy written out by hand on dyadic inputs, over a quaternion and over a matrix,
// and artic_boxsphere_ref's static box on identical poses (both files); the report sink changes no step (tests/test_world_report.py).
// Built by the tests with g++ and oracle/Makefile's CXXFLAGS (-ffp-contract=off: every operation rounds on its own).
#include <cstring>
#include "lcp.hpp"
#include "world.hpp"

using namespace oracle;

namespace {

const mh_world_statics* g_st = nullptr;   // the statics of the scene being stepped (n may be 0); set by the entry points
int g_hg = 0;                             // the scene's has_ground

int slot_of(const World& w, int b) { return b - w.sc->nb - g_hg; }   // static index of body b (-1: the scene's ground)
bool is_sphere(const World& w, int b) { return b >= 0 && b < w.sc->nb && w.sc->geom_type[b] == MH_GEOM_SPHERE; }
bool is_static(const World& w, int b, int type)
{
  if (b < w.sc->nb) return false;
  const int k = slot_of(w, b);
  if (k < 0) return type == MH_STATIC_PLANE;                          // the scene's own ground
  return k < g_st->n && g_st->type[k] == type;
}
bool is_sbox(const World& w, int b) { return is_static(w, b, MH_STATIC_BOX); }
const double* frame_R(const World& w, int b) { const int k = slot_of(w, b); return k < 0 ? w.sc->plane_R : g_st->R[k]; }
const double* frame_o(const World& w, int b) { const int k = slot_of(w, b); return k < 0 ? w.sc->plane_o : g_st->o[k]; }
V3 plane_n(const World& w, int pl) { const double* R = frame_R(w, pl); return v3(R[1], R[4], R[7]); }
V3 to_plane(const World& w, V3 p, int pl)
{
  const double* R = frame_R(w, pl); const double* o = frame_o(w, pl); V3 d = p - v3(o[0], o[1], o[2]);
  return v3((R[0]*d.x + R[3]*d.y) + R[6]*d.z, (R[1]*d.x + R[4]*d.y) + R[7]*d.z, (R[2]*d.x + R[5]*d.y) + R[8]*d.z);
}
V3 from_plane(const World& w, V3 p, int pl)
{
  const double* R = frame_R(w, pl); const double* o = frame_o(w, pl);
  return v3(o[0] + ((R[0]*p.x + R[1]*p.y) + R[2]*p.z), o[1] + ((R[3]*p.x + R[4]*p.y) + R[5]*p.z), o[2] + ((R[6]*p.x + R[7]*p.y) + R[8]*p.z));
}
// pair (a, b) is a box and a sphere: the box a body or a static, the sphere a body
bool bsp_bodies(const World& w, int a, int b, int& bx, int& sp)
{
  if (w.is_box(a) && is_sphere(w, b)) { bx = a; sp = b; return true; }
  if (is_sphere(w, a) && (w.is_box(b) || is_sbox(w, b))) { bx = b; sp = a; return true; }
  return false;
}
bool bsp_pair(const World& w, int p, int& bx, int& sp) { int a, b; w.pair_bodies(p, a, b); return bsp_bodies(w, a, b, bx, sp); }
// axes, centre and edge lengths of box bx
void box_frame(const World& w, int bx, double R[9], V3& cb, const double*& len)
{
  if (bx < w.sc->nb) { w.rot(bx, R); cb = w.X(bx); len = w.sc->geom_dim[bx]; return; }
  const int k = slot_of(w, bx);
  for (int i = 0; i < 9; i++) R[i] = g_st->R[k][i];
  cb = v3(g_st->o[k][0], g_st->o[k][1], g_st->o[k][2]); len = g_st->dim[k];
}

V3 mat_v(const double R[9], V3 p) { return v3((R[0]*p.x + R[1]*p.y) + R[2]*p.z, (R[3]*p.x + R[4]*p.y) + R[5]*p.z, (R[6]*p.x + R[7]*p.y) + R[8]*p.z); }
V3 matT_v(const double R[9], V3 p) { return v3((R[0]*p.x + R[3]*p.y) + R[6]*p.z, (R[1]*p.x + R[4]*p.y) + R[7]*p.z, (R[2]*p.x + R[5]*p.y) + R[8]*p.z); }

// the geometry over raw poses: box axes R (row-major), centre cb, edge lengths len; sphere centre cS, radius Rs
struct BspContact { int has, region; double dist; V3 p, n; };
// region: 0 face, 1 edge, 2 vertex, 3 the centre inside the box (the count of coordinates of p at their extent: 1, 2, 3, 0)
BspContact bsp_contact(const double R[9], V3 cb, const double len[3], V3 cS, double Rs, double TOL)
{
  BspContact o; o.has = 0; o.p = v3(0, 0, 0); o.n = v3(0, 0, 0);
  const V3 cv = matT_v(R, cS - cb);
  const double c[3] = { cv.x, cv.y, cv.z };
  const double h[3] = { len[0] * 0.5, len[1] * 0.5, len[2] * 0.5 };
  double p[3], u[3];
  for (int i = 0; i < 3; i++) { p[i] = (c[i] < -h[i]) ? -h[i] : ((c[i] > h[i]) ? h[i] : c[i]); u[i] = p[i] - c[i]; }
  const double nrm = std::sqrt((u[0]*u[0] + u[1]*u[1]) + u[2]*u[2]);
  { int at = 0; for (int i = 0; i < 3; i++) if (!(std::fabs(p[i]) < h[i])) at++; o.region = (at == 0) ? 3 : at - 1; }
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
  o.dist = dist;
  if (dist > TOL) return o;
  const V3 ug = mat_v(R, v3(u[0], u[1], u[2])), pr = mat_v(R, v3(p[0], p[1], p[2]));
  const V3 sg = cS + ug;                                            // the sphere point
  const double ulen = norm(ug);
  bool own = false;
  if (dist > 0.0) {
    const V3 pg = cb + pr;                                          // the box point
    const V3 nd = pg - sg;
    const double nl = norm(nd);
    o.p = (sg + pg) * 0.5;
    if (nl > NEAR_ZERO) { o.n = nd / nl; own = true; }
  } else o.p = sg;
  if (!own) o.n = ug / ulen;                                        // (a centre inside the box: 0 / 0, as in the reference)
  o.has = 1;
  return o;
}
// pA the box point, pB the sphere point
double bsp_sdist(const double R[9], V3 cb, const double len[3], V3 cS, double Rs, V3& pA, V3& pB)
{
  const V3 cv = matT_v(R, cS - cb);
  const double c[3] = { cv.x, cv.y, cv.z };
  const double h[3] = { len[0] * 0.5, len[1] * 0.5, len[2] * 0.5 };
  double cl[3] = { c[0], c[1], c[2] };
  bool inside = true; double sq = 0.0, in = -INF;
  for (int i = 0; i < 3; i++) {
    if (c[i] < -h[i]) { const double dl = c[i] + h[i]; cl[i] = -h[i]; sq += dl * dl; inside = false; }
    else if (c[i] > h[i]) { const double dl = c[i] - h[i]; cl[i] = h[i]; sq += dl * dl; inside = false; }
    else if (inside) { const double dd = -std::min(std::fabs(h[i] - c[i]), std::fabs(c[i] + h[i])); in = std::max(in, dd); }
  }
  const double dist = (inside ? in : std::sqrt(sq)) - Rs;
  const V3 v = v3(cl[0] - c[0], cl[1] - c[1], cl[2] - c[2]);
  const double vn = norm(v);
  pA = cb + mat_v(R, v3(cl[0], cl[1], cl[2]));
  if (vn == 0.0) pB = cS;
  else {
    const V3 vg = mat_v(R, v);
    const double sc = (Rs + std::min(dist, 0.0)) / vn;
    pB = cS + vg * sc;
  }
  return dist;
}

// ---- the restated members ------------------------------------------------------------------------------------------------
void broad_phase(const World& w, double dt, std::vector<int>& pairs)
{
  const SceneView* sc = w.sc;
  const int ntot = sc->nb + g_hg + g_st->n;
  std::vector<double> lo(3 * (size_t)ntot), hi(3 * (size_t)ntot);
  for (int b = 0; b < ntot; b++) {
    if (is_sbox(w, b)) {                                             // the bounding sphere of a static box: built once, never moved
      const int k = slot_of(w, b);
      const double hx = g_st->dim[k][0] / 2.0, hy = g_st->dim[k][1] / 2.0, hz = g_st->dim[k][2] / 2.0;
      const double r = std::sqrt((hx*hx + hy*hy) + hz*hz);
      for (int q = 0; q < 3; q++) { lo[3*b+q] = g_st->o[k][q] - r; hi[3*b+q] = g_st->o[k][q] + r; }
      continue;
    }
    if (!w.enabled(b)) { for (int k = 0; k < 3; k++) { lo[3*b+k] = -INF; hi[3*b+k] = INF; } continue; }
    const V3 c = w.X(b);
    const V3 vdt = w.Vl(b) * dt, wdt = w.Wa(b) * dt;
    const V3 lin = vdt + cross(c, wdt);
    const V3 p2 = c + lin;
    const double r = w.bounding_radius(b);
    for (int k = 0; k < 3; k++) {
      const double a = comp(c, k), e = comp(p2, k);
      lo[3*b+k] = ((a < e) ? a : e) - r;
      hi[3*b+k] = ((a > e) ? a : e) + r;
    }
  }
  pairs.clear();
  for (int p = 0; p < sc->npairs; p++) {
    int i, j; w.pair_bodies(p, i, j);
    if (w.is_spokes(i) || w.is_spokes(j)) continue;
    if (w.is_box(i) && (w.is_box(j) || is_sbox(w, j))) {             // box-box, a static box included: not built
      if (sc->pair_enabled[p]) w.aux->status |= MH_WORLD_UNSUPPORTED;
      continue;
    }
    bool ov = true;
    for (int k = 0; k < 3; k++) if (!(lo[3*i+k] <= hi[3*j+k] && lo[3*j+k] <= hi[3*i+k])) ov = false;
    if (!ov) continue;
    if (!sc->pair_enabled[p]) continue;
    if (!w.enabled(i) && !w.enabled(j)) continue;
    pairs.push_back(p);
  }
  if (g_hg)                                                           // the wheel's plugin appends (ground, wheel) after CCD's pairs
    for (int i = 0; i < sc->nb; i++) if (w.is_spokes(i)) {
      if (g_st->n > 0) { w.aux->status |= MH_WORLD_UNSUPPORTED; continue; }   // refused at create: the plugin knows one ground
      pairs.push_back(World::pair_index(i, sc->nb, ntot));
    }
}

PairDist signed_dist(const World& w, int p)
{
  PairDist d; d.pair = p; w.pair_bodies(p, d.a, d.b);               // a < b: id order
  if (w.is_spokes(d.a)) return w.signed_dist(p);                    // against the scene's ground: World's own
  int bx, sp;
  if (bsp_bodies(w, d.a, d.b, bx, sp)) {
    double R[9]; V3 cb; const double* len; box_frame(w, bx, R, cb, len);
    V3 pbox, psph;
    d.dist = bsp_sdist(R, cb, len, w.X(sp), w.sc->geom_dim[sp][0], pbox, psph);
    if (bx == d.a) { d.pa = pbox; d.pb = psph; } else { d.pa = psph; d.pb = pbox; }
    return d;
  }
  if (w.is_box(d.a)) {                                              // PlanePrimitive::calc_signed_dist(polyhedral) over the pair's own plane
    double min_dist = INF;
    for (int i = 0; i < 8; i++) {
      const V3 g = w.box_vertex(d.a, i);
      const V3 pp = to_plane(w, g, d.b);
      if (pp.y < min_dist) { min_dist = pp.y; d.pa = g; d.pb = from_plane(w, v3(pp.x, 0.0, pp.z), d.b); }
    }
    d.dist = min_dist;
    return d;
  }
  if (w.enabled(d.a) && w.enabled(d.b)) return w.signed_dist(p);    // two spheres
  const int s = w.enabled(d.a) ? d.a : d.b, pl = w.enabled(d.a) ? d.b : d.a;
  const V3 cp = to_plane(w, w.X(s), pl);
  const double r = w.sc->geom_dim[s][0];
  const double low = cp.y + (-1.0 * r);
  d.dist = low;
  const V3 on_plane = from_plane(w, v3(cp.x, 0.0, cp.z), pl);
  const V3 on_sphere = from_plane(w, v3(cp.x, low, cp.z), pl);
  if (s == d.a) { d.pa = on_sphere; d.pb = on_plane; } else { d.pa = on_plane; d.pb = on_sphere; }
  return d;
}
void calc_pairwise_distances(const World& w, const std::vector<int>& pairs, std::vector<PairDist>& out)
{
  out.clear();
  for (int p : pairs) out.push_back(signed_dist(w, p));
}
// region_out (optional): the region of a box-sphere pair's contact query, or -1 for another kind of pair
void find_contacts(const World& w, int p, double TOL, std::vector<Contact>& out, int* region_out = nullptr)
{
  int a, b; w.pair_bodies(p, a, b);
  if (region_out) *region_out = -1;
  if (w.is_spokes(a)) { w.find_contacts(p, TOL, out); return; }
  Contact c; c.pair = p;
  int bx, sp;
  if (bsp_bodies(w, a, b, bx, sp)) {
    double R[9]; V3 cb; const double* len; box_frame(w, bx, R, cb, len);
    const BspContact bc = bsp_contact(R, cb, len, w.X(sp), w.sc->geom_dim[sp][0], TOL);
    if (region_out) *region_out = bc.region;
    if (!bc.has) return;
    c.p = bc.p; c.n = bc.n; c.g1 = bx; c.g2 = sp; c.dist = bc.dist;  // created as (box, sphere)
    World::orthonormal_basis(c.n, c.s, c.t);
    w.fill_params(c);
    out.push_back(c);
    return;
  }
  if (w.is_box(a)) {                                                // find_contacts_plane_generic(plane, box) over the pair's own plane
    for (int i = 0; i < 8; i++) {
      const V3 g = w.box_vertex(a, i);
      const V3 pp = to_plane(w, g, b);
      if (!(pp.y <= TOL)) continue;
      c.p = g; c.n = -plane_n(w, b); c.g1 = b; c.g2 = a; c.dist = pp.y;
      World::orthonormal_basis(c.n, c.s, c.t);
      w.fill_params(c);
      out.push_back(c);
    }
    return;
  }
  if (w.enabled(a) && w.enabled(b)) { w.find_contacts(p, TOL, out); return; }
  const int s = w.enabled(a) ? a : b, pl = w.enabled(a) ? b : a;
  const V3 cp = to_plane(w, w.X(s), pl);
  const double r = w.sc->geom_dim[s][0];
  const double dist = cp.y - r;
  if (dist > TOL) return;
  c.p = from_plane(w, v3(cp.x, 0.5 * (cp.y - r), cp.z), pl);
  c.n = plane_n(w, pl); c.g1 = s; c.g2 = pl; c.dist = dist;
  World::orthonormal_basis(c.n, c.s, c.t);
  w.fill_params(c);
  out.push_back(c);
}
// World::next_CA_generic / CA_generic / CA_step over the functions above
double next_CA_generic(const World& w, const PairDist& d)
{
  if (w.is_spokes(d.b)) return INF;
  std::vector<Contact> cs; find_contacts(w, d.pair, NEAR_ZERO, cs);
  if (cs.empty()) return INF;
  for (const Contact& c : cs) if (w.contact_vel(c, c.n) < -NEAR_ZERO) return 0.0;
  int bx, sp;
  if (w.is_box(d.a) && !bsp_bodies(w, d.a, d.b, bx, sp)) {          // a box body on a plane (CCD.cpp:285-323, 383-397)
    if (cs.size() >= 3 && !World::collinear(cs[0].p, cs[1].p, cs[2].p)) return INF;
    const Contact& c = cs[0];
    const double dd = dot(c.n, c.p);
    return w.next_CA_box_plane(d.a, -c.n, -dd);
  }
  return INF;
}
double CA_generic(const World& w, const PairDist& d)
{
  if (d.dist <= 0.0) return next_CA_generic(w, d);
  const V3 d0 = d.pa - d.pb;
  const V3 n0 = d0 / norm(d0);
  const double tA = w.calc_max_dist(d.a, -n0, w.rmax_of(d.a));
  const double tB = w.calc_max_dist(d.b, n0, w.rmax_of(d.b));
  double total = tA + tB;
  if (total < 0.0) total = 0.0;
  const double cand = d.dist / total;
  return (cand < INF) ? cand : INF;
}
double CA_step(const World& w, const PairDist& d)
{
  int bx, sp;
  const bool bsp = bsp_pair(w, d.pair, bx, sp);
  if (!bsp && (w.is_spokes(d.b) || w.is_box(d.a))) return CA_generic(w, d);   // no SpherePrimitive in the pair (CCD.cpp:127-133)
  if (d.dist > NEAR_ZERO) return CA_generic(w, d);
  std::vector<Contact> cs; find_contacts(w, d.pair, NEAR_ZERO, cs);
  if (cs.size() == 1 && std::fabs(w.contact_vel(cs[0], cs[0].n)) < NEAR_ZERO * 10) return INF;
  return CA_generic(w, d);
}
double next_CA_step(const World& w)
{
  double t = INF;
  for (const PairDist& d : w.pairwise) { const double e = CA_step(w, d); t = (e < t) ? e : t; }
  return t;
}

// the scene's recurrent forces and the caller's wrench (include/moby_hip.h: mh_world_forces, mh_world_batch_step_wrench)
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
    const V3 vi = matT_v(R, v), wi = matT_v(R, om);
    const V3 fb = vi * (-(fo.F->damp_kl[b] + norm(vi) * fo.F->damp_klsq[b]));
    const V3 tb = wi * (-(fo.F->damp_ka[b] + norm(wi) * fo.F->damp_kasq[b]));
    F = F + mat_v(R, fb);
    const V3 tw = mat_v(R, tb);
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
  const V3 Jww = mat_v(Jw, om);
  const V3 tau = has_t ? T - cross(om, Jww) : -cross(om, Jww);
  double im, Ji[9]; w.inv_inertia(b, im, Ji);
  wd = mat_v(Ji, tau);
}

// region census of one step, over the contact queries the simulator's list makes for box-sphere pairs: a contact counts under the region the sphere's
// centre is in (0 face, 1 edge, 2 vertex) and, when its dist <= 0 or the centre is inside the box, under 3 (penetrating) as well; 4 (none) = a pair
// under the threshold test whose contact query found nothing
struct Census { int* counts; };

// what a step's contacts were like, for the conditions the tests assert on their inputs (per world and step, 6 ints):
//   [0] mini-steps folded with at least one contact; [1] most contacts of one pair in one mini-step; [2] most pairs with cn > 0 in one mini-step;
//   [3] contacts with epsilon > 0 whose restitution pass added a second impulse; [4] contacts counted with zero impulse; [5] contacts with sign = -1
enum { SH_MINI = 0, SH_PAIR_CONTACTS, SH_PAIRS_LOADED, SH_RESTITUTION, SH_ZERO, SH_NEG_SIGN, SH_COUNT };

// the report of one mini-step, summed into rows: npt x MH_REPORT_PAIR of this step; the contacts in constraint-list order
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

// World::do_mini_step over the functions above.  fo: NULL = the oracle's own forward dynamics; rows: this step's report rows, or NULL (shape with them)
double do_mini_step(World& w, double dt, Census* cen, const Forcing* fo, double* rows, int* shape)
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
  for (const PairDist& d : w.pairwise) if (d.dist < sc->contact_dist_thresh) {
    const size_t before = cs.size(); int region = -1;
    find_contacts(w, d.pair, sc->contact_dist_thresh, cs, &region);
    if (cen && region >= 0) {
      if (cs.size() == before) cen->counts[4]++;
      else {
        if (region <= 2) cen->counts[region]++;
        if (region > 2 || cs.back().dist <= 0.0) cen->counts[3]++;
      }
    }
  }
  w.handle_impacts(cs);
  if (w.thrown_) return h;                                           // (the exception leaves before CSim:353: nothing is folded)
  if (rows) fold(w, cs, rows, shape);                                // constraint_post_callback_fn (CSim:353)
  w.aux->time += h;
  w.aux->mini_steps++;
  return h;
}

// ---- constraint stabilisation (World::eval_unilateral, eval_at, ridders, update_q, stabilize: the statements a scene without joints runs) ----
double eval_unilateral(World& w, std::vector<double>& uC)
{
  double vio = INF;
  uC.clear();
  calc_pairwise_distances(w, w.pairs_to_check, w.pairwise);
  for (const PairDist& d : w.pairwise) { uC.push_back(d.dist); vio = (d.dist < vio) ? d.dist : vio; }
  return vio;
}
double eval_at(World& w, double t, unsigned i, const std::vector<double>& dq, const std::vector<double>& q)
{
  std::vector<double> qs(q.size()), uC;
  for (size_t k = 0; k < q.size(); k++) { qs[k] = dq[k] * t; qs[k] = qs[k] + q[k]; }
  w.set_q(qs);
  eval_unilateral(w, uC);
  return uC[i];
}
double ridders(World& w, double x1, double x2, double fl, double fh, unsigned idx, const std::vector<double>& dq, const std::vector<double>& q)
{
  const double TOL = 1e-4;
  double ans = INF, fm, fnew, s, xh, xl, xm, xnew;
  if ((fl > 0.0 && fh < 0.0) || (fl < 0.0 && fh > 0.0)) {
    xl = x1; xh = x2;
    for (unsigned j = 0; j < 25; j++) {
      xm = 0.5 * (xl + xh);
      fm = eval_at(w, xm, idx, dq, q);
      s = std::sqrt(fm * fm - fl * fh);
      if (s == 0.0) return ans;
      xnew = xm + (xm - xl) * ((fl >= fh ? 1.0 : -1.0) * fm / s);
      ans = xnew;
      fnew = eval_at(w, ans, idx, dq, q);
      if (std::fabs(fnew) < TOL && fnew >= 0.0) return xnew;
      if (World::sign2(fm, fnew) != fm) { xl = xm; fl = fm; xh = ans; fh = fnew; }
      else if (World::sign2(fl, fnew) != fl) { xh = ans; fh = fnew; }
      else if (World::sign2(fh, fnew) != fh) { xl = ans; fl = fnew; }
    }
  } else {
    if (fl == 0.0) return x1;
    if (fh == 0.0) return x2;
  }
  return 0.0;
}
bool update_q(World& w, const std::vector<double>& dq, std::vector<double>& q)
{
  std::vector<double> uC, uC_old, qstar(q.size());
  eval_unilateral(w, uC_old);
  for (size_t k = 0; k < q.size(); k++) { qstar[k] = dq[k]; qstar[k] = qstar[k] + q[k]; }
  w.set_q(qstar);
  eval_unilateral(w, uC);
  std::vector<char> br(uC.size(), 0);
  for (size_t i = 0; i < uC.size(); i++)
    br[i] = ((uC_old[i] < 0.0 && uC[i] > 0.0) || (uC_old[i] > 0.0 && uC[i] < 0.0)) ? 1 : 0;
  double t = 1.0;
  for (size_t i = 0; i < br.size(); i++) {
    if (!br[i]) continue;
    const double root = ridders(w, 0, t, uC_old[i], uC[i], (unsigned)i, dq, q);
    if (root > 0.0 && root < 1.0) t = (root < t) ? root : t;
  }
  for (size_t k = 0; k < q.size(); k++) { qstar[k] = dq[k] * t; qstar[k] = qstar[k] + q[k]; }
  w.set_q(qstar);
  eval_unilateral(w, uC);
  const double BETA = 0.6;
  while (true) {
    bool stop = true;
    for (size_t i = 0; i < br.size(); i++) if (!br[i] && uC[i] < 0.0 && uC_old[i] > uC[i]) { stop = false; break; }
    if (stop) break;                                                // (no joints: cvio = 0 < bilateral_eps)
    t *= BETA;
    if (t < NEAR_ZERO) return false;
    for (size_t k = 0; k < q.size(); k++) { qstar[k] = dq[k] * t; qstar[k] = qstar[k] + q[k]; }
    w.set_q(qstar);
    eval_unilateral(w, uC);
  }
  q = qstar;
  return true;
}
void stabilize(World& w)
{
  const SceneView* sc = w.sc;
  if (sc->cstab_max_iterations == 0) return;
  const int nb = sc->nb;
  double* st = w.st;
  std::vector<double> vsave_v(6 * (size_t)nb);
  double (*vsave)[6] = reinterpret_cast<double (*)[6]>(vsave_v.data());
  for (int b = 0; b < nb; b++) for (int k = 0; k < 6; k++) vsave[b][k] = st[13*b + 7 + k];
  std::vector<double> q; w.get_q(q);
  std::vector<double> uC;
  double max_uvio = eval_unilateral(w, uC);
  unsigned iterations = 0;
  while (max_uvio < sc->cstab_eps) {
    if (iterations == sc->cstab_max_iterations) break;
    if (iterations == MH_CSTAB_HARD_CAP) { w.aux->status |= MH_WORLD_STALLED; break; }
    for (int b = 0; b < nb; b++) for (int k = 0; k < 6; k++) st[13*b + 7 + k] = 0.0;
    std::vector<int> cpairs; broad_phase(w, 0.0, cpairs);
    std::vector<Contact> cs;
    for (int p : cpairs) {
      const PairDist d = signed_dist(w, p);
      if (d.dist >= NEAR_ZERO) {
        Contact c; c.pair = p; c.g1 = d.a; c.g2 = d.b; c.p = d.pa;
        const V3 nn = d.pb - d.pa;
        c.n = nn / norm(nn);
        c.dist = d.dist;
        World::orthonormal_basis(c.n, c.s, c.t); w.fill_params(c);
        cs.push_back(c);
      } else find_contacts(w, p, NEAR_ZERO, cs);
    }
    std::vector<World::Island> islands; w.find_islands(cs, islands);
    std::vector<double> dq(q.size(), 0.0);
    for (const World::Island& isl : islands) {
      World::ProblemData pd;
      w.compute_problem_data(cs, isl, pd, true);
      const int nc = pd.nc;
      for (int i = 0; i < nc; i++) pd.Cv[0][i] = pd.c[i]->dist - std::fabs(sc->cstab_eps) - NEAR_ZERO;
      if (nc > w.lcp_cap_) { w.aux->status |= MH_WORLD_UNSUPPORTED; continue; }
      std::vector<double> MM((size_t)nc * nc);
      for (int i = 0; i < nc; i++) for (int j = 0; j < nc; j++) MM[(size_t)i + (size_t)nc * j] = pd.G[0][0][(size_t)i * nc + j];
      Vec z;
      oracle_rand_t rs; std::memcpy(&rs, w.aux->rng, sizeof(rs));
      LCP lcp; lcp.rng = &rs;
      Trace tr; tr.buf = nullptr; tr.cap = 0;
      lcp.trace = &tr;
      unsigned piv = 0;
      bool ok = lcp.lcp_fast(nc, MM.data(), nc, pd.Cv[0].data(), z, -1.0);
      piv += lcp.pivots;
      if (!ok) { ok = lcp.lcp_lemke_regularized(nc, MM.data(), nc, pd.Cv[0].data(), z); piv += lcp.pivots; }
      std::memcpy(w.aux->rng, &rs, sizeof(rs));
      w.lcp_account(nc, piv); w.aux->stab_rows += (unsigned long long)nc;
      for (int i = 0; i < nc; i++) pd.cn[i] = (i < (int)z.size()) ? z[i] : 0.0;
      pd.XJ[1].clear(); pd.XJ[2].clear();
      w.apply_impulses(pd);
      for (int b : pd.bodies) { double qd[7]; w.euler_vel(b, qd); for (int k = 0; k < 7; k++) dq[7*b + k] = qd[k]; }
    }
    if (!update_q(w, dq, q)) { w.aux->status |= MH_WORLD_STAB_FAILED; break; }
    max_uvio = eval_unilateral(w, uC);
    iterations++;
    w.aux->stab_iters++;
  }
  for (int b = 0; b < nb; b++) for (int k = 0; k < 6; k++) st[13*b + 7 + k] = vsave[b][k];
}

void step(World& w, double dt, Census* cen, const Forcing* fo, double* rows, int* shape)
{
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;                   // passed over: the rows stay zero
  broad_phase(w, dt, w.pairs_to_check);
  calc_pairwise_distances(w, w.pairs_to_check, w.pairwise);
  double h = 0.0;
  unsigned guard = 0;
  while (h < dt) {
    h += do_mini_step(w, dt - h, cen, fo, rows, shape);
    if (w.thrown_) return;
    if (++guard > 100000u) { w.aux->status |= MH_WORLD_STALLED; break; }
  }
  stabilize(w);
  w.aux->steps++;
}

// the view World steps: the scene's members with the pair arrays read triangularly over nb + has_ground + n bodies
struct View {
  std::vector<int> pa, pb; SceneView v;
  View(const mh_scene* s, const mh_world_statics* st) {
    const int ntot = s->nb + (s->has_ground ? 1 : 0) + st->n;
    for (int i = 0; i < ntot; i++) for (int j = i + 1; j < ntot; j++) { pa.push_back(i); pb.push_back(j); }
    v = SceneView{ s->nb, s->has_ground, s->geom_type, s->geom_dim, s->mass, s->inertia, s->plane_R, s->plane_o, s->gravity,
                   (int)pa.size(), pa.data(), pb.data(), nullptr,
                   s->pair_enabled, s->cp_epsilon, s->cp_mu_coulomb, s->cp_mu_viscous, s->cp_compliance, s->cp_nk,
                   s->min_step_size, s->contact_dist_thresh, s->cstab_eps, s->cstab_max_iterations,
                   0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
  }
};
const mh_world_statics g_none = {};

}  // namespace

extern "C" {

// B worlds x nsteps steps, in place.  statics: NULL = none.  traj: B x nsteps x nb x 7 or NULL; census: B x nsteps x 5 ints (face, edge, vertex,
// penetrating, none) or NULL; forces, wrench (HOST array rows x B x nb x 6): both NULL = the oracle's own forward dynamics, otherwise the restated one
// (forces with terms == 0 included); report: B x nsteps x npt x MH_REPORT_PAIR (written whole: zero rows first) or NULL; shape: B x nsteps x 6 ints
// (zeroed here; filled only beside a report) or NULL
void world_ref_step(const mh_scene* sc, const mh_world_statics* statics, int B, double dt, int nsteps, double* state, mh_world_aux* aux, double* traj,
                    int* census, const mh_world_forces* forces, const double* wrench, int rows, double* report, int* shape)
{
  g_st = statics ? statics : &g_none; g_hg = sc->has_ground ? 1 : 0;
  const View view(sc, g_st);
  const int npt = view.v.npairs;
  const bool forced = forces || wrench;
  if (report) for (size_t i = 0; i < (size_t)B * nsteps * npt * MH_REPORT_PAIR; i++) report[i] = 0.0;
  if (shape) for (size_t i = 0; i < (size_t)B * nsteps * SH_COUNT; i++) shape[i] = 0;
  for (int b = 0; b < B; b++) {
    double* st = state + (size_t)b * sc->nb * MH_BODY_STATE;
    World w(view.v, st, aux + b, aux[b].zlast, aux[b].zbuf, MH_LCP_MAX_N_WAVE);
    for (int s = 0; s < nsteps; s++) {
      Census cen = { census ? census + ((size_t)b * nsteps + s) * 5 : nullptr };
      const Forcing fo = { forces, wrench, rows, B, b, s };
      step(w, dt, census ? &cen : nullptr, forced ? &fo : nullptr, report ? report + ((size_t)b * nsteps + s) * npt * MH_REPORT_PAIR : nullptr,
           shape ? shape + ((size_t)b * nsteps + s) * SH_COUNT : nullptr);
      if (traj) for (int k = 0; k < sc->nb; k++) for (int i = 0; i < 7; i++) traj[(((size_t)b * nsteps + s) * sc->nb + k) * 7 + i] = st[13*k + i];
    }
  }
}

// probe: the contact of a box (centre cb, axes R row-major, edge lengths len) and a sphere (centre cS, radius Rs) within TOL.
// out[0] = has, out[1] = dist (set either way), out[2..4] = point, out[5..7] = normal, out[8] = region (0 face, 1 edge, 2 vertex, 3 centre inside)
void world_ref_box_contact(const double* cb, const double* R, const double* len, const double* cS, double Rs, double TOL, double* out)
{
  const BspContact c = bsp_contact(R, v3(cb[0], cb[1], cb[2]), len, v3(cS[0], cS[1], cS[2]), Rs, TOL);
  out[0] = c.has; out[1] = c.dist; out[2] = c.p.x; out[3] = c.p.y; out[4] = c.p.z; out[5] = c.n.x; out[6] = c.n.y; out[7] = c.n.z; out[8] = c.region;
}
// probe: the signed distance with both points.  out[0] = dist, out[1..3] = the box point, out[4..6] = the sphere point
void world_ref_box_dist(const double* cb, const double* R, const double* len, const double* cS, double Rs, double* out)
{
  V3 pA, pB;
  out[0] = bsp_sdist(R, v3(cb[0], cb[1], cb[2]), len, v3(cS[0], cS[1], cS[2]), Rs, pA, pB);
  out[1] = pA.x; out[2] = pA.y; out[3] = pA.z; out[4] = pB.x; out[5] = pB.y; out[6] = pB.z;
}
// the axes of a free box body with quaternion xyzw q, as the stepper forms them: World::rot
static void body_axes(const double* cb, const double* q, double R[9])
{
  mh_scene sc; std::memset(&sc, 0, sizeof(sc)); sc.nb = 1;
  double st[13] = { cb[0], cb[1], cb[2], q[0], q[1], q[2], q[3], 0, 0, 0, 0, 0, 0 };
  mh_world_aux aux; std::memset(&aux, 0, sizeof(aux));
  World w(&sc, st, &aux);
  w.rot(0, R);
}
// the two probes above over a box body's pose (centre cb, quaternion xyzw q)
void world_ref_contact(const double* cb, const double* q, const double* len, const double* cS, double Rs, double TOL, double* out)
{
  double R[9]; body_axes(cb, q, R);
  world_ref_box_contact(cb, R, len, cS, Rs, TOL, out);
}
void world_ref_dist(const double* cb, const double* q, const double* len, const double* cS, double Rs, double* out)
{
  double R[9]; body_axes(cb, q, R);
  world_ref_box_dist(cb, R, len, cS, Rs, out);
}
// probe: pair p of a scene with statics in a given state, as the stepper reads it.  out[0] = dist, out[1..3] = pa (body a = the lower index),
// out[4..6] = pb, out[7] = a, out[8] = b; contacts (TOL): out[9] = their number, then of the first out[10] = g1, out[11] = g2, out[12] = dist,
// out[13..15] = point, out[16..18] = normal; out[19] = 1 if the broad phase (dt = 0) keeps the pair
void world_ref_pair(const mh_scene* sc, const mh_world_statics* statics, const double* state, int p, double TOL, double* out)
{
  g_st = statics ? statics : &g_none; g_hg = sc->has_ground ? 1 : 0;
  const View view(sc, g_st);
  std::vector<double> st(state, state + (size_t)sc->nb * MH_BODY_STATE);
  mh_world_aux aux; std::memset(&aux, 0, sizeof(aux));
  World w(view.v, st.data(), &aux, aux.zlast, aux.zbuf, MH_LCP_MAX_N_WAVE);
  const PairDist d = signed_dist(w, p);
  out[0] = d.dist; out[1] = d.pa.x; out[2] = d.pa.y; out[3] = d.pa.z; out[4] = d.pb.x; out[5] = d.pb.y; out[6] = d.pb.z; out[7] = d.a; out[8] = d.b;
  std::vector<Contact> cs; find_contacts(w, p, TOL, cs);
  out[9] = (double)cs.size();
  for (int k = 10; k < 20; k++) out[k] = 0.0;
  if (!cs.empty()) { const Contact& c = cs[0]; out[10] = c.g1; out[11] = c.g2; out[12] = c.dist; out[13] = c.p.x; out[14] = c.p.y; out[15] = c.p.z; out[16] = c.n.x; out[17] = c.n.y; out[18] = c.n.z; }
  std::vector<int> pairs; broad_phase(w, 0.0, pairs);
  for (int q : pairs) if (q == p) out[19] = 1.0;
}

}  // extern "C"
