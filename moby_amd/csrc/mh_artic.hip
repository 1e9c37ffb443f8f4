// mh_artic.hip -- the C entry points of the articulated stepper (include/moby_hip_artic.h) and the code object of its undriven angle-coordinate
// kernels without link geometry beyond spheres (mh_artic_dev.h with no switch set).
//
// mh_artic_batch_step launches those kernels itself, hands a batch in pose coordinates to mh_artic_pose.hip and one whose step goes through a
// geometry family to artic_geom_step below, the one router to the twelve geometry code objects (mh_artic_{box,pair,bsp,rp,pw,wr}[_pose].hip);
// mh_artic_batch_step_driven (mh_artic_drive.hip) calls the same router, and so do mh_artic_batch_step_report, with the rows, and mh_artic_batch_step_wrench, with the wrench.
#include "mh_artic_dev.h"
#include <cstdarg>
#include <cstdio>

// Every step of a batch whose family (artic_geom_family) is box, pair or box-sphere, undriven and driven: the family's checks, then the launcher
// of that family in the batch's coordinates.  To add a family: its switch and token in two wrapper files, an enumerator, its precedence in
// mh_artic_batch_create, and a case here.
int artic_geom_step(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D, double* report, const mh_artic_wrench* wrench)
{
  namespace ar = mh::artic;
  const bool pose = ab->base_coords == MH_ARTIC_BASE_POSE;
  const mh_artic_family fam = artic_geom_family(ab);
  if (fam == MH_ARTIC_FAM_WR) {                                    // link wrenches: the per-world-parameters kernels with the wrench, the same workspace and image
    if (!ab->d_ws || ab->ws_stride < ar::WS_PAIR) return fail(MH_ERR_INVALID_ARG, "the batch's workspace is not sized for the link-wrench kernels");
    const size_t lds = pose ? artic_wr_pose_lds_bytes(ab->nj) : artic_wr_lds_bytes(ab->nj);
    if (lds > 65536) return fail(MH_ERR_INVALID_ARG, "the link-wrench kernels' LDS image (%zu bytes) exceeds a workgroup's 64 KB", lds);
    return pose ? artic_wr_pose_launch(ab, stream, dt, nsteps, D, report, wrench) : artic_wr_launch(ab, stream, dt, nsteps, D, report, wrench);
  }
  if (fam == MH_ARTIC_FAM_PW) {                                    // per-world parameters: the report kernels over B images, an LDS image of their own
    if (!ab->d_ws || ab->ws_stride < ar::WS_PAIR) return fail(MH_ERR_INVALID_ARG, "the batch's workspace is not sized for the per-world-parameters kernels");
    const size_t lds = pose ? artic_pw_pose_lds_bytes(ab->nj) : artic_pw_lds_bytes(ab->nj);
    if (lds > 65536) return fail(MH_ERR_INVALID_ARG, "the per-world-parameters kernels' LDS image (%zu bytes) exceeds a workgroup's 64 KB", lds);
    return pose ? artic_pw_pose_launch(ab, stream, dt, nsteps, D, report) : artic_pw_launch(ab, stream, dt, nsteps, D, report);
  }
  if (fam == MH_ARTIC_FAM_RP) {                                    // the report kernels: the pair workspace, an LDS image of their own
    if (!ab->d_ws || ab->ws_stride < ar::WS_PAIR) return fail(MH_ERR_INVALID_ARG, "the batch's workspace is not sized for the report kernels");
    const size_t lds = pose ? artic_rp_pose_lds_bytes(ab->nj) : artic_rp_lds_bytes(ab->nj);
    if (lds > 65536) return fail(MH_ERR_INVALID_ARG, "the report kernels' LDS image (%zu bytes) exceeds a workgroup's 64 KB", lds);
    return pose ? artic_rp_pose_launch(ab, stream, dt, nsteps, D, report) : artic_rp_launch(ab, stream, dt, nsteps, D, report);
  }
  if (fam == MH_ARTIC_FAM_BOX) {
    if (ab->d_ws && ab->ws_stride < ar::WS_BOX)                  // a sphere batch created before mh_debug_set(12, 1): its workspace has the sphere kernels' layout
      return fail(MH_ERR_INVALID_ARG, "mh_debug_set(12, 1) applies to batches created after it (their workspace is sized for the box kernels at create)");
    return pose ? artic_box_pose_launch(ab, stream, dt, nsteps, D) : artic_box_launch(ab, stream, dt, nsteps, D);
  }
  // pair and box-sphere: one workspace layout and one LDS image (the angle-coordinate pair layout's, as mh_artic_batch_create checks it)
  const bool bsp = fam == MH_ARTIC_FAM_BSP;
  const char* name = bsp ? "box-sphere" : "pair";
  if (ab->d_ws && ab->ws_stride < ar::WS_PAIR) return fail(MH_ERR_INVALID_ARG, "the batch's workspace is not sized for the %s kernels", name);
  const size_t lds = artic_pair_lds_bytes(ab->nj);
  if (lds > 65536) return fail(MH_ERR_INVALID_ARG, "the %s kernels' LDS image (%zu bytes) exceeds a workgroup's 64 KB", name, lds);
  if (bsp) return pose ? artic_bsp_pose_launch(ab, stream, dt, nsteps, D) : artic_bsp_launch(ab, stream, dt, nsteps, D);
  return pose ? artic_pair_pose_launch(ab, stream, dt, nsteps, D) : artic_pair_launch(ab, stream, dt, nsteps, D);
}

extern "C" {

int mh_artic_batch_device(const mh_artic_batch* ab) { return ab ? ab->device : fail(MH_ERR_INVALID_ARG, "null batch"); }

int mh_artic_batch_destroy(mh_artic_batch* ab)
{
  if (!ab) return MH_OK;
  MH_ON_DEVICE(ab);
  (void)hipDeviceSynchronize();
  void* ps[] = { ab->d_model, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws, ab->d_drive, ab->d_pose };
  for (void* p : ps) if (p) (void)hipFree(p);
  delete ab;
  return MH_OK;
}

int mh_artic_report_slots(const mh_artic_model* model)
{
  if (!model) return fail(MH_ERR_INVALID_ARG, "null model");
  if (model->nspheres < 0 || model->nspheres > MH_ARTIC_MAX_SPHERES || model->nboxes < 0 || model->nboxes > MH_ARTIC_MAX_BOXES || model->npairs < 0 || model->npairs > MH_ARTIC_MAX_PAIRS)
    return fail(MH_ERR_INVALID_ARG, "nspheres = %d, nboxes = %d, npairs = %d outside [0, %d], [0, %d], [0, %d]", model->nspheres, model->nboxes, model->npairs,
                MH_ARTIC_MAX_SPHERES, MH_ARTIC_MAX_BOXES, MH_ARTIC_MAX_PAIRS);
  return model->nspheres + model->nboxes + model->npairs;
}

// A refusal of artic_check_model: the message as it is for the shared model (world < 0), with the world in front for a record
static int refuse(int world, const char* fmt, ...)
{
  char buf[512];
  va_list ap; va_start(ap, fmt); std::vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  return world < 0 ? fail(MH_ERR_INVALID_ARG, "%s", buf) : fail(MH_ERR_INVALID_ARG, "world %d: %s", world, buf);
}

// the fields of mh_artic_params, each with the model's name, type and extent
#define MH_ARTIC_PARAM_FIELDS(X) X(Rrel) X(trel) X(axis) X(com) X(inertia) X(mass) X(lolimit) X(hilimit) X(limit_restitution) X(gravity) \
  X(sphere_center) X(sphere_radius) X(plane_R) X(plane_o) X(cp_epsilon) X(cp_mu_coulomb) X(cp_mu_viscous) X(cp_compliance) X(box_center) X(box_R) X(box_len)
// record r written into model m (the topology stays m's)
static void params_into_model(const mh_artic_params& r, mh_artic_model& m)
{
#define X(f) static_assert(sizeof(m.f) == sizeof(r.f), #f); std::memcpy(&m.f, &r.f, sizeof(r.f));
  MH_ARTIC_PARAM_FIELDS(X)
#undef X
}

struct ArticPlan { bool use_rp, use_bsp, use_pair; };   // the family decisions of the model's checks
// Every check of mh_artic_batch_create, and the device image of a model: ONE text for the shared model (world < 0, base NULL) and for "the model
// with record w written into it" (world = w, base = the shared model), so a record is validated as the model's values are and its image is filled
// as the shared one is.  report: the batch is a report batch; params: it holds an image per world (mh_artic_batch_create_params), which steps
// through the per-world-parameters family whatever its geometry, with cp_nk checked and the friction polygon filled whatever cp_mu_coulomb
static int artic_check_model(const mh_artic_model* model, bool report, bool params, int world, const mh_artic_model* base, mh::artic::Model& hm, ArticPlan& plan)
{
  namespace ar = mh::artic;
  const int nj = model->nj;
  if (nj < 1 || nj > MH_ARTIC_MAX_JOINTS) return refuse(world, "nj = %d outside [1, %d]", nj, MH_ARTIC_MAX_JOINTS);
  std::memset(&hm, 0, sizeof(hm)); hm.m = *model;
  std::memset(hm.anc, 0, sizeof(hm.anc)); std::memset(hm.fcos, 0, sizeof(hm.fcos)); std::memset(hm.fsin, 0, sizeof(hm.fsin));   // (they overlay m's box block: bx holds it)
  for (int i = 0; i < nj; i++) {
    const int p = model->parent[i];
    if (p >= i || p < -1) return refuse(world, "joint %d: parent %d must come before it (-1 = base)", i, p);
    if (model->jtype[i] != MH_JOINT_REVOLUTE && model->jtype[i] != MH_JOINT_PRISMATIC) return refuse(world, "joint %d: type %d is not built (revolute, prismatic)", i, model->jtype[i]);
    if (!(model->mass[i] >= 0.0)) return refuse(world, "link %d: mass must be >= 0", i);
    const double* a = model->axis[i]; const double nn = a[0]*a[0] + a[1]*a[1] + a[2]*a[2];
    if (!(nn > 0.999999 && nn < 1.000001)) return refuse(world, "joint %d: axis is not a unit vector", i);
    if (!(model->lolimit[i] <= model->hilimit[i])) return refuse(world, "joint %d: lower limit above the upper one", i);
    hm.anc[i] = (1u << i) | (p >= 0 ? hm.anc[p] : 0u);
  }
  if (model->floating_base != 0 && model->floating_base != 1) return refuse(world, "floating_base = %d: 0 or 1", model->floating_base);
  if (model->floating_base) {                                        // the layout include/moby_hip_artic.h states (conservative advancement reads joints 0..2 as the base's velocity)
    if (nj < 6) return refuse(world, "floating_base needs the six virtual joints in front (nj = %d)", nj);
    for (int v = 0; v < 6; v++) {
      bool ok = model->parent[v] == v - 1 && model->jtype[v] == ((v < 3) ? MH_JOINT_PRISMATIC : MH_JOINT_REVOLUTE);
      for (int k = 0; k < 3; k++) ok = ok && model->axis[v][k] == ((k == v % 3) ? 1.0 : 0.0) && model->com[v][k] == 0.0 && (v == 0 || model->trel[v][k] == 0.0);
      for (int k = 0; k < 9; k++) ok = ok && (v == 3 || model->Rrel[v][k] == ((k % 4 == 0) ? 1.0 : 0.0));
      if (!ok) return refuse(world, "floating_base: joint %d is not the virtual joint the layout states (sliders along global x, y, z, then hinges about the base link's x, y, z through its COM)", v);
    }
  }
  // a link may be massless (the virtual links under a floating base, mh_io_load_xml_artic) as long as every joint moves mass: the composite inertia outboard of it
  { double sub[MH_ARTIC_MAX_JOINTS];
    for (int i = 0; i < nj; i++) sub[i] = model->mass[i];
    for (int i = nj - 1; i >= 0; i--) { if (!(sub[i] > 0.0)) return refuse(world, "joint %d carries no mass (its link and everything outboard of it are massless)", i); if (model->parent[i] >= 0) sub[model->parent[i]] += sub[i]; } }
  if (model->nspheres < 0 || model->nspheres > MH_ARTIC_MAX_SPHERES) return refuse(world, "nspheres = %d outside [0, %d]", model->nspheres, MH_ARTIC_MAX_SPHERES);
  for (int s = 0; s < model->nspheres; s++) {
    if (model->sphere_link[s] < 0 || model->sphere_link[s] >= nj) return refuse(world, "sphere %d: link %d outside [0, %d)", s, model->sphere_link[s], nj);
    if (!(model->sphere_radius[s] > 0.0)) return refuse(world, "sphere %d: radius must be > 0", s);
  }
  if (model->nboxes < 0 || model->nboxes > MH_ARTIC_MAX_BOXES) return refuse(world, "nboxes = %d outside [0, %d]", model->nboxes, MH_ARTIC_MAX_BOXES);
  for (int k = 0; k < model->nboxes; k++) {
    if (model->box_link[k] < -1 || model->box_link[k] >= nj) return refuse(world, "box %d: link %d outside [-1, %d) (-1 = a static box)", k, model->box_link[k], nj);
    for (int c = 0; c < 3; c++) if (!(model->box_len[k][c] > 0.0) || !std::isfinite(model->box_len[k][c])) return refuse(world, "box %d: edge lengths must be finite and > 0", k);
    const double* Rb = model->box_R[k];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) {       // R R' = I
      const double d = (Rb[3*i] * Rb[3*j] + Rb[3*i+1] * Rb[3*j+1]) + Rb[3*i+2] * Rb[3*j+2];
      if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) < 1e-9)) return refuse(world, "box %d: box_R is not orthonormal", k);
    }
    hm.bx.link[k] = model->box_link[k];
    for (int c = 0; c < 3; c++) { hm.bx.center[k][c] = model->box_center[k][c]; hm.bx.len[k][c] = model->box_len[k][c]; }
    for (int c = 0; c < 9; c++) hm.bx.R[k][c] = Rb[c];
  }
  hm.bx.n = model->nboxes;
  int nstatic = 0;
  for (int k = 0; k < model->nboxes; k++) if (model->box_link[k] < 0) nstatic++;
  // sphere pairs between links
  if (model->npairs < 0 || model->npairs > MH_ARTIC_MAX_PAIRS) return refuse(world, "npairs = %d outside [0, %d]", model->npairs, MH_ARTIC_MAX_PAIRS);
  for (int k = 0; k < model->npairs; k++) {
    const int a = model->pair_a[k], b = model->pair_b[k], kind = model->pair_kind[k];
    if (kind != MH_ARTIC_PAIR_SPHERES && kind != MH_ARTIC_PAIR_BOX_SPHERE) return refuse(world, "pair %d: kind %d is not built (0 = two spheres, 1 = a box and a sphere)", k, kind);
    hm.pr.kind[k] = kind;
    if (kind == MH_ARTIC_PAIR_BOX_SPHERE) {
      if (a < 0 || a >= model->nboxes) return refuse(world, "pair %d: box %d outside the box list [0, %d)", k, a, model->nboxes);
      if (b < 0 || b >= model->nspheres) return refuse(world, "pair %d: sphere %d outside the sphere list [0, %d)", k, b, model->nspheres);
      if (model->box_link[a] == model->sphere_link[b]) return refuse(world, "pair %d: box %d and sphere %d sit on the same link %d", k, a, b, model->box_link[a]);
      for (int k2 = 0; k2 < k; k2++)
        if (model->pair_kind[k2] == kind && model->pair_a[k2] == a && model->pair_b[k2] == b) return refuse(world, "pair %d: box %d and sphere %d are pair %d already", k, a, b, k2);
      hm.pr.a[k] = a; hm.pr.b[k] = b;
      continue;
    }
    if (a < 0 || a >= model->nspheres || b < 0 || b >= model->nspheres) return refuse(world, "pair %d: spheres (%d, %d) outside the sphere list [0, %d)", k, a, b, model->nspheres);
    if (a == b) return refuse(world, "pair %d: sphere %d against itself", k, a);
    if (model->sphere_link[a] == model->sphere_link[b]) return refuse(world, "pair %d: spheres %d and %d sit on the same link %d", k, a, b, model->sphere_link[a]);
    for (int k2 = 0; k2 < k; k2++)
      if (model->pair_kind[k2] == kind && ((model->pair_a[k2] == a && model->pair_b[k2] == b) || (model->pair_a[k2] == b && model->pair_b[k2] == a))) return refuse(world, "pair %d: spheres (%d, %d) are pair %d already", k, a, b, k2);
    hm.pr.a[k] = a; hm.pr.b[k] = b;
  }
  if (model->sphere_no_plane < 0 || (model->sphere_no_plane >> model->nspheres) != 0) return refuse(world, "sphere_no_plane = 0x%x has bits beyond the %d spheres", (unsigned)model->sphere_no_plane, model->nspheres);
  hm.pr.n = model->npairs; hm.pr.no_plane = model->sphere_no_plane; hm.pr.nstatic = nstatic;
  bool has_bsp = false;
  for (int k = 0; k < model->nboxes; k++) {
    if (model->box_link[k] >= 0) continue;
    bool paired = false;
    for (int k2 = 0; k2 < model->npairs; k2++) paired = paired || (model->pair_kind[k2] == MH_ARTIC_PAIR_BOX_SPHERE && model->pair_a[k2] == k);
    if (!paired) return refuse(world, "box %d is static (link -1) and appears in no box-sphere pair", k);
  }
  for (int k = 0; k < model->npairs; k++) has_bsp = has_bsp || model->pair_kind[k] == MH_ARTIC_PAIR_BOX_SPHERE;
  const bool has_geom = model->nspheres > 0 || model->nboxes > 0;
  const bool use_bsp = plan.use_bsp = has_bsp || nstatic > 0 || (has_geom && mh_g_debug_artic_bsp != 0);
  const bool use_rp = plan.use_rp = report || (use_bsp && mh_g_debug_artic_rp != 0);          // the report kernels hold all the work of the box-sphere kernels
  if (report && model->nspheres + model->nboxes + model->npairs == 0) return refuse(world, "a contact report needs geometry: the model has no sphere, box or pair (no slot)");
  const bool use_pair = plan.use_pair = params || use_rp || use_bsp || model->npairs > 0 || model->sphere_no_plane != 0 || (has_geom && mh_g_debug_artic_pair != 0);
  if (use_pair && !use_rp && !params && artic_pair_lds_bytes(nj) > 65536) return refuse(world, "the pair kernels' LDS image at %d joints (%zu bytes) exceeds a workgroup's 64 KB", nj, artic_pair_lds_bytes(nj));
  if (params || (use_rp && mh_g_debug_artic_pw != 0)) {             // the per-world-parameters family's image, in either coordinates
    const size_t lds = artic_pw_pose_lds_bytes(nj) > artic_pw_lds_bytes(nj) ? artic_pw_pose_lds_bytes(nj) : artic_pw_lds_bytes(nj);
    if (lds > 65536) return refuse(world, "the per-world-parameters kernels' LDS image at %d joints (%zu bytes) exceeds a workgroup's 64 KB", nj, lds);
  } else if (use_rp) {                                              // this family's own image, in either coordinates (the batch may be switched to poses later)
    const size_t lds = artic_rp_pose_lds_bytes(nj) > artic_rp_lds_bytes(nj) ? artic_rp_pose_lds_bytes(nj) : artic_rp_lds_bytes(nj);
    if (lds > 65536) return refuse(world, "the report kernels' LDS image at %d joints (%zu bytes) exceeds a workgroup's 64 KB", nj, lds);
  }
  if (model->cstab_max_iterations < 0) return refuse(world, "cstab_max_iterations = %d < 0", model->cstab_max_iterations);
  if (model->nspheres > 0 || model->nboxes > 0) {
    const double* Rp = model->plane_R; const double nn = Rp[1]*Rp[1] + Rp[4]*Rp[4] + Rp[7]*Rp[7];
    if (!(nn > 0.999999 && nn < 1.000001)) return refuse(world, "plane_R is not a rotation (its +Y column is the plane normal)");
    if (!(model->min_step_size > 0.0) || !(model->contact_dist_thresh > 0.0)) return refuse(world, "min_step_size and contact_dist_thresh must be > 0 when spheres or boxes are present");
    if (!(model->cp_epsilon >= 0.0) || !(model->cp_mu_coulomb >= 0.0)) return refuse(world, "contact parameters must be >= 0");
    if (params || !(model->cp_mu_coulomb >= 1e2)) {               // the Drumwright-Shell model's parameters (per-world parameters: worlds on either side of 100 may share the batch)
      const int nk = model->cp_nk > 0 ? model->cp_nk : 4;
      if (nk < 4 || nk > 64 || (nk & 1)) return refuse(world, "cp_nk = %d: friction-cone-edges must be even, in [4, 64]", nk);
      if (!(model->cp_mu_viscous >= 0.0) || !(model->cp_compliance >= 0.0)) return refuse(world, "contact parameters must be >= 0");
      const int kh = nk / 2;
      for (int j = 0; j < kh; j++) { const double theta = (double)j / (kh - 1) * M_PI_2; hm.fcos[j] = std::cos(theta); hm.fsin[j] = std::sin(theta); }
    }
  }
  if (base) {                                                       // a record's own rules: it moves values, never the model's decisions
    const double INF_ = 1.7976931348623157e308;
    for (int i = 0; i < nj; i++) {
      if ((model->lolimit[i] > -INF_) != (base->lolimit[i] > -INF_)) return refuse(world, "joint %d: lolimit is %s where the model's is not (a record may move a finite limit, not add or remove one)", i, model->lolimit[i] > -INF_ ? "finite" : "infinite");
      if ((model->hilimit[i] < INF_) != (base->hilimit[i] < INF_)) return refuse(world, "joint %d: hilimit is %s where the model's is not (a record may move a finite limit, not add or remove one)", i, model->hilimit[i] < INF_ ? "finite" : "infinite");
    }
    for (int k = 0; k < 3; k++) if (!std::isfinite(model->gravity[k])) return refuse(world, "gravity is not finite");
    if (model->nspheres > 0 || model->nboxes > 0) {
      const double cp[4] = { model->cp_epsilon, model->cp_mu_coulomb, model->cp_mu_viscous, model->cp_compliance };
      for (int k = 0; k < 4; k++) if (!std::isfinite(cp[k]) || !(cp[k] >= 0.0)) return refuse(world, "contact parameters (cp_epsilon, cp_mu_coulomb, cp_mu_viscous, cp_compliance) must be finite and >= 0");
    }
  }
  return MH_OK;
}

// mh_artic_batch_create (report false) and mh_artic_batch_create_report (true), and mh_artic_batch_create_params (params true; host: B records or
// NULL = the model's): one text, the report and the records only decide the family and the number of images
// (wrench: mh_artic_batch_create_wrench, a params batch whose step goes through the link-wrench family)
static int artic_batch_create(const mh_artic_model* model, int B, mh_artic_batch** out, bool report, bool params = false, const mh_artic_params* host = nullptr, bool wrench = false)
{
  namespace ar = mh::artic;
  if (!out) return fail(MH_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  if (!model) return fail(MH_ERR_INVALID_ARG, "null model");
  if (B <= 0) return fail(MH_ERR_INVALID_ARG, "batch must be > 0");
  ar::Model hm; ArticPlan plan;
  { const int rc = artic_check_model(model, report, false, -1, nullptr, hm, plan); if (rc != MH_OK) return rc; }    // every refusal of mh_artic_batch_create, unchanged
  const bool pw20 = !params && plan.use_rp && mh_g_debug_artic_pw != 0;      // mh_debug_set(20, 1): B images, all the model's
  std::vector<ar::Model> images;
  if (params) {
    images.resize((size_t)B);
    for (int w = 0; w < B; w++) {
      mh_artic_model mw = *model;
      if (host) params_into_model(host[w], mw);
      const int rc = artic_check_model(&mw, report, true, w, model, images[w], plan); if (rc != MH_OK) return rc;
    }
  } else if (pw20) images.assign((size_t)B, hm);
  const size_t nimg = images.empty() ? 1 : (size_t)B;
  const int nj = model->nj;
  const bool use_rp = plan.use_rp, use_bsp = plan.use_bsp, use_pair = plan.use_pair, use_pw = params || pw20;
  const bool use_wr = wrench || (use_pw && mh_g_debug_artic_wr != 0);           // mh_debug_set(21, 1): the link-wrench kernels with a NULL wrench
  if (mh_device_count() <= 0) return fail(MH_ERR_NO_DEVICE, "no HIP device visible");
  { const int rc = init_pow10(); if (rc != MH_OK) return rc; }             // this code object's powers of ten, before its first launch on the device
  mh_artic_batch* ab = new mh_artic_batch();
  if (hipGetDevice(&ab->device) != hipSuccess) { delete ab; return fail(MH_ERR_HIP, "hipGetDevice failed"); }
  ab->B = B; ab->nj = nj; ab->algorithm = model->algorithm; ab->nspheres = model->nspheres; ab->family = use_wr ? MH_ARTIC_FAM_WR : use_pw ? MH_ARTIC_FAM_PW : use_rp ? MH_ARTIC_FAM_RP : use_bsp ? MH_ARTIC_FAM_BSP : use_pair ? MH_ARTIC_FAM_PAIR : model->nboxes > 0 ? MH_ARTIC_FAM_BOX : MH_ARTIC_FAM_NONE; ab->cstab = model->cstab_max_iterations != 0 ? 1 : 0; ab->d_model = nullptr; ab->d_q = nullptr; ab->d_qd = nullptr; ab->d_aux = nullptr; ab->d_ws = nullptr;
  ab->report = report ? 1 : 0; ab->params = params ? 1 : pw20 ? 2 : 0; ab->model = *model; ab->wrench = wrench ? 1 : 0;
  std::memset(&ab->drive, 0, sizeof(ab->drive)); ab->d_drive = nullptr;
  ab->base_coords = MH_ARTIC_BASE_ANGLES; ab->d_pose = nullptr;
  const size_t sB = (size_t)B;
  bool ok = hipMalloc((void**)&ab->d_model, nimg * sizeof(ar::Model)) == hipSuccess && hipMalloc((void**)&ab->d_q, sB * nj * 8) == hipSuccess
         && hipMalloc((void**)&ab->d_qd, sB * nj * 8) == hipSuccess && hipMalloc((void**)&ab->d_aux, sB * sizeof(mh_world_aux)) == hipSuccess;
  // the box kernels' layout for a model with boxes, and for a sphere model created while mh_debug_set(12, 1) sends it to those kernels
  // (and the pair kernels' for a batch that steps through those)
  ab->ws_stride = use_pair ? ar::WS_PAIR : (model->nboxes > 0 || (model->nspheres > 0 && mh_g_debug_artic_box != 0)) ? ar::WS_BOX : 2 * MH_LCP_MAX_N_WAVE * MH_LCP_MAX_N_WAVE;
  if (ok && (use_pw || model->nspheres > 0 || model->nboxes > 0) && (use_pair || !(model->cp_mu_coulomb >= 1e2) || model->cstab_max_iterations != 0))   // (the stabiliser's LCP with contact AND limit rows lives there too)
    ok = hipMalloc((void**)&ab->d_ws, sB * ab->ws_stride * sizeof(double)) == hipSuccess;
  if (ok) {
    std::vector<mh_world_aux> a(sB);
    mh_world_aux_init(&a[0], 1);
    for (int b = 1; b < B; b++) a[b] = a[0];
    ok = hipMemcpy(ab->d_model, images.empty() ? &hm : images.data(), nimg * sizeof(hm), hipMemcpyHostToDevice) == hipSuccess
      && hipMemset(ab->d_q, 0, sB * nj * 8) == hipSuccess && hipMemset(ab->d_qd, 0, sB * nj * 8) == hipSuccess
      && hipMemcpy(ab->d_aux, a.data(), sB * sizeof(mh_world_aux), hipMemcpyHostToDevice) == hipSuccess;
  }
  if (!ok) { mh_artic_batch_destroy(ab); return fail(MH_ERR_HIP, "device allocation / upload failed"); }
  *out = ab;
  return MH_OK;
}

int mh_artic_batch_create(const mh_artic_model* model, int B, mh_artic_batch** out) { return artic_batch_create(model, B, out, false); }
int mh_artic_batch_create_report(const mh_artic_model* model, int B, mh_artic_batch** out) { return artic_batch_create(model, B, out, true); }

void mh_artic_params_from_model(const mh_artic_model* model, mh_artic_params* out)
{
  if (!model || !out) return;
#define X(f) std::memcpy(&out->f, &model->f, sizeof(out->f));
  MH_ARTIC_PARAM_FIELDS(X)
#undef X
}

int mh_artic_batch_create_params(const mh_artic_model* model, const mh_artic_params* host, int B, int flags, mh_artic_batch** out)
{
  if (out) *out = nullptr;
  if (flags & ~MH_ARTIC_CREATE_REPORT) return fail(MH_ERR_INVALID_ARG, "unknown bits 0x%x in flags (MH_ARTIC_CREATE_REPORT or 0)", flags & ~MH_ARTIC_CREATE_REPORT);
  return artic_batch_create(model, B, out, (flags & MH_ARTIC_CREATE_REPORT) != 0, true, host);
}

int mh_artic_batch_create_wrench(const mh_artic_model* model, const mh_artic_params* host, int B, int flags, mh_artic_batch** out)
{
  if (out) *out = nullptr;
  if (flags & ~MH_ARTIC_CREATE_REPORT) return fail(MH_ERR_INVALID_ARG, "unknown bits 0x%x in flags (MH_ARTIC_CREATE_REPORT or 0)", flags & ~MH_ARTIC_CREATE_REPORT);
  return artic_batch_create(model, B, out, (flags & MH_ARTIC_CREATE_REPORT) != 0, true, host, true);
}

// the checks the two record setters share
static int check_params_range(const mh_artic_batch* ab, const void* rec, int first, int count)
{
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  if (ab->params != 1) return fail(MH_ERR_INVALID_ARG, "the batch was not created by mh_artic_batch_create_params: it has no records");
  if (!rec) return fail(MH_ERR_INVALID_ARG, "null records");
  if (first < 0 || count < 0 || first > ab->B || count > ab->B - first) return fail(MH_ERR_INVALID_ARG, "worlds [%d, %d + %d) outside the batch's [0, %d)", first, first, count, ab->B);
  return MH_OK;
}

int mh_artic_batch_set_params(mh_artic_batch* ab, const mh_artic_params* host, int first, int count)
{
  namespace ar = mh::artic;
  { const int rc = check_params_range(ab, host, first, count); if (rc != MH_OK) return rc; }
  std::vector<ar::Model> images((size_t)count);
  ArticPlan plan;
  for (int r = 0; r < count; r++) {                                  // every record before any is written
    mh_artic_model mw = ab->model;
    params_into_model(host[r], mw);
    const int rc = artic_check_model(&mw, ab->report != 0, true, first + r, &ab->model, images[r], plan); if (rc != MH_OK) return rc;
  }
  if (count == 0) return MH_OK;
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());                              // a step may be reading the images on a caller's stream
  MH_HIP(hipMemcpy(ab->d_model + first, images.data(), (size_t)count * sizeof(ar::Model), hipMemcpyHostToDevice));
  return MH_OK;
}

int mh_artic_batch_set_params_dev(mh_artic_batch* ab, void* stream, const mh_artic_params* dev, int first, int count)
{
  { const int rc = check_params_range(ab, dev, first, count); if (rc != MH_OK) return rc; }
  if (count == 0) return MH_OK;
  MH_ON_DEVICE(ab);
  MH_HIP(artic_pw_scatter_launch(ab, stream, dev, first, count));
  return MH_OK;
}

int mh_artic_batch_upload(mh_artic_batch* ab, const double* q, const double* qd, const mh_world_aux* aux)
{
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());                              // a step may be in flight on a caller's non-blocking stream
  const size_t n = (size_t)ab->B * ab->nj * 8;
  if (q) MH_HIP(hipMemcpy(ab->d_q, q, n, hipMemcpyHostToDevice));
  if (qd) MH_HIP(hipMemcpy(ab->d_qd, qd, n, hipMemcpyHostToDevice));
  if (aux) MH_HIP(hipMemcpy(ab->d_aux, aux, (size_t)ab->B * sizeof(mh_world_aux), hipMemcpyHostToDevice));
  return MH_OK;
}

int mh_artic_batch_step(mh_artic_batch* ab, void* stream, double dt, int nsteps)
{
  namespace ar = mh::artic;
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(ab);
  if (nsteps < 0) return fail(MH_ERR_INVALID_ARG, "negative step count");
  if (nsteps == 0) return MH_OK;
  if (!(dt > 0.0)) return fail(MH_ERR_INVALID_ARG, "dt must be > 0");
  if (artic_geom_family(ab) != MH_ARTIC_FAM_NONE) return artic_geom_step(ab, stream, dt, nsteps, nullptr);
  if (ab->base_coords == MH_ARTIC_BASE_POSE) return artic_pose_step(ab, stream, dt, nsteps, nullptr);
  if (ab->nspheres > 0) {                                     // bodies with collision geometry: the full step with mini-steps and contact rows
    hipLaunchKernelGGL(ab->cstab ? ar::k_artic_step_contacts_stab : ar::k_artic_step_contacts, dim3(ab->B), dim3(64), ar::lds_bytes_contacts(ab->nj), (hipStream_t)stream,
                       (const ar::Model*)ab->d_model, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws);
    MH_HIP(hipGetLastError());
    return MH_OK;
  }
  if (ab->cstab) {
    hipLaunchKernelGGL(ar::k_artic_step_stab, dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj, ar::NLSTAB), (hipStream_t)stream,
                       (const ar::Model*)ab->d_model, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux);
    MH_HIP(hipGetLastError());
    return MH_OK;
  }
  // (off by default: measured on ur10 x 8192 x 200 steps it retires a world-step in 27 % fewer vector and 40 % fewer LDS instructions and takes
  //  27.4 ms against 26.2 -- two images per wave halve the resident waves, and with them what hides the LDS round trips; profiles/r04_a_artic_issue.json)
  static const int pack_env = [] { const char* e = std::getenv("MH_ARTIC_PACK"); return e ? std::atoi(e) : 0; }();
  const int pack = pack_env | mh_g_debug_artic_pack;                 // mh_debug_set(9, 1)
  if (pack != 0 && ab->algorithm == MH_ARTIC_CRB && !std::getenv("MH_ARTIC_WAVES")) {          // two worlds per wavefront (k_artic_step_p2)
    hipLaunchKernelGGL(ar::k_artic_step_p2, dim3((ab->B + 1) / 2), dim3(64), 2 * ar::lds_bytes(ab->nj), (hipStream_t)stream,
                       (const ar::Model*)ab->d_model, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux);
    MH_HIP(hipGetLastError());
    return MH_OK;
  }
  static const int waves = [] { const char* e = std::getenv("MH_ARTIC_WAVES"); const int w = e ? std::atoi(e) : 4; return (w == 2 || w == 3 || w == 5) ? w : 4; }();
  hipLaunchKernelGGL(waves == 5 ? ar::k_artic_step_w5 : waves == 4 ? ar::k_artic_step_w4 : (waves == 2 ? ar::k_artic_step_w2 : ar::k_artic_step_w3), dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)stream,
                     (const ar::Model*)ab->d_model, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

int mh_artic_batch_step_report(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* drive, double* report_dev)
{
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  if (!report_dev) return mh_artic_batch_step_driven(ab, stream, dt, nsteps, drive);   // (a report batch launches its kernels with nothing to write)
  if (!ab->report) return fail(MH_ERR_INVALID_ARG, "a report needs a batch created by mh_artic_batch_create_report");
  MH_ON_DEVICE(ab);
  const mh_artic_drive& D = drive ? *drive : ab->drive;
  if (nsteps < 0) return fail(MH_ERR_INVALID_ARG, "negative step count");
  if (D.terms != 0) { const int rc = check_drive(&D, nsteps); if (rc != MH_OK) return rc; }
  if (nsteps == 0) return MH_OK;
  if (!(dt > 0.0)) return fail(MH_ERR_INVALID_ARG, "dt must be > 0");
  return artic_geom_step(ab, stream, dt, nsteps, D.terms != 0 ? &D : nullptr, report_dev);
}

// the checks of a wrench that need no batch (nsteps as check_drive's)
static int check_wrench(const mh_artic_wrench* w, int nsteps)
{
  const int known = MH_LINK_WRENCH | MH_LINK_DAMPING | MH_LINK_WRENCH_LINK_AXES;
  if (w->terms & ~known) return fail(MH_ERR_INVALID_ARG, "wrench: unknown bits 0x%x in terms", w->terms & ~known);
  if ((w->terms & MH_LINK_WRENCH_LINK_AXES) && !(w->terms & MH_LINK_WRENCH)) return fail(MH_ERR_INVALID_ARG, "wrench: terms has MH_LINK_WRENCH_LINK_AXES without MH_LINK_WRENCH");
  if ((w->terms & MH_LINK_WRENCH) && !w->w) return fail(MH_ERR_INVALID_ARG, "wrench: MH_LINK_WRENCH with a NULL w");
  if (w->terms & MH_LINK_DAMPING) {
    const char* name = !w->kl ? "kl" : !w->ka ? "ka" : !w->klsq ? "klsq" : !w->kasq ? "kasq" : nullptr;
    if (name) return fail(MH_ERR_INVALID_ARG, "wrench: MH_LINK_DAMPING with a NULL %s (kl, ka, klsq and kasq are all required)", name);
  }
  if (w->rows < 1) return fail(MH_ERR_INVALID_ARG, "wrench: rows = %d < 1", w->rows);
  if (nsteps >= 0 && w->rows > 1 && w->rows < nsteps) return fail(MH_ERR_INVALID_ARG, "wrench: %d schedule rows for %d steps (1 = held, or at least one per step)", w->rows, nsteps);
  return MH_OK;
}

int mh_artic_batch_step_wrench(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* drive, const mh_artic_wrench* wrench, double* report_dev)
{
  const bool has = wrench && wrench->terms != 0;
  if (has) { const int rc = check_wrench(wrench, nsteps); if (rc != MH_OK) return rc; }       // what needs no batch first, so that it is refused without one
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  if (has && !ab->wrench) return fail(MH_ERR_INVALID_ARG, "wrench: the batch was not created by mh_artic_batch_create_wrench");
  if (report_dev && !ab->report) return fail(MH_ERR_INVALID_ARG, "report_dev: a report needs a batch created with MH_ARTIC_CREATE_REPORT (or by mh_artic_batch_create_report)");
  if (!has) return mh_artic_batch_step_report(ab, stream, dt, nsteps, drive, report_dev);       // the same kernels, a NULL wrench
  const mh_artic_drive& D = drive ? *drive : ab->drive;
  if (nsteps < 0) return fail(MH_ERR_INVALID_ARG, "negative step count");
  if (D.terms != 0) { const int rc = check_drive(&D, nsteps); if (rc != MH_OK) return rc; }
  if (nsteps == 0) return MH_OK;
  if (!(dt > 0.0)) return fail(MH_ERR_INVALID_ARG, "dt must be > 0");
  MH_ON_DEVICE(ab);
  return artic_geom_step(ab, stream, dt, nsteps, D.terms != 0 ? &D : nullptr, report_dev, wrench);
}

int mh_artic_batch_set_drive(mh_artic_batch* ab, const mh_artic_drive* host_drive)
{
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(ab);
  if (host_drive) { const int rc = check_drive(host_drive, -1); if (rc != MH_OK) return rc; }
  MH_HIP(hipDeviceSynchronize());                              // a driven step may be reading the stored arrays on a caller's stream
  if (ab->d_drive) (void)hipFree(ab->d_drive);
  ab->d_drive = nullptr; std::memset(&ab->drive, 0, sizeof(ab->drive));
  if (!host_drive || host_drive->terms == 0) return MH_OK;
  const mh_artic_drive& h = *host_drive;
  const size_t per = (size_t)ab->B * ab->nj, R = (size_t)h.rows;
  const bool pd = (h.terms & MH_DRIVE_PD) != 0, ff = (h.terms & MH_DRIVE_FORCE) != 0;
  const size_t n = (pd ? 2 * per + 2 * R * per : 0) + (ff ? R * per : 0);
  double* d = nullptr;
  MH_HIP(hipMalloc((void**)&d, n * sizeof(double)));
  mh_artic_drive s; std::memset(&s, 0, sizeof(s)); s.terms = h.terms; s.rows = h.rows;
  double* o = d;
  hipError_t e = hipSuccess;
  auto put = [&](const double* src, size_t cnt) -> const double* { double* at = o; o += cnt; if (e == hipSuccess) e = hipMemcpy(at, src, cnt * sizeof(double), hipMemcpyHostToDevice); return at; };
  if (pd) { s.kp = put(h.kp, per); s.kv = put(h.kv, per); s.q_des = put(h.q_des, R * per); s.qd_des = put(h.qd_des, R * per); }
  if (ff) s.tau_ff = put(h.tau_ff, R * per);
  if (e != hipSuccess) { (void)hipFree(d); return fail(MH_ERR_HIP, "drive upload failed: %s", hipGetErrorString(e)); }
  ab->d_drive = d; ab->drive = s;
  return MH_OK;
}

int mh_artic_batch_state_dev(mh_artic_batch* ab, void* stream, double* q_dst, double* qd_dst)
{
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(ab);
  const size_t n = (size_t)ab->B * ab->nj * sizeof(double);
  if (q_dst) MH_HIP(hipMemcpyAsync(q_dst, ab->d_q, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (qd_dst) MH_HIP(hipMemcpyAsync(qd_dst, ab->d_qd, n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MH_OK;
}

// the link poses of the resident states into d_p (device, B x nj x 12) on `stream`: the forward-dynamics kernel of the batch's form -- per-world
// images or the shared one, pose or angle coordinates -- with only the poses asked for.  mh_artic_batch_link_poses and _link_poses_dev share it
static hipError_t link_poses_launch(mh_artic_batch* ab, void* stream, double* d_p)
{
  namespace ar = mh::artic;
  if (ab->params) return ab->base_coords == MH_ARTIC_BASE_POSE ? artic_pw_pose_fwd_dyn_launch(ab, stream, nullptr, nullptr, nullptr, d_p, nullptr) : artic_pw_fwd_dyn_launch(ab, stream, nullptr, nullptr, nullptr, d_p, nullptr);
  if (ab->base_coords == MH_ARTIC_BASE_POSE) return artic_pose_fwd_dyn_launch(ab, stream, nullptr, nullptr, nullptr, d_p, nullptr);
  hipLaunchKernelGGL(ar::k_artic_fwd_dyn, dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)stream,
                     (const ar::Model*)ab->d_model, ab->B, (const double*)ab->d_q, (const double*)ab->d_qd, (const double*)nullptr, (double*)nullptr, (double*)nullptr, d_p, (int*)nullptr);
  return hipGetLastError();
}

int mh_artic_batch_fwd_dyn(mh_artic_batch* ab, const double* tau, double* qdd_out, double* H_out)
{
  namespace ar = mh::artic;
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());                              // a step may be in flight on a caller's non-blocking stream
  const size_t B = (size_t)ab->B, nj = (size_t)ab->nj;
  double *d_tau = nullptr, *d_qdd = nullptr, *d_H = nullptr; int* d_ok = nullptr;
  auto cleanup = [&]() { void* ps[] = { d_tau, d_qdd, d_H, d_ok }; for (void* p : ps) if (p) (void)hipFree(p); };
  bool ok = hipMalloc((void**)&d_qdd, B * nj * 8) == hipSuccess && hipMalloc((void**)&d_ok, B * 4) == hipSuccess;
  if (ok && tau) ok = hipMalloc((void**)&d_tau, B * nj * 8) == hipSuccess && hipMemcpy(d_tau, tau, B * nj * 8, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && H_out) ok = hipMalloc((void**)&d_H, B * nj * nj * 8) == hipSuccess;
  if (!ok) { cleanup(); return fail(MH_ERR_HIP, "device allocation failed"); }
  hipError_t e = hipSuccess;
  if (ab->params) e = ab->base_coords == MH_ARTIC_BASE_POSE ? artic_pw_pose_fwd_dyn_launch(ab, nullptr, d_tau, d_qdd, d_H, nullptr, d_ok) : artic_pw_fwd_dyn_launch(ab, nullptr, d_tau, d_qdd, d_H, nullptr, d_ok);   // each world's own image
  else if (ab->base_coords == MH_ARTIC_BASE_POSE) e = artic_pose_fwd_dyn_launch(ab, nullptr, d_tau, d_qdd, d_H, nullptr, d_ok);
  else hipLaunchKernelGGL(ar::k_artic_fwd_dyn, dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)nullptr,
                          (const ar::Model*)ab->d_model, ab->B, (const double*)ab->d_q, (const double*)ab->d_qd, (const double*)d_tau, d_qdd, d_H, (double*)nullptr, d_ok);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  std::vector<int> hok(B);
  if (e == hipSuccess && qdd_out) e = hipMemcpy(qdd_out, d_qdd, B * nj * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && H_out) e = hipMemcpy(H_out, d_H, B * nj * nj * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(hok.data(), d_ok, B * 4, hipMemcpyDeviceToHost);
  cleanup();
  if (e != hipSuccess) return fail(MH_ERR_HIP, "forward dynamics launch failed: %s", hipGetErrorString(e));
  for (size_t b = 0; b < B; b++) if (!hok[b]) return fail(MH_ERR_INVALID_ARG, "world %zu: the generalized inertia is not positive definite", b);
  return MH_OK;
}

int mh_artic_batch_link_poses(mh_artic_batch* ab, double* poses)
{
  if (!ab || !poses) return fail(MH_ERR_INVALID_ARG, "null batch / buffer");
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());                              // a step may be in flight on a caller's non-blocking stream
  const size_t bytes = (size_t)ab->B * ab->nj * 12 * 8;
  double* d_p = nullptr;
  MH_HIP(hipMalloc((void**)&d_p, bytes));
  hipError_t e = link_poses_launch(ab, nullptr, d_p);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(poses, d_p, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_p);
  if (e != hipSuccess) return fail(MH_ERR_HIP, "link pose launch failed: %s", hipGetErrorString(e));
  return MH_OK;
}

// Episodes on the device (include/moby_hip_artic.h): three launches on the caller's stream -- no synchronisation, no allocation, no host copy
int mh_artic_batch_reset_dev(mh_artic_batch* ab, void* stream, const int* mask_dev, const double* q_src, const double* qd_src, const double* pose_src)
{
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  if (pose_src && ab->base_coords != MH_ARTIC_BASE_POSE) return fail(MH_ERR_INVALID_ARG, "pose_src: the batch is in angle coordinates: no base pose to reset");
  MH_ON_DEVICE(ab);
  MH_HIP(artic_reset_launch(stream, ab->B, ab->nj, mask_dev, q_src, qd_src, pose_src, ab->d_q, ab->d_qd, ab->d_pose, ab->d_aux));
  return MH_OK;
}

int mh_artic_batch_status_dev(mh_artic_batch* ab, void* stream, int* status_dst, double* time_dst)
{
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  if (!status_dst && !time_dst) return fail(MH_ERR_INVALID_ARG, "status_dst and time_dst are both NULL: nothing to write");
  MH_ON_DEVICE(ab);
  MH_HIP(artic_status_launch(stream, ab->B, ab->d_aux, status_dst, time_dst));
  return MH_OK;
}

int mh_artic_batch_link_poses_dev(mh_artic_batch* ab, void* stream, double* poses_dst)
{
  if (!ab || !poses_dst) return fail(MH_ERR_INVALID_ARG, "null batch / buffer");
  MH_ON_DEVICE(ab);
  MH_HIP(link_poses_launch(ab, stream, poses_dst));
  return MH_OK;
}

int mh_artic_batch_jacobian(mh_artic_batch* ab, int link, const double* points, double* J_out)
{
  namespace ar = mh::artic;
  if (!ab || !points || !J_out) return fail(MH_ERR_INVALID_ARG, "null batch / buffer");
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());                              // a step may be in flight on a caller's non-blocking stream
  if (link < 0 || link >= ab->nj) return fail(MH_ERR_INVALID_ARG, "link %d outside [0, %d)", link, ab->nj);
  const size_t pb = (size_t)ab->B * 3 * 8, jb = (size_t)ab->B * 6 * ab->nj * 8;
  double* d_p = nullptr; double* d_J = nullptr;
  MH_HIP(hipMalloc((void**)&d_p, pb));
  hipError_t e = hipMalloc((void**)&d_J, jb);
  if (e == hipSuccess) e = hipMemcpy(d_p, points, pb, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (ab->params) e = ab->base_coords == MH_ARTIC_BASE_POSE ? artic_pw_pose_jacobian_launch(ab, link, d_p, d_J) : artic_pw_jacobian_launch(ab, link, d_p, d_J);
    else if (ab->base_coords == MH_ARTIC_BASE_POSE) e = artic_pose_jacobian_launch(ab, link, d_p, d_J);
    else hipLaunchKernelGGL(ar::k_artic_jacobian, dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)nullptr,
                            (const ar::Model*)ab->d_model, ab->B, (const double*)ab->d_q, link, (const double*)d_p, d_J);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(J_out, d_J, jb, hipMemcpyDeviceToHost);
  (void)hipFree(d_p); if (d_J) (void)hipFree(d_J);
  if (e != hipSuccess) return fail(MH_ERR_HIP, "Jacobian launch failed: %s", hipGetErrorString(e));
  return MH_OK;
}

int mh_artic_batch_download(mh_artic_batch* ab, double* q, double* qd, mh_world_aux* aux)
{
  if (!ab) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(ab);
  MH_HIP(hipDeviceSynchronize());
  const size_t n = (size_t)ab->B * ab->nj * 8;
  if (q) MH_HIP(hipMemcpy(q, ab->d_q, n, hipMemcpyDeviceToHost));
  if (qd) MH_HIP(hipMemcpy(qd, ab->d_qd, n, hipMemcpyDeviceToHost));
  if (aux) MH_HIP(hipMemcpy(aux, ab->d_aux, (size_t)ab->B * sizeof(mh_world_aux), hipMemcpyDeviceToHost));
  return MH_OK;
}

} // extern "C"
