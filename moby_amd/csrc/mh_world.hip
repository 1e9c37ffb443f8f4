// Host side of the many-worlds stepping ABI (include/moby_hip.h: mh_world_batch_*).  The kernels live in
// mh_world_{small,wheel,large,large_bsp,large_st,large_pw,large_rp}.hip; this file chooses the build for a scene (g_builds) and owns the device buffers.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include <algorithm>
#include "../../include/moby_hip.h"
#include "mh_host.h"

namespace mh {
// layouts of the constant tables of mh_world_common.h / mh_lcp_wave.h (checked by size in upload_tables)
struct FricTableH { double c[33][32]; double s[33][32]; };
struct Pow10TableH { double v[64]; };
}
#include <mutex>
namespace {
// The builds of the world kernel (mh_world_wave.inc), one row each: the plain code object, the one with forces in its forward dynamics (MHW_FORCES) and the
// one with the phase profiler's stamps -- null where there is none: mh_world_batch_profile then launches the production object and reports zeros.
// Every object is one mh_world_variant (mh_host.h): its kernel is launched inside its own translation unit, so the kernels' differing argument lists
// (forces and wrench in the forced objects, the report rows in the report build) do not show here.
enum { WB_SMALL = 0, WB_WHEEL, WB_LARGE, WB_LARGE_BSP, WB_LARGE_ST, WB_LARGE_PW, WB_LARGE_RP, WB_COUNT };
struct world_build {
  const mh_world_variant* (*plain)();
  const mh_world_variant* (*forced)();
  const mh_world_variant* (*prof)();
};
const world_build g_builds[WB_COUNT] = {
  { mh_world_variant_small,     mh_world_variant_small_forces,     mh_world_variant_small_prof },
  { mh_world_variant_wheel,     mh_world_variant_wheel_forces,     mh_world_variant_wheel_prof },
  { mh_world_variant_large,     mh_world_variant_large_forces,     mh_world_variant_large_prof },
  { mh_world_variant_large_bsp, mh_world_variant_large_bsp_forces, nullptr },     // box-sphere pairs (MHW_BSP)
  { mh_world_variant_large_st,  mh_world_variant_large_st_forces,  nullptr },     // + static bodies (MHW_STATICS)
  { mh_world_variant_large_pw,  mh_world_variant_large_pw_forces,  nullptr },     // + per-world parameters (MHW_PARAMS)
  { mh_world_variant_large_rp,  mh_world_variant_large_rp_forces,  nullptr },     // + the contact report (MHW_REPORT)
};
// The __constant__ tables are one copy per DEVICE (hipMemcpyToSymbol writes the current device's): uploaded once per device, keyed on the
// device current at create, under a lock -- as mh_artic_batch_create does for its own table.
std::mutex g_tables_mu;
std::vector<char> g_tables_done;
hipError_t init_tables()
{
  hipError_t g_tables_err = hipSuccess;
  static mh::FricTableH ft;
  for (int kh = 0; kh < 33; kh++)
    for (int j = 0; j < 32; j++) {
      double c = 0.0, s = 0.0;
      if (kh >= 2 && j < kh) { const double theta = (double)j / (kh - 1) * M_PI_2; c = std::cos(theta); s = std::sin(theta); }  // ICH-QP:466-468
      ft.c[kh][j] = c; ft.s[kh][j] = s;
    }
  mh::Pow10TableH p10;
  for (int i = 0; i < 64; i++) p10.v[i] = std::pow(10.0, (double)(i - 32)); // LCP.cpp:285
  for (int i = 0; i < WB_COUNT && g_tables_err == hipSuccess; i++) {                                 // (one copy of the tables per code object)
    const world_build& r = g_builds[i];
    g_tables_err = r.plain()->upload_tables(&ft, sizeof(ft), &p10, sizeof(p10));
    if (g_tables_err == hipSuccess) g_tables_err = r.forced()->upload_tables(&ft, sizeof(ft), &p10, sizeof(p10));
    if (g_tables_err == hipSuccess && r.prof) g_tables_err = r.prof()->upload_tables(&ft, sizeof(ft), &p10, sizeof(p10));
  }
  return g_tables_err;
}
hipError_t tables_for_current_device()
{
  std::lock_guard<std::mutex> lk(g_tables_mu);
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if ((int)g_tables_done.size() <= dev) g_tables_done.resize(dev + 1, 0);
  if (!g_tables_done[dev]) { e = init_tables(); if (e == hipSuccess) g_tables_done[dev] = 1; }
  return e;
}
// nstat: the static bodies beside the scene's ground (mh_world_statics.n; 0 for the entries without statics): the pair arrays are triangular over all of them
int check_scene(const mh_scene* sc, int nstat = 0)
{
  if (!sc) return fail(MH_ERR_INVALID_ARG, "null scene");
  if (sc->nb < 1 || sc->nb > MH_MAX_BODIES) return fail(MH_ERR_INVALID_ARG, "nb = %d outside [1, %d]", sc->nb, MH_MAX_BODIES);
  const int ntot = sc->nb + (sc->has_ground ? 1 : 0) + nstat;
  int spokes_body = -1;
  for (int b = 0; b < sc->nb; b++) {
    if (sc->geom_type[b] != MH_GEOM_SPHERE && sc->geom_type[b] != MH_GEOM_SPOKES && sc->geom_type[b] != MH_GEOM_BOX)
      return fail(MH_ERR_INVALID_ARG, "body %d: geometry type %d is not built (sphere, spokes, box)", b, sc->geom_type[b]);
    if (sc->geom_type[b] == MH_GEOM_BOX) {
      if (!(sc->geom_dim[b][1] > 0.0) || !(sc->geom_dim[b][2] > 0.0)) return fail(MH_ERR_INVALID_ARG, "body %d: box edge lengths must be > 0", b);
      for (int o = b + 1; o < sc->nb; o++) if (sc->geom_type[o] == MH_GEOM_BOX) {
        if (sc->pair_enabled[b * ntot - (b * (b + 1)) / 2 + (o - b - 1)])
          return fail(MH_ERR_INVALID_ARG, "bodies %d,%d: box-box contact is not built; disable the pair (box-plane and box-sphere are)", b, o);
      }
    }
    if (sc->geom_type[b] == MH_GEOM_SPOKES) {
      const double N = sc->geom_dim[b][1];
      if (!sc->has_ground) return fail(MH_ERR_INVALID_ARG, "body %d: spokes geometry needs the ground plane", b);
      if (!(N >= 1.0 && N <= (double)MH_MAX_SPOKES) || N != (double)(int)N) return fail(MH_ERR_INVALID_ARG, "body %d: number of spokes outside [1, %d]", b, MH_MAX_SPOKES);
      if (spokes_body >= 0 && (sc->geom_dim[b][0] != sc->geom_dim[spokes_body][0] || N != sc->geom_dim[spokes_body][1]))
        return fail(MH_ERR_INVALID_ARG, "body %d: all spokes geometries of a scene must share R and N", b);
      spokes_body = b;
    }
    if (!(sc->geom_dim[b][0] > 0.0) || !(sc->mass[b] > 0.0)) return fail(MH_ERR_INVALID_ARG, "body %d: radius and mass must be > 0", b);
    for (int k = 0; k < 3; k++) if (!(sc->inertia[b][k] > 0.0)) return fail(MH_ERR_INVALID_ARG, "body %d: inertia must be > 0", b);
  }
  for (int p = 0; p < ntot * (ntot - 1) / 2; p++)
    if (sc->cp_nk[p] < 4 || sc->cp_nk[p] > 64) return fail(MH_ERR_INVALID_ARG, "pair %d: friction-cone-edges %d outside [4, 64]", p, sc->cp_nk[p]);
  if (sc->lcp_n_max < 0 || sc->lcp_n_max > MH_LCP_MAX_N_WAVE) return fail(MH_ERR_INVALID_ARG, "lcp_n_max outside [0, %d]", MH_LCP_MAX_N_WAVE);
  return MH_OK;
}
// the refusals of mh_world_batch_create_statics (include/moby_hip.h); n == 0 passes
int check_statics(const mh_scene* sc, const mh_world_statics* st)
{
  if (!sc) return fail(MH_ERR_INVALID_ARG, "null scene");
  if (st->n < 0 || st->n > MH_MAX_STATICS) return fail(MH_ERR_INVALID_ARG, "statics: n = %d outside [0, %d]", st->n, MH_MAX_STATICS);
  if (st->n == 0) return MH_OK;
  if (sc->nb < 1 || sc->nb > MH_MAX_BODIES) return fail(MH_ERR_INVALID_ARG, "nb = %d outside [1, %d]", sc->nb, MH_MAX_BODIES);
  const int hg = sc->has_ground ? 1 : 0, ntot = sc->nb + hg + st->n;
  if (ntot > MH_MAX_BODIES + 1)
    return fail(MH_ERR_INVALID_ARG, "statics: nb + has_ground + n = %d + %d + %d exceeds %d (the pair arrays hold C(%d, 2) slots)", sc->nb, hg, st->n, MH_MAX_BODIES + 1, MH_MAX_BODIES + 1);
  for (int b = 0; b < sc->nb; b++) if (sc->geom_type[b] == MH_GEOM_SPOKES)
    return fail(MH_ERR_INVALID_ARG, "body %d: spokes geometry in a scene with static bodies is not built (the wheel's collision plugin knows one ground)", b);
  for (int k = 0; k < st->n; k++) {
    if (st->type[k] != MH_STATIC_PLANE && st->type[k] != MH_STATIC_BOX) return fail(MH_ERR_INVALID_ARG, "static %d: type %d is not built (plane, box)", k, st->type[k]);
    for (int q = 0; q < 9; q++) if (!std::isfinite(st->R[k][q])) return fail(MH_ERR_INVALID_ARG, "static %d: rotation is not finite", k);
    for (int q = 0; q < 3; q++) if (!std::isfinite(st->o[k][q])) return fail(MH_ERR_INVALID_ARG, "static %d: origin is not finite", k);
    if (st->type[k] != MH_STATIC_BOX) continue;
    for (int q = 0; q < 3; q++) if (!(st->dim[k][q] > 0.0) || !std::isfinite(st->dim[k][q])) return fail(MH_ERR_INVALID_ARG, "static %d: box edge lengths must be > 0", k);
    const int j = sc->nb + hg + k;
    for (int b = 0; b < sc->nb; b++) if (sc->geom_type[b] == MH_GEOM_BOX && sc->pair_enabled[b * ntot - (b * (b + 1)) / 2 + (j - b - 1)])
      return fail(MH_ERR_INVALID_ARG, "body %d, static %d: box-box contact is not built; disable the pair (box-plane and sphere-box are)", b, k);
  }
  return MH_OK;
}
// the refusals of one mh_world_params record (include/moby_hip.h, "Per-world parameters"): the values that check_scene / check_statics validate in the shared
// records, validated for world w.  sc and st (or null) have passed their own checks: they give the topology.
int check_params(const mh_scene* sc, const mh_world_statics* st, const mh_world_params* r, int w)
{
  const int nstat = st ? st->n : 0, hg = sc->has_ground ? 1 : 0, ntot = sc->nb + hg + nstat;
  for (int b = 0; b < sc->nb; b++) {
    if (!(r->mass[b] > 0.0)) return fail(MH_ERR_INVALID_ARG, "world %d: mass[%d] must be > 0", w, b);
    for (int k = 0; k < 3; k++) if (!(r->inertia[b][k] > 0.0)) return fail(MH_ERR_INVALID_ARG, "world %d: inertia[%d] must be > 0", w, b);
    if (sc->geom_type[b] == MH_GEOM_SPHERE && !(r->geom_dim[b][0] > 0.0)) return fail(MH_ERR_INVALID_ARG, "world %d: geom_dim[%d]: radius must be > 0", w, b);
    if (sc->geom_type[b] == MH_GEOM_BOX)
      for (int k = 0; k < 3; k++) if (!(r->geom_dim[b][k] > 0.0)) return fail(MH_ERR_INVALID_ARG, "world %d: geom_dim[%d]: box edge lengths must be > 0", w, b);
  }
  for (int q = 0; q < 3; q++) if (!std::isfinite(r->gravity[q])) return fail(MH_ERR_INVALID_ARG, "world %d: gravity is not finite", w);
  if (hg) {
    for (int q = 0; q < 9; q++) if (!std::isfinite(r->plane_R[q])) return fail(MH_ERR_INVALID_ARG, "world %d: plane_R is not finite", w);
    for (int q = 0; q < 3; q++) if (!std::isfinite(r->plane_o[q])) return fail(MH_ERR_INVALID_ARG, "world %d: plane_o is not finite", w);
  }
  for (int p = 0; p < ntot * (ntot - 1) / 2; p++) {
    if (!std::isfinite(r->cp_epsilon[p])) return fail(MH_ERR_INVALID_ARG, "world %d: cp_epsilon[%d] is not finite", w, p);
    if (!std::isfinite(r->cp_mu_coulomb[p])) return fail(MH_ERR_INVALID_ARG, "world %d: cp_mu_coulomb[%d] is not finite", w, p);
    if (!std::isfinite(r->cp_mu_viscous[p])) return fail(MH_ERR_INVALID_ARG, "world %d: cp_mu_viscous[%d] is not finite", w, p);
    if (!std::isfinite(r->cp_compliance[p])) return fail(MH_ERR_INVALID_ARG, "world %d: cp_compliance[%d] is not finite", w, p);
  }
  for (int k = 0; k < nstat; k++) {
    for (int q = 0; q < 9; q++) if (!std::isfinite(r->st_R[k][q])) return fail(MH_ERR_INVALID_ARG, "world %d: st_R[%d] is not finite", w, k);
    for (int q = 0; q < 3; q++) if (!std::isfinite(r->st_o[k][q])) return fail(MH_ERR_INVALID_ARG, "world %d: st_o[%d] is not finite", w, k);
    if (st->type[k] != MH_STATIC_BOX) continue;
    for (int q = 0; q < 3; q++) if (!(r->st_dim[k][q] > 0.0) || !std::isfinite(r->st_dim[k][q])) return fail(MH_ERR_INVALID_ARG, "world %d: st_dim[%d]: box edge lengths must be > 0", w, k);
  }
  return MH_OK;
}
} // namespace

extern "C" {

void mh_world_params_from_scene(const mh_scene* sc, const mh_world_statics* st, mh_world_params* out)
{
  std::memset(out, 0, sizeof(*out));
  std::memcpy(out->mass, sc->mass, sizeof(out->mass));
  std::memcpy(out->inertia, sc->inertia, sizeof(out->inertia));
  std::memcpy(out->geom_dim, sc->geom_dim, sizeof(out->geom_dim));
  std::memcpy(out->plane_R, sc->plane_R, sizeof(out->plane_R));
  std::memcpy(out->plane_o, sc->plane_o, sizeof(out->plane_o));
  std::memcpy(out->gravity, sc->gravity, sizeof(out->gravity));
  std::memcpy(out->cp_epsilon, sc->cp_epsilon, sizeof(out->cp_epsilon));
  std::memcpy(out->cp_mu_coulomb, sc->cp_mu_coulomb, sizeof(out->cp_mu_coulomb));
  std::memcpy(out->cp_mu_viscous, sc->cp_mu_viscous, sizeof(out->cp_mu_viscous));
  std::memcpy(out->cp_compliance, sc->cp_compliance, sizeof(out->cp_compliance));
  if (!st) return;
  std::memcpy(out->st_R, st->R, sizeof(out->st_R));
  std::memcpy(out->st_o, st->o, sizeof(out->st_o));
  std::memcpy(out->st_dim, st->dim, sizeof(out->st_dim));
}

void mh_scene_defaults(mh_scene* s)
{
  std::memset(s, 0, sizeof(*s));
  s->min_step_size = std::sqrt(2.220446049250313e-16);       // TimeSteppingSimulator.cpp:48
  s->contact_dist_thresh = 1e-6;                             // ConstraintSimulator.cpp:56
  s->cstab_eps = std::sqrt(2.220446049250313e-16);           // ConstraintStabilization.cpp:59
  s->cstab_max_iterations = MH_CSTAB_DEFAULT_MAX_ITERATIONS; // ConstraintStabilization.cpp:56 is UINT_MAX: see moby_hip.h
  s->plane_R[0] = s->plane_R[4] = s->plane_R[8] = 1.0;
  for (int p = 0; p < MH_MAX_PAIRS; p++) { s->pair_enabled[p] = 1; s->cp_nk[p] = 4; }   // ContactParameters.cpp:26
}

void mh_world_aux_init(mh_world_aux* a, uint32_t seed)
{
  std::memset(a, 0, sizeof(*a));
  mh_rand_seed(a->rng, seed);
}


struct mh_world_batch {
  int device;                // the HIP device the batch lives on (current at create); every entry point runs there (MH_ON_DEVICE)
  mh_scene scene;
  int B;
  int nmax;
  int build;                 // row of g_builds (WB_*)
  mh_scene* d_scene;
  double* d_lu_ws;
  double* d_state;
  mh_world_aux* d_aux;
  bool has_forces;                  // mh_world_batch_set_forces stored terms != 0: the row's forced object is launched (as it is when a wrench is passed)
  mh_world_forces* d_forces;        // their device copy (allocated by the first set_forces)
  bool has_params;                  // created with per-world records (mh_world_batch_create_params): set_params / set_params_dev may replace them
  mh_world_params* d_params;        // the B records behind the statics record in d_scene's allocation (the per-world-parameters build only), or null
  mh_world_statics statics;         // the statics the batch was created with (n = 0 without): the topology set_params validates against
  bool has_report;                  // created for the contact report (mh_world_batch_create_report): mh_world_batch_step_report may pass rows
};

namespace {
// the one launch behind every stepping entry: the row's plain object, or the forced one when the batch stores forces or the caller passes a wrench
// (stamped: mh_world_batch_profile's object instead, the row's plain kernel with the profiler's stamps)
int launch_step(mh_world_batch* wb, hipStream_t stream, int grid, double dt, int nsteps, double* traj_dev, unsigned long long* prof, const int* ids_dev,
                const double* wrench_dev, int rows, double* report_dev = nullptr, const mh_world_variant* stamped = nullptr)
{
  mh_world_launch a;
  a.stream = stream; a.grid = grid;
  a.scene = wb->d_scene; a.B = wb->B; a.dt = dt; a.nsteps = nsteps; a.state = wb->d_state; a.aux = wb->d_aux; a.traj = traj_dev; a.nmax = wb->nmax;
  a.lu_ws = wb->d_lu_ws; a.ka = mh_g_debug_ka; a.prof = prof; a.ids = ids_dev;
  a.forces = wb->has_forces ? wb->d_forces : nullptr; a.wrench = wrench_dev; a.wrench_rows = rows;
  a.report = report_dev;
  const world_build& r = g_builds[wb->build];
  const hipError_t e = (stamped ? stamped : (wb->has_forces || wrench_dev) ? r.forced() : r.plain())->launch(a);
  if (e != hipSuccess) return fail(MH_ERR_HIP, "hipGetLastError() failed: %s", hipGetErrorString(e));
  return MH_OK;
}
}  // namespace

// diagnostic: blocks per CU the runtime's occupancy query reports for the kernel this batch uses
int mh_world_batch_occupancy(mh_world_batch* wb);
int mh_world_batch_occupancy(mh_world_batch* wb)
{
  if (!wb) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(wb);
  int n = 0;
  const hipError_t e = (wb->has_forces ? g_builds[wb->build].forced() : g_builds[wb->build].plain())->occupancy(&n);
  if (e != hipSuccess) return fail(MH_ERR_HIP, "occupancy query failed: %s", hipGetErrorString(e));
  return n;
}

int mh_world_batch_create(const mh_scene* scene, int B, mh_world_batch** out)
{
  return mh_world_batch_create_statics(scene, nullptr, B, out);
}

int mh_world_batch_create_statics(const mh_scene* scene, const mh_world_statics* statics, int B, mh_world_batch** out)
{
  return mh_world_batch_create_params(scene, statics, nullptr, B, out);
}

namespace { int create_batch(const mh_scene* scene, const mh_world_statics* statics, const mh_world_params* params, int B, bool report, mh_world_batch** out); }

int mh_world_batch_create_params(const mh_scene* scene, const mh_world_statics* statics, const mh_world_params* params, int B, mh_world_batch** out)
{
  return create_batch(scene, statics, params, B, false, out);
}

int mh_world_batch_create_report(const mh_scene* scene, const mh_world_statics* statics, const mh_world_params* params, int B, mh_world_batch** out)
{
  return create_batch(scene, statics, params, B, true, out);
}

namespace {
// the one create behind every entry.  report: the batch takes the contact-report build (its records filled from the scene where the caller gave none)
int create_batch(const mh_scene* scene, const mh_world_statics* statics, const mh_world_params* params, int B, bool report, mh_world_batch** out)
{
  if (!out) return fail(MH_ERR_INVALID_ARG, "null out");
  *out = nullptr;
  int rc = statics ? check_statics(scene, statics) : MH_OK;
  if (rc != MH_OK) return rc;
  const int nstat = statics ? statics->n : 0;
  rc = check_scene(scene, nstat);
  if (rc != MH_OK) return rc;
  if (B <= 0) return fail(MH_ERR_INVALID_ARG, "batch must be > 0");
  if (params) for (int w = 0; w < B; w++) { rc = check_params(scene, nstat > 0 ? statics : nullptr, params + w, w); if (rc != MH_OK) return rc; }
  if (mh_device_count() <= 0) return fail(MH_ERR_NO_DEVICE, "no HIP device visible");
  { const hipError_t te = tables_for_current_device();
    if (te != hipSuccess) return fail(MH_ERR_HIP, "constant table upload failed: %s", hipGetErrorString(te)); }
  mh_world_batch* wb = new mh_world_batch();
  if (hipGetDevice(&wb->device) != hipSuccess) { delete wb; return fail(MH_ERR_HIP, "hipGetDevice failed"); }
  wb->scene = *scene; wb->B = B;
  wb->nmax = scene->lcp_n_max ? scene->lcp_n_max : MH_LCP_MAX_N_WAVE;
  {
    // small variant: <= 4 bodies, <= 6 pairs, islands of <= 4 contacts (12 Jacobian rows); the
    // caller opts in by bounding the LCP size (lcp_n_max <= 56 = 4 contacts x (6 + 16/2) rows).
    // A world that outgrows the variant's limits at run time gets MH_WORLD_UNSUPPORTED.
    // Spokes geometry or a pair with mu-coulomb >= 100 (=> the no-slip model, ICH:127-135) needs a
    // variant built with those features: "wheel" for one or two bodies, otherwise "large".
    const int ntot = scene->nb + (scene->has_ground ? 1 : 0) + nstat, npairs = ntot * (ntot - 1) / 2;
    bool noslip = false, box = false;
    for (int b = 0; b < scene->nb; b++) if (scene->geom_type[b] == MH_GEOM_SPOKES) noslip = true;
    for (int b = 0; b < scene->nb; b++) if (scene->geom_type[b] == MH_GEOM_BOX) box = true;
    for (int p = 0; p < npairs; p++) if (scene->pair_enabled[p] && scene->cp_mu_coulomb[p] >= 1e2) noslip = true;
    if (!noslip && !box && scene->nb <= 4 && npairs <= 6 && scene->lcp_n_max > 0 && scene->lcp_n_max <= 56) wb->build = WB_SMALL;
    else if (noslip && !box && scene->nb <= 2 && npairs <= 3) wb->build = WB_WHEEL;
    else wb->build = WB_LARGE;
    // an enabled pair of a box and a sphere (two free bodies) needs the large variant's box-sphere build; every other scene takes what it took
    bool bsp = false;
    for (int i = 0; i < scene->nb; i++) for (int j = i + 1; j < scene->nb; j++) {
      const int gi_ = scene->geom_type[i], gj_ = scene->geom_type[j];
      if (((gi_ == MH_GEOM_BOX && gj_ == MH_GEOM_SPHERE) || (gi_ == MH_GEOM_SPHERE && gj_ == MH_GEOM_BOX)) && scene->pair_enabled[i * ntot - (i * (i + 1)) / 2 + (j - i - 1)]) bsp = true;
    }
    if (wb->build == WB_LARGE && (bsp || mh_g_debug_world_bsp != 0)) wb->build = WB_LARGE_BSP;       // (key 15: every large batch through the box-sphere build)
    // static bodies need the statics build; every other batch launches what it launched (key 16: the box-sphere batches through the statics build)
    if (nstat > 0 || (wb->build == WB_LARGE_BSP && mh_g_debug_world_st != 0)) wb->build = WB_LARGE_ST;
    // per-world records need the per-world-parameters build, whatever the scene; every other batch launches what it launched (key 17: the statics batches
    // through it, every record filled from the scene)
    if (params || (wb->build == WB_LARGE_ST && mh_g_debug_world_pw != 0)) wb->build = WB_LARGE_PW;
    // the contact report needs the report build, whatever the scene; every other batch launches what it launched (key 18: the per-world-parameters
    // batches through it, with a null report)
    if (report || (wb->build == WB_LARGE_PW && mh_g_debug_world_rp != 0)) wb->build = WB_LARGE_RP;
    wb->has_report = report;
    wb->has_forces = false; wb->d_forces = nullptr;
    wb->has_params = params != nullptr; wb->d_params = nullptr;
  }
  wb->d_scene = nullptr; wb->d_state = nullptr; wb->d_aux = nullptr; wb->d_lu_ws = nullptr;
  // device scene record, followed by the spoke-tip table p1 = (cos(theta) R, sin(theta) R), theta = pi i 2 / N
  // (coldet-plugin.cpp:104-110), evaluated with the host's libm like the oracle does
  double tips[2 * MH_MAX_SPOKES] = {0.0};
  for (int b = 0; b < scene->nb; b++) if (scene->geom_type[b] == MH_GEOM_SPOKES) {
    const double Rr = scene->geom_dim[b][0]; const int N = (int)scene->geom_dim[b][1];
    for (int i = 0; i < N; i++) { const double theta = M_PI * i * 2.0 / N; tips[2*i] = std::cos(theta) * Rr; tips[2*i+1] = std::sin(theta) * Rr; }
  }
  // ... and by the statics record (n = 0 without statics), which only the statics build reads
  mh_world_statics strec; std::memset(&strec, 0, sizeof(strec));
  if (nstat > 0) strec = *statics;
  wb->statics = strec;
  // ... and, in the per-world-parameters build and the report build, by the B records (scene | spoke tips | statics | params[B]): the kernel finds them behind the statics record
  const size_t params_off = sizeof(mh_scene) + sizeof(tips) + sizeof(strec);
  static_assert((sizeof(mh_scene) + sizeof(tips) + sizeof(mh_world_statics)) % 8 == 0 && sizeof(mh_world_params) == 335 * sizeof(double), "params records: 8-byte aligned, doubles only");
  const size_t params_bytes = (wb->build == WB_LARGE_PW || wb->build == WB_LARGE_RP) ? (size_t)B * sizeof(mh_world_params) : 0;
  hipError_t e = hipMalloc(&wb->d_scene, params_off + params_bytes);
  if (e == hipSuccess) e = hipMalloc(&wb->d_lu_ws, (size_t)B * wb->nmax * wb->nmax * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&wb->d_state, (size_t)B * scene->nb * MH_BODY_STATE * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&wb->d_aux, (size_t)B * sizeof(mh_world_aux));
  if (e == hipSuccess) e = hipMemcpy(wb->d_scene, scene, sizeof(mh_scene), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(reinterpret_cast<char*>(wb->d_scene) + sizeof(mh_scene), tips, sizeof(tips), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(reinterpret_cast<char*>(wb->d_scene) + sizeof(mh_scene) + sizeof(tips), &strec, sizeof(strec), hipMemcpyHostToDevice);
  if (e == hipSuccess && params_bytes) {
    wb->d_params = reinterpret_cast<mh_world_params*>(reinterpret_cast<char*>(wb->d_scene) + params_off);
    if (params) e = hipMemcpy(wb->d_params, params, params_bytes, hipMemcpyHostToDevice);
    else {                                                        // key 17, or a report batch without records: every world's record is the scene
      std::vector<mh_world_params> rec((size_t)B);
      mh_world_params_from_scene(scene, nstat > 0 ? statics : nullptr, &rec[0]);
      for (int w = 1; w < B; w++) rec[w] = rec[0];
      e = hipMemcpy(wb->d_params, rec.data(), params_bytes, hipMemcpyHostToDevice);
    }
  }
  if (e == hipSuccess) e = hipMemset(wb->d_state, 0, (size_t)B * scene->nb * MH_BODY_STATE * sizeof(double));
  if (e == hipSuccess) {
    std::vector<mh_world_aux> a((size_t)B);
    mh_world_aux_init(&a[0], 1);
    for (int b = 1; b < B; b++) a[b] = a[0];
    e = hipMemcpy(wb->d_aux, a.data(), (size_t)B * sizeof(mh_world_aux), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) { mh_world_batch_destroy(wb); return fail(MH_ERR_HIP, "device allocation/upload failed: %s", hipGetErrorString(e)); }
  *out = wb;
  return MH_OK;
}
}  // namespace

int mh_world_batch_device(const mh_world_batch* wb) { return wb ? wb->device : fail(MH_ERR_INVALID_ARG, "null batch"); }

int mh_world_batch_destroy(mh_world_batch* wb)
{
  if (!wb) return MH_OK;
  MH_ON_DEVICE(wb);
  if (wb->d_scene) (void)hipFree(wb->d_scene);
  if (wb->d_state) (void)hipFree(wb->d_state);
  if (wb->d_aux) (void)hipFree(wb->d_aux);
  if (wb->d_lu_ws) (void)hipFree(wb->d_lu_ws);
  if (wb->d_forces) (void)hipFree(wb->d_forces);
  delete wb;
  return MH_OK;
}

int mh_world_batch_upload(mh_world_batch* wb, const double* state, const mh_world_aux* aux)
{
  if (!wb) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(wb);
  if (state) MH_HIP(hipMemcpy(wb->d_state, state, (size_t)wb->B * wb->scene.nb * MH_BODY_STATE * sizeof(double), hipMemcpyHostToDevice));
  if (aux) MH_HIP(hipMemcpy(wb->d_aux, aux, (size_t)wb->B * sizeof(mh_world_aux), hipMemcpyHostToDevice));
  return MH_OK;
}

int mh_world_batch_step(mh_world_batch* wb, void* stream, double dt, int nsteps, double* traj_dev)
{
  if (!wb) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(wb);
  if (nsteps < 0) return fail(MH_ERR_INVALID_ARG, "negative step count");
  if (nsteps == 0) return MH_OK;
  if (!(dt > 0.0)) return fail(MH_ERR_INVALID_ARG, "dt must be > 0");
  return launch_step(wb, (hipStream_t)stream, wb->B, dt, nsteps, traj_dev, nullptr, nullptr, nullptr, 1);
}

// nsteps x step(dt) of the worlds ids[0 .. count) only (device pointer), on the given stream: worlds are independent, so a batch can be
// split over streams -- e.g. the few worlds whose solver chain runs to its pivot caps in their own launch, so that the next interval of
// the others does not wait for them (bench.py's long_horizon leg).  Launches on different streams must not share a world.
int mh_world_batch_step_ids(mh_world_batch* wb, void* stream, double dt, int nsteps, const int* ids_dev, int count)
{
  if (!wb || !ids_dev) return fail(MH_ERR_INVALID_ARG, "null batch / id list");
  MH_ON_DEVICE(wb);
  if (nsteps < 0 || count < 0 || count > wb->B) return fail(MH_ERR_INVALID_ARG, "bad step count (%d) or id count (%d of %d)", nsteps, count, wb->B);
  if (nsteps == 0 || count == 0) return MH_OK;
  if (!(dt > 0.0)) return fail(MH_ERR_INVALID_ARG, "dt must be > 0");
  return launch_step(wb, (hipStream_t)stream, count, dt, nsteps, nullptr, nullptr, ids_dev, nullptr, 1);
}

int mh_world_batch_set_forces(mh_world_batch* wb, const mh_world_forces* host)
{
  const int terms = host ? host->terms : 0;
  if (terms & ~(MH_FORCE_STOKES | MH_FORCE_DAMPING)) return fail(MH_ERR_INVALID_ARG, "forces: unknown bits in terms (0x%x)", terms);
  if (terms) {
    const double* arr[6] = { host->stokes_b, host->stokes_b_ang, host->damp_kl, host->damp_ka, host->damp_klsq, host->damp_kasq };
    static const char* const nm[6] = { "stokes_b", "stokes_b_ang", "damp_kl", "damp_ka", "damp_klsq", "damp_kasq" };
    for (int k = 0; k < 6; k++) {
      if (!(terms & (k < 2 ? MH_FORCE_STOKES : MH_FORCE_DAMPING))) continue;
      for (int b = 0; b < MH_MAX_BODIES; b++) if (!std::isfinite(arr[k][b])) return fail(MH_ERR_INVALID_ARG, "forces: %s[%d] is not finite", nm[k], b);
    }
  }
  if (!wb) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(wb);
  if (!terms) { wb->has_forces = false; return MH_OK; }
  if (!wb->d_forces) MH_HIP(hipMalloc(&wb->d_forces, sizeof(mh_world_forces)));
  MH_HIP(hipMemcpy(wb->d_forces, host, sizeof(mh_world_forces), hipMemcpyHostToDevice));
  wb->has_forces = true;
  return MH_OK;
}

namespace {
int params_range(mh_world_batch* wb, const void* src, int first, int count)
{
  if (!wb || !src) return fail(MH_ERR_INVALID_ARG, "null batch / records");
  if (!wb->has_params || !wb->d_params) return fail(MH_ERR_INVALID_ARG, "the batch was created without per-world parameters (mh_world_batch_create_params)");
  if (first < 0 || count < 0 || first > wb->B || count > wb->B - first) return fail(MH_ERR_INVALID_ARG, "worlds %d .. %d outside the batch of %d", first, first + count, wb->B);
  return MH_OK;
}
}  // namespace

int mh_world_batch_set_params(mh_world_batch* wb, const mh_world_params* host, int first, int count)
{
  int rc = params_range(wb, host, first, count);
  if (rc != MH_OK) return rc;
  for (int k = 0; k < count; k++) { rc = check_params(&wb->scene, wb->statics.n > 0 ? &wb->statics : nullptr, host + k, first + k); if (rc != MH_OK) return rc; }
  if (count == 0) return MH_OK;
  MH_ON_DEVICE(wb);
  MH_HIP(hipMemcpy(wb->d_params + first, host, (size_t)count * sizeof(mh_world_params), hipMemcpyHostToDevice));
  return MH_OK;
}

int mh_world_batch_set_params_dev(mh_world_batch* wb, void* stream, const mh_world_params* dev, int first, int count)
{
  const int rc = params_range(wb, dev, first, count);
  if (rc != MH_OK) return rc;
  if (count == 0) return MH_OK;
  MH_ON_DEVICE(wb);
  MH_HIP(hipMemcpyAsync(wb->d_params + first, dev, (size_t)count * sizeof(mh_world_params), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MH_OK;
}

int mh_world_batch_step_wrench(mh_world_batch* wb, void* stream, double dt, int nsteps, double* traj_dev,
                               const int* ids_dev, int count, const double* wrench_dev, int rows)
{
  return mh_world_batch_step_report(wb, stream, dt, nsteps, traj_dev, ids_dev, count, wrench_dev, rows, nullptr);
}

// the one stepping entry with every optional argument: report_dev == NULL is mh_world_batch_step_wrench, with its checks and messages
int mh_world_batch_step_report(mh_world_batch* wb, void* stream, double dt, int nsteps, double* traj_dev,
                               const int* ids_dev, int count, const double* wrench_dev, int rows, double* report_dev)
{
  if (nsteps < 0) return fail(MH_ERR_INVALID_ARG, "negative step count");
  if (rows < 1) return fail(MH_ERR_INVALID_ARG, "wrench: rows = %d (must be >= 1)", rows);
  if (rows > 1 && rows < nsteps) return fail(MH_ERR_INVALID_ARG, "wrench: %d rows for %d steps (1 row, or one per step)", rows, nsteps);
  if (traj_dev && ids_dev) return fail(MH_ERR_INVALID_ARG, "a trajectory buffer cannot be combined with an id list");
  if (!wb) return fail(MH_ERR_INVALID_ARG, "null batch");
  if (report_dev && (!wb->has_report || wb->build != WB_LARGE_RP)) return fail(MH_ERR_INVALID_ARG, "the batch was created without the contact report (mh_world_batch_create_report)");
  MH_ON_DEVICE(wb);
  if (ids_dev && (count < 0 || count > wb->B)) return fail(MH_ERR_INVALID_ARG, "bad id count (%d of %d)", count, wb->B);
  if (nsteps == 0 || (ids_dev && count == 0)) return MH_OK;
  if (!(dt > 0.0)) return fail(MH_ERR_INVALID_ARG, "dt must be > 0");
  return launch_step(wb, (hipStream_t)stream, ids_dev ? count : wb->B, dt, nsteps, traj_dev, nullptr, ids_dev, wrench_dev, rows, report_dev);
}

int mh_world_profile_phase_count(void) { return g_builds[WB_LARGE].plain()->ph_count; }

// diagnostic: one launch with per-phase cycle accumulators (mh::PH_*), averaged over worlds on the host
int mh_world_batch_profile(mh_world_batch* wb, double dt, int nsteps, double* phase_cycles, int nphase)
{
  if (!wb || !phase_cycles) return fail(MH_ERR_INVALID_ARG, "null argument");
  MH_ON_DEVICE(wb);
  unsigned long long* dprof = nullptr;
  const int PHC = mh_world_profile_phase_count();       // the same enum in every build
  const size_t sz = (size_t)wb->B * PHC * sizeof(unsigned long long);
  MH_HIP(hipMalloc(&dprof, sz));
  MH_HIP(hipMemset(dprof, 0, sz));
  // the PROFILE object of the batch's build: the production kernel has no stamp code (mh_lcp_wave.h lp_tick)
  // (a batch with stored forces: the forced production kernel -- it steps the worlds under their forces and has no stamps, so every cycle count is 0)
  // (a batch on the box-sphere, the statics, the per-world-parameters or the report build: likewise, there is no stamped object of it -- the production kernel steps the worlds, every cycle count is 0)
  const mh_world_variant* stamped = (wb->has_forces || !g_builds[wb->build].prof) ? nullptr : g_builds[wb->build].prof();
  const int rc = launch_step(wb, (hipStream_t)nullptr, wb->B, dt, nsteps, nullptr, dprof, nullptr, nullptr, 1, nullptr, stamped);
  if (rc != MH_OK) { (void)hipFree(dprof); return rc; }
  hipError_t e = hipDeviceSynchronize();
  std::vector<unsigned long long> h((size_t)wb->B * PHC);
  if (e == hipSuccess) e = hipMemcpy(h.data(), dprof, sz, hipMemcpyDeviceToHost);
  (void)hipFree(dprof);
  if (e != hipSuccess) return fail(MH_ERR_HIP, "profile launch failed: %s", hipGetErrorString(e));
  for (int p = 0; p < nphase; p++) {
    double acc = 0.0;
    if (p < PHC) for (int b = 0; b < wb->B; b++) acc += (double)h[(size_t)b * PHC + p];
    phase_cycles[p] = acc / wb->B;
  }
  // entries PH_COUNT, PH_COUNT+1 (if asked for): the slowest and the fastest world's stamped total --
  // the launch lasts as long as its slowest world
  if (nphase >= PHC + 2) {
    double mx = 0.0, mn = 1e300;
    for (int b = 0; b < wb->B; b++) {
      double t = 0.0;
      for (int p = 0; p < 10; p++) t += (double)h[(size_t)b * PHC + p];
      mx = t > mx ? t : mx; mn = t < mn ? t : mn;
    }
    phase_cycles[PHC] = mx; phase_cycles[PHC + 1] = mn;
    // PH_COUNT + 2, + 3 (if asked for): the mean world's total, and the total of the world at the 99th percentile (1 % of the
    // worlds take longer): with the launch lasting `mx`, (mx - p99) / mx of it runs with under 1 % of the waves alive
    if (nphase >= PHC + 4) {
      std::vector<double> tt((size_t)wb->B);
      double sum = 0.0;
      for (int b = 0; b < wb->B; b++) { double t = 0.0; for (int p = 0; p < 10; p++) t += (double)h[(size_t)b * PHC + p]; tt[b] = t; sum += t; }
      std::sort(tt.begin(), tt.end());
      phase_cycles[PHC + 2] = sum / wb->B;
      phase_cycles[PHC + 3] = tt[(size_t)((wb->B - 1) * 0.99)];
    }
  }
  return MH_OK;
}

int mh_world_batch_download(mh_world_batch* wb, double* state, mh_world_aux* aux)
{
  if (!wb) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(wb);
  MH_HIP(hipDeviceSynchronize());
  if (state) MH_HIP(hipMemcpy(state, wb->d_state, (size_t)wb->B * wb->scene.nb * MH_BODY_STATE * sizeof(double), hipMemcpyDeviceToHost));
  if (aux) MH_HIP(hipMemcpy(aux, wb->d_aux, (size_t)wb->B * sizeof(mh_world_aux), hipMemcpyDeviceToHost));
  return MH_OK;
}

// The per-interval reduction of SURVEY 8(e), device side: what one device contributes to the node's SUM and MAX vectors, left in
// device memory for a collective (RCCL's ncclAllReduce) -- no host round trip, nothing per step.
namespace mh { namespace world_red {
__global__ __launch_bounds__(256)
void k_counters(const mh_world_aux* __restrict__ aux, int B, unsigned long long* __restrict__ sums, unsigned long long* __restrict__ maxs)
{
  __shared__ unsigned long long s_s[MH_COUNTERS][4], s_m[MH_COUNTERS][4];
  unsigned long long v[MH_COUNTERS] = { 0, 0, 0, 0, 0, 0, 0, 0 }, m[MH_COUNTERS] = { 0, 0, 0, 0, 0, 0, 0, 0 };
  for (int w = blockIdx.x * 256 + threadIdx.x; w < B; w += gridDim.x * 256) {
    const mh_world_aux& a = aux[w];
    const unsigned long long c[MH_COUNTERS] = { a.steps, a.lcp_rows, a.lcp_pivots, (unsigned long long)((a.status & ~MH_WORLD_IMPACT_TOL) != 0),
                                                a.lcp_solves, a.mini_steps, a.stab_iters, a.lcp_alg_bytes };
#pragma unroll
    for (int k = 0; k < MH_COUNTERS; k++) { v[k] += c[k]; m[k] = (c[k] > m[k]) ? c[k] : m[k]; }
  }
#pragma unroll
  for (int k = 0; k < MH_COUNTERS; k++) {
    for (int off = 32; off > 0; off >>= 1) { v[k] += __shfl_xor(v[k], off); const unsigned long long o = __shfl_xor(m[k], off); m[k] = (o > m[k]) ? o : m[k]; }
    if ((threadIdx.x & 63) == 0) { s_s[k][threadIdx.x >> 6] = v[k]; s_m[k][threadIdx.x >> 6] = m[k]; }
  }
  __syncthreads();
  if (threadIdx.x < MH_COUNTERS) {
    const int k = threadIdx.x;
    unsigned long long a = 0, b = 0;
    for (int q = 0; q < 4; q++) { a += s_s[k][q]; b = (s_m[k][q] > b) ? s_m[k][q] : b; }
    atomicAdd(sums + k, a); atomicMax(maxs + k, b);
  }
}
}}

int mh_world_batch_counters_dev(mh_world_batch* wb, void* stream, unsigned long long* sums_dev, unsigned long long* maxs_dev)
{
  if (!wb || !sums_dev || !maxs_dev) return fail(MH_ERR_INVALID_ARG, "null batch / buffer");
  MH_ON_DEVICE(wb);
  MH_HIP(hipMemsetAsync(sums_dev, 0, MH_COUNTERS * sizeof(unsigned long long), (hipStream_t)stream));
  MH_HIP(hipMemsetAsync(maxs_dev, 0, MH_COUNTERS * sizeof(unsigned long long), (hipStream_t)stream));
  const int grid = std::min((wb->B + 255) / 256, 1024);
  hipLaunchKernelGGL(mh::world_red::k_counters, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const mh_world_aux*)wb->d_aux, wb->B, sums_dev, maxs_dev);
  MH_HIP(hipGetLastError());
  return MH_OK;
}

int mh_world_batch_device_ptrs(mh_world_batch* wb, double** state_dev, mh_world_aux** aux_dev)
{
  if (!wb) return fail(MH_ERR_INVALID_ARG, "null batch");
  MH_ON_DEVICE(wb);
  if (state_dev) *state_dev = wb->d_state;
  if (aux_dev) *aux_dev = wb->d_aux;
  return MH_OK;
}

int mh_world_step_batch(const mh_scene* scene, int B, double dt, int nsteps,
                        double* state, mh_world_aux* aux, double* traj)
{
  return mh_world_step_batch_statics(scene, nullptr, B, dt, nsteps, state, aux, traj, nullptr);
}

int mh_world_step_batch_forces(const mh_scene* scene, const mh_world_forces* forces, int B, double dt, int nsteps,
                               double* state, mh_world_aux* aux, double* traj)
{
  return mh_world_step_batch_statics(scene, forces, B, dt, nsteps, state, aux, traj, nullptr);
}

int mh_world_step_batch_statics(const mh_scene* scene, const mh_world_forces* forces, int B, double dt, int nsteps,
                                double* state, mh_world_aux* aux, double* traj, const mh_world_statics* statics)
{
  return mh_world_step_batch_params(scene, forces, statics, nullptr, B, dt, nsteps, state, aux, traj);
}

int mh_world_step_batch_params(const mh_scene* scene, const mh_world_forces* forces, const mh_world_statics* statics, const mh_world_params* params,
                               int B, double dt, int nsteps, double* state, mh_world_aux* aux, double* traj)
{
  return mh_world_step_batch_report(scene, forces, statics, params, B, dt, nsteps, state, aux, traj, nullptr);
}

// report == NULL: mh_world_step_batch_params (a batch created by mh_world_batch_create_params); otherwise a report batch and its rows
int mh_world_step_batch_report(const mh_scene* scene, const mh_world_forces* forces, const mh_world_statics* statics, const mh_world_params* params,
                               int B, double dt, int nsteps, double* state, mh_world_aux* aux, double* traj, double* report)
{
  if (B == 0 || nsteps == 0) return MH_OK;
  if (B < 0 || nsteps < 0) return fail(MH_ERR_INVALID_ARG, "negative batch or step count");
  if (!state || !aux) return fail(MH_ERR_INVALID_ARG, "null state/aux");
  mh_world_batch* wb = nullptr;
  int rc = report ? mh_world_batch_create_report(scene, statics, params, B, &wb) : mh_world_batch_create_params(scene, statics, params, B, &wb);
  if (rc != MH_OK) return rc;
  double* dtraj = nullptr; double* drep = nullptr;
  const size_t sz_tr = (size_t)B * nsteps * scene->nb * 7 * sizeof(double);
  const int ntot = scene->nb + (scene->has_ground ? 1 : 0) + (statics ? statics->n : 0);
  const size_t sz_rep = (size_t)B * nsteps * (ntot * (ntot - 1) / 2) * MH_REPORT_PAIR * sizeof(double);
  rc = mh_world_batch_upload(wb, state, aux);
  if (rc == MH_OK && forces) rc = mh_world_batch_set_forces(wb, forces);
  if (rc == MH_OK && traj && hipMalloc(&dtraj, sz_tr) != hipSuccess) rc = fail(MH_ERR_HIP, "trajectory allocation failed");
  if (rc == MH_OK && report && sz_rep && hipMalloc(&drep, sz_rep) != hipSuccess) rc = fail(MH_ERR_HIP, "report allocation failed");
  if (rc == MH_OK) rc = mh_world_batch_step_report(wb, nullptr, dt, nsteps, dtraj, nullptr, 0, nullptr, 1, drep);
  if (rc == MH_OK) rc = mh_world_batch_download(wb, state, aux);
  if (rc == MH_OK && traj && hipMemcpy(traj, dtraj, sz_tr, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(MH_ERR_HIP, "trajectory download failed");
  if (rc == MH_OK && drep && hipMemcpy(report, drep, sz_rep, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(MH_ERR_HIP, "report download failed");
  if (dtraj) (void)hipFree(dtraj);
  if (drep) (void)hipFree(drep);
  mh_world_batch_destroy(wb);
  return rc;
}

} // extern "C"