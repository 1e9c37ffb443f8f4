// MobyHipArticulatedBody.h -- reference-side adapter for fixed-base articulated bodies (include/moby_hip_artic.h): the
// forward-dynamics seam B4 (Ravelin::RCArticulatedBodyd::calc_fwd_dyn / get_generalized_inertia as Moby calls them:
// src/Simulator.cpp:552, src/ImpactConstraintHandler.cpp:1600-1607) and the whole-step seam for B copies of one model.
//
//   mh_io_artic io; mh_io_load_sdf("model.sdf", gravity, &io);        // or fill mh_artic_model from Moby's Joint / RigidBody objects
//   MobyHip::BatchedArticulatedBody robots(io.model, B, q, qd);
//   robots.calc_fwd_dyn(tau, qdd);                 // qdd = H^-1 (tau - C) for every copy (tau may be NULL)
//   robots.get_generalized_inertia(H);             // B x nj x nj, row-major
//   robots.step(5e-4, 200);                        // TimeSteppingSimulator::step x 200 in one launch (joint limits included)
//   mh_artic_drive servo = { MH_DRIVE_PD, 1, kp, kv, q_des, qd_des, NULL };   // host arrays, B x nj (a controller plugin's PD law)
//   robots.set_drive(servo); robots.step(5e-4, 200);   // ... now driven once per mini-step
//   floater.set_base_coords(MH_ARTIC_BASE_POSE);     // a floating base carried as a pose per copy (no singular middle hinge)
//   floater.base_pose(P); floater.set_base_pose(P);   // B x 7: COM px py pz, unit quaternion qw qx qy qz (checkpoint = q(), qd(), base_pose)
//
// Collision geometry (sphere and box primitives on links against one static plane, contacts with mu-coulomb >= 100 as ur10.xml:19 has
// them) is part of the model: fill it before constructing the batch, e.g.
//   MobyHip::add_link_sphere(io.model, finger_link, centre_in_link_frame, 0.03);     // <Sphere> CollisionGeometry on a link
//   MobyHip::add_link_box(io.model, foot_link, centre_in_link_frame, R_in_link_frame, lengths);   // <Box> CollisionGeometry on a link
//   MobyHip::add_sphere_pair(io.model, 0, 1);                                        // spheres 0 and 1 (on different links) can collide
//   MobyHip::add_box_sphere_pair(io.model, 0, 1);                                    // box 0 and sphere 1 (on different links; the box may be static: link -1)
//   MobyHip::set_ground_plane(io.model, normal, point_on_plane, /*epsilon*/ 0.0, /*mu_coulomb*/ 100.0);
// step() then runs TimeSteppingSimulator::step in full: conservative advancement, mini-steps, contact + limit rows in one LCP.
//
// The contact report (include/moby_hip_artic.h, "Contact report": what ConstraintSimulator::constraint_post_callback_fn would see, reduced per
// slot -- sphere on the plane, box on the plane, pair -- inside the step):
//   MobyHip::BatchedArticulatedBody* r = MobyHip::BatchedArticulatedBody::with_report(model, B, q, qd);
//   double* rows_dev;  hipMalloc(&rows_dev, sizeof(double) * B * n * r->report_slots() * MH_REPORT_PAIR);   // the caller owns the device array
//   r->step_report(1e-3, n, rows_dev);             // row of world w, step s, slot k at rows_dev + ((w * n + s) * report_slots() + k) * MH_REPORT_PAIR
//
// Episodes on the device (include/moby_hip_artic.h, "Episodes on the device": device arrays of the caller, stream-ordered, no host round trip):
//   robots.link_poses_dev(poses_dev);              // B x nj x 12: where the tip is -- the caller's kernel fills done_dev (B ints) from it
//   robots.reset_dev(done_dev, q0_dev, qd0_dev);   // a new episode in the copies whose done_dev is nonzero; the others are not touched
//   robots.status_dev(status_dev);                 // B ints: which copies carry MH_WORLD_LCP_FAILED / _STALLED / _UNSUPPORTED
//
// Generalized coordinates / velocities are the joint positions / velocities in the model's joint order (parents first),
// as get_generalized_coordinates_euler / get_generalized_velocity return them for a fixed-base RCArticulatedBody.
#ifndef MOBY_HIP_ARTICULATED_ADAPTER_H
#define MOBY_HIP_ARTICULATED_ADAPTER_H
#include <cmath>
#include <stdexcept>
#include <vector>
#include "../../include/moby_hip_artic.h"

namespace MobyHip {

// CollisionGeometry of a SpherePrimitive on link `link` (centre in the link frame)
inline void add_link_sphere(mh_artic_model& m, int link, const double centre[3], double radius)
{
  if (m.nspheres >= MH_ARTIC_MAX_SPHERES) throw std::runtime_error("MobyHip::add_link_sphere: more than MH_ARTIC_MAX_SPHERES spheres");
  const int s = m.nspheres++;
  m.sphere_link[s] = link; m.sphere_radius[s] = radius;
  for (int k = 0; k < 3; k++) m.sphere_center[s][k] = centre[k];
}
// CollisionGeometry of a BoxPrimitive on link `link`: centre and axes (row-major R, orthonormal) in the link frame, full edge lengths
// xlen ylen zlen (include/moby_hip_artic.h, mh_artic_model.nboxes); it meets the same plane as the spheres
inline void add_link_box(mh_artic_model& m, int link, const double centre[3], const double R[9], const double lengths[3])
{
  if (m.nboxes >= MH_ARTIC_MAX_BOXES) throw std::runtime_error("MobyHip::add_link_box: more than MH_ARTIC_MAX_BOXES boxes");
  const int b = m.nboxes++;
  m.box_link[b] = link;
  for (int k = 0; k < 3; k++) { m.box_center[b][k] = centre[k]; m.box_len[b][k] = lengths[k]; }
  for (int k = 0; k < 9; k++) m.box_R[b][k] = R[k];
}
// A sphere contact between links: spheres a and b of the model's sphere list (add_link_sphere first), on different links; a is the reference's
// geometry A, the contact normal points from b to a (include/moby_hip_artic.h, mh_artic_model.npairs).  The pair shares the ContactParameters
// of set_ground_plane.  meets_plane_a / _b = false takes that sphere off the plane (mh_artic_model.sphere_no_plane).
inline void add_sphere_pair(mh_artic_model& m, int a, int b, bool meets_plane_a = true, bool meets_plane_b = true)
{
  if (m.npairs >= MH_ARTIC_MAX_PAIRS) throw std::runtime_error("MobyHip::add_sphere_pair: more than MH_ARTIC_MAX_PAIRS pairs");
  if (a < 0 || a >= m.nspheres || b < 0 || b >= m.nspheres || a == b) throw std::runtime_error("MobyHip::add_sphere_pair: two different spheres of the sphere list");
  const int k = m.npairs++;
  m.pair_a[k] = a; m.pair_b[k] = b;
  if (!meets_plane_a) m.sphere_no_plane |= 1 << a;
  if (!meets_plane_b) m.sphere_no_plane |= 1 << b;
}
// A box-sphere contact between links: box `box` of the model's box list (add_link_box first; link -1 = a static box whose centre and R are given
// in the model frame) and sphere `sphere` of its sphere list, on different links; the box is the reference's geometry A
// (include/moby_hip_artic.h, mh_artic_model.pair_kind).  The pair shares the ContactParameters of set_ground_plane.  sphere_meets_plane = false
// takes the sphere off the plane.
inline void add_box_sphere_pair(mh_artic_model& m, int box, int sphere, bool sphere_meets_plane = true)
{
  if (m.npairs >= MH_ARTIC_MAX_PAIRS) throw std::runtime_error("MobyHip::add_box_sphere_pair: more than MH_ARTIC_MAX_PAIRS pairs");
  if (box < 0 || box >= m.nboxes || sphere < 0 || sphere >= m.nspheres) throw std::runtime_error("MobyHip::add_box_sphere_pair: a box of the box list and a sphere of the sphere list");
  const int k = m.npairs++;
  m.pair_a[k] = box; m.pair_b[k] = sphere; m.pair_kind[k] = MH_ARTIC_PAIR_BOX_SPHERE;
  if (!sphere_meets_plane) m.sphere_no_plane |= 1 << sphere;
}
// The static PlanePrimitive (its +Y axis is the normal, PlanePrimitive.cpp) through `point`, and the ContactParameters of the
// (robot, plane) pair; simulator constants at the reference's defaults (TimeSteppingSimulator.cpp:48, ConstraintSimulator.cpp:56)
inline void set_ground_plane(mh_artic_model& m, const double normal[3], const double point[3], double epsilon, double mu_coulomb)
{
  double n[3] = { normal[0], normal[1], normal[2] };
  const double len = std::sqrt(n[0]*n[0] + n[1]*n[1] + n[2]*n[2]);
  for (int k = 0; k < 3; k++) n[k] /= len;
  int a = 0; for (int k = 1; k < 3; k++) if (std::fabs(n[k]) < std::fabs(n[a])) a = k;
  double e[3] = { 0.0, 0.0, 0.0 }; e[a] = 1.0;
  double x[3] = { n[1]*e[2] - n[2]*e[1], n[2]*e[0] - n[0]*e[2], n[0]*e[1] - n[1]*e[0] };
  const double xl = std::sqrt(x[0]*x[0] + x[1]*x[1] + x[2]*x[2]);
  for (int k = 0; k < 3; k++) x[k] /= xl;
  const double z[3] = { x[1]*n[2] - x[2]*n[1], x[2]*n[0] - x[0]*n[2], x[0]*n[1] - x[1]*n[0] };
  for (int k = 0; k < 3; k++) { m.plane_R[3*k] = x[k]; m.plane_R[3*k+1] = n[k]; m.plane_R[3*k+2] = z[k]; m.plane_o[k] = point[k]; }
  m.cp_epsilon = epsilon; m.cp_mu_coulomb = mu_coulomb; m.cp_mu_viscous = 0.0; m.cp_compliance = 0.0; m.cp_nk = 4;   // set the last three directly for the D-S model
  m.min_step_size = 1.4901161193847656e-08; m.contact_dist_thresh = 1e-6;
}

class BatchedArticulatedBody {
 public:
  BatchedArticulatedBody(const mh_artic_model& model, int B, const double* q, const double* qd) : _nj(model.nj), _B(B), _ab(NULL), _dirty(false), _nslots(-1)
  { init(model, q, qd, false); }
  /// A batch whose steps can report contact impulses (mh_artic_batch_create_report: it steps through the report kernels, whatever its geometry;
  /// step() writes no rows).  The model needs at least one sphere, box or pair.
  static BatchedArticulatedBody* with_report(const mh_artic_model& model, int B, const double* q, const double* qd)
  { return new BatchedArticulatedBody(model, B, q, qd, true); }
  /// A batch whose copies each step their own VALUES of the model (mh_artic_batch_create_params; include/moby_hip_artic.h, "Per-world parameters"):
  /// params holds B records (NULL: every record = the model; mh_artic_params_from_model writes the one that reproduces a model), copy w steps as
  /// a batch of the model with record w written into it would.  report = true makes it a report batch too (step_report).  The topology -- joints,
  /// geometry lists, which limits are finite -- stays the model's.
  static BatchedArticulatedBody* with_params(const mh_artic_model& model, const mh_artic_params* params, int B, const double* q, const double* qd, bool report = false)
  { return new BatchedArticulatedBody(model, B, q, qd, report, true, params); }
  /// Replaces the records of copies first .. first + count - 1 (HOST records, validated; a refused record leaves every copy as it was)
  void set_params(const mh_artic_params* params, int first, int count) { if (mh_artic_batch_set_params(_ab, params, first, count) != MH_OK) throw std::runtime_error(mh_last_error()); }
  /// A with_params batch that also takes forces on its links (mh_artic_batch_create_wrench; include/moby_hip_artic.h, "Link wrenches"): what a
  /// controller of the reference does with link->add_force(...), and DampingForce on an articulated body.  params NULL: every record = the model.
  static BatchedArticulatedBody* with_wrench(const mh_artic_model& model, const mh_artic_params* params, int B, const double* q, const double* qd, bool report = false)
  { return new BatchedArticulatedBody(model, B, q, qd, report, true, params, true); }
  /// step(dt, nsteps) with the wrench applied inside every mini-step: its pointers are DEVICE arrays the caller owns (this header knows no HIP),
  /// read in the order of the null stream; report_dev as step_report's, or NULL.  With the drive of set_drive when one is set.
  double step_wrench(double dt, int nsteps, const mh_artic_wrench& wrench, double* report_dev = NULL) {
    if (mh_artic_batch_step_wrench(_ab, NULL, dt, nsteps, NULL, &wrench, report_dev) != MH_OK) throw std::runtime_error(mh_last_error());
    _dirty = true; return dt;
  }
  /// Episodes on the device (include/moby_hip_artic.h, "Episodes on the device"): DEVICE arrays the caller owns, ordered on `stream` (NULL: the
  /// null stream), no synchronisation.  reset_dev: copy w starts a new episode iff mask_dev[w] != 0 (NULL: every copy) from its rows of q_src,
  /// qd_src (B x nj) and pose_src (B x 7, pose coordinates only), NULL leaving that array; its aux record becomes a fresh one.  NOT validated.
  void reset_dev(const int* mask_dev, const double* q_src, const double* qd_src, const double* pose_src = NULL, void* stream = NULL) {
    if (mh_artic_batch_reset_dev(_ab, stream, mask_dev, q_src, qd_src, pose_src) != MH_OK) throw std::runtime_error(mh_last_error());
    _dirty = true;
  }
  /// every copy's status bits (B ints) and time (B doubles) into device arrays; either may be NULL
  void status_dev(int* status_dst, double* time_dst = NULL, void* stream = NULL) { if (mh_artic_batch_status_dev(_ab, stream, status_dst, time_dst) != MH_OK) throw std::runtime_error(mh_last_error()); }
  /// the link poses of the resident states (B x nj x 12: row-major R, origin; model frame) into a device array
  void link_poses_dev(double* poses_dst, void* stream = NULL) { if (mh_artic_batch_link_poses_dev(_ab, stream, poses_dst) != MH_OK) throw std::runtime_error(mh_last_error()); }
  /// nspheres + nboxes + npairs of a batch made by with_report: the rows per world and step
  int report_slots() const { return _nslots; }
  /// step(dt, nsteps) with the launch's rows written to report_dev, a DEVICE array of B x nsteps x report_slots() x MH_REPORT_PAIR doubles that the
  /// caller owns (this header knows no HIP); the rows are written in the order of the null stream.  With the drive of set_drive when one is set.
  double step_report(double dt, int nsteps, double* report_dev) {
    if (_nslots < 0) throw std::runtime_error("step_report: the batch was not made by with_report");
    if (mh_artic_batch_step_report(_ab, NULL, dt, nsteps, NULL, report_dev) != MH_OK) throw std::runtime_error(mh_last_error());
    _dirty = true; return dt;
  }
  ~BatchedArticulatedBody() { if (_ab) mh_artic_batch_destroy(_ab); }
  void set_generalized_coordinates_euler(const double* q) { _q.assign(q, q + _q.size()); if (mh_artic_batch_upload(_ab, _q.data(), NULL, NULL) != MH_OK) throw std::runtime_error(mh_last_error()); }
  void set_generalized_velocity(const double* qd) { _qd.assign(qd, qd + _qd.size()); if (mh_artic_batch_upload(_ab, NULL, _qd.data(), NULL) != MH_OK) throw std::runtime_error(mh_last_error()); }
  void calc_fwd_dyn(const double* tau /* B x nj or NULL */, double* qdd /* B x nj */) { if (mh_artic_batch_fwd_dyn(_ab, tau, qdd, NULL) != MH_OK) throw std::runtime_error(mh_last_error()); }
  void get_generalized_inertia(double* H /* B x nj x nj */) { std::vector<double> qdd((size_t)_B * _nj); if (mh_artic_batch_fwd_dyn(_ab, NULL, qdd.data(), H) != MH_OK) throw std::runtime_error(mh_last_error()); }
  // joint forces / PD servos evaluated inside every mini-step (mh_artic_drive: HOST arrays, copied to the device); terms = 0 clears
  void set_drive(const mh_artic_drive& drive) { if (mh_artic_batch_set_drive(_ab, &drive) != MH_OK) throw std::runtime_error(mh_last_error()); }
  // floating bases: MH_ARTIC_BASE_POSE folds the virtual joints into a per-copy base pose after every step (include/moby_hip_artic.h); one way
  void set_base_coords(int coords) { if (mh_artic_batch_set_base_coords(_ab, coords) != MH_OK) throw std::runtime_error(mh_last_error()); _dirty = true; }
  int base_coords() const { int c = 0; if (mh_artic_batch_base_coords(_ab, &c) != MH_OK) throw std::runtime_error(mh_last_error()); return c; }
  void base_pose(double* pose /* B x 7 */) { if (mh_artic_batch_base_pose(_ab, pose) != MH_OK) throw std::runtime_error(mh_last_error()); }
  void set_base_pose(const double* pose /* B x 7 */) { if (mh_artic_batch_set_base_pose(_ab, pose) != MH_OK) throw std::runtime_error(mh_last_error()); }
  // with the drive of set_drive when one is set
  double step(double dt, int nsteps = 1) { if (mh_artic_batch_step_driven(_ab, NULL, dt, nsteps, NULL) != MH_OK) throw std::runtime_error(mh_last_error()); _dirty = true; return dt; }
  const std::vector<double>& q() { sync(); return _q; }
  const std::vector<double>& qd() { sync(); return _qd; }
  int status(int w) { sync(); return _aux[(size_t)w].status; }
  const mh_world_aux& aux(int w) { sync(); return _aux[(size_t)w]; }   // counters: mini_steps, lcp_solves, lcp_rows ...
  int num_joints() const { return _nj; }
 private:
  BatchedArticulatedBody(const BatchedArticulatedBody&);
  BatchedArticulatedBody& operator=(const BatchedArticulatedBody&);
  BatchedArticulatedBody(const mh_artic_model& model, int B, const double* q, const double* qd, bool report, bool with_records = false, const mh_artic_params* params = NULL, bool wrench = false)
    : _nj(model.nj), _B(B), _ab(NULL), _dirty(false), _nslots(-1)
  { init(model, q, qd, report, with_records, params, wrench); }
  void init(const mh_artic_model& model, const double* q, const double* qd, bool report, bool with_records = false, const mh_artic_params* params = NULL, bool wrench = false)
  {
    const int rc = wrench ? mh_artic_batch_create_wrench(&model, params, _B, report ? MH_ARTIC_CREATE_REPORT : 0, &_ab)
                 : with_records ? mh_artic_batch_create_params(&model, params, _B, report ? MH_ARTIC_CREATE_REPORT : 0, &_ab)
                                : report ? mh_artic_batch_create_report(&model, _B, &_ab) : mh_artic_batch_create(&model, _B, &_ab);
    if (rc != MH_OK) throw std::runtime_error(mh_last_error());
    if (report) _nslots = mh_artic_report_slots(&model);
    _q.assign(q, q + (size_t)_B * _nj); _qd.assign(qd, qd + (size_t)_B * _nj); _aux.resize((size_t)_B);
    if (mh_artic_batch_upload(_ab, _q.data(), _qd.data(), NULL) != MH_OK) { mh_artic_batch_destroy(_ab); _ab = NULL; throw std::runtime_error(mh_last_error()); }
  }
  void sync() { if (!_dirty) return; if (mh_artic_batch_download(_ab, _q.data(), _qd.data(), _aux.data()) != MH_OK) throw std::runtime_error(mh_last_error()); _dirty = false; }
  int _nj, _B; mh_artic_batch* _ab; bool _dirty; int _nslots;
  std::vector<double> _q, _qd; std::vector<mh_world_aux> _aux;
};

} // namespace MobyHip
#endif
