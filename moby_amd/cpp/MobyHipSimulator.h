// MobyHipSimulator.h -- reference-side adapter for the whole-step seam:
// a class with the calling conventions of Moby::TimeSteppingSimulator
// (/root/reference/include/Moby/TimeSteppingSimulator.h:36, include/Moby/Simulator.h:50) that advances
// B copies of one scene on the GPU through libmoby_hip.so.
//
//   MobyHip::BatchedTimeSteppingSimulator sim(scene, B, state);     // or ::from_xml(path, B) with libmoby_hip_io
//   sim.step(1e-3);                 // Simulator::step(dt): every world advances by dt; returns dt
//   sim.step(1e-3, 1000);           // the same step 1000 times inside ONE launch
//   sim.current_time;               // Simulator::current_time of world 0
//   sim.set_forces(forces);         // the simulator's recurrent forces besides gravity (StokesDragForce, DampingForce): mh_world_forces
//   sim.step_wrench(1e-3, wrench_dev);   // ... and what the bodies' controllers add_force this step: a DEVICE array B x nb x 6
//   MobyHip::BatchedTimeSteppingSimulator* s2 = MobyHip::BatchedTimeSteppingSimulator::with_statics(scene, statics, B, state);
//                                   // the same with static planes and boxes beside the scene's ground (mh_world_statics); delete it when done
//   MobyHip::BatchedTimeSteppingSimulator* s3 = MobyHip::BatchedTimeSteppingSimulator::with_params(scene, &statics /* or NULL */, params, B, state);
//                                   // ... and with one mh_world_params record per world: masses, shapes, gravity, frames, contact parameters of its own
//   s3->set_params(records, first, count);   // replaces the records of worlds first .. first + count - 1 between steps
//   MobyHip::BatchedTimeSteppingSimulator* s4 = MobyHip::BatchedTimeSteppingSimulator::with_report(scene, NULL, NULL, B, state);
//   s4->step_report(1e-3, 10);      // ... and with the per-pair contact impulse report (include/moby_hip.h, "Contact report")
//   const double* row = s4->report_row(w, /*step=*/9, /*pair slot=*/p);   // contacts, cn, impulse on the pair's lower body (3), point x cn (3)
//   sim.get_generalized_coordinates_euler(w, b, q);   // x y z qx qy qz qw of body b of world w
//
// Conventions kept from the reference: step() returns the step size; bodies are addressed in id order
// (programs/regress.cpp:66-69); exceptions of the reference become sticky per-world status bits
// (status(w) & MH_WORLD_LCP_FAILED <=> LCPSolverException, MH_WORLD_IMPACT_TOL <=> the warned
// ImpactToleranceException); the rand() stream of every world starts at srand(1) like a fresh process.
// Throws std::runtime_error only for a broken library / device / unsupported scene.
#ifndef MOBY_HIP_SIMULATOR_ADAPTER_H
#define MOBY_HIP_SIMULATOR_ADAPTER_H
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/moby_hip.h"

namespace MobyHip {

class BatchedTimeSteppingSimulator {
 public:
  double current_time;

  BatchedTimeSteppingSimulator(const mh_scene& scene, int B, const double* state /* B x nb x 13, or nb x 13 replicated if replicate */,
                               bool replicate = false)
      : current_time(0.0), _scene(scene), _B(B), _wb(NULL), _dirty(false), _report_on(false), _has_statics(false), _has_forces(false), _npt(0), _report_steps(0)
  {
    init(NULL, state, replicate);
  }
  /// The simulator of a scene with static bodies beside its ground (include/moby_hip.h, "Static bodies"): walls, tables, steps.  A named factory, not a
  /// constructor overload, so that no existing call can become ambiguous; the caller owns the object.
  static BatchedTimeSteppingSimulator* with_statics(const mh_scene& scene, const mh_world_statics& statics, int B, const double* state, bool replicate = false)
  {
    return new BatchedTimeSteppingSimulator(scene, &statics, NULL, B, state, replicate);
  }
  /// The simulator of B worlds that share the scene's topology and carry values of their own (include/moby_hip.h, "Per-world parameters"): `params` holds
  /// B records (mh_world_params_from_scene gives the one that reproduces the scene); statics may be NULL.  The caller owns the object.
  static BatchedTimeSteppingSimulator* with_params(const mh_scene& scene, const mh_world_statics* statics, const mh_world_params* params, int B, const double* state,
                                                   bool replicate = false)
  {
    return new BatchedTimeSteppingSimulator(scene, statics, params, B, state, replicate);
  }
  /// The same (statics and params may each be NULL) for a caller who wants the contact report (include/moby_hip.h, "Contact report"): what the reference hands
  /// to ConstraintSimulator::constraint_post_callback_fn, reduced per pair.  step_report() steps and keeps the launch's rows for report() / report_row().
  /// The simulator's batch is created by mh_world_batch_create_report, so step() and step_wrench() launch the report objects too (they write no rows).
  static BatchedTimeSteppingSimulator* with_report(const mh_scene& scene, const mh_world_statics* statics, const mh_world_params* params, int B, const double* state,
                                                   bool replicate = false)
  {
    BatchedTimeSteppingSimulator* s = new BatchedTimeSteppingSimulator(scene, statics, params, B, state, replicate, /*report=*/true);
    const int ntot = scene.nb + (scene.has_ground ? 1 : 0) + (statics ? statics->n : 0);
    s->_npt = ntot * (ntot - 1) / 2;
    if (statics) { s->_statics = *statics; s->_has_statics = true; }
    if (params) s->_params.assign(params, params + B);
    return s;
  }
  ~BatchedTimeSteppingSimulator() { if (_wb) mh_world_batch_destroy(_wb); }

  /// Simulator::step(dt), for every world; nsteps > 1 repeats it inside one launch
  double step(double dt, int nsteps = 1) {
    if (mh_world_batch_step(_wb, /*stream=*/NULL, dt, nsteps, /*traj=*/NULL) != MH_OK) throw std::runtime_error(mh_last_error());
    _dirty = true;
    current_time += dt * nsteps;
    return dt;
  }
  /// The simulator's recurrent forces besides gravity (Simulator::recurrent_forces: StokesDragForce, DampingForce), evaluated once per mini-step like the
  /// reference's; they hold for every later step of every world.  clear_forces() returns to gravity alone.
  void set_forces(const mh_world_forces& forces) {
    if (mh_world_batch_set_forces(_wb, &forces) != MH_OK) throw std::runtime_error(mh_last_error());
    _forces = forces; _has_forces = forces.terms != 0;                      // (step_report hands them to the host entry)
  }
  void clear_forces() { if (mh_world_batch_set_forces(_wb, NULL) != MH_OK) throw std::runtime_error(mh_last_error()); _has_forces = false; }
  /// Simulator::step(dt) with the wrenches the bodies' controllers would add_force: wrench_dev is a DEVICE array of rows x B x nb x 6 doubles
  /// (fx fy fz tx ty tz, world axes at the COM); rows == 1 holds it for all nsteps, rows >= nsteps is one row per step.  NULL: recurrent forces only.
  /// (A name of its own, not an overload of step: step(dt, NULL) would be ambiguous between a null pointer and nsteps = 0.)
  double step_wrench(double dt, const double* wrench_dev, int nsteps = 1, int rows = 1) {
    if (mh_world_batch_step_wrench(_wb, /*stream=*/NULL, dt, nsteps, /*traj=*/NULL, /*ids=*/NULL, 0, wrench_dev, rows) != MH_OK) throw std::runtime_error(mh_last_error());
    _dirty = true;
    current_time += dt * nsteps;
    return dt;
  }
  /// step(dt, nsteps) of a simulator made by with_report, keeping the rows of this launch: report() holds B x nsteps x npt x MH_REPORT_PAIR doubles until the
  /// next step_report().  It steps what step() would step: the forces stored by set_forces and the records as set_params left them hold here too.
  /// COST: this header knows no HIP and cannot own a device array, so every call goes through the host entry mh_world_step_batch_report -- it downloads
  /// state and solver records, creates a device batch for the call (allocations, record upload), steps it, fetches the rows, destroys it, and uploads state
  /// and records into the simulator's own batch again.  That is a convenience for reading loads now and then, not a stepping loop: a caller who wants the
  /// rows every step allocates a device array and passes it to mh_world_batch_step_report, which writes them where they are read.
  double step_report(double dt, int nsteps = 1) {
    if (!_report_on) throw std::runtime_error("step_report: the simulator was not made by with_report");
    sync();
    _report.assign((size_t)_B * nsteps * _npt * MH_REPORT_PAIR, 0.0);
    _report_steps = nsteps;
    if (mh_world_step_batch_report(&_scene, _has_forces ? &_forces : NULL, _has_statics ? &_statics : NULL, _params.empty() ? NULL : _params.data(), _B, dt, nsteps, _state.data(), _aux.data(),
                                   NULL, _report.data()) != MH_OK) throw std::runtime_error(mh_last_error());
    if (mh_world_batch_upload(_wb, _state.data(), _aux.data()) != MH_OK) throw std::runtime_error(mh_last_error());
    current_time += dt * nsteps;
    return dt;
  }
  /// The rows of the last step_report(): world w, step s of that launch, pair slot p (triangular over nb + has_ground + n bodies) -> MH_REPORT_PAIR doubles
  const std::vector<double>& report() const { return _report; }
  const double* report_row(int w, int s, int p) const { return &_report[(((size_t)w * _report_steps + s) * _npt + p) * MH_REPORT_PAIR]; }
  int num_pair_slots() const { return _npt; }
  /// Replaces the records of worlds first .. first + count - 1 (a simulator made with records only: with_params, or with_report with params != NULL); not
  /// while a step is in flight on another stream.
  void set_params(const mh_world_params* records, int first, int count) {
    if (mh_world_batch_set_params(_wb, records, first, count) != MH_OK) throw std::runtime_error(mh_last_error());
    if (!_params.empty()) for (int k = 0; k < count; k++) _params[(size_t)(first + k)] = records[k];      // (the library checked the range; step_report reads these)
  }
  int num_worlds() const { return _B; }
  int num_bodies() const { return _scene.nb; }
  /// DynamicBodyd::get_generalized_coordinates_euler of body b of world w
  void get_generalized_coordinates_euler(int w, int b, double q[7]) { sync(); for (int k = 0; k < 7; k++) q[k] = _state[((size_t)w * _scene.nb + b) * MH_BODY_STATE + k]; }
  /// get_generalized_velocity(eSpatial): linear (COM, world axes) then angular
  void get_generalized_velocity(int w, int b, double v[6]) { sync(); for (int k = 0; k < 6; k++) v[k] = _state[((size_t)w * _scene.nb + b) * MH_BODY_STATE + 7 + k]; }
  int status(int w) { sync(); return _aux[(size_t)w].status; }
  const mh_world_aux& solver_state(int w) { sync(); return _aux[(size_t)w]; }   // what a checkpoint must keep besides the body state
  const std::vector<double>& state() { sync(); return _state; }

 private:
  BatchedTimeSteppingSimulator(const mh_scene& scene, const mh_world_statics* statics, const mh_world_params* params, int B, const double* state, bool replicate,
                               bool report = false)
      : current_time(0.0), _scene(scene), _B(B), _wb(NULL), _dirty(false), _report_on(report), _has_statics(false), _has_forces(false), _npt(0), _report_steps(0)
  {
    init(statics, state, replicate, params);
  }
  void init(const mh_world_statics* statics, const double* state, bool replicate, const mh_world_params* params = NULL)
  {
    const int rc = _report_on ? mh_world_batch_create_report(&_scene, statics, params, _B, &_wb) : mh_world_batch_create_params(&_scene, statics, params, _B, &_wb);
    if (rc != MH_OK) throw std::runtime_error(mh_last_error());
    const size_t nst = (size_t)_scene.nb * MH_BODY_STATE;
    _state.resize((size_t)_B * nst);
    for (int w = 0; w < _B; w++) for (size_t k = 0; k < nst; k++) _state[(size_t)w * nst + k] = state[replicate ? k : (size_t)w * nst + k];
    _aux.resize((size_t)_B);
    mh_world_aux_init(&_aux[0], 1);
    for (int w = 1; w < _B; w++) _aux[(size_t)w] = _aux[0];
    if (mh_world_batch_upload(_wb, _state.data(), NULL) != MH_OK) { mh_world_batch_destroy(_wb); _wb = NULL; throw std::runtime_error(mh_last_error()); }
  }
  BatchedTimeSteppingSimulator(const BatchedTimeSteppingSimulator&);
  BatchedTimeSteppingSimulator& operator=(const BatchedTimeSteppingSimulator&);
  void sync() {
    if (!_dirty) return;
    if (mh_world_batch_download(_wb, _state.data(), _aux.data()) != MH_OK) throw std::runtime_error(mh_last_error());
    _dirty = false;
  }
  mh_scene _scene; int _B; mh_world_batch* _wb; bool _dirty;
  std::vector<double> _state; std::vector<mh_world_aux> _aux;
  bool _report_on, _has_statics, _has_forces; int _npt, _report_steps;    // with_report: the scene's statics, records and stored forces (the host entry takes them again)
  mh_world_forces _forces; mh_world_statics _statics; std::vector<mh_world_params> _params; std::vector<double> _report;
};

} // namespace MobyHip
#endif
