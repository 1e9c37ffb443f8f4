// The batched simulator adapter on a scene file: 100 calls of step(dt) against one call of step(dt, 100).
//   g++ -std=c++11 example_world.cpp -L.. -lmoby_hip -lmoby_hip_io -Wl,-rpath,.. -o example_world
//   ./example_world ../../tests/scenes/three_spheres_on_a_plane.xml
#include <cstdio>
#include <cstring>
#include "MobyHipSimulator.h"
#include "../../include/moby_hip_io.h"

static bool same_drag_is_plain(const std::vector<double>& a, const std::vector<double>& b) { return std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; }

int main(int argc, char** argv)
{
  if (argc < 2) { std::printf("usage: example_world <scene.xml>\n"); return 2; }
  mh_io_scene io;
  if (mh_io_load_xml(argv[1], &io) != 0) { std::printf("error: %s\n", mh_io_last_error()); return 1; }
  try {
    const int B = 4;
    MobyHip::BatchedTimeSteppingSimulator a(io.scene, B, io.state, /*replicate=*/true), b(io.scene, B, io.state, true);
    for (int s = 0; s < 100; s++) a.step(1e-3);
    b.step(1e-3, 100);
    const bool same = std::memcmp(a.state().data(), b.state().data(), a.state().size() * sizeof(double)) == 0;
    double q[7]; a.get_generalized_coordinates_euler(0, io.scene.nb - 1, q);
    std::printf("worlds=%d bodies=%d time=%.3f same=%d status=%d top body: %.9g %.9g %.9g\n", a.num_worlds(), a.num_bodies(), a.current_time, (int)same,
                a.status(0), q[0], q[1], q[2]);
    // the same under Stokes drag (a StokesDragForce among the simulator's recurrent forces): once per mini-step inside the launch, so the split run equals the single one
    mh_world_forces drag; std::memset(&drag, 0, sizeof(drag));
    drag.terms = MH_FORCE_STOKES;
    for (int k = 0; k < io.scene.nb; k++) { drag.stokes_b[k] = 0.3; drag.stokes_b_ang[k] = 0.05; }
    MobyHip::BatchedTimeSteppingSimulator c(io.scene, B, io.state, true), d(io.scene, B, io.state, true);
    c.set_forces(drag); d.set_forces(drag);
    for (int s = 0; s < 100; s++) c.step_wrench(1e-3, /*wrench_dev=*/NULL);
    d.step_wrench(1e-3, NULL, 100);
    const bool same_drag = std::memcmp(c.state().data(), d.state().data(), c.state().size() * sizeof(double)) == 0;
    std::printf("with drag: same_drag=%d status=%d\n", (int)same_drag, c.status(0));
    // per-world parameters: the same topology, gravity weaker from world to world; world 0 keeps the scene and must equal the plain simulator
    std::vector<mh_world_params> rec((size_t)B);
    for (int w = 0; w < B; w++) {
      mh_world_params_from_scene(&io.scene, /*statics=*/NULL, &rec[w]);
      for (int k = 0; k < 3; k++) rec[w].gravity[k] *= 1.0 - 0.1 * w;
    }
    MobyHip::BatchedTimeSteppingSimulator* e = MobyHip::BatchedTimeSteppingSimulator::with_params(io.scene, NULL, rec.data(), B, io.state, true);
    e->step(1e-3, 50);
    e->set_params(&rec[0], /*first=*/1, /*count=*/1);          // world 1 gets the scene's gravity back for the second half
    e->step(1e-3, 50);
    const size_t nst = (size_t)io.scene.nb * MH_BODY_STATE;
    const bool same_w0 = std::memcmp(e->state().data(), b.state().data(), nst * sizeof(double)) == 0;
    const bool differ = std::memcmp(e->state().data() + 3 * nst, b.state().data() + 3 * nst, nst * sizeof(double)) != 0;
    std::printf("per-world gravity: same_w0=%d world 3 differs=%d status=%d\n", (int)same_w0, (int)differ, e->status(3));
    delete e;
    // the contact report: the same worlds with the per-pair impulse rows of each step; the state must equal the plain simulator's, and the normal impulses
    // of the 100 steps must be what holds the spheres up somewhere (a positive sum)
    MobyHip::BatchedTimeSteppingSimulator* r = MobyHip::BatchedTimeSteppingSimulator::with_report(io.scene, NULL, NULL, B, io.state, true);
    r->step_report(1e-3, 100);
    const bool same_rep = std::memcmp(r->state().data(), b.state().data(), b.state().size() * sizeof(double)) == 0;
    double cn_sum = 0.0, contacts = 0.0;
    for (int s = 0; s < 100; s++) for (int p = 0; p < r->num_pair_slots(); p++) { contacts += r->report_row(0, s, p)[0]; cn_sum += r->report_row(0, s, p)[1]; }
    std::printf("contact report: same_state=%d contacts=%g sum cn=%g\n", (int)same_rep, contacts, cn_sum);
    // ... and under the drag: step_report steps what step steps, so it must end where the drag simulator `d` ended (not where the plain one did)
    MobyHip::BatchedTimeSteppingSimulator* q2 = MobyHip::BatchedTimeSteppingSimulator::with_report(io.scene, NULL, NULL, B, io.state, true);
    q2->set_forces(drag);
    q2->step_report(1e-3, 50);
    q2->step_wrench(1e-3, NULL, 50);
    const bool same_rep_drag = std::memcmp(q2->state().data(), d.state().data(), d.state().size() * sizeof(double)) == 0 && !same_drag_is_plain(d.state(), b.state());
    std::printf("contact report with drag: same_rep_drag=%d\n", (int)same_rep_drag);
    delete q2;
    delete r;
    return (same && same_drag && same_w0 && differ && same_rep && same_rep_drag && cn_sum > 0.0 && contacts > 0.0) ? 0 : 1;
  } catch (const std::exception& e) { std::printf("error: %s\n", e.what()); return 1; }
}
