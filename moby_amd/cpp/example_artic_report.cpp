// The articulated adapter's contact report: a ball on a floating base dropped onto the ground, B copies from different heights; every step's
// normal impulse and contact count per copy, read back from the device array the report was written to.
//   hipcc -std=c++17 example_artic_report.cpp -L.. -lmoby_hip -Wl,-rpath,.. -o example_artic_report     (g++ with the HIP include path and
//   -D__HIP_PLATFORM_AMD__ -lamdhip64 works too: the adapter header itself knows no HIP, the example owns the device array)
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime_api.h>
#include "MobyHipArticulatedBody.h"

int main()
{
  // a floating ball: the six virtual joints of mh_artic_model.floating_base, link 5 the ball (mass 2, radius 0.5), gravity along -y, the plane y = 0
  mh_artic_model m; std::memset(&m, 0, sizeof(m));
  m.nj = 6; m.floating_base = 1; m.gravity[1] = -9.81; m.cstab_eps = 1.4901161193847656e-08;
  for (int v = 0; v < 6; v++) {
    m.parent[v] = v - 1; m.jtype[v] = v < 3 ? MH_JOINT_PRISMATIC : MH_JOINT_REVOLUTE; m.axis[v][v % 3] = 1.0;
    for (int k = 0; k < 3; k++) m.Rrel[v][4 * k] = 1.0;
    m.lolimit[v] = -1.7976931348623157e308; m.hilimit[v] = 1.7976931348623157e308;
  }
  m.mass[5] = 2.0; for (int k = 0; k < 3; k++) m.inertia[5][4 * k] = 0.2;
  const double origin[3] = { 0.0, 0.0, 0.0 }, up[3] = { 0.0, 1.0, 0.0 };
  MobyHip::add_link_sphere(m, 5, origin, 0.5);
  MobyHip::set_ground_plane(m, up, origin, /*epsilon*/ 0.25, /*mu_coulomb*/ 100.0);
  const int B = 4, n = 200;
  std::vector<double> q((size_t)B * 6, 0.0), qd((size_t)B * 6, 0.0);
  for (int w = 0; w < B; w++) q[(size_t)w * 6 + 1] = 0.5 + 0.002 * (w + 1);           // the ball's centre: 2, 4, 6, 8 mm above touching
  MobyHip::BatchedArticulatedBody* r = NULL;
  double* rows_dev = NULL;
  try {
    r = MobyHip::BatchedArticulatedBody::with_report(m, B, q.data(), qd.data());
    const size_t cnt = (size_t)B * n * r->report_slots() * MH_REPORT_PAIR;
    if (hipMalloc((void**)&rows_dev, cnt * sizeof(double)) != hipSuccess) throw std::runtime_error("hipMalloc failed");
    r->step_report(1e-3, n, rows_dev);
    std::vector<double> rows(cnt);
    if (hipMemcpy(rows.data(), rows_dev, cnt * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    bool ok = true;
    for (int w = 0; w < B; w++) {
      double cn = 0.0, contacts = 0.0; int first = -1;
      for (int s = 0; s < n; s++) { const double* row = &rows[(((size_t)w * n + s) * r->report_slots()) * MH_REPORT_PAIR]; contacts += row[0]; cn += row[1]; if (first < 0 && row[1] > 0.0) first = s; }
      std::printf("copy %d: first impact in step %d, contacts %.0f, normal impulse %.6g, status %d\n", w, first, contacts, cn, r->status(w));
      ok = ok && first >= 0 && cn > 0.0 && r->status(w) == 0;
    }
    (void)hipFree(rows_dev); delete r;
    return ok ? 0 : 1;
  } catch (const std::exception& e) { std::printf("error: %s\n", e.what()); if (rows_dev) (void)hipFree(rows_dev); delete r; return 1; }
}
