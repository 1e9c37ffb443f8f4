// The articulated adapter's link wrenches: a box on a floating base standing on the ground, B copies each pushed sideways at the COM with its own
// force for 200 steps; every copy's drift and the normal impulse the ground returned, from the report written beside the step.
//   hipcc -std=c++17 example_artic_wrench.cpp -L.. -lmoby_hip -Wl,-rpath,.. -o example_artic_wrench     (g++ with the HIP include path and
//   -D__HIP_PLATFORM_AMD__ -lamdhip64 works too: the adapter header itself knows no HIP, the example owns the device arrays)
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime_api.h>
#include "MobyHipArticulatedBody.h"

int main()
{
  // a floating box: the six virtual joints of mh_artic_model.floating_base, link 5 the box (mass 2, edges 0.4 x 0.2 x 0.4), gravity along -y, the
  // plane y = 0, friction mu = 0.5 (the Drumwright-Shell model), so that a push above mu m g slides it
  mh_artic_model m; std::memset(&m, 0, sizeof(m));
  m.nj = 6; m.floating_base = 1; m.gravity[1] = -9.81; m.cstab_eps = 1.4901161193847656e-08;
  for (int v = 0; v < 6; v++) {
    m.parent[v] = v - 1; m.jtype[v] = v < 3 ? MH_JOINT_PRISMATIC : MH_JOINT_REVOLUTE; m.axis[v][v % 3] = 1.0;
    for (int k = 0; k < 3; k++) m.Rrel[v][4 * k] = 1.0;
    m.lolimit[v] = -1.7976931348623157e308; m.hilimit[v] = 1.7976931348623157e308;
  }
  m.mass[5] = 2.0; for (int k = 0; k < 3; k++) m.inertia[5][4 * k] = 0.05;
  const double origin[3] = { 0.0, 0.0, 0.0 }, up[3] = { 0.0, 1.0, 0.0 }, len[3] = { 0.4, 0.2, 0.4 };
  const double I3[9] = { 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0 };
  MobyHip::add_link_box(m, 5, origin, I3, len);
  MobyHip::set_ground_plane(m, up, origin, /*epsilon*/ 0.0, /*mu_coulomb*/ 0.5);
  const int B = 4, n = 200, nj = 6;
  std::vector<double> q((size_t)B * nj, 0.0), qd((size_t)B * nj, 0.0);
  for (int w = 0; w < B; w++) q[(size_t)w * nj + 1] = 0.1;                              // standing: the box's centre half an edge above the ground
  std::vector<double> push((size_t)B * nj * 6, 0.0);
  for (int w = 0; w < B; w++) push[((size_t)w * nj + 5) * 6 + 0] = 4.0 * w;             // 0, 4, 8, 12 N along x on the base link (mu m g = 9.81 N)
  MobyHip::BatchedArticulatedBody* r = NULL;
  double* rows_dev = NULL; double* push_dev = NULL;
  try {
    r = MobyHip::BatchedArticulatedBody::with_wrench(m, NULL, B, q.data(), qd.data(), /*report*/ true);
    const size_t cnt = (size_t)B * n * r->report_slots() * MH_REPORT_PAIR;
    if (hipMalloc((void**)&rows_dev, cnt * sizeof(double)) != hipSuccess || hipMalloc((void**)&push_dev, push.size() * sizeof(double)) != hipSuccess) throw std::runtime_error("hipMalloc failed");
    if (hipMemcpy(push_dev, push.data(), push.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    mh_artic_wrench wr; std::memset(&wr, 0, sizeof(wr));
    wr.terms = MH_LINK_WRENCH; wr.rows = 1; wr.w = push_dev;                           // one row, held for the whole launch
    r->step_wrench(1e-3, n, wr, rows_dev);
    std::vector<double> rows(cnt);
    if (hipMemcpy(rows.data(), rows_dev, cnt * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    bool ok = true;
    for (int w = 0; w < B; w++) {
      double cn = 0.0, fx = 0.0;
      for (int s = 0; s < n; s++) { const double* row = &rows[(((size_t)w * n + s) * r->report_slots()) * MH_REPORT_PAIR]; cn += row[1]; fx += row[2]; }
      std::printf("copy %d: push %4.1f N, drift x %.6f m, normal impulse %.6g, friction impulse x %.6g, status %d\n", w, 4.0 * w, r->q()[(size_t)w * nj], cn, fx, r->status(w));
      ok = ok && r->status(w) == 0 && cn > 0.0;
    }
    ok = ok && std::fabs(r->q()[0]) < r->q()[(size_t)3 * nj] && r->q()[(size_t)3 * nj] > r->q()[(size_t)1 * nj];     // the hardest push drifts furthest, the copy without a push least
    (void)hipFree(rows_dev); (void)hipFree(push_dev); delete r;
    return ok ? 0 : 1;
  } catch (const std::exception& e) { std::printf("error: %s\n", e.what()); if (rows_dev) (void)hipFree(rows_dev); if (push_dev) (void)hipFree(push_dev); delete r; return 1; }
}
