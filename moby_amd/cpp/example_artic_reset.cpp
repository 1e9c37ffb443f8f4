// The articulated adapter's episodes on the device: B three-link pendulums released from different heights, stepped in launches of 100 steps; after
// every launch the link poses are written to device memory, a kernel of the example marks the copies whose last link has fallen below a height,
// and those copies alone start a new episode from their start state -- poses, mask and reset never leave the device; only the printout does.
//   hipcc --offload-arch=gfx950 -std=c++17 example_artic_reset.cpp -L.. -lmoby_hip -Wl,-rpath,.. -o example_artic_reset
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>
#include <hip/hip_runtime.h>
#include "MobyHipArticulatedBody.h"

// done[w] = 1 when the origin of link `link` of copy w lies below z_min (poses: B x nj x 12, row-major R then the origin)
__global__ void k_fell(int B, int nj, int link, const double* poses, double z_min, int* done)
{
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < B) done[w] = poses[((size_t)w * nj + link) * 12 + 11] < z_min ? 1 : 0;
}

int main()
{
  // three rods of 0.5 m hanging along -z, hinged about y, limits at +-3 rad
  mh_artic_model m; std::memset(&m, 0, sizeof(m));
  m.nj = 3; m.gravity[2] = -9.81; m.cstab_eps = 1.4901161193847656e-08;
  for (int i = 0; i < 3; i++) {
    m.parent[i] = i - 1; m.jtype[i] = MH_JOINT_REVOLUTE; m.axis[i][1] = 1.0; m.mass[i] = 1.0; m.com[i][2] = -0.25;
    if (i > 0) m.trel[i][2] = -0.5;
    m.lolimit[i] = -3.0; m.hilimit[i] = 3.0;
    for (int k = 0; k < 3; k++) { m.Rrel[i][4 * k] = 1.0; m.inertia[i][4 * k] = 0.02; }
  }
  const int B = 4, nj = 3, n = 100, launches = 6;
  const double z_min = -0.6;                                                            // the last hinge hangs at z = -1 at rest
  std::vector<double> q((size_t)B * nj, 0.0), qd((size_t)B * nj, 0.0);
  for (int w = 0; w < B; w++) q[(size_t)w * nj] = 1.5 - 0.15 * w;                       // released at 1.5, 1.35, 1.2, 1.05 rad from the vertical
  MobyHip::BatchedArticulatedBody* r = NULL;
  double *q0_dev = NULL, *qd0_dev = NULL, *poses_dev = NULL, *time_dev = NULL; int *done_dev = NULL, *status_dev = NULL;
  auto cleanup = [&]() { void* ps[] = { q0_dev, qd0_dev, poses_dev, time_dev, done_dev, status_dev }; for (void* p : ps) if (p) (void)hipFree(p); delete r; };
  try {
    r = new MobyHip::BatchedArticulatedBody(m, B, q.data(), qd.data());
    const size_t sb = (size_t)B * nj * sizeof(double);
    if (hipMalloc((void**)&q0_dev, sb) != hipSuccess || hipMalloc((void**)&qd0_dev, sb) != hipSuccess || hipMalloc((void**)&poses_dev, 12 * sb) != hipSuccess
        || hipMalloc((void**)&time_dev, B * sizeof(double)) != hipSuccess || hipMalloc((void**)&done_dev, B * sizeof(int)) != hipSuccess
        || hipMalloc((void**)&status_dev, B * sizeof(int)) != hipSuccess) throw std::runtime_error("hipMalloc failed");
    if (hipMemcpy(q0_dev, q.data(), sb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(qd0_dev, qd.data(), sb, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
    int resets = 0; bool ok = true;
    for (int l = 0; l < launches; l++) {
      r->step(1e-3, n);
      r->link_poses_dev(poses_dev);                                                     // all on the null stream, in order, no synchronisation
      hipLaunchKernelGGL(k_fell, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)NULL, B, nj, 2, (const double*)poses_dev, z_min, done_dev);
      if (hipGetLastError() != hipSuccess) throw std::runtime_error("the example's kernel did not launch");
      r->reset_dev(done_dev, q0_dev, qd0_dev);
      r->status_dev(status_dev, time_dev);
      int done[B], status[B]; double t[B]; std::vector<double> poses((size_t)B * nj * 12);                       // the printout: this is the only host copy
      if (hipMemcpy(done, done_dev, sizeof(done), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(status, status_dev, sizeof(status), hipMemcpyDeviceToHost) != hipSuccess
          || hipMemcpy(t, time_dev, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(poses.data(), poses_dev, 12 * sb, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("hipMemcpy failed");
      for (int w = 0; w < B; w++) {
        std::printf("launch %d copy %d: last hinge at z = %+.4f, %s, status %d, time %.3f\n", l, w, poses[((size_t)w * nj + 2) * 12 + 11], done[w] ? "reset" : "goes on", status[w], t[w]);
        resets += done[w];
        ok = ok && status[w] == 0 && (done[w] ? t[w] == 0.0 : t[w] > 0.0);               // a reset copy's clock restarts, the others' runs on
      }
    }
    std::printf("%d resets in %d launches\n", resets, launches);
    ok = ok && resets > 0 && resets < B * launches;
    cleanup();
    return ok ? 0 : 1;
  } catch (const std::exception& e) { std::printf("error: %s\n", e.what()); cleanup(); return 1; }
}
