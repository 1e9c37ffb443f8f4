// mh_artic_reset.hip -- episodes on the device (include/moby_hip_artic.h, "Episodes on the device"): the kernels of mh_artic_batch_reset_dev and
// mh_artic_batch_status_dev, a code object of its own that knows nothing of the model -- it walks q, qd, the base poses and the aux records as
// arrays, so every kernel of the fifteen older articulated code objects keeps its code.  The entry points are in mh_artic.hip.
#include "mh_host.h"
#include "../../include/moby_hip_artic.h"
#include <cstddef>
#include <cstring>

namespace mh { namespace artic {

// a record as the 8-byte words the reset writes: the rand() stream in front, everything after it zero in a fresh record (mh_world_aux_init)
constexpr int AUX_WORDS = (int)(sizeof(mh_world_aux) / 8);
constexpr int RNG_WORDS = (int)(sizeof(((mh_world_aux*)nullptr)->rng) / 8);
static_assert(sizeof(mh_world_aux) % 8 == 0 && alignof(mh_world_aux) == 8 && offsetof(mh_world_aux, rng) == 0 && sizeof(((mh_world_aux*)nullptr)->rng) % 8 == 0,
              "an aux record is walked as 8-byte words, the rand() stream first");
static_assert(RNG_WORDS <= 64, "one pass of the wave covers the rand() stream");
static_assert(MH_ARTIC_MAX_JOINTS <= 64, "lanes j < nj copy a world's rows of q / qd: one lane per joint");
struct FreshRng { unsigned long long w[RNG_WORDS]; };              // rand() at srand(1), by value in the kernel arguments

// One wavefront per world.  mask NULL: every world; otherwise world b is reset iff mask[b] != 0, read once as a wave-uniform value -- a world that
// is not reset writes nothing.  Lanes j < nj copy the world's rows of q_src / qd_src (a NULL source leaves the array), lanes 0..6 its row of
// pose_src with the quaternion divided by n = sqrt(((w w + x x) + y y) + z z) -- the arithmetic of mh_artic_batch_set_base_pose, no contraction
// (-ffp-contract=off) -- and the wave writes the fresh aux record as 8-byte words, consecutive lanes to consecutive words.  Rows of worlds that
// are not reset are never read.  Every index lies inside world b's own rows: b < B, j < nj, k < 7, word < AUX_WORDS.
__global__ __launch_bounds__(64)
void k_artic_reset(int B, int nj, const int* __restrict__ mask, const double* __restrict__ q_src, const double* __restrict__ qd_src,
                   const double* __restrict__ pose_src, double* __restrict__ qg, double* __restrict__ qdg, double* __restrict__ poseg,
                   unsigned long long* __restrict__ auxg, FreshRng rng)
{
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  if (mask && __builtin_amdgcn_readfirstlane(mask[b]) == 0) return;
  if (lane < nj) {
    const size_t e = (size_t)b * nj + lane;
    if (q_src) qg[e] = q_src[e];
    if (qd_src) qdg[e] = qd_src[e];
  }
  if (pose_src && poseg && lane < 7) {
    const double* P = pose_src + 7 * (size_t)b;
    double v = P[lane];
    if (lane >= 3) {
      const double w = P[3], x = P[4], y = P[5], z = P[6];
      const double n = sqrt(((w * w + x * x) + y * y) + z * z);
      v = v / n;
    }
    poseg[7 * (size_t)b + lane] = v;
  }
  unsigned long long* a = auxg + (size_t)b * AUX_WORDS;
  unsigned long long head = 0ull;                                  // this lane's word of the rand() stream (a select chain: no indexed copy of the arguments)
#pragma unroll
  for (int i = 0; i < RNG_WORDS; i++) head = (lane == i) ? rng.w[i] : head;
  a[lane] = head;                                                  // words 0..63: AUX_WORDS > 64 (asserted below)
  for (int k = 64 + lane; k < AUX_WORDS; k += 64) a[k] = 0ull;
}
static_assert(AUX_WORDS > 64, "the first pass of k_artic_reset writes words 0..63 without a bound");

// one thread per world: status and time out of the strided records
__global__ __launch_bounds__(64)
void k_artic_status(int B, const mh_world_aux* __restrict__ auxg, int* __restrict__ status_dst, double* __restrict__ time_dst)
{
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (status_dst) status_dst[b] = auxg[b].status;
  if (time_dst) time_dst[b] = auxg[b].time;
}

}} // namespace mh::artic

hipError_t artic_reset_launch(void* stream, int B, int nj, const int* mask, const double* q_src, const double* qd_src, const double* pose_src,
                              double* q, double* qd, double* pose, mh_world_aux* aux)
{
  namespace ar = mh::artic;
  static const ar::FreshRng fresh = [] {                             // what mh_artic_batch_create gives every world: mh_world_aux_init(&a, 1)
    mh_world_aux a; mh_world_aux_init(&a, 1);
    ar::FreshRng r; std::memcpy(r.w, a.rng, sizeof(r.w));
    return r;
  }();
  hipLaunchKernelGGL(ar::k_artic_reset, dim3(B), dim3(64), 0, (hipStream_t)stream, B, nj, mask, q_src, qd_src, pose_src, q, qd, pose,
                     reinterpret_cast<unsigned long long*>(aux), fresh);
  return hipGetLastError();
}

hipError_t artic_status_launch(void* stream, int B, const mh_world_aux* aux, int* status_dst, double* time_dst)
{
  hipLaunchKernelGGL(mh::artic::k_artic_status, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, B, aux, status_dst, time_dst);
  return hipGetLastError();
}
