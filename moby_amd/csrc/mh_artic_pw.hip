// mh_artic_pw.hip -- the articulated step with per-world model parameters (include/moby_hip_artic.h, "Per-world parameters").
//
// The report kernels of mh_artic_rp.hip with MH_ARTIC_PARAMS_TU, under which a kernel reads world b's own image Mg[b] of the B the batch holds where
// the others read the one shared *Mg -- one wavefront steps one world, so the image is still wave-uniform.  That is the whole difference on the
// device: the image of world w is filled on the host by the code that fills the shared one, applied to the model with record w written into it
// (mh_artic.hip: artic_check_model), so world w steps exactly as a batch of that model would.  Every line of it sits under the switch, and this is
// a code object of its own, so that the eleven older articulated code objects keep their code.  Here the plain and the stabilising step in angle
// coordinates, each undriven and driven (k_artic_step_pw...), with the rows or NULL as the report kernels take them, their launcher
// artic_pw_launch and image size artic_pw_lds_bytes; the per-world forms of the forward dynamics / link poses and Jacobian kernels
// (k_artic_fwd_dyn_pw, k_artic_jacobian_pw); and the scatter of mh_artic_batch_set_params_dev.  Pose forms: mh_artic_pw_pose.hip.  The router
// (mh_artic.hip: artic_geom_step) sends every batch of mh_artic_batch_create_params here, whatever its geometry -- none at all included -- and
// every batch that would take the report kernels created under mh_debug_set(20, 1).
#define MH_ARTIC_BOX_TU 1
#define MH_ARTIC_PAIR_TU 1
#define MH_ARTIC_BSP_TU 1
#define MH_ARTIC_REPORT_TU 1
#define MH_ARTIC_PARAMS_TU 1
#define MH_ARTIC_GEOM pw
#include "mh_artic_dev.h"

namespace mh { namespace artic {

// where a record's fields live in a world's image, in doubles: the image is not laid out as the record is (the model's integers lie between its
// doubles, and the box block is valid in Model::bx only: anc / fcos / fsin overlay it in Model::m)
struct ParamSeg { int src, dst, n; };
#define MH_PW_SEG(field, where) { (int)(offsetof(mh_artic_params, field) / 8), (int)((where) / 8), (int)(sizeof(mh_artic_params::field) / 8) }
#define MH_PW_M(field) MH_PW_SEG(field, offsetof(Model, m) + offsetof(mh_artic_model, field))
__constant__ ParamSeg c_param_segs[] = {
  MH_PW_M(Rrel), MH_PW_M(trel), MH_PW_M(axis), MH_PW_M(com), MH_PW_M(inertia), MH_PW_M(mass), MH_PW_M(lolimit), MH_PW_M(hilimit),
  MH_PW_M(limit_restitution), MH_PW_M(gravity), MH_PW_M(sphere_center), MH_PW_M(sphere_radius), MH_PW_M(plane_R), MH_PW_M(plane_o),
  MH_PW_M(cp_epsilon), MH_PW_M(cp_mu_coulomb), MH_PW_M(cp_mu_viscous), MH_PW_M(cp_compliance),
  MH_PW_SEG(box_center, offsetof(Model, bx) + offsetof(Boxes, center)), MH_PW_SEG(box_R, offsetof(Model, bx) + offsetof(Boxes, R)),
  MH_PW_SEG(box_len, offsetof(Model, bx) + offsetof(Boxes, len)),
};
constexpr int N_PARAM_SEGS = 21;                                   // every field of mh_artic_params, once
static_assert(sizeof(c_param_segs) == N_PARAM_SEGS * sizeof(ParamSeg), "one segment per field of the record");
static_assert(sizeof(mh_artic_params) % 8 == 0 && sizeof(Model) % 8 == 0 && offsetof(Model, bx) % 8 == 0 && offsetof(Boxes, center) % 8 == 0, "records and images are walked as doubles");

// one workgroup per record: record r of `count` into image first + r.  Plain vector loads and stores of doubles; the segment table is the only
// source of offsets, and every one of them lies inside one record and one image
__global__ __launch_bounds__(64)
void k_artic_params_scatter(Model* __restrict__ Mg, const mh_artic_params* __restrict__ rec, int first, int count)
{
  const int r = blockIdx.x;
  if (r >= count) return;
  const double* src = reinterpret_cast<const double*>(rec + r);
  double* dst = reinterpret_cast<double*>(Mg + (size_t)first + r);
  for (int s = 0; s < N_PARAM_SEGS; s++) {
    const ParamSeg g = c_param_segs[s];
    for (int k = threadIdx.x; k < g.n; k += 64) dst[g.dst + k] = src[g.src + k];
  }
}

}} // namespace mh::artic

hipError_t artic_pw_scatter_launch(mh_artic_batch* ab, void* stream, const mh_artic_params* dev, int first, int count)
{
  hipLaunchKernelGGL(mh::artic::k_artic_params_scatter, dim3(count), dim3(64), 0, (hipStream_t)stream, ab->d_model, dev, first, count);
  return hipGetLastError();
}
