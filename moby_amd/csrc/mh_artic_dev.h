// mh_artic_dev.h -- many-worlds stepper for fixed-base articulated bodies (include/moby_hip_artic.h; BASELINE config 5): the device code and
// the host declarations every articulated translation unit shares.
//
// Each of the fifteen articulated .hip files sets its switches (MH_ARTIC_DRIVE_TU, MH_ARTIC_POSE_TU, MH_ARTIC_BOX_TU, MH_ARTIC_PAIR_TU,
// MH_ARTIC_BSP_TU, MH_ARTIC_REPORT_TU, MH_ARTIC_PARAMS_TU, MH_ARTIC_WRENCH_TU; a geometry file also its family token MH_ARTIC_GEOM) and includes this header once: the switches pick the
// kernels of that code object.  mh_artic.hip (no switch) holds the C entry points and the router to the geometry kernels, mh_artic_drive.hip and
// mh_artic_pose.hip their own entry points; a geometry file (mh_artic_{box,pair,bsp,rp,pw,wr}[_pose].hip) holds nothing else (mh_artic_pw.hip: the record scatter): its launcher is stamped at
// the end of this header.
//
// One wavefront per world. Per step (TimeSteppingSimulator::do_mini_step with no collision geometry, TSS:114-222):
//   q += dt qd (old velocity)  ->  link frames (chain walk, 12 lanes per link), motion subspaces and spatial inertias
//   about the world origin (lane = link)  ->  bias C(q, qd) by recursive Newton-Euler (6 lanes per link, gravity as a
//   base acceleration)  ->  composite inertias (36 lanes) and H = S' Ic S (lane = matrix entry)  ->  Cholesky
//   (lane = row) and  qdd = H^-1 (tau - C)  ->  qd += dt qdd  ->  joint limits (ballot masks -> the reference's
//   constraint order, ArticulatedBody.inl:9-43)  ->  X = H^-1 (lane = column), the limit LCP  L X L' l + L v >= 0  through
//   the wave solver of mh_lcp_wave.h (lcp_fast on the persistent _v, then the Lemke ladder: ICH:1239-1283)  ->  impulses,
//   restitution (ICH:298-525).
// H, its factor, H^-1, the LCP and all link quantities live in LDS (dynamic, sized by the joint count; the link quantities
// and the limit LCP share one region: 10 KB at 10 joints => 16 worlds per CU); HBM sees q, qd and the aux record once per launch.
// The dynamics algorithm is Featherstone's (Ravelin's source is not in the reference tree: SURVEY F2); operation
// order = oracle/artic.hpp, checked bit for bit.  sin / cos: the same explicit kernel as the oracle (no libm call).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <cstddef>
#include <vector>
#include <mutex>
#include "../../include/moby_hip_artic.h"
#include "mh_host.h"
#include "mh_lcp_wave.h"

namespace mh { namespace artic {

constexpr int NJ = MH_ARTIC_MAX_JOINTS;
constexpr int NLMAX = MH_NOSLIP_MAX;
constexpr double NEAR_ZERO_ = 1.4901161193847656e-08;

struct Boxes {            // mh_artic_model's box block (mh_artic_batch_create copies it here)
  int n;
  int link[MH_ARTIC_MAX_BOXES];
  double center[MH_ARTIC_MAX_BOXES][3], R[MH_ARTIC_MAX_BOXES][9], len[MH_ARTIC_MAX_BOXES][3];
};
struct Pairs {            // mh_artic_model's pair block (mh_artic_batch_create copies it here)
  int n;
  int a[MH_ARTIC_MAX_PAIRS], b[MH_ARTIC_MAX_PAIRS];
  int no_plane;           // mh_artic_model.sphere_no_plane
  int kind[MH_ARTIC_MAX_PAIRS];   // mh_artic_model.pair_kind (behind what the pair kernels read: only the box-sphere kernels of mh_artic_bsp.hip look at it)
  int nstatic;            // boxes with link -1
};
struct Model {            // mh_artic_model + what the kernel wants precomputed: ancestor masks
  // anc, fcos and fsin sit where they sat before the box block was appended to mh_artic_model -- over that block, which is therefore NOT valid
  // in m on the device (read bx) -- so that every kernel written before boxes existed keeps its code byte for byte.  The pair block at the end
  // of m is valid there, but the kernels read the copy in pr, beside bx
  union {
    mh_artic_model m;
    struct {
      unsigned char head_[offsetof(mh_artic_model, nboxes)];
      unsigned anc[NJ];       // bit j: joint j lies on the path from joint i to the base (i itself included)
      double fcos[32], fsin[32];   // friction polygon of the Drumwright-Shell model: cos / sin(j / (nk/2 - 1) pi/2) by the HOST's libm (ICH-QP:462-470)
    };
  };
  Boxes bx;
  Pairs pr;
};

__constant__ Pow10Table c_pow10a;

MH_DEV void sincos_kernel(double x, double& s, double& c)
{
  const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00, pio2_1t = 6.07710050650619224932e-11;
  const double kf = floor(x * invpio2 + 0.5);
  const double r = (x - kf * pio2_1) - kf * pio2_1t;
  const double z = r * r;
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double v = z * r;
  const double rs = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
  const double ks = r + v * (S1 + z * rs);
  const double rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
  const double kc = 1.0 - (0.5 * z - z * rc);
  const long long k = (long long)kf;
  const int n = (int)(((k % 4) + 4) % 4);
  if (n == 0) { s = ks; c = kc; } else if (n == 1) { s = kc; c = -ks; } else if (n == 2) { s = -ks; c = -kc; } else { s = -kc; c = ks; }
}

MH_DEV double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
MH_DEV void cross3(const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
MH_DEV void mat3mul(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) C[3*i+j] = (A[3*i] * B[j] + A[3*i+1] * B[3+j]) + A[3*i+2] * B[6+j];
}
MH_DEV void mat3vec(const double* A, const double* v, double* y) { for (int i = 0; i < 3; i++) y[i] = (A[3*i] * v[0] + A[3*i+1] * v[1]) + A[3*i+2] * v[2]; }
MH_DEV double dot6(const double* a, const double* b) { double acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + a[k] * b[k]; return acc; }
// component k of the spatial cross products ([angular; linear]), operands in LDS
MH_DEV double cross_c(const double* a, const double* b, int k) { const int k1 = (k + 1) % 3, k2 = (k + 2) % 3; return a[k1] * b[k2] - a[k2] * b[k1]; }
MH_DEV double crm_c(const double* v, const double* m, int k) { return (k < 3) ? cross_c(v, m, k) : cross_c(v, m + 3, k - 3) + cross_c(v + 3, m, k - 3); }
MH_DEV double crf_c(const double* v, const double* f, int k) { return (k < 3) ? cross_c(v, f, k) + cross_c(v + 3, f + 3, k) : cross_c(v, f + 3, k - 3); }

// the LDS image of one world (doubles), nj = number of joints
struct Lay {
  int nj;
  int q, qd, qdd, C, R, x, Rl, tl, S, I6, v, a, f, F, Iv, H, L, X, MM, A, art, Lv, l, idx, total;
#ifdef MH_ARTIC_POSE_TU
  int pR, pp, pQ;       // pose coordinates (mh_artic_pose.hip): the base pose R(Q) (9), p (3), Q (4), alive for the whole launch, behind everything else
#endif
  // q, qd, qdd, C and H, L, X live for the whole step; the link quantities of dynamics() (R .. Iv) and the limit LCP's
  // storage (MM .. idx) are never alive together -- handle_limits reads q, qd, L, X only and the next dynamics() call
  // rebuilds everything from q, qd -- so they share one region: 10 KB per world at 10 joints = 16 worlds per CU
  MH_DEV Lay(int n, int nlcap = NLMAX) : nj(n) {     // nlcap: rows the limit LCP's storage takes (NLSTAB in the stabilising kernel)
    int o = 0;
    q = o; o += n; qd = o; o += n; qdd = o; o += n; C = o; o += n;
    H = o; o += n * n; L = o; o += n * n; X = o; o += n * n;
    const int u = o;
    R = o; o += 9 * n; x = o; o += 3 * n;
    S = o; o += 6 * n; I6 = o; o += 36 * n; v = o; o += 6 * n; a = o; o += 6 * n; f = o; o += 6 * n; F = o; o += 6 * n; Iv = o; o += 12;
    // the local transforms live only from kin_inertia's first loop to the end of its chain walk, before anything writes v or a (RNEA / the articulated-body
    // recursion come after): they share those 12 n doubles (round 5: 1252 -> 1132 doubles at 10 joints = 18 images per CU instead of 16)
    Rl = v; tl = v + 9 * n;
    const int end_dyn = o;
    o = u;
    MM = o; o += nlcap * nlcap; A = o; o += nlcap * nlcap; art = o; o += nlcap; Lv = o; o += nlcap; l = o; o += nlcap;
    idx = o; o += nlcap;           // ints stored as doubles' slots (one int each, low half)
    total = (o > end_dyn) ? o : end_dyn;
#ifdef MH_ARTIC_POSE_TU
    pR = total; pp = pR + 9; pQ = pp + 3; total += 16;
#endif
  }
};
constexpr int NLSTAB = 2 * NJ;      // the stabiliser's LCP has a row for every finite limit (CStab:257-304): up to two per joint
static size_t lds_bytes(int nj, int nlcap = NLMAX) {
  const int n = nj;
  const int dyn = 78 * n + 12, lim = 2 * nlcap * nlcap + 4 * nlcap;
#ifdef MH_ARTIC_POSE_TU
  return sizeof(double) * (size_t)(4 * n + 3 * n * n + (dyn > lim ? dyn : lim) + 16);     // + Lay's pose slots
#else
  return sizeof(double) * (size_t)(4 * n + 3 * n * n + (dyn > lim ? dyn : lim));
#endif
}

// pose coordinates (MH_ARTIC_POSE_TU): the floating base's pose in LDS stands in for the model's trel[0] (the sliders' origin, the base COM) and
// Rrel[3] (the first hinge's frame) -- exactly where the reference's per-world model copy puts them
#ifdef MH_ARTIC_POSE_TU
#define MH_RREL(i) (((i) == 3) ? (const double*)(g + Y.pR) : (const double*)m.Rrel[i])
#define MH_TREL(i) (((i) == 0) ? (const double*)(g + Y.pp) : (const double*)m.trel[i])
#else
#define MH_RREL(i) m.Rrel[i]
#define MH_TREL(i) m.trel[i]
#endif

// link frames, motion subspaces and spatial inertias about the world origin for the q in LDS (oracle Artic::kinematics)
// PACK worlds per wavefront: PACK = 1 -- the whole wave works on the image at g; PACK = 2 -- lanes 0-31 and 32-63 each work on THEIR
// world's image (g is then a per-lane pointer, `lane` the lane's index within its half): the same instruction stream steps two worlds
template <int PACK = 1>
MH_DEV void kin_inertia(const Model& M, const Lay& Y, double* g)
{
  const mh_artic_model& m = M.m;
  const int nj = Y.nj, lane = (PACK == 1) ? lane_id() : (lane_id() & (64 / PACK - 1));
  // local transforms: lane = link
  if (lane < nj) {
    const int i = lane;
    const double* ax = m.axis[i];
    double Rl[9], tl[3];
    const double qi = g[Y.q + i];
    if (m.jtype[i] == MH_JOINT_REVOLUTE) {
      double s, c; sincos_kernel(qi, s, c);
      const double t = 1.0 - c;
      const double K[9] = { 0.0, -ax[2], ax[1], ax[2], 0.0, -ax[0], -ax[1], ax[0], 0.0 };
      double Rq[9];
      for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Rq[3*a+b] = (((a == b) ? c : 0.0) + (t * ax[a]) * ax[b]) + s * K[3*a+b];
      mat3mul(MH_RREL(i), Rq, Rl);
      for (int k = 0; k < 3; k++) tl[k] = MH_TREL(i)[k];
    } else {
      for (int k = 0; k < 9; k++) Rl[k] = MH_RREL(i)[k];
      double d[3], Rd[3];
      for (int k = 0; k < 3; k++) d[k] = ax[k] * qi;
      mat3vec(MH_RREL(i), d, Rd);
      for (int k = 0; k < 3; k++) tl[k] = MH_TREL(i)[k] + Rd[k];
    }
    for (int k = 0; k < 9; k++) g[Y.Rl + 9 * i + k] = Rl[k];
    for (int k = 0; k < 3; k++) g[Y.tl + 3 * i + k] = tl[k];
  }
  wave_sync();
  // chain walk: lanes 0..8 = entries of R_i, lanes 9..11 = x_i
  for (int i = 0; i < nj; i++) {
    const int p = m.parent[i];
    if (lane < 9) {
      const int a = lane / 3, b = lane - 3 * a;
      double e;
      if (p < 0) e = g[Y.Rl + 9 * i + lane];
      else { const double* Rp = g + Y.R + 9 * p; const double* Rl = g + Y.Rl + 9 * i; e = (Rp[3*a] * Rl[b] + Rp[3*a+1] * Rl[3+b]) + Rp[3*a+2] * Rl[6+b]; }
      g[Y.R + 9 * i + lane] = e;
    } else if (lane < 12) {
      const int k = lane - 9;
      double e;
      if (p < 0) e = g[Y.tl + 3 * i + k];
      else { const double* Rp = g + Y.R + 9 * p; const double* tl = g + Y.tl + 3 * i; e = g[Y.x + 3 * p + k] + ((Rp[3*k] * tl[0] + Rp[3*k+1] * tl[1]) + Rp[3*k+2] * tl[2]); }
      g[Y.x + 3 * i + k] = e;
    }
    wave_sync();
  }
  // motion subspace and spatial inertia about the world origin: lane = link
  if (lane < nj) {
    const int i = lane;
    double R[9], x[3];
    for (int k = 0; k < 9; k++) R[k] = g[Y.R + 9 * i + k];
    for (int k = 0; k < 3; k++) x[k] = g[Y.x + 3 * i + k];
    double aw[3]; mat3vec(R, m.axis[i], aw);
    double* S = g + Y.S + 6 * i;
    if (m.jtype[i] == MH_JOINT_REVOLUTE) { double xa[3]; cross3(x, aw, xa); for (int k = 0; k < 3; k++) { S[k] = aw[k]; S[3+k] = xa[k]; } }
    else for (int k = 0; k < 3; k++) { S[k] = 0.0; S[3+k] = aw[k]; }
    double rc[3], r[3]; mat3vec(R, m.com[i], rc);
    for (int k = 0; k < 3; k++) r[k] = x[k] + rc[k];
    double T[9], Iw[9];
    mat3mul(R, m.inertia[i], T);
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) Iw[3*a+b] = (T[3*a] * R[3*b] + T[3*a+1] * R[3*b+1]) + T[3*a+2] * R[3*b+2];
    Iw[1] = Iw[3]; Iw[2] = Iw[6]; Iw[5] = Iw[7];
    const double mass = m.mass[i];
    const double rr = dot3(r, r);
    const double rx[9] = { 0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0 };
    double* I6 = g + Y.I6 + 36 * i;
    for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {
      I6[6*a+b] = Iw[3*a+b] + mass * (((a == b) ? rr : 0.0) - r[a] * r[b]);
      I6[6*a+3+b] = mass * rx[3*a+b];
      I6[6*(3+a)+b] = mass * rx[3*b+a];
      I6[6*(3+a)+3+b] = (a == b) ? mass : 0.0;
    }
  }
  wave_sync();
}

#ifdef MH_ARTIC_WRENCH_TU
// Link wrenches (moby_hip_artic.h, mh_artic_wrench; operation order = tests/native/artic_wrench_ref.cpp, bit for bit): called by the forward
// dynamics right after kin_inertia, when R, x, S of the mini-step's q are in LDS and nothing of the bias pass has been written.  Lane i < nj forms
// link i's velocity V_i (link_velocities' sum), its damping and the caller's wrench of schedule row s (world b of B) in registers and leaves
// F6_i = [T + c x F; F] in the bias forces' region `f`, which the bias pass rewrites afterwards; then lane j sums S_j . F6_i over the links outboard
// of joint j into the tau slot the drive writes (the qdd slot, see drive_tau), on top of the drive's tau_w[j] when there is one.  No LDS of its own;
// gains and schedule rows come from global memory at every mini-step, as the drive's.  Returns the tau the dynamics reads.
MH_DEV const double* link_wrench(const Model& M, const Lay& Y, double* g, const double* tau_w, const mh_artic_wrench& W, int B, int b, int s)
{
  const mh_artic_model& m = M.m;
  const int nj = Y.nj, lane = lane_id();
  if (lane < nj) {
    const int i = lane;
    double R[9], c[3], rc[3], F[3], T[3];
    for (int k = 0; k < 9; k++) R[k] = g[Y.R + 9 * i + k];
    mat3vec(R, m.com[i], rc);
    for (int k = 0; k < 3; k++) c[k] = g[Y.x + 3 * i + k] + rc[k];
    const bool damp = (W.terms & MH_LINK_DAMPING) != 0;
    if (damp) {
      const size_t o = (size_t)b * nj + i;
      double V[6];
      for (int k = 0; k < 6; k++) {
        double acc = 0.0; bool first = true;
        for (int j = 0; j <= i; j++) if ((M.anc[i] >> j) & 1u) { const double vj = g[Y.S + 6 * j + k] * g[Y.qd + j]; acc = first ? vj : acc + vj; first = false; }
        V[k] = acc;
      }
      double wxc[3], vc[3], vi[3], wi[3], fb[3], tb[3];
      cross3(V, c, wxc);
      for (int k = 0; k < 3; k++) vc[k] = V[3 + k] + wxc[k];
      for (int k = 0; k < 3; k++) { vi[k] = (R[k] * vc[0] + R[3 + k] * vc[1]) + R[6 + k] * vc[2]; wi[k] = (R[k] * V[0] + R[3 + k] * V[1]) + R[6 + k] * V[2]; }
      const double nv = sqrt((vi[0] * vi[0] + vi[1] * vi[1]) + vi[2] * vi[2]), nw = sqrt((wi[0] * wi[0] + wi[1] * wi[1]) + wi[2] * wi[2]);
      const double cl = -(W.kl[o] + nv * W.klsq[o]), ca = -(W.ka[o] + nw * W.kasq[o]);
      for (int k = 0; k < 3; k++) { fb[k] = vi[k] * cl; tb[k] = wi[k] * ca; }
      mat3vec(R, fb, F); mat3vec(R, tb, T);
    }
    if (W.terms & MH_LINK_WRENCH) {
      const double* e = W.w + (((size_t)(W.rows == 1 ? 0 : s) * (size_t)B + (size_t)b) * nj + i) * 6;
      double f[3] = { e[0], e[1], e[2] }, n[3] = { e[3], e[4], e[5] };
      if (W.terms & MH_LINK_WRENCH_LINK_AXES) { double t[3]; mat3vec(R, f, t); for (int k = 0; k < 3; k++) f[k] = t[k]; mat3vec(R, n, t); for (int k = 0; k < 3; k++) n[k] = t[k]; }
      for (int k = 0; k < 3; k++) { F[k] = damp ? F[k] + f[k] : f[k]; T[k] = damp ? T[k] + n[k] : n[k]; }
    }
    double cxF[3]; cross3(c, F, cxF);
    for (int k = 0; k < 3; k++) { g[Y.f + 6 * i + k] = T[k] + cxF[k]; g[Y.f + 6 * i + 3 + k] = F[k]; }
  }
  wave_sync();
  if (lane < nj) {
    const int j = lane;
    double acc = 0.0;
    for (int i = j; i < nj; i++) if ((M.anc[i] >> j) & 1u) acc = acc + dot6(g + Y.S + 6 * j, g + Y.f + 6 * i);   // (a link outboard of joint j has an index >= j)
    g[Y.qdd + j] = tau_w ? tau_w[j] + acc : acc;
  }
  wave_sync();
  return g + Y.qdd;
}
#endif

// kinematics + spatial inertias + bias + H + Cholesky + qdd for the q / qd in LDS.  Returns false if H is not PD.
// (MH_ARTIC_WRENCH_TU: Wp not NULL = the step's own call, with world wb of wB at schedule row ws: link_wrench adds to tau_w)
template <int PACK = 1>
MH_DEV bool dynamics(const Model& M, const Lay& Y, double* g, const double* tau_w
#ifdef MH_ARTIC_WRENCH_TU
                     , const mh_artic_wrench* Wp = nullptr, int wB = 0, int wb = 0, int ws = 0
#endif
                     )
{
  const mh_artic_model& m = M.m;
  constexpr int STR = 64 / PACK;
  const int nj = Y.nj, lane = (PACK == 1) ? lane_id() : (lane_id() & (STR - 1));
  kin_inertia<PACK>(M, Y, g);
#ifdef MH_ARTIC_WRENCH_TU
  static_assert(PACK == 1, "link_wrench works on one world per wavefront (whole-wave lanes and barriers): no packed form in a wrench code object");
  if (Wp) tau_w = link_wrench(M, Y, g, tau_w, *Wp, wB, wb, ws);
#endif
  // recursive Newton-Euler with qdd = 0 (the links' OWN inertias): lanes 0..5 = spatial components
  for (int i = 0; i < nj; i++) {
    const int p = m.parent[i];
    const double* S = g + Y.S + 6 * i;
    const double qdi = g[Y.qd + i];
    double* vj = g + Y.Iv;                        // S_i qd_i (6), then I v (6)
    if (lane < 6) { const double e = S[lane] * qdi; vj[lane] = e; g[Y.v + 6 * i + lane] = (p < 0) ? e : g[Y.v + 6 * p + lane] + e; }
    wave_sync();
    if (lane < 6) {
      const double cv = crm_c(g + Y.v + 6 * i, vj, lane);
      const double ap = (p < 0) ? ((lane < 3) ? 0.0 : -m.gravity[lane - 3]) : g[Y.a + 6 * p + lane];
      g[Y.a + 6 * i + lane] = ap + cv;
    }
    wave_sync();
    double Ia = 0.0;
    if (lane < 6) {
      const double* I6 = g + Y.I6 + 36 * i + 6 * lane;
      const double* a = g + Y.a + 6 * i; const double* v = g + Y.v + 6 * i;
      double acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + I6[k] * a[k];
      Ia = acc;
      acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + I6[k] * v[k];
      g[Y.Iv + 6 + lane] = acc;
    }
    wave_sync();
    if (lane < 6) g[Y.f + 6 * i + lane] = Ia + crf_c(g + Y.v + 6 * i, g + Y.Iv + 6, lane);
    wave_sync();
  }
  for (int i = nj - 1; i >= 0; i--) {
    const int p = m.parent[i];
    if (lane == 6) g[Y.C + i] = dot6(g + Y.S + 6 * i, g + Y.f + 6 * i);
    if (p >= 0 && lane < 6) g[Y.f + 6 * p + lane] = g[Y.f + 6 * p + lane] + g[Y.f + 6 * i + lane];
    wave_sync();
  }
  // composite inertias, in place: lanes 0..35 = entries
  for (int i = nj - 1; i >= 0; i--) {
    const int p = m.parent[i];
    if (p >= 0) for (int e = lane; e < 36; e += STR) g[Y.I6 + 36 * p + e] = g[Y.I6 + 36 * p + e] + g[Y.I6 + 36 * i + e];
    wave_sync();
  }
  // F_i = Ic_i S_i: lanes (i, r)
  for (int e = lane; e < 6 * nj; e += STR) {
    const int i = e / 6, r = e - 6 * i;
    const double* I6 = g + Y.I6 + 36 * i + 6 * r; const double* S = g + Y.S + 6 * i;
    double acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + I6[k] * S[k];
    g[Y.F + e] = acc;
  }
  wave_sync();
  // H(i, j) = S_j' F_i for j on i's path to the base (and its mirror); 0 elsewhere: lanes = entries
  for (int e = lane; e < nj * nj; e += STR) {
    const int i = e / nj, j = e - nj * i;
    double h = 0.0;
    if ((M.anc[i] >> j) & 1u) h = dot6(g + Y.S + 6 * j, g + Y.F + 6 * i);
    else if ((M.anc[j] >> i) & 1u) h = dot6(g + Y.S + 6 * i, g + Y.F + 6 * j);
    g[Y.H + e] = h;
  }
  wave_sync();
  // dpotf2('L') on a copy: lane = row
  for (int e = lane; e < nj * nj; e += STR) g[Y.L + e] = g[Y.H + e];
  wave_sync();
  double* L = g + Y.L;                             // symmetric: row-major == column-major; L(i, k) at L[i + nj k]
  bool pd = true;
  for (int j = 0; j < nj; j++) {
    if (lane == j) {
      double ajj = L[j + nj * j];
      for (int k = 0; k < j; k++) ajj = ajj - L[j + nj * k] * L[j + nj * k];
      g[Y.Iv] = ajj;
    }
    wave_sync();
    const double ajj0 = g[Y.Iv];
    if (!(ajj0 > 0.0)) { pd = false; if (PACK == 1) break; }      // (packed: the other world of the wave goes on; this one computes on, its result is dropped)
    const double ajj = sqrt(ajj0);
    if (lane == j) L[j + nj * j] = ajj;
    if (lane > j && lane < nj) {
      double s = L[lane + nj * j];
      for (int k = 0; k < j; k++) s = s - L[lane + nj * k] * L[j + nj * k];
      L[lane + nj * j] = s / ajj;
    }
    wave_sync();
  }
  if (PACK == 1 && !pd) return false;
  // dpotrs: lane = row for the column sweeps
  double* b = g + Y.qdd;
  if (lane < nj) b[lane] = (tau_w ? tau_w[lane] : 0.0) - g[Y.C + lane];
  wave_sync();
  for (int k = 0; k < nj; k++) {
    if (lane == k) b[k] = b[k] / L[k + nj * k];
    wave_sync();
    const double bk = b[k];
    if (lane > k && lane < nj) b[lane] = b[lane] - bk * L[lane + nj * k];
    wave_sync();
  }
  for (int k = nj - 1; k >= 0; k--) {
    if (lane == k) { double s = b[k]; for (int i = k + 1; i < nj; i++) s = s - L[i + nj * k] * b[i]; b[k] = s / L[k + nj * k]; }
    wave_sync();
  }
  return pd;
}

// calc_fwd_dyn, eFeatherstone (RCArticulatedBody::algorithm_type): the articulated-body recursion, every spatial quantity at the
// world origin (oracle Artic::fwd_dyn_aba, same operation order).  In place: I6 becomes the articulated inertias, `a` holds the
// bias accelerations c_i and then the accelerations, `f` the bias forces, `F` the U_i; d_i and u_i sit in the (unused) H region.
// Returns false when some d_i = S' IA S is not positive.
MH_DEV bool dynamics_aba(const Model& M, const Lay& Y, double* g, const double* tau_w
#ifdef MH_ARTIC_WRENCH_TU
                         , const mh_artic_wrench* Wp = nullptr, int wB = 0, int wb = 0, int ws = 0
#endif
                         )
{
  const mh_artic_model& m = M.m;
  const int nj = Y.nj, lane = lane_id();
  kin_inertia(M, Y, g);
#ifdef MH_ARTIC_WRENCH_TU
  if (Wp) tau_w = link_wrench(M, Y, g, tau_w, *Wp, wB, wb, ws);
#endif
  double* dd = g + Y.H; double* uu = g + Y.H + nj;
  for (int i = 0; i < nj; i++) {                          // pass 1, outward
    const int p = m.parent[i];
    const double* S = g + Y.S + 6 * i;
    const double qdi = g[Y.qd + i];
    double* vj = g + Y.Iv;                                // S_i qd_i (6), then I v (6)
    if (lane < 6) { const double e = S[lane] * qdi; vj[lane] = e; g[Y.v + 6 * i + lane] = (p < 0) ? e : g[Y.v + 6 * p + lane] + e; }
    wave_sync();
    if (lane < 6) {
      g[Y.a + 6 * i + lane] = crm_c(g + Y.v + 6 * i, vj, lane);
      const double* I6 = g + Y.I6 + 36 * i + 6 * lane; const double* v = g + Y.v + 6 * i;
      double acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + I6[k] * v[k];
      g[Y.Iv + 6 + lane] = acc;
    }
    wave_sync();
    if (lane < 6) g[Y.f + 6 * i + lane] = crf_c(g + Y.v + 6 * i, g + Y.Iv + 6, lane);
    wave_sync();
  }
  bool pd = true;
  for (int i = nj - 1; i >= 0; i--) {                     // pass 2, inward
    const int p = m.parent[i];
    const double* S = g + Y.S + 6 * i;
    double* IA = g + Y.I6 + 36 * i;
    double* U = g + Y.F + 6 * i;
    if (lane < 6) { double acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + IA[6 * lane + k] * S[k]; U[lane] = acc; }
    wave_sync();
    if (lane == 0) { dd[i] = dot6(S, U); uu[i] = (tau_w ? tau_w[i] : 0.0) - dot6(S, g + Y.f + 6 * i); }
    wave_sync();
    const double d = dd[i], u = uu[i];
    if (!(d > 0.0)) { pd = false; break; }
    if (p >= 0) {
      if (lane < 36) { const int r = lane / 6, c = lane - 6 * r; double t = U[r] * U[c]; t = t / d; IA[lane] = IA[lane] - t; }   // Ia, in place
      wave_sync();
      if (lane < 36) g[Y.I6 + 36 * p + lane] = g[Y.I6 + 36 * p + lane] + IA[lane];
      else if (lane < 42) {
        const int r = lane - 36;
        const double* c = g + Y.a + 6 * i;
        double acc = 0.0; for (int k = 0; k < 6; k++) acc = acc + IA[6 * r + k] * c[k];
        double e = U[r] * u; e = e / d;
        const double pa = (g[Y.f + 6 * i + r] + acc) + e;
        g[Y.f + 6 * p + r] = g[Y.f + 6 * p + r] + pa;
      }
      wave_sync();
    }
  }
  if (!pd) return false;
  for (int i = 0; i < nj; i++) {                          // pass 3, outward
    const int p = m.parent[i];
    double* ap = g + Y.Iv;
    if (lane < 6) { const double base = (p < 0) ? ((lane < 3) ? 0.0 : -m.gravity[lane - 3]) : g[Y.a + 6 * p + lane]; ap[lane] = base + g[Y.a + 6 * i + lane]; }
    wave_sync();
    if (lane == 0) { const double t = uu[i] - dot6(g + Y.F + 6 * i, ap); g[Y.qdd + i] = t / dd[i]; }
    wave_sync();
    if (lane < 6) g[Y.a + 6 * i + lane] = ap[lane] + g[Y.S + 6 * i + lane] * g[Y.qdd + i];
    wave_sync();
  }
  return true;
}

// X = inverse_SPD(H) from the factor in Y.L (linalg.hpp inverse_spd): lane = column
MH_DEV void inverse_from_factor(const Lay& Y, double* g)
{
  const int nj = Y.nj, lane = lane_id();
  const double* L = g + Y.L;
  if (lane < nj) {
    double e[NJ];
    for (int i = 0; i < nj; i++) e[i] = (i == lane) ? 1.0 : 0.0;
    for (int k = 0; k < nj; k++) { e[k] = e[k] / L[k + nj * k]; const double bk = e[k]; for (int i = k + 1; i < nj; i++) e[i] = e[i] - bk * L[i + nj * k]; }
    for (int k = nj - 1; k >= 0; k--) { double s = e[k]; for (int i = k + 1; i < nj; i++) s = s - L[i + nj * k] * e[i]; e[k] = s / L[k + nj * k]; }
    for (int i = 0; i < nj; i++) g[Y.X + i + nj * lane] = e[i];          // column `lane`
  }
  wave_sync();
  // mirror the lower triangle into the upper one: A(c, i) = A(i, c), i > c
  for (int e2 = lane; e2 < nj * nj; e2 += 64) { const int r = e2 % nj, c = e2 / nj; if (r < c) g[Y.X + r + nj * c] = g[Y.X + c + nj * r]; }
  wave_sync();
}

// find_limit_constraints + the impact handler's no-slip path with NC = 0 (oracle Artic::handle_limits)
MH_DEV void handle_limits(const Model& M, const Lay& Y, double* g, mh_world_aux* aux, WaveRand& rng, int& status,
                          unsigned long long& solves, unsigned long long& rows, unsigned long long& pivs, unsigned long long& bytes)
{
  const mh_artic_model& m = M.m;
  const int nj = Y.nj, lane = lane_id();
  const double qi = (lane < nj) ? g[Y.q + lane] : 0.0;
  const bool up = lane < nj && qi >= m.hilimit[lane], lo = lane < nj && qi <= m.lolimit[lane];
  const uint64_t mu = ballot(up), ml = ballot(lo);
  const int nl = popc(mu) + popc(ml);
  if (nl == 0) return;
  const double qdi = (lane < nj) ? g[Y.qd + lane] : 0.0;
  const bool impacting = ballot((up && -qdi < -NEAR_ZERO_) || (lo && qdi < -NEAR_ZERO_)) != 0ull;   // CSim:313-323
  if (!impacting) return;
  if (nl > NLMAX) { status |= MH_WORLD_UNSUPPORTED; return; }
  // eFeatherstone bodies: the handler's X is still the inverse of the generalized inertia (get_generalized_inertia + inverse_SPD,
  // ICH:1600-1607): H and its factor by the CRB path, at the current q (before the limit storage below reuses the link arrays)
  if (m.algorithm == MH_ARTIC_FSAB) { wave_sync(); if (!dynamics(M, Y, g, nullptr)) { status |= MH_WORLD_LCP_FAILED; return; } }
  int* idx = reinterpret_cast<int*>(g + Y.idx);                  // idx[k] = joint | (upper << 8)
  if (lane < nj) {
    const int base = popc(mu & lanes_below(lane)) + popc(ml & lanes_below(lane));
    if (up) idx[base] = lane | 256;
    if (lo) idx[base + (up ? 1 : 0)] = lane;
  }
  wave_sync();
  inverse_from_factor(Y, g);                                     // compute_X (ICH:1607)
  const double* X = g + Y.X;
  // compute_limit_components (ICH:1755-1781): L_X_LT(a, b) = X(idx_a, idx_b) for b >= a, mirrored; L_v = +-qd
  double* MM = g + Y.MM;
  for (int e = lane; e < nl * nl; e += 64) {
    const int a = e % nl, b2 = e / nl;
    const int ia = idx[a] & 255, ib = idx[b2] & 255;
    MM[e] = (b2 >= a) ? X[ia * nj + ib] : X[ib * nj + ia];
  }
  const bool valid = lane < nl;
  const int my = valid ? idx[lane] : 0;
  const int myj = my & 255; const bool myup = (my & 256) != 0;
  double Lv = 0.0;
  if (valid) { Lv = g[Y.qd + myj]; if (myup) Lv = -Lv; }
  wave_sync();
  // lcp_fast on the persistent _v, then the Lemke ladder (ICH:1239, 1281)
  double nrm0 = 0.0;
  for (int e = lane; e < nl * nl; e += 64) { const double a = fabs(MM[e]); nrm0 = (a > nrm0) ? a : nrm0; }
  nrm0 = wave_max(nrm0);
  const double dii = valid ? MM[lane + nl * lane] : 0.0;
  int zsize = uni(aux->vns_size);
  double zi = (valid && zsize == nl) ? aux->vns[lane] : 0.0;
  DenseLds Md; Md.M = MM; Md.n = nl;
  LuScratch S; S.small = g + Y.A; S.ka = nl; S.big = g + Y.A;
  Trace tr; tr.buf = nullptr; tr.cap = 0; tr.len = 0;
  LcpParams P; P.kind = MH_LCP_FAST; P.min_exp = -20; P.step_exp = 1u; P.max_exp = 1; P.piv_tol = -1.0; P.zero_tol = -1.0;
  unsigned piv = 0, total = 0;
  bool ok = lcp_solve_wave(P, c_pow10a, nl, Md, S, g + Y.art, nrm0, dii, Lv, zi, zsize, rng, piv, tr);
  total += piv;
  if (!ok) {
    P.kind = MH_LCP_LEMKE_REG;
    ok = lcp_solve_wave(P, c_pow10a, nl, Md, S, g + Y.art, nrm0, dii, Lv, zi, zsize, rng, piv, tr);
    total += piv;
  }
  solves += 1ull; rows += (unsigned long long)nl; pivs += total; bytes += 8ull * ((unsigned long long)nl * nl + 2ull * nl);
  if (!ok) { status |= MH_WORLD_LCP_FAILED; return; }           // std::runtime_error("Unable to solve constraint LCP!")
  if (valid) aux->vns[lane] = zi;
  if (lane == 0) aux->vns_size = nl;
  double li = zi;
  double* lv = g + Y.Lv; double* ll = g + Y.l;
  auto apply = [&]() {                                           // update_from_stacked (ICH:298-397) + ICH:452
    if (valid) ll[lane] = li;
    wave_sync();
    if (lane < nj) {
      double dv = 0.0;
      for (int k = 0; k < nl; k++) { const int c = idx[k]; const double ls = (c & 256) ? -ll[k] : ll[k]; dv = dv + ls * X[(c & 255) * nj + lane]; }
      g[Y.qd + lane] = g[Y.qd + lane] + dv;
    }
    if (valid) { double t = 0.0; for (int k = 0; k < nl; k++) t = t + ll[k] * MM[lane + nl * k]; Lv = Lv + t; }
    wave_sync();
  };
  auto minv_of = [&]() -> double {                               // first-minimum over rows 0 .. nl-1, like the oracle's scan
    if (valid) lv[lane] = Lv;
    wave_sync();
    double mn = lv[0];
    for (int k = 1; k < nl; k++) mn = (lv[k] < mn) ? lv[k] : mn;
    wave_sync();
    return mn;
  };
  apply();
  const double minv = minv_of();
  if (valid) li = li * m.limit_restitution[myj];
  const bool changed = ballot(valid && li > NEAR_ZERO_) != 0ull;   // apply_restitution(q) (ICH:497-525)
  if (changed) {
    apply();
    const double minv_plus = minv_of();
    if (minv_plus < 0.0 && minv_plus < minv - NEAR_ZERO_) status |= MH_WORLD_UNSUPPORTED;   // ICH:284-291 reads an unsized _z
  }
  const double qd2 = valid ? g[Y.qd + myj] : 0.0;
  if (ballot(valid && ((myup ? -qd2 : qd2) < -NEAR_ZERO_)) != 0ull) status |= MH_WORLD_IMPACT_TOL;   // ICH:157-167
}

// ConstraintStabilization::stabilize for this body, joint-limit rows (oracle Artic::stabilize; CStab:167-254, 257-304, 434-441, 932-970,
// 1056-1216, 1322-1379).  evaluate_unilateral_constraints reads joints[i] with i the BODY's index (CStab:117) -- joint 0 here, once per
// joint: every entry of uC is one of joint 0's two slacks, so the line search of update_q is wave-uniform scalar code on
// (q0, dq0); the LCP has a row for every finite limit of every joint and needs H^-1 at the current configuration.
struct StabSlack { double hi0, lo0;
  MH_DEV double at(double q0, unsigned i) const { return (i & 1u) ? (q0 + 0.0) - lo0 : (hi0 - q0) - 0.0; }     // hilimit - q - tare / q + tare - lolimit, tare = 0
  MH_DEV double vio(double q0) const { const double a = (hi0 - q0) - 0.0, b = (q0 + 0.0) - lo0; return (b < a) ? b : a; } };
MH_DEV double stab_sign2(double x, double y) { return (y > 0.0) ? fabs(x) : -fabs(x); }
MH_DEV double stab_q0_at(double t, double dq0, double qv0) { double v = dq0 * t; v = v + qv0; return v; }
MH_DEV double stab_ridders(const StabSlack& K, double x1, double x2, double fl, double fh, unsigned idx, double dq0, double qv0) {   // CStab:1322-1379
  const double TOL = 1e-4, INF_ = 1.7976931348623157e308;
  double ans = INF_, fm, fnew, s2, xh, xl, xm, xnew;
  if ((fl > 0.0 && fh < 0.0) || (fl < 0.0 && fh > 0.0)) {
    xl = x1; xh = x2;
    for (unsigned j = 0; j < 25; j++) {
      xm = 0.5 * (xl + xh);
      fm = K.at(stab_q0_at(xm, dq0, qv0), idx);
      s2 = sqrt(fm * fm - fl * fh);
      if (s2 == 0.0) return ans;
      xnew = xm + (xm - xl) * ((fl >= fh ? 1.0 : -1.0) * fm / s2);
      ans = xnew;
      fnew = K.at(stab_q0_at(ans, dq0, qv0), idx);
      if (fabs(fnew) < TOL && fnew >= 0.0) return xnew;
      if (stab_sign2(fm, fnew) != fm) { xl = xm; fl = fm; xh = ans; fh = fnew; }
      else if (stab_sign2(fl, fnew) != fl) { xh = ans; fh = fnew; }
      else if (stab_sign2(fh, fnew) != fh) { xl = ans; fl = fnew; }
    }
  } else {
    if (fl == 0.0) return x1;
    if (fh == 0.0) return x2;
  }
  return 0.0;
}
__device__ __noinline__ void stabilize_limits(const Model& M, const Lay& Y, double* g, WaveRand& rng, int& status,
                                              unsigned long long& solves, unsigned long long& rows, unsigned long long& pivs, unsigned long long& bytes,
                                              unsigned long long& stab_iters, unsigned long long& stab_rows)
{
  const mh_artic_model& m = M.m;
  const unsigned maxit = (unsigned)m.cstab_max_iterations;
  if (maxit == 0) return;
  const int nj = Y.nj, lane = lane_id();
  const double INF_ = 1.7976931348623157e308;
  StabSlack K; K.hi0 = m.hilimit[0]; K.lo0 = m.lolimit[0];
  const double qd_save = (lane < nj) ? g[Y.qd + lane] : 0.0;
  double qv = (lane < nj) ? g[Y.q + lane] : 0.0;                   // the stabiliser's q (CStab:183)
  double max_uvio = K.vio(uni(g[Y.q]));
  unsigned iterations = 0;
  const bool hfin = lane < nj && m.hilimit[lane] < INF_, lfin = lane < nj && m.lolimit[lane] > -INF_;
  const uint64_t mu = ballot(hfin), ml = ballot(lfin);
  const int nl = popc(mu) + popc(ml);                              // a row for every finite limit (CStab:257-304), upper before lower per joint
  while (max_uvio < m.cstab_eps) {
    if (iterations == maxit) break;
    if (iterations == MH_CSTAB_HARD_CAP) { status |= MH_WORLD_STALLED; break; }
    wave_sync();
    if (lane < nj) g[Y.qd + lane] = 0.0;
    double dq = 0.0;
    wave_sync();
    if (nl > 0) {
      if (nl > NLSTAB) { status |= MH_WORLD_UNSUPPORTED; break; }
      // compute_X at the CURRENT configuration: H by the CRB path, its factor, the inverse (ICH:1600-1607)
      if (!dynamics(M, Y, g, nullptr)) { status |= MH_WORLD_LCP_FAILED; break; }
      int* idx = reinterpret_cast<int*>(g + Y.idx);              // idx[k] = joint | (upper << 8)
      if (lane < nj) {
        const int base = popc(mu & lanes_below(lane)) + popc(ml & lanes_below(lane));
        if (hfin) idx[base] = lane | 256;
        if (lfin) idx[base + (hfin ? 1 : 0)] = lane;
      }
      wave_sync();
      inverse_from_factor(Y, g);
      const double* X = g + Y.X;
      double* MM = g + Y.MM;
      for (int e = lane; e < nl * nl; e += 64) {                   // L X L' without the limits' signs (ICH:1763-1771)
        const int a = e % nl, b2 = e / nl;
        const int ia = idx[a] & 255, ib = idx[b2] & 255;
        MM[e] = (b2 >= a) ? X[ia * nj + ib] : X[ib * nj + ia];
      }
      const bool valid = lane < nl;
      const int my = valid ? idx[lane] : 0;
      const int myj = my & 255; const bool myup = (my & 256) != 0;
      double Lv = 0.0;
      if (valid) { const double qj = g[Y.q + myj]; const double viol = myup ? (m.hilimit[myj] - qj) - 0.0 : (qj + 0.0) - m.lolimit[myj];
                   Lv = (viol - fabs(m.cstab_eps)) - NEAR_ZERO_; }     // CStab:434-441
      wave_sync();
      double nrm0 = 0.0;
      for (int e = lane; e < nl * nl; e += 64) { const double a = fabs(MM[e]); nrm0 = (a > nrm0) ? a : nrm0; }
      nrm0 = wave_max(nrm0);
      const double dii = valid ? MM[lane + nl * lane] : 0.0;
      int zsize = 0;                                               // determine_dq's local z: cold lcp_fast, then the Lemke ladder (CStab:954-955)
      double zi = 0.0;
      DenseLds Md; Md.M = MM; Md.n = nl;
      LuScratch S; S.small = g + Y.A; S.ka = nl; S.big = g + Y.A;
      Trace tr; tr.buf = nullptr; tr.cap = 0; tr.len = 0;
      LcpParams P; P.kind = MH_LCP_FAST; P.min_exp = -20; P.step_exp = 1u; P.max_exp = 1; P.piv_tol = -1.0; P.zero_tol = -1.0;
      unsigned piv = 0, total = 0;
      bool ok = lcp_solve_wave(P, c_pow10a, nl, Md, S, g + Y.art, nrm0, dii, Lv, zi, zsize, rng, piv, tr);
      total += piv;
      if (!ok) {
        P.kind = MH_LCP_LEMKE_REG;
        ok = lcp_solve_wave(P, c_pow10a, nl, Md, S, g + Y.art, nrm0, dii, Lv, zi, zsize, rng, piv, tr);
        total += piv;
      }
      solves += 1ull; rows += (unsigned long long)nl; pivs += total; bytes += 8ull * ((unsigned long long)nl * nl + 2ull * nl);
      stab_rows += (unsigned long long)nl;
      // update_from_stacked(pd, z): l = z whatever it holds; dv = X_LT ls; v += dv; dq = the joint velocities
      double* ll = g + Y.l;
      wave_sync();
      if (valid) ll[lane] = (lane < uni(zsize)) ? zi : 0.0;
      wave_sync();
      if (lane < nj) {
        double dv = 0.0;
        for (int k = 0; k < nl; k++) { const int c = idx[k]; const double ls = (c & 256) ? -ll[k] : ll[k]; dv = dv + ls * X[(c & 255) * nj + lane]; }
        const double v = g[Y.qd + lane] + dv;
        g[Y.qd + lane] = v; dq = v;
      }
      wave_sync();
    }
    // update_q (CStab:1056-1216): the line search lives on joint 0's slacks alone
    { const double dq0 = read_lane(dq, 0), qv0 = read_lane(qv, 0);
      double t = 1.0;
      const double q1 = stab_q0_at(1.0, dq0, qv0);                 // qstar = dq + q: dq * 1.0 is dq
      for (unsigned i = 0; i < 2u * (unsigned)nj; i++) {
        const double fo = K.at(qv0, i), fn = K.at(q1, i);
        if (!((fo < 0.0 && fn > 0.0) || (fo > 0.0 && fn < 0.0))) continue;
        const double root = stab_ridders(K, 0.0, t, fo, fn, i, dq0, qv0);
        if (root > 0.0 && root < 1.0) t = (root < t) ? root : t;
      }
      bool failed = false;
      while (true) {
        const double qt = stab_q0_at(t, dq0, qv0);
        bool stop = true;
        for (unsigned i = 0; i < 2u * (unsigned)nj; i++) {
          const double fo = K.at(qv0, i), fn1 = K.at(q1, i), fc = K.at(qt, i);
          const bool br = (fo < 0.0 && fn1 > 0.0) || (fo > 0.0 && fn1 < 0.0);
          if (!br && fc < 0.0 && fo > fc) { stop = false; break; }
        }
        if (stop) break;
        t *= 0.6;
        if (t < NEAR_ZERO_) { failed = true; break; }
      }
      if (failed) { status |= MH_WORLD_STAB_FAILED; break; }
      if (lane < nj) { double v = dq * t; v = v + qv; qv = v; g[Y.q + lane] = v; }
      wave_sync();
    }
    max_uvio = K.vio(uni(g[Y.q]));
    iterations++;
    stab_iters += 1ull;
  }
  wave_sync();
  if (lane < nj) { g[Y.qd + lane] = qd_save; g[Y.q + lane] = qv; }
  wave_sync();
}

#if defined(MH_ARTIC_DRIVE_TU) || defined(MH_ARTIC_POSE_TU) || defined(MH_ARTIC_BOX_TU)
// The drive (moby_hip_artic.h, mh_artic_drive): lane j < nj evaluates tau_j of step s from q / qd in LDS -- q already advanced by the
// mini-step's position update, qd still its starting velocity -- and leaves it in the qdd slot of the image: dynamics() reads
// tau_w[lane] there before the same lane writes b[lane] (CRB), dynamics_aba() reads every tau_w[i] on lane 0 in its inward pass,
// before the outward pass writes qdd.  No LDS of its own; kp / kv come from L2 at every mini-step.
MH_DEV void drive_tau(const mh_artic_drive& D, int B, int b, int s, const Lay& Y, double* g)
{
  const int nj = Y.nj, lane = lane_id();
  if (lane < nj) {
    const size_t o = (size_t)b * nj + lane;
    const size_t r = (size_t)(D.rows == 1 ? 0 : s) * (size_t)B * nj + o;
    double t = 0.0;
    if (D.terms & MH_DRIVE_PD) {
      const double ep = D.q_des[r] - g[Y.q + lane], ev = D.qd_des[r] - g[Y.qd + lane];
      const double tp = D.kp[o] * ep, tv = D.kv[o] * ev;
      t = tp + tv;
      if (D.terms & MH_DRIVE_FORCE) t = t + D.tau_ff[r];
    } else t = D.tau_ff[r];
    g[Y.qdd + lane] = t;
  }
}
#endif

#ifdef MH_ARTIC_POSE_TU
// Pose coordinates of a floating base (moby_hip_artic.h, MH_ARTIC_BASE_POSE).  Operation order = tests/native/artic_pose_ref.cpp, bit for bit.
// Hamilton product o = a (x) b, quaternions stored w, x, y, z
MH_DEV void quat_mul(const double* a, const double* b, double* o)
{
  o[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
  o[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
  o[2] = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
  o[3] = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
}
// R(Q), row-major, for a unit Q
MH_DEV void quat_R(const double* Q, double* R)
{
  const double w = Q[0], x = Q[1], y = Q[2], z = Q[3];
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
  R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz);       R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz);       R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy);       R[7] = 2.0 * (yz + wx);       R[8] = 1.0 - 2.0 * (xx + yy);
}
// The fold: the six virtual joints' coordinates into the pose, q[0..5] back to zero (one thread; q, qd: the world's joint arrays; p, Q, R: its
// pose).  p += q[0..2] (the sum kinematics forms for the base COM); Q = normalize(Q (x) Qx(q3) (x) Qy(q4) (x) Qz(q5)); qd[3..5] = the base's
// angular velocity in its new axes, Rh' (e_x qd3 + Rx e_y qd4 + Rx Ry e_z qd5) = Rz(q5)' (Ry(q4)' (e_x qd3 + e_y qd4) + e_z qd5), full-angle
// sin / cos by the double-angle formulas from the half angles; qd[0..2] (the COM velocity, global axes) stay
MH_DEV void pose_fold(double* q, double* qd, double* p, double* Q, double* R)
{
  for (int k = 0; k < 3; k++) p[k] = p[k] + q[k];
  double s3, c3, s4, c4, s5, c5;
  sincos_kernel(0.5 * q[3], s3, c3); sincos_kernel(0.5 * q[4], s4, c4); sincos_kernel(0.5 * q[5], s5, c5);
  const double qx[4] = { c3, s3, 0.0, 0.0 }, qy[4] = { c4, 0.0, s4, 0.0 }, qz[4] = { c5, 0.0, 0.0, s5 };
  double t1[4], t2[4], t3[4];
  quat_mul(Q, qx, t1); quat_mul(t1, qy, t2); quat_mul(t2, qz, t3);
  const double n = sqrt(((t3[0] * t3[0] + t3[1] * t3[1]) + t3[2] * t3[2]) + t3[3] * t3[3]);
  for (int k = 0; k < 4; k++) Q[k] = t3[k] / n;
  const double S4 = 2.0 * (s4 * c4), C4 = c4 * c4 - s4 * s4, S5 = 2.0 * (s5 * c5), C5 = c5 * c5 - s5 * s5;
  const double u0 = C4 * qd[3], u1 = qd[4], u2 = S4 * qd[3] + qd[5];
  qd[3] = C5 * u0 + S5 * u1; qd[4] = C5 * u1 - S5 * u0; qd[5] = u2;
  for (int k = 0; k < 6; k++) q[k] = 0.0;
  quat_R(Q, R);
}
// world b's pose from HBM (B x 7: p, Q) into the image's slots, R(Q) rebuilt; the caller syncs
MH_DEV void pose_load(const Lay& Y, double* g, const double* __restrict__ pose)
{
  if (lane_id() == 0) {
    for (int k = 0; k < 3; k++) g[Y.pp + k] = pose[k];
    for (int k = 0; k < 4; k++) g[Y.pQ + k] = pose[3 + k];
    quat_R(g + Y.pQ, g + Y.pR);
  }
}
MH_DEV void pose_store(const Lay& Y, const double* g, double* __restrict__ pose)
{
  if (lane_id() == 0) { for (int k = 0; k < 3; k++) pose[k] = g[Y.pp + k]; for (int k = 0; k < 4; k++) pose[3 + k] = g[Y.pQ + k]; }
}
// after a step that ran to its end: lane 0 folds the image's q / qd into its pose
MH_DEV void pose_fold_lds(const Lay& Y, double* g)
{
  wave_sync();
  if (lane_id() == 0) pose_fold(g + Y.q, g + Y.qd, g + Y.pp, g + Y.pQ, g + Y.pR);
  wave_sync();
}
#endif

// MH_ARTIC_DRIVE_TU (mh_artic_drive.hip): the same step with a drive -- the undriven kernels are compiled from exactly the code they had before drives existed.
// MH_ARTIC_POSE_TU (mh_artic_pose.hip): the same step in pose coordinates, driven when Dp is not NULL (a constant after inlining)
template <bool STAB>
MH_DEV void artic_step_body(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                            mh_world_aux* __restrict__ auxg
#ifdef MH_ARTIC_DRIVE_TU
                            , const mh_artic_drive& D
#endif
#ifdef MH_ARTIC_POSE_TU
                            , const mh_artic_drive* Dp, double* __restrict__ poseg
#endif
                            )
{
  extern __shared__ double g[];
  const int b = blockIdx.x;
  if (b >= B) return;
  const Model& M = *Mg;
  const int nj = M.m.nj, lane = lane_id();
  const Lay Y(nj, STAB ? NLSTAB : NLMAX);
  mh_world_aux* aux = auxg + b;
  if (lane < nj) { g[Y.q + lane] = qg[(size_t)b * nj + lane]; g[Y.qd + lane] = qdg[(size_t)b * nj + lane]; }
#ifdef MH_ARTIC_POSE_TU
  pose_load(Y, g, poseg + 7 * (size_t)b);
#endif
  WaveRand rng; rng.load(aux->rng);
  if (lane == 0) g_lcp_prof_on = 0;
  int status = uni(aux->status);
  unsigned long long solves = 0, rows = 0, pivs = 0, bytes = 0, stab_iters = 0, stab_rows = 0;
  // An exception of calc_fwd_dyn, the impact handler or compute_X ends the run (oracle Artic::step): the state stays where the throw left it (positions
  // integrated, velocities without the impulses), time and counters without that step, and a world that carries MH_WORLD_LCP_FAILED is not stepped again.
  int minis = 0, steps = 0;                                          // mini-steps whose time was added / steps that ran to their end
  wave_sync();
  for (int s = 0; s < nsteps; s++) {
    if (status & MH_WORLD_LCP_FAILED) break;
    // positions with the OLD velocity (TSS:156-164)
    if (lane < nj) { double qn = g[Y.qd + lane] * dt; qn = qn + g[Y.q + lane]; g[Y.q + lane] = qn; }
#ifdef MH_ARTIC_DRIVE_TU
    drive_tau(D, B, b, s, Y, g);                                      // precalc_fwd_dyn's controller (Simulator.cpp:319-350): lane j reads the q it just wrote
    wave_sync();
    const bool ok = (M.m.algorithm == MH_ARTIC_FSAB) ? dynamics_aba(M, Y, g, g + Y.qdd) : dynamics(M, Y, g, g + Y.qdd);
#elif defined(MH_ARTIC_POSE_TU)
    if (Dp) drive_tau(*Dp, B, b, s, Y, g);
    wave_sync();
    const double* tw = Dp ? g + Y.qdd : nullptr;
    const bool ok = (M.m.algorithm == MH_ARTIC_FSAB) ? dynamics_aba(M, Y, g, tw) : dynamics(M, Y, g, tw);
#else
    wave_sync();
    const bool ok = (M.m.algorithm == MH_ARTIC_FSAB) ? dynamics_aba(M, Y, g, nullptr) : dynamics(M, Y, g, nullptr);
#endif
    if (!ok) { status |= MH_WORLD_LCP_FAILED; break; }
    if (lane < nj) g[Y.qd + lane] = g[Y.qd + lane] + g[Y.qdd + lane] * dt;   // TSS:182-192
    wave_sync();
    handle_limits(M, Y, g, aux, rng, status, solves, rows, pivs, bytes);
    wave_sync();
    if (status & MH_WORLD_LCP_FAILED) break;
    minis++;
    if (STAB) { stabilize_limits(M, Y, g, rng, status, solves, rows, pivs, bytes, stab_iters, stab_rows); if (status & MH_WORLD_LCP_FAILED) break; }   // TSS:97
    steps++;
#ifdef MH_ARTIC_POSE_TU
    pose_fold_lds(Y, g);                                              // after the stabiliser: the step ran to its end
#endif
  }
  wave_sync();
  if (lane < nj) { qg[(size_t)b * nj + lane] = g[Y.q + lane]; qdg[(size_t)b * nj + lane] = g[Y.qd + lane]; }
#ifdef MH_ARTIC_POSE_TU
  pose_store(Y, g, poseg + 7 * (size_t)b);
#endif
  rng.store(aux->rng);
  if (lane == 0) {
    double tm = aux->time; for (int s = 0; s < minis; s++) tm += dt;
    aux->time = tm; aux->status = status;
    aux->steps += (unsigned long long)steps; aux->mini_steps += (unsigned long long)minis;
    aux->lcp_solves += solves; aux->lcp_rows += rows; aux->lcp_pivots += pivs; aux->lcp_alg_bytes += bytes;
    aux->stab_iters += stab_iters; aux->stab_rows += stab_rows;
  }
}

#if !defined(MH_ARTIC_DRIVE_TU) && !defined(MH_ARTIC_POSE_TU) && !defined(MH_ARTIC_BOX_TU)
// The same step at three register budgets: 128 VGPRs (4 waves per SIMD = the 16 worlds per CU the 10 KB LDS image allows; 95 spilled
// VGPRs), 168 (3 per SIMD, 14 spilled) and 193 (2 per SIMD, none).  The kernel waits on ~250 LDS round trips per step, so
// resident waves win over spills: ur10 x 8192, 200 steps: 25.6 / 31.2 / 39.0 ms (profiles/r02_c_artic_occupancy.jsonl).
// Default 4; MH_ARTIC_WAVES=2|3|5 selects the others (experiments).  Round 5: with the local transforms sharing v / a the image is 9 KB = 18 worlds per CU, and the
// five-waves build (96 VGPRs, 132 spilled) was measured on them: 29.2 ms against 25.5 -- at this point the SPILLS cost more than the fifth wave hides, so a smaller
// image alone buys nothing: the routine needs fewer live registers first (profiles/r05_d_artic_occupancy.txt).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void k_artic_step_w3(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                     mh_world_aux* __restrict__ auxg) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_artic_step_w4(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                     mh_world_aux* __restrict__ auxg) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5)))
void k_artic_step_w5(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                     mh_world_aux* __restrict__ auxg) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg); }
__global__ __launch_bounds__(64)
void k_artic_step_w2(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                     mh_world_aux* __restrict__ auxg) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg); }

// TWO worlds per wavefront (round 4): lanes 0-31 step world 2b, lanes 32-63 world 2b + 1, out of two LDS images, through ONE instruction
// stream -- the kernel is bound by instruction issue and LDS round trips with 6-36 of 64 lanes at work, so the second world rides on
// instructions the first one pays for.  The forward dynamics (kinematics, RNEA, CRBA, Cholesky: no data-dependent control flow) run
// packed; the joint-limit handler, whose pivoting loops are wave-uniform per WORLD, runs on each world in turn with the whole wave (it
// leaves at once when no limit is hit).  16 worlds per CU as before (8 waves x 2 images of 10 KB) at 256 registers per lane: no spills.
// CRB bodies without spheres and without the stabiliser (config 5).  Selected by MH_ARTIC_PACK=1 (see mh_artic_batch_step for what it measured).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_artic_step_p2(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                     mh_world_aux* __restrict__ auxg)
{
  extern __shared__ double g[];
  const int b0 = 2 * (int)blockIdx.x;
  if (b0 >= B) return;
  const Model& M = *Mg;
  const int nj = M.m.nj, lane = lane_id(), wl = lane >> 5, hl = lane & 31;
  const Lay Y(nj);
  const bool two = b0 + 1 < B;                                       // (an odd batch: the last wave's second half idles on an image nobody reads)
  const int b = b0 + wl;
  double* gw = g + (size_t)wl * Y.total;                             // this lane's world
  const bool mine = hl < nj && (wl == 0 || two);
  if (hl < nj) { gw[Y.q + hl] = mine ? qg[(size_t)b * nj + hl] : 0.0; gw[Y.qd + hl] = mine ? qdg[(size_t)b * nj + hl] : 0.0; }
  WaveRand rng0, rng1; rng0.load(auxg[b0].rng); rng1.load(auxg[two ? b0 + 1 : b0].rng);
  if (lane == 0) g_lcp_prof_on = 0;
  int status0 = uni(auxg[b0].status), status1 = two ? uni(auxg[b0 + 1].status) : 0;
  unsigned long long solves0 = 0, rows0 = 0, pivs0 = 0, bytes0 = 0, solves1 = 0, rows1 = 0, pivs1 = 0, bytes1 = 0;
  int n0 = 0, n1 = 0;                                                // steps each world ran to their end (an exception ends a world's run: artic_step_body)
  wave_sync();
  for (int s = 0; s < nsteps; s++) {
    const bool a0 = !(status0 & MH_WORLD_LCP_FAILED), a1 = two && !(status1 & MH_WORLD_LCP_FAILED);    // still running (uniform)
    if (!a0 && !a1) break;
    const bool alive = (wl == 0) ? a0 : a1;                           // this lane's world: a dead world's image is computed on and never written back
    if (hl < nj && alive) { double qn = gw[Y.qd + hl] * dt; qn = qn + gw[Y.q + hl]; gw[Y.q + hl] = qn; }      // positions with the OLD velocity (TSS:156-164)
    wave_sync();
    const bool okl = dynamics<2>(M, Y, gw, nullptr);
    const bool ok0 = (ballot(okl) & 1ull) != 0ull, ok1 = ((ballot(okl) >> 32) & 1ull) != 0ull;
    if (a0 && !ok0) status0 |= MH_WORLD_LCP_FAILED;
    if (a1 && !ok1) status1 |= MH_WORLD_LCP_FAILED;
    if (hl < nj && alive && okl) gw[Y.qd + hl] = gw[Y.qd + hl] + gw[Y.qdd + hl] * dt;   // TSS:182-192
    wave_sync();
    if (a0 && ok0) handle_limits(M, Y, g, auxg + b0, rng0, status0, solves0, rows0, pivs0, bytes0);
    wave_sync();
    if (a1 && ok1) handle_limits(M, Y, g + Y.total, auxg + b0 + 1, rng1, status1, solves1, rows1, pivs1, bytes1);
    wave_sync();
    if (a0 && !(status0 & MH_WORLD_LCP_FAILED)) n0++;
    if (a1 && !(status1 & MH_WORLD_LCP_FAILED)) n1++;
  }
  if (mine) { qg[(size_t)b * nj + hl] = gw[Y.q + hl]; qdg[(size_t)b * nj + hl] = gw[Y.qd + hl]; }
  rng0.store(auxg[b0].rng);
  if (two) rng1.store(auxg[b0 + 1].rng);
  if (lane == 0) {
    for (int w = 0; w < (two ? 2 : 1); w++) {
      mh_world_aux* aux = auxg + b0 + w;
      const int nw = w ? n1 : n0;
      double tm = aux->time; for (int s = 0; s < nw; s++) tm += dt;
      aux->time = tm; aux->status = w ? status1 : status0;
      aux->steps += (unsigned long long)nw; aux->mini_steps += (unsigned long long)nw;
      aux->lcp_solves += w ? solves1 : solves0; aux->lcp_rows += w ? rows1 : rows0; aux->lcp_pivots += w ? pivs1 : pivs0; aux->lcp_alg_bytes += w ? bytes1 : bytes0;
    }
  }
}

// the same step followed by ConstraintStabilization::stabilize (joint-limit rows): its own kernel, so that bodies stepped with
// stabilisation off (ur10.xml:11) carry neither its registers nor its 20 KB LDS image (a row for every finite limit: 2 nj)
__global__ __launch_bounds__(64)
void k_artic_step_stab(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                       mh_world_aux* __restrict__ auxg) { artic_step_body<true>(Mg, B, dt, nsteps, qg, qdg, auxg); }
#endif

#if (!defined(MH_ARTIC_DRIVE_TU) && !defined(MH_ARTIC_BOX_TU)) || (defined(MH_ARTIC_PARAMS_TU) && !defined(MH_ARTIC_WRENCH_TU))   // (a wrench batch's queries go through mh_artic_pw[_pose].hip)
// k_artic_fwd_dyn / k_artic_jacobian, and in pose coordinates k_artic_fwd_dyn_pose / k_artic_jacobian_pose: one more argument, the B x 7 poses
// (MH_ARTIC_PARAMS_TU: k_artic_fwd_dyn_pw[_pose] / k_artic_jacobian_pw[_pose], which read world b's own image of B)
#if defined(MH_ARTIC_PARAMS_TU) && defined(MH_ARTIC_POSE_TU)
#define MH_POSE_KERNEL(name) name##_pw_pose
#define MH_POSE_ARG , const double* __restrict__ poseg
#define MH_POSE_LOAD() pose_load(Y, g, poseg + 7 * (size_t)b)
#elif defined(MH_ARTIC_PARAMS_TU)
#define MH_POSE_KERNEL(name) name##_pw
#define MH_POSE_ARG
#define MH_POSE_LOAD() ((void)0)
#elif defined(MH_ARTIC_POSE_TU)
#define MH_POSE_KERNEL(name) name##_pose
#define MH_POSE_ARG , const double* __restrict__ poseg
#define MH_POSE_LOAD() pose_load(Y, g, poseg + 7 * (size_t)b)
#else
#define MH_POSE_KERNEL(name) name
#define MH_POSE_ARG
#define MH_POSE_LOAD() ((void)0)
#endif
// seam B4: qdd = H^-1 (tau - C), H, link poses of the resident states
__global__ __launch_bounds__(64)
void MH_POSE_KERNEL(k_artic_fwd_dyn)(const Model* __restrict__ Mg, int B, const double* __restrict__ qg, const double* __restrict__ qdg,
                     const double* __restrict__ tau, double* __restrict__ qdd_out, double* __restrict__ H_out, double* __restrict__ poses,
                     int* __restrict__ okflag MH_POSE_ARG)
{
  extern __shared__ double g[];
  const int b = blockIdx.x;
  if (b >= B) return;
#ifdef MH_ARTIC_PARAMS_TU
  const Model& M = Mg[b];
#else
  const Model& M = *Mg;
#endif
  const int nj = M.m.nj, lane = lane_id();
  const Lay Y(nj);
  if (lane < nj) { g[Y.q + lane] = qg[(size_t)b * nj + lane]; g[Y.qd + lane] = qdg[(size_t)b * nj + lane]; }
  MH_POSE_LOAD();
  wave_sync();
  const double* tw = tau ? tau + (size_t)b * nj : nullptr;
  bool ok;
  if (M.m.algorithm == MH_ARTIC_FSAB) {
    ok = dynamics_aba(M, Y, g, tw);
    if (qdd_out && lane < nj) qdd_out[(size_t)b * nj + lane] = ok ? g[Y.qdd + lane] : 0.0;
    wave_sync();
    if (H_out) (void)dynamics(M, Y, g, tw);                // the generalized inertia is CRB's whatever the algorithm
  } else {
    ok = dynamics(M, Y, g, tw);
    if (qdd_out && lane < nj) qdd_out[(size_t)b * nj + lane] = ok ? g[Y.qdd + lane] : 0.0;
  }
  if (H_out) for (int e = lane; e < nj * nj; e += 64) H_out[(size_t)b * nj * nj + e] = g[Y.H + e];
  if (poses) for (int e = lane; e < 12 * nj; e += 64) { const int i = e / 12, k = e - 12 * i; poses[(size_t)b * 12 * nj + e] = (k < 9) ? g[Y.R + 9 * i + k] : g[Y.x + 3 * i + k - 9]; }
  if (okflag && lane == 0) okflag[b] = ok ? 1 : 0;
}

// calc_jacobian: column j = the twist of joint j (S_j, about the world origin) moved to the point, for j on the link's path
__global__ __launch_bounds__(64)
void MH_POSE_KERNEL(k_artic_jacobian)(const Model* __restrict__ Mg, int B, const double* __restrict__ qg, int link, const double* __restrict__ points,
                      double* __restrict__ J_out MH_POSE_ARG)
{
  extern __shared__ double g[];
  const int b = blockIdx.x;
  if (b >= B) return;
#ifdef MH_ARTIC_PARAMS_TU
  const Model& M = Mg[b];
#else
  const Model& M = *Mg;
#endif
  const int nj = M.m.nj, lane = lane_id();
  const Lay Y(nj);
  if (lane < nj) { g[Y.q + lane] = qg[(size_t)b * nj + lane]; g[Y.qd + lane] = 0.0; }
  MH_POSE_LOAD();
  wave_sync();
  kin_inertia(M, Y, g);
  const double* p = points + (size_t)b * 3;
  for (int e = lane; e < 6 * nj; e += 64) {
    const int r = e / nj, j = e - r * nj;
    double v = 0.0;
    if ((M.anc[link] >> j) & 1u) {
      const double* S = g + Y.S + 6 * j;                  // [angular; linear at the origin]
      if (r >= 3) v = S[r - 3];
      else { const int k1 = (r + 1) % 3, k2 = (r + 2) % 3; v = S[3 + r] + (S[k1] * p[k2] - S[k2] * p[k1]); }   // v_o + w x p
    }
    J_out[(size_t)b * 6 * nj + e] = v;
  }
}
#endif

#if defined(MH_ARTIC_DRIVE_TU)   // the driven step kernels: their own code object (mh_artic_drive.hip)
// the four budgets of k_artic_step_w{2..5} with a drive (mh_artic_batch_step_driven)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void k_artic_step_w3_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                           mh_world_aux* __restrict__ auxg, mh_artic_drive D) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, D); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_artic_step_w4_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                           mh_world_aux* __restrict__ auxg, mh_artic_drive D) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, D); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5)))
void k_artic_step_w5_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                           mh_world_aux* __restrict__ auxg, mh_artic_drive D) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, D); }
__global__ __launch_bounds__(64)
void k_artic_step_w2_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                           mh_world_aux* __restrict__ auxg, mh_artic_drive D) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, D); }

// k_artic_step_stab with a drive
__global__ __launch_bounds__(64)
void k_artic_step_stab_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                             mh_world_aux* __restrict__ auxg, mh_artic_drive D) { artic_step_body<true>(Mg, B, dt, nsteps, qg, qdg, auxg, D); }
#elif defined(MH_ARTIC_POSE_TU) && !defined(MH_ARTIC_BOX_TU)  // the pose-coordinate step kernels: their own code object (mh_artic_pose.hip)
// the default budget of k_artic_step_w4 (MH_ARTIC_WAVES and MH_ARTIC_PACK do not apply in pose coordinates), undriven and driven
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_artic_step_w4_pose(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                          mh_world_aux* __restrict__ auxg, double* __restrict__ poseg) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, nullptr, poseg); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_artic_step_w4_pose_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                mh_world_aux* __restrict__ auxg, double* __restrict__ poseg, mh_artic_drive D) { artic_step_body<false>(Mg, B, dt, nsteps, qg, qdg, auxg, &D, poseg); }
// k_artic_step_stab in pose coordinates, undriven and driven
__global__ __launch_bounds__(64)
void k_artic_step_stab_pose(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                            mh_world_aux* __restrict__ auxg, double* __restrict__ poseg) { artic_step_body<true>(Mg, B, dt, nsteps, qg, qdg, auxg, nullptr, poseg); }
__global__ __launch_bounds__(64)
void k_artic_step_stab_pose_drive(const Model* __restrict__ Mg, int B, double dt, int nsteps, double* __restrict__ qg, double* __restrict__ qdg,
                                  mh_world_aux* __restrict__ auxg, double* __restrict__ poseg, mh_artic_drive D) { artic_step_body<true>(Mg, B, dt, nsteps, qg, qdg, auxg, &D, poseg); }
// the switch from angles to pose coordinates (mh_artic_batch_set_base_coords): one thread per world folds its resident q / qd into the pose the
// host wrote (the model's); a world carrying MH_WORLD_LCP_FAILED keeps its q, which still describe its configuration against that pose
__global__ __launch_bounds__(64)
void k_artic_pose_fold(int B, int nj, double* __restrict__ qg, double* __restrict__ qdg, const mh_world_aux* __restrict__ auxg, double* __restrict__ poseg)
{
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B || (auxg[b].status & MH_WORLD_LCP_FAILED)) return;
  double R[9];
  pose_fold(qg + (size_t)b * nj, qdg + (size_t)b * nj, poseg + 7 * (size_t)b, poseg + 7 * (size_t)b + 3, R);
}
#endif

#include "mh_artic_contacts.inc"

}} // namespace mh::artic

// the kernels a batch with geometry beyond spheres against the plane steps through; a later family holds all the work of the earlier ones
enum mh_artic_family { MH_ARTIC_FAM_NONE = 0,  // no geometry, or spheres against the plane: the kernels of mh_artic.hip / mh_artic_drive.hip / mh_artic_pose.hip
                       MH_ARTIC_FAM_BOX,       // box primitives (mh_artic_box.hip)
                       MH_ARTIC_FAM_PAIR,      // sphere pairs between links or a plane mask (mh_artic_pair.hip), and every model with geometry created under mh_debug_set(13, 1)
                       MH_ARTIC_FAM_BSP,       // a box-sphere pair or a static box (mh_artic_bsp.hip), and every model with geometry created under mh_debug_set(14, 1)
                       MH_ARTIC_FAM_RP,        // the contact report (mh_artic_rp.hip): every batch of mh_artic_batch_create_report, and one that would take BSP created under mh_debug_set(19, 1)
                       MH_ARTIC_FAM_PW,        // per-world parameters (mh_artic_pw.hip): every batch of mh_artic_batch_create_params, and one that would take RP created under mh_debug_set(20, 1)
                       MH_ARTIC_FAM_WR };      // link wrenches (mh_artic_wr.hip): every batch of mh_artic_batch_create_wrench, and one that would take PW created under mh_debug_set(21, 1)

struct mh_artic_batch {
  int device;                // the HIP device the batch lives on (current at create); every entry point runs there (MH_ON_DEVICE)
  int B, nj, nspheres, cstab, algorithm;
  mh_artic_family family;    // fixed at create, and with it the workspace layout (artic_geom_family: what a step goes through)
  int report;                // created by mh_artic_batch_create_report: mh_artic_batch_step_report may hand it rows to write
  int params;                // d_model holds B images, one per world, and the step goes through MH_ARTIC_FAM_PW: 1 = created by mh_artic_batch_create_params
                             // (the setters take it), 2 = created under mh_debug_set(20, 1) with every image the model's; 0 = one shared image
  mh_artic_model model;      // the shared model as it was handed to create: the topology every record is written into and validated against
  int wrench;                // created by mh_artic_batch_create_wrench: mh_artic_batch_step_wrench may hand it a wrench (the step goes through MH_ARTIC_FAM_WR)
  mh::artic::Model* d_model;
  double* d_q; double* d_qd; mh_world_aux* d_aux;
  double* d_ws;           // link contacts with the Drumwright-Shell model: _MM + LU workspace, 2 x 64 x 64 doubles per world
  size_t ws_stride;       // doubles per world in d_ws: 2 x 64 x 64, WS_BOX for the box kernels (their stabiliser keeps its rows there too), WS_PAIR for the pair and box-sphere kernels
  mh_artic_drive drive;   // the drive of mh_artic_batch_set_drive (terms 0 = none); its arrays live in d_drive
  double* d_drive;
  int base_coords;        // MH_ARTIC_BASE_ANGLES / MH_ARTIC_BASE_POSE (mh_artic_batch_set_base_coords)
  double* d_pose;         // pose coordinates: B x 7 (p, Q) per world; NULL in angle coordinates
};

// the pose-coordinate launches (mh_artic_pose.hip): the step (D NULL or terms 0 = undriven; arguments checked by the caller), and the
// kernels of mh_artic_batch_fwd_dyn / link_poses (on `stream`: the host entries pass the null stream, mh_artic_batch_link_poses_dev the caller's) /
// jacobian (the null stream)
int artic_pose_step(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D);
hipError_t artic_pose_fwd_dyn_launch(mh_artic_batch* ab, void* stream, const double* d_tau, double* d_qdd, double* d_H, double* d_poses, int* d_ok);
hipError_t artic_pose_jacobian_launch(mh_artic_batch* ab, int link, const double* d_p, double* d_J);

// the family a step of the batch goes through: the one fixed at create, except that mh_debug_set(12, 1) sends a sphere-only batch through the box
// kernels when it steps (artic_geom_step refuses one created before the key was set: its workspace has the sphere kernels' layout)
static inline mh_artic_family artic_geom_family(const mh_artic_batch* ab)
{
  return (ab->family == MH_ARTIC_FAM_NONE && ab->nspheres > 0 && mh_g_debug_artic_box != 0) ? MH_ARTIC_FAM_BOX : ab->family;
}
// the router (mh_artic.hip): every step of a batch whose family is not MH_ARTIC_FAM_NONE -- the family's workspace and LDS checks, then the
// launcher of that family and of the batch's coordinates; D as artic_pose_step's
// report: the rows a batch of the report family writes (NULL: none; every other family ignores it)
// wrench: the link wrench a batch of the wrench family applies (NULL or terms 0: none; every other family ignores it)
int artic_geom_step(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D, double* report = nullptr, const mh_artic_wrench* wrench = nullptr);
// the launchers, one per geometry code object (stamped at the end of this header): nothing but the launch of one of its four kernels
#define MH_ARTIC_LAUNCHER(name) int name(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D)
MH_ARTIC_LAUNCHER(artic_box_launch);  MH_ARTIC_LAUNCHER(artic_box_pose_launch);
MH_ARTIC_LAUNCHER(artic_pair_launch); MH_ARTIC_LAUNCHER(artic_pair_pose_launch);
MH_ARTIC_LAUNCHER(artic_bsp_launch);  MH_ARTIC_LAUNCHER(artic_bsp_pose_launch);
// the LDS image of the pair layout at nj joints in angle coordinates, in bytes (mh_artic_pair.hip: the contact list's length differs per code object;
// the box-sphere kernels' image is the same).  mh_artic_batch_create and the router refuse a model whose image would not fit a workgroup
size_t artic_pair_lds_bytes(int nj);
// the report family's launchers take the rows too, and its LDS image is its own (the pair layout plus the accumulators and the slot table), per
// coordinate kind: mh_artic_rp.hip and mh_artic_rp_pose.hip each export theirs
#define MH_ARTIC_REPORT_LAUNCHER(name) int name(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D, double* report)
MH_ARTIC_REPORT_LAUNCHER(artic_rp_launch); MH_ARTIC_REPORT_LAUNCHER(artic_rp_pose_launch);
size_t artic_rp_lds_bytes(int nj);
size_t artic_rp_pose_lds_bytes(int nj);
// the per-world-parameters family (mh_artic_pw.hip, mh_artic_pw_pose.hip): the report family's launchers and image sizes over B images, the
// kernels of mh_artic_batch_fwd_dyn / link_poses / jacobian that read world b's image (streams as the pose forms above), and the scatter of
// mh_artic_batch_set_params_dev (records rec[0 .. count) into images first ..; the launch's hipGetLastError)
MH_ARTIC_REPORT_LAUNCHER(artic_pw_launch); MH_ARTIC_REPORT_LAUNCHER(artic_pw_pose_launch);
size_t artic_pw_lds_bytes(int nj);
size_t artic_pw_pose_lds_bytes(int nj);
hipError_t artic_pw_fwd_dyn_launch(mh_artic_batch* ab, void* stream, const double* d_tau, double* d_qdd, double* d_H, double* d_poses, int* d_ok);
hipError_t artic_pw_pose_fwd_dyn_launch(mh_artic_batch* ab, void* stream, const double* d_tau, double* d_qdd, double* d_H, double* d_poses, int* d_ok);
hipError_t artic_pw_jacobian_launch(mh_artic_batch* ab, int link, const double* d_p, double* d_J);
hipError_t artic_pw_pose_jacobian_launch(mh_artic_batch* ab, int link, const double* d_p, double* d_J);
hipError_t artic_pw_scatter_launch(mh_artic_batch* ab, void* stream, const mh_artic_params* dev, int first, int count);
// episodes on the device (mh_artic_reset.hip: a code object of two small kernels that knows nothing of the model): the launches of
// mh_artic_batch_reset_dev and mh_artic_batch_status_dev on `stream`, raw pointers into the batch's arrays; the launch's hipGetLastError
hipError_t artic_reset_launch(void* stream, int B, int nj, const int* mask, const double* q_src, const double* qd_src, const double* pose_src,
                              double* q, double* qd, double* pose, mh_world_aux* aux);
hipError_t artic_status_launch(void* stream, int B, const mh_world_aux* aux, int* status_dst, double* time_dst);
// the wrench family (mh_artic_wr.hip, mh_artic_wr_pose.hip): the per-world-parameters family's step launchers with the wrench (NULL or terms 0: none),
// and its image sizes -- the per-world-parameters family's, the wrench lives in regions the image already has
#define MH_ARTIC_WRENCH_LAUNCHER(name) int name(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* D, double* report, const mh_artic_wrench* W)
MH_ARTIC_WRENCH_LAUNCHER(artic_wr_launch); MH_ARTIC_WRENCH_LAUNCHER(artic_wr_pose_launch);
size_t artic_wr_lds_bytes(int nj);
size_t artic_wr_pose_lds_bytes(int nj);

// the checks mh_artic_batch_step_driven (mh_artic_drive.hip) and mh_artic_batch_set_drive share (nsteps < 0: no schedule length to check against)
static int check_drive(const mh_artic_drive* d, int nsteps)
{
  if (d->terms & ~(MH_DRIVE_FORCE | MH_DRIVE_PD)) return fail(MH_ERR_INVALID_ARG, "drive: unknown bits 0x%x in terms", d->terms & ~(MH_DRIVE_FORCE | MH_DRIVE_PD));
  if ((d->terms & MH_DRIVE_FORCE) && !d->tau_ff) return fail(MH_ERR_INVALID_ARG, "drive: MH_DRIVE_FORCE with a NULL tau_ff");
  if ((d->terms & MH_DRIVE_PD) && (!d->kp || !d->kv || !d->q_des || !d->qd_des)) return fail(MH_ERR_INVALID_ARG, "drive: MH_DRIVE_PD with a NULL kp, kv, q_des or qd_des");
  if (d->rows < 1) return fail(MH_ERR_INVALID_ARG, "drive: rows = %d < 1", d->rows);
  if (nsteps >= 0 && d->rows > 1 && d->rows < nsteps) return fail(MH_ERR_INVALID_ARG, "drive: %d schedule rows for %d steps (1 = held, or at least one per step)", d->rows, nsteps);
  return MH_OK;
}

// the regularisation ladder's powers of ten into c_pow10a: every code object has its own copy of the symbol, and a second GPU of the process its own
// again, so once per translation unit (the function and its `done` are static) and per device, under a lock.  Called before a code object's
// first launch on a device: by mh_artic_batch_create for mh_artic.hip's, by every other launcher for its own
static int init_pow10()
{
  static std::mutex mu; static std::vector<char> done;
  std::lock_guard<std::mutex> lk(mu);
  int dev = 0; MH_HIP(hipGetDevice(&dev));
  if ((int)done.size() <= dev) done.resize(dev + 1, 0);
  if (!done[dev]) {
    mh::Pow10Table p10; for (int i = 0; i < 64; i++) p10.v[i] = std::pow(10.0, (double)(i - 32));   // LCP.cpp:285
    MH_HIP(hipMemcpyToSymbol(HIP_SYMBOL(mh::artic::c_pow10a), &p10, sizeof(p10)));
    done[dev] = 1;
  }
  return MH_OK;
}

#ifdef MH_ARTIC_GEOM
// a geometry code object's launcher, artic_<fam>_launch or artic_<fam>_pose_launch: this code object's powers of ten, one of the four kernels
// stamped at the end of mh_artic_contacts.inc by the stabiliser and the drive, the launch.  Every check is the router's
#ifdef MH_ARTIC_POSE_TU
#define MH_GEOM_LAUNCHER_(fam) artic_##fam##_pose_launch
#define MH_GEOM_POSE_PTR , ab->d_pose
#else
#define MH_GEOM_LAUNCHER_(fam) artic_##fam##_launch
#define MH_GEOM_POSE_PTR
#endif
#define MH_GEOM_LAUNCHER(fam) MH_GEOM_LAUNCHER_(fam)
#ifdef MH_ARTIC_WRENCH_TU
#define MH_GEOM_REPORT_PTR , report, wv
MH_ARTIC_WRENCH_LAUNCHER(MH_GEOM_LAUNCHER(MH_ARTIC_GEOM))
#elif defined(MH_ARTIC_REPORT_TU)
#define MH_GEOM_REPORT_PTR , report
MH_ARTIC_REPORT_LAUNCHER(MH_GEOM_LAUNCHER(MH_ARTIC_GEOM))
#else
#define MH_GEOM_REPORT_PTR
MH_ARTIC_LAUNCHER(MH_GEOM_LAUNCHER(MH_ARTIC_GEOM))
#endif
{
  namespace ar = mh::artic;
  if (init_pow10() != MH_OK) return MH_ERR_HIP;
  const ar::Model* M = ab->d_model;
  const size_t lds = ar::lds_bytes_contacts(ab->nj);
  const hipStream_t st = (hipStream_t)stream;
#ifdef MH_ARTIC_WRENCH_TU
  mh_artic_wrench wv; std::memset(&wv, 0, sizeof(wv)); if (W && W->terms != 0) wv = *W;      // by value, as the drive; terms 0 = the kernel's NULL
#endif
  if (D && D->terms != 0) hipLaunchKernelGGL(ab->cstab ? ar::MH_GEOM_KERNEL(_stab, _drive) : ar::MH_GEOM_KERNEL(, _drive), dim3(ab->B), dim3(64), lds, st,
                                             M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws MH_GEOM_POSE_PTR, *D MH_GEOM_REPORT_PTR);
  else hipLaunchKernelGGL(ab->cstab ? ar::MH_GEOM_KERNEL(_stab, ) : ar::MH_GEOM_KERNEL(, ), dim3(ab->B), dim3(64), lds, st,
                          M, ab->B, dt, nsteps, ab->d_q, ab->d_qd, ab->d_aux, ab->d_ws MH_GEOM_POSE_PTR MH_GEOM_REPORT_PTR);
  MH_HIP(hipGetLastError());
  return MH_OK;
}
#if defined(MH_ARTIC_PAIR_TU) && !defined(MH_ARTIC_BSP_TU) && !defined(MH_ARTIC_POSE_TU)
size_t artic_pair_lds_bytes(int nj) { return mh::artic::lds_bytes_contacts(nj); }
#endif
#if defined(MH_ARTIC_WRENCH_TU) && defined(MH_ARTIC_POSE_TU)
size_t artic_wr_pose_lds_bytes(int nj) { return mh::artic::lds_bytes_contacts(nj); }
#elif defined(MH_ARTIC_WRENCH_TU)
size_t artic_wr_lds_bytes(int nj) { return mh::artic::lds_bytes_contacts(nj); }
#elif defined(MH_ARTIC_PARAMS_TU)
// the per-world-parameters code objects: their image size, and the launches of their fwd_dyn / jacobian kernels
#ifdef MH_ARTIC_POSE_TU
#define MH_PW_NAME(stem) artic_pw_pose_##stem
#define MH_PW_KERNEL(name) name##_pw_pose
#define MH_PW_POSE_PTR , (const double*)ab->d_pose
#else
#define MH_PW_NAME(stem) artic_pw_##stem
#define MH_PW_KERNEL(name) name##_pw
#define MH_PW_POSE_PTR
#endif
size_t MH_PW_NAME(lds_bytes)(int nj) { return mh::artic::lds_bytes_contacts(nj); }
hipError_t MH_PW_NAME(fwd_dyn_launch)(mh_artic_batch* ab, void* stream, const double* d_tau, double* d_qdd, double* d_H, double* d_poses, int* d_ok)
{
  namespace ar = mh::artic;
  hipLaunchKernelGGL(ar::MH_PW_KERNEL(k_artic_fwd_dyn), dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)stream,
                     (const ar::Model*)ab->d_model, ab->B, (const double*)ab->d_q, (const double*)ab->d_qd, d_tau, d_qdd, d_H, d_poses, d_ok MH_PW_POSE_PTR);
  return hipGetLastError();
}
hipError_t MH_PW_NAME(jacobian_launch)(mh_artic_batch* ab, int link, const double* d_p, double* d_J)
{
  namespace ar = mh::artic;
  hipLaunchKernelGGL(ar::MH_PW_KERNEL(k_artic_jacobian), dim3(ab->B), dim3(64), ar::lds_bytes(ab->nj), (hipStream_t)nullptr,
                     (const ar::Model*)ab->d_model, ab->B, (const double*)ab->d_q, link, d_p, d_J MH_PW_POSE_PTR);
  return hipGetLastError();
}
#elif defined(MH_ARTIC_REPORT_TU) && defined(MH_ARTIC_POSE_TU)
size_t artic_rp_pose_lds_bytes(int nj) { return mh::artic::lds_bytes_contacts(nj); }
#elif defined(MH_ARTIC_REPORT_TU)
size_t artic_rp_lds_bytes(int nj) { return mh::artic::lds_bytes_contacts(nj); }
#endif
#endif
