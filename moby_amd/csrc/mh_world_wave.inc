// One Moby world per wavefront: TimeSteppingSimulator::step and everything it drives, for scenes of
// free rigid bodies (spheres, boxes against the plane, rimless-wheel spokes) + one static plane (with MHW_STATICS: + up to 8 static planes and boxes).
//
// Replaces (per world; same results as the CPU oracle oracle/world.hpp, which restates these
// reference functions statement by statement):
//   TimeSteppingSimulator::step / do_mini_step / calc_next_CA_Euler_step
//                                   src/TimeSteppingSimulator.cpp:52-111,114-222,272-331
//   CCD::broad_phase, calc_CA_Euler_step*, calc_max_dist, find_contacts_sphere_*, find_contacts_plane_generic,
//   calc_next_CA_Euler_step_generic / _polyhedron_plane
//                                   src/CCD.cpp:122-235,238-468,585-609,702-876; include/Moby/CCD.inl:804-886,1164-1207
//   BladePlanePlugin (rimless wheel)  example/rimless-wheel/coldet-plugin.cpp:53-288
//   ConstraintSimulator::calc_pairwise_distances / find_unilateral_constraints /
//   calc_impacting_unilateral_constraint_forces   src/ConstraintSimulator.cpp:298-355,450-537
//   UnilateralConstraint::determine_connected_constraints / remove_inactive_groups
//                                   src/UnilateralConstraint.cpp:940-1225
//   ImpactConstraintHandler::apply_model_to_connected_constraints, apply_no_slip_model[_to_connected_constraints],
//   compute_problem_data, update_from_stacked, update_constraint_velocities_from_impulses, apply_restitution
//                                   src/ImpactConstraintHandler.cpp:236-626,1009-1417,1590-2166
//   ImpactConstraintHandler::solve_qp_work / setup_QP   src/ImpactConstraintHandlerQP.cpp:94-497
//   ConstraintStabilization::stabilize / compute_problem_data / determine_dq /
//   update_q / ridders_unilateral   src/ConstraintStabilization.cpp:167-254,347-492,932-970,1056-1216,1322-1379
//
// MI355X mapping
//   * the wave's 64 lanes are, phase by phase, BODY lanes (state integration, inverse inertias), PAIR lanes
//     (swept-bounds overlap, signed distance, conservative-advancement time, contact generation -- compacted
//     with ballot/popcount), CONTACT lanes, JACOBIAN-ROW lanes (rows [d, r x d], X J^T), G-ENTRY lanes (one
//     entry of C X C' each) and LCP-VARIABLE lanes (mh_lcp_wave.h); per-world control flow (mini-step loop,
//     islands, restitution, Ridders, backtracking) is wave-uniform and runs on scalar masks;
//   * the WHOLE world -- body state, contacts, Jacobian rows, G = C X C', the handlers' _z/_zlast/_v, the
//     rand() ring, the scene constants and every scalar of the stepper -- lives in one LDS image (9.2 KB for
//     the small variant => 16 worlds per CU); nothing persistent is held in registers, the 42x42 LCP matrix
//     is never materialised (WorldMat), the LU block aliases the dead Jacobian rows;
//   * what one phase hands to the NEXT one of the same call chain is a value, not a word of the image: the pair count (broad_phase -> do_mini_step ->
//     find_unilateral_constraints), the contact count (-> handle_impacts, report_fold, the island search), the island search's masks and each island's
//     body and contact sets (islands_begin -> next_island -> the handlers: IslandSearch, Island), the matrix norm (compute_problem_data -> the LCP
//     chain) and the polygon offsets (poly_index -> WorldMat).  The words of the image that are still mailboxes are listed at the I_* enum below;
//   * routines with several call sites are single out-of-line device functions over that image, single-site
//     ones and the LCP chain are inlined: fully inlined the kernel is 31 K instructions and instruction-fetch
//     bound, fully out-of-line it drowns in callee-saved register traffic;
//   * HBM is touched only to load the state once and to store it (and the optional trajectory), plus the LU
//     workspace of the rare factorisations that do not fit LDS: all `nsteps` steps run inside one launch.
//
// This file is compiled once per variant: the includer defines MHW_BASE (its base name: the namespace mh::MHW_NS and the host-side getter at the end of this
// file, mh_world_variant_<MHW_NS>, are derived from it below), MHW_NB, MHW_MAX_PAIRS, MHW_MAX_CONTACTS, MHW_MAX_ROWS, MHW_MAX_GROWS, MHW_WAVES_PER_SIMD and the
// feature switches MHW_NOSLIP (no-slip model + spokes geometry) and MHW_BOX (box-plane contacts).  More switches are 1 in the units named and undefined = 0
// elsewhere:
//   MHW_FORCES  (mh_world_*_forces.hip, which define MH_FORCES_BUILD: set below) adds the scene's recurrent forces and the caller's wrench to the forward
//               dynamics; every line it adds sits under #if MHW_FORCES.
//   MHW_BSP     (mh_world_large_bsp*.hip, mh_world_large_st*.hip; needs MHW_BOX) adds box-sphere contacts between two free bodies (include/moby_hip.h,
//               "box-sphere pairs").
//   MHW_STATICS (mh_world_large_st*.hip; needs MHW_BSP) adds several static bodies -- planes and boxes, each with a frame of its own -- beside the free
//               bodies (include/moby_hip.h, "static bodies").
//   MHW_PARAMS  (mh_world_large_pw*.hip; needs MHW_STATICS) takes every VALUE of the scene -- masses, inertias, shapes, gravity, the ground frame, contact
//               parameters, the statics' frames and sizes -- from the world's own mh_world_params record instead of the shared scene and statics records
//               (include/moby_hip.h, "per-world parameters").  The topology (counts, types, enabled pairs, cone edges, tolerances) stays the scene's.
//   MHW_REPORT  (mh_world_large_rp*.hip; needs MHW_PARAMS) adds the per-pair contact impulse report (include/moby_hip.h, "Contact report"): one trailing kernel
//               argument, the report rows (or NULL: nothing is written, the steps are the same).  Every line it adds sits under #if MHW_REPORT: the
//               per-contact accumulators g_racc (cleared when the simulator's constraint list is built, added to by apply_impulses(.., 3)) and the fold of
//               a mini-step's contacts into the step's rows after handle_impacts (report_fold).
// The geometry that mirrors the reference is written ONCE for all builds.  A plane is always named by its body index; the builds differ in a few small
// accessors only, and these are all the MHW_BSP / MHW_STATICS conditionals of the file:
//   MHW_STATICS  the gs / gst tables (declaration; filled in the kernel entry, with ntot); plane_R / plane_o / plane_body; is_ground / is_sbox (is_sbox is
//                `false` without); the table arm of box_frame; the static-box arm of bounds()
//   MHW_BSP      the box-sphere section itself (is_sphere ... bsp_sdist) and its two call sites in pair_geom and contact_geom_body; box_plane_pair; the
//                box-box arm of broad_phase (without MHW_BSP a box-sphere pair is not kept either)
//   MHW_PARAMS   in the kernel entry only: `pv`, the record the cache fill reads its values from (the world's mh_world_params, or the scene itself), and
//                MHW_ST_R / MHW_ST_O / MHW_ST_DIM, the statics' values (the world's st_* rows, or the shared statics record).  The fill under them is
//                written once; nothing after the fill reads global scene memory, so there is no other conditional and no LDS of its own.
// A feature that changes this file keeps the INSTRUCTIONS of the builds it does not concern, not their text: tools/world_asm_diff.py compares every world
// code object of two source trees function by function (DESIGN.md 4.1).
#include "mh_world_common.h"

// the build's names from its base name: <base>_prof (MH_PROFILE_BUILD: the stamped object), <base>_forces (MH_FORCES_BUILD) or <base>
#define MHW_CAT_(a, b) a##b
#define MHW_CAT(a, b) MHW_CAT_(a, b)
#if defined(MH_PROFILE_BUILD)
#define MHW_NS MHW_CAT(MHW_BASE, _prof)
#elif defined(MH_FORCES_BUILD)
#define MHW_NS MHW_CAT(MHW_BASE, _forces)
#define MHW_FORCES 1
#else
#define MHW_NS MHW_BASE
#endif
#define MHW_VARIANT_GETTER MHW_CAT(mh_world_variant_, MHW_NS)

#define MHW_NS_MAXC ((MHW_MAX_CONTACTS < 6) ? MHW_MAX_CONTACTS : 6)   /* contacts of a no-slip island */
/* edge of the LDS-resident LU block: the largest square inside the 12 * MHW_MAX_ROWS doubles of D_J */
#define MHW_KA_V ((12 * MHW_MAX_ROWS >= 256) ? 16 : 12)
#define MHW_NS_MAXM (2 * MHW_NS_MAXC)

namespace mh { namespace MHW_NS {

// ---- the LDS image -------------------------------------------------------------------
enum {
  D_ST = 0,                                  // 13 per body: x(3) quat xyzw(4) v(3) omega(3)
  D_QSAVE = D_ST + 13 * MHW_NB,              // do_mini_step's qsave
  D_VSAVE = D_QSAVE + 7 * MHW_NB,            // stabilisation: saved velocities
  D_QV = D_VSAVE + 6 * MHW_NB,               // stabilisation: q
  D_DQV = D_QV + 7 * MHW_NB,                 // stabilisation: dq
  D_XINV = D_DQV + 7 * MHW_NB,               // per body: 1/m, inverse world inertia (9)
  D_XQ = D_XINV + 10 * MHW_NB,               // the quaternion D_XINV was computed for (the X block depends on nothing else)
  D_JW = D_XQ + 4 * MHW_NB,                  // world inertia R J R' of the same quaternion (forward dynamics)
  D_CPT = D_JW + 9 * MHW_NB,                 // contacts: point, normal, tangents
  D_CNR = D_CPT + 3 * MHW_MAX_CONTACTS,
  D_CS1 = D_CNR + 3 * MHW_MAX_CONTACTS,
  D_CS2 = D_CS1 + 3 * MHW_MAX_CONTACTS,
  D_CDIST = D_CS2 + 3 * MHW_MAX_CONTACTS,
  D_CMU = D_CDIST + MHW_MAX_CONTACTS,
  D_CMUV = D_CMU + MHW_MAX_CONTACTS,
  D_CEPS = D_CMUV + MHW_MAX_CONTACTS,
  D_CCOMP = D_CEPS + MHW_MAX_CONTACTS,
  D_J = D_CCOMP + MHW_MAX_CONTACTS,          // Jacobian rows: 2 blocks x 6
  D_XJ = D_J + 12 * MHW_MAX_ROWS,            // X * row^T per block
  D_G = D_XJ + 12 * MHW_MAX_ROWS,            // C X C' (rows x rows)
  D_CV = D_G + MHW_MAX_GROWS * MHW_MAX_GROWS,
  D_IMP = D_CV + MHW_MAX_ROWS,
  D_A = D_J,                                 // LU block MHW_KA_V x MHW_KA_V: ALIASES the Jacobian rows, which are dead once
                                             //  G = C X C' is built (the solvers only read G, C v and the contact parameters)
  D_ART = D_IMP + MHW_MAX_ROWS,              // Lemke's artificial column
  D_ZLAST = D_ART + 64,                      // ImpactConstraintHandler::_zlast
  D_ZBUF = D_ZLAST + 64,                     // storage of ImpactConstraintHandler::_z (= the last solution,
  D_ZSOL = D_ZBUF,                           //  repacked / restitution-scaled in place, ICH-QP:244, ICH:477)
  D_RADIUS = D_ZBUF + 64,                    // scene cache
  D_RMAX = D_RADIUS + MHW_NB,               // CCD::_rmax (farthest point distance)
  D_GDIM = D_RMAX + MHW_NB,                  // box edge lengths
  D_MASS = D_GDIM + (MHW_BOX ? 3 * MHW_NB : 0),
  D_INERTIA = D_MASS + MHW_NB,
  D_PLANE_R = D_INERTIA + 3 * MHW_NB,
  D_PLANE_O = D_PLANE_R + 9,
  D_GRAV = D_PLANE_O + 3,
  D_PMU = D_GRAV + 3,
  D_PMUV = D_PMU + MHW_MAX_PAIRS,
  D_PEPS = D_PMUV + MHW_MAX_PAIRS,
  D_PCOMP = D_PEPS + MHW_MAX_PAIRS,
  D_MINSTEP = D_PCOMP + MHW_MAX_PAIRS,
  D_THRESH = D_MINSTEP + 1,
  D_CSTABEPS = D_THRESH + 1,
  D_TIME = D_CSTABEPS + 1,
  // no-slip model / spokes geometry (variants built with MHW_NOSLIP only)
  D_SPK = D_TIME + 1,                        // spoke tips (x, z) in the wheel frame, host libm
  D_VNS = D_SPK + (MHW_NOSLIP ? 2 * MH_MAX_SPOKES : 0),      // ImpactConstraintHandler::_v
  D_NSY = D_VNS + (MHW_NOSLIP ? MH_NOSLIP_MAX : 0),          // Y = [S X S' S X T'; . T X T'] / its Cholesky factor
  D_NSQX = D_NSY + (MHW_NOSLIP ? MHW_NS_MAXM * MHW_NS_MAXM : 0),
  D_NSW = D_NSQX + (MHW_NOSLIP ? MHW_NS_MAXC * MHW_NS_MAXM : 0),
  D_NSMM = D_NSW + (MHW_NOSLIP ? MHW_NS_MAXC * MHW_NS_MAXM : 0),
  D_NSQ = D_NSMM + (MHW_NOSLIP ? MHW_NS_MAXC * MHW_NS_MAXC : 0),
  D_NSYXV = D_NSQ + (MHW_NOSLIP ? MHW_NS_MAXC : 0),
  D_NST2 = D_NSYXV + (MHW_NOSLIP ? MHW_NS_MAXM : 0),
  D_END = D_NST2 + (MHW_NOSLIP ? MHW_NS_MAXM : 0)
};
enum {
  I_PAIRS = 0,                               // ConstraintSimulator::_pairs_to_check
  I_CG1 = I_PAIRS + MHW_MAX_PAIRS,
  I_CG2 = I_CG1 + MHW_MAX_CONTACTS,
  I_CPAIR = I_CG2 + MHW_MAX_CONTACTS,
  I_CNK = I_CPAIR + MHW_MAX_CONTACTS,
  I_ROWOFF = I_CNK + MHW_MAX_CONTACTS,
  I_ISLC = I_ROWOFF + 2 * MHW_MAX_ROWS,
  I_ISLB = I_ISLC + MHW_MAX_CONTACTS,
  I_KOFF = I_ISLB + MHW_NB,
  I_SCR = I_KOFF + MHW_MAX_CONTACTS + 1,     // BFS queue / CStab pair list
  I_RNG = I_SCR + 64,                        // glibc rand() ring (31 words + idx)
  I_PNK = I_RNG + 32,                        // scene cache: friction-cone-edges, enabled
  I_PEN = I_PNK + MHW_MAX_PAIRS,
  I_NB = I_PEN + MHW_MAX_PAIRS, I_NTOT, I_NPT, I_NMAX, I_KA, I_NPAIRS, I_NC, I_STATUS,
  I_ZLAST_SIZE, I_ZBUF_SIZE, I_ZBUF_CAP, I_NODEMASK, I_DONEMASK, I_DONEMASK_HI, I_CSTAB_MAXIT,
  I_NSPOKES, I_VNS_SIZE, I_NSM, I_NSNS,
  // Of the scalars above, the ones a phase hands to the next travel as values (return values, arguments, uniform registers), not through their word here:
  // the contact count and the island search's masks are never stored (I_NC, I_NODEMASK, I_DONEMASK, I_DONEMASK_HI keep their slots so that the image is
  // laid out as it was); I_NPAIRS is stored once per mini-step for the stabiliser (eval_unilateral, update_q), which reads it at the end of the step;
  // I_KOFF is filled for the polygon columns of islands of more than 7 contacts only (WorldMat::at_row).  What stays a mailbox: I_STATUS (read at the
  // launch's end and by world_step's entry test), the sizes of _z/_zlast/_v, and I_NSM / I_NSNS between noslip_setup and noslip_finish.
  I_GEOM,                                   // geometry type per body
  I_NSS = I_GEOM + MHW_NB,                   // no-slip S / T index sets
  I_NST = I_NSS + (MHW_NOSLIP ? MHW_NS_MAXC : 0),
  I_END = I_NST + (MHW_NOSLIP ? MHW_NS_MAXC : 0)
};
__shared__ double gd[D_END];
__shared__ int gi[I_END];
__shared__ double* g_lu_ws;                  // this world's HBM LU workspace (nmax x nmax)

enum { CN_STEPS = 0, CN_MINI, CN_LCP, CN_ROWS, CN_PIV, CN_STAB, CN_BYTES, CN_SROWS, CN_COUNT };
enum { PH_BROAD_CA = 0, PH_INTEGRATE, PH_FWDDYN, PH_CONTACTS, PH_ISLANDS, PH_PDATA, PH_MBUILD, PH_LCP, PH_APPLY, PH_STAB,
       PH_LP0, PH_COUNT = PH_LP0 + LP_COUNT };
__shared__ unsigned long long g_cnt[CN_COUNT];
__shared__ unsigned long long g_pacc[PH_COUNT];
#if MHW_FORCES
// Recurrent forces of the scene and the caller's wrench (include/moby_hip.h: mh_world_forces, mh_world_batch_step_wrench).  An image of its own beside
// gd, so that the plain variants' image is the text it was: 6 coefficients per body, cached at launch, and this step's wrench row, staged once per
// step (a step runs one to three mini-steps and each reads the row; one global read per step, issued before the step's broad phase, instead of one
// per mini-step in front of the forward dynamics that waits for it).  12 MHW_NB doubles: 384 bytes in the small variant, 16 worlds per CU kept.
enum { F_SB = 0, F_SBA = MHW_NB, F_KL = 2 * MHW_NB, F_KA = 3 * MHW_NB, F_KLSQ = 4 * MHW_NB, F_KASQ = 5 * MHW_NB, F_WR = 6 * MHW_NB, F_END = 12 * MHW_NB };
#define MHW_FORCE_WRENCH 0x100               /* g_fterms: a wrench row is staged (beside the MH_FORCE_* bits of the stored terms) */
__shared__ double gf[F_END];
__shared__ int g_fterms;
#endif

#if MHW_STATICS
// The static bodies of the scene (include/moby_hip.h: mh_world_statics), cached at launch in an image of its own beside gd, as gf is, so that gd's offsets
// stay where they were.  Slot s serves body nb + s: the scene's own ground (if any) is slot 0, from plane_R / plane_o; static k follows at has_ground + k.
// nb >= 1 and ntot <= MH_MAX_BODIES + 1 leave at most MH_MAX_STATICS slots.  Per slot: rotation (9, row-major), origin (3), box edge lengths (3) and the
// box's bounding radius (half diagonal, CCD.cpp:1056-1063): 16 MH_MAX_STATICS doubles + a type word each = 1056 bytes.
enum { S_R = 0, S_O = 9 * MH_MAX_STATICS, S_DIM = 12 * MH_MAX_STATICS, S_RAD = 15 * MH_MAX_STATICS, S_END = 16 * MH_MAX_STATICS };
__shared__ double gs[S_END];
__shared__ int gst[MH_MAX_STATICS];
#endif

#if MHW_REPORT
// The contact report (include/moby_hip.h, "Contact report").  g_racc: accumulated (cn, cs, ct) of every contact of the simulator's constraint list -- the
// reference's contact_impulse in the contact frame, oracle Contact::imp -- 3 MHW_MAX_CONTACTS doubles; g_rep: the rows of this world's current step in the
// caller's report (npt rows of MH_REPORT_PAIR doubles), or null.  The rows themselves stay in global memory: lane p owns row p, zeroes it at the step's start
// and adds to it once per mini-step, so no lane ever reads what another wrote.
__shared__ double g_racc[3 * MHW_MAX_CONTACTS];
__shared__ double* g_rep;
#endif

#define MHW_FN __device__ __noinline__
// (measured with tools/variants.sh: the impulse application / constraint-velocity update, the island search and
//  compute_problem_data are faster inlined, +1.8 %; apply_impulses, store_contact and broad_phase are not)

MH_DEV int geti(int i) { return uni(gi[i]); }
MH_DEV void seti(int i, int v) { if (lane_id() == 0) gi[i] = v; }
#ifdef MH_PROFILE_BUILD      /* (see lp_tick in mh_lcp_wave.h: the stamps exist in the profile translation units only) */
MH_DEV unsigned long long tick() { return g_lcp_prof_on ? __builtin_amdgcn_s_memtime() : 0ull; }
MH_DEV void tock(int ph, unsigned long long t0) { if (g_lcp_prof_on) { const unsigned long long d = __builtin_amdgcn_s_memtime() - t0; lds_add(&g_pacc[ph], d); } }
#else
MH_DEV unsigned long long tick() { return 0ull; }
MH_DEV void tock(int, unsigned long long) {}
#endif
// the counters of the aux record
MH_DEV void count(int c, unsigned long long v) { if (lane_id() == 0) g_cnt[c] += v; }
MH_DEV void account(int n, unsigned piv) {
  count(CN_LCP, 1ull); count(CN_ROWS, (unsigned long long)n); count(CN_PIV, piv); count(CN_BYTES, 8ull * ((unsigned long long)n * n + 2ull * n));
}

// ---- state helpers (any lane, any body) ---------------------------------------------------
MH_DEV bool enabled(int b) { return b < gi[I_NB]; }
MH_DEV V3 X(int b) { return v3(gd[D_ST + 13*b], gd[D_ST + 13*b+1], gd[D_ST + 13*b+2]); }
MH_DEV V3 Vl(int b) { return v3(gd[D_ST + 13*b+7], gd[D_ST + 13*b+8], gd[D_ST + 13*b+9]); }
MH_DEV V3 Wa(int b) { return v3(gd[D_ST + 13*b+10], gd[D_ST + 13*b+11], gd[D_ST + 13*b+12]); }
MH_DEV V3 point_vel(int b, V3 p) {
  if (!enabled(b)) return v3(0.0, 0.0, 0.0);
  return Vl(b) + cross(Wa(b), p - X(b));
}
MH_DEV void pair_bodies(int p, int& a, int& b) {
  const int ntot = gi[I_NTOT];
  int i = 0, rem = p;
  while (rem >= ntot - 1 - i) { rem -= ntot - 1 - i; i++; }
  a = i; b = i + 1 + rem;
}
// ---- the plane of a body-plane pair.  `pl` is the plane's body index (>= nb; the scene's ground is nb).  These three accessors hold the build switch; the
// geometry below them is written once.  With MHW_STATICS every static plane has a frame of its own in the gs table; without, there is one plane, the
// scene's ground, and `pl` is not looked at: plane_body is then gi[I_NB], not `pl`, so that enabled(plane_body(pl)) folds to false at compile time.
// (plane_body is a macro: as an inline function returning gi[I_NB] it moved the exec-mask code of ca_step in the large kernels, tools/world_asm_diff.py.) ----
#if MHW_STATICS
MH_DEV const double* plane_R(int pl) { return gs + S_R + 9 * (pl - gi[I_NB]); }
MH_DEV const double* plane_o(int pl) { return gs + S_O + 3 * (pl - gi[I_NB]); }
#define plane_body(pl) (pl)
#else
MH_DEV const double* plane_R(int) { return gd + D_PLANE_R; }
MH_DEV const double* plane_o(int) { return gd + D_PLANE_O; }
#define plane_body(pl) gi[I_NB]
#endif
MH_DEV V3 plane_n(int pl) { const double* R = plane_R(pl); return v3(R[1], R[4], R[7]); }
MH_DEV V3 to_plane(V3 p, int pl) {
  const double* R = plane_R(pl); const double* o = plane_o(pl); V3 d = p - v3(o[0], o[1], o[2]);
  return v3((R[0]*d.x + R[3]*d.y) + R[6]*d.z, (R[1]*d.x + R[4]*d.y) + R[7]*d.z, (R[2]*d.x + R[5]*d.y) + R[8]*d.z);
}
MH_DEV V3 from_plane(V3 p, int pl) {
  const double* R = plane_R(pl); const double* o = plane_o(pl);
  return v3(o[0] + ((R[0]*p.x + R[1]*p.y) + R[2]*p.z),
            o[1] + ((R[3]*p.x + R[4]*p.y) + R[5]*p.z),
            o[2] + ((R[6]*p.x + R[7]*p.y) + R[8]*p.z));
}
MH_DEV void orthonormal_basis(V3 n, V3& s, V3& t) {
  const double ax = fabs(n.x), ay = fabs(n.y), az = fabs(n.z);
  V3 e;
  if (ax <= ay && ax <= az) e = v3(1.0, 0.0, 0.0); else if (ay <= az) e = v3(0.0, 1.0, 0.0); else e = v3(0.0, 0.0, 1.0);
  s = cross(n, e); s = s / norm(s);
  t = cross(n, s);
}

MH_DEV void rot(int b, double R[9]) {
  const double x = gd[D_ST + 13*b+3], y = gd[D_ST + 13*b+4], z = gd[D_ST + 13*b+5], w = gd[D_ST + 13*b+6];
  R[0] = 1.0 - 2.0 * (y*y + z*z); R[1] = 2.0 * (x*y - z*w);       R[2] = 2.0 * (x*z + y*w);
  R[3] = 2.0 * (x*y + z*w);       R[4] = 1.0 - 2.0 * (x*x + z*z); R[5] = 2.0 * (y*z - x*w);
  R[6] = 2.0 * (x*z - y*w);       R[7] = 2.0 * (y*z + x*w);       R[8] = 1.0 - 2.0 * (x*x + y*y);
}
// rimless-wheel spokes (example/rimless-wheel/coldet-plugin.cpp): geometry type and tips
MH_DEV bool is_spokes(int b) {
#if MHW_NOSLIP
  return b < gi[I_NB] && gi[I_GEOM + b] == MH_GEOM_SPOKES;
#else
  (void)b; return false;
#endif
}
#if MHW_NOSLIP
MH_DEV V3 spoke_tip_at(const double R[9], V3 c, int i) {           // coldet-plugin.cpp:104-113
  const double px = gd[D_SPK + 2*i], py = 0.0, pz = gd[D_SPK + 2*i + 1];
  return v3(c.x + ((R[0]*px + R[1]*py) + R[2]*pz), c.y + ((R[3]*px + R[4]*py) + R[5]*pz), c.z + ((R[6]*px + R[7]*py) + R[8]*pz));
}
MH_DEV V3 spoke_tip(int b, int i) { double R[9]; rot(b, R); return spoke_tip_at(R, X(b), i); }
#endif

MH_DEV bool is_box(int b) {
#if MHW_BOX
  return b < gi[I_NB] && gi[I_GEOM + b] == MH_GEOM_BOX;
#else
  (void)b; return false;
#endif
}
#if MHW_BOX
// BoxPrimitive::get_vertices order (BoxPrimitive.cpp:358-365): vertex i in the box frame / global frame
MH_DEV V3 box_corner(int b, int i) {
  const double hx = gd[D_GDIM + 3*b] * 0.5, hy = gd[D_GDIM + 3*b + 1] * 0.5, hz = gd[D_GDIM + 3*b + 2] * 0.5;
  return v3((i & 4) ? -hx : hx, (i & 2) ? -hy : hy, (i & 1) ? -hz : hz);
}
MH_DEV V3 box_vertex(int b, int i) {
  const V3 p = box_corner(b, i);
  double R[9]; rot(b, R);
  const V3 c = X(b);
  return v3(c.x + ((R[0]*p.x + R[1]*p.y) + R[2]*p.z), c.y + ((R[3]*p.x + R[4]*p.y) + R[5]*p.z), c.z + ((R[6]*p.x + R[7]*p.y) + R[8]*p.z));
}
// find_contacts_plane_generic(plane, box) (CCD.inl:848-886): bit i set <=> vertex i is within TOL (<=) of the plane
MH_DEV unsigned box_contact_mask(int b, double TOL, int pl) {
  unsigned m = 0;
  for (int i = 0; i < 8; i++) { const V3 pp = to_plane(box_vertex(b, i), pl); if (pp.y <= TOL) m |= 1u << i; }
  return m;
}
MH_DEV bool rel_equal(double x, double y) {                         // CompGeom.h:110
  const double ax = fabs(x), ay = fabs(y);
  const double m1 = (ay > 1.0) ? ay : 1.0; const double m = (ax > m1) ? ax : m1;
  return fabs(x - y) <= MH_NEAR_ZERO * m;
}
MH_DEV bool collinear(V3 a, V3 b, V3 c) {                           // CompGeom.cpp:1923-1931
  return rel_equal((c.z-a.z)*(b.y-a.y), (b.z-a.z)*(c.y-a.y)) && rel_equal((b.z-a.z)*(c.x-a.x), (b.x-a.x)*(c.z-a.z)) &&
         rel_equal((b.x-a.x)*(c.y-a.y), (b.y-a.y)*(c.x-a.x));
}
#endif
#if MHW_BSP
// ---- box-sphere pairs of two free bodies (include/moby_hip.h).  The box is the reference's geometry A whichever body has the lower id; the frames are
// the bodies' own (box centre = COM, box axes = rot(box)), a static box's its table row (box_frame).  Operation order = tests/native/world_ref.cpp (= artic_boxsphere_ref.cpp):
// three-term sums as (a + b) + c.  Each function forms the box rotation once. ----
MH_DEV bool is_sphere(int b) { return b < gi[I_NB] && gi[I_GEOM + b] == MH_GEOM_SPHERE; }
#if MHW_STATICS
MH_DEV bool is_static(int b, int type) { const int s = b - gi[I_NB]; return s >= 0 && s < MH_MAX_STATICS && b < gi[I_NTOT] && gst[s] == type; }
MH_DEV bool is_ground(int b) { return is_static(b, MH_STATIC_PLANE); }                 // "a static plane": the scene's ground or any other
MH_DEV bool is_sbox(int b) { return is_static(b, MH_STATIC_BOX); }
#else
MH_DEV bool is_ground(int b) { return b == gi[I_NB]; }
MH_DEV bool is_sbox(int) { return false; }
#endif
MH_DEV bool bsp_pair(int a, int b, int& bx, int& sp) {
  if (is_box(a) && is_sphere(b)) { bx = a; sp = b; return true; }
  if (is_sphere(a) && (is_box(b) || is_sbox(b))) { bx = b; sp = a; return true; }       // (a static has the higher index: it is never a)
  return false;
}
// rotation, centre and half lengths of box bx: a body's own frame, or a static box's from the table
MH_DEV void box_frame(int bx, double R[9], V3& cb, V3& h) {
#if MHW_STATICS
  if (bx >= gi[I_NB]) {
    const int s = bx - gi[I_NB];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = gs[S_R + 9*s + k];
    cb = v3(gs[S_O + 3*s], gs[S_O + 3*s + 1], gs[S_O + 3*s + 2]);
    h = v3(gs[S_DIM + 3*s] * 0.5, gs[S_DIM + 3*s + 1] * 0.5, gs[S_DIM + 3*s + 2] * 0.5);
    return;
  }
#endif
  rot(bx, R); cb = X(bx);
  h = v3(gd[D_GDIM + 3*bx] * 0.5, gd[D_GDIM + 3*bx + 1] * 0.5, gd[D_GDIM + 3*bx + 2] * 0.5);
}
MH_DEV V3 mat_v(const double R[9], V3 p) { return v3((R[0]*p.x + R[1]*p.y) + R[2]*p.z, (R[3]*p.x + R[4]*p.y) + R[5]*p.z, (R[6]*p.x + R[7]*p.y) + R[8]*p.z); }
MH_DEV V3 matT_v(const double R[9], V3 p) { return v3((R[0]*p.x + R[3]*p.y) + R[6]*p.z, (R[1]*p.x + R[4]*p.y) + R[7]*p.z, (R[2]*p.x + R[5]*p.y) + R[8]*p.z); }
MH_DEV double clampd(double c, double h) { return (c < -h) ? -h : ((c > h) ? h : c); }
// BoxPrimitive::calc_closest_points (BoxPrimitive.cpp:183-254; the QP's fixed point is the clamp) + find_contacts_box_sphere (CCD.inl:1208-1259)
MH_DEV int bsp_contact(int bx, int sp, double TOL, V3& pt, V3& n, double& dist) {
  double R[9]; V3 cb, h; box_frame(bx, R, cb, h);
  const V3 cS = X(sp);
  const V3 c = matT_v(R, cS - cb);
  const double Rs = gd[D_RADIUS + sp];
  const V3 p = v3(clampd(c.x, h.x), clampd(c.y, h.y), clampd(c.z, h.z));
  V3 u = p - c;
  const double nrm = norm(u);
  if (fabs(p.x) < h.x || fabs(p.y) < h.y || fabs(p.z) < h.z || nrm < Rs) {             // an OR: every face and edge region, and every penetration
    const double b1 = h.y - fabs(p.y), b2 = h.z - fabs(p.z);
    const double b12 = (b2 < b1) ? b2 : b1, b0 = h.x - fabs(p.x);
    const double bd = (b12 < b0) ? b12 : b0;
    const double rn = Rs - nrm;
    dist = -((rn < bd) ? rn : bd);
  } else {                                                                             // a vertex region: the sphere point goes to the surface
    u = u * (Rs / nrm);
    dist = norm((c + u) - p);
  }
  if (dist > TOL) return 0;
  const V3 ug = mat_v(R, u);
  const V3 sg = cS + ug;
  bool own = false;
  if (dist > 0.0) {
    const V3 pg = cb + mat_v(R, p);
    const V3 nd = pg - sg;
    const double nl = norm(nd);
    pt = (sg + pg) * 0.5;
    if (nl > MH_NEAR_ZERO) { n = nd / nl; own = true; }
  } else pt = sg;
  if (!own) n = ug / norm(ug);                                                         // (a centre inside the box: 0 / 0, as in the reference)
  return 1;
}
// BoxPrimitive::calc_signed_dist for a sphere (BoxPrimitive.cpp:256-276, 788-836): pA the box point, pB the sphere point
MH_DEV double bsp_sdist(int bx, int sp, V3& pA, V3& pB) {
  double R[9]; V3 cb, hv; box_frame(bx, R, cb, hv);
  const V3 cS = X(sp);
  const V3 cv = matT_v(R, cS - cb);
  const double c[3] = { cv.x, cv.y, cv.z };
  const double h[3] = { hv.x, hv.y, hv.z };
  const double Rs = gd[D_RADIUS + sp];
  double cl[3] = { c[0], c[1], c[2] };
  bool inside = true; double sq = 0.0, in = -MHW_INF;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if (c[i] < -h[i]) { const double dl = c[i] + h[i]; cl[i] = -h[i]; sq = sq + dl * dl; inside = false; }
    else if (c[i] > h[i]) { const double dl = c[i] - h[i]; cl[i] = h[i]; sq = sq + dl * dl; inside = false; }
    else if (inside) { const double f1 = fabs(h[i] - c[i]), f2 = fabs(c[i] + h[i]); const double dd = -((f2 < f1) ? f2 : f1); in = (in < dd) ? dd : in; }
  }
  const double dist = (inside ? in : sqrt(sq)) - Rs;
  const V3 v = v3(cl[0] - c[0], cl[1] - c[1], cl[2] - c[2]);
  const double vn = norm(v);
  pA = cb + mat_v(R, v3(cl[0], cl[1], cl[2]));
  if (vn == 0.0) pB = cS;
  else pB = cS + mat_v(R, v) * ((Rs + ((0.0 < dist) ? 0.0 : dist)) / vn);
  return dist;
}
#endif
// "box against a plane" (PlanePrimitive's and CCD's polyhedron-plane paths); with MHW_BSP a box-sphere pair follows the sphere rules instead.  Without it a
// box body's only kept partner is the ground (broad_phase).  (A macro: as an inline function its && reached gen_contacts as a value and the statics
// build's gen_contacts came out 8 bytes longer, tools/world_asm_diff.py.)
#if MHW_BSP
#define box_plane_pair(a, b) (is_box(a) && is_ground(b))
#else
#define box_plane_pair(a, b) is_box(a)
#endif

// ---- pair-lane geometry ---------------------------------------------------------------------
// swept bounds of body b (BoundingSphere.cpp:71-95, SSL.cpp:550-579, DummyBV.h:53-56)
MH_DEV void bounds(int b, double dt, V3& lo, V3& hi) {
#if MHW_STATICS
  if (is_sbox(b)) {                                                  // a static box: its bounding sphere, which does not move (CCD.cpp:735-768 rebuilds enabled bodies' only)
    const int s = b - gi[I_NB];
    const V3 c = v3(gs[S_O + 3*s], gs[S_O + 3*s + 1], gs[S_O + 3*s + 2]); const double r = gs[S_RAD + s];
    lo = v3(c.x - r, c.y - r, c.z - r); hi = v3(c.x + r, c.y + r, c.z + r); return;
  }
#endif
  if (!enabled(b)) { lo = v3(-MHW_INF, -MHW_INF, -MHW_INF); hi = v3(MHW_INF, MHW_INF, MHW_INF); return; }
  const V3 c = X(b);
  const V3 vdt = Vl(b) * dt, wdt = Wa(b) * dt;
  const V3 lin = vdt + cross(c, wdt);
  const V3 p2 = c + lin;
  const double r = gd[D_RADIUS + b];
  lo = v3(((c.x < p2.x) ? c.x : p2.x) - r, ((c.y < p2.y) ? c.y : p2.y) - r, ((c.z < p2.z) ? c.z : p2.z) - r);
  hi = v3(((c.x > p2.x) ? c.x : p2.x) + r, ((c.y > p2.y) ? c.y : p2.y) + r, ((c.z > p2.z) ? c.z : p2.z) + r);
}
// CCD::broad_phase (CCD.cpp:702-876): compacted pair list into gi[out_off..]; returns its length
MHW_FN int broad_phase(double dt, int out_off) {
  const int lane = lane_id();
  bool keep = false, spk = false;
  if (lane < gi[I_NPT]) {
    int a, b; pair_bodies(lane, a, b);
    if (is_spokes(a) || is_spokes(b)) {
      // the wheel is removed from CCD's body list and (ground, wheel) is appended unconditionally,
      // after CCD's pairs (coldet-plugin.cpp:53-74)
      spk = true; keep = is_spokes(a) && b == gi[I_NB];
#if MHW_BSP
    } else if (is_box(a) && (is_box(b) || is_sbox(b))) {
      keep = false;                                                 // box-box, a static box included: rejected at create unless disabled (box-sphere: swept bounds, below)
#else
    } else if ((is_box(a) || is_box(b)) && b != gi[I_NB]) {
      keep = false;                                                 // box-box / box-sphere: rejected by check_scene unless disabled
#endif
    } else {
      V3 loa, hia, lob, hib; bounds(a, dt, loa, hia); bounds(b, dt, lob, hib);
      keep = (loa.x <= hib.x && lob.x <= hia.x) && (loa.y <= hib.y && lob.y <= hia.y) && (loa.z <= hib.z && lob.z <= hia.z);
      keep = keep && (gi[I_PEN + lane] != 0) && (enabled(a) || enabled(b));
    }
  }
  const uint64_t m = ballot(keep && !spk);
  const uint64_t ms = ballot(keep && spk);
  wave_sync();
  if (keep) gi[out_off + (spk ? popc(m) + popc(ms & lanes_below(lane)) : popc(m & lanes_below(lane)))] = lane;
  wave_sync();
  return popc(m) + popc(ms);
}
// signed distance + closest points of pair p (SpherePrimitive.cpp:104-136, PlanePrimitive.cpp:385-411)
struct PairGeom { double dist; V3 pa, pb; int a, b; };
MHW_FN PairGeom pair_geom(int p) {
  PairGeom g; pair_bodies(p, g.a, g.b);
#if MHW_NOSLIP
  if (is_spokes(g.a)) {
    // calc_signed_dist_wheel_plane (coldet-plugin.cpp:88-137); the plugin returns pA = wheel point,
    // pB = ground point for the pair (ground, wheel)
    const int w = g.a, N = gi[I_NSPOKES];
    double min_dist = MHW_INF;
    g.pa = v3(0.0, 0.0, 0.0); g.pb = v3(0.0, 0.0, 0.0);
    double Rw[9]; rot(w, Rw);
    const V3 cw = X(w);
    for (int i = 0; i < N; i++) {
      const V3 tip = spoke_tip_at(Rw, cw, i);
      const V3 pp = to_plane(tip, gi[I_NB]);
      if (pp.y < min_dist) { min_dist = pp.y; g.pb = from_plane(v3(pp.x, 0.0, pp.z), gi[I_NB]); g.pa = tip; }
    }
    g.dist = min_dist; g.a = gi[I_NB]; g.b = w;
    return g;
  }
#endif
#if MHW_BSP
  { int bx, sp;
    if (bsp_pair(g.a, g.b, bx, sp)) {
      // a sphere as A forwards to the box with the point arguments swapped (SpherePrimitive.cpp:282-290): the points stay with their bodies
      V3 pbox, psph; g.dist = bsp_sdist(bx, sp, pbox, psph);
      if (bx == g.a) { g.pa = pbox; g.pb = psph; } else { g.pa = psph; g.pb = pbox; }
      return g;
    } }
#endif
#if MHW_BOX
  if (is_box(g.a)) {
    // PlanePrimitive::calc_signed_dist(polyhedral) (PlanePrimitive.cpp:338-376): lowest vertex, first wins ties
    double min_dist = MHW_INF;
    g.pa = v3(0.0, 0.0, 0.0); g.pb = v3(0.0, 0.0, 0.0);
    for (int i = 0; i < 8; i++) {
      const V3 vtx = box_vertex(g.a, i);
      const V3 pp = to_plane(vtx, g.b);                             // (a box body's partner here is a plane: box-sphere went above, box-box is never kept)
      if (pp.y < min_dist) { min_dist = pp.y; g.pa = vtx; g.pb = from_plane(v3(pp.x, 0.0, pp.z), g.b); }
    }
    g.dist = min_dist;
    return g;
  }
#endif
  if (enabled(g.a) && enabled(g.b)) {
    const V3 ca = X(g.a), cb = X(g.b);
    const double ra = gd[D_RADIUS + g.a], rb = gd[D_RADIUS + g.b];
    const V3 ab = cb - ca;
    const double len = norm(ab);
    const double d = len - ra - rb;
    const V3 u = ab / len;
    const double sa = (d > 0.0) ? ra : ra + d, sb = (d > 0.0) ? rb : rb + d;
    g.pa = ca + u * sa; g.pb = cb - u * sb; g.dist = d;
    return g;
  }
  const int s = enabled(g.a) ? g.a : g.b, pl = enabled(g.a) ? g.b : g.a;
  const V3 cp = to_plane(X(s), pl);
  const double r = gd[D_RADIUS + s];
  const double low = cp.y + (-1.0 * r);
  const V3 on_plane = from_plane(v3(cp.x, 0.0, cp.z), pl);
  const V3 on_sphere = from_plane(v3(cp.x, low, cp.z), pl);
  if (s == g.a) { g.pa = on_sphere; g.pb = on_plane; } else { g.pa = on_plane; g.pb = on_sphere; }
  g.dist = low;
  return g;
}
// contact of pair p if within TOL (CCD.inl:804-847, 1164-1207)
struct ContactGeom { int has, g1, g2; V3 pt, n; double dist; };
// (the out-of-line body returns has/g1/g2 packed in one word: 15 dwords come back in registers, 17 went
//  through a scratch-memory return slot -- 13 scratch stores + reloads per call)
struct ContactGeomPacked { int code; V3 pt, n; double dist; };
MH_DEV ContactGeom contact_geom_body(int p, double TOL);
MHW_FN ContactGeomPacked contact_geom_packed(int p, double TOL) {
  const ContactGeom c = contact_geom_body(p, TOL);
  ContactGeomPacked q; q.code = c.has | (c.g1 << 8) | (c.g2 << 16); q.pt = c.pt; q.n = c.n; q.dist = c.dist;
  return q;
}
MH_DEV ContactGeom contact_geom(int p, double TOL) {
  const ContactGeomPacked q = contact_geom_packed(p, TOL);
  ContactGeom c; c.has = q.code & 0xff; c.g1 = (q.code >> 8) & 0xff; c.g2 = (q.code >> 16) & 0xff; c.pt = q.pt; c.n = q.n; c.dist = q.dist;
  return c;
}
MH_DEV ContactGeom contact_geom_body(int p, double TOL) {
  ContactGeom c; c.has = 0; c.g1 = 0; c.g2 = 0; c.pt = v3(0.0, 0.0, 0.0); c.n = v3(0.0, 0.0, 0.0); c.dist = 0.0;
  int a, b; pair_bodies(p, a, b);
#if MHW_BSP
  { int bx, sp;
    if (bsp_pair(a, b, bx, sp)) {                                   // created as (box, sphere): the normal points from the sphere towards the box
      c.has = bsp_contact(bx, sp, TOL, c.pt, c.n, c.dist); c.g1 = bx; c.g2 = sp;
      return c;
    } }
#endif
  if (enabled(a) && enabled(b)) {
    const V3 cA = X(a), cB = X(b);
    const double rA = gd[D_RADIUS + a], rB = gd[D_RADIUS + b];
    const V3 d = cA - cB;
    const double len = norm(d);
    c.dist = len - rA - rB;
    if (c.dist > TOL) return c;
    c.n = d / len;
    const V3 closest_A = cA - c.n * rA, closest_B = cB + c.n * rB;
    c.pt = (closest_A + closest_B) * 0.5;
    c.g1 = a; c.g2 = b; c.has = 1;
    return c;
  }
  const int s = enabled(a) ? a : b, pl = enabled(a) ? b : a;
  const V3 cp = to_plane(X(s), pl);
  const double r = gd[D_RADIUS + s];
  c.dist = cp.y - r;
  if (c.dist > TOL) return c;
  c.pt = from_plane(v3(cp.x, 0.5 * (cp.y - r), cp.z), pl);
  c.n = plane_n(pl); c.g1 = s; c.g2 = pl; c.has = 1;
  return c;
}
MH_DEV double rel_vel(int g1, int g2, V3 pt, V3 dir) { return dot(dir, point_vel(g1, pt) - point_vel(g2, pt)); }
MH_DEV double calc_max_dist(int b, V3 n, double rmax) {           // CCD.cpp:585-609
  if (!enabled(b)) return 0.0;
  const V3 xd0 = Vl(b) + cross(X(b), Wa(b));
  return dot(n, xd0) + norm(cross(Wa(b), n)) * rmax;
}
// CCD::calc_CA_Euler_step_sphere / _generic / calc_next_CA_Euler_step_generic
// (CCD.cpp:138-166, 169-235, 238-405) for pair p
MH_DEV double ca_step(int p) {
  const PairGeom g = pair_geom(p);
  ContactGeom c; c.has = 0;
  bool have_c = false;
  if (is_spokes(g.b)) {
    // no SpherePrimitive in the pair: generic step (CCD.cpp:127-133); in contact the plugin's
    // calc_next_CA_Euler_step reports "never" (coldet-plugin.cpp:205-208); _rmax of the wheel is 0
    if (g.dist <= 0.0) return MHW_INF;
  } else
#if MHW_BOX
  if (box_plane_pair(g.a, g.b)) {                                   // a box-sphere pair follows the sphere rule below
    if (g.dist <= 0.0) {
      // calc_next_CA_Euler_step_generic (CCD.cpp:238-405) for plane (geom1) / box (geom2)
      const unsigned m = box_contact_mask(g.a, MH_NEAR_ZERO, g.b);   // the pair's own plane
      if (m == 0u) return MHW_INF;
      const V3 cn = -plane_n(g.b);
      const int gnd = plane_body(g.b);
      V3 p3[3]; int np = 0; V3 first = v3(0.0, 0.0, 0.0);
      for (int i = 0; i < 8; i++) if ((m >> i) & 1u) {
        const V3 vtx = box_vertex(g.a, i);
        if (rel_vel(gnd, g.a, vtx, cn) < -MH_NEAR_ZERO) return 0.0;
        if (np == 0) first = vtx;
        if (np < 3) p3[np] = vtx;
        np++;
      }
      if (np >= 3 && !collinear(p3[0], p3[1], p3[2])) return MHW_INF;   // only the first three are ever tested (:313-318)
      // calc_next_CA_Euler_step_polyhedron_plane (CCD.cpp:410-468) with normal = -cn, offset0 = -<cn, point>
      const V3 normal = -cn; const double offset0 = -dot(cn, first);
      double R[9]; rot(g.a, R);
      const V3 nP = v3((R[0]*normal.x + R[3]*normal.y) + R[6]*normal.z, (R[1]*normal.x + R[4]*normal.y) + R[7]*normal.z, (R[2]*normal.x + R[5]*normal.y) + R[8]*normal.z);
      const V3 dp = normal * offset0 - X(g.a);
      const V3 dpb = v3((R[0]*dp.x + R[3]*dp.y) + R[6]*dp.z, (R[1]*dp.x + R[4]*dp.y) + R[7]*dp.z, (R[2]*dp.x + R[5]*dp.y) + R[8]*dp.z);
      const double offset = dot(nP, dpb);
      const V3 w = Wa(g.a), vl = Vl(g.a);
      const V3 wb = v3((R[0]*w.x + R[3]*w.y) + R[6]*w.z, (R[1]*w.x + R[4]*w.y) + R[7]*w.z, (R[2]*w.x + R[5]*w.y) + R[8]*w.z);
      const V3 vb = v3((R[0]*vl.x + R[3]*vl.y) + R[6]*vl.z, (R[1]*vl.x + R[4]*vl.y) + R[7]*vl.z, (R[2]*vl.x + R[5]*vl.y) + R[8]*vl.z);
      const double av_norm = norm(wb);
      const double lv_dot_n = -dot(nP, vb);
      double max_step = MHW_INF;
      for (int i = 0; i < 8; i++) {
        const V3 vtx = box_corner(g.a, i);
        const double r = norm(vtx);
        const double dist = dot(nP, vtx) - offset;
        if (dist < MH_NEAR_ZERO) continue;
        const double sp = lv_dot_n + av_norm * r;
        const double speed = (0.0 > sp) ? 0.0 : sp;
        const double cand = dist / speed;
        max_step = (cand < max_step) ? cand : max_step;
      }
      return max_step;
    }
  } else
#endif
  if (!(g.dist > MH_NEAR_ZERO)) {
    c = contact_geom(p, MH_NEAR_ZERO); have_c = true;
    if (c.has && fabs(rel_vel(c.g1, c.g2, c.pt, c.n)) < MH_NEAR_ZERO * 10) return MHW_INF;
  }
  // CA_generic
  if (g.dist <= 0.0 && !is_spokes(g.b) && !box_plane_pair(g.a, g.b)) {
    if (!have_c) c = contact_geom(p, MH_NEAR_ZERO);
    if (!c.has) return MHW_INF;
    if (rel_vel(c.g1, c.g2, c.pt, c.n) < -MH_NEAR_ZERO) return 0.0;
    return MHW_INF;
  }
  const V3 d0 = g.pa - g.pb;
  const V3 n0 = d0 / norm(d0);
  const double tA = calc_max_dist(g.a, -n0, enabled(g.a) ? gd[D_RMAX + g.a] : 0.0);
  const double tB = calc_max_dist(g.b, n0, enabled(g.b) ? gd[D_RMAX + g.b] : 0.0);
  double total = tA + tB;
  if (total < 0.0) total = 0.0;
  const double cand = g.dist / total;
  return (cand < MHW_INF) ? cand : MHW_INF;
}

// ---- body-lane dynamics -------------------------------------------------------------------------
MH_DEV void inertia_world(int b, double Jw[9]) {
  double R[9]; rot(b, R);
  double T[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) T[3*i+j] = R[3*i+j] * gd[D_INERTIA + 3*b + j];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Jw[3*i+j] = (T[3*i] * R[3*j] + T[3*i+1] * R[3*j+1]) + T[3*i+2] * R[3*j+2];
  Jw[1] = Jw[3]; Jw[2] = Jw[6]; Jw[5] = Jw[7];
}
// X blocks of all bodies into the image (lane b): inverse_SPD of the 1x1 mass block and of
// the 3x3 world inertia, same operation order as oracle/linalg.hpp (left-looking dpotf2 + solves).
// Also leaves the world inertia product Jw*w for the forward dynamics in registers of nobody:
// fwd dyn recomputes it (different call site, same arithmetic).
MHW_FN void compute_xinv() {
  const int lane = lane_id();
  wave_sync();
  // a body that has not turned since the last call keeps its X block: the block is a function of the
  // quaternion (and of scene constants) only, so the cached values are the ones this call would compute
  bool stale = false;
  if (lane < gi[I_NB]) {
#pragma unroll
    for (int k = 0; k < 4; k++) stale = stale || !(gd[D_XQ + 4*lane + k] == gd[D_ST + 13*lane + 3 + k]);
  }
  if (ballot(stale) == 0ull) return;
  if (stale) {
    const int b = lane;
#pragma unroll
    for (int k = 0; k < 4; k++) gd[D_XQ + 4*b + k] = gd[D_ST + 13*b + 3 + k];
    double im;
    { const double l = sqrt(gd[D_MASS + b]); const double e = 1.0 / l; im = e / l; }
    double Jw[9]; inertia_world(b, Jw);
#pragma unroll
    for (int k = 0; k < 9; k++) gd[D_JW + 9*b + k] = Jw[k];
    double l00, l10, l20, l11, l21, l22;
    { double ajj = Jw[0]; ajj = sqrt(ajj); l00 = ajj; l10 = Jw[3] / ajj; l20 = Jw[6] / ajj; }
    { double ajj = Jw[4]; ajj = ajj - l10 * l10; ajj = sqrt(ajj); l11 = ajj; double s = Jw[7]; s = s - l20 * l10; l21 = s / ajj; }
    { double ajj = Jw[8]; ajj = ajj - l20 * l20; ajj = ajj - l21 * l21; ajj = sqrt(ajj); l22 = ajj; }
    double col[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double b0 = (c == 0) ? 1.0 : 0.0, b1 = (c == 1) ? 1.0 : 0.0, b2 = (c == 2) ? 1.0 : 0.0;
      b0 = b0 / l00; b1 = b1 - b0 * l10; b2 = b2 - b0 * l20;
      b1 = b1 / l11; b2 = b2 - b1 * l21;
      b2 = b2 / l22;
      { double s = b2; b2 = s / l22; }
      { double s = b1; s = s - l21 * b2; b1 = s / l11; }
      { double s = b0; s = s - l10 * b1; s = s - l20 * b2; b0 = s / l00; }
      col[c][0] = b0; col[c][1] = b1; col[c][2] = b2;
    }
    double Ai[9];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int i = 0; i < 3; i++) Ai[i + 3*c] = col[c][i];
    Ai[0 + 3*1] = Ai[1 + 3*0]; Ai[0 + 3*2] = Ai[2 + 3*0]; Ai[1 + 3*2] = Ai[2 + 3*1];
    gd[D_XINV + 10*b] = im;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) gd[D_XINV + 10*b + 1 + 3*r + c] = Ai[r + 3*c];
  }
  wave_sync();
}
MH_DEV void euler_vel(int b, double qd[7]) {
  const V3 v = Vl(b), w = Wa(b);
  const double x = gd[D_ST + 13*b+3], y = gd[D_ST + 13*b+4], z = gd[D_ST + 13*b+5], ww = gd[D_ST + 13*b+6];
  qd[0] = v.x; qd[1] = v.y; qd[2] = v.z;
  qd[3] = 0.5 * ((ww * w.x + z * w.y) - y * w.z);
  qd[4] = 0.5 * ((ww * w.y + x * w.z) - z * w.x);
  qd[5] = 0.5 * ((ww * w.z + y * w.x) - x * w.y);
  qd[6] = 0.5 * (((-x * w.x) - y * w.y) - z * w.z);
}
MH_DEV void set_coords(int b, const double q[7]) {
  gd[D_ST + 13*b] = q[0]; gd[D_ST + 13*b+1] = q[1]; gd[D_ST + 13*b+2] = q[2];
  const double nrm = sqrt(((q[3]*q[3] + q[4]*q[4]) + q[5]*q[5]) + q[6]*q[6]);
  gd[D_ST + 13*b+3] = q[3] / nrm; gd[D_ST + 13*b+4] = q[4] / nrm; gd[D_ST + 13*b+5] = q[5] / nrm; gd[D_ST + 13*b+6] = q[6] / nrm;
}
// coordinates <- base + (scale ? t : 1) * dq for all bodies, normalising the quaternion
// (set_generalized_coordinates_euler).  base/dq are offsets into gd.  mode 2: base + (h) * eulervel
MHW_FN void set_q_from(int base_off, int dq_off, double t, int scale) {
  const int lane = lane_id();
  wave_sync();
  if (lane < gi[I_NB]) {
    double q[7];
#pragma unroll
    for (int k = 0; k < 7; k++) { double v = gd[dq_off + 7*lane + k]; if (scale) v = v * t; q[k] = v + gd[base_off + 7*lane + k]; }
    set_coords(lane, q);
  }
  wave_sync();
}
// TSS:156-164: q = qsave + (h + tc) * eulervel(qsave)
MH_DEV void integrate_positions(double hh) {
  const int lane = lane_id();
  wave_sync();
  if (lane < gi[I_NB]) {
    set_coords(lane, gd + D_QSAVE + 7 * lane);
    double qd[7]; euler_vel(lane, qd);
    double q[7];
#pragma unroll
    for (int i = 0; i < 7; i++) { q[i] = qd[i] * hh; q[i] = q[i] + gd[D_QSAVE + 7*lane + i]; }
    set_coords(lane, q);
  }
  wave_sync();
}
#if MHW_FORCES
// The same with the scene's recurrent forces and the caller's wrench (Simulator::precalc_fwd_dyn, Simulator.cpp:319-350: accumulators cleared, recurrent
// forces, then the controller, once per mini-step): positions are this mini-step's, v and omega still its starting velocities.  Terms accumulate in the
// canonical order gravity, Stokes drag (StokesDragForce.cpp:39-44), damping (DampingForce.cpp:32-51: velocities into the body frame, the wrench back),
// caller wrench; an absent term is left out, not added as zero.  Every operation rounds on its own; world axes at the COM throughout.
MH_DEV void integrate_velocities_forced(double h, int ft) {
  const int lane = lane_id();
  compute_xinv();
  if (lane < gi[I_NB]) {
    const int b = lane;
    const double m = gd[D_MASS + b];
    V3 F = v3(gd[D_GRAV] * m, gd[D_GRAV + 1] * m, gd[D_GRAV + 2] * m);
    V3 T = v3(0.0, 0.0, 0.0);
    bool has_t = false;
    const V3 v = Vl(b), w = Wa(b);
    if (ft & MH_FORCE_STOKES) {
      F = F + v * (-gf[F_SB + b]);
      T = w * (-gf[F_SBA + b]); has_t = true;
    }
    if (ft & MH_FORCE_DAMPING) {
      double R[9]; rot(b, R);                                      // the rotation inertia_world() formed Jw from: same function, same quaternion
      const V3 vi = v3((R[0]*v.x + R[3]*v.y) + R[6]*v.z, (R[1]*v.x + R[4]*v.y) + R[7]*v.z, (R[2]*v.x + R[5]*v.y) + R[8]*v.z);
      const V3 wi = v3((R[0]*w.x + R[3]*w.y) + R[6]*w.z, (R[1]*w.x + R[4]*w.y) + R[7]*w.z, (R[2]*w.x + R[5]*w.y) + R[8]*w.z);
      const V3 fb = vi * (-(gf[F_KL + b] + norm(vi) * gf[F_KLSQ + b]));
      const V3 tb = wi * (-(gf[F_KA + b] + norm(wi) * gf[F_KASQ + b]));
      const V3 fw = v3((R[0]*fb.x + R[1]*fb.y) + R[2]*fb.z, (R[3]*fb.x + R[4]*fb.y) + R[5]*fb.z, (R[6]*fb.x + R[7]*fb.y) + R[8]*fb.z);
      const V3 tw = v3((R[0]*tb.x + R[1]*tb.y) + R[2]*tb.z, (R[3]*tb.x + R[4]*tb.y) + R[5]*tb.z, (R[6]*tb.x + R[7]*tb.y) + R[8]*tb.z);
      F = F + fw;
      T = has_t ? T + tw : tw; has_t = true;
    }
    if (ft & MHW_FORCE_WRENCH) {
      const double* r = gf + F_WR + 6*b;
      F = F + v3(r[0], r[1], r[2]);
      const V3 tq = v3(r[3], r[4], r[5]);
      T = has_t ? T + tq : tq; has_t = true;
    }
    const V3 xdd = F / m;
    const double* Jw = gd + D_JW + 9*b;
    const V3 Jww = v3((Jw[0]*w.x + Jw[1]*w.y) + Jw[2]*w.z, (Jw[3]*w.x + Jw[4]*w.y) + Jw[5]*w.z, (Jw[6]*w.x + Jw[7]*w.y) + Jw[8]*w.z);
    const V3 tau = has_t ? T - cross(w, Jww) : -cross(w, Jww);
    const double* Ji = gd + D_XINV + 10*b + 1;
    const V3 wd = v3((Ji[0]*tau.x + Ji[1]*tau.y) + Ji[2]*tau.z, (Ji[3]*tau.x + Ji[4]*tau.y) + Ji[5]*tau.z, (Ji[6]*tau.x + Ji[7]*tau.y) + Ji[8]*tau.z);
    const V3 vn = v + xdd * h, wn = w + wd * h;
    gd[D_ST + 13*b+7] = vn.x; gd[D_ST + 13*b+8] = vn.y; gd[D_ST + 13*b+9] = vn.z;
    gd[D_ST + 13*b+10] = wn.x; gd[D_ST + 13*b+11] = wn.y; gd[D_ST + 13*b+12] = wn.z;
  }
  wave_sync();
}
#endif
// forward dynamics + velocity integration (TSS:173-192; GravityForce.cpp:33-69)
MH_DEV void integrate_velocities(double h) {
#if MHW_FORCES
  { const int ft = uni(g_fterms); if (ft != 0) { integrate_velocities_forced(h, ft); return; } }   // no term at all: the text below, as it was
#endif
  const int lane = lane_id();
  compute_xinv();
  if (lane < gi[I_NB]) {
    const int b = lane;
    const double m = gd[D_MASS + b];
    const V3 f = v3(gd[D_GRAV] * m, gd[D_GRAV + 1] * m, gd[D_GRAV + 2] * m);
    const V3 xdd = f / m;
    const double* Jw = gd + D_JW + 9*b;                            // inertia_world(b), kept by compute_xinv for this orientation
    const V3 w = Wa(b);
    const V3 Jww = v3((Jw[0]*w.x + Jw[1]*w.y) + Jw[2]*w.z, (Jw[3]*w.x + Jw[4]*w.y) + Jw[5]*w.z, (Jw[6]*w.x + Jw[7]*w.y) + Jw[8]*w.z);
    const V3 tau = -cross(w, Jww);
    const double* Ji = gd + D_XINV + 10*b + 1;
    const V3 wd = v3((Ji[0]*tau.x + Ji[1]*tau.y) + Ji[2]*tau.z, (Ji[3]*tau.x + Ji[4]*tau.y) + Ji[5]*tau.z, (Ji[6]*tau.x + Ji[7]*tau.y) + Ji[8]*tau.z);
    const V3 vn = Vl(b) + xdd * h, wn = w + wd * h;
    gd[D_ST + 13*b+7] = vn.x; gd[D_ST + 13*b+8] = vn.y; gd[D_ST + 13*b+9] = vn.z;
    gd[D_ST + 13*b+10] = wn.x; gd[D_ST + 13*b+11] = wn.y; gd[D_ST + 13*b+12] = wn.z;
  }
  wave_sync();
}

// ---- constraint list (contact lanes) ----------------------------------------------------------------
MHW_FN void store_contact(int slot, int p, int g1, int g2, V3 pt, V3 n, double dist) {
  V3 s, t; orthonormal_basis(n, s, t);
  gi[I_CG1 + slot] = g1; gi[I_CG2 + slot] = g2; gi[I_CPAIR + slot] = p; gi[I_CNK + slot] = gi[I_PNK + p];
  gd[D_CPT + 3*slot] = pt.x; gd[D_CPT + 3*slot+1] = pt.y; gd[D_CPT + 3*slot+2] = pt.z;
  gd[D_CNR + 3*slot] = n.x; gd[D_CNR + 3*slot+1] = n.y; gd[D_CNR + 3*slot+2] = n.z;
  gd[D_CS1 + 3*slot] = s.x; gd[D_CS1 + 3*slot+1] = s.y; gd[D_CS1 + 3*slot+2] = s.z;
  gd[D_CS2 + 3*slot] = t.x; gd[D_CS2 + 3*slot+1] = t.y; gd[D_CS2 + 3*slot+2] = t.z;
  gd[D_CDIST + slot] = dist; gd[D_CMU + slot] = gd[D_PMU + p]; gd[D_CMUV + slot] = gd[D_PMUV + p];
  gd[D_CEPS + slot] = gd[D_PEPS + p]; gd[D_CCOMP + slot] = gd[D_PCOMP + p];
}
MH_DEV V3 Cpt(int i) { return v3(gd[D_CPT + 3*i], gd[D_CPT + 3*i+1], gd[D_CPT + 3*i+2]); }
MH_DEV V3 Cdir(int i, int d) {
  const int o = (d == 0) ? D_CNR : (d == 1 ? D_CS1 : D_CS2);
  return v3(gd[o + 3*i], gd[o + 3*i+1], gd[o + 3*i+2]);
}
MH_DEV double contact_vn(int i) { return rel_vel(gi[I_CG1 + i], gi[I_CG2 + i], Cpt(i), Cdir(i, 0)); }

#if MHW_NOSLIP
// find_contacts_wheel_plane (coldet-plugin.cpp:211-288): spoke lanes; one contact per tip below
// sim->contact_dist_thresh (whatever tolerance the caller passed, :214), appended at slot nc
MHW_FN int spoke_contacts(int p, int nc) {
  p = uni(p); nc = uni(nc);
  const int lane = lane_id();
  int a, b; pair_bodies(p, a, b);
  bool has = false; V3 pt = v3(0.0, 0.0, 0.0); double dist = 0.0;
  if (lane < gi[I_NSPOKES]) {
    const V3 tip = spoke_tip(a, lane);
    const V3 pp = to_plane(tip, b);
    has = pp.y < gd[D_THRESH];
    pt = (tip + from_plane(v3(pp.x, 0.0, pp.z), b)) * 0.5;
    dist = pp.y;
  }
  const uint64_t m = ballot(has);
  wave_sync();
  if (nc + popc(m) > MHW_MAX_CONTACTS) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); return nc; }
  if (has) store_contact(nc + popc(m & lanes_below(lane)), p, a, b, pt, plane_n(b), dist);
  wave_sync();
  return nc + popc(m);
}
#endif

#if MHW_BOX
// Constraint list of a pair list (gi[list_off .. list_off+count)), pairs in list order, for variants
// whose pairs can carry several contacts (box vertices).  mode 0: the simulator's list
// (find_unilateral_constraints, CSim:488-537: contacts of pairs closer than contact_dist_thresh);
// mode 1: the stabiliser's (add_contact_constraints, CStab:300-345: one synthetic contact for a
// separated pair, find_contacts otherwise).  Spokes pairs are appended by the caller.
// Returns the number of contacts, or -1 if they do not fit.
MHW_FN int gen_contacts(int list_off, int count, int mode) {
  list_off = uni(list_off); count = uni(count); mode = uni(mode);
  const int lane = lane_id();
  const double thresh = gd[D_THRESH];
  ContactGeom c; c.has = 0; c.g1 = 0; c.g2 = 0; c.pt = v3(0, 0, 0); c.n = v3(0, 0, 0); c.dist = 0.0;
  int p = 0, cnt = 0, bx = -1; unsigned bmask = 0u;
  int bpl = 0;                                                      // the plane of this lane's box-plane pair
  if (lane < count) {
    p = gi[list_off + lane];
    const PairGeom g = pair_geom(p);
    if (is_spokes(g.b)) { }
    else if (mode == 1 && g.dist >= MH_NEAR_ZERO) {
      const V3 nn = g.pb - g.pa;
      c.n = nn / norm(nn); c.pt = g.pa; c.g1 = g.a; c.g2 = g.b; c.dist = g.dist; c.has = 1; cnt = 1;
    } else if (mode == 1 || g.dist < thresh) {
      const double TOL = (mode == 1) ? MH_NEAR_ZERO : thresh;
      if (box_plane_pair(g.a, g.b)) { bx = g.a; bpl = g.b; bmask = box_contact_mask(bx, TOL, bpl); cnt = popc((uint64_t)bmask); }
      else { c = contact_geom(p, TOL); cnt = c.has; }
    }
  }
  // exclusive prefix sum of the per-pair counts (few pairs carry contacts)
  int off = 0, total = 0;
  { uint64_t m = ballot(cnt > 0);
    while (m) { const int k = ctz(m); m &= m - 1; const int ck = read_lane(cnt, k); if (lane > k) off += ck; total += ck; } }
  wave_sync();
  if (total > MHW_MAX_CONTACTS) return -1;
  if (bx >= 0) {
    const V3 cn = -plane_n(bpl); const int gnd = plane_body(bpl);
    for (int i = 0; i < 8; i++) if ((bmask >> i) & 1u) {
      const V3 vtx = box_vertex(bx, i);
      store_contact(off, p, gnd, bx, vtx, cn, to_plane(vtx, bpl).y);   // create_contact(plane, box, vertex, -n, dist)
      off++;
    }
  } else if (c.has) store_contact(off, p, c.g1, c.g2, c.pt, c.n, c.dist);
  wave_sync();
  return total;
}
#endif

// ---- islands (UC:940-1194): uniform scalar BFS; one island at a time ----------------------------------
// The search's state is two wave-uniform masks that the caller holds between the calls: the enabled bodies not yet visited and the contacts already
// handed out.
struct IslandSearch { unsigned node_mask; uint64_t done; };
struct Island { int nic, nib; unsigned bodies; uint64_t contacts; };   // counts, and the same two sets as bit masks (body b, contact lane c)
MH_DEV IslandSearch islands_begin(int nc) {
  nc = uni(nc);
  const int lane = lane_id();
  const int nb = geti(I_NB);
  const bool in = lane < nc;
  const int a = in ? gi[I_CG1 + lane] : -1, b = in ? gi[I_CG2 + lane] : -1;
  unsigned nodes = 0;
  for (int k = 0; k < nb; k++) if (ballot(in && (a == k || b == k)) != 0ull) nodes |= 1u << k;   // enabled bodies are 0..nb-1
  IslandSearch s; s.node_mask = nodes; s.done = 0ull;
  return s;
}
// pops the next island into gi[I_ISLC..] (contacts, in the order the reference's BFS collects them)
// and gi[I_ISLB..] (sorted unique bodies) and describes it in `isl`; returns false when none is left.
// Contact lanes hold (g1, g2); the BFS itself runs on wave-uniform bit masks: a node's contacts and
// neighbours are ballots, the FIFO is a string of nibbles.  (The reference pushes a neighbour again
// while it waits in the queue; the second visit adds nothing, so visiting on push gives the same order.)
MH_DEV bool next_island(int nc, IslandSearch& s, Island& isl) {
  nc = uni(nc);
  const int lane = lane_id();
  unsigned node_mask = s.node_mask;
  uint64_t done = s.done;
  const bool in = lane < nc;
  const int a = in ? gi[I_CG1 + lane] : -1, b = in ? gi[I_CG2 + lane] : -1;
  const uint64_t both = ballot(in && enabled(a) && enabled(b));
  bool found = false;
  wave_sync();
  while (node_mask) {
    const int start = __ffs((int)node_mask) - 1;
    unsigned visited = 1u << start, bodies = 0;
    uint64_t queue = (uint64_t)start; int qlen = 1;
    int nic = 0;
    uint64_t contacts = 0ull;
    while (qlen > 0) {
      const int nd = (int)(queue & 15ull); queue >>= 4; qlen--;
      node_mask &= ~(1u << nd);
      bodies |= 1u << nd;
      const uint64_t touch = ballot(in && (a == nd || b == nd));
      uint64_t m = touch & both;
      while (m) {
        const int i = ctz(m); m &= m - 1;
        const int ai = read_lane(a, i), bi = read_lane(b, i);
        const int nbr = (ai == nd) ? bi : ai;
        if (!((visited >> nbr) & 1u)) { visited |= 1u << nbr; queue |= (uint64_t)nbr << (4 * qlen); qlen++; }
      }
      const uint64_t fresh = touch & ~done;
      if ((fresh >> lane) & 1ull) gi[I_ISLC + nic + popc(fresh & lanes_below(lane))] = lane;
      nic += popc(fresh);
      done |= fresh; contacts |= fresh;
    }
    if (nic == 0) continue;
    if (lane < 32 && ((bodies >> lane) & 1u)) gi[I_ISLB + popc((uint64_t)(bodies & ((1u << lane) - 1u)))] = lane;
    isl.nic = nic; isl.nib = popc((uint64_t)bodies); isl.bodies = bodies; isl.contacts = contacts;
    found = true;
    break;
  }
  wave_sync();
  s.node_mask = node_mask; s.done = done;
  return found;
}

// ---- problem data (Jacobian-row lanes): rows r = d*nic + i, ndir = 3 (impact) or 1 (stabilisation) ----
// offset of `body`'s generalised coordinates among the island's: gi[I_ISLB..] lists the bodies of the mask `bodies` in ascending order, so the position
// of a body in that list is the number of the island's bodies below it
MH_DEV int gc_of(int body, unsigned bodies) { return ((bodies >> body) & 1u) ? 6 * popc((uint64_t)(bodies & ((1u << body) - 1u))) : -1; }
// Returns norm_inf of the QP model's LCP matrix (want_norm, which needs ndir == 3; 0.0 otherwise), uniform.
MH_DEV double compute_problem_data(int nic, unsigned bodies, int ndir, int fresh_xinv, bool want_norm) {   // bodies: Island::bodies
  nic = uni(nic); bodies = uni(bodies); ndir = uni(ndir); fresh_xinv = uni(fresh_xinv);
  const int lane = lane_id();
  const int R = ndir * nic;   // callers guarantee R <= MHW_MAX_ROWS (rows_fit)
  // the X blocks depend on the orientations only: the impact handler reuses the ones
  // integrate_velocities() just computed for this mini-step; stabilisation moves the bodies
  if (fresh_xinv) compute_xinv();
  if (lane < R) {
    const int d = small_div(lane, nic), i = lane - d * nic;
    const int ci = gi[I_ISLC + i];
    const V3 dir = Cdir(ci, d), pt = Cpt(ci);
    double cv = 0.0;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int b = (k == 0) ? gi[I_CG1 + ci] : gi[I_CG2 + ci];
      double* Jr = gd + D_J + 12 * lane + 6 * k; double* XJr = gd + D_XJ + 12 * lane + 6 * k;
      if (!enabled(b)) { gi[I_ROWOFF + 2*lane + k] = -1; continue; }
      const V3 dd = (k == 0) ? dir : -dir;
      const V3 r = pt - X(b);
      const V3 rxd = cross(r, dd);
      gi[I_ROWOFF + 2*lane + k] = gc_of(b, bodies);
      Jr[0] = dd.x; Jr[1] = dd.y; Jr[2] = dd.z; Jr[3] = rxd.x; Jr[4] = rxd.y; Jr[5] = rxd.z;
      const double im = gd[D_XINV + 10*b]; const double* Ji = gd + D_XINV + 10*b + 1;
      XJr[0] = dd.x * im; XJr[1] = dd.y * im; XJr[2] = dd.z * im;
#pragma unroll
      for (int c = 0; c < 3; c++) XJr[3 + c] = (rxd.x * Ji[c] + rxd.y * Ji[3 + c]) + rxd.z * Ji[6 + c];
      const V3 vl = Vl(b), wa = Wa(b);
      double tmp = 0.0;
      tmp = tmp + dd.x * vl.x; tmp = tmp + dd.y * vl.y; tmp = tmp + dd.z * vl.z;
      tmp = tmp + rxd.x * wa.x; tmp = tmp + rxd.y * wa.y; tmp = tmp + rxd.z * wa.z;
      cv = cv + tmp;
    }
    gd[D_CV + lane] = cv;
  }
  wave_sync();
  // G(r,c) = sum over the blocks of row r of dot6(J_r[blk], XJ_c[same body]) for the direction blocks a <= b;
  // the lower blocks are the transposes setup_QP reads (ICH-QP:392-401): entry (r,c) there is computed as
  // (c,r).  One ENTRY per lane (R^2 <= 144 entries over 64 lanes), not one row per lane.
  // The QP model (want_norm) also takes norm_inf of the LCP matrix here, where every entry of G passes through a register: max |entry| over G (the
  // compliance added on the normal diagonal first), the mu's and the polygon edges (cos 0 = sin pi/2 = 1), which is what WorldMat::norm_all() found by
  // scanning G again (a > m ? a : m from 0.0: independent of the order, and a NaN is passed over as there).
  double nmax = 0.0;
  {
    const unsigned mnic = small_div_magic(nic), mR = small_div_magic(R);
    for (int e = lane; e < R * R; e += 64) {
      int r = small_div_m(e, mR), c = e - r * R;
      const bool ndiag = (r == c) && (r < nic);                     // entry e of G itself: the swap below keeps a diagonal entry where it is
      if (small_div_m(c, mnic) < small_div_m(r, mnic)) { const int t = r; r = c; c = t; }
      double res = 0.0;
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const int off = gi[I_ROWOFF + 2*r + k];
        if (off < 0) continue;
        double tmp = 0.0;
        int kk = -1;
        if (gi[I_ROWOFF + 2*c] == off) kk = 0; else if (gi[I_ROWOFF + 2*c + 1] == off) kk = 1;
        if (kk >= 0) {
          const double* Jr = gd + D_J + 12 * r + 6 * k; const double* XJc = gd + D_XJ + 12 * c + 6 * kk;
#pragma unroll
          for (int q = 0; q < 6; q++) tmp = tmp + Jr[q] * XJc[q];
        }
        res = res + tmp;
      }
      gd[D_G + e] = res;
      if (want_norm) {
        double g = res;
        if (ndiag) g = g + gd[D_CCOMP + gi[I_ISLC + r]];
        const double a = fabs(g); nmax = (a > nmax) ? a : nmax;
      }
    }
  }
  if (want_norm) {
    if (lane < nic) { const double a = fabs(gd[D_CMU + gi[I_ISLC + lane]]); nmax = (a > nmax) ? a : nmax; }
    nmax = wave_max(nmax);
    nmax = (nmax > 1.0) ? nmax : 1.0;
  }
  wave_sync();
  return nmax;
}

// ---- implicit LCP matrices ------------------------------------------------------------------------
// mode 0: _MM of solve_qp_work (ICH-QP:129-148 + setup_QP :271-497), never materialised:
//   [ H  -N' ]   H = [n s t -s -t] blocks of C X C' (+ compliance), N = [Cn rows of H ; friction polygons]
//   [ N   0  ]
// Every entry is one value of G = [Cn;Cs;Ct] X [Cn;Cs;Ct]' (upper blocks stored, lower ones
// read transposed exactly as setup_QP does), mu_i, or -cos/-sin of a polygon edge.
// mode 1: the stabilisation matrix Cn X Cn' (CStab:932-947), read straight from G.
// Lane r caches the description of ITS row; the column is wave-uniform.
//
// The friction polygons of mode 0 (rows and columns from 6 nic on): contact i of the island owns the edges [koff_i, koff_i+1), koff being the running sum
// of the contacts' edge counts gi[I_CNK] / 2.  poly_index() forms the sums once per solve, one contact per lane: `total` is koff_nic; `pack` holds koff_0
// .. koff_7 in one byte each (a sum is at most MH_LCP_MAX_N_WAVE), which serves every island of up to POLY_PACK contacts from a uniform register -- a
// larger island reads gi[I_KOFF..], filled for it alone; `ri` / `rbase` are the contact and its koff of the polygon row this lane stands for, if it does.
struct PolyIndex { int total; uint64_t pack; int ri, rbase; };
enum { POLY_PACK = 7 };
MH_DEV int poly_koff(uint64_t pack, int i) { return (int)((pack >> (8 * i)) & 0xffull); }
MH_DEV PolyIndex poly_index(int nic) {
  const int lane = lane_id();
  const int cnk = (lane < nic) ? gi[I_CNK + gi[I_ISLC + lane]] / 2 : 0;
  const int rr = lane - 6 * nic;
  PolyIndex x; x.pack = 0ull; x.ri = 0; x.rbase = 0;
  int off = 0, total = 0;
  for (int k = 0; k < nic; k++) {
    const int ck = read_lane(cnk, k);
    if (lane > k) off += ck;
    total += ck;                                            // koff_k+1
    if (k < POLY_PACK) x.pack |= (uint64_t)(unsigned)total << (8 * (k + 1));
    if (k + 1 < nic && rr >= total) { x.ri = k + 1; x.rbase = total; }   // (the sums do not decrease: the last one at or below rr is the row's)
  }
  if (nic > POLY_PACK && lane <= nic) gi[I_KOFF + lane] = off;
  x.total = total;
  return x;
}
struct WorldMat {
  int mode, nic, R, nvars, n, doff; unsigned mnic;
  uint64_t kpack;                                          // PolyIndex::pack (uniform)
  // this lane's row: kind 0 = a row of G (variable rows and the Cn v+ >= 0 rows, which repeat block-row 0),
  // 2 = friction polygon row, 3 = none.  grow = offset of the row in G, gcol = its column index in G
  // (the transposed reads of -N'), rneg = the row belongs to a -s / -t block.
  int rkind, ra, ri, grow, gcol, rneg, rvar;
  double rmu, rcos, rsin, rcomp;
  double nrm;                                              // mode 0: norm_inf(M), from compute_problem_data (uniform)
  MH_DEV static int dir_of(int a) { return (a == 0) ? 0 : ((a == 1 || a == 3) ? 1 : 2); }
  MH_DEV void init(int mode_, int nic_, int n_, double nrm_, const PolyIndex& px) {
    mode = mode_; nic = nic_; n = n_; nrm = nrm_; kpack = uni(px.pack);
    doff = (mode == 2) ? (int)D_NSMM : (int)D_G;          // mode 2: the no-slip model's dense Schur complement
    R = (mode == 0) ? 3 * nic_ : nic_; nvars = 5 * nic_; mnic = 0u;
    const int r = lane_id();
    rkind = 3; ra = 0; ri = 0; grow = 0; gcol = 0; rneg = 0; rvar = 0; rmu = 0.0; rcos = 0.0; rsin = 0.0; rcomp = 0.0;
    if (mode != 0) return;
    mnic = small_div_magic(nic);
    if (r < nvars) { rkind = 0; rvar = 1; ra = small_div_m(r, mnic); ri = r - ra * nic; }
    else if (r < nvars + nic) { rkind = 0; ra = 0; ri = r - nvars; }
    else if (r < n) {
      rkind = 2;
      const int rr = r - nvars - nic;
      const int i = px.ri;
      ri = i; const int rj = rr - px.rbase;
      const int ci = gi[I_ISLC + i]; const int kh = gi[I_CNK + ci] / 2;
      rmu = gd[D_CMU + ci]; rcos = c_fric.c[kh][rj]; rsin = c_fric.s[kh][rj];
    }
    if (rkind == 0) {
      rcomp = gd[D_CCOMP + gi[I_ISLC + ri]];
      gcol = dir_of(ra) * nic + ri; grow = D_G + gcol * R; rneg = (ra >= 3) ? 1 : 0;
    }
  }
  // M(lane, c), c wave-uniform.  Entries: +-G (+ compliance on the normal diagonal), mu, -cos/-sin, 0.
  MH_DEV double at_row(int c) const {
    if (mode != 0) { const int l = lane_id(); return (l < n) ? gd[doff + l * n + c] : 0.0; }
    if (c < nvars) {
      const int b = small_div_m(c, mnic), j = c - b * nic;
      const int bneg = (b >= 3) ? 1 : 0;
      if (rkind == 0) {
        double g = gd[grow + dir_of(b) * nic + j];
        if (rneg != bneg) g = -g;
        if (ra == 0 && b == 0 && ri == j) g = g + rcomp;
        return g;
      }
      if (rkind == 2 && j == ri) return (b == 0) ? rmu : ((b == 1 || b == 3) ? -rcos : -rsin);
      return 0.0;
    }
    if (!rvar) return 0.0;
    const int cc = c - nvars;
    if (cc < nic) {
      double g = gd[D_G + cc * R + gcol];
      if (rneg) g = -g;
      if (ra == 0 && ri == cc) g = g + rcomp;
      return -g;
    }
    int i = 0, k0; const int rr = cc - nic;
    if (nic <= POLY_PACK) { while (rr >= poly_koff(kpack, i + 1)) i++; k0 = poly_koff(kpack, i); }
    else { while (rr >= gi[I_KOFF + i + 1]) i++; k0 = gi[I_KOFF + i]; }
    if (i != ri) return -0.0;
    const int jj = rr - k0; const int ci = gi[I_ISLC + i]; const int kh = gi[I_CNK + ci] / 2;
    const double v = (ra == 0) ? gd[D_CMU + ci] : ((ra == 1 || ra == 3) ? -c_fric.c[kh][jj] : -c_fric.s[kh][jj]);
    return -v;
  }
  MH_DEV double diag() const {
    if (mode != 0) { const int l = lane_id(); return (l < n) ? gd[doff + l * n + l] : 0.0; }
    if (!rvar) return 0.0;
    double g = gd[grow + gcol];                              // H(ra, ri, ra, ri): same sign class, + compliance on the normal block
    if (ra == 0) g = g + rcomp;
    return g;
  }
  // norm_inf(M) = max |entry|.  mode 0: H entries, mu, and the polygon edges (cos 0 = sin pi/2 = 1): taken by compute_problem_data while it builds G
  MH_DEV double norm_all() const {
    if (mode == 0) return nrm;
    const int lane = lane_id();
    double m = 0.0;
    if (lane < n) for (int c = 0; c < n; c++) { const double a = fabs(gd[doff + lane * n + c]); m = (a > m) ? a : m; }
    return wave_max(m);
  }
  MH_DEV double offdiag_max() const {
    if (mode != 0) {
      const int lane = lane_id(); double m = 0.0;
      if (lane < n) for (int c = 0; c < n; c++) { const double a = fabs(gd[doff + lane * n + c]); if (c != lane && a > m) m = a; }
      return wave_max(m);
    }
    // mode 0: the off-diagonal part contains every polygon edge, every mu, every off-diagonal
    // H entry and the H DIAGONAL values again through the Cn v+ rows / -N' columns: norm_inf(M) itself
    return nrm;
  }
};

// The solver chains of the two handlers (inlined at its two call sites: the hot impact path in the
// kernel body and the cold stabilisation routine -- as an out-of-line function its register
// save/restore traffic cost more than the second copy):
//   mode 0  ICH-QP:219-225  lcp_fast_regularized(-20,4,-8); on failure z.set_zero(), lcp_lemke_regularized
//   mode 1  CStab:954-955   lcp_fast; on failure lcp_lemke_regularized
//   mode 2  ICH:1239,1281   the same chain on the no-slip model's dense matrix, warm-started from _v
// The rand() ring is read from / written back to the image.
struct ChainOut { int ok; double zi; int zsize; unsigned piv; };
// nrm, px: mode 0's norm_inf(M) (compute_problem_data) and polygon index (poly_index); modes 1 and 2 scan their dense matrix and look at neither.
MH_DEV ChainOut world_lcp_chain(int mode, int nic, int n, double qi, double zi, int zsize, double nrm, const PolyIndex& px)
{
  mode = uni(mode); nic = uni(nic); n = uni(n); zsize = uni(zsize); nrm = uni(nrm);
  const int lane = lane_id();
  const unsigned long long ts = lp_tick();
  WorldMat M; M.init(mode, nic, n, nrm, px);
  const double nrm0 = M.norm_all(), dii = M.diag();
  lp_tock(LP_SETUP, ts);
  WaveRand rng; rng.r = (lane < 31) ? (unsigned)gi[I_RNG + lane] : 0u; rng.idx = geti(I_RNG + 31);
  LuScratch S; S.small = gd + D_A; S.ka = geti(I_KA);     // I_KA <= MHW_KA_V (clamped at launch)
  S.big = reinterpret_cast<double*>(uni((uint64_t)reinterpret_cast<uintptr_t>(g_lu_ws)));
  Trace tr; tr.buf = nullptr; tr.cap = 0; tr.len = 0;
  unsigned ptot = 0;
  bool ok = false;
  for (int stage = 0; stage < 2; stage++) {
    LcpParams P; P.piv_tol = -1.0; P.zero_tol = -1.0; P.min_exp = -20;
    if (stage == 0) {
      if (mode == 0) { P.kind = MH_LCP_FAST_REG; P.step_exp = 4; P.max_exp = -8; }
      else { P.kind = MH_LCP_FAST; P.step_exp = 1; P.max_exp = 1; }
    } else {
      if (mode == 0) zi = 0.0;                              // z.set_zero() keeps the size (ICH-QP:222)
      P.kind = MH_LCP_LEMKE_REG; P.step_exp = 1; P.max_exp = 1;
    }
    unsigned piv = 0;
    ok = lcp_solve_wave(P, c_pow10, n, M, S, gd + D_ART, nrm0, dii, qi, zi, zsize, rng, piv, tr);
    ptot += piv;
    if (ok) break;
  }
  wave_sync();
  if (lane < 31) gi[I_RNG + lane] = (int)rng.r;
  if (lane == 31) gi[I_RNG + 31] = rng.idx;
  wave_sync();
  ChainOut o; o.ok = ok ? 1 : 0; o.zi = zi; o.zsize = zsize; o.piv = ptot;
  return o;
}

// solve_qp_work's chain on the persistent _z/_zlast (ICH-QP:157-233); on success the solution is
// left in gd[D_ZSOL..] and in zlast/zbuf.  Returns 1 on success, 0 when the island is beyond this variant (MH_WORLD_UNSUPPORTED), -1 when the handler threw.
MH_DEV int solve_impact_lcp(int nic, double nrm) {               // nrm: norm_inf of _MM, as compute_problem_data returned it
  nic = uni(nic);
  const int lane = lane_id();
  const PolyIndex px = poly_index(nic);
  wave_sync();
  const int nk_total = px.total;
  const int nvars = 5 * nic, n = nvars + nic + nk_total;
  if (n > geti(I_NMAX) || n > MH_LCP_MAX_N_WAVE) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); return 0; }
  // _MM stays implicit (WorldMat mode 0); _qq per lane
  unsigned long long tm = tick();
  double qi = 0.0;
  if (lane < n) {
    const int r = lane;
    if (r < nvars) { const int a = small_div(r, nic), i = r - a * nic; const double v = gd[D_CV + WorldMat::dir_of(a) * nic + i]; qi = (a >= 3) ? -v : v; }
    else if (r < nvars + nic) qi = gd[D_CV + r - nvars];
    else {
      const int i = px.ri;
      const double cs = gd[D_CV + nic + i], ct = gd[D_CV + 2 * nic + i];
      const double vel = sqrt(cs * cs + ct * ct);
      qi = gd[D_CMUV + gi[I_ISLC + i]] * vel;
    }
  }
  tock(PH_MBUILD, tm);
  tm = tick();
  // z.resize(n); warm start from _zlast when sizes match (ICH-QP:158-162)
  const int zbuf_cap = geti(I_ZBUF_CAP), zlast_size = geti(I_ZLAST_SIZE);
  double zi;
  if (n > zbuf_cap) zi = 0.0; else zi = gd[D_ZBUF + lane];
  if (lane >= n) zi = 0.0;
  if (n == zlast_size) zi = (lane < n) ? gd[D_ZLAST + lane] : 0.0;
  const ChainOut co = world_lcp_chain(0, nic, n, qi, zi, n, nrm, px);
  zi = co.zi;
  const bool ok = uni(co.ok) != 0;
  account(n, uni(co.piv));
  tock(PH_LCP, tm);
  if (!ok) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_LCP_FAILED); wave_sync(); return -1; }      // LCPSolverException: thrown (see handle_impacts)
  wave_sync();
  if (lane < n) { gd[D_ZLAST + lane] = zi; gd[D_ZBUF + lane] = zi; }
  seti(I_ZLAST_SIZE, n);
  if (zbuf_cap < n) seti(I_ZBUF_CAP, n);
  seti(I_ZBUF_SIZE, 5 * nic);           // z is repacked to the epd layout = its first 5 nic entries (ICH-QP:244)
  wave_sync();
  return 1;
}

// dv = X_CnT cn + X_CsT cs + X_CtT ct ; v += dv   (ICH:343-348, 1784-1798); gc lanes
MHW_FN void apply_impulses(int nic, int nib, int ndir) {
  nic = uni(nic); nib = uni(nib); ndir = uni(ndir);
  const int lane = lane_id();
  wave_sync();
  const int ngc = 6 * nib;
  if (lane < ngc) {
    const int bi = lane / 6, k = lane - 6 * bi;
    double dv = 0.0;
    for (int d = 0; d < ndir; d++) {
      double tmp = 0.0;
      for (int j = 0; j < nic; j++) {
        const int r = d * nic + j;
        const double t = gd[D_IMP + r];
        int kk = -1;
        if (gi[I_ROWOFF + 2*r] == 6 * bi) kk = 0; else if (gi[I_ROWOFF + 2*r + 1] == 6 * bi) kk = 1;
        if (kk >= 0) tmp = tmp + t * gd[D_XJ + 12 * r + 6 * kk + k];
      }
      if (d == 0) dv = tmp; else dv = dv + tmp;
    }
    const int b = gi[I_ISLB + bi];
    gd[D_ST + 13*b + 7 + k] = gd[D_ST + 13*b + 7 + k] + dv;
  }
#if MHW_REPORT
  // contact_impulse += (cn, cs, ct) (ICH:298-327; oracle apply_impulses): the impact side only -- the stabiliser's call (ndir == 1) moves positions and
  // leaves no impulse (CStab:457).  Lane j owns contact gi[I_ISLC + j]; the contacts of an island are distinct.
  if (ndir == 3 && lane < nic) {
    const int ci = gi[I_ISLC + lane];
    for (int d = 0; d < 3; d++) g_racc[3*ci + d] = g_racc[3*ci + d] + gd[D_IMP + d * nic + lane];
  }
#endif
  wave_sync();
}
// update_constraint_velocities_from_impulses (ICH:427-464); row lanes
MH_DEV double Gab3(int R, int nic, int a, int b, int i, int j) {
  return gd[D_G + (a * nic + i) * R + (b * nic + j)];      // lower blocks are mirrored by compute_problem_data
}
MH_DEV void update_constraint_vels(int nic) {
  nic = uni(nic);
  const int lane = lane_id();
  const int R = 3 * nic;
  double cv = 0.0;
  if (lane < R) {
    const int a = small_div(lane, nic), i = lane - a * nic;
    cv = gd[D_CV + lane];
    for (int b = 0; b < 3; b++) {
      double t = 0.0;
      for (int j = 0; j < nic; j++) t = t + gd[D_IMP + b * nic + j] * Gab3(R, nic, a, b, i, j);
      cv = cv + t;
    }
  }
  wave_sync();
  if (lane < R) gd[D_CV + lane] = cv;
  wave_sync();
}
// q.update_from_stacked_qp(z) (UCPD:218-228) + update_from_stacked (ICH:298-397)
MH_DEV void impulses_from_z_and_apply(int nic, int nib) {
  nic = uni(nic);
  const int lane = lane_id();
  wave_sync();
  if (lane < nic) {
    const int i = lane;
    gd[D_IMP + i] = gd[D_ZSOL + i];
    double s = gd[D_ZSOL + nic + i];   s = s - gd[D_ZSOL + 3 * nic + i]; gd[D_IMP + nic + i] = s;
    double t = gd[D_ZSOL + 2 * nic + i]; t = t - gd[D_ZSOL + 4 * nic + i]; gd[D_IMP + 2 * nic + i] = t;
  }
  wave_sync();
  apply_impulses(nic, nib, 3);
}
MH_DEV double min_cnv(int nic) { const int lane = lane_id(); return wave_min((lane < nic) ? gd[D_CV + lane] : MHW_INF); }

// apply_model_to_connected_constraints (ICH:530-626)
MH_DEV bool apply_model(const Island& isl) {                        // returns true when the handler threw (LCPSolverException)
  const int nic = uni(isl.nic), nib = uni(isl.nib);
  const int lane = lane_id();
  if (3 * nic > MHW_MAX_ROWS) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); return false; }
  unsigned long long t0 = tick();
  const double nrm = compute_problem_data(nic, isl.bodies, 3, 0, true);  // G, and with it the matrix's norm, is the same for both passes
  tock(PH_PDATA, t0);
  double minv = 0.0;
  for (int pass = 0; pass < 2; pass++) {
    { const int rs = solve_impact_lcp(nic, nrm); if (rs <= 0) return rs < 0; }
    t0 = tick();
    impulses_from_z_and_apply(nic, nib);                            // ICH:569 / :600
    if (pass == 1) { tock(PH_APPLY, t0); break; }
    update_constraint_vels(nic);                                    // ICH:572
    minv = min_cnv(nic);                                            // ICH:575
    // apply_restitution(_epd, _z) (ICH:470-491)
    bool ch = false;
    double zr = 0.0;
    if (lane < nic) { zr = gd[D_ZSOL + lane] * gd[D_CEPS + gi[I_ISLC + lane]]; ch = zr > MH_NEAR_ZERO; }
    const bool changed = ballot(ch) != 0ull;
    wave_sync();
    if (lane < nic) gd[D_ZBUF + lane] = zr;
    wave_sync();
    bool again = false;
    if (changed) {
      impulses_from_z_and_apply(nic, nib);                          // ICH:581
      update_constraint_vels(nic);
      const double minv_plus = min_cnv(nic);
      again = (minv_plus < 0.0 && minv_plus < minv - MH_NEAR_ZERO);  // ICH:591
    }
    tock(PH_APPLY, t0);
    if (!again) break;
  }
  return false;
}

#if MHW_NOSLIP
// ---- no-slip model (ImpactConstraintHandler::apply_no_slip_model, ICH:1009-1417), contacts only ----
// The dense algebra is tiny (<= 2 x 6 tangent rows) and sequential by construction (greedy Cholesky
// tests of a growing matrix): lane 0 does it serially over LDS, in exactly the operation order of
// oracle/world.hpp::apply_no_slip_model; only the LCP runs wave-wide.
MH_DEV bool ns_chol_factor(int n, double* A) {                      // oracle/linalg.hpp chol_factor (dpotf2 'L')
  for (int j = 0; j < n; j++) {
    double ajj = A[j + n*j];
    for (int k = 0; k < j; k++) ajj = ajj - A[j + n*k] * A[j + n*k];
    if (!(ajj > 0.0)) return false;
    ajj = sqrt(ajj);
    A[j + n*j] = ajj;
    for (int i = j+1; i < n; i++) {
      double t = A[i + n*j];
      for (int k = 0; k < j; k++) t = t - A[i + n*k] * A[j + n*k];
      A[i + n*j] = t / ajj;
    }
  }
  return true;
}
MH_DEV void ns_chol_solve(int n, const double* L, double* b) {      // oracle/linalg.hpp chol_solve
  for (int k = 0; k < n; k++) {
    b[k] = b[k] / L[k + n*k];
    const double bk = b[k];
    for (int i = k+1; i < n; i++) b[i] = b[i] - bk * L[i + n*k];
  }
  for (int k = n-1; k >= 0; k--) {
    double t = b[k];
    for (int i = k+1; i < n; i++) t = t - L[i + n*k] * b[i];
    b[k] = t / L[k + n*k];
  }
}
MH_DEV int ns_build_Y(int nic, int R, int ns, int nt, bool skew) {  // ICH:1098-1111
  double* Y = gd + D_NSY;
  const int m = ns + nt;
  for (int a = 0; a < ns; a++) for (int b = 0; b < ns; b++) Y[a + m*b] = gd[D_G + (nic + gi[I_NSS + a]) * R + nic + gi[I_NSS + b]];
  for (int a = 0; a < nt; a++) for (int b = 0; b < nt; b++) Y[(ns + a) + m*(ns + b)] = gd[D_G + (2*nic + gi[I_NST + a]) * R + 2*nic + gi[I_NST + b]];
  for (int a = 0; a < ns; a++) for (int b = 0; b < nt; b++) {
    const double g = gd[D_G + (nic + gi[I_NSS + a]) * R + 2*nic + gi[I_NST + b]];
    Y[a + m*(ns + b)] = g; Y[(ns + b) + m*a] = g;
  }
  if (skew) for (int j = 0; j < m; j++) Y[j + m*j] = Y[j + m*j] - MH_NEAR_ZERO;
  return m;
}
// builds the Schur-complement LCP (dense MM row-major at D_NSMM, qq at D_NSQ); keeps the Cholesky
// factor of Y, Q X X' and Y^-1 X v for the back-substitution.  Returns 0 if Y is not PD.
MHW_FN int noslip_setup(int nic) {
  nic = uni(nic);
  const int R = 3 * nic;
  wave_sync();
  if (lane_id() == 0) {
    double* Y = gd + D_NSY; double* QX = gd + D_NSQX; double* W = gd + D_NSW; double* col = gd + D_NST2; double* YXv = gd + D_NSYXV;
    int ns = 0, nt = 0;
    for (int i = 0; i < nic; i++) {                                 // greedy largest non-singular tangent set (ICH:1087-1145)
      gi[I_NSS + ns] = i; ns++;
      int m = ns_build_Y(nic, R, ns, nt, true);
      if (!ns_chol_factor(m, Y)) ns--;
      gi[I_NST + nt] = i; nt++;
      m = ns_build_Y(nic, R, ns, nt, true);
      if (!ns_chol_factor(m, Y)) nt--;
    }
    const int m = ns_build_Y(nic, R, ns, nt, false);               // ICH:1166-1183
    int ok = ns_chol_factor(m, Y) ? 1 : 0;
    if (ok) {
      for (int i = 0; i < nic; i++) {                               // Q X X' (ICH:1198-1203)
        for (int a = 0; a < ns; a++) QX[i*m + a] = gd[D_G + i * R + nic + gi[I_NSS + a]];
        for (int a = 0; a < nt; a++) QX[i*m + ns + a] = gd[D_G + i * R + 2*nic + gi[I_NST + a]];
      }
      for (int j = 0; j < nic; j++) {                               // W = Y^-1 (Q X X')' (ICH:1210-1211)
        for (int a = 0; a < m; a++) col[a] = QX[j*m + a];
        ns_chol_solve(m, Y, col);
        for (int a = 0; a < m; a++) W[a + m*j] = col[a];
      }
      for (int i = 0; i < nic; i++) for (int j = 0; j < nic; j++) { // MM = Cn X Cn' - QX W (ICH:1190-1215)
        double acc = 0.0;
        for (int a = 0; a < m; a++) acc = acc + QX[i*m + a] * W[a + m*j];
        gd[D_NSMM + i*nic + j] = gd[D_G + i * R + j] - acc;
      }
      for (int a = 0; a < ns; a++) YXv[a] = gd[D_CV + nic + gi[I_NSS + a]];     // Y^-1 [Cs v(S); Ct v(T)] (ICH:1222-1232)
      for (int a = 0; a < nt; a++) YXv[ns + a] = gd[D_CV + 2*nic + gi[I_NST + a]];
      ns_chol_solve(m, Y, YXv);
      for (int i = 0; i < nic; i++) {                               // qq = Cn v - QX YXv (ICH:1217-1236)
        double acc = 0.0;
        for (int a = 0; a < m; a++) acc = acc + QX[i*m + a] * YXv[a];
        gd[D_NSQ + i] = gd[D_CV + i] - acc;
      }
    }
    gi[I_NSM] = ok ? m : -1; gi[I_NSNS] = ns;
  }
  wave_sync();
  return geti(I_NSM) >= 0 ? 1 : 0;
}
// [cs; ct] = -(Y^-1 X v + Y^-1 (QX)' cn) scattered over the S / T sets (ICH:1293-1308); cn is in D_IMP[0..nic)
MHW_FN void noslip_finish(int nic) {
  nic = uni(nic);
  wave_sync();
  if (lane_id() == 0) {
    const int m = gi[I_NSM], ns = gi[I_NSNS], nt = m - ns;
    double* Y = gd + D_NSY; double* QX = gd + D_NSQX; double* t2 = gd + D_NST2; double* YXv = gd + D_NSYXV;
    for (int a = 0; a < m; a++) {
      double acc = 0.0;
      for (int i = 0; i < nic; i++) acc = acc + QX[i*m + a] * gd[D_IMP + i];
      t2[a] = acc;
    }
    ns_chol_solve(m, Y, t2);
    for (int i = 0; i < nic; i++) { gd[D_IMP + nic + i] = 0.0; gd[D_IMP + 2*nic + i] = 0.0; }
    for (int a = 0; a < ns; a++) gd[D_IMP + nic + gi[I_NSS + a]] = -(YXv[a] + t2[a]);
    for (int a = 0; a < nt; a++) gd[D_IMP + 2*nic + gi[I_NST + a]] = -(YXv[ns + a] + t2[ns + a]);
  }
  wave_sync();
}
// apply_no_slip_model_to_connected_constraints (ICH:236-295)
MH_DEV bool apply_no_slip_model_to_island(const Island& isl) {      // returns true when the handler threw (the assert of ICH:1184-1186, std::runtime_error of ICH:1282)
  const int nic = uni(isl.nic), nib = uni(isl.nib);
  const int lane = lane_id();
  if (3 * nic > MHW_MAX_ROWS || nic > MHW_NS_MAXC) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); return false; }
  unsigned long long t0 = tick();
  compute_problem_data(nic, isl.bodies, 3, 0, false);
  tock(PH_PDATA, t0);
  t0 = tick();
  if (!noslip_setup(nic)) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_LCP_FAILED); wave_sync(); return true; }   // assert(success), ICH:1184-1186
  tock(PH_MBUILD, t0);
  t0 = tick();
  const int n = nic;
  const int zsize = geti(I_VNS_SIZE);
  const double qi = (lane < n) ? gd[D_NSQ + lane] : 0.0;
  double zi = (lane < MH_NOSLIP_MAX) ? gd[D_VNS + lane] : 0.0;
  if (lane >= n) zi = 0.0;
  const ChainOut co = world_lcp_chain(2, nic, n, qi, zi, zsize, 0.0, PolyIndex());   // lcp_fast(_MM, _qq, _v), then the Lemke ladder (ICH:1239, 1281)
  account(n, uni(co.piv));
  tock(PH_LCP, t0);
  if (!uni(co.ok)) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_LCP_FAILED); wave_sync(); return true; }
  t0 = tick();
  wave_sync();
  if (lane < n) { gd[D_VNS + lane] = co.zi; gd[D_IMP + lane] = co.zi; }
  seti(I_VNS_SIZE, n);
  noslip_finish(nic);
  apply_impulses(nic, nib, 3);                                      // ICH:1351-1385
  update_constraint_vels(nic);                                      // ICH:265
  const double minv = min_cnv(nic);
  // apply_restitution(q) (ICH:497-525)
  bool ch = false; double cn = 0.0;
  if (lane < nic) { cn = gd[D_IMP + lane] * gd[D_CEPS + gi[I_ISLC + lane]]; ch = cn > MH_NEAR_ZERO; }
  const bool changed = ballot(ch) != 0ull;
  wave_sync();
  if (lane < nic) gd[D_IMP + lane] = cn;
  if (changed) {
    if (lane < nic) { gd[D_IMP + nic + lane] = 0.0; gd[D_IMP + 2*nic + lane] = 0.0; }
    wave_sync();
    apply_impulses(nic, nib, 3);                                    // update_from_stacked(q) (ICH:274)
    update_constraint_vels(nic);
    const double minv_plus = min_cnv(nic);
    // ICH:284-291 would re-solve and then read the D-S solver's _z, which this path never sized
    if (minv_plus < 0.0 && minv_plus < minv - MH_NEAR_ZERO) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); }
  }
  wave_sync();
  tock(PH_APPLY, t0);
  return false;
}
#endif

// calc_impacting_unilateral_constraint_forces + apply_model (CSim:298-355, ICH:96-168)
// An exception of the impact handler -- LCPSolverException (ICH-QP:225), std::runtime_error (ICH:1282), the assert of ICH:1184-1186 -- is caught nowhere
// between apply_model and main() (CSim:342-350 catches ImpactToleranceException only): it unwinds process_constraints, do_mini_step and step, and the run of
// that simulator is over.  So: the islands after the failing one are not processed, the tolerance check is not reached, the mini-step does not advance
// current_time (TSS:215), the step does not stabilise, and a world that carries MH_WORLD_LCP_FAILED is not stepped again (oracle World::handle_impacts / step).
// The throw travels up as a return value (a uniform register): only world_step's entry test reads the status word from LDS.
MH_DEV bool thrown() { return (uni(geti(I_STATUS)) & MH_WORLD_LCP_FAILED) != 0; }
MH_DEV bool handle_impacts(int nc) {                                // nc: the contacts of the constraint list; returns true when the handler threw
  nc = uni(nc);
  const int lane = lane_id();
  if (nc == 0) return false;
  const uint64_t impacting = ballot(lane < nc && contact_vn(lane) < -MH_NEAR_ZERO);
  if (impacting == 0ull) return false;
  IslandSearch search = islands_begin(nc);
  // islands share no enabled body, so applying the model island by island equals the
  // reference's "filter inactive groups first, then apply" (UC:1197-1225, ICH:107-151).  For the same reason the bodies of an island still have the
  // velocities `impacting` was taken at when the island's turn comes: its contacts' normal velocities are those of that ballot, not computed again.
  uint64_t active_contacts = 0;
  while (true) {
    const unsigned long long ti = tick();
    Island isl;
    const bool more = next_island(nc, search, isl);
    tock(PH_ISLANDS, ti);
    if (!more) break;
    const int nic = isl.nic;
    if ((impacting & isl.contacts) == 0ull) continue;               // remove_inactive_groups
    const bool all_inf = ballot(lane < nic && gd[D_CMU + gi[I_ISLC + (lane < nic ? lane : 0)]] < 1e2) == 0ull;
    active_contacts |= isl.contacts;
#if MHW_NOSLIP
    if (all_inf) { if (apply_no_slip_model_to_island(isl)) return true; continue; }    // ICH:134-135
#else
    if (all_inf) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); continue; }   // variant built without the no-slip model
#endif
    if (apply_model(isl)) return true;
  }
  if (ballot(lane < nc && ((active_contacts >> lane) & 1ull) && contact_vn(lane) < -MH_NEAR_ZERO) != 0ull) {
    seti(I_STATUS, geti(I_STATUS) | MH_WORLD_IMPACT_TOL); wave_sync();
  }
  return false;
}

// ---- time stepping ----------------------------------------------------------------------------------
// fills the constraint list from the sim pair list (CSim:488-537)
MH_DEV int find_unilateral_constraints(int npairs) {               // npairs: the length of the pair list; returns the number of contacts
  npairs = uni(npairs);
  const int lane = lane_id();
#if MHW_REPORT
  for (int e = lane; e < 3 * MHW_MAX_CONTACTS; e += 64) g_racc[e] = 0.0;    // a new constraint list: no contact has received an impulse yet
#endif
  ContactGeom c; c.has = 0; c.g1 = 0; c.g2 = 0; c.pt = v3(0, 0, 0); c.n = v3(0, 0, 0); c.dist = 0.0;
  int p = 0;
  const double thresh = gd[D_THRESH];
  bool spk = false;
#if MHW_BOX
  int nc = gen_contacts(I_PAIRS, npairs, 0);
  if (nc < 0) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); nc = 0; }
  if (lane < npairs) { int a, b; pair_bodies(gi[I_PAIRS + lane], a, b); spk = is_spokes(a); }
  (void)c; (void)p; (void)thresh;
#else
  if (lane < npairs) {
    p = gi[I_PAIRS + lane];
    int pa_, pb_; pair_bodies(p, pa_, pb_);
    spk = is_spokes(pa_);
    // CSim:488-537 takes pairs with signed distance < thresh and lets find_contacts (tolerance thresh) produce the
    // contact.  For the closed-form sphere pairs the contact routine computes that very distance (same operands, same
    // operations: len - rA - rB, cp.y - r), so one evaluation serves both tests.
    if (!spk) { c = contact_geom(p, thresh); if (c.has && !(c.dist < thresh)) c.has = 0; }
  }
  const uint64_t m = ballot(c.has != 0);
  int nc = popc(m);
  wave_sync();
  if (nc > MHW_MAX_CONTACTS) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); nc = 0; }
  else if (c.has) store_contact(popc(m & lanes_below(lane)), p, c.g1, c.g2, c.pt, c.n, c.dist);
#endif
#if MHW_NOSLIP
  { uint64_t sm = ballot(spk);                                      // spokes pairs come last in the pair list
    while (sm) { const int k = ctz(sm); sm &= sm - 1; nc = spoke_contacts(geti(I_PAIRS + k), nc); } }
#endif
  wave_sync();
  return nc;
}
#if MHW_NOSLIP
// The conservative-advancement loop of do_mini_step for a world that is ONE spokes body over the plane
// (BASELINE config 3).  That loop is where the rimless wheel spends its time -- ~330 sub-steps per step,
// see DESIGN.md -- and every pass only moves the wheel along its (constant) velocity and re-measures the
// six tips.  Here the whole loop runs out of registers, redundantly on every lane: coordinates, the
// loop-invariant Euler rates, the plane frame and the tip table are loaded once, nothing touches LDS until
// the result is written back.  Same statements, same operation order as broad_phase / pair_geom / ca_step /
// integrate_positions, so the states stay bit-identical to the generic loop (and to the oracle).
MH_DEV double wheel_ca_loop(double dt) {
  const double min_step = gd[D_MINSTEP];
  const int lane = lane_id();
  double q[7], qs[7], pl[12];
#pragma unroll
  for (int k = 0; k < 7; k++) { q[k] = gd[D_ST + k]; qs[k] = gd[D_QSAVE + k]; }
#pragma unroll
  for (int k = 0; k < 9; k++) pl[k] = gd[D_PLANE_R + k];
#pragma unroll
  for (int k = 0; k < 3; k++) pl[9 + k] = gd[D_PLANE_O + k];
  const int N = geti(I_NSPOKES);
  const double mytx = (lane < MH_MAX_SPOKES) ? gd[D_SPK + 2*lane] : 0.0, mytz = (lane < MH_MAX_SPOKES) ? gd[D_SPK + 2*lane + 1] : 0.0;
  const V3 vl = Vl(0), wa = Wa(0);
  // Euler rates at the saved coordinates with their quaternion normalised (integrate_positions: set_coords(qsave), euler_vel)
  double qd[7];
  { const double nrm = sqrt(((qs[3]*qs[3] + qs[4]*qs[4]) + qs[5]*qs[5]) + qs[6]*qs[6]);
    const double x = qs[3] / nrm, y = qs[4] / nrm, z = qs[5] / nrm, ww = qs[6] / nrm;
    qd[0] = vl.x; qd[1] = vl.y; qd[2] = vl.z;
    qd[3] = 0.5 * ((ww * wa.x + z * wa.y) - y * wa.z);
    qd[4] = 0.5 * ((ww * wa.y + x * wa.z) - z * wa.x);
    qd[5] = 0.5 * ((ww * wa.z + y * wa.x) - x * wa.y);
    qd[6] = 0.5 * (((-x * wa.x) - y * wa.y) - z * wa.z); }
  double h = 0.0;
  unsigned guard = 0;
  while (h < dt) {
    if (++guard > MH_CA_HARD_CAP) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_STALLED); break; }
    // pair_geom (spokes): lowest tip in the plane frame, first one wins ties
    const double x = q[3], y = q[4], z = q[5], w = q[6];
    double R[9];
    R[0] = 1.0 - 2.0 * (y*y + z*z); R[1] = 2.0 * (x*y - z*w);       R[2] = 2.0 * (x*z + y*w);
    R[3] = 2.0 * (x*y + z*w);       R[4] = 1.0 - 2.0 * (x*x + z*z); R[5] = 2.0 * (y*z - x*w);
    R[6] = 2.0 * (x*z - y*w);       R[7] = 2.0 * (y*z + x*w);       R[8] = 1.0 - 2.0 * (x*x + y*y);
    const V3 c = v3(q[0], q[1], q[2]);
    // one spoke per lane (lane i < N), then the first-index minimum across lanes -- the same tip wins as in the
    // serial scan of pair_geom, and its coordinates are broadcast with v_readlane
    double min_dist; V3 pa, ppm;
    { const double px = mytx, py = 0.0, pz = mytz;
      const V3 tip = v3(c.x + ((R[0]*px + R[1]*py) + R[2]*pz), c.y + ((R[3]*px + R[4]*py) + R[5]*pz), c.z + ((R[6]*px + R[7]*py) + R[8]*pz));
      const V3 d = tip - v3(pl[9], pl[10], pl[11]);
      const V3 pp = v3((pl[0]*d.x + pl[3]*d.y) + pl[6]*d.z, (pl[1]*d.x + pl[4]*d.y) + pl[7]*d.z, (pl[2]*d.x + pl[5]*d.y) + pl[8]*d.z);
      int imin; argmin_first(pp.y, lane < N, min_dist, imin);
      if (imin > 63) { imin = 0; min_dist = MHW_INF; }
      pa = v3(read_lane(tip.x, imin), read_lane(tip.y, imin), read_lane(tip.z, imin));
      ppm = v3(read_lane(pp.x, imin), min_dist, read_lane(pp.z, imin)); }
    // ca_step (spokes): in contact "never"; otherwise dist / (n0 . velocity of the body point at the origin), _rmax = 0
    double CA = MHW_INF;
    if (!(min_dist <= 0.0)) {
      const V3 pp = v3(ppm.x, 0.0, ppm.z);
      const V3 pb = v3(pl[9] + ((pl[0]*pp.x + pl[1]*pp.y) + pl[2]*pp.z), pl[10] + ((pl[3]*pp.x + pl[4]*pp.y) + pl[5]*pp.z), pl[11] + ((pl[6]*pp.x + pl[7]*pp.y) + pl[8]*pp.z));
      const V3 d0 = pa - pb;
      const V3 n0 = d0 / norm(d0);
      const V3 xd0 = vl + cross(c, wa);
      const double tB = dot(n0, xd0) + norm(cross(wa, n0)) * 0.0;
      double total = 0.0 + tB;
      if (total < 0.0) total = 0.0;
      const double cand = min_dist / total;
      CA = (cand < MHW_INF) ? cand : MHW_INF;
    }
    if (CA <= 0.0) break;
    double tc = (min_step > CA) ? min_step : CA;
    tc = ((dt - h) < tc) ? (dt - h) : tc;
    // integrate_positions(h + tc): q = qsave + (h + tc) * rates, quaternion normalised
    const double hh = h + tc;
    double qn[7];
#pragma unroll
    for (int k = 0; k < 7; k++) { qn[k] = qd[k] * hh; qn[k] = qn[k] + qs[k]; }
    const double nrm = sqrt(((qn[3]*qn[3] + qn[4]*qn[4]) + qn[5]*qn[5]) + qn[6]*qn[6]);
    q[0] = qn[0]; q[1] = qn[1]; q[2] = qn[2];
    q[3] = qn[3] / nrm; q[4] = qn[4] / nrm; q[5] = qn[5] / nrm; q[6] = qn[6] / nrm;
    h += tc;
  }
  wave_sync();
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < 7; k++) gd[D_ST + k] = q[k];
    gi[I_PAIRS] = 0;                                                 // the (wheel, ground) pair, as broad_phase leaves it (do_mini_step: its length, 1)
  }
  wave_sync();
  return h;
}
#endif

#if MHW_REPORT
// Folds the mini-step's contacts into the step's rows, where ConstraintSimulator::constraint_post_callback_fn sees them (CSim:353): after handle_impacts
// returned without a throw, also when it returned early (the contacts then count with zero impulse).  Lane p owns pair slot p and walks the constraint
// list in its order, so the order of a row's additions is fixed and no two lanes share a row.
MH_DEV void report_fold(int nc) {                                  // nc: the contacts of the constraint list
  const int lane = lane_id();
  double* rep = g_rep;
  wave_sync();
  if (!rep || lane >= gi[I_NPT]) return;
  int a, b; pair_bodies(lane, a, b);                                // a < b: the row holds the impulse on body a
  double* row = rep + MH_REPORT_PAIR * lane;
  for (int c = 0; c < nc; c++) {
    if (gi[I_CPAIR + c] != lane) continue;
    const double cn = g_racc[3*c], cs = g_racc[3*c + 1], ct = g_racc[3*c + 2];
    const V3 n = Cdir(c, 0), s = Cdir(c, 1), t = Cdir(c, 2), pt = Cpt(c);
    const V3 jv = (n * cn + s * cs) + t * ct;
    const double sg = (gi[I_CG1 + c] == a) ? 1.0 : -1.0;
    row[0] = row[0] + 1.0;
    row[1] = row[1] + cn;
    row[2] = row[2] + sg * jv.x; row[3] = row[3] + sg * jv.y; row[4] = row[4] + sg * jv.z;
    row[5] = row[5] + pt.x * cn; row[6] = row[6] + pt.y * cn; row[7] = row[7] + pt.z * cn;
  }
}
#endif

// a world that is ONE spokes body over the plane: wheel_ca_loop's case.  (Read from the image where it is needed: found once in the kernel entry and handed
// down as a value, it made the wheel leg 1.2 % slower than this form, ranges apart -- DESIGN.md 4.1.)
MH_DEV bool lone_wheel() {
#if MHW_NOSLIP
  return geti(I_NB) == 1 && geti(I_NTOT) == 2 && geti(I_GEOM) == MH_GEOM_SPOKES;
#else
  return false;
#endif
}
MH_DEV double do_mini_step(double dt, bool& threw) {               // TSS:114-222; threw: the impact handler's exception left the mini-step before TSS:215
  const int lane = lane_id();
  wave_sync();
  if (lane < gi[I_NB]) for (int k = 0; k < 7; k++) gd[D_QSAVE + 7*lane + k] = gd[D_ST + 13*lane + k];
  wave_sync();
  double h = 0.0;
  const double min_step = gd[D_MINSTEP];
  // the length of the pair list travels as a value to the constraint list and the impact handler; gi[I_NPAIRS] is written once, below, for the
  // stabiliser, which reads it after the step's last mini-step
  int npairs = 0;
#if MHW_NOSLIP
  if (lone_wheel()) { const unsigned long long tw = tick(); h = uni(wheel_ca_loop(dt)); tock(PH_BROAD_CA, tw); npairs = 1; }   // (the loop leaves the one-pair list)
  else
#endif
  for (unsigned guard = 0; h < dt; ) {
    if (++guard > MH_CA_HARD_CAP) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_STALLED); wave_sync(); break; }
    unsigned long long t0 = tick();
    npairs = broad_phase(dt - h, I_PAIRS);
    const double e = (lane < npairs) ? ca_step(gi[I_PAIRS + lane]) : MHW_INF;   // TSS:272-331
    const double CA = wave_min(e);
    tock(PH_BROAD_CA, t0);
    if (CA <= 0.0) break;
    t0 = tick();
    double tc = (min_step > CA) ? min_step : CA;
    tc = ((dt - h) < tc) ? (dt - h) : tc;
    integrate_positions(h + tc);
    h += tc;
    tock(PH_INTEGRATE, t0);
  }
  seti(I_NPAIRS, npairs);
  unsigned long long t1 = tick();
  integrate_velocities(h);
  tock(PH_FWDDYN, t1);
  t1 = tick();
  const int nc = find_unilateral_constraints(npairs);
  tock(PH_CONTACTS, t1);
  threw = handle_impacts(nc);
  if (threw) return h;
#if MHW_REPORT
  report_fold(nc);
#endif
  if (lane == 0) gd[D_TIME] = gd[D_TIME] + h;
  count(CN_MINI, 1ull);
  wave_sync();
  return h;
}

// ---- constraint stabilisation ----------------------------------------------------------------------
// pairwise distances over the SIM pair list: lane k <-> k-th pair (CStab:88-131)
struct UniEval { double vmin, uC; };
MHW_FN UniEval eval_unilateral() {
  const int lane = lane_id();
  UniEval r; r.uC = MHW_INF;
  if (lane < geti(I_NPAIRS)) { const PairGeom g = pair_geom(gi[I_PAIRS + lane]); r.uC = g.dist; }
  r.vmin = wave_min(r.uC);
  return r;
}
MH_DEV double eval_at(double t, int idx) {                         // CStab:1281-1298
  set_q_from(D_QV, D_DQV, t, 1);
  const UniEval e = eval_unilateral();
  return read_lane(e.uC, idx);
}
MH_DEV double sign2(double x, double y) { return (y > 0.0) ? fabs(x) : -fabs(x); }
MH_DEV double ridders(double x1, double x2, double fl, double fh, int idx) {   // CStab:1322-1379
  idx = uni(idx);
  const double TOL = 1e-4;
  double ans = MHW_INF, fm, fnew, s, xh, xl, xm, xnew;
  if ((fl > 0.0 && fh < 0.0) || (fl < 0.0 && fh > 0.0)) {
    xl = x1; xh = x2;
    for (unsigned j = 0; j < 25; j++) {
      xm = 0.5 * (xl + xh);
      fm = eval_at(xm, idx);
      s = sqrt(fm * fm - fl * fh);
      if (s == 0.0) return ans;
      xnew = xm + (xm - xl) * ((fl >= fh ? 1.0 : -1.0) * fm / s);
      ans = xnew;
      fnew = eval_at(ans, idx);
      if (fabs(fnew) < TOL && fnew >= 0.0) return xnew;
      if (sign2(fm, fnew) != fm) { xl = xm; fl = fm; xh = ans; fh = fnew; }
      else if (sign2(fl, fnew) != fl) { xh = ans; fh = fnew; }
      else if (sign2(fh, fnew) != fh) { xl = ans; fl = fnew; }
    }
  } else {
    if (fl == 0.0) return x1;
    if (fh == 0.0) return x2;
  }
  return 0.0;
}
MH_DEV int update_q() {                                            // CStab:1056-1216 (unilateral part)
  const int lane = lane_id();
  const int npairs = geti(I_NPAIRS);
  const double uC_old = eval_unilateral().uC;
  set_q_from(D_QV, D_DQV, 1.0, 0);
  double uC = eval_unilateral().uC;
  const bool br = (lane < npairs) && ((uC_old < 0.0 && uC > 0.0) || (uC_old > 0.0 && uC < 0.0));
  const uint64_t brm = ballot(br);
  double t = 1.0;
  { uint64_t m = brm;
    while (m) {
      const int i = ctz(m); m &= m - 1;
      const double root = uni(ridders(0.0, t, read_lane(uC_old, i), read_lane(uC, i), i));
      if (root > 0.0 && root < 1.0) t = (root < t) ? root : t;
    } }
  set_q_from(D_QV, D_DQV, t, 1);
  uC = eval_unilateral().uC;
  const double BETA = 0.6;
  while (true) {
    const bool bad = (lane < npairs) && !br && uC < 0.0 && uC_old > uC;
    if (ballot(bad) == 0ull) break;
    t *= BETA;
    if (t < MH_NEAR_ZERO) return 0;
    set_q_from(D_QV, D_DQV, t, 1);
    uC = eval_unilateral().uC;
  }
  // q = qstar (the un-normalised dq*t + q, as the reference keeps it)
  wave_sync();
  if (lane < gi[I_NB]) for (int k = 0; k < 7; k++) { const double v = gd[D_DQV + 7*lane + k] * t; gd[D_QV + 7*lane + k] = v + gd[D_QV + 7*lane + k]; }
  wave_sync();
  return 1;
}
// The loop of CStab:167-254 once the entry test has found a violated pair.  Out of line: its prologue saves ~50 callee-saved VGPRs
// to scratch, which is what every step of a world at rest used to pay (13 KB per world-step, 10 of the 13.7 GB a 200-step launch
// of the sphere-stack batch wrote) before the entry test moved into the inlined wrapper below.
MHW_FN void stabilize_work(double max_uvio) {
  const int lane = lane_id();
  const unsigned max_it = (unsigned)geti(I_CSTAB_MAXIT);
  const int nb = geti(I_NB);
  const double cstab_eps = gd[D_CSTABEPS];
  wave_sync();
  if (lane < nb) {                                                 // save_velocities / get_body_configurations (CStab:181-184)
    for (int k = 0; k < 6; k++) gd[D_VSAVE + 6*lane + k] = gd[D_ST + 13*lane + 7 + k];
    for (int k = 0; k < 7; k++) gd[D_QV + 7*lane + k] = gd[D_ST + 13*lane + k];
  }
  wave_sync();
  unsigned iterations = 0;
  while (max_uvio < cstab_eps) {
    if (iterations == max_it) break;
    if (iterations == MH_CSTAB_HARD_CAP) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_STALLED); wave_sync(); break; }
    wave_sync();
    if (lane < nb) { for (int k = 0; k < 6; k++) gd[D_ST + 13*lane + 7 + k] = 0.0; for (int k = 0; k < 7; k++) gd[D_DQV + 7*lane + k] = 0.0; }
    wave_sync();
    // compute_problem_data (CStab:347-492): own broad phase (dt = 0), one contact per pair
    const int ncp = broad_phase(0.0, I_SCR);
    ContactGeom c; c.has = 0; c.g1 = 0; c.g2 = 0; c.pt = v3(0, 0, 0); c.n = v3(0, 0, 0); c.dist = 0.0;
    int p = 0;
    bool spk = false;
    PairGeom g; g.dist = 0.0; g.a = 0; g.b = 0; g.pa = v3(0, 0, 0); g.pb = v3(0, 0, 0);
#if MHW_BOX
    int nc = gen_contacts(I_SCR, ncp, 1);
    if (nc < 0) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); break; }
    if (lane < ncp) { p = gi[I_SCR + lane]; int a, b; pair_bodies(p, a, b); spk = is_spokes(a); if (spk) g = pair_geom(p); }
    (void)c;
#else
    if (lane < ncp) {
      p = gi[I_SCR + lane];
      g = pair_geom(p);
      spk = is_spokes(g.b);
      if (spk) { }                                                 // spokes pairs: appended in pair order below
      else if (g.dist >= MH_NEAR_ZERO) {                           // separated: synthetic contact (CStab:316-331)
        const V3 nn = g.pb - g.pa;
        c.n = nn / norm(nn); c.pt = g.pa; c.g1 = g.a; c.g2 = g.b; c.dist = g.dist; c.has = 1;
      } else c = contact_geom(p, MH_NEAR_ZERO);
    }
    const uint64_t m = ballot(c.has != 0);
    int nc = popc(m);
    wave_sync();
    if (nc > MHW_MAX_CONTACTS) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); break; }
    if (c.has) store_contact(popc(m & lanes_below(lane)), p, c.g1, c.g2, c.pt, c.n, c.dist);
#endif
#if MHW_NOSLIP
    { uint64_t sm = ballot(spk);
      bool over = false;
      while (sm) {
        const int k = ctz(sm); sm &= sm - 1;
        const double dk = read_lane(g.dist, k);
        if (dk >= MH_NEAR_ZERO) {                                  // synthetic contact: geom1 = ground, point = wheel tip,
          if (nc >= MHW_MAX_CONTACTS) { over = true; break; }      // normal = ground point - wheel tip (CStab:316-331)
          wave_sync();
          if (lane == k) { const V3 nn = g.pb - g.pa; store_contact(nc, p, g.a, g.b, g.pa, nn / norm(nn), g.dist); }
          wave_sync();
          nc++;
        } else nc = spoke_contacts(geti(I_SCR + k), nc);
      }
      if (over) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); break; } }
#endif
    wave_sync();
    IslandSearch search = islands_begin(nc);
    while (true) {
      Island isl;
      if (!next_island(nc, search, isl)) break;
      const int nic = isl.nic, nib = isl.nib;
      const int n_ = nic;
      if (n_ > MHW_MAX_ROWS) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); continue; }
      compute_problem_data(nic, isl.bodies, 1, 1, false);
      if (n_ > geti(I_NMAX)) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_UNSUPPORTED); wave_sync(); continue; }
      // determine_dq (CStab:932-970): MM = Cn X Cn', qq = dist - |eps| - NEAR_ZERO; cold lcp_fast, then Lemke ladder
      double qi = 0.0;
      if (lane < n_) qi = gd[D_CDIST + gi[I_ISLC + lane]] - fabs(cstab_eps) - MH_NEAR_ZERO;
      wave_sync();
      const ChainOut co = world_lcp_chain(1, nic, n_, qi, 0.0, 0, 0.0, PolyIndex());   // fresh local z: cold start
      const double zi = co.zi; const int zsize = uni(co.zsize);
      account(n_, uni(co.piv)); count(CN_SROWS, (unsigned long long)n_);
      // update_from_stacked(pd, z): cn = z[0..nc) (zeros where z is shorter)
      wave_sync();
      if (lane < n_) gd[D_IMP + lane] = (lane < zsize) ? zi : 0.0;
      wave_sync();
      apply_impulses(nic, nib, 1);
      // dq of the island's bodies = their Euler-form velocities (CStab:962-969)
      if (lane < nib) { const int b = gi[I_ISLB + lane]; double qd[7]; euler_vel(b, qd); for (int k = 0; k < 7; k++) gd[D_DQV + 7*b + k] = qd[k]; }
      wave_sync();
    }
    if (!update_q()) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_STAB_FAILED); wave_sync(); break; }
    max_uvio = eval_unilateral().vmin;
    iterations++;
    count(CN_STAB, 1ull);
  }
  wave_sync();
  if (lane < nb) for (int k = 0; k < 6; k++) gd[D_ST + 13*lane + 7 + k] = gd[D_VSAVE + 6*lane + k];
  wave_sync();
}

MH_DEV void stabilize() {                                          // CStab:167-254
  if (geti(I_CSTAB_MAXIT) == 0) return;
  const double max_uvio = eval_unilateral().vmin;
  if (!(max_uvio < gd[D_CSTABEPS])) return;                        // nothing to do: velocities and q are untouched
  stabilize_work(max_uvio);
}

MH_DEV bool world_step(double dt) {                                // TSS:52-111; returns true when the impact handler threw (the world's run is over)
  // TSS:60 runs the broad phase at the step's start.  The first pass of do_mini_step's advancement loop runs it again with dt - 0.0 on the same state and
  // overwrites the same list, so the call is made in two cases only:
  //   * a step without a mini-step, !(0.0 < dt): stabilize() is the reader -- eval_unilateral measures the pairs of this list, gi[I_NPAIRS] of them;
  //   * the lone wheel, whose wheel_ca_loop takes the place of the advancement loop and runs no broad phase.  NOTHING reads this list there either:
  //     wheel_ca_loop leaves the same one-pair list when it ends (gi[I_PAIRS] = 0, length 1: the (wheel, ground) pair is appended unconditionally) and
  //     broad_phase has no other effect.  The call stays so that the wheel's step makes the calls the parent's made, no more and no fewer; whoever
  //     removes it has the wheel objects' timing to show for it, not a result to fear for.
  if (lone_wheel() || !(0.0 < dt)) { seti(I_NPAIRS, broad_phase(dt, I_PAIRS)); wave_sync(); }
  double h = 0.0;
  unsigned guard = 0;
  while (h < dt) {
    bool threw = false;
    h += uni(do_mini_step(dt - h, threw));
    if (threw) return true;
    if (++guard > 100000u) { seti(I_STATUS, geti(I_STATUS) | MH_WORLD_STALLED); wave_sync(); break; }
  }
  const unsigned long long ts = tick();
  stabilize();
  tock(PH_STAB, ts);
  count(CN_STEPS, 1ull);
  return false;
}

// ---- the kernel: one wavefront (= one 64-thread workgroup) per world ------------------------------
__global__ __launch_bounds__(64, MHW_WAVES_PER_SIMD)
void mh_k_world_step(const mh_scene* __restrict__ scp, int B, double dt, int nsteps, double* __restrict__ state,
                     mh_world_aux* __restrict__ aux, double* __restrict__ traj, int nmax, double* __restrict__ lu_ws, int ka,
                     unsigned long long* __restrict__ prof, const int* __restrict__ ids
#if MHW_FORCES
                     , const mh_world_forces* __restrict__ frc, const double* __restrict__ wrench, int wrows   // stored terms (or NULL), rows x B x nb x 6 wrench (or NULL)
#endif
#if MHW_REPORT
                     , double* __restrict__ report                                                            // B x nsteps x npt x MH_REPORT_PAIR rows (or NULL)
#endif
                     )
{
  const int w = ids ? ids[blockIdx.x] : (int)blockIdx.x;      // ids: a subset of the batch in its own launch (mh_world_batch_step_ids)
  if ((unsigned)w >= (unsigned)B) return;                     // B: the worlds of the BATCH (an id outside it is ignored, never dereferenced)
  const int lane = lane_id();
  const mh_scene& sc = *scp;
#if MHW_STATICS
  // the statics record follows the spoke-tip table behind the scene record (mh_world.hip lays all three out in one allocation)
  const mh_world_statics& sst = *reinterpret_cast<const mh_world_statics*>(reinterpret_cast<const double*>(scp + 1) + 2 * MH_MAX_SPOKES);
#endif
  // `pv` is where the cache fill below takes the scene's VALUES from; counts, types, enabled pairs, cone edges and tolerances are always `sc`'s / `sst`'s
#if MHW_PARAMS
  // the B per-world records follow the statics record (scene | spoke tips | statics | params[B]); w is the world's index in the batch, also under ids
  static_assert((sizeof(mh_scene) + 2 * MH_MAX_SPOKES * sizeof(double) + sizeof(mh_world_statics)) % 8 == 0 && sizeof(mh_world_params) % 8 == 0, "params records must be 8-byte aligned");
  const mh_world_params& pv = reinterpret_cast<const mh_world_params*>(&sst + 1)[w];
#define MHW_ST_R(k) pv.st_R[k]
#define MHW_ST_O(k) pv.st_o[k]
#define MHW_ST_DIM(k) pv.st_dim[k]
#else
  const mh_scene& pv = sc;
#define MHW_ST_R(k) sst.R[k]
#define MHW_ST_O(k) sst.o[k]
#define MHW_ST_DIM(k) sst.dim[k]
#endif
#if MHW_STATICS
  const int hg = sc.has_ground ? 1 : 0, nst_ = sst.n;
  const int nb = sc.nb, ntot = sc.nb + hg + nst_, npt = ntot * (ntot - 1) / 2;
  if (nb < 1 || nst_ < 0 || ntot > MH_MAX_BODIES + 1) return;      // (refused at create; never index past the tables)
  if (lane < hg + nst_) {
    const int k = lane - hg;                                        // slot `lane` = body nb + lane: the scene's ground first, static k at has_ground + k
    const bool gr = k < 0;
    gst[lane] = gr ? MH_STATIC_PLANE : sst.type[k];
    for (int q = 0; q < 9; q++) gs[S_R + 9*lane + q] = gr ? pv.plane_R[q] : MHW_ST_R(k)[q];
    for (int q = 0; q < 3; q++) gs[S_O + 3*lane + q] = gr ? pv.plane_o[q] : MHW_ST_O(k)[q];
    const double x = gr ? 0.0 : MHW_ST_DIM(k)[0], y = gr ? 0.0 : MHW_ST_DIM(k)[1], z = gr ? 0.0 : MHW_ST_DIM(k)[2];
    gs[S_DIM + 3*lane] = x; gs[S_DIM + 3*lane + 1] = y; gs[S_DIM + 3*lane + 2] = z;
    const double hx = x / 2.0, hy = y / 2.0, hz = z / 2.0;
    gs[S_RAD + lane] = sqrt((hx*hx + hy*hy) + hz*hz);
  } else if (lane < MH_MAX_STATICS) gst[lane] = -1;
#else
  const int nb = sc.nb, ntot = sc.nb + (sc.has_ground ? 1 : 0), npt = ntot * (ntot - 1) / 2;
#endif
  // scene cache
  if (lane < nb) {
    gi[I_GEOM + lane] = sc.geom_type[lane];
    { const int gt = sc.geom_type[lane];
      const double x = pv.geom_dim[lane][0], y = pv.geom_dim[lane][1], z = pv.geom_dim[lane][2];
      double rad = 0.0, rmax = 0.0;
      if (gt == MH_GEOM_SPHERE) { rad = x; rmax = x; }
      else if (gt == MH_GEOM_BOX) {                                  // CCD.cpp:1056-1063 (half diagonal) / BoxPrimitive.h:44 (full diagonal)
        const double hx = x / 2.0, hy = y / 2.0, hz = z / 2.0;
        rad = sqrt((hx*hx + hy*hy) + hz*hz); rmax = sqrt((x*x + y*y) + z*z);
      }
      gd[D_RADIUS + lane] = rad; gd[D_RMAX + lane] = rmax;
#if MHW_BOX
      gd[D_GDIM + 3*lane] = x; gd[D_GDIM + 3*lane + 1] = y; gd[D_GDIM + 3*lane + 2] = z;
#endif
    }
    gd[D_MASS + lane] = pv.mass[lane];
    for (int k = 0; k < 3; k++) gd[D_INERTIA + 3*lane + k] = pv.inertia[lane][k];
  }
  if (lane < 9) gd[D_PLANE_R + lane] = pv.plane_R[lane];
  if (lane < 3) { gd[D_PLANE_O + lane] = pv.plane_o[lane]; gd[D_GRAV + lane] = pv.gravity[lane]; }
  if (lane < npt) {
    gd[D_PMU + lane] = pv.cp_mu_coulomb[lane]; gd[D_PMUV + lane] = pv.cp_mu_viscous[lane];
    gd[D_PEPS + lane] = pv.cp_epsilon[lane]; gd[D_PCOMP + lane] = pv.cp_compliance[lane];
    gi[I_PNK + lane] = sc.cp_nk[lane]; gi[I_PEN + lane] = sc.pair_enabled[lane];
  }
#if MHW_FORCES
  { const int ft = frc ? frc->terms : 0;
    if (lane < nb) {
      const bool st = (ft & MH_FORCE_STOKES) != 0, dm = (ft & MH_FORCE_DAMPING) != 0;
      gf[F_SB + lane] = st ? frc->stokes_b[lane] : 0.0; gf[F_SBA + lane] = st ? frc->stokes_b_ang[lane] : 0.0;
      gf[F_KL + lane] = dm ? frc->damp_kl[lane] : 0.0; gf[F_KA + lane] = dm ? frc->damp_ka[lane] : 0.0;
      gf[F_KLSQ + lane] = dm ? frc->damp_klsq[lane] : 0.0; gf[F_KASQ + lane] = dm ? frc->damp_kasq[lane] : 0.0;
    }
    if (lane == 0) g_fterms = (ft & (MH_FORCE_STOKES | MH_FORCE_DAMPING)) | (wrench ? MHW_FORCE_WRENCH : 0); }
#endif
  mh_world_aux* a = aux + w;
  if (lane == 0) {
    gd[D_MINSTEP] = sc.min_step_size; gd[D_THRESH] = sc.contact_dist_thresh; gd[D_CSTABEPS] = sc.cstab_eps; gd[D_TIME] = a->time;
    gi[I_NB] = nb; gi[I_NTOT] = ntot; gi[I_NPT] = npt; gi[I_NMAX] = nmax; gi[I_KA] = (ka < MHW_KA_V) ? ka : MHW_KA_V; gi[I_NPAIRS] = 0;
    gi[I_STATUS] = a->status; gi[I_ZLAST_SIZE] = a->zlast_size; gi[I_ZBUF_SIZE] = a->zbuf_size; gi[I_ZBUF_CAP] = a->zbuf_cap;
    gi[I_CSTAB_MAXIT] = (int)sc.cstab_max_iterations;
    gi[I_NSPOKES] = 0; gi[I_VNS_SIZE] = a->vns_size; gi[I_NSM] = 0; gi[I_NSNS] = 0;
    for (int b = 0; b < nb; b++) if (sc.geom_type[b] == MH_GEOM_SPOKES) gi[I_NSPOKES] = (int)sc.geom_dim[b][1];
    g_lu_ws = lu_ws + (size_t)w * nmax * nmax;
    g_cnt[CN_STEPS] = a->steps; g_cnt[CN_MINI] = a->mini_steps; g_cnt[CN_LCP] = a->lcp_solves; g_cnt[CN_ROWS] = a->lcp_rows;
    g_cnt[CN_PIV] = a->lcp_pivots; g_cnt[CN_STAB] = a->stab_iters; g_cnt[CN_BYTES] = a->lcp_alg_bytes; g_cnt[CN_SROWS] = a->stab_rows;
    for (int i = 0; i < PH_COUNT; i++) g_pacc[i] = 0ull;
    g_lcp_prof_on = prof ? 1 : 0; for (int i = 0; i < LP_COUNT; i++) g_lcp_prof[i] = 0ull;
  }
  const int nst = MH_BODY_STATE * nb;
  double* stg = state + (size_t)w * nst;
  for (int e = lane; e < nst; e += 64) gd[D_ST + e] = stg[e];
  if (lane < 32) gi[I_RNG + lane] = (int)a->rng[lane];
  gd[D_ZLAST + lane] = a->zlast[lane]; gd[D_ZBUF + lane] = a->zbuf[lane];
  if (lane < 4 * nb) gd[D_XQ + lane] = __longlong_as_double(0x7ff8000000000000ll);   // no X block cached yet (NaN never compares equal)
#if MHW_NOSLIP
  { const double* spk = reinterpret_cast<const double*>(scp + 1);   // spoke tips follow the scene record (host libm)
    if (lane < 2 * MH_MAX_SPOKES) gd[D_SPK + lane] = spk[lane];
    if (lane < MH_NOSLIP_MAX) gd[D_VNS + lane] = a->vns[lane]; }
#endif
  wave_sync();
  bool dead = thrown();                                       // a world whose handler threw in an earlier launch is not stepped again
  for (int s = 0; s < nsteps; s++) {
#if MHW_FORCES
    if (wrench && !dead && (s == 0 || wrows > 1)) {            // this step's wrench row of THIS world (its index in the batch, also under ids): rows == 1 holds row 0
      wave_sync();
      if (lane < 6 * nb) gf[F_WR + lane] = wrench[((size_t)(wrows > 1 ? s : 0) * B + w) * (size_t)(6 * nb) + lane];
      wave_sync();
    }
#endif
#if MHW_REPORT
    // this step's rows of THIS world (its index in the batch, also under ids) start at zero, each zeroed by the lane that folds into it; a world that
    // is passed over keeps them zero
    wave_sync();
    { double* rows = report ? report + ((size_t)w * nsteps + s) * (size_t)npt * MH_REPORT_PAIR : nullptr;
      if (lane == 0) g_rep = rows;
      if (rows && lane < npt) for (int k = 0; k < MH_REPORT_PAIR; k++) rows[MH_REPORT_PAIR * lane + k] = 0.0; }
    wave_sync();
#endif
    if (!dead) dead = world_step(dt);
    if (traj) {
      wave_sync();
      for (int e = lane; e < 7 * nb; e += 64) { const int b = e / 7, k = e - 7 * b; traj[(((size_t)w * nsteps + s) * nb + b) * 7 + k] = gd[D_ST + 13 * b + k]; }
    }
  }
  wave_sync();
  for (int e = lane; e < nst; e += 64) stg[e] = gd[D_ST + e];
  if (lane < 32) a->rng[lane] = (uint32_t)gi[I_RNG + lane];
  a->zlast[lane] = gd[D_ZLAST + lane]; a->zbuf[lane] = gd[D_ZBUF + lane];
#if MHW_NOSLIP
  if (lane < MH_NOSLIP_MAX) a->vns[lane] = gd[D_VNS + lane];
  if (lane == 0) a->vns_size = gi[I_VNS_SIZE];
#endif
  if (lane == 0) {
    a->zlast_size = gi[I_ZLAST_SIZE]; a->zbuf_size = gi[I_ZBUF_SIZE]; a->zbuf_cap = gi[I_ZBUF_CAP]; a->status = gi[I_STATUS]; a->time = gd[D_TIME];
    a->steps = g_cnt[CN_STEPS]; a->mini_steps = g_cnt[CN_MINI]; a->lcp_solves = g_cnt[CN_LCP]; a->lcp_rows = g_cnt[CN_ROWS];
    a->lcp_pivots = g_cnt[CN_PIV]; a->stab_iters = g_cnt[CN_STAB]; a->lcp_alg_bytes = g_cnt[CN_BYTES]; a->stab_rows = g_cnt[CN_SROWS];
    if (prof) { for (int i = 0; i < LP_COUNT; i++) g_pacc[PH_LP0 + i] = g_lcp_prof[i]; for (int i = 0; i < PH_COUNT; i++) prof[(size_t)w * PH_COUNT + i] = g_pacc[i]; }
  }
}

#undef MHW_FN
#undef MHW_ST_R
#undef MHW_ST_O
#undef MHW_ST_DIM
#undef plane_body
#undef box_plane_pair
} } // namespace mh::MHW_NS

// ---- what the host side (mh_world.hip) sees of this code object (mh_world_variant, mh_host.h): the launch of its kernel, the occupancy query for it, and the
// upload of the __constant__ tables, of which every code object has a copy of its own.  The kernel is named here only: the host holds no typed kernel pointer. ----
// the trailing arguments stand under the switches of the kernel's own parameter list; a field this build has no parameter for is ignored
#if MHW_FORCES
#define MHW_FORCES_ARGS(a) , (a).forces, (a).wrench, (a).wrench_rows
#else
#define MHW_FORCES_ARGS(a)
#endif
#if MHW_REPORT
#define MHW_REPORT_ARGS(a) , (a).report
#else
#define MHW_REPORT_ARGS(a)
#endif
static hipError_t launch(const mh_world_launch& a)
{
  hipLaunchKernelGGL(mh::MHW_NS::mh_k_world_step, dim3(a.grid), dim3(64), 0, a.stream,
                     a.scene, a.B, a.dt, a.nsteps, a.state, a.aux, a.traj, a.nmax, a.lu_ws, a.ka, a.prof, a.ids MHW_FORCES_ARGS(a) MHW_REPORT_ARGS(a));
  return hipGetLastError();
}
static hipError_t occupancy(int* blocks_per_cu)
{
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, mh::MHW_NS::mh_k_world_step, 64, 0);
}
static hipError_t upload_tables(const void* fric, size_t fric_bytes, const void* pow10, size_t pow10_bytes)
{
  if (fric_bytes != sizeof(mh::FricTable) || pow10_bytes != sizeof(mh::Pow10Table)) return hipErrorInvalidValue;
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(mh::c_fric), fric, fric_bytes);
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(mh::c_pow10), pow10, pow10_bytes);
  return e;
}

const mh_world_variant* MHW_VARIANT_GETTER()
{
  static const mh_world_variant v = { launch, occupancy, mh::MHW_NS::PH_COUNT, upload_tables };
  return &v;
}
