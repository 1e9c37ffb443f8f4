/* moby_hip.h -- C ABI of libmoby_hip.so, the MI355X (gfx950) many-worlds
 * contact-dynamics core that stands in for Moby's LCP / impact-handling hot
 * path.  Plain pointers and sizes only; no C++ or torch types cross this line.
 *
 * The reference has no plugin boundary around this path; each
 * entry point below names the C++ seam of /root/reference it replaces.
 * INTEGRATION.md shows the reference-side adapter (a Moby::LCP-shaped C++
 * class, moby_amd/cpp/MobyHipLCP.h) that a maintainer links instead of
 * src/LCP.cpp.
 *
 * Conventions
 *   - all matrices are column-major doubles (Ravelin::MatrixNd::data()/
 *     leading_dim()), all vectors contiguous doubles;
 *   - functions return MH_OK (0) or a negative MH_ERR_* code and never throw;
 *     mh_last_error() returns a thread-local message for the last failure;
 *   - `_dev` entry points take DEVICE pointers and enqueue on `stream`
 *     (a hipStream_t, NULL = default stream) without synchronising;
 *     the unsuffixed ones take HOST pointers, copy, run and synchronise;
 *   - per-problem outputs: status[b] = 1 where the reference solver would
 *     return true, 0 where it would return false (it never throws,
 *     include/Moby/LCP.h:21-27);
 *   - every world carries its own libc rand() stream (32 uint32 words,
 *     mh_rand_seed(state, 1) == a fresh process of the reference).
 */
#ifndef MOBY_HIP_H
#define MOBY_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MH_OK 0
#define MH_ERR_INVALID_ARG   (-1)
#define MH_ERR_UNSUPPORTED_N (-2)  /* n outside the range the kernels cover */
#define MH_ERR_HIP           (-3)  /* a HIP runtime call failed */
#define MH_ERR_NO_DEVICE     (-4)

#define MH_RAND_WORDS 32
#define MH_LCP_MAX_N_WAVE 64       /* one-wavefront-per-problem solver (M in LDS); also the many-worlds limit */
#define MH_LCP_MAX_N_BLOCK 4096    /* n above MH_LCP_MAX_N_WAVE: one 256-thread workgroup per problem, M read in
                                      place from HBM, LU scratch in an HBM workspace of B (n^2 + 5n) doubles */

/* solver selector: include/Moby/LCP.h:21-27 */
#define MH_LCP_FAST       0  /* LCP::lcp_fast              src/LCP.cpp:41   */
#define MH_LCP_FAST_REG   1  /* LCP::lcp_fast_regularized  src/LCP.cpp:212  */
#define MH_LCP_LEMKE      2  /* LCP::lcp_lemke (dense)     src/LCP.cpp:545  */
#define MH_LCP_LEMKE_REG  3  /* LCP::lcp_lemke_regularized src/LCP.cpp:353  */

/* trace encoding (optional pivot trace, one int32 stream per problem)
 *   lcp_fast : +(i+1) variable i moved basic->nonbasic, -(i+1) the reverse
 *   lcp_lemke: (entering+1), (leaving+1) per pivot
 *   0x40000000|k : start of attempt k of a regularised wrapper (0 = lambda 0) */
#define MH_TRACE_ATTEMPT 0x40000000

typedef struct mh_lcp_opts {
  int      min_exp;   /* regularised wrappers: first exponent (default -20)   */
  unsigned step_exp;  /* exponent step (lcp_fast_regularized default 4)       */
  int      max_exp;   /* exclusive upper exponent                             */
  double   piv_tol;   /* <= 0: solver default (LCP.cpp:761)                   */
  double   zero_tol;  /* <= 0: solver default (LCP.cpp:58,228,570)            */
} mh_lcp_opts;

/* library / device ------------------------------------------------------- */
/* 100 * major + minor.  101: mh_impact_batch_lu_work / mh_big_batch_lu_work fill B x 4 doubles per call (100: B x 2) -- a caller built against the
 * two-column layout must check for >= 101 and size its buffer accordingly (#define MH_VERSION is what this header describes). */
#define MH_VERSION 102   /* 102: recurrent forces and per-world body wrenches in the many-worlds stepper (mh_world_forces, mh_world_batch_set_forces / _step_wrench) */
/* Box-sphere contacts between free bodies in the many-worlds stepper (mh_world_batch_create accepts scenes with such pairs enabled; "Box-sphere pairs"
 * below) add no entry point and change no layout, so MH_VERSION stays 102; a caller that needs to know tests this macro, and at run time
 * mh_world_batch_create's answer to such a scene (MH_ERR_INVALID_ARG from a library without the feature). */
#define MH_WORLD_BOX_SPHERE 1
int         mh_version(void);
const char* mh_last_error(void);
int         mh_device_count(void);
/* Devices.  One process may drive every GPU of a node: worlds are independent, so a batch of B worlds is split
 * into one batch per device and nothing but per-interval counters crosses devices (moby_amd/cpp/example_multi_gpu.cpp: one
 * batch + stream per device, the counters reduced with RCCL's ncclAllReduce).
 *   - a batch (mh_world_batch, mh_big_batch, mh_impact_batch, mh_artic_batch) lives on the device that is CURRENT in the calling
 *     thread when its `create` runs (mh_device_set, or hipSetDevice in a HIP program); `mh_*_batch_device` returns it;
 *   - every later entry point that takes the batch runs on THAT device, whatever device the calling thread has current at the
 *     time: the library switches to the batch's device for the call and restores the caller's before it returns;
 *   - a `stream` argument must belong to the batch's device (HIP refuses the launch otherwise: MH_ERR_HIP); device pointers
 *     handed to a batch's entry points (traj_dev, ids_dev, `device_ptrs` results) are that device's;
 *   - the stateless entries (mh_lcp_solve_batch[_dev], mh_world_step_batch, mh_impact_process_batch) run on the current device. */
int         mh_device_get(void);        /* the calling thread's current device, or MH_ERR_NO_DEVICE */
int         mh_device_set(int device);  /* 0 <= device < mh_device_count(); MH_ERR_INVALID_ARG otherwise, MH_ERR_NO_DEVICE without a GPU */

/* glibc srand(seed) state for one world (host helper, no GPU needed) */
void        mh_rand_seed(uint32_t* state32, uint32_t seed);
/* next rand() of that stream (host helper; used by adapters and tests) */
int         mh_rand_next(uint32_t* state32);

/* B independent dense LCPs  w = M z + q, w,z >= 0, w'z = 0  of equal size n.
 * Replaces Moby::LCP::{lcp_fast, lcp_fast_regularized, lcp_lemke,
 * lcp_lemke_regularized} (include/Moby/LCP.h:21-27; callers
 * src/ImpactConstraintHandlerQP.cpp:219,224, src/ConstraintStabilization.cpp:954-955,
 * src/ImpactConstraintHandler.cpp:1239-1281).
 *
 *   M       B matrices, problem b at M + b*strideM, leading dimension ld >= n
 *   q       B*n
 *   z       B*n, in/out: warm start in (only read where z_size_in[b] == n),
 *           solution out
 *   z_size_in   B ints or NULL (= all n): z.size() on entry.  lcp_fast
 *           warm-starts iff it equals n (LCP.cpp:65); lcp_lemke draws n rand()
 *           values iff it differs from n (LCP.cpp:564-567,611-621)
 *   z_size_out  B ints or NULL: z.size() on return (2n after some Lemke
 *           failures, LCP.cpp:840-903)
 *   rng     B*32 words in/out (mh_rand_seed)
 *   status  B ints; pivots B unsigned (LCP::pivots) or NULL
 *   trace   B*trace_cap int32 or NULL; trace_len B ints or NULL
 */
int mh_lcp_solve_batch_dev(void* stream, int kind, int B, int n,
                           const double* M, int ld, long strideM,
                           const double* q, double* z,
                           const int* z_size_in, int* z_size_out,
                           uint32_t* rng, int* status, unsigned* pivots,
                           int32_t* trace, int trace_cap, int* trace_len,
                           const mh_lcp_opts* opts);

int mh_lcp_solve_batch(int kind, int B, int n,
                       const double* M, int ld, long strideM,
                       const double* q, double* z,
                       const int* z_size_in, int* z_size_out,
                       uint32_t* rng, int* status, unsigned* pivots,
                       int32_t* trace, int trace_cap, int* trace_len,
                       const mh_lcp_opts* opts);


/* ------------------------------------------------------------------------
 * Many-worlds stepping: B independent instances of one scene topology.
 * Replaces, per world, TimeSteppingSimulator::step (src/TimeSteppingSimulator.cpp:
 * 52-222), ConstraintSimulator::{broad_phase, calc_pairwise_distances,
 * find_unilateral_constraints, calc_impacting_unilateral_constraint_forces}
 * (src/ConstraintSimulator.cpp:298-537), ImpactConstraintHandler::
 * process_constraints (src/ImpactConstraintHandler.cpp:75) with the Drumwright-
 * Shell QP->LCP model (src/ImpactConstraintHandlerQP.cpp:94-497) and
 * ConstraintStabilization::stabilize (src/ConstraintStabilization.cpp:167).
 *
 * Scene scope of this build: up to MH_MAX_BODIES free rigid bodies with sphere,
 * box (against the plane and against spheres) or rimless-wheel spokes geometry plus
 * one static plane (the closed-form pairs of CCD.inl:804-886, 1164-1259 and of example/
 * rimless-wheel/coldet-plugin.cpp), gravity, per-pair ContactParameters; impact
 * models: Drumwright-Shell QP->LCP and, for islands whose contacts all have
 * mu-coulomb >= 100, the no-slip model (ImpactConstraintHandler.cpp:1009-1417).
 * Body ids are 0..nb-1 in the order the reference sorts them (by id string); the
 * ground plane, when present, has id nb.  Pair p enumerates (i<j) lexicographically.
 *
 * Box-sphere pairs.  A pair of two enabled bodies, one MH_GEOM_BOX and one MH_GEOM_SPHERE, may be enabled and is stepped.  Pair p = (i < j) keeps its
 * bodies in id order everywhere; the box is the reference's geometry A of the CONTACT whichever body has the lower id (CCD.inl:15,26 swaps the
 * arguments so that it is).  The frames are the bodies' own: box centre = the body's COM, box axes = the rotation of its quaternion (a box body has no
 * primitive offset).  With c the sphere's centre in the box's frame, h the half lengths, R the radius, p = clamp(c, -h, h) (the fixed point of the
 * reference's projected-gradient QP, BoxPrimitive.cpp:183-254), v = p - c:
 *   contact          find_contacts_box_sphere (CCD.inl:1208-1259), created as (box, sphere): contact_geom1 = the box, contact_geom2 = the sphere, the
 *                    normal points from the sphere towards the box.  If any |p_i| < h_i or |v| < R (every face and edge region, and every
 *                    penetration): dist = -min(min_i(h_i - |p_i|), R - |v|), the sphere point stays c + v; otherwise (a vertex region) the sphere
 *                    point is c + v R / |v| and dist = the distance between the two points.  None if dist > TOL.  dist > 0: the point is the
 *                    midpoint of the two points, the normal their difference box - sphere normalised, or -- when that is no longer than
 *                    NEAR_ZERO -- the unit vector from the sphere's centre to p.  dist <= 0: the sphere point and that unit vector.  A centre
 *                    inside the box gives v = 0 and a NaN normal, as in the reference; there is no fallback.  A pair gives at most one contact.
 *   signed distance  BoxPrimitive::calc_signed_dist for a sphere (BoxPrimitive.cpp:256-276, 788-836), a DIFFERENT function: the closest-point
 *                    distance of c (the negative interior depth when c is inside) minus R; box point = p, sphere point = centre + v (R + min(dist, 0))
 *                    / |v|, the centre if |v| = 0.  With the sphere as the lower id, SpherePrimitive::calc_signed_dist(Primitive)
 *                    (SpherePrimitive.cpp:282-290) forwards to the box with the point arguments swapped, so the points stay with their bodies:
 *                    the first point is on body i, the second on body j.  The contact list reads THIS distance for its
 *                    < contact_dist_thresh test (ConstraintSimulator.cpp:488-537) and then the contact function's own for the contact.
 *   conservative     the pair contains a sphere: the sphere rule (CCD.cpp:121-235).  dist > NEAR_ZERO -> dist / max(0, calc_max_dist(i, -n0, rmax_i)
 *   advancement      + calc_max_dist(j, n0, rmax_j)), n0 from the signed-distance function's two points, j to i; rmax of the box is its full
 *                    diagonal, of the sphere its radius.  dist <= NEAR_ZERO: the contact above with TOL = NEAR_ZERO, as for sphere pairs.
 *   stabiliser       one row per pair: dist >= NEAR_ZERO -> the synthetic contact at body i's closest point with normal (pb - pa) / |pb - pa|;
 *                    otherwise the contact above with TOL = NEAR_ZERO.  The line search reads the signed distance.
 *   broad phase      the swept-bounds overlap test like any other pair; the box's bounding radius is its half diagonal.
 * Canonical contact order is unchanged: pairs in pair-list order, a pair's contacts in generator order.  Such a scene steps through code objects of its
 * own (mh_world_large_bsp.hip, mh_world_large_bsp_forces.hip: the large variant built with MHW_BSP); every other scene launches what it did.
 * NOT built: box against box (mh_world_batch_create refuses an enabled box-box pair) and the pair in the large-world stepper (moby_hip_stack.h), which
 * keeps its refusal.
 *
 * Static bodies.  mh_scene knows one static object, its ground plane.  mh_world_batch_create_statics takes up to MH_MAX_STATICS more (mh_world_statics
 * below): planes and boxes, each with a frame of its own, shared by all worlds of the batch.  Body indices: enabled bodies 0 .. nb-1, the scene's ground
 * (if has_ground) nb as before, static k at nb + has_ground + k.  The scene's pair_enabled / cp_* arrays are read triangularly over
 * ntot = nb + has_ground + n bodies -- the rule that exists, with a larger ntot; C(9, 2) = MH_MAX_PAIRS is why ntot <= MH_MAX_BODIES + 1.  A slot of two
 * statics is ignored whatever it holds.  Per pair kind:
 *   sphere or box body   the closed forms of the ground, over that plane's own R and o: contact CCD.inl:804-886 (sphere: one contact, geom1 = the
 *   against plane k      sphere; box: one per vertex within TOL, geom1 = the plane, normal = -(its normal)); signed distance PlanePrimitive.cpp:338-411;
 *                        conservative advancement CCD.cpp:121-235 (sphere) and CCD.cpp:238-468 (box) with the pair's own plane; stabiliser rows and
 *                        broad phase as for the ground: a plane's bound is infinite.
 *   sphere against       the box is geometry A, as in "Box-sphere pairs" (CCD.inl swaps): contact find_contacts_box_sphere (CCD.inl:1208-1259), created
 *   static box k         as (box, sphere) with contact_geom1 = the static; signed distance BoxPrimitive::calc_signed_dist (BoxPrimitive.cpp:256-276,
 *                        788-836) -- both over R[k] (box axes), o[k] (box centre) and dim[k] instead of a body's quaternion and COM; the sphere has the
 *                        lower index, so the first point is the sphere's.  Conservative advancement: the sphere rule (CCD.cpp:121-235) with
 *                        calc_max_dist = 0 for the static (CCD.cpp:585-609).  Stabiliser: one row per pair, as for box-sphere pairs.  Broad phase: the
 *                        static box's bounding sphere (centre o[k], radius the half diagonal) does not move (CCD.cpp:735-768 rebuilds enabled bodies'
 *                        bounds only); pairs of two disabled bodies are dropped (CCD.cpp:864-866).
 * Canonical contact order is unchanged: pair-list order.  A static never moves, carries no velocity and is no node of an island.  Such a batch steps
 * through code objects of its own (mh_world_large_st.hip, mh_world_large_st_forces.hip: the large variant built with MHW_STATICS); every other batch
 * launches what it did.  NOT built: a box body against a static box (refused while the pair is enabled), static spheres, statics that move within a launch (per-world
 * statics: "Per-world parameters" below),
 * spokes bodies in a scene with statics (the plugin knows one ground), statics in the large-world and articulated steppers.
 */
#define MH_MAX_BODIES 8
#define MH_MAX_PAIRS  36            /* C(MH_MAX_BODIES + 1, 2) */
#define MH_BODY_STATE 13            /* x(3) quat xyzw(4) v(3) omega(3), world axes, at the COM */
#define MH_GEOM_SPHERE 0
#define MH_GEOM_SPOKES 1            /* rimless wheel: N point "spoke tips" at radius R in the body's x-z plane
                                       (example/rimless-wheel/coldet-plugin.cpp:104-137, params.h:4-6); it is
                                       only ever tested against the ground plane, and always (plugin :53-74) */
#define MH_GEOM_BOX 2               /* BoxPrimitive, tested against the ground plane (vertex-plane contacts, CCD.inl:848-886)
                                       and against spheres ("Box-sphere pairs" above); box-box pairs must be disabled */
#define MH_GEOM_PIN 3               /* a body point (geom_dim, body frame) held at the global origin by six frictionless contacts with
                                       normals +-y, +-z, +-x: the collision plugin of example/contact-constrained-pendulum
                                       (contact-constrained-pendulum-coldet-plugin.cpp:53-146).  Large-world stepper (moby_hip_stack.h)
                                       and oracle only; the pair (body, static world) is always a candidate */
#define MH_MAX_SPOKES 8
#define MH_NOSLIP_MAX 16            /* largest no-slip LCP (contacts of one island) whose warm start is kept */

typedef struct mh_scene {
  int    nb;                               /* enabled rigid bodies */
  int    has_ground;                       /* static Plane primitive present */
  int    geom_type[MH_MAX_BODIES];         /* MH_GEOM_* */
  double geom_dim[MH_MAX_BODIES][3];       /* sphere: radius,-,- ; spokes: R, number of spokes, - ; box: xlen, ylen, zlen */
  double mass[MH_MAX_BODIES];
  double inertia[MH_MAX_BODIES][3];        /* body-frame principal inertia (SpherePrimitive.cpp:138-155) */
  double plane_R[9];                       /* row-major rotation of the plane frame; its +Y is the normal (PlanePrimitive) */
  double plane_o[3];
  double gravity[3];                       /* GravityForce accel (GravityForce.cpp:33-69) */
  int    pair_enabled[MH_MAX_PAIRS];       /* 0 = <DisabledPair> */
  double cp_epsilon[MH_MAX_PAIRS];         /* ContactParameters.cpp:98-135 */
  double cp_mu_coulomb[MH_MAX_PAIRS];
  double cp_mu_viscous[MH_MAX_PAIRS];
  double cp_compliance[MH_MAX_PAIRS];
  int    cp_nk[MH_MAX_PAIRS];              /* friction-cone-edges (>= 4) */
  double min_step_size;                    /* TimeSteppingSimulator.cpp:48  (sqrt eps) */
  double contact_dist_thresh;              /* ConstraintSimulator.cpp:56    (1e-6)     */
  double cstab_eps;                        /* ConstraintStabilization.cpp:59 (sqrt eps) */
  unsigned cstab_max_iterations;           /* ConstraintStabilization.cpp:56 (reference: UINT_MAX; here MH_CSTAB_DEFAULT_MAX_ITERATIONS) */
  int    lcp_n_max;                        /* largest LCP the wave solver must hold in LDS (0 = 64); worlds
                                              that exceed it get MH_WORLD_UNSUPPORTED */
} mh_scene;

/* status bits of mh_world_aux.status */
#define MH_WORLD_OK            0
#define MH_WORLD_LCP_FAILED    1   /* LCPSolverException (ImpactConstraintHandlerQP.cpp:225) */
#define MH_WORLD_IMPACT_TOL    2   /* ImpactToleranceException (warned only, ConstraintSimulator.cpp:342) */
#define MH_WORLD_UNSUPPORTED   4   /* island larger than the wave solver covers / unsupported model */
#define MH_WORLD_STAB_FAILED   8   /* update_q gave up (ConstraintStabilization.cpp:230-234) */
#define MH_WORLD_STALLED       16   /* > 100000 zero-length mini-steps in one step, or MH_CSTAB_HARD_CAP stabilisation
                                       iterations in one call (the reference would not return) */
#define MH_CSTAB_HARD_CAP 10000u
/* Default of mh_scene.cstab_max_iterations in EVERY entry path (mh_scene_defaults, the XML loader when the attribute
 * constraint-stabilization-max-iterations is absent, moby_amd/scene.py).  The reference's default is UINT_MAX
 * (ConstraintStabilization.cpp:56); with the restated arithmetic its loop 2-cycles on resting stacks (DESIGN.md 2,
 * deviation 1) and would not return, so the documented default is a cap the loop reaches about once in 1000 steps.
 * A scene that sets the attribute explicitly (e.g. ur10.xml: 0) is honoured as written. */
#define MH_CSTAB_DEFAULT_MAX_ITERATIONS 10u
#define MH_CA_HARD_CAP 10000000u     /* conservative-advancement sub-steps of one mini-step before MH_WORLD_STALLED */

/* persistent per-world solver state (what the reference keeps in the
 * simulator / handler / libc between steps) + counters */
typedef struct mh_world_aux {
  uint32_t rng[MH_RAND_WORDS];     /* libc rand() stream                                   */
  double   time;                   /* Simulator::current_time                              */
  double   zlast[MH_LCP_MAX_N_WAVE];  /* ImpactConstraintHandler::_zlast (ICH-QP:158-162,233) */
  double   zbuf[MH_LCP_MAX_N_WAVE];   /* storage of ImpactConstraintHandler::_z            */
  int      zlast_size;
  int      zbuf_size;              /* _z.size()                                            */
  int      zbuf_cap;               /* entries of zbuf ever written (Ravelin keeps them)    */
  int      status;                 /* MH_WORLD_* bits, sticky                              */
  double   vns[MH_NOSLIP_MAX];     /* ImpactConstraintHandler::_v, the no-slip LCP's z (ICH:1239) */
  int      vns_size;               /* _v.size()                                            */
  int      pad0;
  unsigned long long steps;        /* step() calls                                         */
  unsigned long long mini_steps;   /* do_mini_step calls                                   */
  unsigned long long lcp_solves;   /* impact + stabilisation LCPs solved                   */
  unsigned long long lcp_rows;     /* sum of their dimensions (BASELINE metric "rows")     */
  unsigned long long lcp_pivots;
  unsigned long long stab_iters;
  unsigned long long lcp_alg_bytes;/* sum of 8 (n^2 + 2n): bytes the same solves move through the LCP entry */
  unsigned long long stab_rows;    /* the part of lcp_rows that ConstraintStabilization::determine_dq solved (impact rows = lcp_rows - stab_rows) */
} mh_world_aux;

/* test hooks: key 1 = edge of the LDS-resident LU block of the world kernel (0..64, clamped to what the
 * kernel variant holds: 12 or 16; 0 sends every LU factorisation through the HBM workspace path) */
int  mh_debug_set(int key, int value);   /* key 2: block LCP solver (n > 64) thread geometry -- 0 choose by n and B,
                                            1 = 256 threads per problem, 2 = 1024 threads per problem, 3 / 4 = 64 / 128 threads per problem
                                            (the lcp_lemke kinds with n <= 512 only; the lcp_fast kinds keep the choice of 0);
                                            key 3: lcp_lemke's bases (n > 64) through the structure-exploiting LU (1, default) or the dense one (0);
                                            key 4: the Lemke ladder of the island pipeline in sequence (0), as (world, attempt) tasks (1),
                                                   tasks started beside lcp_fast when n >= 256 (2); 3 (default) = 2, and when the batch fills the chip
                                                   with LCPs of 384..512 rows the tasks follow lcp_fast's launch on a second stream, behind a gate that
                                                   opens once its last workgroup has started; 4 = 3 for LCPs of any size;
                                            key 5: lcp_fast (n > 64) skips the repetitions of a repeating pivot sequence (1, default) or
                                                   runs every iteration (0);
                                            key 6: the structure-exploiting LU reuses the factors of the unchanged leading columns from one Lemke
                                                   pivot to the next (1, default) or factorises every basis from scratch (0).
                                            key 7: ladder tasks started after lcp_fast are handed out by need (1, default) or by block index (0).
                                            key 8: thread geometry of the lcp_fast kinds alone for n <= 512 (0 choose, 1-4 as key 2);
                                            key 9: fixed-base CRB articulated bodies without spheres / stabiliser stepped two worlds per wavefront (1; default 0:
                                                   measured no faster, profiles/r04_a_artic_issue.json).
                                            key 10: lcp_fast in the 1024-thread geometry solves a nonbasic system of up to 191 rows in the registers of
                                                   its sixteen waves (1, default) or through the HBM workspace (0).
                                            key 12: sphere-only articulated bodies stepped by the box kernels (1, for batches created after it; default 0: their own kernels;
                                                   include/moby_hip_artic.h, mh_artic_model.nboxes).
                                            key 13: articulated bodies with link spheres or boxes stepped by the pair kernels (1, for batches created after it; default 0:
                                                   their own kernels; include/moby_hip_artic.h, mh_artic_model.npairs).
                                            key 14: articulated bodies with link spheres, boxes or sphere pairs stepped by the box-sphere kernels (1, for batches created
                                                   after it; default 0: their own kernels; include/moby_hip_artic.h, mh_artic_model.pair_kind).
                                            key 15: world batches that would take the large variant stepped by its box-sphere build, mh_world_large_bsp*.hip (1, for
                                                   batches created after it; default 0: only scenes with an enabled box-sphere pair; for A/B runs).
                                            key 16: world batches that would take the box-sphere build stepped by the statics build, mh_world_large_st*.hip (1, for
                                                   batches created after it; default 0: only batches created with statics; for A/B runs).
                                            key 17: world batches that would take the statics build stepped by the per-world-parameters build, mh_world_large_pw*.hip, every
                                                   record filled from the scene (1, for batches created after it; default 0: only batches created with records; for A/B runs).
                                            key 18: world batches that would take the per-world-parameters build stepped by the contact-report build, mh_world_large_rp*.hip, with
                                                   a NULL report (1, for batches created after it; default 0: only batches created for the report; for A/B runs).
                                            key 19: articulated batches that would take the box-sphere kernels stepped by the contact-report kernels, mh_artic_rp*.hip, with a
                                                   NULL report (1, for batches created after it; default 0: only batches of mh_artic_batch_create_report; for A/B runs;
                                                   include/moby_hip_artic.h, "Contact report").
                                            key 20: articulated batches that would take the contact-report kernels stepped by the per-world-parameters kernels, mh_artic_pw*.hip, with
                                                   B images all equal to the model (1, for batches created after it; default 0: only batches of mh_artic_batch_create_params;
                                                   for A/B runs; include/moby_hip_artic.h, "Per-world parameters").
                                            key 21: articulated batches that would take the per-world-parameters kernels stepped by the link-wrench kernels, mh_artic_wr*.hip, with a
                                                   NULL wrench (1, for batches created after it; default 0: only batches of mh_artic_batch_create_wrench; for A/B runs;
                                                   include/moby_hip_artic.h, "Link wrenches").
                                            None of the switches changes a result */
void mh_scene_defaults(mh_scene* s);   /* zero + the reference's default tolerances */
void mh_world_aux_init(mh_world_aux* a, uint32_t seed);

/* A batch of B worlds resident on the GPU (device copies of the scene, the
 * body states and the per-world solver state).  This is what a batched
 * TimeSteppingSimulator subclass holds instead of B simulator objects.
 *   create    allocates device memory, uploads the scene, initialises every
 *             world's aux record (rand() stream at srand(1))
 *   upload    state: B * nb * MH_BODY_STATE doubles (host); aux: B records or NULL
 *   step      enqueues ONE launch that advances every world by nsteps steps of dt
 *             (TimeSteppingSimulator::step called nsteps times) on `stream`
 *             (hipStream_t, NULL = default); does not synchronise.
 *             traj_dev: optional DEVICE buffer B * nsteps * nb * 7 doubles receiving
 *             the generalized coordinates (x, quat xyzw) after each step -- the rows
 *             programs/regress.cpp:82-93 prints -- or NULL
 *   download  synchronises the device and copies state / aux back (either may be NULL)
 *   device_ptrs  raw device pointers for zero-copy interop (e.g. torch tensors)
 */
typedef struct mh_world_batch mh_world_batch;
int mh_world_batch_create(const mh_scene* scene, int B, mh_world_batch** out);
int mh_world_batch_destroy(mh_world_batch* wb);
/* The per-interval reduction of a multi-GPU run, device side.  Enqueues on `stream` a pass over the batch's solver records
 * that leaves, in DEVICE memory, the MH_COUNTERS-element vectors a collective then reduces over the devices of the node (RCCL:
 * ncclAllReduce(sums, ncclUint64, ncclSum) and (maxs, ncclUint64, ncclMax); moby_amd/cpp/example_multi_gpu.cpp):
 *   [0] steps  [1] lcp_rows  [2] lcp_pivots  [3] worlds with an error bit (MH_WORLD_IMPACT_TOL, a warning, not counted)
 *   [4] lcp_solves  [5] mini_steps  [6] stab_iters  [7] lcp_alg_bytes
 * sums = the totals over this batch's worlds, maxs = the largest value any one world holds (the slowest world of the interval). */
#define MH_COUNTERS 8
int mh_world_batch_counters_dev(mh_world_batch* wb, void* stream, unsigned long long* sums_dev, unsigned long long* maxs_dev);
int mh_world_batch_device(const mh_world_batch* wb);   /* the device the batch lives on (see Devices above) */
int mh_world_batch_upload(mh_world_batch* wb, const double* state, const mh_world_aux* aux);
int mh_world_batch_step(mh_world_batch* wb, void* stream, double dt, int nsteps, double* traj_dev);
/* step of a SUBSET: nsteps x step(dt) of the worlds ids_dev[0 .. count) (a DEVICE array of world indices) on `stream`.  Worlds are
 * independent: a batch may be split over streams, e.g. the few worlds whose solver chain runs to its pivot caps every
 * step in a launch of their own, so that the next interval of the others does not wait for them.  Concurrent launches must not
 * share a world, and the ids of ONE launch must be unique (two wavefronts on one world race); an id outside [0, B) is ignored. */
int mh_world_batch_step_ids(mh_world_batch* wb, void* stream, double dt, int nsteps, const int* ids_dev, int count);
int mh_world_batch_download(mh_world_batch* wb, double* state, mh_world_aux* aux);
int mh_world_batch_device_ptrs(mh_world_batch* wb, double** state_dev, mh_world_aux** aux_dev);
/* diagnostic build of the same launch with in-kernel s_memtime stamps: mean cycles per world spent in
 * each phase (order: broad phase + CA, position integration, forward dynamics, contact generation,
 * islands, problem data, LCP matrix build, LCP solve, impulse application, stabilisation); after the per-phase entries: the slowest
 * and the fastest world's total, the mean world's total and the total of the world at the 99th percentile (if nphase leaves room) */
int mh_world_batch_occupancy(mh_world_batch* wb);   /* diagnostic: resident workgroups per CU (runtime query) */
int mh_world_batch_profile(mh_world_batch* wb, double dt, int nsteps, double* phase_cycles, int nphase);
int mh_world_profile_phase_count(void);            /* entries per world of the stamped launch (the four totals follow them) */

/* Recurrent forces of the scene and per-world body wrenches, inside the step.  Replaces Simulator::precalc_fwd_dyn (src/Simulator.cpp:319-350): the
 * accumulators are cleared, then the simulator's recurrent forces run, then the body's controller, once per MINI-STEP (TimeSteppingSimulator.cpp:173),
 * immediately before that mini-step's forward dynamics: positions are the mini-step's, v and omega still its starting velocities.  For body b (mass m,
 * rotation R of its quaternion, row-major; all vectors in world axes at the COM, as MH_BODY_STATE is) the terms accumulate in this fixed order, every
 * operation rounded on its own, three-term sums as (a + b) + c, an absent term left out (not added as zero):
 *   1. gravity                                   F = g m                                            (no torque)
 *   2. Stokes drag (StokesDragForce.cpp:39-44)   F = F + v (-stokes_b[b])            T = omega (-stokes_b_ang[b])
 *   3. damping (DampingForce.cpp:32-51)          vi = R' v, wi = R' omega, fb = vi (-(kl[b] + |vi| klsq[b])), tb = wi (-(ka[b] + |wi| kasq[b]))
 *                                                F = F + R fb                        T = T + R tb   (T = R tb when it is the first torque term)
 *   4. the caller's wrench (f, tau) of this world, body and schedule row
 *                                                F = F + f                           T = T + tau    (T = tau when it is the first torque term)
 * then xdd = F / m and omega' = Jw^-1 (T - omega x (Jw omega)) -- or Jw^-1 (-(omega x (Jw omega))), the expression of the plain step, when no torque
 * term is present.  The coefficients belong to the SCENE (one set for all worlds of the batch: a DampingForce body without a <Gains> child has zero gains and
 * still carries the term); the wrench is per world.  Conservative advancement, contact generation, the impact handler and the stabiliser never read forces. */
#define MH_FORCE_STOKES  1
#define MH_FORCE_DAMPING 2
typedef struct mh_world_forces {           /* recurrent forces of the scene: shared by all worlds of the batch */
  int    terms;                            /* MH_FORCE_* bits; 0 = none */
  double stokes_b[MH_MAX_BODIES], stokes_b_ang[MH_MAX_BODIES];
  double damp_kl[MH_MAX_BODIES], damp_ka[MH_MAX_BODIES], damp_klsq[MH_MAX_BODIES], damp_kasq[MH_MAX_BODIES];
} mh_world_forces;
/* Stores the scene's recurrent forces in the batch (HOST pointer; copied).  NULL or terms == 0 clears them: the batch launches the plain kernels again.
 * MH_ERR_INVALID_ARG: unknown bits in `terms`, or a non-finite coefficient in an array of a term that is set (all MH_MAX_BODIES entries are looked at:
 * zero the unused ones).  Once stored, mh_world_batch_step, _step_ids and _profile honour them too -- they belong to the scene.  A batch with stored
 * forces, and any launch with a wrench, runs the FORCED code objects (mh_world_{small,wheel,large}_forces.hip: same variants, same launch bounds);
 * mh_world_batch_occupancy then reports those -- it reports the forced kernel while forces are STORED; a batch stepped with a wrench alone also launches the
 * forced object of its variant but is reported as the plain one (to query the forced kernel of such a batch, store any term, ask, and clear it).  The forced launch of _profile is the forced production kernel, which has no stamps: it steps the worlds
 * and reports zero cycles.  Likewise a batch on the box-sphere build (an enabled box-sphere pair, or key 15): there is no stamped build of it, _profile launches
 * the production object (plain or forced), steps the worlds and reports zero cycles; mh_world_batch_occupancy reports the object the batch launches.  Not to be called while a launch of the batch is in flight. */
int mh_world_batch_set_forces(mh_world_batch* wb, const mh_world_forces* host);
/* mh_world_batch_step (ids_dev == NULL: the whole batch, `count` ignored) or _step_ids (ids_dev: a DEVICE array of `count` world indices) with a wrench
 * schedule: wrench_dev is a DEVICE array of rows x B x nb x 6 doubles (fx fy fz tx ty tz; B = the worlds of the BATCH: a world reads the entries at its own
 * index in the batch, also when ids_dev selects a subset).  rows == 1: row 0 holds for the whole launch; rows >= nsteps: every mini-step of step s reads
 * row s.  wrench_dev == NULL: the stored recurrent forces only; with none stored the call IS mh_world_batch_step / _step_ids.  MH_ERR_INVALID_ARG:
 * rows < 1, 1 < rows < nsteps, traj_dev together with ids_dev.  A world carrying MH_WORLD_LCP_FAILED is passed over, as in every launch. */
int mh_world_batch_step_wrench(mh_world_batch* wb, void* stream, double dt, int nsteps, double* traj_dev,
                               const int* ids_dev, int count, const double* wrench_dev, int rows);

/* Host convenience: create + upload + step + download (+ trajectory) + destroy. */
int mh_world_step_batch(const mh_scene* scene, int B, double dt, int nsteps,
                        double* state, mh_world_aux* aux, double* traj);
/* The same under the scene's recurrent forces (NULL or terms == 0: none, which is mh_world_step_batch).  It exists for callers that hold no
 * device memory of their own: the regress runner (moby-hip-regress: a scene file with drag from the reference's command line, trajectory rows on
 * the host) and moby_amd.world.WorldBatch(forces=) go through it; a wrench needs a DEVICE array and therefore a resident batch. */
int mh_world_step_batch_forces(const mh_scene* scene, const mh_world_forces* forces, int B, double dt, int nsteps,
                               double* state, mh_world_aux* aux, double* traj);


/* Static bodies among the free ones ("Static bodies" above).  The record belongs to the SCENE: one set for all worlds of the batch. */
#define MH_WORLD_STATICS 1
#define MH_MAX_STATICS 8
#define MH_STATIC_PLANE 0
#define MH_STATIC_BOX   1
typedef struct mh_world_statics {
  int    n;                               /* 0..MH_MAX_STATICS, nb + has_ground + n <= MH_MAX_BODIES + 1 */
  int    type[MH_MAX_STATICS];            /* MH_STATIC_* */
  double R[MH_MAX_STATICS][9];            /* row-major rotation of the static's frame (plane: +Y is the normal, as plane_R) */
  double o[MH_MAX_STATICS][3];            /* frame origin (box: its centre) */
  double dim[MH_MAX_STATICS][3];          /* box: xlen, ylen, zlen; plane: unused */
} mh_world_statics;
/* mh_world_batch_create with static bodies.  statics == NULL or n == 0: exactly mh_world_batch_create.  MH_ERR_INVALID_ARG (with a message): n outside
 * [0, MH_MAX_STATICS] or nb + has_ground + n > MH_MAX_BODIES + 1; an unknown type; a box with a non-positive edge; an enabled pair of a box body and a
 * static box (box-box); a spokes body in a scene with n > 0.  Every other entry point takes the batch as before; mh_world_batch_occupancy reports the object
 * it launches, and mh_world_batch_profile launches the production object (there is no stamped build) and reports zero cycles. */
int mh_world_batch_create_statics(const mh_scene* scene, const mh_world_statics* statics, int B, mh_world_batch** out);
/* Host convenience: mh_world_step_batch_forces with static bodies (forces and statics may each be NULL). */
int mh_world_step_batch_statics(const mh_scene* scene, const mh_world_forces* forces, int B, double dt, int nsteps,
                                double* state, mh_world_aux* aux, double* traj, const mh_world_statics* statics);


/* Per-world parameters.  The worlds of a batch share one TOPOLOGY -- the scene's nb, has_ground, geom_type, pair_enabled, cp_nk, the three tolerances,
 * cstab_max_iterations, lcp_n_max and the statics' n and type -- and may each carry VALUES of their own: one mh_world_params record per world, which
 * replaces, for that world, the scene's mass / inertia / geom_dim / plane_R / plane_o / gravity / cp_epsilon / cp_mu_coulomb / cp_mu_viscous /
 * cp_compliance and the statics' R / o / dim (same indexing: bodies 0 .. nb-1, pair slots triangular over ntot = nb + has_ground + n, static k).  The
 * record holds doubles only, so nothing in it can become an index.  Rule: world w of such a batch is stepped exactly as a batch of the scene and statics
 * with record w written into them would step it (that is how it is tested: one reference run per world).  The records follow the statics record in the
 * batch's device allocation; the kernel entry copies the entries the scene uses (nb bodies, the pair slots, has_ground + n frames) into the wavefront's
 * own cache at launch and reads nothing of the record afterwards.  The impact model is chosen per island from its contacts' own mu-coulomb, so worlds on
 * either side of mu = 100 may share a batch.
 * A spokes body keeps the SCENE's R and N in every world (the spoke-tip table is evaluated once on the host): its geom_dim row in the record is not read.
 * Its mass, inertia, gravity (the wheel's slope), ground frame and contact parameters are per world like any other body's.
 * A batch created with records steps through code objects of its own (mh_world_large_pw.hip, mh_world_large_pw_forces.hip: the statics build with
 * MHW_PARAMS) whatever its scene -- also a scene that would otherwise take the small or the wheel variant; every other batch launches what it launched.
 * There is no stamped build: mh_world_batch_profile launches the production object, steps the worlds and reports zero cycles; mh_world_batch_occupancy
 * reports the object the batch launches.  Key 17 of mh_debug_set sends batches that would take the statics build through these objects with every record
 * equal to the scene (A/B runs; no result changes).
 * NOT built: per-world parameters inside the small and wheel variants (such batches take the objects above); per-world topology (nb, geometry types,
 * enabled pairs, cp_nk, number or type of statics); per-world spoke radius or count; statics that move within a launch; per-world parameters in the
 * large-world stepper (moby_hip_stack.h; the articulated stepper has its own record, moby_hip_artic.h "Per-world parameters"); per-world drag
 * coefficients (mh_world_forces stays the scene's). */
/* (no existing layout changes, so MH_VERSION stays 102; a caller that needs to know tests this macro) */
#define MH_WORLD_PARAMS 1
typedef struct mh_world_params {
  double mass[MH_MAX_BODIES];
  double inertia[MH_MAX_BODIES][3];
  double geom_dim[MH_MAX_BODIES][3];       /* sphere: radius,-,- ; box: xlen, ylen, zlen ; spokes: NOT READ (the scene's R and N hold in every world) */
  double plane_R[9];
  double plane_o[3];
  double gravity[3];
  double cp_epsilon[MH_MAX_PAIRS];
  double cp_mu_coulomb[MH_MAX_PAIRS];
  double cp_mu_viscous[MH_MAX_PAIRS];
  double cp_compliance[MH_MAX_PAIRS];
  double st_R[MH_MAX_STATICS][9];          /* mh_world_statics.R / o / dim of this world */
  double st_o[MH_MAX_STATICS][3];
  double st_dim[MH_MAX_STATICS][3];
} mh_world_params;                         /* 335 doubles, 2680 bytes */
/* The record that reproduces the shared scene (statics == NULL: the st_* rows are zero).  Host helper, no GPU needed. */
void mh_world_params_from_scene(const mh_scene* scene, const mh_world_statics* statics, mh_world_params* out);
/* mh_world_batch_create_statics with one record per world (HOST pointer, B records; copied).  params == NULL: exactly mh_world_batch_create_statics.
 * Otherwise, after the refusals of the scene and the statics (which stay as they are: box-box, spokes beside statics, sizes), every record is validated as
 * the shared values are: for each body of the scene mass and inertia > 0, a sphere's radius > 0, a box's three edges > 0 (a spokes body's row is not
 * looked at); gravity finite; with has_ground the ground frame finite; the four contact parameters of every pair slot finite; each static's frame
 * finite and a static box's edges > 0 and finite.  MH_ERR_INVALID_ARG with a message that names the world and the field; the checks run before the
 * device is looked for. */
int mh_world_batch_create_params(const mh_scene* scene, const mh_world_statics* statics, const mh_world_params* params, int B, mh_world_batch** out);
/* Replaces the records of worlds first .. first + count - 1 (HOST pointer, `count` records), validated as at create; synchronous.  Not to be called while
 * a launch of the batch is in flight, like mh_world_batch_set_forces.  MH_ERR_INVALID_ARG: a batch created without records, a range outside the batch, a
 * refused record (none is then written). */
int mh_world_batch_set_params(mh_world_batch* wb, const mh_world_params* host, int first, int count);
/* The same from DEVICE memory, as an asynchronous copy on `stream`: ordered with the launches of that stream, for a caller that randomises on the GPU
 * between launches.  The records are NOT validated.  What a bad value does: that world's state goes non-finite or the world gets a status bit
 * (MH_WORLD_STALLED, MH_WORLD_LCP_FAILED, MH_WORLD_STAB_FAILED); nothing outside the world's own memory is touched, because every index, count and
 * loop bound of the kernel comes from the shared scene or from integers the kernel computes itself, and every loop a non-finite value can reach ends by
 * a cap (MH_CA_HARD_CAP, the 100000 mini-step guard, MH_CSTAB_HARD_CAP, the solvers' pivot caps, Ridders' iteration count) or by a comparison that is
 * false for NaN.  The other worlds of the batch are not affected. */
int mh_world_batch_set_params_dev(mh_world_batch* wb, void* stream, const mh_world_params* dev, int first, int count);
/* Host convenience: mh_world_step_batch_statics with per-world records (forces, statics and params may each be NULL). */
int mh_world_step_batch_params(const mh_scene* scene, const mh_world_forces* forces, const mh_world_statics* statics, const mh_world_params* params,
                               int B, double dt, int nsteps, double* state, mh_world_aux* aux, double* traj);


/* Contact report.  What the reference hands to ConstraintSimulator::constraint_post_callback_fn (ConstraintSimulator.cpp:353) -- the step's contact
 * constraints, each with the contact_impulse that ImpactConstraintHandler::update_from_stacked accumulated (ImpactConstraintHandler.cpp:298-327) --
 * reduced per PAIR inside the step and left in device memory.  For world w (its index in the BATCH, also under ids_dev, as the wrench schedule is
 * indexed), step s of the launch and pair slot p (the scene's triangular index over ntot = nb + has_ground + n bodies, npt = ntot (ntot - 1) / 2 slots)
 * there is one row of MH_REPORT_PAIR doubles at report_dev[((w * nsteps + s) * npt + p) * MH_REPORT_PAIR].  The rows of a step start at zero and
 * accumulate over the step's mini-steps, in mini-step order.
 * A mini-step's contacts are folded once handle_impacts has returned without a throw (the point of CSim:353), in constraint-list order (canonical:
 * pair-list order, then generator order) -- also when the handler returned early because nothing was impacting: its contacts then count, with zero
 * impulse.  A mini-step whose handler threw is not folded: the step's rows keep what earlier mini-steps left.  Every step of a world that is passed
 * over (MH_WORLD_LCP_FAILED) writes zero rows.  A world with MH_WORLD_UNSUPPORTED or MH_WORLD_STALLED has undefined rows from then on, as its state is.
 * Contact c of pair p = (i < j) carries accumulated (cn, cs, ct): zeroed when the list is built; every application of impulses of the impact side adds
 * to them (QP model, restitution passes, no-slip model; oracle/world.hpp Contact::imp is the same quantity, moby_hip_impact.h returns it per contact);
 * the stabiliser's corrections add nothing.  It adds to the row:
 *   [0]     += 1.0                  contacts, summed over mini-steps
 *   [1]     += cn
 *   [2..4]  += sign * jv            jv = (n cn + s cs) + t ct componentwise, every product and sum rounded on its own, n / s / t the stored normal and
 *                                   tangents; sign = +1 if contact_geom1 is body i, otherwise -1: the impulse ON THE LOWER-INDEX BODY of the pair, in world
 *                                   axes (body j received the negative; against the ground or a static, i is the body)
 *   [5..7]  += pt * cn              the contact point weighted by its normal impulse: the centre of pressure is [5..7] / [1]
 * Entries of disabled or never-touching slots stay 0.
 * Such a batch steps through code objects of its own (mh_world_large_rp.hip, mh_world_large_rp_forces.hip: the per-world-parameters build with
 * MHW_REPORT) whatever its scene; every other batch launches what it launched.  There is no stamped build: mh_world_batch_profile reports zero cycles.
 * Key 18 of mh_debug_set sends batches that would take the per-world-parameters build through these objects with a NULL report (A/B runs; no result
 * changes).
 * NOT built: the report inside the small and wheel variants (such batches take the objects above, as batches with records take theirs); per-contact
 * lists (the row is per pair); the angular impulse about the centre of mass ([5..7] gives the lever); the report in the large-world stepper
 * (moby_hip_stack.h; the articulated stepper has its own, per slot: moby_hip_artic.h, "Contact report"); the stabiliser's corrections (they move positions and carry no impulse in the reference either,
 * ConstraintStabilization.cpp:457). */
/* (no existing layout changes, so MH_VERSION stays 102; a caller that needs to know tests this macro) */
#define MH_WORLD_REPORT 1
#define MH_REPORT_PAIR 8
/* mh_world_batch_create_params with the report build.  params == NULL fills every record from the scene (as key 17 does); mh_world_batch_set_params
 * then refuses, as for any batch created without records.  The refusals are mh_world_batch_create_params' and run before the device is looked for. */
int mh_world_batch_create_report(const mh_scene* scene, const mh_world_statics* statics, const mh_world_params* params, int B, mh_world_batch** out);
/* mh_world_batch_step_wrench plus the report: report_dev is a DEVICE array B x nsteps x npt x MH_REPORT_PAIR doubles (B the worlds of the batch, also
 * with ids_dev: only the listed worlds' rows are written).  report_dev == NULL IS mh_world_batch_step_wrench.  MH_ERR_INVALID_ARG if report_dev != NULL
 * on a batch not created by mh_world_batch_create_report.  Every other stepping entry takes such a batch and writes no report. */
int mh_world_batch_step_report(mh_world_batch* wb, void* stream, double dt, int nsteps, double* traj_dev,
                               const int* ids_dev, int count, const double* wrench_dev, int rows, double* report_dev);
/* Host convenience: mh_world_step_batch_params with the report in a HOST array B x nsteps x npt x MH_REPORT_PAIR (NULL: mh_world_step_batch_params). */
int mh_world_step_batch_report(const mh_scene* scene, const mh_world_forces* forces, const mh_world_statics* statics, const mh_world_params* params,
                               int B, double dt, int nsteps, double* state, mh_world_aux* aux, double* traj, double* report);

#ifdef __cplusplus
}
#endif
#endif
