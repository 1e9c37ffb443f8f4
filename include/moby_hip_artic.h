/* moby_hip_artic.h -- C ABI of the many-worlds stepper for ARTICULATED bodies (BASELINE config 5: the ur10 arm of
 * example/ur10/model.sdf x8192 initial states): reduced-coordinate forward dynamics by the composite-rigid-body
 * algorithm + Cholesky, and joint limits as unilateral constraints.
 *
 * Replaces, per world (one Moby::RCArticulatedBody with 1-DOF revolute / prismatic joints and a fixed base -- or a floating one carried by six virtual joints,
 * mh_artic_model.floating_base -- which is
 * what SDFReader::read_model builds: eCRB + eLinkCOM, src/SDFReader.cpp:934-935),
 *   TimeSteppingSimulator::step / do_mini_step                        src/TimeSteppingSimulator.cpp:52-222
 *   Ravelin::RCArticulatedBodyd::calc_fwd_dyn (CRB or FSAB, mh_artic_model.algorithm)  [seam B4]
 *                                                                      call site src/Simulator.cpp:552 -- Ravelin's source is
 *                                                                      NOT in the reference tree: the algorithm is
 *                                                                      Featherstone's (CRBA for H, RNEA for the bias), "parity unpinned"
 *   ArticulatedBody::find_limit_constraints                            include/Moby/ArticulatedBody.inl:9-43
 *   ImpactConstraintHandler::compute_problem_data / compute_X /
 *     compute_limit_components for limit rows                          src/ImpactConstraintHandler.cpp:1590-1695, 1755-1781
 *   ::apply_no_slip_model[_to_connected_constraints] with NC = 0       src/ImpactConstraintHandler.cpp:236-295, 1009-1417
 *     (an island without contacts has all_inf == true, ICH:123-135: LCP  L X L' l + L v >= 0  with X = H^-1)
 *   ::update_from_stacked, update_constraint_velocities_from_impulses, apply_restitution   src/ImpactConstraintHandler.cpp:298-525
 * One wavefront per world; H, its Cholesky factor, H^-1 and the limit LCP live in LDS.
 *
 * MH_WORLD_LCP_FAILED is the end of a world's run here as everywhere (moby_hip.h): the exception it stands for -- LCPSolverException, a generalized inertia that is not
 * positive definite, a failed compute_X -- is caught nowhere in the reference; the state stays where the throw left it and later steps pass the world over.
 *
 * Scope: config 5 is the robot alone (self-collision disabled as in ur10.xml:12: no contact rows, one mini-step per step);
 * optionally sphere primitives on links against a static plane (mh_artic_model.nspheres, no-slip contacts); joint forces and PD joint servos
 * through a drive (mh_artic_drive below: what controller plugins hand in as tau, evaluated inside the step).  Constraint stabilisation with joint-limit rows and, for bodies with link spheres, contact
 * rows: mh_artic_model.cstab_max_iterations (ur10.xml:11 sets constraint-stabilization-max-iterations = 0 = off).
 */
#ifndef MOBY_HIP_ARTIC_H
#define MOBY_HIP_ARTIC_H
#include "moby_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MH_ARTIC_MAX_JOINTS 16
#define MH_JOINT_REVOLUTE 0
#define MH_JOINT_PRISMATIC 1
#define MH_ARTIC_CRB  0
#define MH_ARTIC_FSAB 1
#define MH_ARTIC_MAX_SPHERES 4    /* sphere primitives carried by links (contacts against the one static plane) */
#define MH_ARTIC_MAX_BOXES 8      /* box primitives carried by links (the same plane) */
#define MH_ARTIC_MAX_PAIRS 6      /* every pair of MH_ARTIC_MAX_SPHERES spheres */
#define MH_ARTIC_PAIR_SPHERES    0   /* mh_artic_model.pair_kind */
#define MH_ARTIC_PAIR_BOX_SPHERE 1

/* Joint i carries link i; joints are listed parents first.  A link may be massless as long as its joint moves mass (something outboard of it has mass).  All quantities are LOCAL (constant), as a reader of
 * model.sdf derives them once at q = 0 (mh_io_load_sdf, moby_amd/host/mh_io.cpp):
 *   Rrel, trel   pose of link i's frame in its parent link's frame at q = 0 (row-major rotation; parent -1 = model frame)
 *   axis         joint axis in link i's frame, unit (revolute: rotation about it through the link origin; prismatic:
 *                translation along it)
 *   com, inertia centre of mass in link i's frame; inertia about the COM in link i's axes (row-major 3 x 3, symmetric) */
typedef struct mh_artic_model {
  int    nj;
  int    parent[MH_ARTIC_MAX_JOINTS];
  int    jtype[MH_ARTIC_MAX_JOINTS];
  double Rrel[MH_ARTIC_MAX_JOINTS][9];
  double trel[MH_ARTIC_MAX_JOINTS][3];
  double axis[MH_ARTIC_MAX_JOINTS][3];
  double com[MH_ARTIC_MAX_JOINTS][3];
  double inertia[MH_ARTIC_MAX_JOINTS][9];
  double mass[MH_ARTIC_MAX_JOINTS];
  double lolimit[MH_ARTIC_MAX_JOINTS];     /* Joint::lolimit / hilimit (src/Joint.cpp:201-262); +-DBL_MAX = none */
  double hilimit[MH_ARTIC_MAX_JOINTS];
  double limit_restitution[MH_ARTIC_MAX_JOINTS];   /* restitution-coeff, default 0 (src/Joint.cpp:33) */
  double gravity[3];
  int    algorithm;      /* RCArticulatedBody::algorithm_type (include/Moby/RCArticulatedBody.h: eFeatherstone / eCRB; the SDF
                            reader sets eCRB, src/SDFReader.cpp:934): MH_ARTIC_CRB (0) or MH_ARTIC_FSAB -- forward dynamics by
                            Featherstone's articulated-body recursion; the impact handler's X = H^-1 is the generalized inertia's
                            inverse either way (ICH:1600-1607) */
  int    floating_base;  /* RCArticulatedBody floating-base="true" (src/RCArticulatedBody.cpp:172-175), carried by VIRTUAL joints: 1 = joints 0..2 are prismatic
                            along the global x, y, z (Rrel = identity; trel of joint 0 = the base link's COM at q = 0) and joints 3..5 revolute about the base
                            link's own x, y, z through that COM, links 0..4 massless, link 5 the base link; the body's own joints follow (what
                            mh_io_load_xml_artic builds).  The dynamics, calc_jacobian and the contact rows need no special case -- six more 1-DOF columns;
                            the one place that reads the flag is conservative advancement, which adds the base's linear velocity along the direction of
                            approach as CCD::calc_max_dist does for a moving base (CCD.cpp:547-555).  By default NOT Ravelin's base coordinates (spatial
                            velocity + unit quaternion): the orientation is integrated in three angles, singular when joint 4 reaches +-pi/2; a batch in
                            pose coordinates (mh_artic_batch_set_base_coords below) has no such point.  0 = fixed base */
  /* Collision geometry (optional; nspheres = 0 is the robot alone: no pairs, one mini-step per step).  Sphere primitives fixed to
   * links against ONE static plane -- the closed-form pair of CCD.inl:804-847; the body's own pairs are disabled as ur10.xml:12
   * does.  With spheres the step is TimeSteppingSimulator::step in full: conservative advancement over the pairs
   * (CCD::calc_CA_Euler_step_sphere, the ARTICULATED CCD::calc_max_dist, CCD.cpp:545-583), mini-steps, contact + limit rows in one
   * island.  Contact rows are [d, r x d] . calc_jacobian(link) (ICH:1817-1895).  Impact models as the reference picks them
   * (ICH:123-146): every contact mu-coulomb >= 100 (what ur10.xml:19 gives the robot's contacts) -> the no-slip model
   * (ICH:1009-1417) over NC + NL <= MH_NOSLIP_MAX rows; otherwise the Drumwright-Shell QP -> LCP with contact AND limit variables
   * (ICH-QP:94-497: n = 6 NC + NC nk/2 + 2 NL <= MH_LCP_MAX_N_WAVE rows, lcp_fast_regularized(-20, 4, -8) on the persistent _z /
   * _zlast, then the Lemke ladder). */
  int    nspheres;
  int    sphere_link[MH_ARTIC_MAX_SPHERES];
  double sphere_center[MH_ARTIC_MAX_SPHERES][3];   /* link frame */
  double sphere_radius[MH_ARTIC_MAX_SPHERES];
  double plane_R[9];                               /* as mh_scene: row-major rotation of the plane frame, its +Y is the normal */
  double plane_o[3];
  double cp_epsilon, cp_mu_coulomb;                /* ContactParameters of the (robot, plane) pair */
  double min_step_size;                            /* TimeSteppingSimulator.cpp:48 (sqrt eps) */
  double contact_dist_thresh;                      /* ConstraintSimulator.cpp:56 (1e-6) */
  double cp_mu_viscous, cp_compliance;             /* used by the Drumwright-Shell model only (mu_coulomb < 100) */
  int    cp_nk;                                    /* friction-cone-edges (>= 4, even; ur10.xml:19 has 4); 0 is read as 4 */
  int    cstab_max_iterations;                     /* ConstraintStabilization::max_iterations ("constraint-stabilization-max-iterations"; ur10.xml:11
                                                      sets 0 = off; the reference's own default is UINT_MAX, see MH_CSTAB_DEFAULT_MAX_ITERATIONS) */
  /* ConstraintStabilization::stabilize after every step (TSS:97) with the body's JOINT LIMITS as rows (CStab:257-304 add_limit_constraints:
   * one row per finite limit, signed_violation = its distance; L_v = violation - |eps| - NEAR_ZERO, CStab:434-441; MM = L X L',
   * CStab:932-970; the line search of update_q over the limit slacks, CStab:1056-1216, 1322-1379).  Bodies WITH sphere primitives add a
   * contact row per (sphere, plane) pair (CStab:306-345: the synthetic contact "between separated bodies" when the signed distance is
   * at least NEAR_ZERO, find_contacts' otherwise; Cn_v = distance - |eps| - NEAR_ZERO, CStab:431) and the mixed LCP
   * MM = [Cn X Cn'  Cn X L'; .  L X L'] (CStab:705-904, 932-970); update_q's line search then evaluates the sphere distances too. */
  double cstab_eps;                                /* ConstraintStabilization::eps ("unilateral-stabilization-tol"), default NEAR_ZERO (CStab:59) */
  /* Box primitives fixed to links against the same static plane (appended: every field above keeps its offset).  They share plane_R / plane_o,
   * the cp_* ContactParameters, min_step_size and contact_dist_thresh with the spheres.  A box is BoxPrimitive (full edge lengths, as
   * mh_scene.geom_dim) with its centre and axes in its link's frame; vertices in BoxPrimitive::get_vertices order (BoxPrimitive.cpp:358-365):
   * vertex i = centre + R (+-xlen/2, +-ylen/2, +-zlen/2), the minus sign on x / y / z when bit 2 / 1 / 0 of i is set.
   *   contacts         find_contacts_plane_generic (CCD.inl:848-886): every vertex whose plane-frame height is <= TOL gives one contact AT the
   *                    vertex, normal = the plane's.  Canonical order: the spheres in index order, then the boxes in index order, each box's
   *                    vertices in get_vertices order.
   *   signed distance  BoxPrimitive::calc_signed_dist -> PlanePrimitive (the lowest vertex's height; the first vertex wins ties)
   *   conservative     calc_CA_Euler_step_generic (CCD.cpp:169-235): distance > 0 -> dist / calc_max_dist(link, -n0, rmax), the same articulated
   *   advancement      calc_max_dist as the spheres', rmax = the box's full diagonal + |link COM - box centre| (CollisionGeometry.cpp:52-68);
   *                    distance <= 0 -> calc_next_CA_Euler_step_generic: no vertex within NEAR_ZERO = no bound; a vertex approaching = 0; three
   *                    non-collinear contacts among the FIRST three = rest (CCD.cpp:285-323); otherwise calc_next_CA_Euler_step_polyhedron_plane
   *                    (CCD.cpp:405-468) with the link's angular velocity and its linear velocity at the box centre, in box axes.
   *   stabiliser       per (box, plane) pair (CStab:306-345): distance >= NEAR_ZERO -> one contact at the lowest vertex, normal towards its
   *                    projection on the plane; otherwise the vertex contacts within NEAR_ZERO.  cstab_eval reads the spheres', then the boxes' distances.
   * Capacity (the oracle's rules in handle_impacts / stabilize): no-slip NC + NL <= MH_NOSLIP_MAX, Drumwright-Shell N <= MH_LCP_MAX_N_WAVE, the
   * stabiliser's n <= MH_LCP_MAX_N_WAVE; a world beyond them carries MH_WORLD_UNSUPPORTED and its run ends, as for spheres.  Models with boxes
   * step through their own kernels (mh_artic_box.hip); sphere-only models keep theirs (mh_debug_set(12, 1) sends them through the box kernels). */
  int    nboxes;
  int    box_link[MH_ARTIC_MAX_BOXES];
  double box_center[MH_ARTIC_MAX_BOXES][3];        /* link frame */
  double box_R[MH_ARTIC_MAX_BOXES][9];             /* the box's axes in the link frame, row-major, orthonormal */
  double box_len[MH_ARTIC_MAX_BOXES][3];           /* full edge lengths xlen ylen zlen, > 0 */
  /* Sphere contacts between links (appended: every field above keeps its offset).  A pair names two spheres of the sphere list that sit on
   * DIFFERENT links: an arm against itself, two fingers, two chains that hang from the world in one model (several joints with parent = -1).
   * The pairs share the model's one set of cp_* ContactParameters, min_step_size and contact_dist_thresh with the plane contacts.  A sphere
   * whose bit is set in sphere_no_plane does not meet the plane (its pair with the plane body is disabled, or the scene has no plane); it still
   * counts in pairs.  Centres cA, cB and link frames in the model frame:
   *   contact          find_contacts_sphere_sphere (CCD.inl:1163-1206): d = cA - cB, dist = |d| - rA - rB (= (|d| - rA) - rB); none if dist > TOL;
   *                    n = d / |d| (from b to a); point = ((cA - n rA) + (cB + n rB)) * 0.5; tangents by orthonormal_basis(n).  Canonical order
   *                    of a world's contact list: spheres against the plane in index order (masked ones skipped), boxes, then pairs in index order.
   *   row              for each of the three directions (ICH:1817-1895, two add_contact_dir_to_Jacobian blocks): column j =
   *                    [dir, (p - comA) x dir] . J_A(comA)_j  +  [-dir, (p - comB) x -dir] . J_B(comB)_j, A's term FIRST, each term the one-link
   *                    expression; a joint that is an ancestor of only one of the two links gets that term alone, of neither 0.0.
   *   constraint       A's point velocity along n MINUS B's (the impacting test, conservative advancement, the tolerance test after the impact);
   *   velocity         a plane contact keeps its single term.
   *   conservative     the sphere rule (CCD.cpp:138-235): dist > NEAR_ZERO -> dist / max(0, calc_max_dist(linkA, -n0, rmaxA) + calc_max_dist(linkB, n0, rmaxB)),
   *   advancement      n0 = n of the closest points; dist <= NEAR_ZERO -> a contact with |constraint velocity| < 10 NEAR_ZERO = no bound; dist <= 0 ->
   *                    no contact = no bound, approaching (< -NEAR_ZERO) = 0, else no bound.  calc_max_dist adds the floating base's linear
   *                    velocity only for links that descend from joint 0 (a second root does not ride on the base); for a single-root model that
   *                    is every link, as before.
   *   stabiliser       one row per pair and iteration (CStab:306-345): dist >= NEAR_ZERO -> the synthetic contact at cA - n rA with normal n,
   *                    otherwise the contact above (TOL = NEAR_ZERO); Cn_v = dist - |eps| - NEAR_ZERO.  cstab_eval reads the distances of the spheres that meet the plane
   *                    (a masked sphere has no entry), the boxes', then the pairs'.
   * Capacity as for boxes.  Models with pairs or a mask step through their own kernels (mh_artic_pair.hip, mh_artic_pair_pose.hip);
   * mh_debug_set(13, 1) sends box and sphere models through them too (batches created after it).
   * mh_artic_batch_create refuses (MH_ERR_INVALID_ARG): npairs outside [0, MH_ARTIC_MAX_PAIRS], an index outside the sphere list, a == b, both
   * spheres on one link, a pair listed twice in either order, bits of sphere_no_plane beyond nspheres. */
  int    npairs;                                   /* 0 = no link-link contacts */
  int    pair_a[MH_ARTIC_MAX_PAIRS];               /* indices into the sphere list; a is the reference's geometry A */
  int    pair_b[MH_ARTIC_MAX_PAIRS];               /*   (the normal points from b to a) */
  int    sphere_no_plane;                          /* bit s set: sphere s does not meet the plane; 0 = every sphere does */
  /* Box-sphere contacts between links and static boxes (appended: every field above keeps its offset; a zeroed pair_kind is the model above).
   * A pair of kind MH_ARTIC_PAIR_BOX_SPHERE names a box (pair_a: index into the BOX list) and a sphere (pair_b: index into the sphere list) on
   * different links; the box is the reference's geometry A wherever the pair is read (CCD.inl:15,26 swaps the arguments so that it is).  npairs
   * counts both kinds, at most MH_ARTIC_MAX_PAIRS together.  box_link = -1 is a STATIC box: box_center / box_R are its pose in the model frame; it
   * never meets the plane (no plane contacts, no entry in the plane's conservative-advancement or stabiliser distance lists), must appear in at
   * least one box-sphere pair, and stands for a disabled body: no Jacobian term, calc_max_dist = 0 (CCD.cpp:589-590).  A link box in a pair still
   * meets the plane as before: there is no plane mask for boxes.  A sphere that appears only in box-sphere pairs may carry its sphere_no_plane bit.
   * With c the sphere's centre in the box's frame, h the half lengths, R the radius, p = clamp(c, -h, h) (the fixed point of the reference's
   * projected-gradient QP, BoxPrimitive.cpp:183-254), v = p - c:
   *   contact          find_contacts_box_sphere (CCD.inl:1208-1259).  If any |p_i| < h_i or |v| < R (every face and edge region, and every
   *                    penetration): dist = -min(min_i(h_i - |p_i|), R - |v|), the sphere point stays c + v; otherwise (a vertex region) the sphere
   *                    point is c + v R / |v| and dist = the distance between the two points.  None if dist > TOL.  dist > 0: the point is the
   *                    midpoint of the two points (over a face or an edge that is the box point itself), the normal their difference box - sphere
   *                    normalised, or -- when that is no longer than NEAR_ZERO -- the sphere-frame vector to the box point, normalised: the unit
   *                    vector from the sphere's centre to p.  dist <= 0: the sphere point and that unit vector.  A centre inside the box gives
   *                    v = 0 and a NaN normal, as in the reference; there is no fallback.  One pair gives at most one contact; canonical order:
   *                    spheres on the plane, boxes, then the pairs in index order, both kinds mixed.
   *   signed distance  BoxPrimitive::calc_signed_dist (BoxPrimitive.cpp:256-276, 788-836), a DIFFERENT function: the closest-point distance of c
   *                    (the negative interior depth when c is inside) minus R; sphere point = centre + v (R + min(dist, 0)) / |v|, the centre if
   *                    |v| = 0.  Conservative advancement, the contact threshold test and the stabiliser read this one.
   *   row, velocity    the two-term form of the sphere pairs: A = the box's link, B = the sphere's, A's term first; a static box has no term (the
   *                    row is B's term with -dir, the constraint velocity minus B's point velocity).
   *   conservative     the sphere rule: dist > NEAR_ZERO -> dist / max(0, calc_max_dist(linkA, -n0, rmaxA) + calc_max_dist(linkB, n0, rmaxB)), n0 from
   *   advancement      the signed-distance function's two points, B to A; a static box's term is 0.0 and still added first; dist <= 0 as for sphere pairs.
   *   stabiliser       one row per pair: dist >= NEAR_ZERO -> the synthetic contact at A's closest point with normal n0; otherwise the contact
   *                    above with TOL = NEAR_ZERO; Cn_v = dist - |eps| - NEAR_ZERO.  cstab_eval appends the pairs' signed distances in index order.
   * Box against box between links and a static sphere are not built.  Models with a box-sphere pair or a static box step through their own kernels
   * (mh_artic_bsp.hip, mh_artic_bsp_pose.hip); mh_debug_set(14, 1) sends pair, box and sphere models through them too (batches created after it).
   * mh_artic_batch_create refuses (MH_ERR_INVALID_ARG): an unknown kind, an index outside the list the kind names, a box-sphere pair whose box and
   * sphere sit on one link, a pair listed twice, a static box in no pair, box_link < -1. */
  int    pair_kind[MH_ARTIC_MAX_PAIRS];            /* MH_ARTIC_PAIR_SPHERES (0): pair_a, pair_b index the sphere list; MH_ARTIC_PAIR_BOX_SPHERE (1): pair_a the box list */
} mh_artic_model;

/* B worlds resident on the GPU: joint positions q and velocities qd (B x nj each) + mh_world_aux (rand() stream, time,
 * status, counters; vns / vns_size hold ImpactConstraintHandler::_v, the warm start of the limit LCP).
 *   step      nsteps x TimeSteppingSimulator::step(dt) in ONE launch
 *   fwd_dyn   seam B4: qdd = H(q)^-1 (tau - C(q, qd)) for the resident states (tau: B x nj device-side copy of host
 *             values, or NULL = 0); H_out (B x nj x nj, row-major) optional -- the generalized inertia
 *             (get_generalized_inertia, used by compute_X)
 */
typedef struct mh_artic_batch mh_artic_batch;
int mh_artic_batch_create(const mh_artic_model* model, int B, mh_artic_batch** out);
int mh_artic_batch_destroy(mh_artic_batch* ab);
int mh_artic_batch_device(const mh_artic_batch* ab);   /* the device the batch lives on (moby_hip.h, Devices) */
int mh_artic_batch_upload(mh_artic_batch* ab, const double* q, const double* qd, const mh_world_aux* aux);
int mh_artic_batch_step(mh_artic_batch* ab, void* stream, double dt, int nsteps);
int mh_artic_batch_fwd_dyn(mh_artic_batch* ab, const double* tau, double* qdd_out, double* H_out);
int mh_artic_batch_download(mh_artic_batch* ab, double* q, double* qd, mh_world_aux* aux);
/* link poses of the resident states (B x nj x 12: row-major R (9), origin (3), model frame): what a viewer or a
 * collision front end on the host needs */
int mh_artic_batch_link_poses(mh_artic_batch* ab, double* poses);
/* RCArticulatedBodyd::calc_jacobian(frame at a point, link, J) of the resident states: the 6 x nj map from joint velocities to
 * the velocity of link `link` at the given points (B x 3, model frame) -- rows 0..2 the linear velocity of the point, rows 3..5
 * the angular velocity, global axes; column j is zero unless joint j lies between the link and the base.  What a contact on a
 * link multiplies its direction row [d, r x d] with (ImpactConstraintHandler::add_contact_dir_to_Jacobian, ICH:1817-1845).
 * J_out: B x 6 x nj, row-major. */
int mh_artic_batch_jacobian(mh_artic_batch* ab, int link, const double* points, double* J_out);

/* Drives: joint forces and PD joint servos inside the step -- what the reference's controller plugins do (example/ur10/controller.cpp), called
 * once per mini-step from precalc_fwd_dyn (TimeSteppingSimulator.cpp:173 -> Simulator.cpp:319-350, ArticulatedBody.cpp:95-115).
 * A drive gives every world a generalized force per joint, evaluated inside the step ONCE PER MINI-STEP, immediately before that mini-step's
 * forward dynamics: q has already been advanced by the mini-step's position update, qd is still the mini-step's starting velocity,
 *   tau_j = (kp_j * (q_des_j - q_j) + kv_j * (qd_des_j - qd_j)) + tau_ff_j
 * every operation rounded on its own (no FMA); a term whose bit is not set is ABSENT (MH_DRIVE_FORCE alone: tau = tau_ff; MH_DRIVE_PD alone:
 * tau = the bracket).  The forward dynamics then solve H qdd = tau - C, as mh_artic_batch_fwd_dyn does.  The virtual joints of a floating
 * base are driven like any other column.  tau does NOT enter compute_X / the generalized inertia: impulses, restitution and constraint
 * stabilisation are unchanged, as in the reference.  A world carrying MH_WORLD_LCP_FAILED is passed over as by mh_artic_batch_step.
 * Arrays are row-major with the batch's joint order; world b, joint j of schedule row r is element (r B + b) nj + j. */
#define MH_DRIVE_FORCE 1      /* tau_ff */
#define MH_DRIVE_PD    2      /* kp, kv, q_des, qd_des */
typedef struct mh_artic_drive {
  int terms;                  /* MH_DRIVE_* bits; 0 = undriven (nothing else is read) */
  int rows;                   /* schedule rows R: 1 = row 0 held for the whole launch; R >= nsteps = step s of the launch (all its mini-steps) reads row s */
  const double* kp;           /* B x nj */
  const double* kv;           /* B x nj */
  const double* q_des;        /* R x B x nj */
  const double* qd_des;       /* R x B x nj */
  const double* tau_ff;       /* R x B x nj */
} mh_artic_drive;
/* nsteps x TimeSteppingSimulator::step(dt) in one launch with a drive.  The drive's pointers are DEVICE pointers on the batch's device, read in
 * stream order; drive == NULL: the drive stored by mh_artic_batch_set_drive (none stored: exactly mh_artic_batch_step).  MH_ERR_INVALID_ARG:
 * unknown bits in terms, a NULL pointer for a requested term, rows < 1, 1 < rows < nsteps.  The kernel is the one mh_artic_batch_step picks
 * (spheres -> contacts, cstab -> the stabilising kernel, otherwise MH_ARTIC_WAVES); the two-worlds-per-wave kernel (mh_debug_set key 9,
 * MH_ARTIC_PACK) has no driven form: a driven launch takes the one-world kernels whatever it is set to. */
int mh_artic_batch_step_driven(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* drive);
/* HOST arrays, copied into batch-owned device storage (synchronously, after the work in flight on the device) and used by
 * mh_artic_batch_step_driven(..., NULL) until replaced; host_drive == NULL or terms == 0 clears it.  rows >= 1 is checked here, rows against
 * nsteps at each step. */
int mh_artic_batch_set_drive(mh_artic_batch* ab, const mh_artic_drive* host_drive);
/* the resident q / qd into caller DEVICE buffers (B x nj each, either may be NULL), stream-ordered (hipMemcpyAsync on `stream`): the
 * observation half of a GPU-resident control loop (state_dev -> a policy on the device -> step_driven with device pointers) */
int mh_artic_batch_state_dev(mh_artic_batch* ab, void* stream, double* q_dst, double* qd_dst);

/* Base coordinates of a floating base (mh_artic_model.floating_base = 1).  MH_ARTIC_BASE_ANGLES, the default: the six virtual joints carry the
 * base's whole configuration, the orientation as three angles from the model's start pose, singular when joint 4 reaches +-pi/2.
 * MH_ARTIC_BASE_POSE: every world also carries a base pose P = (p, Q) -- p the base link's COM in the model frame, Q a unit quaternion (w, x, y, z)
 * -- that stands in for the model's trel[0] and Rrel[3] wherever the kinematics reads them; the virtual joints measure the motion from P.  After
 * every step that ran to its end (after the stabiliser) the step FOLDS them into P, which changes coordinates only -- configuration and link
 * velocities stay the same up to round-off:
 *   p += q[0..2];   Q = normalize(Q (x) Qx(q3) (x) Qy(q4) (x) Qz(q5));
 *   qd[3..5] = Rh' (e_x qd3 + Rx(q3) e_y qd4 + Rx(q3) Ry(q4) e_z qd5), Rh = Rx(q3) Ry(q4) Rz(q5): the base's angular velocity in its new axes;
 *   q[0..5] = 0;  qd[0..2] (the COM velocity, global axes) and the body's own joints unchanged.
 * So after a completed step q[0..5] are exactly 0, and the middle hinge only ever turns by one step's rotation.  A world whose step throws
 * (MH_WORLD_LCP_FAILED) is not folded: (P, q) still describe where the throw left it.  Everything else is the step of angle coordinates:
 * dynamics, limits, contacts, conservative advancement, the stabiliser, the drive.  A drive works on every column: tau_ff on the virtual
 * columns is a global force at the COM and a torque about the base's own axes; a PD target on a virtual column is measured against the
 * re-zeroed q -- rarely what a caller wants.  Side effect on conservative advancement: q[0..2] return to zero every step, so the slider terms of
 * calc_max_dist no longer grow with the distance from the origin.  Every step route (mh_artic_batch_step, _step_driven; spheres, the stabiliser)
 * has a pose form; MH_ARTIC_WAVES and MH_ARTIC_PACK (key 9) do not apply (the default four-waves budget).  link_poses, jacobian and fwd_dyn read
 * each world's P.  upload / download keep their shapes: uploaded virtual q are relative to the current P.  A checkpoint of a pose batch is
 * download + base_pose; restore is upload + set_base_pose. */
#define MH_ARTIC_BASE_ANGLES 0
#define MH_ARTIC_BASE_POSE   1
/* ANGLES -> POSE: every world's P from the model (p = trel[0], Q = the quaternion of Rrel[3]), then the resident q / qd folded into it (a world
 * carrying MH_WORLD_LCP_FAILED is not: its q still hold its configuration against the model's pose).  POSE -> POSE does nothing.
 * MH_ERR_INVALID_ARG: a fixed base, a finite limit on one of joints 0..5, POSE -> ANGLES, an unknown value. */
int mh_artic_batch_set_base_coords(mh_artic_batch* ab, int coords);
int mh_artic_batch_base_coords(const mh_artic_batch* ab, int* coords);   /* the batch's MH_ARTIC_BASE_* */
/* the poses as HOST arrays, B x 7 (px py pz qw qx qy qz), synchronously; pose coordinates only.  The setter normalises each Q and refuses a zero or
 * non-finite quaternion (nothing is written then). */
int mh_artic_batch_base_pose(mh_artic_batch* ab, double* pose);
int mh_artic_batch_set_base_pose(mh_artic_batch* ab, const double* pose);
/* the poses into a caller DEVICE buffer (B x 7), stream-ordered: the pose counterpart of mh_artic_batch_state_dev */
int mh_artic_batch_base_pose_dev(mh_artic_batch* ab, void* stream, double* dst);

/* Contact report.  What the reference hands to ConstraintSimulator::constraint_post_callback_fn (ConstraintSimulator.cpp:353) -- the mini-step's contact
 * constraints, each with the contact_impulse that ImpactConstraintHandler::update_from_stacked accumulated (ImpactConstraintHandler.cpp:298-327) --
 * reduced per SLOT inside the step and left in device memory: the contact half of a GPU-resident control loop's observation (is the foot down, how
 * hard does the tip press on the crate, where is the centre of pressure under a box foot), beside mh_artic_batch_state_dev.
 * Slots: nslots = nspheres + nboxes + npairs (mh_artic_report_slots).  Slot s < nspheres is sphere s against the plane; slot nspheres + b is box b
 * against the plane, all of its vertex contacts; slot nspheres + nboxes + k is pair k, of either kind.  A sphere masked off the plane and a static box
 * keep their slot: its rows stay zero.  For world w, step s of the launch and a slot there is one row of MH_REPORT_PAIR (moby_hip.h: 8) doubles at
 * report_dev[((w * nsteps + s) * nslots + slot) * MH_REPORT_PAIR].  The rows of a step start at zero and accumulate over the step's mini-steps, in
 * mini-step order; within a mini-step in constraint-list order (canonical: spheres, then boxes with their vertices in get_vertices order, then pairs).
 * A mini-step's contacts are folded once handle_impacts has returned without a throw (the point of CSim:353) -- also when the handler returned early
 * because nothing was impacting, or because there was neither a contact nor a limit: its contacts then count, with zero impulse.  A mini-step that threw
 * (the forward dynamics failed before the contacts were generated, or the handler set MH_WORLD_LCP_FAILED) is not folded: the step's rows keep what
 * earlier mini-steps left.  Every step of a world that is passed over (MH_WORLD_LCP_FAILED) writes zero rows.  A world with MH_WORLD_UNSUPPORTED or
 * MH_WORLD_STALLED has undefined rows from then on, as its state is; they are still written inside the world's own rows only.
 * Contact c carries accumulated (cn, cs, ct): zeroed when the contact list is built; every application of impulses by the impact handler adds what it
 * applied (the no-slip solve and its restitution pass; the Drumwright-Shell solve, its restitution pass with the tangential impulses applied again in
 * full, and the second solve); the stabiliser's corrections add nothing.  The handler refuses more than MH_NOSLIP_MAX contacts, so a contact beyond
 * them folds with zero impulse.  With p the stored contact point, n the normal and s, t the tangents, contact c adds to its slot's row:
 *   [0]     += 1.0                  contacts, summed over mini-steps
 *   [1]     += cn
 *   [2..4]  += jv                   jv = (n cn + s cs) + t ct componentwise, every product and sum rounded on its own, model-frame axes: the impulse ON
 *                                   THE REFERENCE'S GEOMETRY A.  For a plane contact A is the link that carries the sphere or box; for a pair A is
 *                                   pair_a's link, and pair_b's link received -jv.  With a static box as A only -jv on the sphere's link is physical.
 *   [5..7]  += p * cn               the contact point weighted by its normal impulse: the centre of pressure is [5..7] / [1]
 * Such a batch steps through code objects of its own (mh_artic_rp.hip, mh_artic_rp_pose.hip: the box-sphere kernels with MH_ARTIC_REPORT_TU) whatever
 * its geometry -- sphere-only, box, pair and box-sphere models alike; every batch of mh_artic_batch_create launches what it launched.  Pose coordinates
 * work as for every family.  Key 19 of mh_debug_set sends batches that would take the box-sphere kernels through these objects with a NULL report (A/B
 * runs; no result changes).
 * NOT built: joint-limit impulses (the rows hold contacts only); per-contact lists (the row is per slot); angular impulses ([5..7] gives the lever);
 * the report in the large-world stepper (moby_hip_stack.h); a host convenience entry. */
/* (no existing layout changes, so MH_VERSION stays as it is; a caller that needs to know tests this macro) */
#define MH_ARTIC_REPORT 1
/* host only: nspheres + nboxes + npairs, or a negative MH_ERR_* for a NULL model or one whose counts lie outside their ranges */
int mh_artic_report_slots(const mh_artic_model* model);
/* mh_artic_batch_create with the report kernels: every check of mh_artic_batch_create, and MH_ERR_INVALID_ARG for a model without a slot. */
int mh_artic_batch_create_report(const mh_artic_model* model, int B, mh_artic_batch** out);
/* mh_artic_batch_step_driven plus the report (drive == NULL: the stored drive, or none): report_dev is a DEVICE array B x nsteps x nslots x
 * MH_REPORT_PAIR doubles, written in stream order.  report_dev == NULL: the same kernels with nothing written.  MH_ERR_INVALID_ARG if
 * report_dev != NULL on a batch not created by mh_artic_batch_create_report.  mh_artic_batch_step and _step_driven take such a batch and write no report. */
int mh_artic_batch_step_report(mh_artic_batch* ab, void* stream, double dt, int nsteps, const mh_artic_drive* drive, double* report_dev);

/* Per-world parameters.  Every world of a batch steps its own VALUES of one shared model: a range of robots (masses, centres of mass, inertias, link
 * lengths, joint limits, foot radii, friction, the slope of the ground, the place of the crate) in one launch.  The rule: world w of a batch created
 * with records is stepped exactly as a batch of the model with record w written into it would step it -- state, aux record, base pose and report rows,
 * bit for bit.  A record holds doubles only, with the model's indexing, so nothing in it can become an index.
 * The TOPOLOGY stays the model's for every world: nj, parent, jtype, algorithm, floating_base; the counts and link indices of spheres and boxes (a
 * static box stays static); the pair lists and kinds, sphere_no_plane; cp_nk, min_step_size, contact_dist_thresh, cstab_max_iterations, cstab_eps; and
 * WHICH limits are finite (a bound with |value| < DBL_MAX) -- a record may move a finite limit but may not add or remove one, so the stabiliser's row
 * count and the pose-coordinate refusal stay decisions of the model.  The impact model is chosen per world from its own cp_mu_coulomb (>= 100: no-slip,
 * below: Drumwright-Shell), as the kernel does from the model's; worlds on either side may share a batch, and so for such a batch the friction polygon
 * is filled from cp_nk and cp_nk is validated whatever the model's own mu, and the solver workspace is always allocated.
 * In pose coordinates (MH_ARTIC_BASE_POSE) a record's trel[0] and Rrel[3] are NOT read by a step: the per-world pose stands in for them.
 * mh_artic_batch_set_base_coords takes each world's start pose from its own record (p = trel[0], Q of Rrel[3]); a per-world start pose later is
 * mh_artic_batch_set_base_pose.
 * Such a batch steps through code objects of its own (mh_artic_pw.hip, mh_artic_pw_pose.hip: the report kernels with MH_ARTIC_PARAMS_TU, under which
 * the step reads image w of B) whatever its geometry -- also a model with no geometry at all, the robot alone with randomised masses; the contact
 * kernels step an empty contact list as the plain kernels do.  Report rows are written only when the batch was created with MH_ARTIC_CREATE_REPORT.
 * fwd_dyn, link_poses, jacobian and set_base_coords read each world's own image.  Every other batch launches what it launched.  Key 20 of mh_debug_set
 * sends batches that would take the report kernels through these objects with B images equal to the model (A/B runs; no result changes).
 * NOT built: per-world topology; adding or removing limits; per-world cp_nk; the record in the large-world stepper (moby_hip_stack.h). */
/* (no existing layout changes, so MH_VERSION stays as it is; a caller that needs to know tests this macro) */
#define MH_ARTIC_PARAMS 1
#define MH_ARTIC_CREATE_REPORT 1     /* flags of mh_artic_batch_create_params: the batch is a report batch too (mh_artic_batch_create_report) */
typedef struct mh_artic_params {
  double Rrel[MH_ARTIC_MAX_JOINTS][9];
  double trel[MH_ARTIC_MAX_JOINTS][3];
  double axis[MH_ARTIC_MAX_JOINTS][3];
  double com[MH_ARTIC_MAX_JOINTS][3];
  double inertia[MH_ARTIC_MAX_JOINTS][9];
  double mass[MH_ARTIC_MAX_JOINTS];
  double lolimit[MH_ARTIC_MAX_JOINTS];
  double hilimit[MH_ARTIC_MAX_JOINTS];
  double limit_restitution[MH_ARTIC_MAX_JOINTS];
  double gravity[3];
  double sphere_center[MH_ARTIC_MAX_SPHERES][3];
  double sphere_radius[MH_ARTIC_MAX_SPHERES];
  double plane_R[9];
  double plane_o[3];
  double cp_epsilon, cp_mu_coulomb, cp_mu_viscous, cp_compliance;
  double box_center[MH_ARTIC_MAX_BOXES][3];
  double box_R[MH_ARTIC_MAX_BOXES][9];
  double box_len[MH_ARTIC_MAX_BOXES][3];
} mh_artic_params;
/* host only: the record that reproduces the model (every field above copied from it) */
void mh_artic_params_from_model(const mh_artic_model* model, mh_artic_params* out);
/* mh_artic_batch_create with a record per world (HOST pointer, B records; NULL: every record = the model); flags: MH_ARTIC_CREATE_REPORT or 0.
 * First every refusal of mh_artic_batch_create (and of _create_report with the flag), unchanged; then every record is validated as the model's values
 * are, through the same checks: mass >= 0 and every joint moves mass; unit axes; lolimit <= hilimit and the model's pattern of finite limits; on a
 * floating base the virtual joints' fixed entries equal the layout; with geometry sphere radii > 0, box edges finite and > 0, box_R orthonormal, the
 * plane's +Y column a unit vector, the four contact parameters finite and >= 0; gravity finite.  The last two are stricter than the model's own
 * checks (mh_artic_batch_create takes an infinite cp_mu_coulomb or a non-finite gravity), and they hold for host == NULL too: such a model is then
 * refused through its record, as world 0.  MH_ERR_INVALID_ARG with a message that names the world and the field; all of it runs before the device is
 * looked for. */
int mh_artic_batch_create_params(const mh_artic_model* model, const mh_artic_params* host, int B, int flags, mh_artic_batch** out);
/* Replaces the records of worlds first .. first + count - 1 (HOST pointer, `count` records), validated as at create; synchronous (after the work in
 * flight on the device).  MH_ERR_INVALID_ARG: a batch not created by mh_artic_batch_create_params, a range outside the batch, a refused record (none
 * is then written). */
int mh_artic_batch_set_params(mh_artic_batch* ab, const mh_artic_params* host, int first, int count);
/* The same from DEVICE memory, by a small kernel on `stream` that scatters the records into the worlds' images: ordered with the launches of that
 * stream, for a caller that randomises on the GPU between launches.  The records are NOT validated.  What a bad value does, as read from the step
 * kernels: nothing outside the world's own memory is touched, because a record holds doubles only and no double of the image is ever converted to
 * an index, a count or a loop bound -- every index, count and bound of the step comes from the shared topology (nj, parent, the ancestor masks, the
 * sphere, box and pair lists, cp_nk, cstab_max_iterations) or from integers the kernel computes itself (contact and limit counts, capped by
 * MH_NOSLIP_MAX / MH_LCP_MAX_N_WAVE, beyond which the world gets MH_WORLD_UNSUPPORTED), and every loop a non-finite value can reach ends by a cap
 * (MH_CA_HARD_CAP in the conservative-advancement loop, the 100000 mini-step guard, the stabiliser's iteration count -- cstab_max_iterations and
 * MH_CSTAB_HARD_CAP --, Ridders' 25 iterations, the backtracking that shrinks its step by 0.6 down to NEAR_ZERO, the solvers' pivot caps) or by a
 * comparison that is false for NaN (h < dt, max violation < cstab_eps).  That world's state goes
 * non-finite or it gets a status bit (MH_WORLD_STALLED, MH_WORLD_LCP_FAILED, MH_WORLD_UNSUPPORTED); the other worlds are not affected.  A record
 * that adds or removes a finite limit is not refused here: the limit rows follow the record (the kernel tests each bound against DBL_MAX itself, and
 * the row tables are sized for two rows per joint), but results then no longer follow the rule above for the shared model's pattern.  In pose
 * coordinates trel[0] and Rrel[3] are not read.  MH_ERR_INVALID_ARG: a batch not created by mh_artic_batch_create_params, a range outside the batch. */
int mh_artic_batch_set_params_dev(mh_artic_batch* ab, void* stream, const mh_artic_params* dev, int first, int count);

/* Link wrenches.  A force that acts on a LINK, inside the step: a shove against the torso, a rotor's thrust in the axes of the arm that carries it, a
 * tether's tug, velocity-proportional damping of the links -- what a controller of the reference does with link->add_force(...) and what
 * DampingForce::add_force does for an articulated body (DampingForce.cpp:32-51 and its articulated branch), both inside precalc_fwd_dyn, once per
 * mini-step.  The wrench is evaluated once per mini-step inside the forward dynamics, immediately after the link frames of that mini-step's q exist:
 * q has been advanced by the position update, qd is still the mini-step's starting velocity, the drive's tau is already evaluated.  Every operation
 * is rounded on its own, three-term sums are (a + b) + c, and an absent term is left out, not added as zero.  It enters the dynamics as a generalized
 * force and nowhere else: compute_X, the impact handler, restitution, conservative advancement and the stabiliser never read it (nor the drive).
 * For world w, schedule row r and link i (R_i, x_i the link frame; S_j the motion subspaces about the model origin, [angular; linear];
 * c_i = x_i + R_i com_i the link's COM in the model frame; V_i = [w_i; v_i] the link's spatial velocity about the model origin):
 *   damping (MH_LINK_DAMPING)   vc = v_i + w_i x c_i;  vi = R_i' vc, wi = R_i' w_i;  fb = vi * (-(kl + |vi| klsq)), tb = wi * (-(ka + |wi| kasq)),
 *                               |a| = sqrt((a0^2 + a1^2) + a2^2);  F = R_i fb, T = R_i tb
 *   the caller's (MH_LINK_WRENCH)  (f, n) = entry ((r B + w) nj + i) 6 of w: f acts at the link's COM, n is a free torque, model axes; with
 *                               MH_LINK_WRENCH_LINK_AXES both are rotated first, f <- R_i f, n <- R_i n.  F = F + f, T = T + n (F = f, T = n without damping)
 *   F6_i = [T + c_i x F; F]     (the cross product first, then the sum)
 *   tau_x[j] = sum of dot6(S_j, F6_i) over the links i, in increasing i, on whose path to the base joint j lies (i itself included), from 0.0
 *   tau_j = tau_drive_j + tau_x[j], or tau_x[j] alone in an undriven launch
 * and H qdd = tau - C is solved as ever, by either algorithm.  The virtual links of a floating base are links like any other: a caller zeroes their
 * coefficients, and a wrench on link 5 is a wrench on the base.  Gains kl, ka, klsq, kasq are per world and link (B x nj each).
 * A batch that takes wrenches is one of mh_artic_batch_create_wrench: a per-world-parameters batch (every rule of "Per-world parameters" holds for it:
 * set_params, set_params_dev, pose coordinates, drives, the report) that steps through code objects of its own (mh_artic_wr.hip, mh_artic_wr_pose.hip:
 * the per-world-parameters kernels with MH_ARTIC_WRENCH_TU).  The LDS image of a world does not grow: F6 lives in the bias forces' region, which the
 * bias pass rewrites afterwards, and tau_x is added into the slot the drive writes.  Coefficients and schedule rows are read from global memory at
 * every mini-step.  Every other batch launches what it launched.  Key 21 of mh_debug_set sends batches that would take the per-world-parameters
 * kernels through these objects with a NULL wrench (A/B runs; no result changes).
 * NOT built: StokesDragForce on articulated bodies (the reference's articulated branch dereferences a null pointer, StokesDragForce.cpp:55-62: there
 * is no behaviour to reproduce); <DampingForce> read from scene files by mh_io_load_xml_artic; a force at a point other than the COM (the caller adds
 * r x f to n); wrenches in mh_artic_batch_fwd_dyn; a wrench form of the plain, non-contact kernels (the family inherits the per-world-parameters
 * family's measured 6.9x on a robot without geometry); the large-world stepper (moby_hip_stack.h). */
/* (no existing layout changes, so MH_VERSION stays as it is; a caller that needs to know tests this macro) */
#define MH_ARTIC_WRENCH 1
#define MH_LINK_WRENCH            1
#define MH_LINK_DAMPING           2
#define MH_LINK_WRENCH_LINK_AXES  4   /* only with MH_LINK_WRENCH */
typedef struct mh_artic_wrench {
  int terms;                  /* MH_LINK_* bits; 0 = none: nothing else is read */
  int rows;                   /* as mh_artic_drive.rows: 1 = held, >= nsteps = row s for all mini-steps of step s */
  const double* w;            /* DEVICE, rows x B x nj x 6: fx fy fz nx ny nz */
  const double* kl;           /* DEVICE, B x nj each: linear, angular, quadratic linear, quadratic angular damping */
  const double* ka;
  const double* klsq;
  const double* kasq;
} mh_artic_wrench;
/* mh_artic_batch_create_params with every one of its refusals (flags: MH_ARTIC_CREATE_REPORT or 0); the batch it returns also takes wrenches. */
int mh_artic_batch_create_wrench(const mh_artic_model* model, const mh_artic_params* host, int B, int flags, mh_artic_batch** out);
/* mh_artic_batch_step_report plus the wrench (DEVICE pointers on the batch's device, read in stream order).  wrench == NULL or terms == 0: the same
 * kernels with no force, results equal to the per-world-parameters batch bit for bit.  MH_ERR_INVALID_ARG, with a message that names the field, all
 * checked before the device is looked for: a wrench on a batch not created by mh_artic_batch_create_wrench, unknown bits in terms,
 * MH_LINK_WRENCH_LINK_AXES without MH_LINK_WRENCH, a NULL pointer for a requested term (kl, ka, klsq and kasq are all four required for damping),
 * rows < 1 or 1 < rows < nsteps, report_dev on a batch without the report flag.  mh_artic_batch_step, _step_driven and _step_report take such a
 * batch and apply no wrench. */
int mh_artic_batch_step_wrench(mh_artic_batch* ab, void* stream, double dt, int nsteps,
                               const mh_artic_drive* drive, const mh_artic_wrench* wrench, double* report_dev);

/* Episodes on the device.  What a learning or sampling loop needs between two launches without a host round trip: a new episode in the worlds that
 * ended (reset_dev), which worlds have ended (status_dev), and where the links are (link_poses_dev: a tip position is what a reward or a termination
 * test reads).  All pointers are DEVICE pointers on the batch's device; every call is ordered on `stream` with the launches of that stream; none
 * synchronises the device, allocates or frees device memory, or copies through the host.  They work on every batch -- of mh_artic_batch_create,
 * _create_report, _create_params and _create_wrench, every geometry family, both coordinate kinds.
 *
 * mh_artic_batch_reset_dev: world w is reset iff mask_dev[w] != 0 (B ints: a policy's `done` vector as it is; NULL = every world).  q_src, qd_src
 * (B x nj each) and pose_src (B x 7: px py pz qw qx qy qz) hold a row per world; only the rows of reset worlds are read; a NULL source leaves that
 * array as it is, as mh_artic_batch_upload does.  The quaternion is normalised on the device with the arithmetic of mh_artic_batch_set_base_pose --
 * n = sqrt(((w*w + x*x) + y*y) + z*z), every component divided by n, no contraction -- so the stored pose is bit-equal to the host setter's.
 * A reset world's mh_world_aux becomes the record of a freshly created batch, what mh_world_aux_init(&a, 1) gives: rand() at srand(1), time 0,
 * status 0, the warm starts _zlast / _z / _v empty, every counter 0 -- whatever sources were given, so a world that carried MH_WORLD_LCP_FAILED,
 * MH_WORLD_STALLED or MH_WORLD_UNSUPPORTED lives again.  Nothing else of it changes: not its parameter record, the stored drive, or the batch's
 * coordinates.  A world whose mask is 0 is not touched: not one byte of its q, qd, pose or aux is written.
 * The rule: after a reset, world w steps exactly as world w of a batch would after mh_artic_batch_upload and mh_artic_batch_set_base_pose had
 * written the same values and a fresh aux record into it -- state, aux record, base pose and report rows, bit for bit.  (q, qd, the pose and the
 * aux record are all that a world carries from one launch to the next: the solver workspace of a batch is scratch that every mini-step writes
 * before it reads.)
 * The values are NOT validated, as those of mh_artic_batch_set_params_dev are not.  A zero quaternion stores NaN in all four components (0 / 0), a
 * non-finite one NaN or, for an infinite component against finite ones, zeros and NaN; a non-finite p, q or qd is stored as it is.  What such a
 * world then does is what the step does with any non-finite state: no double of the state becomes an index, a count or a loop bound, so nothing
 * outside the world's own memory is touched; its state goes non-finite or it gets a status bit, and the other worlds are not affected.  The host
 * setter mh_artic_batch_set_base_pose is the validated route.
 * MH_ERR_INVALID_ARG: a NULL batch; a non-NULL pose_src on a batch in angle coordinates.
 *
 * mh_artic_batch_status_dev: aux[w].status into status_dst[w] (B ints) and aux[w].time into time_dst[w] (B doubles); either may be NULL.
 * MH_ERR_INVALID_ARG: a NULL batch; both NULL.
 *
 * mh_artic_batch_link_poses_dev: mh_artic_batch_link_poses into a caller buffer (B x nj x 12) on `stream`: the same kernels, so bit-equal to the
 * host call, in all four forms (the shared image or per-world images, angles or pose).  MH_ERR_INVALID_ARG: a NULL batch or buffer.
 * NOT built: a reset inside a multi-step launch (a world that ends mid-launch waits for the launch's end); a per-world seed (every reset world
 * restarts rand() at srand(1), as every created one does); validation on the device; link velocities; any of this in the large-world stepper
 * (moby_hip_stack.h). */
/* (no existing layout changes, so MH_VERSION stays as it is; a caller that needs to know tests this macro) */
#define MH_ARTIC_EPISODES 1
int mh_artic_batch_reset_dev(mh_artic_batch* ab, void* stream, const int* mask_dev,
                             const double* q_src, const double* qd_src, const double* pose_src);
int mh_artic_batch_status_dev(mh_artic_batch* ab, void* stream, int* status_dst, double* time_dst);
int mh_artic_batch_link_poses_dev(mh_artic_batch* ab, void* stream, double* poses_dst);

#ifdef __cplusplus
}
#endif
#endif
