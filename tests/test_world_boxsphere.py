"""Box-sphere contacts between free bodies (include/moby_hip.h, "Box-sphere pairs") without a GPU: the reference the kernels are held to
(tests/native/world_ref.cpp, a restatement of what the pair changes in oracle::World) pinned to the oracle -- with no box-sphere pair
enabled it IS oracle_world_step_batch -- and to the geometry written out by hand in numpy on dyadic inputs; both id orders of the pair; what a
contact must do physically (a head-on hit, a ball resting on a crate); the scene file and the scene check.  The reference's ctypes face lives in
tests/world_ref.py, the batches shared with the GPU tests in tests/world_boxsphere_ref.py."""
import ctypes

import numpy as np
import pytest

from moby_amd import io as mio
from moby_amd import scene as S
from tests.world_ref import assert_aux_equal, reference
from tests.world_boxsphere_ref import BOX_DIMS, RADIUS, SCENE_XML, disabled_mixed_batch, mixed_scene



@pytest.fixture(scope="session")
def ref():
    return reference()


# ---- 1. no box-sphere pair: the oracle ---------------------------------------------------------------------------------------------------------
PIN = {
    "mixed_disabled": lambda: disabled_mixed_batch(6) + (0.01,),
    "sphere_stack": lambda: (S.sphere_stack_scene(), S.sphere_stack_state(6), 0.01),
}


@pytest.mark.parametrize("name", sorted(PIN))
def test_reference_without_the_pair_is_the_oracle(oracle, ref, name):
    """6 worlds x 40 steps: states and whole aux records equal oracle_world_step_batch bit for bit"""
    sc, st0, dt = PIN[name]()
    B = st0.shape[0]
    st_o, aux_o = st0.copy(), S.new_aux(B)
    oracle.world_step_batch(sc, st_o, aux_o, dt, 40)
    assert (aux_o["lcp_solves"] > 0).all() and aux_o["stab_iters"].sum() > 0
    st_r, aux_r = st0.copy(), S.new_aux(B)
    ref.step(sc, st_r, aux_r, dt, 40)
    np.testing.assert_array_equal(st_r, st_o)
    assert_aux_equal(aux_r, aux_o)
    assert aux_r.tobytes() == aux_o.tobytes()


# ---- 2. geometry against numpy written out by hand ---------------------------------------------------------------------------------------------
# Box half lengths h = (1, 0.5, 0.75); every number below is a multiple of 2^-4, and the offsets of the edge and vertex cases are 3-4-5 triples
# (0.375, 0.5 -> 0.625; 0.75, 1 -> 1.25), so every operation of the two functions is exact except the division that normalises such an offset:
# that one is a single correctly rounded division of the same operands on both sides.  Two box poses, both exact: the identity at the origin, and a
# half turn about z (quaternion (0, 0, 1, 0): rotation diag(-1, -1, 1)) at (0.5, -0.25, 2).  (A quarter turn's quaternion has components sqrt(1/2),
# whose products are not exact: the rotation the stepper forms from it is not a permutation matrix.)
DIMS = (2.0, 1.0, 1.5)
POSES = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0), np.diag([1.0, 1.0, 1.0])), ((0.5, -0.25, 2.0), (0.0, 0.0, 1.0, 0.0), np.diag([-1.0, -1.0, 1.0]))]
nan = float("nan")
# name: (sphere centre c in the box frame, radius, TOL) -> (has, dist, point, normal, region), point and normal in the box frame
CONTACTS = {
    # face region: p = (0.25, 0.5, 0.125), v = (0, -0.625, 0); the sphere point stays c + v = p, so box point - sphere point = 0 <= NEAR_ZERO and the
    # normal is the fallback: the unit vector from the centre to p
    "face_separated": ((0.25, 1.125, 0.125), 0.5, 0.25, (1, 0.125, (0.25, 0.5, 0.125), (0.0, -1.0, 0.0), 0)),
    "face_out_of_tolerance": ((0.25, 1.125, 0.125), 0.5, 0.0625, (0, 0.125, None, None, 0)),
    "face_touching": ((0.25, 1.0, 0.125), 0.5, 0.0, (1, 0.0, (0.25, 0.5, 0.125), (0.0, -1.0, 0.0), 0)),
    # edge region: p = (1, 0.5, 0.25), v = (-0.375, -0.5, 0), |v| = 0.625
    "edge_separated": ((1.375, 1.0, 0.25), 0.5, 0.25, (1, 0.125, (1.0, 0.5, 0.25), (-0.375 / 0.625, -0.5 / 0.625, 0.0), 1)),
    "edge_touching": ((1.375, 1.0, 0.25), 0.625, 0.0, (1, 0.0, (1.0, 0.5, 0.25), (-0.375 / 0.625, -0.5 / 0.625, 0.0), 1)),
    # vertex region: p = (1, 0.5, 0.75), v = (-0.75, -1, 0), |v| = 1.25; R = 0.625: the sphere point is c + v / 2 = (1.375, 1, 0.75), dist = |(0.375, 0.5, 0)|,
    # the point the midpoint, the normal the pair's own (box point - sphere point) / 0.625
    "vertex_separated": ((1.75, 1.5, 0.75), 0.625, 1.0, (1, 0.625, (1.1875, 0.75, 0.75), (-0.375 / 0.625, -0.5 / 0.625, 0.0), 2)),
    # R = |v|: not < R, so still the vertex branch; the sphere point is p itself, dist = 0, the normal the fallback v / |v|
    "vertex_touching": ((1.75, 1.5, 0.75), 1.25, 0.0, (1, 0.0, (1.0, 0.5, 0.75), (-0.75 / 1.25, -1.0 / 1.25, 0.0), 2)),
    # the centre inside the box: p = c, v = 0, depths h - |c| = (0.75, 0.25, 0.625); dist = -min(0.25, R - 0): R - |v| wins for R = 0.125, the box depth
    # for R = 0.5; the point is the centre, the normal 0 / 0
    "inside_radius_wins": ((0.25, 0.25, 0.125), 0.125, 0.0, (1, -0.125, (0.25, 0.25, 0.125), (nan, nan, nan), 3)),
    "inside_depth_wins": ((0.25, 0.25, 0.125), 0.5, 0.0, (1, -0.25, (0.25, 0.25, 0.125), (nan, nan, nan), 3)),
    # the centre outside, the sphere overlapping the face: one coordinate of p is at its extent, so the box depth is 0 and dist = -min(0, R - |v|) = -0
    "overlapping_face": ((0.25, 0.75, 0.125), 0.5, 0.0, (1, 0.0, (0.25, 0.5, 0.125), (0.0, -1.0, 0.0), 0)),
}
# name: (c, radius) -> (dist, box point, sphere point), box frame
DISTS = {
    "face": ((0.25, 1.125, 0.125), 0.5, (0.125, (0.25, 0.5, 0.125), (0.25, 1.125 + (-0.625) * (0.5 / 0.625), 0.125))),
    "edge": ((1.375, 1.0, 0.25), 0.5, (0.125, (1.0, 0.5, 0.25), (1.375 + (-0.375) * (0.5 / 0.625), 1.0 + (-0.5) * (0.5 / 0.625), 0.25))),
    "vertex": ((1.75, 1.5, 0.75), 0.625, (0.625, (1.0, 0.5, 0.75), (1.375, 1.0, 0.75))),
    # overlapping from outside: dist = 0.25 - 0.5 < 0, the sphere point c + v (R + dist) / |v| = the box point
    "overlapping_face": ((0.25, 0.75, 0.125), 0.5, (-0.25, (0.25, 0.5, 0.125), (0.25, 0.75 + (-0.25) * (0.25 / 0.25), 0.125))),
    # the interior branch: max_i(-min(|h_i - c_i|, |c_i + h_i|)) = max(-0.75, -0.25, -0.625) = -0.25, minus R; v = 0: the sphere point is the centre
    "interior": ((0.25, 0.25, 0.125), 0.5, (-0.75, (0.25, 0.25, 0.125), (0.25, 0.25, 0.125))),
    # on the surface: v = 0 without being inside in the strict sense (c_y = h_y takes the interior branch: -min(0, 1) = -0): the centre again
    "centre_on_face": ((0.25, 0.5, 0.125), 0.25, (-0.25, (0.25, 0.5, 0.125), (0.25, 0.5, 0.125))),
}


def to_world(pose, v, point=True):
    cb, _, Rw = pose
    return (np.array(cb) if point else 0.0) + Rw @ np.array(v)


@pytest.mark.parametrize("pose", range(len(POSES)))
@pytest.mark.parametrize("name", sorted(CONTACTS))
def test_contact_geometry_equals_the_hand_written_values(ref, name, pose):
    P = POSES[pose]
    c, radius, TOL, (has, dist, point, normal, region) = CONTACTS[name]
    got = ref.contact(P[0], P[1], DIMS, to_world(P, c), radius, TOL)
    assert got["has"] == has and got["region"] == region
    assert got["dist"] == dist
    if has:
        np.testing.assert_array_equal(got["point"], to_world(P, point))
        np.testing.assert_array_equal(got["normal"], to_world(P, normal, point=False))       # (NaN == NaN for assert_array_equal)


@pytest.mark.parametrize("pose", range(len(POSES)))
@pytest.mark.parametrize("name", sorted(DISTS))
def test_signed_distance_equals_the_hand_written_values(ref, name, pose):
    P = POSES[pose]
    c, radius, (dist, pbox, psph) = DISTS[name]
    d, pa, pb = ref.dist(P[0], P[1], DIMS, to_world(P, c), radius)
    assert d == dist
    np.testing.assert_array_equal(pa, to_world(P, pbox))
    np.testing.assert_array_equal(pb, to_world(P, psph))


def test_contact_and_signed_distance_are_different_functions(ref):
    """the sphere overlapping a face from outside: the contact function says -0, the signed-distance function 0.25 - R"""
    P = POSES[0]
    c = CONTACTS["overlapping_face"][0]
    assert ref.contact(P[0], P[1], DIMS, c, 0.5, 0.0)["dist"] == 0.0 and ref.dist(P[0], P[1], DIMS, c, 0.5)[0] == -0.25


def test_geometry_equals_the_articulated_reference_on_bit_identical_poses(ref):
    """tests/native/artic_boxsphere_ref.cpp with a static axis-aligned box at the origin and the sphere on three sliders with zero offsets (q = its
    centre): the same contact (found, point, normal, distance, region) and the same signed distance, bit for bit, on every case of the tables"""
    from moby_amd import artic as A
    from tests import artic_boxsphere_ref as BS
    from tests import artic_pair_ref as APR
    aref = BS.build_boxsphere_ref()
    cb, quat, _ = POSES[0]

    def model(radius):
        links = [dict(parent=k - 1, type=A.MH_JOINT_PRISMATIC, R0=np.eye(3), x0=(0.0, 0.0, 0.0), axis=np.eye(3)[k], com=(0.0, 0.0, 0.0),
                      inertia=np.eye(3) * (0.4 if k == 2 else 0.0), mass=1.0 if k == 2 else 0.0) for k in range(3)]
        m = A.model_from_links(links, gravity=(0.0, 0.0, 0.0))
        A.add_spheres(m, [(2, (0.0, 0.0, 0.0), radius)], plane_normal=APR.UP, plane_point=(0.0, -50.0, 0.0))
        A.add_boxes(m, [(-1, (0.0, 0.0, 0.0), np.eye(3), DIMS)], plane_normal=APR.UP, plane_point=(0.0, -50.0, 0.0))
        A.add_box_sphere_pairs(m, [(0, 0)], no_plane=(0,))
        return m

    for name, (c, radius, TOL, _) in sorted(CONTACTS.items()):
        got = ref.contact(cb, quat, DIMS, c, radius, TOL)
        has, pt, nn, dist, region = aref.contact(model(radius), np.array(c), 0, TOL)
        assert (int(has), region) == (got["has"], got["region"]), name
        assert dist == got["dist"], name
        if has:
            np.testing.assert_array_equal(pt, got["point"], err_msg=name)
            np.testing.assert_array_equal(nn, got["normal"], err_msg=name)
    for name, (c, radius, _) in sorted(DISTS.items()):
        assert aref.regions(model(radius), np.array(c)[None, :])[1][0, 0] == ref.dist(cb, quat, DIMS, c, radius)[0], name


# ---- 3. both id orders -------------------------------------------------------------------------------------------------------------------------
def test_both_id_orders_give_the_same_contact(ref):
    """(box 0, sphere 1) and the relabelled (sphere 0, box 1): the same contact with g1 = the box; the signed-distance points swap with the bodies"""
    q = np.array([0.1, -0.3, 0.2, 0.9]); q /= np.linalg.norm(q)
    box = np.zeros(13); box[:3] = (0.3, 1.0, -0.2); box[3:7] = q
    for centre in ((0.3, 1.0 + 0.25 + RADIUS + 1e-3, -0.2), (1.1, 1.6, 0.4), (0.35, 1.05, -0.15)):
        sph = np.zeros(13); sph[:3] = centre; sph[6] = 1.0
        a = ref.pair(S.ball_on_crate_scene(), np.concatenate([box, sph]), 0, 10.0)
        b = ref.pair(S.ball_on_crate_scene(sphere_first=True), np.concatenate([sph, box]), 0, 10.0)
        assert (a["a"], a["b"], b["a"], b["b"]) == (0, 1, 0, 1)
        assert a["ncontacts"] == b["ncontacts"] == 1 and (a["g1"], a["g2"]) == (0, 1) and (b["g1"], b["g2"]) == (1, 0)
        for f in ("cdist", "point", "normal", "dist"):
            np.testing.assert_array_equal(a[f], b[f], err_msg=f)
        np.testing.assert_array_equal(a["pa"], b["pb"])
        np.testing.assert_array_equal(a["pb"], b["pa"])
    # the normal points from the sphere towards the box (last case: the centre is inside, the normal NaN)
    sph = np.zeros(13); sph[:3] = (0.3, 3.0, -0.2); sph[6] = 1.0
    n = ref.pair(S.ball_on_crate_scene(), np.concatenate([box, sph]), 0, 10.0)["normal"]
    assert np.dot(n, box[:3] - sph[:3]) > 0


# ---- 4. physics ----------------------------------------------------------------------------------------------------------------------------------
def test_head_on_hit_conserves_momentum_and_restitutes(ref):
    """A sphere hits the +x face of a box through both centres of mass, no gravity, no friction, epsilon = 0.5.  Linear momentum is conserved to
    round-off and the separating normal speed is epsilon x the approach speed.  Tolerance 1e-12, absolute, on velocities of order 1: the one
    tests/test_oracle_world.py::test_bouncing_ball_energy_and_restitution holds its post-impact velocities to."""
    eps, mb, ms = 0.5, 3.0, 0.5
    sc = S.ball_on_crate_scene(box_mass=mb, ball_mass=ms, epsilon=eps, mu_coulomb=0.0, gravity=(0.0, 0.0, 0.0), ground=False)
    st = np.zeros((1, 2, 13)); st[:, :, 6] = 1.0
    st[0, 1, 0] = 0.5 * BOX_DIMS[0] + RADIUS + 2.5e-3; st[0, 1, 7] = -1.0
    p0 = mb * st[0, 0, 7:10] + ms * st[0, 1, 7:10]
    st = st.reshape(1, -1); aux = S.new_aux(1)
    census = ref.step(sc, st, aux, 1e-3, 10, want_census=True).census
    assert aux["status"][0] == 0 and aux["lcp_solves"][0] > 0 and census[0, :, 0].sum() > 0
    v = st.reshape(2, 13)[:, 7:10]; w = st.reshape(2, 13)[:, 10:13]
    print("momentum error", mb * v[0] + ms * v[1] - p0, "separating speed", v[1, 0] - v[0, 0])
    np.testing.assert_allclose(mb * v[0] + ms * v[1], p0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(v[1, 0] - v[0, 0], eps * 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.concatenate([v[:, 1:].ravel(), w.ravel()]), 0.0, rtol=0, atol=1e-12)


def test_ball_rests_on_a_crate_on_the_plane(ref):
    """a ball at rest on a crate at rest on the plane, 200 steps: no error bit besides MH_WORLD_IMPACT_TOL / MH_WORLD_STAB_FAILED, both heights within
    contact_dist_thresh + cstab_eps of their start"""
    sc = S.ball_on_crate_scene(epsilon=0.0)
    st = S.ball_on_crate_state(1, gap=0.0, speed=0.0); aux = S.new_aux(1)
    traj, census = ref.step(sc, st, aux, 1e-3, 200, want_traj=True, want_census=True)[:2]
    assert (aux["status"][0] & ~(S.MH_WORLD_IMPACT_TOL | S.MH_WORLD_STAB_FAILED)) == 0
    assert aux["lcp_solves"][0] > 0 and census[0, :, 0].sum() > 0
    y0 = np.array([0.5 * BOX_DIMS[1], BOX_DIMS[1] + RADIUS])
    drift = np.abs(traj[0, :, :, 1] - y0).max(axis=0)
    print("largest height change (box, ball)", drift)
    assert (drift <= sc.contact_dist_thresh + sc.cstab_eps).all()


# ---- 5. loader and scene check ---------------------------------------------------------------------------------------------------------------------
def test_full_image_with_parameters_per_pair_meets_its_conditions(ref):
    """the "full_params" batch of the GPU tests as an input: 36 slots over ntot = 9 with pairwise different (epsilon, mu-coulomb, NK), NK in {4, 8}; beside
    the six box-box pairs two sphere-sphere pairs and one sphere-ground pair are disabled.  reference_run asserts the rest (check_full_params_conditions):
    no fatal bit, LCPs solved, the mini-step cap, contacts on box-sphere, sphere-sphere and box-ground slots, the ball sinking into the disabled plane"""
    from tests import world_boxsphere_ref as W
    c, st, aux, _, _ = W.reference_run("full_params")
    sc = c["scene"]
    assert (sc.nb, sc.has_ground) == (8, 1)
    triples = [(sc.cp_epsilon[p], sc.cp_mu_coulomb[p], sc.cp_nk[p]) for p in range(36)]
    en = {(i, j): sc.pair_enabled[S.pair_index(i, j, 9)] for i in range(9) for j in range(i + 1, 9)}
    assert len(set(triples[p] for p in range(36) if sc.pair_enabled[p])) == sum(en.values()) == 36 - 6 - 3 and {t[2] for t in triples} == {4, 8}
    assert [k for k in sorted(en) if not en[k] and k in W.FULL_PARAMS_DISABLED] == W.FULL_PARAMS_DISABLED
    assert (aux["mini_steps"] <= 50 * c["nsteps"]).all()
    assert not np.array_equal(st, W.reference_run("full")[1])


def test_scene_file_loads_with_its_three_pairs(ref):
    sc, st, ids, dt = mio.load_xml(SCENE_XML)
    assert ids == ["ball", "crate", "ground"] and sc.nb == 2 and sc.has_ground == 1 and dt == 1e-3
    assert [sc.geom_type[b] for b in range(2)] == [S.MH_GEOM_SPHERE, S.MH_GEOM_BOX]
    assert sc.geom_dim[0][0] == 0.25 and [sc.geom_dim[1][k] for k in range(3)] == [1.0, 0.5, 0.8]
    want = {(0, 1): (0.2, 0.4, 4), (0, 2): (0.1, 0.5, 8), (1, 2): (0.0, 0.3, 8)}
    for (i, j), (e, mu, nk) in want.items():
        p = S.pair_index(i, j, 3)
        assert sc.pair_enabled[p] == 1 and (sc.cp_epsilon[p], sc.cp_mu_coulomb[p], sc.cp_nk[p]) == (e, mu, nk), (i, j)
    np.testing.assert_array_equal(st.reshape(2, 13)[:, :3], [[0.0, 0.752, 0.0], [0.0, 0.25, 0.0]])
    # the reference steps it: the scene is in scope (no MH_WORLD_UNSUPPORTED from the broad phase) and the ball lands on the crate
    aux = S.new_aux(1); s = st.copy()
    census = ref.step(sc, s, aux, dt, 30, want_census=True).census
    assert (aux["status"][0] & ~S.MH_WORLD_IMPACT_TOL) == 0 and census[0, :, 0].sum() > 0


def test_scene_check_accepts_box_sphere_and_still_refuses_box_box():
    """mh_world_batch_create checks the scene before it looks for a device: a refusal is MH_ERR_INVALID_ARG with its message, an accepted scene gets past
    the check (MH_ERR_NO_DEVICE without a GPU, a batch with one)"""
    from moby_amd import _lib
    lib = _lib.load()
    assert lib.mh_version() >= 102

    def create(sc):
        h = ctypes.c_void_p()
        rc = lib.mh_world_batch_create(ctypes.addressof(sc), 1, ctypes.byref(h))
        msg = lib.mh_last_error().decode()
        if rc == _lib.MH_OK:
            lib.mh_world_batch_destroy(h)
        return rc, msg

    for sc in (mio.load_xml(SCENE_XML)[0], S.ball_on_crate_scene(), S.ball_on_crate_scene(sphere_first=True)):
        rc, msg = create(sc)
        assert rc in (_lib.MH_OK, _lib.MH_ERR_NO_DEVICE), (rc, msg)
    sc = mixed_scene([("box", BOX_DIMS, 3.0), ("sphere", RADIUS, 0.5), ("box", BOX_DIMS, 3.0)])
    assert create(sc)[0] in (_lib.MH_OK, _lib.MH_ERR_NO_DEVICE)             # the box-box pair disabled
    sc.pair_enabled[S.pair_index(0, 2, 4)] = 1
    rc, msg = create(sc)
    assert rc == _lib.MH_ERR_INVALID_ARG and "bodies 0,2: box-box contact is not built" in msg and "box-sphere" not in msg.split(";")[0], msg
