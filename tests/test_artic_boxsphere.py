"""Box-sphere contacts between links and static boxes (include/moby_hip_artic.h, mh_artic_model.pair_kind, box_link = -1) without a GPU: the
readers, the box-sphere reference (tests/native/artic_boxsphere_ref.cpp) pinned to the pair reference where the feature is absent, the regions
of the reference's contact function against hand-computed contacts, and the physics of a box-sphere contact (head-on collision, a sphere
dropped on a static box against the same sphere dropped on a plane, non-penetration of an arm on a static box)."""
import os

import numpy as np
import pytest

from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import artic_pair_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "scenes")


@pytest.fixture(scope="module")
def ref():
    return BS.build_boxsphere_ref()


# ---- readers ----
def test_reader_box_sphere_scene():
    """the tip Sphere of a hinged arm can meet a Box on a second root and a Box on the fixed base: two box-sphere pairs, one static box"""
    m, links, _, q0, qd0, dt = A.load_xml(os.path.join(SCENES, "arm_box_sphere.xml"))
    assert (m.nj, m.nspheres, m.nboxes, m.npairs) == (3, 1, 2, 2)
    assert [m.pair_kind[k] for k in range(2)] == [A.MH_ARTIC_PAIR_BOX_SPHERE] * 2
    assert sorted(m.box_link[k] for k in range(2)) == [-1, links.index("cart")]
    assert all(m.pair_b[k] == 0 for k in range(2)) and sorted(m.pair_a[k] for k in range(2)) == [0, 1]
    st = [k for k in range(2) if m.box_link[k] < 0][0]
    assert np.allclose(m.box_center[st], (-0.5, -0.3, 0.0)) and list(m.box_len[st]) == [0.3, 0.1, 0.3]      # its pose in the model (base) frame
    assert m.sphere_no_plane == 0 and m.cp_epsilon == 0.2 and m.sphere_link[0] == links.index("l2")


def test_reader_still_refuses_box_box(tmp_path):
    from moby_amd import io as mio
    src = open(os.path.join(SCENES, "arm_box_sphere.xml")).read()
    f = tmp_path / "boxbox.xml"
    f.write_text(src.replace('<DisabledPair object1-id="cart" object2-id="post" />', ''))
    with pytest.raises(mio.SceneError, match="box-box contact between links is not supported"):
        A.load_xml(str(f))
    f = tmp_path / "staticsphere.xml"
    f.write_text(src.replace('<CollisionGeometry primitive-id="shelf" />', '<CollisionGeometry primitive-id="tip" />'))
    with pytest.raises(mio.SceneError, match="static Sphere"):
        A.load_xml(str(f))


def test_python_model_helpers():
    m, _, _ = BS.mixed_all()
    assert m.npairs == 3 and [m.pair_kind[k] for k in range(3)] == [0, 1, 1] and m.box_link[1] == -1
    assert (m.pair_a[1], m.pair_b[1], m.pair_a[2], m.pair_b[2]) == (1, 0, 1, 1) and m.sphere_no_plane == 2


# ---- the reference where the feature is absent ----
@pytest.mark.parametrize("name", ["arm_self", "arm_pendulum", "long_legs", "floating_legs", "mixed_box"])
def test_reference_without_the_feature_is_the_pair_reference(ref, name):
    """no box-sphere pair, no static box: artic_boxsphere_ref_step equals artic_pair_ref_step bit for bit, in angle and (floating bases) pose coordinates"""
    m, q, qd, dt = getattr(P, name)(4, 3)
    for pose in ([False, True] if m.floating_base else [False]):
        Pp = None
        if pose:
            Pp = np.tile(np.array([m.trel[0][0], m.trel[0][1], m.trel[0][2], 1.0, 0.0, 0.0, 0.0]), (4, 1))
        a = [q.copy(), qd.copy(), S.new_aux(4), None if Pp is None else Pp.copy()]
        b = [q.copy(), qd.copy(), S.new_aux(4), None if Pp is None else Pp.copy()]
        ref.step(m, a[0], a[1], a[2], dt, 150, pose=a[3])
        ref.pair_step(m, b[0], b[1], b[2], dt, 150, pose=b[3])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert a[2].tobytes() == b[2].tobytes()
        if pose: assert np.array_equal(a[3], b[3])
        assert (a[2]["lcp_solves"] > 0).any()


# ---- the regions of find_contacts_box_sphere ----
H = np.array([0.25, 0.15, 0.12])
RAD = 0.06


def probe_model():
    """a sphere on three sliders along x, y, z (q = its centre) and a static box at the origin with half lengths H"""
    ax = np.eye(3)
    links = [dict(parent=k - 1, type=A.MH_JOINT_PRISMATIC, R0=np.eye(3), x0=(0.0, 0.0, 0.0), axis=ax[k], com=(0.0, 0.0, 0.0),
                  inertia=np.eye(3) * (0.4 if k == 2 else 0.0), mass=1.0 if k == 2 else 0.0) for k in range(3)]
    m = A.model_from_links(links, gravity=(0.0, 0.0, 0.0))
    A.add_spheres(m, [(2, (0.0, 0.0, 0.0), RAD)], plane_normal=P.UP, plane_point=(0.0, -5.0, 0.0))
    A.add_boxes(m, [(-1, (0.0, 0.0, 0.0), np.eye(3), tuple(2 * H))], plane_normal=P.UP, plane_point=(0.0, -5.0, 0.0))
    A.add_box_sphere_pairs(m, [(0, 0)], no_plane=(0,))
    return m


@pytest.mark.parametrize("case", ["face", "edge", "vertex"])
def test_contact_regions_against_hand_computed_contacts(ref, case):
    """the OR of BoxPrimitive.cpp:237-238: over a face and over an edge the sphere point is not moved to the surface, so the contact point is the
    box point itself and the normal the unit vector from the sphere's centre to it; only over a vertex is the contact at the midpoint"""
    m = probe_model()
    if case == "face":            # above the top face, 0.01 clear
        c = np.array([0.1, H[1] + RAD + 0.01, 0.05]); p = np.array([0.1, H[1], 0.05]); n = np.array([0.0, -1.0, 0.0]); d = 0.01; reg = BS.FACE
    elif case == "edge":          # off the edge x = +hx, y = +hy by (0.06, 0.08): 0.1 from it, 0.04 clear
        c = np.array([H[0] + 0.06, H[1] + 0.08, 0.0]); p = np.array([H[0], H[1], 0.0]); n = np.array([-0.6, -0.8, 0.0]); d = 0.04; reg = BS.EDGE
    else:                         # off the corner by (0.04, 0.08, 0.08): 0.12 from it, 0.06 clear; the sphere point is halfway, the contact a quarter
        c = H + np.array([0.04, 0.08, 0.08]); p = H + np.array([0.01, 0.02, 0.02]); n = -np.array([1.0, 2.0, 2.0]) / 3.0; d = 0.06; reg = BS.VERTEX
    has, pt, nn, dist, region = ref.contact(m, c, 0, 0.1)
    assert has and region == reg
    assert np.max(np.abs(pt - p)) < 1e-15 and np.max(np.abs(nn - n)) < 1e-15 and abs(dist - d) < 1e-15
    if case != "vertex":          # ON the box
        assert np.all(np.abs(pt) <= H + 1e-15) and np.any(np.abs(np.abs(pt) - H) < 1e-15)
    assert not ref.contact(m, c, 0, d - 1e-6)[0]                           # accepted if dist <= TOL only
    # the signed-distance function (BoxPrimitive::calc_signed_dist) agrees on the distance here
    assert abs(BS.BoxSphereRef.regions(ref, m, c[None, :])[1][0, 0] - d) < 1e-15


def test_centre_inside_the_box_gives_the_reference_nan_normal(ref):
    m = probe_model()
    has, pt, nn, dist, region = ref.contact(m, np.array([0.1, 0.05, 0.02]), 0, 0.1)
    assert has and region == BS.INSIDE and np.isnan(nn).all() and dist == -RAD      # -min(0.1, R - 0)


# ---- physics ----
def head_on(mu):
    links = [P.slider((0.0, 5.0, 0.0), (1.0, 0.0, 0.0)), P.slider((1.0, 5.0, 0.0), (1.0, 0.0, 0.0))]
    m = A.model_from_links(links, gravity=(0.0, 0.0, 0.0))
    A.add_spheres(m, [(1, (0.0, 0.0, 0.0), 0.1)], plane_normal=P.UP, epsilon=1.0, mu_coulomb=mu)
    A.add_boxes(m, [(0, (0.0, 0.0, 0.0), np.eye(3), (0.4, 0.3, 0.3))], plane_normal=P.UP, epsilon=1.0, mu_coulomb=mu)
    A.add_box_sphere_pairs(m, [(0, 0)], no_plane=(0,))
    return m


@pytest.mark.parametrize("mu", [100.0, 0.0])
def test_head_on_collision_exchanges_the_velocities(ref, mu):
    """(a) a unit-mass sphere on a slider hits a unit-mass box on a slider head-on with epsilon = 1: the velocities exchange (no-slip and
    Drumwright-Shell).  Measured error: 0 under both models; the bound is the sphere pin's 1e-12."""
    m = head_on(mu)
    q = np.zeros((1, 2)); qd = np.array([[0.0, -1.0]]); aux = S.new_aux(1)
    ref.step(m, q, qd, aux, 1e-3, 900)
    err = max(abs(qd[0, 0] + 1.0), abs(qd[0, 1]))
    print("head-on mu = %g: qd = %r, error %.3e" % (mu, qd[0], err))
    assert aux["lcp_solves"][0] >= 1 and aux["status"][0] == 0
    assert err <= 1e-12
    assert 1.0 + q[0, 1] - q[0, 0] >= 0.2 + 0.1 - 1e-9                       # the sphere never entered the box: centre gap >= hx + R


DROP_DIFF = 7.622e-4       # the largest height difference measured with the reference (7.6216e-4): the bounces fall a mini-step apart


def test_drop_on_a_static_box_is_a_drop_on_a_plane(ref):
    """(b) a sphere on a vertical slider dropped on the top face of a static box, against the same sphere dropped on a plane at that height
    through the sphere route: the largest height difference over 1500 steps, asserted at ten times what the reference gave when the feature
    was written (DROP_DIFF)"""
    top = 0.4
    def model(static):
        m = A.model_from_links([P.slider((0.0, 1.0, 0.0), (0.0, 1.0, 0.0))], gravity=P.G)
        pp = (0.0, -5.0, 0.0) if static else (0.0, top, 0.0)
        A.add_spheres(m, [(0, (0.0, 0.0, 0.0), 0.1)], plane_normal=P.UP, plane_point=pp, epsilon=0.5, mu_coulomb=100.0)
        if static:
            A.add_boxes(m, [(-1, (0.0, top - 0.2, 0.0), np.eye(3), (1.0, 0.4, 1.0))], plane_normal=P.UP, plane_point=pp, epsilon=0.5, mu_coulomb=100.0)
            A.add_box_sphere_pairs(m, [(0, 0)], no_plane=(0,))
        m.cstab_max_iterations = 10
        return m
    ms, mp = model(True), model(False)
    a = [np.zeros((1, 1)), np.zeros((1, 1)), S.new_aux(1)]; b = [np.zeros((1, 1)), np.zeros((1, 1)), S.new_aux(1)]
    worst = 0.0
    for _ in range(1500):
        ref.step(ms, a[0], a[1], a[2], 1e-3, 1); ref.pair_step(mp, b[0], b[1], b[2], 1e-3, 1)
        worst = max(worst, abs(a[0][0, 0] - b[0][0, 0]))
    print("drop: largest height difference %.3e, bounces %d / %d" % (worst, a[2]["lcp_solves"][0], b[2]["lcp_solves"][0]))
    assert a[2]["lcp_solves"][0] >= 3 and a[2]["status"][0] == 0 and b[2]["status"][0] == 0
    assert 1.0 + a[0][0, 0] - 0.1 - top > -1e-6                              # resting on the face
    assert worst <= 10 * DROP_DIFF


def test_arm_on_a_static_box_does_not_penetrate(ref):
    """(c) an arm swings its tip sphere onto a static box with the stabiliser on for 2000 steps: no pair signed distance below -1e-6"""
    m, sampler, dt = BS.arm_static()
    q, qd = BS.aim(ref, m, sampler, 12, 21)
    aux = S.new_aux(len(q))
    worst = np.inf; touched = False
    for _ in range(100):
        ref.step(m, q, qd, aux, dt, 20)
        d = ref.regions(m, q)[1][:, 0]
        worst = min(worst, d.min()); touched = touched or (d < 1e-5).any()
    print("arm on a static box: smallest signed distance %.3e over %d worlds" % (worst, len(q)))
    assert touched and (aux["status"] & ~S.MH_WORLD_IMPACT_TOL == 0).all()
    assert worst >= -1e-6
