"""Sphere contacts between links (include/moby_hip_artic.h, mh_artic_model.npairs / sphere_no_plane) without a GPU: the pair reference
(tests/native/artic_pair_ref.cpp) pinned to the box reference on models without pairs, the physics of a pair contact (head-on collision, the
reference's sphere stack, three dropped spheres against the rigid-body oracle, non-penetration of an arm hitting a pendulum), the readers,
and the conservative advancement of a second root."""
import os

import numpy as np
import pytest

from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_pair_ref as P
from tests.artic_box_ref import build_box_ref
from tests.test_artic_drive import FIELDS, random_drive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "scenes")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def pair_ref():
    return P.build_pair_ref()


@pytest.fixture(scope="module")
def box_ref():
    return build_box_ref()


def assert_same(a, b):
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x, y), "max diff %.3e" % np.max(np.abs(x - y))
    for f in FIELDS:
        assert np.array_equal(a[2][f], b[2][f]), f
    for f in ("vns", "zlast", "zbuf"):
        assert np.array_equal(a[2][f], b[2][f]), f


def pin_scenes():
    """the box tests' scenes: sphere-only (XML), boxes (XML) and the mixed sphere-and-box body"""
    from tests.test_artic_box import PIN_SCENES, pin_state
    from tests.test_artic_box_gpu import mixed, scene
    out = {}
    for name in PIN_SCENES:
        out[name] = (lambda n=name: pin_state(n))
    out["sitting_box_ds"] = lambda: scene("floating_sitting_box.xml", 2, 1, iters=10) + (25,)
    out["table_noslip"] = lambda: scene("floating_box_table.xml", 3, 3) + (60,)
    out["arm_box_foot"] = lambda: scene("arm_with_box_foot_urdf.xml", 3, 5, iters=10) + (60,)
    out["mixed"] = lambda: mixed(3, 6) + (60,)
    return out


@pytest.mark.parametrize("name", ["arm_on_table", "floating_welded_pair", "floating_spinning_ball", "sitting_box_ds", "table_noslip", "arm_box_foot", "mixed"])
@pytest.mark.parametrize("stab", [False, True])
def test_pair_reference_without_pairs_is_the_box_reference(pair_ref, box_ref, name, stab):
    """test 1 (and 7, first half): npairs = 0, sphere_no_plane = 0 -- the restated handle_impacts / stabilize / calc_max_dist step exactly as
    artic_box_ref_step: plain, driven and, for floating bases, in pose coordinates"""
    m, q, qd, dt, n = pin_scenes()[name]()
    if not stab: m.cstab_max_iterations = 0
    assert m.npairs == 0 and m.sphere_no_plane == 0
    B, nj = q.shape
    for driven in (False, True):
        d = random_drive(np.random.default_rng(5), B, nj, rows=n, tau=2.0) if driven else None
        a = [q.copy(), qd.copy(), S.new_aux(B)]; b = [q.copy(), qd.copy(), S.new_aux(B)]
        pair_ref.step(m, a[0], a[1], a[2], dt, n, drive=d)
        box_ref.step(m, b[0], b[1], b[2], dt, n, drive=d)
        assert_same(a, b)
        if not driven: assert (b[2]["lcp_solves"] > 0).any()
        if m.floating_base:
            from tests.test_artic_pose import model_pose
            P0 = model_pose(m, B)
            a = [np.zeros_like(q), qd.copy(), S.new_aux(B)]; b = [np.zeros_like(q), qd.copy(), S.new_aux(B)]
            Pa, Pb = P0.copy(), P0.copy()
            pair_ref.step(m, a[0], a[1], a[2], dt, n, pose=Pa, drive=d)
            box_ref.step(m, b[0], b[1], b[2], dt, n, pose=Pb, drive=d)
            assert_same(a, b)
            assert np.array_equal(Pa, Pb)


@pytest.mark.parametrize("mu", [100.0, 0.0])
@pytest.mark.parametrize("eps", [1.0, 0.0])
def test_head_on_collision_of_two_equal_spheres(pair_ref, mu, eps):
    """test 2: two equal spheres on parallel prismatic roots, gravity off, masked off the plane.  Restitution 1 exchanges the velocities,
    restitution 0 leaves both at the mean; m1 v1 + m2 v2 is kept.  Exact in real arithmetic: 1e-12 relative, under both impact models."""
    m = A.model_from_links([P.slider((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)), P.slider((1.0, 0.0, 0.0), (1.0, 0.0, 0.0))], gravity=(0.0, 0.0, 0.0))
    A.add_spheres(m, [(0, (0.0, 0.0, 0.0), 0.1), (1, (0.0, 0.0, 0.0), 0.1)], plane_normal=(0.0, 1.0, 0.0), plane_point=(0.0, -5.0, 0.0), epsilon=eps, mu_coulomb=mu)
    A.add_pairs(m, [(1, 0)], no_plane=(0, 1))
    v1, v2 = 1.0, -0.5
    q = np.zeros((1, 2)); qd = np.array([[v1, v2]]); aux = S.new_aux(1)
    pair_ref.step(m, q, qd, aux, 1e-2, 100)
    assert aux["status"][0] == 0 and aux["lcp_solves"][0] >= 1
    want = (v2, v1) if eps == 1.0 else (0.5 * (v1 + v2),) * 2
    print("head-on mu=%g eps=%g: qd = %r, want %r" % (mu, eps, qd[0], want))
    np.testing.assert_allclose(qd[0], want, rtol=1e-12, atol=0)
    assert abs((qd[0, 0] + qd[0, 1]) - (v1 + v2)) <= 1e-12 * abs(v1 + v2)
    # they did not pass through each other.  (calc_max_dist bounds a slider's travel by 2 rmax |qd|, as the reference's articulated form does,
    # so the landing mini-step may overshoot by less than one step's closing travel, 1.5e-2; the stabiliser is off here)
    gap = (1.0 + q[0, 1]) - q[0, 0] - 0.2
    assert gap > -1.5e-2
    if eps == 1.0: assert gap > 0.1


def test_sphere_stack_follows_the_reference_recording(pair_ref):
    """test 3: example/stacks/sphere-stack.xml as three vertical sliders (one plane contact, two pairs, mu = 0, 16 cone edges): the heights follow
    the z columns of regress/sphere-stack.dat to the file's six printed digits (atol 1e-6, as tests/test_oracle_world.py), no world flagged"""
    g = np.load(os.path.join(GOLD, "sphere_stack_dat.npz"))
    m = P.sphere_stack()
    q = np.zeros((1, 3)); qd = np.zeros((1, 3)); aux = S.new_aux(1)
    done = 0; worst = 0.0
    for row, k in zip(g["rows"], g["row_index"]):
        k = int(k)
        pair_ref.step(m, q, qd, aux, 1e-3, k - done); done = k
        z = np.array([1.0, 3.0, 5.0]) + q[0]
        worst = max(worst, np.abs(z - row[1:][[2, 9, 16]]).max())
        np.testing.assert_allclose(z, row[1:][[2, 9, 16]], rtol=0, atol=1e-6, err_msg="row %d" % k)
    print("sphere stack: largest height difference to the recording %.3e" % worst)
    assert aux["status"][0] == 0


def test_sphere_stack_first_impact_is_a_42_row_lcp(pair_ref):
    """test 3, second half: as the rigid oracle's first step, the first step solves one impact LCP of 42 rows (3 contacts x (6 + 16/2)) and leaves
    every sphere at rest"""
    m = P.sphere_stack()
    q = np.zeros((1, 3)); qd = np.zeros((1, 3)); aux = S.new_aux(1)
    pair_ref.step(m, q, qd, aux, 1e-3, 1)
    assert aux["status"][0] == 0
    assert int(aux["lcp_rows"][0]) - int(aux["stab_rows"][0]) == 42 and int(aux["lcp_solves"][0]) >= 1
    assert np.abs(qd).max() < 1e-14


def test_three_dropped_spheres_against_the_rigid_oracle(oracle, pair_ref):
    """test 4: the stack's three spheres dropped from separated heights (1.2, 3.6, 6.1), stepped as sliders by the pair reference and as three free
    spheres by the rigid-body oracle (oracle.world_step, the sphere-stack scene).  The two differ in coordinates and in impact bookkeeping;
    measured on the CPU (g++, the oracle's flags) over 1500 steps the largest height difference is 1.812e-6 (printed below); the bound is ten times
    that, far below the 1e-3 an O(dt) error would show."""
    sc = S.sphere_stack_scene()
    st = S.sphere_stack_state(1, perturb=False)[0].copy().reshape(3, 13)
    h0 = np.array([1.2, 3.6, 6.1])
    st[:, 2] = h0
    st = st.ravel(); aux = S.new_aux(1)
    m = P.sphere_stack(heights=tuple(h0))
    q = np.zeros((1, 3)); qd = np.zeros((1, 3)); ax = S.new_aux(1)
    worst = 0.0
    for k in range(1500):
        oracle.world_step(sc, st, aux, 1e-3, 1, want_traj=False)
        pair_ref.step(m, q, qd, ax, 1e-3, 1)
        worst = max(worst, np.abs((h0 + q[0]) - st.reshape(3, 13)[:, 2]).max())
    print("dropped spheres: largest height difference to the rigid oracle %.3e" % worst)
    assert ax["status"][0] & ~S.MH_WORLD_IMPACT_TOL == 0 and ax["lcp_solves"][0] > 0
    assert (h0 + q[0])[0] < 1.01                                            # they did land
    assert worst < 10 * 1.812e-6


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_arm_hitting_a_pendulum_never_penetrates(pair_ref, seed):
    """test 5: a two-link arm whose tip sphere swings into the bob of a pendulum on a second root, stabiliser on, 2000 steps: no pair distance
    below -1e-6 after any completed step (the tumbling die's bound), no world flagged, every world finishes"""
    B = 4
    m, q, qd, dt = P.arm_pendulum(B, seed)
    aux = S.new_aux(B)
    low = np.full(B, np.inf); touched = np.zeros(B, bool)
    for k in range(2000):
        pair_ref.step(m, q, qd, aux, dt, 1)
        assert (aux["status"] == 0).all(), "step %d: status %r" % (k, aux["status"])
        d = pair_distance(m, q)
        low = np.minimum(low, d); touched |= d < 1e-3
    print("arm and pendulum, seed %d: lowest pair distance %r" % (seed, low))
    assert (aux["steps"] == 2000).all()
    assert low.min() > -1e-6
    assert touched.any() and (aux["lcp_solves"] > 0).all()                   # the pair did meet (sampled after whole steps: within a millimetre)


def pair_distance(m, q):
    """pair 0's signed distance of planar (z-hinge, identity rest frames) chains, computed independently of the reference"""
    out = []
    for b in range(q.shape[0]):
        c = []
        for s in (m.pair_a[0], m.pair_b[0]):
            l = m.sphere_link[s]; chain = []
            while l >= 0:
                chain.append(l); l = m.parent[l]
            x = np.zeros(3); ang = 0.0
            for l in reversed(chain):
                c_, s_ = np.cos(ang), np.sin(ang)
                R = np.array([[c_, -s_, 0], [s_, c_, 0], [0, 0, 1.0]])
                x = x + R @ np.array(m.trel[l]); ang += q[b, l]
            c_, s_ = np.cos(ang), np.sin(ang)
            R = np.array([[c_, -s_, 0], [s_, c_, 0], [0, 0, 1.0]])
            c.append(x + R @ np.array(m.sphere_center[s]))
        out.append(np.linalg.norm(c[0] - c[1]) - m.sphere_radius[m.pair_a[0]] - m.sphere_radius[m.pair_b[0]])
    return np.array(out)


def test_reader_self_collision_scene():
    """test 6: two link spheres whose pair is not disabled load as a pair; l1's pair with the ground is disabled, so it is masked off the plane"""
    m, links, _, q0, _, dt = A.load_xml(os.path.join(SCENES, "arm_self_collision.xml"))
    assert (m.nj, m.nspheres, m.nboxes, m.npairs, links) == (3, 2, 0, 1, ["l1", "l2", "l3"])
    assert (m.pair_a[0], m.pair_b[0]) == (0, 1) and (m.sphere_link[0], m.sphere_link[1]) == (0, 2)
    assert m.sphere_no_plane == 1 and m.cp_epsilon == 0.2 and m.cp_mu_coulomb == 100.0 and m.cstab_max_iterations == 10
    assert list(m.plane_o) == [0.0, -1.3, 0.0]


def test_reader_disabled_pair_loads_as_before(tmp_path):
    """test 6: the same scene with the <DisabledPair> has no pair, and drops l1's sphere as it always did"""
    src = open(os.path.join(SCENES, "arm_self_collision.xml")).read()
    f = tmp_path / "disabled.xml"
    f.write_text(src.replace('<DisabledPair object1-id="l1" object2-id="ground" />',
                             '<DisabledPair object1-id="l1" object2-id="ground" />\n      <DisabledPair object1-id="l1" object2-id="l3" />'))
    m, _, _, _, _, _ = A.load_xml(str(f))
    assert (m.nspheres, m.npairs, m.sphere_no_plane) == (1, 0, 0) and m.sphere_link[0] == 2


def test_reader_refuses_box_pairs_and_base_geometry(tmp_path):
    """test 6: a pair that involves a box, or a geometry on the fixed base, keeps the refusal, with a message that names what is missing"""
    from moby_amd import io as mio
    src = open(os.path.join(SCENES, "arm_self_collision.xml")).read()
    f = tmp_path / "boxpair.xml"
    f.write_text(src.replace('<Sphere id="tip" radius="0.06" mass="0.3" />', '<Box id="tip" xlen="0.1" ylen="0.1" zlen="0.1" mass="0.3" />'))
    with pytest.raises(mio.SceneError, match="between two Spheres only"):
        A.load_xml(str(f))
    f = tmp_path / "basegeom.xml"
    f.write_text(src.replace('<RigidBody id="base" position="0 0 0" />', '<RigidBody id="base" position="0 0 0">\n<CollisionGeometry primitive-id="ball" />\n</RigidBody>'))
    with pytest.raises(mio.SceneError, match="fixed base"):
        A.load_xml(str(f))


def test_second_root_advancement_ignores_the_floating_base(pair_ref):
    """test 7: calc_max_dist adds the floating base's linear velocity only for links that descend from joint 0 -- the bound of the second root's
    sphere against the plane does not change with the base's qd[0..2]; the base's own sphere's does"""
    m, q, qd, _ = P.mixed_box(1, 4)
    m.sphere_no_plane = 0; m.npairs = 0
    a = pair_ref.ca(m, q[0], qd[0])
    qd2 = qd.copy(); qd2[0, :3] += (0.7, -1.3, 0.4)
    b = pair_ref.ca(m, q[0], qd2[0])
    assert len(a) == 3 and np.isfinite(a).all()                             # arm-tip sphere, pendulum bob, box
    assert a[1] == b[1]
    assert a[0] != b[0] and a[2] != b[2]


def test_add_pairs_fills_the_block():
    m, _, _, _ = P.arm_pendulum(1, 0)
    assert (m.npairs, m.pair_a[0], m.pair_b[0], m.sphere_no_plane) == (1, 0, 1, 2)
    assert A.mh_artic_model.npairs.offset == A.mh_artic_model.box_len.offset + 8 * 3 * 8 * 1   # appended behind box_len: nothing before it moved


REFUSALS = [  # (what to break, the message's words)
    (lambda m: setattr(m, "npairs", 7), "npairs = 7 outside"),
    (lambda m: m.pair_b.__setitem__(0, 2), "outside the sphere list"),
    (lambda m: m.pair_a.__setitem__(0, -1), "outside the sphere list"),
    (lambda m: m.pair_b.__setitem__(0, 0), "against itself"),
    (lambda m: m.sphere_link.__setitem__(1, m.sphere_link[0]), "same link"),
    (lambda m: (setattr(m, "npairs", 2), m.pair_a.__setitem__(1, 1), m.pair_b.__setitem__(1, 0)), "are pair 0 already"),
    (lambda m: setattr(m, "sphere_no_plane", 4), "bits beyond the 2 spheres"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_create_refuses(k):
    """test 6: mh_artic_batch_create refuses a bad pair block with MH_ERR_INVALID_ARG and a message, before anything is launched or allocated
    (the checks come before the device is looked for, so this runs without one)"""
    from moby_amd import _lib
    m, q, qd, _ = P.arm_pendulum(1, 0)
    assert (m.pair_a[0], m.pair_b[0]) == (0, 1)
    brk, words = REFUSALS[k]
    brk(m)
    with pytest.raises(_lib.MobyHipError, match=words):
        A.ArticBatch(m, q, qd)


def test_cpp_adapter_add_sphere_pair(tmp_path):
    """the C++ adapter's add_sphere_pair fills the model's pair block (header-only: compiled and run without the library)"""
    import subprocess
    src = tmp_path / "pair.cpp"
    src.write_text('#include "MobyHipArticulatedBody.h"\n#include <cstdio>\n#include <cstring>\n'
                   'int main() { mh_artic_model m; std::memset(&m, 0, sizeof(m)); m.nj = 3; m.nspheres = 3;\n'
                   '  MobyHip::add_sphere_pair(m, 2, 0, true, false);\n'
                   '  std::printf("%d %d %d %d\\n", m.npairs, m.pair_a[0], m.pair_b[0], m.sphere_no_plane); std::fflush(stdout);\n'
                   '  MobyHip::add_sphere_pair(m, 1, 1);\n  return 0; }\n')
    exe = tmp_path / "pair"
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "moby_amd", "cpp"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.stdout.split() == ["1", "2", "0", "1"]
    assert r.returncode != 0                                       # a sphere against itself throws
