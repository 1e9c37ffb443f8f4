"""Box primitives on links against the plane (include/moby_hip_artic.h, mh_artic_model.nboxes) without a GPU: the readers (Moby XML with a floating
base, welded legs and a URDF box), the box reference (tests/native/artic_box_ref.cpp) pinned to the oracle and the drive / pose references on
sphere-only models, and the free box held to the reference's own recording regress/sitting-box.dat."""
import os
import subprocess

import numpy as np
import pytest

from moby_amd import artic as A
from moby_amd import io as mio
from moby_amd import scene as S
from tests.artic_box_ref import build_box_ref
from tests.test_artic_drive import FIELDS, drive_ref, random_drive  # noqa: F401  (drive_ref: the session fixture)
from tests.test_artic_pose import pose_ref  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "scenes")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def box_ref():
    return build_box_ref()


def Ry(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def Rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def boxes_of(m):
    return [(m.box_link[k], np.array(m.box_center[k]), np.array(m.box_R[k]).reshape(3, 3), np.array(m.box_len[k])) for k in range(m.nboxes)]


def test_reader_floating_one_box():
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(SCENES, "floating_sitting_box.xml"))
    assert (m.nj, m.nspheres, m.nboxes, dt) == (6, 0, 1, 1e-3)
    (link, c, R, L), = boxes_of(m)
    assert link == 5 and np.array_equal(c, np.zeros(3)) and np.array_equal(R, np.eye(3)) and np.array_equal(L, np.ones(3))
    assert list(m.trel[0]) == [0.0, 0.50001, 0.0] and m.cp_nk == 8 and m.cp_mu_coulomb == 0.0


def test_reader_table_with_welded_box_legs():
    """the top's posed collision box and two legs welded on by FixedJoints, all carried into the base link's frame (its COM)"""
    m, _, _, _, _, _ = A.load_xml(os.path.join(SCENES, "floating_box_table.xml"))
    assert (m.nj, m.nboxes) == (6, 3)
    mt, ml = 1.0 * 0.1 * 0.6, 2.0 * 0.1 * 0.4 * 0.1
    com = (mt * np.array([0.0, 0.5, 0.0]) + ml * np.array([0.4, 0.28, 0.2]) + ml * np.array([-0.4, 0.28, -0.2])) / (mt + 2 * ml)
    Rt = Ry(0.3)
    want = [(np.array([0.0, 0.5, 0.0]) + Rt @ np.array([0.0, 0.02, 0.0]), Rt @ Rz(0.1), (1.0, 0.1, 0.6)),
            (np.array([0.4, 0.28, 0.2]), np.eye(3), (0.1, 0.4, 0.1)),
            (np.array([-0.4, 0.28, -0.2]), Ry(0.5), (0.1, 0.4, 0.1))]
    for (link, c, R, L), (cw, Rw, Lw) in zip(boxes_of(m), want):
        assert link == 5
        np.testing.assert_allclose(c, Rt.T @ (cw - com), rtol=0, atol=1e-15)
        np.testing.assert_allclose(R, Rt.T @ Rw, rtol=0, atol=1e-15)
        assert np.array_equal(L, np.array(Lw))


def test_reader_urdf_box_foot():
    m, links, _, _, _, _ = A.load_xml(os.path.join(SCENES, "arm_with_box_foot_urdf.xml"))
    assert (m.nj, m.nboxes, links) == (2, 1, ["upper", "foot"])
    (link, c, R, L), = boxes_of(m)
    assert link == 1
    np.testing.assert_allclose(c, [0.01, 0.0, 0.4], rtol=0, atol=1e-15)
    np.testing.assert_allclose(R, Rz(0.2), rtol=0, atol=1e-15)
    assert np.array_equal(L, [0.2, 0.1, 0.05])
    assert list(m.plane_o) == [0.0, -0.75, 0.0]


def test_reader_fixed_base_arm_with_box_links():
    """Box geometry on a moving link of a fixed-base Moby-XML arm: the end link's own posed box (the link is a composite: a pad is welded onto it,
    so its COM moved) and the pad's box, both carried into the end link's model frame (origin at its joint, 0 -1.0 0)"""
    m, links, _, _, _, _ = A.load_xml(os.path.join(SCENES, "arm_with_box_link.xml"))
    assert (m.nj, m.nspheres, m.nboxes, links) == (3, 1, 2, ["l1", "l2", "l3"])
    (l0, c0, R0, L0), (l1, c1, R1, L1) = boxes_of(m)
    assert l0 == l1 == 2
    np.testing.assert_allclose(c0, [0.0, -0.15, 0.1], rtol=0, atol=1e-15)          # the welded pad at (0, -1.15, 0.1)
    assert np.array_equal(R0, np.eye(3)) and np.array_equal(L0, [0.08, 0.02, 0.08])
    np.testing.assert_allclose(c1, [0.02, -0.15, 0.0], rtol=0, atol=1e-15)         # l3 at (0, -1.1, 0) + the primitive's (0.02, -0.05, 0)
    np.testing.assert_allclose(R1, Ry(0.3), rtol=0, atol=1e-15)
    assert np.array_equal(L1, [0.2, 0.06, 0.1])


def test_add_boxes_shares_the_plane():
    m = A.model_from_links([], gravity=(0.0, -9.81, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 1.0, 0.0), mass=1.0, inertia=np.eye(3)))
    A.add_spheres(m, [(5, (0.0, 0.0, 0.0), 0.1)], plane_normal=(0.0, 1.0, 0.0))
    A.add_boxes(m, [(5, (0.0, 0.0, 0.0), np.eye(3), (0.1, 0.2, 0.3))], plane_normal=(0.0, 1.0, 0.0))
    assert (m.nspheres, m.nboxes) == (1, 1)
    with pytest.raises(ValueError):
        A.add_boxes(m, [(5, (0.0, 0.0, 0.0), np.eye(3), (0.1, 0.2, 0.3))], plane_normal=(0.0, 0.0, 1.0))


PIN_SCENES = {  # sphere-only scenes: name -> (file, worlds, steps, stabiliser iterations)
    "arm_on_table": ("arm_on_table.xml", 3, 150, 10),
    "floating_welded_pair": ("floating_welded_pair.xml", 3, 80, 10),
    "floating_spinning_ball": ("floating_spinning_ball.xml", 3, 60, 10),
}


def pin_state(name):
    f, B, n, iters = PIN_SCENES[name]
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(SCENES, f))
    m.cstab_max_iterations = iters
    rng = np.random.default_rng(len(name))
    q = np.tile(q0, (B, 1)) + rng.uniform(-0.05, 0.05, (B, m.nj)); qd = np.tile(qd0, (B, 1)) + rng.uniform(-0.5, 0.5, (B, m.nj))
    return m, q, qd, dt, n


def assert_same(a, b):
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x, y), "max diff %.3e" % np.max(np.abs(x - y))
    for f in FIELDS:
        assert np.array_equal(a[2][f], b[2][f]), f


@pytest.mark.parametrize("name", list(PIN_SCENES))
def test_box_reference_without_boxes_is_the_oracle(oracle, box_ref, name):
    """restatement pin: nboxes = 0, stabiliser on -- the box reference steps exactly as oracle_artic_step"""
    m, q, qd, dt, n = pin_state(name)
    B = q.shape[0]
    ref = [q.copy(), qd.copy(), S.new_aux(B)]
    box_ref.step(m, ref[0], ref[1], ref[2], dt, n)
    o = [q.copy(), qd.copy(), S.new_aux(B)]
    oracle.artic_step(m, o[0], o[1], o[2], dt, n)
    assert_same(ref, o)
    assert (o[2]["lcp_solves"] > 0).any()


@pytest.mark.parametrize("name", list(PIN_SCENES))
def test_box_reference_without_boxes_is_the_drive_and_pose_references(drive_ref, pose_ref, box_ref, name):
    """restatement pin: with a drive it equals artic_drive_ref_step; in pose coordinates (floating bases) artic_pose_ref_step"""
    m, q, qd, dt, n = pin_state(name)
    B, nj = q.shape
    d = random_drive(np.random.default_rng(5), B, nj, rows=n, tau=2.0)
    a = [q.copy(), qd.copy(), S.new_aux(B)]; b = [q.copy(), qd.copy(), S.new_aux(B)]
    box_ref.step(m, a[0], a[1], a[2], dt, n, drive=d)
    drive_ref.step(m, b[0], b[1], b[2], dt, n, d)
    assert_same(a, b)
    if m.floating_base:
        from tests.test_artic_pose import model_pose
        P0 = model_pose(m, B)
        a = [np.zeros_like(q), qd.copy(), S.new_aux(B)]; b = [np.zeros_like(q), qd.copy(), S.new_aux(B)]
        Pa, Pb = P0.copy(), P0.copy()
        box_ref.step(m, a[0], a[1], a[2], dt, n, pose=Pa, drive=d)
        pose_ref.step(m, b[0], b[1], b[2], Pb, dt, n, d)
        assert_same(a, b)
        assert np.array_equal(Pa, Pb)


def test_floating_box_matches_the_sitting_box_recording(box_ref):
    """regress/sitting-box.dat (the reference's free unit cube released at y = 0.50001) against the same cube as a floating-base articulated body
    stepped by the box reference, at test_oracle_box.py's tolerances (row 1: 1.1e-5, the recording closes the gap one step earlier; then the
    file's 6-digit resolution), over the whole recording (10 000 steps)."""
    g = np.load(os.path.join(GOLD, "sitting_box_dat.npz"))
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(SCENES, "floating_sitting_box.xml"))
    q = q0[None].copy(); qd = qd0[None].copy(); aux = S.new_aux(1)
    rows = [(k, r) for r, k in zip(g["rows"], g["row_index"]) if k > 0]
    done = 0
    for k, r in rows:
        box_ref.step(m, q, qd, aux, dt, k - done); done = k
        p = np.array(m.trel[0]) + q[0, :3]
        np.testing.assert_allclose(p, r[1:4], rtol=0, atol=(1.1e-5 if k == 1 else 1e-6), err_msg="row %d" % k)
        assert np.max(np.abs(q[0, 3:6])) < 1e-6
    assert aux["status"][0] == 0 and aux["lcp_solves"][0] > 0


def test_sliding_box_equals_the_rigid_oracles_free_box(oracle, box_ref):
    """A unit cube dropped flat with a lateral velocity, mu = 0.5 (Drumwright-Shell), slides to rest: the floating-base box against the rigid
    oracle's free box (oracle.world_step) after every step.  Post-impact body velocities are unique (the QP minimises kinetic energy) even where the
    vertex impulses are not; what separates the two is the conservative advancement: the articulated calc_max_dist bounds the approach
    differently from the rigid one, so the two split the landing step at different times.  Measured over 800 steps: height 9.6e-9, linear
    velocity 1.3e-7, angular velocity 2.7e-14; the bounds below are about four times that."""
    sc, st0, _, _ = mio.load_xml(os.path.join(SCENES, "sliding_box.xml"))
    st = st0[0].copy(); aux = S.new_aux(1)
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(SCENES, "floating_sliding_box.xml"))
    assert m.nboxes == 1 and m.cp_mu_coulomb == 0.5
    q = q0[None].copy(); qd = qd0[None].copy(); ax = S.new_aux(1)
    for k in range(800):
        oracle.world_step(sc, st, aux, dt, 1, want_traj=False)
        box_ref.step(m, q, qd, ax, dt, 1)
        p = np.array(m.trel[0]) + q[0, :3]
        assert abs(p[1] - st[1]) < 4e-8, "step %d: height" % k
        assert np.abs(qd[0, :3] - st[7:10]).max() < 5e-7, "step %d: velocity" % k
        assert np.abs(qd[0, 3:6] - st[10:13]).max() < 1e-13, "step %d: angular velocity" % k
    assert np.abs(qd[0]).max() < 1e-12 and np.abs(p - st[:3]).max() < 4e-8       # at rest, where the rigid box rests
    assert aux["status"][0] == 0 and ax["status"][0] == 0 and ax["lcp_solves"][0] > 0


def R_of_quat(Q):
    w, x, y, z = Q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def test_tumbling_die_never_penetrates_in_pose_coordinates(box_ref):
    """test/TestDie.cpp's property for the articulated die: a unit cube thrown tumbling onto the plane (mu = 0.5, epsilon = 0.3, stabiliser on),
    stepped in pose coordinates; its lowest vertex stays above -1e-6 after every step, and its motion dies down"""
    m = A.model_from_links([], gravity=(0.0, -9.81, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 1.2, 0.0), mass=1.0, inertia=np.eye(3) / 6.0))
    A.add_boxes(m, [(5, (0.0, 0.0, 0.0), np.eye(3), (1.0, 1.0, 1.0))], plane_normal=(0.0, 1.0, 0.0), epsilon=0.3, mu_coulomb=0.5)
    m.cstab_max_iterations = 10
    from tests.test_artic_pose import model_pose, quat_of_R
    P = model_pose(m)
    P[0, 3:] = quat_of_R(Ry(0.4) @ Rz(0.7))
    q = np.zeros((1, 6)); qd = np.array([[0.8, 0.0, -0.3, 4.0, 2.0, -3.0]]); aux = S.new_aux(1)
    corners = np.array([[sx, sy, sz] for sx in (0.5, -0.5) for sy in (0.5, -0.5) for sz in (0.5, -0.5)])
    low = []
    for k in range(5000):
        box_ref.step(m, q, qd, aux, 1e-3, 1, pose=P)
        assert aux["status"][0] == 0, "step %d: status %d" % (k, aux["status"][0])
        low.append((P[0, :3] + corners @ R_of_quat(P[0, 3:]).T)[:, 1].min())
    assert min(low) > -1e-6
    assert min(low[:400]) < 1e-3                                  # it did land
    assert np.abs(qd[0]).max() < 2e-2                             # and its motion has died down
    assert aux["stab_iters"][0] >= 0 and aux["lcp_solves"][0] > 0


def test_over_capacity_ends_unsupported_at_the_first_impact(box_ref):
    """capacity under the no-slip model: NC + NL <= MH_NOSLIP_MAX (16).  Five flat box feet land together: 20 vertex contacts, so the first
    impacting mini-step leaves the world MH_WORLD_UNSUPPORTED: that step ends there (stabilised and counted, as Artic::step does) and no later
    step runs; four feet (16 contacts) land and rest"""
    def body(nfeet):
        m = A.model_from_links([], gravity=(0.0, -9.81, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 0.06, 0.0), mass=5.0, inertia=np.eye(3)))
        xz = ((-0.4, -0.4), (0.4, -0.4), (-0.4, 0.4), (0.4, 0.4), (0.0, 0.0))[:nfeet]
        A.add_boxes(m, [(5, (x, -0.05, z), np.eye(3), (0.1, 0.02, 0.1)) for x, z in xz], plane_normal=(0.0, 1.0, 0.0), mu_coulomb=100.0)
        return m
    # the feet's soles start 0.06 - 0.05 - 0.01 = 0 above the plane: falling from rest they impact in the first steps
    m5 = body(5)
    q = np.zeros((1, 6)); qd = np.zeros((1, 6)); aux = S.new_aux(1)
    for k in range(50):
        box_ref.step(m5, q, qd, aux, 1e-3, 1)
        if aux["status"][0]:
            break
    assert aux["status"][0] == S.MH_WORLD_UNSUPPORTED and aux["steps"][0] == k + 1 and k < 5
    q2 = q.copy(); aux2 = aux.copy()
    box_ref.step(m5, q2, qd.copy(), aux2, 1e-3, 10)                   # frozen: nothing moves any more
    assert np.array_equal(q2, q) and aux2["steps"][0] == aux["steps"][0]
    m4 = body(4)
    q = np.zeros((1, 6)); qd = np.zeros((1, 6)); aux = S.new_aux(1)
    box_ref.step(m4, q, qd, aux, 1e-3, 300)
    assert aux["status"][0] == 0 and aux["steps"][0] == 300 and aux["lcp_solves"][0] > 0 and aux["lcp_rows"][0] >= 16


def test_cpp_adapter_add_link_box(tmp_path):
    """the C++ adapter's box counterpart of add_link_sphere fills the model's box block (header-only: compiled and run without the library)"""
    src = tmp_path / "box.cpp"
    src.write_text('#include "MobyHipArticulatedBody.h"\n#include <cstdio>\n#include <cstring>\n'
                   'int main() { mh_artic_model m; std::memset(&m, 0, sizeof(m)); m.nj = 2;\n'
                   '  const double c[3] = {0.1, -0.2, 0.3}, R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, L[3] = {0.2, 0.1, 0.05};\n'
                   '  MobyHip::add_link_box(m, 1, c, R, L);\n'
                   '  std::printf("%d %d %g %g %g %g %g\\n", m.nboxes, m.box_link[0], m.box_center[0][1], m.box_R[0][1], m.box_R[0][3], m.box_len[0][2], m.box_len[0][0]); std::fflush(stdout);\n'
                   '  for (int i = 0; i < 8; i++) MobyHip::add_link_box(m, 0, c, R, L);\n  return 0; }\n')
    exe = tmp_path / "box"
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "moby_amd", "cpp"), str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.stdout.split() == ["1", "1", "-0.2", "-1", "1", "0.05", "0.2"]
    assert r.returncode != 0                                       # the ninth box throws (MH_ARTIC_MAX_BOXES = 8)
