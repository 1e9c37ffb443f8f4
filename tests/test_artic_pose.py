"""Pose coordinates of a floating base (include/moby_hip_artic.h, MH_ARTIC_BASE_POSE) without a GPU: the pose-coordinate reference
(tests/native/artic_pose_ref.cpp: a model copy per world with trel[0] = p, Rrel[3] = R(Q), stepped by the driven reference, then the fold) --
the fold changes coordinates only, a free ball turned through a quarter turn of the middle hinge is still the rigid oracle's ball, a tumbling
body keeps |Q| = 1 and its angular momentum -- and the ctypes mirrors of the new entry points."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import io as mio
from moby_amd import scene as S
from tests import native_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "scenes")
TUMBLE = os.path.join(SCENES, "floating_tumbling_ball.xml")
TUMBLE_RIGID = os.path.join(SCENES, "dropped_tumbling_ball.xml")


class PoseRef:
    """ctypes face of tests/native/artic_pose_ref.cpp"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for f in ("artic_pose_ref_step", "artic_pose_ref_fold", "artic_pose_ref_model"):
            getattr(self.lib, f).restype = None

    @staticmethod
    def _drive(drive, B, nj):
        if drive is None:
            return None, None
        drive.check(B, nj)
        d = A.mh_artic_drive(terms=drive.terms, rows=drive.rows)
        keep = {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in drive.arrays.items() if a is not None}
        for k, a in keep.items():
            setattr(d, k, a.ctypes.data)
        return d, keep

    def step(self, model, q, qd, aux, pose, dt, nsteps, drive=None):
        """B worlds x nsteps in pose coordinates, in place (pose: (B, 7))"""
        d, keep = self._drive(drive, q.shape[0], model.nj)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self.lib.artic_pose_ref_step(ctypes.byref(model), int(q.shape[0]), ctypes.c_double(dt), int(nsteps), P(q), P(qd), P(aux), P(pose),
                                     None if d is None else ctypes.byref(d))
        del keep

    def fold(self, q, qd, pose):
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self.lib.artic_pose_ref_fold(int(q.shape[0]), int(q.shape[1]), P(q), P(qd), P(pose))

    def model(self, model, pose_row):
        out = A.mh_artic_model()
        p = np.ascontiguousarray(pose_row, dtype=np.float64)
        self.lib.artic_pose_ref_model(ctypes.byref(model), p.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out))
        return out


@pytest.fixture(scope="session")
def pose_ref():
    """the pose-coordinate reference and the driven one it steps with, one library"""
    return PoseRef(native_build.build(("artic_pose_ref.cpp", "artic_drive_ref.cpp"), "artic_pose_ref"))


def quat_of_R(R):
    """unit quaternion (w, x, y, z) of a rotation matrix (numpy, for starting poses)"""
    R = np.asarray(R, dtype=float).reshape(3, 3)
    w = np.sqrt(max(0.0, 1.0 + np.trace(R))) / 2.0
    x = np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0
    y = np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2.0
    z = np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2.0
    x = np.copysign(x, R[2, 1] - R[1, 2]); y = np.copysign(y, R[0, 2] - R[2, 0]); z = np.copysign(z, R[1, 0] - R[0, 1])
    Q = np.array([w, x, y, z])
    return Q / np.linalg.norm(Q)


def R_of_quat(Q):
    w, x, y, z = Q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def model_pose(m, B=1):
    """the pose a batch switched to pose coordinates starts from: p = trel[0], Q = the quaternion of Rrel[3]"""
    return np.tile(np.concatenate([np.array(m.trel[0]), quat_of_R(np.array(m.Rrel[3]))]), (B, 1))


def rand_rot(rng):
    Q = rng.normal(size=4)
    return R_of_quat(Q / np.linalg.norm(Q))


def random_floating(rng, nbody=None, gravity=(0.0, -9.81, 0.0)):
    """a random floating body: a base link of random pose and inertia, 0..3 revolute / prismatic links of its own (unlimited)"""
    nbody = int(rng.integers(0, 4)) if nbody is None else nbody
    def inertia():
        d = rng.uniform(0.05, 0.5, 3); R = rand_rot(rng)
        return R @ np.diag(d) @ R.T
    base = dict(R0=rand_rot(rng), x0=rng.uniform(-1.0, 1.0, 3), mass=float(rng.uniform(0.5, 3.0)), inertia=inertia())
    links = []
    for i in range(nbody):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        links.append(dict(parent=int(rng.integers(-1, i)), type=A.MH_JOINT_PRISMATIC if rng.random() < 0.25 else A.MH_JOINT_REVOLUTE,
                          R0=rand_rot(rng), x0=rng.uniform(-0.5, 0.5, 3), axis=ax, com=rng.uniform(-0.2, 0.2, 3), inertia=inertia(),
                          mass=float(rng.uniform(0.2, 1.5))))
    return A.model_from_links(links, gravity=gravity, floating_base=base)


def spatial_velocities(poses, q, qd, m, oracle):
    """the spatial velocity (angular; linear of its origin) of the base link and every link of the body (links 5..; links 0..4 are the virtual
    joints' massless links, whose frames ARE the coordinates), global frame, from the oracle's link poses and Jacobians"""
    nj = m.nj
    out = np.zeros((nj - 5, 6))
    for i in range(5, nj):
        J = oracle.artic_jacobian(m, q, i, poses[i, 9:12])
        out[i - 5, :3] = J[3:] @ qd; out[i - 5, 3:] = J[:3] @ qd
    return out


def test_the_fold_changes_coordinates_only(oracle, pose_ref):
    """test 1: random floating bodies and states; the poses (the oracle's fwd_dyn) and spatial velocities (its Jacobian) of the base link and the
    body's links before and after one fold agree to round-off, every virtual q is exactly zero after it, |Q| = 1"""
    rng = np.random.default_rng(7)
    worst_p = worst_v = 0.0
    for case in range(40):
        m = random_floating(rng)
        nj = m.nj
        q = rng.uniform(-2.5, 2.5, (1, nj)); qd = rng.uniform(-3.0, 3.0, (1, nj))
        pose = model_pose(m)
        if case % 2:                                          # a pose that is not the model's
            pose[0, :3] += rng.uniform(-1, 1, 3); Q = rng.normal(size=4); pose[0, 3:] = Q / np.linalg.norm(Q)
        mb = pose_ref.model(m, pose[0])
        before = oracle.artic_fwd_dyn(mb, q[0], qd[0])["poses"][5:]
        vb = spatial_velocities(oracle.artic_fwd_dyn(mb, q[0], qd[0])["poses"], q[0], qd[0], mb, oracle)
        q1, qd1, pose1 = q.copy(), qd.copy(), pose.copy()
        pose_ref.fold(q1, qd1, pose1)
        assert (q1[0, :6] == 0.0).all() and np.array_equal(q1[0, 6:], q[0, 6:]) and np.array_equal(qd1[0, :3], qd[0, :3]) and np.array_equal(qd1[0, 6:], qd[0, 6:])
        assert abs(np.linalg.norm(pose1[0, 3:]) - 1.0) < 1e-15
        ma = pose_ref.model(m, pose1[0])
        after = oracle.artic_fwd_dyn(ma, q1[0], qd1[0])["poses"][5:]
        va = spatial_velocities(oracle.artic_fwd_dyn(ma, q1[0], qd1[0])["poses"], q1[0], qd1[0], ma, oracle)
        sp = max(1.0, np.abs(before).max()); sv = max(1.0, np.abs(vb).max())
        worst_p = max(worst_p, np.abs(after - before).max() / sp)
        worst_v = max(worst_v, np.abs(va - vb).max() / sv)
    print("fold: worst relative change of link poses %.2e, of link velocities %.2e" % (worst_p, worst_v))
    assert worst_p < 1e-14 and worst_v < 1e-14, (worst_p, worst_v)


def rigid_R(st, b):
    """the rigid ball's orientation (the state stores its quaternion x y z w)"""
    return S.quat_to_R(st[13 * b + 3:13 * b + 7])


UNTURNED = os.path.join(SCENES, "floating_spinning_ball_unturned.xml")
DROPPED = os.path.join(SCENES, "dropped_spinning_ball.xml")


def run_ball(oracle, pose_ref, scene, rigid, dt, steps):
    m, _, _, q0, qd0, _ = A.load_xml(scene)
    sc, st0, ids, _ = mio.load_xml(rigid)
    assert abs(qd0[4] - 10.0) < 1e-12 and abs(qd0[3]) < 1e-12 and abs(qd0[5]) < 1e-12     # the spin is the middle hinge's rate
    q = q0.reshape(1, -1).copy(); qd = qd0.reshape(1, -1).copy(); aux = S.new_aux(1); pose = model_pose(m)
    pose_ref.fold(q, qd, pose)
    st = st0.copy().reshape(-1); auxw = S.new_aux(1)
    traj = oracle.world_step(sc, st, auxw, dt, steps)["traj"]
    b = ids.index("ball")
    ya = np.zeros(steps)
    for k in range(steps):
        pose_ref.step(m, q, qd, aux, pose, dt, 1)
        ya[k] = pose[0, 1]
    assert (q[0] == 0.0).all() and abs(np.linalg.norm(pose[0, 3:]) - 1.0) < 1e-15
    R = R_of_quat(pose[0, 3:]) @ np.array(m.Rrel[3]).reshape(3, 3).T       # the rigid ball's body frame is the model frame at rest
    assert aux["status"][0] == 0 and auxw["status"][0] == 0 and aux["lcp_solves"][0] == auxw["lcp_solves"][0] >= 3 and aux["mini_steps"][0] == auxw["mini_steps"][0] > steps
    return dict(h=np.abs(ya - traj[:, b, 1]).max(), vy=abs(qd[0, 1] - st[13 * b + 8]), w=np.abs(R_of_quat(pose[0, 3:]) @ qd[0, 3:6] - st[13 * b + 10:13 * b + 13]).max(),
                R_rigid=np.abs(R - rigid_R(st, b)).max(), R=R, t=dt * steps, ya=ya)


def rot(axis, a):
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]], dtype=float)
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


@pytest.mark.parametrize("dt,steps,tol,tol_R", [(1e-3, 3000, 1e-12, 3e-4), (0.025, 120, 1e-6, 0.2)])
def test_the_free_ball_across_a_quarter_turn_of_the_middle_hinge(oracle, pose_ref, dt, steps, tol, tol_R):
    """test 2: tests/scenes/floating_spinning_ball_unturned.xml -- the ball of floating_spinning_ball.xml without its quarter turn, so that the
    spin of 10 rad/s about the vertical is the MIDDLE hinge's rate (in angle coordinates joint 4 passes pi/2 after 0.157 s) -- in pose coordinates
    against its rigid twin dropped_spinning_ball.xml (oracle/world.hpp): height, vertical velocity and world-frame spin to the tolerances of
    test_a_floating_base_of_one_link_is_the_free_rigid_body (measured: 0 at both step sizes), status 0, equal LCP and mini-step counts, 30 rad of
    spin.  Orientation: against the exact rotation exp(10 t e_y) to 1e-11 (measured 2.8e-15 / 2.4e-15); against the rigid oracle's quaternion to
    3e-4 at dt = 1e-3 and 0.2 at 0.025 (measured 2.47e-4 / 0.151) -- that difference is the rigid stepper's own orientation update, second order
    in dt per step (it scales as dt^2: 625 x 2.47e-4 = 0.154), which the fold's exact rotation does not share."""
    r = run_ball(oracle, pose_ref, UNTURNED, DROPPED, dt, steps)
    assert r["h"] < tol and r["vy"] < 10 * tol and r["w"] < 1e-12
    assert r["R_rigid"] < tol_R, r["R_rigid"]
    assert np.abs(r["R"] - rot((0.0, 1.0, 0.0), 10.0 * r["t"])).max() < 1e-11
    assert r["ya"].min() > 1.0 - 1e-9


def test_the_free_ball_tumbling_about_a_horizontal_middle_hinge(oracle, pose_ref):
    """test 2, the horizontal variant: tests/scenes/floating_tumbling_ball.xml (the middle hinge horizontal, the spin about it) against
    dropped_tumbling_ball.xml.  Here the two steppers' conservative advancement differ by construction -- the rigid CCD::calc_max_dist adds
    |w x n| rmax for the spin (CCD.cpp:585-609), the articulated one 2 rmax |qd5| (CCD.cpp:545-583) -- so the bounces land 1e-7 apart IN ANGLE
    COORDINATES TOO (measured there: height 2.99e-7).  Pose coordinates, dt = 1e-3, 3000 steps: height 2.99e-7, vertical velocity 9.3e-7, spin
    3.3e-14 (asserted at 1e-6, 1e-5, 1e-12); status 0, equal counts; orientation against exp(10 t e_z) to 1e-11 (measured 3.1e-15)."""
    r = run_ball(oracle, pose_ref, TUMBLE, TUMBLE_RIGID, 1e-3, 3000)
    assert r["h"] < 1e-6 and r["vy"] < 1e-5 and r["w"] < 1e-12
    assert np.abs(r["R"] - rot((0.0, 0.0, 1.0), 10.0 * r["t"])).max() < 1e-11


def tumbling_body():
    """one free link of inertia diag(1, 2, 3) about its COM, mass 2, g = 0, no geometry"""
    return A.model_from_links([], gravity=(0.0, 0.0, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 0.0, 0.0), mass=2.0, inertia=np.diag([1.0, 2.0, 3.0])))


def test_torque_free_tumbling_keeps_the_quaternion_and_the_angular_momentum(pose_ref):
    """test 3: spun about its intermediate axis with a small perturbation (the Dzhanibekov flip), 1e4 steps of 1e-3: the body turns over
    about every axis many times.  |Q| stays 1 to 1e-14, the world angular momentum R(Q) I w to 1e-2 relative (measured 5.5e-3, and 2.7e-3 at
    dt = 5e-4: first order in dt -- the semi-implicit step does not conserve it exactly), status 0.
    Recorded, not asserted: the same run in angle coordinates (oracle_artic_step) keeps status 0, but joint 4 comes within 0.054 rad of pi/2
    and the world angular momentum ends up 287 % away from its start."""
    m = tumbling_body()
    I = np.diag([1.0, 2.0, 3.0])
    q = np.zeros((1, 6)); qd = np.array([[0.0, 0.0, 0.0, 0.02, 2.0, 0.02]]); aux = S.new_aux(1); pose = model_pose(m)
    L0 = I @ qd[0, 3:]
    worst_n = worst_L = 0.0
    Qs = []
    for k in range(100):
        pose_ref.step(m, q, qd, aux, pose, 1e-3, 100)
        worst_n = max(worst_n, abs(np.linalg.norm(pose[0, 3:]) - 1.0))
        L = R_of_quat(pose[0, 3:]) @ (I @ qd[0, 3:])
        worst_L = max(worst_L, np.abs(L - L0).max() / np.linalg.norm(L0))
        Qs.append(pose[0, 3:].copy())
    assert aux["status"][0] == 0 and aux["steps"][0] == 10000
    assert worst_n <= 1e-14, worst_n
    assert worst_L < 1e-2, worst_L
    # it did tumble: the body's y axis points both ways along the world's over the run
    ys = np.array([R_of_quat(Q)[:, 1] @ np.array([0.0, 1.0, 0.0]) for Q in Qs])
    assert ys.max() > 0.9 and ys.min() < -0.9


def test_ctypes_mirrors_of_the_pose_entry_points(tmp_path):
    """test 4 (host side): the constants against the header, the ctypes table against the exported symbols, the C++ adapter's pose calls
    compile with plain g++"""
    src = tmp_path / "pose.c"
    src.write_text('#include <stdio.h>\n#include "moby_hip_artic.h"\n'
                   'int main(void) { printf("%d %d\\n", MH_ARTIC_BASE_ANGLES, MH_ARTIC_BASE_POSE); return 0; }\n')
    exe = str(tmp_path / "pose")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    assert [int(x) for x in subprocess.check_output([exe]).split()] == [A.MH_ARTIC_BASE_ANGLES, A.MH_ARTIC_BASE_POSE]
    lib = _lib.load()
    for name in ("mh_artic_batch_set_base_coords", "mh_artic_batch_base_coords", "mh_artic_batch_base_pose", "mh_artic_batch_set_base_pose",
                 "mh_artic_batch_base_pose_dev"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS, name
    # every entry point refuses a NULL batch without touching a device
    assert lib.mh_artic_batch_set_base_coords(None, A.MH_ARTIC_BASE_POSE) != 0
    assert lib.mh_artic_batch_base_pose(None, None) != 0 and lib.mh_artic_batch_set_base_pose(None, None) != 0
    assert lib.mh_artic_batch_base_pose_dev(None, None, None) != 0
    c = ctypes.c_int(-1)
    assert lib.mh_artic_batch_base_coords(None, ctypes.byref(c)) != 0
    cpp = tmp_path / "pose.cpp"
    cpp.write_text('#include "MobyHipArticulatedBody.h"\n'
                   'void f(MobyHip::BatchedArticulatedBody& r, double* pose) {\n'
                   '  r.set_base_coords(MH_ARTIC_BASE_POSE); r.base_pose(pose); pose[3] = 1.0; r.set_base_pose(pose); r.step(1e-3, 10); (void)r.base_coords(); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "moby_amd", "cpp"), str(cpp)])


def test_scenes_differ_from_the_untumbled_ones_only_in_the_spin():
    """the two new scenes are the ball of floating_spinning_ball.xml / dropped_spinning_ball.xml with the middle hinge horizontal and the spin
    about it"""
    m, _, _, q0, qd0, dt = A.load_xml(TUMBLE)
    assert m.nj == 6 and m.floating_base == 1 and m.nspheres == 1 and dt == 0.025
    R = np.array(m.Rrel[3]).reshape(3, 3)
    assert np.allclose(R[:, 1], [0.0, 0.0, 1.0], atol=1e-15)                  # the link's y axis (the middle hinge) is the world's horizontal z
    sc, st0, ids, _ = mio.load_xml(TUMBLE_RIGID)
    b = ids.index("ball")
    st0 = st0.reshape(-1)
    assert np.allclose(st0[13 * b + 10:13 * b + 13], [0.0, 0.0, 10.0]) and np.allclose(rigid_R(st0, b), np.eye(3))
    m, _, _, q0, qd0, _ = A.load_xml(UNTURNED)
    assert np.array_equal(np.array(m.Rrel[3]).reshape(3, 3), np.eye(3)) and qd0[4] == 10.0
