"""Pose coordinates on the GPU (include/moby_hip_artic.h: MH_ARTIC_BASE_POSE, mh_artic_batch_set_base_coords / base_pose / set_base_pose /
base_pose_dev): every pose kernel bit for bit against the pose-coordinate reference (tests/native/artic_pose_ref.cpp) -- q, qd, the poses and
the aux record -- the seams with each world's pose against the oracle with each world's model copy, a world that fails, the switch from angles,
the refusals, and the C++ adapter."""
import os
import subprocess

import numpy as np
import pytest

from moby_amd import artic as A
from moby_amd import scene as S
from tests.test_artic_drive import FIELDS
from tests.test_artic_pose import UNTURNED, pose_ref  # noqa: F401  (pose_ref: the session fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "tests", "scenes")
PAIR = os.path.join(SCENES, "floating_hinged_pair.xml")
WELDED = os.path.join(SCENES, "floating_welded_pair.xml")


def same(got, ref, B):
    (q_g, qd_g, P_g, aux_g), (q_r, qd_r, P_r, aux_r) = got, ref
    assert np.array_equal(q_g, q_r), "max |dq| = %.3e" % np.nanmax(np.abs(q_g - q_r))
    assert np.array_equal(qd_g, qd_r), "max |dqd| = %.3e" % np.nanmax(np.abs(qd_g - qd_r))
    assert np.array_equal(P_g, P_r), "max |dP| = %.3e" % np.nanmax(np.abs(P_g - P_r))
    for f in FIELDS:
        assert np.array_equal(aux_g[f], aux_r[f]), f
    for w in range(B):
        k = int(aux_r["vns_size"][w]); assert np.array_equal(aux_g["vns"][w, :k], aux_r["vns"][w, :k])
        k = int(aux_r["zlast_size"][w]); assert np.array_equal(aux_g["zlast"][w, :k], aux_r["zlast"][w, :k])


def perturbed(path, B, seed, iters=None, mu=None):
    m, _, _, q0, qd0, dt = A.load_xml(path)
    if iters is not None: m.cstab_max_iterations = iters
    if mu is not None: m.cp_mu_coulomb = mu
    rng = np.random.default_rng(seed)
    nj = m.nj
    q = np.tile(q0, (B, 1)); qd = np.tile(qd0, (B, 1))
    q[1:, :3] += rng.uniform(-0.05, 0.05, (B - 1, 3)); q[1:, 3:6] += rng.uniform(-0.3, 0.3, (B - 1, 3))
    qd[1:] += rng.uniform(-0.5, 0.5, (B - 1, nj)); qd[1:, 4] += rng.uniform(8.0, 14.0, B - 1)      # a spin through the middle hinge's quarter turn
    return m, q, qd, dt


def tumblers(B, seed, stab=False):
    """the torque-free body of tests/test_artic_pose.py with a limited hinged tail, spun fast about random axes: every world's rotation passes a
    quarter turn of the middle hinge in a few hundred steps"""
    rng = np.random.default_rng(seed)
    tail = dict(parent=-1, type=A.MH_JOINT_REVOLUTE, R0=np.eye(3), x0=(0.3, 0.0, 0.0), axis=(0.0, 0.0, 1.0), com=(0.2, 0.0, 0.0),
                inertia=np.eye(3) * 0.01, mass=0.3, lo=-0.4, hi=0.4, restitution=0.3)
    m = A.model_from_links([tail], gravity=(0.0, -9.81, 0.0), floating_base=dict(R0=np.eye(3), x0=(0.0, 1.0, 0.0), mass=2.0, inertia=np.diag([1.0, 2.0, 3.0])))
    if stab:
        m.cstab_max_iterations = 10
    q = np.zeros((B, 7)); qd = np.zeros((B, 7))
    q[:, 3:6] = rng.uniform(-0.5, 0.5, (B, 3)); q[:, 6] = rng.uniform(-0.3, 0.3, B)
    qd[:, :3] = rng.uniform(-1, 1, (B, 3)); qd[:, 3:6] = rng.uniform(-6, 6, (B, 3)); qd[:, 4] += rng.choice([-1.0, 1.0], B) * 12.0
    qd[:, 6] = rng.uniform(-3, 3, B)
    return m, q, qd, 1e-3


def virtual_drive(rng, B, nj, rows):
    """tau_ff on the six virtual columns (a force at the COM, a torque about the base's axes), a PD servo on the body's joints"""
    sh = (rows, B, nj)
    on = np.zeros(nj); on[6:] = 1.0
    ff = rng.uniform(-2.0, 2.0, sh); ff[..., 6:] = 0.0
    return A.Drive(kp=rng.uniform(0.0, 5.0, (B, nj)) * on, kv=rng.uniform(0.0, 0.5, (B, nj)) * on,
                   q_des=rng.uniform(-0.3, 0.3, sh), qd_des=rng.uniform(-0.5, 0.5, sh), tau_ff=ff)


CASES = {  # name -> (builder, steps per launch)
    "tumble_w4": (lambda: tumblers(64, 1), 150),
    "tumble_stab": (lambda: tumblers(16, 2, stab=True), 100),
    "ball": (lambda: perturbed(UNTURNED, 6, 3)[:3] + (1e-3,), 150),
    "pair_noslip_stab": (lambda: perturbed(PAIR, 3, 79, iters=10), 10),
    "pair_ds": (lambda: perturbed(PAIR, 4, 77, iters=0, mu=0.5), 60),
    "welded": (lambda: perturbed(WELDED, 4, 44), 40),
}


def run_pose(pose_ref, name, alg, driven):
    build, n = CASES[name]
    m, q0, qd0, dt = build()
    m.algorithm = alg
    B, nj = q0.shape
    ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords="pose")
    assert ab.base_coords == "pose"
    P = ab.base_pose()
    ab.upload(q0, qd0, S.new_aux(B))                      # virtual q relative to the current pose
    ref = [q0.copy(), qd0.copy(), P.copy(), S.new_aux(B)]
    rng = np.random.default_rng(len(name) + 10 * alg)
    for launch in range(2):
        d = virtual_drive(rng, B, nj, rows=1 if launch == 0 else n) if driven else None
        ab.step(dt, n, drive=d)
        pose_ref.step(m, ref[0], ref[1], ref[3], ref[2], dt, n, d)
        q_g, qd_g, aux_g = ab.download()
        same((q_g, qd_g, ab.base_pose(), aux_g), (ref[0], ref[1], ref[2], ref[3]), B)
    ab.close()
    return m, ref


@pytest.mark.parametrize("driven", [False, True])
@pytest.mark.parametrize("alg", [A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB])
@pytest.mark.parametrize("name", list(CASES))
def test_pose_kernels_match_the_reference(pose_ref, name, alg, driven):
    """test 5: k_artic_step_w4_pose[_drive] (64 and 16 tumbling bodies with a limited tail), k_artic_step_stab_pose[_drive], the contact kernels
    k_artic_step_contacts[_stab]_pose[_drive] (the ball spun through the middle hinge, the hinged pair under no-slip + stabiliser and under
    Drumwright-Shell, the welded pair); CRB and FSAB; undriven and driven (tau_ff on the virtual columns, PD on the body's joints, a held row
    then a row per step): q, qd, the poses and every aux field bit for bit over two launches"""
    m, (q, qd, P, aux) = run_pose(pose_ref, name, alg, driven)
    steps = aux["steps"]
    done = (aux["status"] & S.MH_WORLD_LCP_FAILED) == 0
    assert (q[done, :6] == 0.0).all()
    assert (np.abs(np.linalg.norm(P[:, 3:], axis=1) - 1.0) < 1e-14).all()
    if name.startswith("tumble"):
        # the middle hinge's quarter turn: every world's base turned by more than pi/2 about some axis
        ang = [2 * np.arccos(min(1.0, abs(P[b, 3]))) for b in range(q.shape[0])]
        assert done.all() and min(ang) > 0.2 and (steps > 0).all()
    # (tumble_stab: the stabilising kernel runs, but its limit rows never iterate on a floating body -- update_q's slacks are joint 0's, CStab:117,
    #  and a virtual slider has no limits; pair_noslip_stab's contact rows do)
    if name == "pair_noslip_stab":
        assert (aux["stab_iters"] > 0).any()
    if name in ("ball", "pair_noslip_stab", "pair_ds", "welded"):
        assert (aux["lcp_solves"] > 0).any()


def test_seams_read_each_worlds_pose(oracle, pose_ref):
    """test 6: link_poses, jacobian and fwd_dyn (qdd, H) of a pose batch after some steps equal the oracle's with each world's model copy,
    bit for bit"""
    m, q0, qd0, dt = tumblers(8, 5)
    B, nj = q0.shape
    ab = A.ArticBatch(m, q0, qd0, base_coords="pose")
    ab.step(dt, 120)
    q, qd, _ = ab.download(); P = ab.base_pose()
    q[:, 3:6] += np.random.default_rng(3).uniform(-1, 1, (B, 3)); ab.upload(q, None, None)   # non-zero virtual q against the pose
    tau = np.random.default_rng(4).uniform(-1, 1, (B, nj))
    poses = ab.link_poses(); qdd, H = ab.fwd_dyn(tau)
    pts = np.random.default_rng(5).uniform(-1, 1, (B, 3))
    J = ab.jacobian(6, pts)
    for b in range(B):
        mb = pose_ref.model(m, P[b])
        r = oracle.artic_fwd_dyn(mb, q[b], qd[b], tau[b])
        assert np.array_equal(poses[b], r["poses"]) and np.array_equal(qdd[b], r["qdd"]) and np.array_equal(H[b], r["H"]), b
        assert np.array_equal(J[b], oracle.artic_jacobian(mb, q[b], 6, pts[b])), b
    ab.close()


def test_a_failed_world_is_neither_folded_nor_stepped(oracle, pose_ref):
    """test 7: worlds 1 and 3 carry MH_WORLD_LCP_FAILED (what a throw leaves) with non-zero virtual q: the launch leaves their q, qd, pose and
    counters alone, and their link poses are the oracle's for (P, q) -- the configuration they stopped in; worlds 0 and 2 step and fold"""
    m, q0, qd0, dt = tumblers(4, 6)
    B = 4
    ab = A.ArticBatch(m, np.zeros_like(q0), np.zeros_like(qd0), base_coords="pose")
    P0 = ab.base_pose()
    aux0 = S.new_aux(B); aux0["status"][[1, 3]] = S.MH_WORLD_LCP_FAILED; aux0["steps"][[1, 3]] = [7, 3]
    ab.upload(q0, qd0, aux0)
    ab.step(dt, 40)
    q, qd, aux = ab.download(); P = ab.base_pose()
    ref = [q0.copy(), qd0.copy(), P0.copy(), aux0.copy()]
    pose_ref.step(m, ref[0], ref[1], ref[3], ref[2], dt, 40)
    same((q, qd, P, aux), (ref[0], ref[1], ref[2], ref[3]), B)
    for w in (1, 3):
        assert np.array_equal(q[w], q0[w]) and np.array_equal(qd[w], qd0[w]) and np.array_equal(P[w], P0[w]) and aux["steps"][w] == aux0["steps"][w]
        assert (q[w, 3:6] != 0.0).all()
        assert np.array_equal(ab.link_poses()[w], oracle.artic_fwd_dyn(pose_ref.model(m, P[w]), q[w], qd[w])["poses"])
    assert (aux["steps"][[0, 2]] == 40).all() and (q[[0, 2], :6] == 0.0).all()
    ab.close()


def test_switching_an_angle_batch_keeps_its_configuration(oracle):
    """test 8: an angle batch stepped for a while, then switched to POSE: the link poses of the base and the body equal the ones before to
    round-off (1e-14), every virtual q is zero; it steps on in pose coordinates; POSE -> POSE does nothing"""
    m, q0, qd0, dt = tumblers(8, 7)
    ab = A.ArticBatch(m, q0, qd0)
    assert ab.base_coords == "angles"
    ab.step(dt, 30)
    before = ab.link_poses()[:, 5:]
    ab.set_base_coords("pose")
    after = ab.link_poses()[:, 5:]
    q, qd, aux = ab.download()
    assert np.abs(after - before).max() < 1e-14 and (q[:, :6] == 0.0).all()
    ab.set_base_coords("pose")
    assert np.array_equal(ab.download()[0], q)
    ab.step(dt, 30)
    assert (ab.download()[2]["status"] == 0).all()
    ab.close()


def test_pose_entry_points_and_refusals():
    """test 4 (device side): a fixed base, a finite limit on a virtual joint, POSE -> ANGLES, an unknown mode, a zero or NaN quaternion are
    refused; angle batches have no pose; set_base_pose normalises; base_pose_into is base_pose on the device"""
    import torch
    fixed = A.chain_model(2)
    ab = A.ArticBatch(fixed, np.zeros((2, 2)), np.zeros((2, 2)))
    with pytest.raises(RuntimeError, match="floating base"):
        ab.set_base_coords("pose")
    ab.close()
    m, q0, qd0, dt = tumblers(2, 8)
    m.hilimit[4] = 1.0
    ab = A.ArticBatch(m, q0, qd0)
    with pytest.raises(RuntimeError, match="virtual joint"):
        ab.set_base_coords("pose")
    with pytest.raises(RuntimeError, match="angle coordinates"):
        ab.base_pose()
    ab.close()
    m, q0, qd0, dt = tumblers(2, 8)
    ab = A.ArticBatch(m, q0, qd0, base_coords="pose")
    with pytest.raises(RuntimeError, match="back to angles"):
        ab.set_base_coords("angles")
    with pytest.raises(RuntimeError):
        ab.set_base_coords(7)
    P = ab.base_pose()
    for bad in (0.0, np.nan):
        Pb = P.copy(); Pb[1, 3:] = bad
        with pytest.raises(RuntimeError):
            ab.set_base_pose(Pb)
    assert np.array_equal(ab.base_pose(), P)                     # nothing written
    Pn = P.copy(); Pn[:, 3:] *= 3.0; Pn[0, :3] = (1.0, 2.0, 3.0)
    ab.set_base_pose(Pn)
    got = ab.base_pose()
    assert np.allclose(got[:, 3:], P[:, 3:], rtol=0, atol=1e-15) and np.array_equal(got[0, :3], [1.0, 2.0, 3.0])
    t = torch.zeros((2, 7), dtype=torch.float64, device="cuda")
    ab.base_pose_into(t)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), got)
    ab.close()


def test_cpp_adapter_moves_a_pose_round_trip(tmp_path):
    """test 9: MobyHipArticulatedBody.h built with g++ against libmoby_hip.so: a floating body switched to pose coordinates, stepped, its pose
    read, moved and written back, read again"""
    src = tmp_path / "pose.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "MobyHipArticulatedBody.h"
int main() {
  mh_artic_model m; std::memset(&m, 0, sizeof(m));
  m.nj = 6; m.floating_base = 1;
  for (int v = 0; v < 6; v++) {
    m.parent[v] = v - 1; m.jtype[v] = v < 3 ? MH_JOINT_PRISMATIC : MH_JOINT_REVOLUTE;
    for (int k = 0; k < 9; k++) m.Rrel[v][k] = (k % 4 == 0) ? 1.0 : 0.0;
    m.axis[v][v % 3] = 1.0; m.lolimit[v] = -1.7976931348623157e308; m.hilimit[v] = 1.7976931348623157e308;
  }
  m.trel[0][1] = 1.0; m.mass[5] = 2.0; m.inertia[5][0] = 1.0; m.inertia[5][4] = 2.0; m.inertia[5][8] = 3.0;
  double q[12] = { 0 }, qd[12] = { 0 };
  qd[4] = 12.0; qd[10] = -12.0; qd[3] = 0.1;
  MobyHip::BatchedArticulatedBody r(m, 2, q, qd);
  r.set_base_coords(MH_ARTIC_BASE_POSE);
  r.step(1e-3, 200);
  double P[14];
  r.base_pose(P);
  P[0] += 5.0;
  r.set_base_pose(P);
  double P2[14];
  r.base_pose(P2);
  std::printf("%d %.17g %.17g %.17g %.17g %.17g\n", r.base_coords(), P2[0] - P[0], P2[3] * P2[3] + P2[4] * P2[4] + P2[5] * P2[5] + P2[6] * P2[6], r.q()[4], P[3], P[10]);
  return 0;
}
''')
    exe = str(tmp_path / "pose")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-I" + os.path.join(ROOT, "moby_amd", "cpp"), "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + os.path.join(ROOT, "moby_amd"), "-lmoby_hip", "-Wl,-rpath," + os.path.join(ROOT, "moby_amd"), "-o", exe])
    out = subprocess.check_output([exe], timeout=120).split()
    assert int(out[0]) == A.MH_ARTIC_BASE_POSE and float(out[1]) == 0.0 and abs(float(out[2]) - 1.0) < 1e-15 and float(out[3]) == 0.0
    assert abs(float(out[4]) - np.cos(0.5 * 12.0 * 0.2)) < 0.05         # a fifth of a second at about 12 rad/s about the middle axis
