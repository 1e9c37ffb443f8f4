"""Drives of the articulated stepper (include/moby_hip_artic.h, mh_artic_drive) without a GPU: the driven reference
(tests/native/artic_drive_ref.cpp, a restatement of oracle::Artic::step / do_mini_step with tau) pinned to the oracle -- undriven it IS
oracle_artic_step, driven it is the oracle's own forward dynamics composed with the semi-implicit step -- a servoed pendulum that settles
where the servo balances gravity, and the ctypes mirror of the new struct."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from moby_amd import artic as A
from moby_amd import scene as S
from tests import native_build
from tests.test_artic_gpu import ur10_states
from tests.test_oracle_artic_contacts import tip_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UR10 = os.path.join(ROOT, "tests", "scenes", "ten_joint_arm.sdf")
BALL = os.path.join(ROOT, "tests", "scenes", "floating_spinning_ball.xml")
FIELDS = ("rng", "time", "status", "steps", "mini_steps", "lcp_solves", "lcp_rows", "lcp_pivots", "lcp_alg_bytes", "stab_iters", "stab_rows",
          "vns_size", "zlast_size", "zbuf_size", "zbuf_cap")
INF = np.finfo(float).max


class DriveRef:
    """ctypes face of tests/native/artic_drive_ref.cpp"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.artic_drive_ref_step.restype = None

    def step(self, model, q, qd, aux, dt, nsteps, drive=None):
        """B worlds x nsteps in place; drive: an A.Drive of numpy arrays (or None)"""
        d = None
        if drive is not None:
            drive.check(q.shape[0], model.nj)
            d = A.mh_artic_drive(terms=drive.terms, rows=drive.rows)
            keep = {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in drive.arrays.items() if a is not None}
            for k, a in keep.items():
                setattr(d, k, a.ctypes.data)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self.lib.artic_drive_ref_step(ctypes.byref(model), int(q.shape[0]), ctypes.c_double(dt), int(nsteps), P(q), P(qd), P(aux),
                                      None if d is None else ctypes.byref(d))


@pytest.fixture(scope="session")
def drive_ref():
    return DriveRef(native_build.build(("artic_drive_ref.cpp",), "artic_drive_ref"))


def random_drive(rng, B, nj, rows=1, terms=A.MH_DRIVE_PD | A.MH_DRIVE_FORCE, kp=(0.0, 40.0), kv=(0.0, 4.0), qspan=0.5, tau=5.0):
    """random per-world gains and targets (the PD and feed-forward terms as `terms` asks)"""
    sh = (B, nj) if rows == 1 else (rows, B, nj)
    a = {}
    if terms & A.MH_DRIVE_PD:
        a.update(kp=rng.uniform(*kp, (B, nj)), kv=rng.uniform(*kv, (B, nj)), q_des=rng.uniform(-qspan, qspan, sh), qd_des=rng.uniform(-1.0, 1.0, sh))
    if terms & A.MH_DRIVE_FORCE:
        a.update(tau_ff=rng.uniform(-tau, tau, sh))
    return A.Drive(**a)


def stabilised_chain():
    m = A.chain_model(3, lo=-0.6, hi=0.6, restitution=0.4)
    m.cstab_max_iterations = 10
    return m


def pin_models():
    """name -> (model, q0, qd0, dt, nsteps): every route of the step (limits, restitution + the stabiliser, link contacts under both impact models
    and with the stabiliser, a floating base)"""
    rng = np.random.default_rng(11)
    out = {}
    m, _, _ = A.load_sdf(UR10)
    q, qd = ur10_states(m, 3)
    out["ur10"] = (m, q, qd, 5e-4, 60)
    m = stabilised_chain()
    out["chain_stab"] = (m, rng.uniform(-0.5, 0.5, (3, 3)), rng.uniform(-3.0, 3.0, (3, 3)), 1e-3, 60)
    tips = {"tip_noslip": tip_model(2, floor=-0.75), "tip_ds": tip_model(2, floor=-0.75, mu=0.5), "tip_stab": tip_model(2, floor=-0.75)}
    tips["tip_stab"].cstab_max_iterations = 10
    for name, m in tips.items():
        q = np.column_stack([rng.uniform(0.7, 0.8, 3), rng.uniform(0.1, 0.2, 3)])
        out[name] = (m, q, rng.uniform(-0.5, 0.5, (3, 2)), 1e-3, 200)
    m, _, _, q0, qd0, dt = A.load_xml(BALL)
    q = np.tile(q0, (2, 1)); qd = np.tile(qd0, (2, 1)); q[1, 1] += 0.3; qd[1, 0] = 0.4
    out["ball"] = (m, q, qd, dt, 120)
    return out


@pytest.mark.parametrize("alg", [A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB])
@pytest.mark.parametrize("name", ["ur10", "chain_stab", "tip_noslip", "tip_ds", "tip_stab", "ball"])
def test_undriven_reference_is_the_oracle(oracle, drive_ref, name, alg):
    """pin 1: terms = 0 (and no drive at all) step exactly as oracle_artic_step: q, qd, every counter, the warm starts"""
    m, q0, qd0, dt, n = pin_models()[name]
    m.algorithm = alg
    B = q0.shape[0]
    q_o, qd_o, aux_o = q0.copy(), qd0.copy(), S.new_aux(B)
    oracle.artic_step(m, q_o, qd_o, aux_o, dt, n)
    for drive in (None, A.Drive()):
        q_r, qd_r, aux_r = q0.copy(), qd0.copy(), S.new_aux(B)
        drive_ref.step(m, q_r, qd_r, aux_r, dt, n, drive)
        assert np.array_equal(q_r, q_o) and np.array_equal(qd_r, qd_o)
        for f in FIELDS:
            assert np.array_equal(aux_r[f], aux_o[f]), f
        for w in range(B):
            k = int(aux_o["vns_size"][w]); assert np.array_equal(aux_r["vns"][w, :k], aux_o["vns"][w, :k])
            k = int(aux_o["zlast_size"][w]); assert np.array_equal(aux_r["zlast"][w, :k], aux_o["zlast"][w, :k])
    assert (aux_o["lcp_solves"] > 0).any() or name == "chain_stab"


@pytest.mark.parametrize("alg", [A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB])
@pytest.mark.parametrize("terms", [A.MH_DRIVE_FORCE, A.MH_DRIVE_PD, A.MH_DRIVE_FORCE | A.MH_DRIVE_PD])
def test_one_driven_step_is_the_oracles_forward_dynamics(oracle, drive_ref, alg, terms):
    """pin 2: one step of a chain without limits or spheres is q1 = q0 + qd0 dt, tau(q1, qd0), qdd = oracle_artic_fwd_dyn(q1, qd0, tau),
    qd1 = qd0 + qdd dt -- bit for bit, each term of tau rounded on its own and an absent term left out"""
    m = A.chain_model(4, lo=-INF, hi=INF, prismatic_last=True)
    m.algorithm = alg
    B, dt = 5, 1e-3
    rng = np.random.default_rng(3 + terms)
    q0 = rng.uniform(-1.0, 1.0, (B, 4)); qd0 = rng.uniform(-2.0, 2.0, (B, 4))
    drive = random_drive(rng, B, 4, terms=terms)
    q1, qd1, aux = q0.copy(), qd0.copy(), S.new_aux(B)
    drive_ref.step(m, q1, qd1, aux, dt, 1, drive)
    a = drive.arrays
    for w in range(B):
        qa = qd0[w] * dt; qa = qa + q0[w]
        if terms & A.MH_DRIVE_PD:
            tp = a["kp"][w] * (a["q_des"][w] - qa); tv = a["kv"][w] * (a["qd_des"][w] - qd0[w]); tau = tp + tv
            if terms & A.MH_DRIVE_FORCE:
                tau = tau + a["tau_ff"][w]
        else:
            tau = a["tau_ff"][w].copy()
        r = oracle.artic_fwd_dyn(m, qa, qd0[w], tau)
        assert r["ok"]
        assert np.array_equal(q1[w], qa) and np.array_equal(qd1[w], qd0[w] + r["qdd"] * dt), w
    assert (aux["steps"] == 1).all() and (aux["lcp_solves"] == 0).all()


def test_servoed_pendulum_settles_where_the_servo_balances_gravity(drive_ref):
    """One rod of mass m, length L hinged about y at the origin, hanging along -z (chain_model(1)): its COM sits at
    (-l sin q, 0, -l cos q), l = L / 2, so gravity's torque about the hinge is -m g l sin q.  A PD servo to q_des with kv > 0 comes to rest
    where kp (q_des - q) = m g l sin q; after 10 s the pendulum is there to 1e-6 rad, on both dynamics algorithms."""
    mass, L, g = 1.0, 0.5, 9.81
    for alg in (A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB):
        m = A.chain_model(1, length=L, mass=mass, lo=-INF, hi=INF, gravity=(0.0, 0.0, -g))
        m.algorithm = alg
        q_des = np.array([[0.6], [-1.1], [2.0]]); kp = np.array([[50.0], [20.0], [80.0]]); kv = np.full((3, 1), 2.0)
        q, qd, aux = np.zeros((3, 1)), np.zeros((3, 1)), S.new_aux(3)
        drive_ref.step(m, q, qd, aux, 1e-3, 10000, A.Drive(kp=kp, kv=kv, q_des=q_des, qd_des=np.zeros((3, 1))))
        qe = q_des.copy()
        for _ in range(50):                                    # Newton on f(q) = kp (q_des - q) - m g l sin q
            f = kp * (q_des - qe) - mass * g * (0.5 * L) * np.sin(qe)
            qe = qe - f / (-kp - mass * g * (0.5 * L) * np.cos(qe))
        assert np.abs(q - qe).max() < 1e-6, (q.ravel(), qe.ravel())
        assert np.abs(qd).max() < 1e-6 and (aux["status"] == 0).all()
        assert np.abs(q - q_des).min() > 1e-2                  # gravity holds it off the target: the servo, not the target, sets the rest angle


def test_drive_mirror_has_the_c_struct_size(tmp_path):
    """moby_amd/artic.py's mh_artic_drive against the C struct (size and the last field's offset)"""
    src = tmp_path / "drv.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "moby_hip_artic.h"\n'
                   'int main(void) { printf("%zu %zu %zu %d %d\\n", sizeof(mh_artic_drive), offsetof(mh_artic_drive, kp), offsetof(mh_artic_drive, tau_ff), MH_DRIVE_FORCE, MH_DRIVE_PD); return 0; }\n')
    exe = str(tmp_path / "drv")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    D = A.mh_artic_drive
    assert got == [ctypes.sizeof(D), D.kp.offset, D.tau_ff.offset, A.MH_DRIVE_FORCE, A.MH_DRIVE_PD]


def test_drive_shapes_are_checked():
    B, nj = 3, 2
    z = np.zeros((B, nj))
    with pytest.raises(ValueError):
        A.Drive(kp=z, kv=z, q_des=z)                             # PD without qd_des
    with pytest.raises(ValueError):
        A.Drive(tau_ff=np.zeros((4, B, nj)), kp=z, kv=z, q_des=np.zeros((5, B, nj)), qd_des=z)   # schedules of different lengths
    with pytest.raises(ValueError):
        A.Drive(tau_ff=np.zeros((B, nj + 1))).check(B, nj)
    d = A.Drive(kp=z, kv=z, q_des=np.zeros((7, B, nj)), qd_des=np.zeros((7, B, nj)), tau_ff=np.zeros((7, B, nj)))
    d.check(B, nj)
    assert (d.terms, d.rows) == (A.MH_DRIVE_PD | A.MH_DRIVE_FORCE, 7)
    assert (A.Drive(tau_ff=z).terms, A.Drive().terms) == (A.MH_DRIVE_FORCE, 0)


def test_cpp_adapter_takes_a_drive(tmp_path):
    """MobyHipArticulatedBody.h: set_drive + step build with plain g++ against the C ABI"""
    src = tmp_path / "drv.cpp"
    src.write_text('#include "MobyHipArticulatedBody.h"\n'
                   'void f(MobyHip::BatchedArticulatedBody& r, const double* kp, const double* kv, const double* qdes, const double* qddes) {\n'
                   '  mh_artic_drive d = { MH_DRIVE_PD, 1, kp, kv, qdes, qddes, NULL }; r.set_drive(d); r.step(5e-4, 10); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "moby_amd", "cpp"), str(src)])
