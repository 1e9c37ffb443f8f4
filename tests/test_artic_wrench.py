"""Link wrenches and link damping of the articulated stepper (include/moby_hip_artic.h, "Link wrenches") without a GPU: the reference the kernels
are held to (tests/native/artic_wrench_ref.cpp) pinned from four sides -- it is the report reference when there is no wrench, its generalized
force is the Jacobian transpose's, a one-link floating base under it is the free rigid body of the world reference, its damping dissipates and
follows the header's formulas -- then the refusals (they run before the device is looked for) and the layout of the struct."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import io as mio
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import artic_report_ref as R
from tests import artic_wrench_ref as W
from tests import world_ref
from tests.test_artic_box_gpu import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
MH_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def ref():
    return W.build_wrench_ref()


# one no-slip case, one Drumwright-Shell case, one floating case in pose coordinates (tests/artic_report_ref.py)
NULL_CASES = [c for c in R.CASES if (c[0], c[1], c[2], c[3], c[4]) in (("arm_static", "angles", False, False, 100.0), ("arm_slider_box", "angles", False, True, 0.5),
                                                                      ("floating_box_pendulum", "pose", True, True, 100.0))]


@pytest.mark.parametrize("case", NULL_CASES, ids=R.case_id)
def test_without_a_wrench_it_is_the_report_reference(ref, case):
    """with a NULL wrench and with terms = 0, artic_wrench_ref_step equals artic_report_ref_step bit for bit: q, qd, every aux field, the base pose
    and every report row, over the two launches of the case"""
    assert len(NULL_CASES) == 3
    m, q0, qd0, dt, n, want = R.reference_run(ref, case)
    for null_struct in (False, True):
        q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(R.B)
        Pp = R.model_pose(m, R.B) if case[1] == "pose" else None
        for w in want:
            rep = ref.step_wrench(m, q, qd, aux, dt, n, pose=Pp, drive=w["drive"], wrench=None, null_struct=null_struct)
            same((q, qd, aux), (w["q"], w["qd"], w["aux"]), R.B)
            assert np.array_equal(rep, w["report"])
            if Pp is not None:
                assert np.array_equal(Pp, w["pose"])
    assert (want[-1]["aux"]["lcp_solves"] > 0).any()


@pytest.mark.parametrize("algorithm", [A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB], ids=["crb", "fsab"])
@pytest.mark.parametrize("link_axes", [False, True], ids=["model_axes", "link_axes"])
def test_the_generalized_force_is_the_jacobian_transpose(oracle, ref, algorithm, link_axes):
    """a wrench on the last link of a 3-joint chain against a driven step whose tau_ff is J' [f; n], J the oracle's Jacobian of the link's COM at
    q + qd dt (rows [linear; angular]), built in numpy: one step of dt = 1e-3, the resulting qd to rtol 1e-11, atol 1e-12 (the bounds
    tests/test_artic_floating.py uses for two routes to one qdd)"""
    m = W.chain3(algorithm)
    dt = 1e-3
    q0 = np.array([[0.3, -0.5, 0.7]]); qd0 = np.array([[0.4, -0.2, 0.9]])
    f = np.array([1.5, -0.7, 2.0]); nn = np.array([0.3, 0.8, -0.4])
    wr = np.zeros((1, 3, 6)); wr[0, 2, :3] = f; wr[0, 2, 3:] = nn
    q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(1)
    ref.step_wrench(m, q, qd, aux, dt, 1, wrench=A.LinkWrench(w=wr, link_axes=link_axes))
    q1 = q0[0] + qd0[0] * dt
    Rk, _, _, c = W.fk(m, q1)
    fm, nm = (Rk[2] @ f, Rk[2] @ nn) if link_axes else (f, nn)
    J = oracle.artic_jacobian(m, q1, 2, c[2])
    tau = J[:3].T @ fm + J[3:].T @ nm
    q2, qd2, aux2 = q0.copy(), qd0.copy(), S.new_aux(1)
    ref.step_wrench(m, q2, qd2, aux2, dt, 1, drive=A.Drive(tau_ff=tau.reshape(1, 3)))
    assert np.array_equal(q, q2)
    assert np.allclose(qd, qd2, rtol=1e-11, atol=1e-12), np.abs(qd - qd2).max()
    q3, qd3, aux3 = q0.copy(), qd0.copy(), S.new_aux(1)
    ref.step_wrench(m, q3, qd3, aux3, dt, 1)
    assert np.abs(qd - qd3).max() > 1e-4                              # the wrench does something


def test_a_one_link_floating_base_under_a_wrench_is_the_free_rigid_body(oracle, ref):
    """tests/scenes/floating_spinning_ball.xml against tests/scenes/dropped_spinning_ball.xml through the tests' world reference, both under the same
    constant force at the COM (all three components) and torque, model axes: 300 steps of dt = 1e-3 (the ball is in free flight).  The torque lies
    along the ball's spin axis: the two steppers integrate the orientation in different coordinates (three hinge angles against omega itself), and a
    torque across a 10 rad/s spin makes them differ at first order in dt -- measured 4.0e-5 in omega at dt = 1e-3 and 2.0e-5 at dt = 5e-4 -- which is
    truncation, not the wrench (the components across the axis are pinned by the Jacobian test above).  Measured here: position 2.2e-16 (the largest
    over the trajectory), linear velocity 0 exactly, angular velocity 2.0e-17 (the same pair without a wrench agrees to 1e-12 over 3000 steps,
    tests/test_artic_floating.py).  The bounds are ten times the measured values; anything near 1e-9 would be a bug, not round-off."""
    m, _, _, q0, qd0, _ = A.load_xml(os.path.join(HERE, "scenes", "floating_spinning_ball.xml"))
    sc, st0, ids, _ = mio.load_xml(os.path.join(HERE, "scenes", "dropped_spinning_ball.xml"))
    b = ids.index("ball")
    dt, steps = 1e-3, 300
    wrench = np.array([0.8, 0.3, -0.5, 0.0, -0.05, 0.0])
    ww = np.zeros((1, sc.nb, 6)); ww[0, b] = wrench
    st = st0.copy().reshape(1, -1); auxw = S.new_aux(1)
    traj = world_ref.reference().step(sc, st, auxw, dt, steps, wrench=ww, want_traj=True).traj
    wa = np.zeros((1, m.nj, 6)); wa[0, 5] = wrench
    q = q0.reshape(1, -1).copy(); qd = qd0.reshape(1, -1).copy(); aux = S.new_aux(1)
    lw = A.LinkWrench(w=wa)
    dx = 0.0
    for k in range(steps):
        ref.step_wrench(m, q, qd, aux, dt, 1, wrench=lw, sink=False)
        dx = max(dx, np.abs(W.fk(m, q[0])[3][5] - traj[0, k, b, :3]).max())
    J = oracle.artic_jacobian(m, q[0], 5, np.zeros(3))               # rows 3..5: the hinges' axes by the oracle's own kinematics (no libm in the bound)
    om = np.array([(J[3 + k, 3] * qd[0, 3] + J[3 + k, 4] * qd[0, 4]) + J[3 + k, 5] * qd[0, 5] for k in range(3)])
    s = st.reshape(-1, S.MH_BODY_STATE)[b]
    dv = np.abs(qd[0, :3] - s[7:10]).max(); dw = np.abs(om - s[10:13]).max()
    print("free-body pin: max |dx| = %.3e, |dv| = %.3e, |domega| = %.3e" % (dx, dv, dw))
    assert aux["status"][0] == 0 and auxw["status"][0] == 0 and aux["mini_steps"][0] == auxw["mini_steps"][0] == steps
    assert np.abs(s[7:10] - st0.reshape(-1, S.MH_BODY_STATE)[b, 7:10] - np.array([0.0, -9.81, 0.0]) * dt * steps).max() > 0.05    # the force moved it
    assert abs(s[11] - st0.reshape(-1, S.MH_BODY_STATE)[b, 11]) > 5e-3                                        # ... and the torque slowed the spin
    assert dx < 2.3e-15 and dv == 0.0 and dw < 2.1e-16


def test_a_torque_across_the_spin_differs_by_truncation_only(oracle, ref):
    """the same pair under a torque with components across the 10 rad/s spin, over the same 0.3 s at dt = 1e-3 and at dt = 5e-4: the angular
    velocities differ by 4.0e-5 and 2.0e-5 (measured) -- the difference halves with dt, which is what a first-order truncation of two orientation
    coordinate sets does and what an error of the wrench (the same at every dt) would not; the ratio is asserted within 5 % of 2 (its own
    correction is of relative order dt |omega| = 1e-2).  Position and linear velocity do not involve the orientation and stay at round-off."""
    m, _, _, q0, qd0, _ = A.load_xml(os.path.join(HERE, "scenes", "floating_spinning_ball.xml"))
    sc, st0, ids, _ = mio.load_xml(os.path.join(HERE, "scenes", "dropped_spinning_ball.xml"))
    b = ids.index("ball")
    wrench = np.array([0.8, 0.3, -0.5, 0.02, -0.05, 0.03])
    dw = []
    for dt, steps in ((1e-3, 300), (5e-4, 600)):
        ww = np.zeros((1, sc.nb, 6)); ww[0, b] = wrench
        st = st0.copy().reshape(1, -1); auxw = S.new_aux(1)
        world_ref.reference().step(sc, st, auxw, dt, steps, wrench=ww)
        wa = np.zeros((1, m.nj, 6)); wa[0, 5] = wrench
        q = q0.reshape(1, -1).copy(); qd = qd0.reshape(1, -1).copy(); aux = S.new_aux(1)
        ref.step_wrench(m, q, qd, aux, dt, steps, wrench=A.LinkWrench(w=wa), sink=False)
        J = oracle.artic_jacobian(m, q[0], 5, np.zeros(3))
        om = np.array([(J[3 + k, 3] * qd[0, 3] + J[3 + k, 4] * qd[0, 4]) + J[3 + k, 5] * qd[0, 5] for k in range(3)])
        s = st.reshape(-1, S.MH_BODY_STATE)[b]
        assert np.abs(qd[0, :3] - s[7:10]).max() < 1e-14 and np.abs(W.fk(m, q[0])[3][5] - s[:3]).max() < 1e-14
        dw.append(np.abs(om - s[10:13]).max())
    print("cross-axis torque: |domega| = %.3e at dt = 1e-3, %.3e at dt = 5e-4" % tuple(dw))
    assert 1e-5 < dw[0] < 1e-4 and 1.9 < dw[0] / dw[1] < 2.1


def test_gpu_cases_keep_their_point(ref):
    """the cases of tests/test_artic_wrench_gpu.py on the reference alone: in every one the wrench changes the result; the arm and both floating-box
    cases have a step with more than one mini-step in every world (so the wrench is evaluated at two configurations inside one step), solve LCPs and
    report a contact; the records of the params case lie on both sides of mu = 100 and exchanging two worlds' wrench rows changes exactly those worlds"""
    N = W.NSTEPS
    for c, contacts in ((W.case_chain(W.CRB, 1), False), (W.case_chain(W.FSAB, N), False), (W.case_chain_damped(), False), (W.case_arm(), True),
                        (W.case_foot(), True), (W.case_params(), True)):
        r, r0 = W.reference_of(ref, c), W.reference_of(ref, c, wrench=None)
        for w in range(W.B):
            assert np.abs(r["qd"][w] - r0["qd"][w]).max() > 1e-3
        assert (r["aux"]["status"] == 0).all() and (r["aux"]["steps"] == N).all()
        if contacts:
            assert (r["aux"]["mini_steps"] > N).all() and (r["aux"]["lcp_solves"] > 0).all() and (r["report"][..., 0] > 0).any(axis=(1, 2)).all()
    c = W.case_params()
    mu = c["params"]["cp_mu_coulomb"]
    assert (mu < 100.0).any() and (mu >= 100.0).any()
    r, r2 = W.reference_of(ref, c), W.reference_of(ref, c, wrench=W.swapped(c["wrench"], 0, 2))
    assert np.array_equal(r["qd"][1], r2["qd"][1]) and not np.array_equal(r["qd"][0], r2["qd"][0]) and not np.array_equal(r["qd"][2], r2["qd"][2])


def test_cpp_example_compiles_and_fails_loudly_without_a_gpu(tmp_path):
    """example_artic_wrench.cpp (with_wrench / step_wrench with device arrays of its own): the example builds; without a device it reports the error
    (no fallback), with one it runs to its end -- the harder push drifts further, the ground returns an impulse in every copy"""
    import torch
    cpp = os.path.join(ROOT, "moby_amd", "cpp")
    exe = str(tmp_path / "example_artic_wrench")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-Wall", os.path.join(cpp, "example_artic_wrench.cpp"), "-L" + os.path.join(ROOT, "moby_amd"), "-lmoby_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "moby_amd"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, timeout=120)
    if torch.cuda.is_available():
        assert p.returncode == 0 and b"copy 3: push 12.0 N" in p.stdout, p.stdout
    else:
        assert p.returncode == 1 and b"no HIP device" in p.stdout, p.stdout


def _damped(nB=1):
    m = W.free_body()
    rng = np.random.default_rng(4)
    q0 = np.zeros((nB, 6)); q0[:, 3:] = rng.uniform(-0.3, 0.3, (nB, 3))
    qd0 = np.concatenate([rng.uniform(0.5, 1.5, (nB, 3)), rng.uniform(1.0, 2.0, (nB, 3))], axis=1)
    k = {name: np.zeros((nB, 6)) for name in A.LinkWrench._DAMP}
    k["kl"][:, 5] = 0.8; k["ka"][:, 5] = 0.03; k["klsq"][:, 5] = 0.5; k["kasq"][:, 5] = 0.01
    return m, q0, qd0, k


def test_damping_dissipates_and_follows_the_formulas(oracle, ref):
    """a spinning, drifting one-link floating body without gravity, all four gains positive on the base link (isotropic inertia, so that |omega| has
    no exchange between axes to hide the damping behind): |v| and |omega| decrease at every one of 200 steps; the first step equals a numpy
    evaluation of the header's damping rules (tau_x by numpy, H qdd = tau_x - C by the oracle) to 1e-14 relative"""
    m, q0, qd0, k = _damped()
    dt = 1e-3
    lw = A.LinkWrench(**k)
    q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(1)
    nv, nw = [np.linalg.norm(qd0[0, :3])], [np.linalg.norm(W.link_velocity(m, W.fk(m, q0[0])[2], qd0[0], 5)[:3])]
    first = None
    for s in range(200):
        ref.step_wrench(m, q, qd, aux, dt, 1, wrench=lw, sink=False)
        if s == 0:
            first = qd.copy()
        nv.append(np.linalg.norm(qd[0, :3])); nw.append(np.linalg.norm(W.link_velocity(m, W.fk(m, q[0])[2], qd[0], 5)[:3]))
    assert (np.diff(nv) < 0.0).all() and (np.diff(nw) < 0.0).all()
    assert nv[-1] < 0.95 * nv[0] and nw[-1] < 0.95 * nw[0]
    # the first step by hand
    q1 = q0[0] + qd0[0] * dt
    Rk, _, Sm, c = W.fk(m, q1)
    V = W.link_velocity(m, Sm, qd0[0], 5)
    vc = V[3:] + np.cross(V[:3], c[5])
    vi, wi = Rk[5].T @ vc, Rk[5].T @ V[:3]
    fb = vi * (-(k["kl"][0, 5] + np.linalg.norm(vi) * k["klsq"][0, 5])); tb = wi * (-(k["ka"][0, 5] + np.linalg.norm(wi) * k["kasq"][0, 5]))
    F, T = Rk[5] @ fb, Rk[5] @ tb
    F6 = np.concatenate([T + np.cross(c[5], F), F])
    tau = Sm @ F6                                                     # every joint is an ancestor of link 5; the virtual links carry zero gains
    qdd = oracle.artic_fwd_dyn(m, q1, qd0[0], tau=tau)["qdd"]
    want = qd0[0] + qdd * dt
    assert np.abs(first[0] - want).max() <= 1e-14 * np.abs(want).max(), np.abs(first[0] - want).max()


def _step_wrench(ab, w, nsteps=4, report=None, drive=None):
    rc = _lib.load().mh_artic_batch_step_wrench(ab, None, ctypes.c_double(1e-3), nsteps, drive, None if w is None else ctypes.byref(w), report)
    return rc, _lib.load().mh_last_error().decode()


def test_refusals_name_the_field_without_a_device():
    """every refusal of mh_artic_batch_step_wrench that needs no batch comes before the batch is looked at (so: before the device is looked for) and
    names its field; mh_artic_batch_create_wrench has the refusals of mh_artic_batch_create_params.  The two refusals that need a batch (a wrench on a
    batch of another create, report_dev without the flag) are in tests/test_artic_wrench_gpu.py"""
    buf = np.zeros(64)
    p = buf.ctypes.data
    T = A.mh_artic_wrench
    for w, word in ((T(terms=8, rows=1, w=p), "unknown bits 0x8 in terms"),
                    (T(terms=A.MH_LINK_WRENCH_LINK_AXES, rows=1, w=p), "MH_LINK_WRENCH_LINK_AXES without MH_LINK_WRENCH"),
                    (T(terms=A.MH_LINK_WRENCH, rows=1), "NULL w"),
                    (T(terms=A.MH_LINK_DAMPING, rows=1, ka=p, klsq=p, kasq=p), "NULL kl "),
                    (T(terms=A.MH_LINK_DAMPING, rows=1, kl=p, klsq=p, kasq=p), "NULL ka "),
                    (T(terms=A.MH_LINK_DAMPING, rows=1, kl=p, ka=p, kasq=p), "NULL klsq"),
                    (T(terms=A.MH_LINK_DAMPING | A.MH_LINK_WRENCH, rows=1, w=p, kl=p, ka=p, klsq=p), "NULL kasq"),
                    (T(terms=A.MH_LINK_WRENCH, rows=0, w=p), "rows = 0 < 1"),
                    (T(terms=A.MH_LINK_WRENCH, rows=3, w=p), "3 schedule rows for 4 steps")):
        rc, msg = _step_wrench(None, w)
        assert rc == MH_ERR_INVALID_ARG and msg.startswith("wrench:") and word in msg, msg
    for w in (None, T(terms=0), T(terms=A.MH_LINK_WRENCH, rows=4, w=p), T(terms=A.MH_LINK_WRENCH, rows=1, w=p)):
        rc, msg = _step_wrench(None, w)
        assert rc == MH_ERR_INVALID_ARG and "null batch" in msg, msg
    lib = _lib.load()
    m = BS.mixed_all()[0]
    h = ctypes.c_void_p()
    assert lib.mh_artic_batch_create_wrench(ctypes.byref(m), None, 2, 2, ctypes.byref(h)) == MH_ERR_INVALID_ARG and "unknown bits 0x2 in flags" in lib.mh_last_error().decode()
    bad = A.make_params(m, 3); bad["mass"][1, 7] = -1.0
    assert lib.mh_artic_batch_create_wrench(ctypes.byref(m), bad.ctypes.data, 3, 0, ctypes.byref(h)) == MH_ERR_INVALID_ARG
    assert lib.mh_last_error().decode().startswith("world 1: link 7: mass") and not h
    assert lib.mh_artic_batch_create_wrench(ctypes.byref(m), None, 0, 0, ctypes.byref(h)) == MH_ERR_INVALID_ARG and "batch must be > 0" in lib.mh_last_error().decode()
    nogeom = W.chain3(A.MH_ARTIC_CRB)
    assert lib.mh_artic_batch_create_wrench(ctypes.byref(nogeom), None, 2, A.MH_ARTIC_CREATE_REPORT, ctypes.byref(h)) == MH_ERR_INVALID_ARG and "needs geometry" in lib.mh_last_error().decode()
    assert lib.mh_debug_set(21, 2) == MH_ERR_INVALID_ARG and lib.mh_debug_set(21, 0) == 0


def test_python_side_checks_the_wrench():
    z = np.zeros((2, 3))
    with pytest.raises(ValueError, match="kl, ka, klsq and kasq"):
        A.LinkWrench(kl=z, ka=z)
    with pytest.raises(ValueError, match="link_axes without w"):
        A.LinkWrench(kl=z, ka=z, klsq=z, kasq=z, link_axes=True)
    lw = A.LinkWrench(w=np.zeros((3, 2, 3, 6)), kl=z, ka=z, klsq=z, kasq=z, link_axes=True)
    assert lw.terms == 7 and lw.rows == 3
    lw.check(2, 3, 3); lw.check(2, 3, 1)
    with pytest.raises(ValueError, match="3 schedule rows for 4 steps"):
        lw.check(2, 3, 4)
    with pytest.raises(ValueError, match="LinkWrench.w"):
        lw.check(2, 4, 3)
    assert A.LinkWrench(w=np.zeros((2, 3, 6))).rows == 1 and A.LinkWrench(w=np.zeros((2, 3, 6))).terms == A.MH_LINK_WRENCH


def test_mirror_has_the_c_layout(tmp_path):
    src = tmp_path / "sz.c"
    fields = [f for f, _ in A.mh_artic_wrench._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "moby_hip_artic.h"\nint main(void) {\n'
                   '  printf("%zu %d %d %d %d\\n", sizeof(mh_artic_wrench), MH_ARTIC_WRENCH, MH_LINK_WRENCH, MH_LINK_DAMPING, MH_LINK_WRENCH_LINK_AXES);\n'
                   + "".join('  printf("%%zu\\n", offsetof(mh_artic_wrench, %s));\n' % f for f in fields) + "  return 0; }\n")
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [[int(x) for x in ln.split()] for ln in subprocess.check_output([exe]).decode().splitlines()]
    assert got[0] == [ctypes.sizeof(A.mh_artic_wrench), 1, A.MH_LINK_WRENCH, A.MH_LINK_DAMPING, A.MH_LINK_WRENCH_LINK_AXES] == [48, 1, 1, 2, 4]
    assert [g[0] for g in got[1:]] == [getattr(A.mh_artic_wrench, f).offset for f in fields]


def test_cpp_adapter_takes_wrenches(tmp_path):
    """MobyHipArticulatedBody.h: with_wrench + step_wrench build with plain g++ against the C ABI, and a refusal of mh_artic_batch_create_wrench
    reaches the caller as an exception"""
    src = tmp_path / "wr.cpp"
    src.write_text('#include <cstdio>\n#include <vector>\n#include "MobyHipArticulatedBody.h"\n'
                   'int main() {\n  mh_artic_model m = mh_artic_model();\n  m.nj = 3; m.gravity[2] = -9.81;\n'
                   '  for (int i = 0; i < 3; i++) { m.parent[i] = i - 1; m.axis[i][1] = 1.0; m.mass[i] = 1.0; m.trel[i][2] = -0.5; m.lolimit[i] = -1.0; m.hilimit[i] = 1.0;\n'
                   '    for (int k = 0; k < 3; k++) { m.Rrel[i][4 * k] = 1.0; m.inertia[i][4 * k] = 0.01; } }\n  std::vector<mh_artic_params> p(2);\n'
                   '  for (size_t w = 0; w < p.size(); w++) mh_artic_params_from_model(&m, &p[w]);\n  p[1].axis[2][1] = 0.5;\n'
                   '  std::vector<double> q(6, 0.0);\n  mh_artic_wrench w = mh_artic_wrench(); w.terms = MH_LINK_WRENCH | MH_LINK_WRENCH_LINK_AXES; w.rows = 1;\n'
                   '  try { MobyHip::BatchedArticulatedBody* r = MobyHip::BatchedArticulatedBody::with_wrench(m, p.data(), 2, q.data(), q.data()); r->step_wrench(1e-3, 2, w); delete r; }\n'
                   '  catch (const std::exception& e) { std::printf("%s\\n", e.what()); return 3; }\n  return 0; }\n')
    exe = str(tmp_path / "wr")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "moby_amd", "cpp"), str(src), "-L" + os.path.join(ROOT, "moby_amd"),
                           "-lmoby_hip", "-Wl,-rpath," + os.path.join(ROOT, "moby_amd"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE)
    assert r.returncode == 3 and r.stdout.decode().startswith("world 1: joint 2: axis"), r.stdout
