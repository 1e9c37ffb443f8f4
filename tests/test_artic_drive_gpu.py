"""Drives on the GPU (include/moby_hip_artic.h: mh_artic_batch_step_driven, mh_artic_batch_set_drive, mh_artic_batch_state_dev): every driven
kernel bit for bit against the driven reference (tests/native/artic_drive_ref.cpp), the undriven paths through the new entry points equal to
mh_artic_batch_step, a GPU-resident control loop, exceptions, argument checks, and the reference's ur10 controller as a drive."""
import ctypes
import os

import numpy as np
import pytest

from moby_amd import _lib
from moby_amd import artic as A
from moby_amd import scene as S
from tests.test_artic_drive import FIELDS, drive_ref, pin_models, random_drive  # noqa: F401  (drive_ref: the session fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UR10 = os.path.join(ROOT, "tests", "scenes", "ten_joint_arm.sdf")
PDF = A.MH_DRIVE_PD | A.MH_DRIVE_FORCE
# launch L: (terms, schedule rows or None = one row per step) -- the host changes the drive between launches, held and per-step rows alternate
LAUNCHES = [(PDF, 1), (PDF, None), (A.MH_DRIVE_FORCE, 1), (A.MH_DRIVE_PD, None)]


def same(ab_out, ref, B):
    (q_g, qd_g, aux_g), (q_r, qd_r, aux_r) = ab_out, ref
    assert np.array_equal(q_g, q_r), "max |dq| = %.3e" % np.abs(q_g - q_r).max()
    assert np.array_equal(qd_g, qd_r), "max |dqd| = %.3e" % np.abs(qd_g - qd_r).max()
    for f in FIELDS:
        assert np.array_equal(aux_g[f], aux_r[f]), f
    for w in range(B):
        k = int(aux_r["vns_size"][w]); assert np.array_equal(aux_g["vns"][w, :k], aux_r["vns"][w, :k])
        k = int(aux_r["zlast_size"][w]); assert np.array_equal(aux_g["zlast"][w, :k], aux_r["zlast"][w, :k])


ROUTES = [("ur10", A.MH_ARTIC_CRB), ("ur10", A.MH_ARTIC_FSAB), ("chain_stab", None), ("tip_noslip", None), ("tip_ds", None), ("tip_stab", None), ("ball", None)]


@pytest.mark.parametrize("name,alg", ROUTES)
def test_driven_kernels_match_the_reference(drive_ref, name, alg):
    """k_artic_step_w4_drive (the arm, CRB and FSAB), k_artic_step_stab_drive (the stabilised chain), k_artic_step_contacts[_stab]_drive (tip
    spheres under the no-slip model, the Drumwright-Shell model, with the stabiliser), the floating ball: random per-world gains, targets and
    forces, held and per-step schedules, four launches with the drive changed in between"""
    m, q0, qd0, dt, n = pin_models()[name]
    if alg is not None:
        m.algorithm = alg
    n = min(n, 60)
    B, nj = q0.shape[0], m.nj
    gains = {"ur10": dict(kp=(0.0, 5.0), kv=(0.0, 0.05), tau=2.0), "ball": dict(kp=(0.0, 5.0), kv=(0.0, 0.05), tau=2.0),
             "chain_stab": dict(tau=20.0)}.get(name, {})            # (chain_stab: forces that push joint 0 past a limit, where the stabiliser looks)
    rng = np.random.default_rng(sum(map(ord, name)))
    ab = A.ArticBatch(m, q0, qd0)
    q_r, qd_r, aux_r = q0.copy(), qd0.copy(), S.new_aux(B)
    for terms, rows in LAUNCHES:
        d = random_drive(rng, B, nj, rows=rows or n, terms=terms, **gains)
        ab.step(dt, n, drive=d)
        drive_ref.step(m, q_r, qd_r, aux_r, dt, n, d)
        same(ab.download(), (q_r, qd_r, aux_r), B)
    assert np.isfinite(q_r).all()
    if name.startswith("tip") or name in ("ur10", "ball"):
        assert (aux_r["lcp_solves"] > 0).any()
    if name in ("chain_stab", "tip_stab"):
        assert (aux_r["stab_iters"] > 0).any()
    ab.close()


def test_undriven_through_the_new_entry_points_is_the_plain_step(drive_ref):
    """step_driven with terms = 0, and after set_drive + clear, is mh_artic_batch_step bit for bit; a stored drive is the same drive passed per launch"""
    m, q0, qd0, dt, n = pin_models()["ur10"]
    B = q0.shape[0]
    lib = _lib.load()
    runs = [A.ArticBatch(m, q0, qd0) for _ in range(3)]
    _lib.check(lib.mh_artic_batch_step(runs[0].handle, None, dt, n))
    zero = A.mh_artic_drive()                                      # terms 0, every pointer NULL, rows 0: nothing else is read
    _lib.check(lib.mh_artic_batch_step_driven(runs[1].handle, None, dt, n, ctypes.byref(zero)))
    runs[2].set_drive(random_drive(np.random.default_rng(1), B, m.nj)); runs[2].set_drive(None)
    runs[2].step(dt, n)
    out = [r.download() for r in runs]
    for o in out[1:]:
        same(o, out[0], B)
    d = random_drive(np.random.default_rng(2), B, m.nj, rows=n, kp=(0.0, 5.0), kv=(0.0, 0.05), tau=2.0)
    runs[0].set_drive(d); runs[0].step(dt, n)
    runs[1].step(dt, n, drive=d)
    same(runs[0].download(), runs[1].download(), B)
    for r in runs:
        r.close()


def test_gpu_resident_control_loop_equals_the_host_loop():
    """state_into -> a policy in torch on the device (q_des from q) -> step with tensor pointers, 20 launches on torch's stream, equals the same loop
    with numpy on the host bit for bit"""
    import torch
    m, _, _ = A.load_sdf(UR10)
    from tests.test_artic_gpu import ur10_states
    B, nj, dt, n = 64, m.nj, 5e-4, 10
    q0, qd0 = ur10_states(m, B, seed=5)
    rng = np.random.default_rng(9)
    kp = rng.uniform(0.0, 5.0, (B, nj)); kv = rng.uniform(0.0, 0.05, (B, nj)); target = rng.uniform(-0.5, 0.5, (B, nj))
    dev = torch.device("cuda", 0)
    ab_d = A.ArticBatch(m, q0, qd0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    q_t = torch.empty((B, nj), dtype=torch.float64, device=dev); qd_t = torch.empty_like(q_t)
    kp_t, kv_t, tg_t = (torch.from_numpy(a).to(dev) for a in (kp, kv, target))
    zero_t = torch.zeros_like(q_t)
    for _ in range(20):
        ab_d.state_into(q_t, qd_t, stream=stream)
        q_des = 0.5 * q_t + tg_t                                    # (two kernels: no contraction into an FMA)
        ab_d.step(dt, n, stream=stream, drive=A.Drive(kp=kp_t, kv=kv_t, q_des=q_des, qd_des=zero_t, tau_ff=-qd_t))
    torch.cuda.synchronize(dev)
    ab_h = A.ArticBatch(m, q0, qd0)
    for _ in range(20):
        q, qd, _ = ab_h.download()
        ab_h.step(dt, n, drive=A.Drive(kp=kp, kv=kv, q_des=0.5 * q + target, qd_des=np.zeros((B, nj)), tau_ff=-qd))
    same(ab_d.download(), ab_h.download(), B)
    q, qd, aux = ab_d.download()
    assert (aux["steps"] == 200).all() and np.isfinite(q).all()
    ab_d.close(); ab_h.close()


def test_a_failed_world_is_passed_over_under_a_drive(drive_ref):
    """a world uploaded with MH_WORLD_LCP_FAILED keeps its state and counters (the run ended at the exception), the others are driven on"""
    m, q0, qd0, dt, n = pin_models()["tip_noslip"]
    B = q0.shape[0]
    aux0 = S.new_aux(B); aux0["status"][1] = S.MH_WORLD_LCP_FAILED; aux0["steps"][1] = 7
    ab = A.ArticBatch(m, q0, qd0, aux0)
    d = random_drive(np.random.default_rng(4), B, m.nj)
    ab.step(dt, n, drive=d)
    q_r, qd_r, aux_r = q0.copy(), qd0.copy(), aux0.copy()
    drive_ref.step(m, q_r, qd_r, aux_r, dt, n, d)
    out = ab.download()
    same(out, (q_r, qd_r, aux_r), B)
    q, qd, aux = out
    assert np.array_equal(q[1], q0[1]) and np.array_equal(qd[1], qd0[1]) and aux[1].tobytes() == aux0[1].tobytes()
    assert (aux["steps"][[0, 2]] == n).all()
    ab.close()


def test_invalid_drives_are_refused():
    m, q0, qd0, dt, n = pin_models()["ur10"]
    B, nj = q0.shape[0], m.nj
    lib = _lib.load()
    ab = A.ArticBatch(m, q0, qd0)
    z = np.zeros((B, nj)); p = z.ctypes.data
    import torch
    zt = torch.zeros((B, nj), dtype=torch.float64, device="cuda"); pt = zt.data_ptr()
    full = dict(kp=pt, kv=pt, q_des=pt, qd_des=pt, tau_ff=pt)
    bad = [dict(full, terms=4, rows=1),                                            # unknown bit
           dict(full, terms=A.MH_DRIVE_FORCE, rows=1, tau_ff=None),                # NULL for a requested term
           dict(full, terms=A.MH_DRIVE_PD, rows=1, kv=None),
           dict(full, terms=PDF, rows=0),                                          # rows < 1
           dict(full, terms=PDF, rows=2)]                                          # 1 < rows < nsteps (nsteps = 5 below)
    for kw in bad:
        d = A.mh_artic_drive(**kw)
        assert lib.mh_artic_batch_step_driven(ab.handle, None, dt, 5, ctypes.byref(d)) == _lib.MH_ERR_INVALID_ARG, kw
        assert b"drive" in lib.mh_last_error()
    for kw in bad[:4]:
        d = A.mh_artic_drive(**dict(kw, **{k: p for k in ("kp", "kv", "q_des", "qd_des", "tau_ff") if kw.get(k)}))
        assert lib.mh_artic_batch_set_drive(ab.handle, ctypes.byref(d)) == _lib.MH_ERR_INVALID_ARG, kw
    # a stored schedule shorter than the launch is refused at the step
    ab.set_drive(A.Drive(tau_ff=np.zeros((3, B, nj))))
    assert lib.mh_artic_batch_step_driven(ab.handle, None, dt, 5, None) == _lib.MH_ERR_INVALID_ARG
    assert lib.mh_artic_batch_step_driven(ab.handle, None, dt, 3, None) == _lib.MH_OK
    q, qd, aux = ab.download()
    assert (aux["steps"] == 3).all()                               # only the valid launch ran
    ab.close()


def ur10_controller(t):
    """example/ur10/controller.cpp's targets at time t (PERIOD 5, AMP 0.5): joint -> (q_des, qd_des), in the model's joint order"""
    P, AMP = 5.0, 0.5
    SMALL = AMP * 0.1
    w = {1: (1.0, AMP * P), 2: (2.0, SMALL * P * 2.0), 3: (2.0 / 3.0, AMP * P * 2.0 / 3.0), 4: (1.0 / 7.0, AMP * P / 7.0),
         5: (2.0 / 11.0, AMP * P * 2.0 / 11.0), 6: (3.0 / 13.0, AMP * P * 3.0 / 13.0)}
    q = np.zeros(10); qd = np.zeros(10)
    for j, (f, a) in w.items():
        q[j] = np.sin(t * f) * a; qd[j] = np.cos(t * f) * a
    return q, qd


def test_ur10_controller_as_a_drive_tracks_the_shoulder_pan():
    """The reference's config-5 controller as a drive: gains 300/120 (shoulder), 60/24 (elbow), 15/6 (wrists), its sinusoids sampled per step into
    R = nsteps schedules, the fingers pushed with +-100 N, for 1 s from the targets' start state (no transient).
    Step size: 1e-4, not ur10.xml's 5e-4.  The shoulder pan's torque acts between the arm and the light base link on the near-fixed world_joint,
    and the velocity gain enters explicitly: at 5e-4, kv dt (H^-1)_11 = 120 x 5e-4 x 89 = 5.3 > 2 and the run diverges within 20 steps (the
    reference's controller, evaluated the same way, would do the same); at 1e-4 it is stable.
    Bound: the pan turns about the vertical, so gravity puts no torque on it; its error e obeys H11 e'' + kv e' + kp e = H11 q_des'' + (the other
    joints' coupling), with |q_des''| <= 2.5 rad/s^2 at w = 1 rad/s.  The forced response is |e| <= H11 2.5 / |kp - H11 w^2 + i kv w|, H11 read
    from the generalized inertia along the run (about 13 kg m^2: 0.105 rad); half as much again covers the coupling.  Undriven, the same start
    state ends five times farther from the targets at the least."""
    m, _, _ = A.load_sdf(UR10)
    dt, steps, per = 1e-4, 10000, 500
    B = 2
    q0, qd0 = ur10_controller(0.0)
    kp = np.zeros(10); kv = np.zeros(10)
    kp[[1, 2]], kv[[1, 2]] = 300.0, 120.0
    kp[3], kv[3] = 60.0, 24.0
    kp[[4, 5, 6]], kv[[4, 5, 6]] = 15.0, 6.0
    tau = np.zeros(10); tau[8], tau[9] = 100.0, -100.0
    Q = np.tile(q0, (B, 1)); QD = np.tile(qd0, (B, 1))
    driven, free = A.ArticBatch(m, Q, QD), A.ArticBatch(m, Q, QD)
    H11 = driven.fwd_dyn()[1][:, 1, 1].max()
    err = 0.0
    for L in range(steps // per):
        sched = [ur10_controller((L * per + s) * dt) for s in range(per)]
        qs = np.array([np.tile(a, (B, 1)) for a, _ in sched]); qds = np.array([np.tile(b, (B, 1)) for _, b in sched])
        driven.step(dt, per, drive=A.Drive(kp=np.tile(kp, (B, 1)), kv=np.tile(kv, (B, 1)), q_des=qs, qd_des=qds, tau_ff=np.tile(tau, (per, B, 1))))
        free.step(dt, per)
        q, qd, aux = driven.download()
        q_end, _ = ur10_controller((L + 1) * per * dt)
        err = max(err, float(np.abs(q[:, 1] - q_end[1]).max()))
        H11 = max(H11, driven.fwd_dyn()[1][:, 1, 1].max())
    bound = 1.5 * H11 * 2.5 / abs(complex(300.0 - H11, 120.0))
    assert err < bound, (err, bound, H11)
    assert (aux["status"] & ~S.MH_WORLD_IMPACT_TOL == 0).all() and (aux["steps"] == steps).all() and np.isfinite(q).all()
    qf, _, _ = free.download()
    q_end, _ = ur10_controller(steps * dt)
    arm = slice(1, 7)
    assert np.linalg.norm(qf[0, arm] - q_end[arm]) > 5 * np.linalg.norm(q[0, arm] - q_end[arm])
    driven.close(); free.close()
