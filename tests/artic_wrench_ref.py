"""The link-wrench reference's ctypes face (tests/native/artic_wrench_ref.cpp) and what the CPU tests (tests/test_artic_wrench.py) and the GPU tests
(tests/test_artic_wrench_gpu.py) of the articulated stepper's link wrenches share (include/moby_hip_artic.h, "Link wrenches").  A batch that takes
wrenches is a per-world-parameters batch, so the per-world runner of tests/artic_params_ref.py is reused: one reference run per world on the model
with that world's record, here with that world's rows of the wrench."""
import ctypes

import numpy as np

from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import artic_params_ref as P
from tests import artic_report_ref as R
from tests import native_build

RP = A.REPORT_PAIR


class WrenchRef(R.ReportRef):
    """ctypes face of tests/native/artic_wrench_ref.cpp; the library holds the report reference too (that file is included into it)"""

    def __init__(self, path):
        super().__init__(path)
        self.lib.artic_wrench_ref_step.restype = None

    def step_wrench(self, model, q, qd, aux, dt, nsteps, pose=None, drive=None, wrench=None, sink=True, diag=False, null_struct=False):
        """ReportRef.step_report with a wrench: an A.LinkWrench of numpy arrays (host arrays take the place of the device arrays), or None -- then a
        NULL pointer is passed, or with null_struct=True a struct whose terms are 0"""
        keep = []
        d = None
        if drive is not None:
            drive.check(q.shape[0], model.nj)
            d = A.mh_artic_drive(terms=drive.terms, rows=drive.rows)
            for k, a in drive.arrays.items():
                if a is not None:
                    keep.append(np.ascontiguousarray(a, dtype=np.float64)); setattr(d, k, keep[-1].ctypes.data)
        B = int(q.shape[0])
        w = None
        if wrench is not None:
            wrench.check(B, model.nj, int(nsteps))
            w = A.mh_artic_wrench(terms=wrench.terms, rows=wrench.rows)
            for k, a in wrench.arrays.items():
                if a is not None:
                    keep.append(np.ascontiguousarray(a, dtype=np.float64)); setattr(w, k, keep[-1].ctypes.data)
        elif null_struct:
            w = A.mh_artic_wrench(terms=0, rows=0)
        rep = np.full((B, int(nsteps), A.report_slots(model), RP), np.nan) if sink else None
        dg = np.zeros((B, int(nsteps), 2)) if diag else None
        Pt = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        self.lib.artic_wrench_ref_step(ctypes.byref(model), B, ctypes.c_double(dt), int(nsteps), Pt(q), Pt(qd), Pt(aux), Pt(pose),
                                       None if d is None else ctypes.byref(d), None if w is None else ctypes.byref(w), Pt(rep), Pt(dg))
        del keep
        return (rep, dg[..., 0].astype(int), dg[..., 1]) if diag else rep


def build_wrench_ref():
    srcs = ("artic_wrench_ref.cpp", "artic_pair_ref.cpp", "artic_box_ref.cpp", "artic_drive_ref.cpp", "artic_pose_ref.cpp")
    return WrenchRef(native_build.build(srcs, "artic_wrench_ref"))


def world_wrench(wr, w):
    """world w's rows of a LinkWrench of numpy arrays, as a one-world LinkWrench"""
    if wr is None:
        return None
    a = wr.arrays
    return A.LinkWrench(w=None if a["w"] is None else np.ascontiguousarray(a["w"][..., w:w + 1, :, :]),
                        link_axes=bool(wr.terms & A.MH_LINK_WRENCH_LINK_AXES),
                        **{k: (None if a[k] is None else np.ascontiguousarray(a[k][w:w + 1])) for k in A.LinkWrench._DAMP})


class _WorldOf:
    """the face P.step_worlds asks for (step_report), stepping with one world's wrench"""

    def __init__(self, ref, wr):
        self.ref, self.wr = ref, wr

    def step_report(self, *a, **k):
        return self.ref.step_wrench(*a, wrench=self.wr, **k)


def step_worlds(ref, model, params, q, qd, aux, dt, n, pose=None, drive=None, wrench=None):
    """P.step_worlds with a wrench: every world in place by the wrench reference with B = 1 on its own model -> the launch's report"""
    rep = np.full((q.shape[0], int(n), A.report_slots(model), RP), np.nan)
    for w in range(q.shape[0]):
        rep[w] = P.step_worlds(_WorldOf(ref, world_wrench(wrench, w)), model, params, q, qd, aux, dt, n, pose=pose, drive=drive, worlds=[w])[w]
    return rep


def to_device(wr, dev):
    """a LinkWrench of numpy arrays as one of torch tensors on dev"""
    import torch
    t = {k: (None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)) for k, a in wr.arrays.items()}
    return A.LinkWrench(link_axes=bool(wr.terms & A.MH_LINK_WRENCH_LINK_AXES), **t)


DBL_MAX = np.finfo(float).max


def chain3(algorithm):
    """a 3-joint chain, no limits, no geometry"""
    m = A.chain_model(3, lo=-DBL_MAX, hi=DBL_MAX)
    m.algorithm = algorithm
    return m


def free_body(mass=2.0, inertia=0.02, x0=(0.0, 1.0, 0.0), gravity=(0.0, 0.0, 0.0)):
    """a one-link floating base, no geometry: the base link is link 5"""
    return A.model_from_links([], gravity=gravity, floating_base=dict(R0=np.eye(3), x0=x0, mass=mass, inertia=np.eye(3) * inertia))


def fk(model, q):
    """numpy forward kinematics of one state, independent of the native code -> (R (nj, 3, 3), x (nj, 3), S (nj, 6), motion subspaces about the model
    origin [angular; linear], c (nj, 3), the links' centres of mass)"""
    nj = model.nj
    R = np.zeros((nj, 3, 3)); x = np.zeros((nj, 3)); Sm = np.zeros((nj, 6)); c = np.zeros((nj, 3))
    for i in range(nj):
        ax = np.array(list(model.axis[i])); Rrel = np.array(list(model.Rrel[i])).reshape(3, 3); trel = np.array(list(model.trel[i]))
        if model.jtype[i] == A.MH_JOINT_REVOLUTE:
            K = np.array([[0.0, -ax[2], ax[1]], [ax[2], 0.0, -ax[0]], [-ax[1], ax[0], 0.0]])
            Rl = Rrel @ (np.cos(q[i]) * np.eye(3) + (1.0 - np.cos(q[i])) * np.outer(ax, ax) + np.sin(q[i]) * K); tl = trel
        else:
            Rl = Rrel; tl = trel + Rrel @ (ax * q[i])
        p = model.parent[i]
        R[i] = Rl if p < 0 else R[p] @ Rl
        x[i] = tl if p < 0 else x[p] + R[p] @ tl
        aw = R[i] @ ax
        Sm[i] = np.concatenate([aw, np.cross(x[i], aw)]) if model.jtype[i] == A.MH_JOINT_REVOLUTE else np.concatenate([np.zeros(3), aw])
        c[i] = x[i] + R[i] @ np.array(list(model.com[i]))
    return R, x, Sm, c


def link_velocity(model, Sm, qd, i):
    """[omega; v about the model origin] of link i"""
    V = np.zeros(6)
    j = i
    while j >= 0:
        V += Sm[j] * qd[j]; j = model.parent[j]
    return V


# ---- the cases the GPU test runs (tests/test_artic_wrench_gpu.py), each in one launch; tests/test_artic_wrench.py
# (test_gpu_cases_keep_their_point) proves on the reference alone that each keeps its point ----
B = 3
NSTEPS = 4
CRB, FSAB = A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB
G = (0.0, -9.81, 0.0)


def _wrench(rng, nj, rows, scale=2.0, links=None):
    """(B, nj, 6) held or (rows, B, nj, 6): a different wrench for every world, link and row (links: only those, the others zero)"""
    w = rng.uniform(-scale, scale, ((B, nj, 6) if rows == 1 else (rows, B, nj, 6)))
    if links is not None:
        keep = np.zeros(nj, dtype=bool); keep[list(links)] = True
        w[..., ~keep, :] = 0.0
    return w


def _gains(rng, nj, links=None):
    k = dict(kl=rng.uniform(0.1, 1.0, (B, nj)), ka=rng.uniform(0.01, 0.1, (B, nj)), klsq=rng.uniform(0.05, 0.5, (B, nj)), kasq=rng.uniform(0.005, 0.05, (B, nj)))
    if links is not None:
        for a in k.values():
            keep = np.zeros(nj, dtype=bool); keep[list(links)] = True
            a[:, ~keep] = 0.0
    return k


def case_chain(algorithm, rows):
    """the chain of 3 without geometry, a wrench on every link"""
    m = chain3(algorithm)
    rng = np.random.default_rng(30 + rows)
    return dict(m=m, q=rng.uniform(-0.8, 0.8, (B, 3)), qd=rng.uniform(-1.0, 1.0, (B, 3)), dt=1e-3, wrench=A.LinkWrench(w=_wrench(rng, 3, rows)))


def case_chain_damped():
    """the chain of 3, FSAB, damping alone with gains that differ per world and link"""
    m = chain3(FSAB)
    rng = np.random.default_rng(41)
    return dict(m=m, q=rng.uniform(-0.8, 0.8, (B, 3)), qd=rng.uniform(-2.0, 2.0, (B, 3)), dt=1e-3, wrench=A.LinkWrench(**_gains(rng, 3)))


def case_arm():
    """a two-link arm whose tip sphere lands on the floor during the launch (a step with two mini-steps): the wrench in the links' own axes, a
    schedule row per step, a drive, the report"""
    m = A.add_spheres(A.chain_model(2, lo=-3.0, hi=3.0), [(1, (0.0, 0.0, -0.5), 0.05)], plane_point=(0.0, 0.0, -0.9), epsilon=0.2)
    rng = np.random.default_rng(42)
    # the tip's lowest point is at z = -(cos q0 + cos(q0 + q1)) / 2 - 0.05 over the floor z = -0.9: q0 by bisection for a gap of a millimetre or so,
    # closing at about 0.8 m/s, so that every world lands inside the launch
    q = np.zeros((B, 2)); qd = np.zeros((B, 2))
    for w, (q1, gap) in enumerate(((0.1, 3e-4), (0.2, 9e-4), (0.15, 1.4e-3))):
        lo, hi = 0.2, 1.2
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if np.cos(mid) + np.cos(mid + q1) > 1.7 - 2.0 * gap else (lo, mid)
        q[w] = (hi, q1)
    qd[:, 0] = -1.5
    sh = (NSTEPS, B, 2)                                               # a PD servo and a feed-forward force on both joints, a row per step
    drive = A.Drive(kp=rng.uniform(0.0, 3.0, (B, 2)), kv=rng.uniform(0.0, 0.3, (B, 2)), q_des=rng.uniform(-0.3, 0.3, sh),
                    qd_des=rng.uniform(-0.5, 0.5, sh), tau_ff=rng.uniform(-1.0, 1.0, sh))
    return dict(m=m, q=q, qd=qd, dt=1e-3, report=True, drive=drive, wrench=A.LinkWrench(w=_wrench(rng, 2, NSTEPS), link_axes=True))


def case_foot():
    """the floating box of BS.floating_box_pendulum coming down flat onto the plane, pose coordinates, the stabiliser on: damping on the base link
    and the pendulum, a held wrench on both, the report"""
    m = BS.floating_box_pendulum(mu=100.0)[0]
    rng = np.random.default_rng(43)
    q = np.zeros((B, 7)); qd = np.zeros((B, 7))
    q[:, 1] = -0.2 + np.array([2e-4, 1.2e-3, 2.5e-3]); qd[:, 1] = -1.0; qd[:, 0] = rng.uniform(-0.3, 0.3, B); qd[:, 3:6] = rng.uniform(-0.2, 0.2, (B, 3))
    q[:, 6] = rng.uniform(-0.5, 0.5, B); qd[:, 6] = rng.uniform(-0.5, 0.5, B)
    return dict(m=m, q=q, qd=qd, dt=1e-3, report=True, coords="pose", wrench=A.LinkWrench(w=_wrench(rng, 7, 1, links=(5, 6)), **_gains(rng, 7, links=(5, 6))))


def case_params():
    """the same floating box in angle coordinates without the stabiliser, a record per world (P.vary: masses, inertias, the plane, mu on either
    side of 100) and a wrench that differs per world, in the links' own axes"""
    m = BS.floating_box_pendulum(mu=100.0, iters=0)[0]
    m.cp_nk = m.cp_nk or 4
    rng = np.random.default_rng(44)
    p = P.vary(m, B, 3, [0.5, 100.0, 0.4])
    q = np.zeros((B, 7)); qd = np.zeros((B, 7))
    q[:, 1] = -0.2 + 6e-3; qd[:, 1] = -6.0; qd[:, 0] = rng.uniform(-0.3, 0.3, B)
    q[:, 6] = rng.uniform(-0.5, 0.5, B); qd[:, 6] = rng.uniform(-0.5, 0.5, B)
    return dict(m=m, q=q, qd=qd, dt=1e-3, report=True, params=p, wrench=A.LinkWrench(w=_wrench(rng, 7, NSTEPS, links=(5, 6)), link_axes=True))


def swapped(wr, a, b):
    """wr with the rows of worlds a and b exchanged"""
    arr = {k: (None if v is None else v.copy()) for k, v in wr.arrays.items()}
    for v in arr.values():
        if v is not None:
            ax = v.ndim - (3 if v.shape[-1] == 6 else 2)
            idx = [slice(None)] * v.ndim
            ia, ib = list(idx), list(idx); ia[ax] = a; ib[ax] = b
            t = v[tuple(ia)].copy(); v[tuple(ia)] = v[tuple(ib)]; v[tuple(ib)] = t
    return A.LinkWrench(link_axes=bool(wr.terms & A.MH_LINK_WRENCH_LINK_AXES), **arr)


def reference_of(ref, c, wrench="case", aux0=None):
    """the per-world reference's run of a case -> dict(q, qd, aux, pose, report) after the launch"""
    m = c["m"]
    p = c.get("params")
    if p is None:
        p = A.make_params(m, B)
    q, qd = c["q"].copy(), c["qd"].copy()
    aux = S.new_aux(B) if aux0 is None else aux0.copy()
    pose = P.world_pose(m, p) if c.get("coords") == "pose" else None
    rep = step_worlds(ref, m, p, q, qd, aux, c["dt"], NSTEPS, pose=pose, drive=c.get("drive"), wrench=c["wrench"] if isinstance(wrench, str) else wrench)
    return dict(q=q, qd=qd, aux=aux, pose=pose, report=rep)
