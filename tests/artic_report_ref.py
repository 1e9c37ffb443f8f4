"""The report reference's ctypes face (tests/native/artic_report_ref.cpp) and the cases shared by the CPU tests, the GPU tests and the bench of the
articulated stepper's contact report (include/moby_hip_artic.h, "Contact report")."""
import ctypes
import os

import numpy as np

from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import native_build
from tests.artic_pair_ref import G, UP, _hinge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RP = A.REPORT_PAIR


class ReportRef(BS.BoxSphereRef):
    """ctypes face of tests/native/artic_report_ref.cpp; the library holds the box-sphere reference too (that file is included into it)"""

    def __init__(self, path):
        super().__init__(path)
        self.lib.artic_report_ref_step.restype = None

    def step_report(self, model, q, qd, aux, dt, nsteps, pose=None, drive=None, sink=True, diag=False):
        """steps in place; -> the launch's report (B, nsteps, nslots, 8), or None with sink=False (the NULL sink); with diag=True
        -> (report, folds (B, nsteps) ints, first_cn (B, nsteps)): per world and step the folded mini-steps and the sum of the normal impulses of
        every handler call's first application"""
        keep = None
        d = None
        if drive is not None:
            drive.check(q.shape[0], model.nj)
            d = A.mh_artic_drive(terms=drive.terms, rows=drive.rows)
            keep = {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in drive.arrays.items() if a is not None}
            for k, a in keep.items():
                setattr(d, k, a.ctypes.data)
        B = int(q.shape[0])
        rep = np.full((B, int(nsteps), A.report_slots(model), RP), np.nan) if sink else None
        dg = np.zeros((B, int(nsteps), 2)) if diag else None
        P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        self.lib.artic_report_ref_step(ctypes.byref(model), B, ctypes.c_double(dt), int(nsteps), P(q), P(qd), P(aux), P(pose),
                                       None if d is None else ctypes.byref(d), P(rep), P(dg))
        del keep
        return (rep, dg[..., 0].astype(int), dg[..., 1]) if diag else rep


def build_report_ref():
    srcs = ("artic_report_ref.cpp", "artic_pair_ref.cpp", "artic_box_ref.cpp", "artic_drive_ref.cpp", "artic_pose_ref.cpp")
    return ReportRef(native_build.build(srcs, "artic_report_ref"))


# ---- the cases the GPU test runs (tests/test_artic_report_gpu.py) and whose coverage the CPU test proves on the reference's own run ----
B = 64


def long_arm_16(mu=100.0, eps=0.2, iters=10):
    """BS.long_arm_static with 16 joints, the most a model may have: the report kernels' largest LDS image"""
    links = [BS._yaw((0.0, 0.9, 0.0))]
    for k in range(15):
        links.append(_hinge(k, (0.1 * k, 0.9, 0.0), (0.05, 0.0, 0.0), mass=0.1, lo=-0.5 if k else None, hi=0.5 if k else None, restitution=0.1))
    m = A.model_from_links(links, gravity=G)
    A.add_spheres(m, [(15, (0.1, 0.0, 0.0), 0.05)], plane_normal=UP, epsilon=eps, mu_coulomb=mu)
    A.add_boxes(m, [(-1, (1.7, 0.45, 0.0), np.eye(3), (0.5, 0.3, 0.24))], plane_normal=UP, epsilon=eps, mu_coulomb=mu)
    A.add_box_sphere_pairs(m, [(0, 0)])
    m.cstab_max_iterations = iters
    lo = [-0.4, -0.5] + [-0.12] * 14; hi = [0.4, 0.1] + [0.06] * 14
    return m, BS._uniform(lo, hi, [0.3] * 16), 1e-3


_aims = {}


def _aimed(ref, build, seed, mu):
    """the scene's 64 states aimed with the reference (BS.aim reads the geometry only: once per scene and process)"""
    m, sampler, dt = build(mu=mu) if mu >= 100.0 else build(mu=mu, eps=0.2)
    if build not in _aims:
        _aims[build] = BS.aim(ref, m, sampler, B, seed)
    return m, _aims[build][0].copy(), _aims[build][1].copy(), dt


def _four_feet(ref, mu):
    from tests.test_artic_box_gpu import four_feet
    return four_feet(B, 7)


def _arm_on_table(ref, mu):
    """a sphere-only scene (tests/scenes/arm_on_table.xml) with a restitution coefficient, so that a restitution pass is there to report"""
    m, _, _, q0, qd0, dt = A.load_xml(os.path.join(ROOT, "tests", "scenes", "arm_on_table.xml"))
    m.cp_epsilon = 0.3
    rng = np.random.default_rng(3)
    q = np.tile(q0, (B, 1)) + rng.uniform(-0.05, 0.05, (B, m.nj)); qd = np.tile(qd0, (B, 1)) + rng.uniform(-0.5, 0.5, (B, m.nj))
    return m, q, qd, dt


_BUILD = {
    "arm_static": lambda ref, mu: _aimed(ref, BS.arm_static, len("arm_static"), mu),
    "arm_slider_box": lambda ref, mu: _aimed(ref, BS.arm_slider_box, len("arm_slider_box"), mu),
    "floating_box_pendulum": lambda ref, mu: _aimed(ref, BS.floating_box_pendulum, len("floating_box_pendulum"), mu),
    "mixed_all": lambda ref, mu: _aimed(ref, BS.mixed_all, len("mixed_all"), mu),
    "long_arm_static": lambda ref, mu: _aimed(ref, BS.long_arm_static, len("long_arm_static"), mu),
    "long_arm_16": lambda ref, mu: _aimed(ref, long_arm_16, 16, mu),
    "four_feet": _four_feet,
    "arm_on_table": _arm_on_table,
}
STEPS = {"arm_static": 100, "arm_slider_box": 60, "floating_box_pendulum": 100, "mixed_all": 100, "long_arm_static": 100, "long_arm_16": 100,
         "four_feet": 100, "arm_on_table": 400}          # the existing scenes' step counts (tests/test_artic_boxsphere_gpu.py, test_artic_box_gpu.py)

# (scene, coordinates, driven, stabiliser, mu, algorithm): the stabiliser, the drive and the dynamics algorithm alternate over the cases so that
# each of the eight report kernels (k_artic_step_rp[_stab][_pose][_drive]) runs at least twice
CRB, FSAB = A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB
CASES = [
    ("arm_static", "angles", False, False, 100.0, CRB),
    ("arm_slider_box", "angles", True, True, 100.0, FSAB),
    ("arm_slider_box", "angles", False, True, 0.5, CRB),
    ("floating_box_pendulum", "angles", True, False, 100.0, FSAB),
    ("floating_box_pendulum", "pose", False, False, 0.5, CRB),
    ("floating_box_pendulum", "pose", True, True, 100.0, FSAB),
    ("floating_box_pendulum", "pose", False, True, 100.0, CRB),
    ("mixed_all", "angles", False, True, 100.0, CRB),
    ("mixed_all", "pose", True, False, 100.0, FSAB),
    ("mixed_all", "pose", False, True, 100.0, CRB),
    ("mixed_all", "pose", True, True, 0.5, FSAB),
    ("mixed_all", "pose", False, False, 100.0, FSAB),
    ("long_arm_static", "angles", True, False, 100.0, CRB),
    ("long_arm_16", "angles", False, False, 100.0, FSAB),
    ("long_arm_16", "angles", True, True, 100.0, CRB),
    ("four_feet", "angles", False, True, 100.0, CRB),
    ("four_feet", "pose", True, False, 100.0, FSAB),
    ("arm_on_table", "angles", True, False, 100.0, CRB),
]


def case_id(c):
    return "%s-%s-%s-%s-mu%g-%s" % (c[0], c[1], "driven" if c[2] else "undriven", "stab" if c[3] else "plain", c[4], "fsab" if c[5] else "crb")


_runs = {}


def case_model(ref, case):
    """-> (model with the case's switches, q0, qd0, dt, steps per launch)"""
    name, _, _, stab, mu, algorithm = case
    m, q, qd, dt = _BUILD[name](ref, mu)
    if mu < 100.0: m.cp_mu_coulomb = mu; m.cp_nk = m.cp_nk or 4
    m.cstab_max_iterations = 10 if stab else 0
    m.algorithm = algorithm
    return m, q, qd, dt, STEPS[name]


def case_drive(rng, nj, n, launch):
    from tests.test_artic_box_gpu import virtual_drive
    return virtual_drive(rng, B, nj, rows=1 if launch == 0 else n)


def model_pose(m, nB):
    """the base poses a batch switched to pose coordinates starts from (mh_artic_batch_set_base_coords with q = 0): p = trel[0], Q of Rrel[3]"""
    R = np.array(list(m.Rrel[3])).reshape(3, 3)
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    assert np.array_equal(R, np.eye(3)), "the cases' floating bases start unrotated"
    return np.tile(np.array([m.trel[0][0], m.trel[0][1], m.trel[0][2], w, 0.0, 0.0, 0.0]), (nB, 1))


def reference_run(ref, case):
    """the reference's own run of a case, once per process: two launches as the GPU test makes them -> a list of per-launch dicts
    (q, qd, aux, pose, report, folds, first_cn, drive), the arrays as they stand after the launch"""
    key = case_id(case)
    if key not in _runs:
        m, q0, qd0, dt, n = case_model(ref, case)
        pose = case[1] == "pose"
        q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(B)
        Pp = model_pose(m, B) if pose else None        # (the GPU test switches a batch at q = 0 to poses, then uploads q0 against that pose)
        rng = np.random.default_rng(len(case[0]))
        out = []
        for launch in range(2):
            d = case_drive(rng, m.nj, n, launch) if case[2] else None
            rep, folds, first = ref.step_report(m, q, qd, aux, dt, n, pose=Pp, drive=d, diag=True)
            out.append(dict(q=q.copy(), qd=qd.copy(), aux=aux.copy(), pose=None if Pp is None else Pp.copy(), report=rep, folds=folds, first_cn=first, drive=d))
        _runs[key] = (m, q0, qd0, dt, n, out)
    return _runs[key]
