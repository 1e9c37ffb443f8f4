"""Episodes on the device of the articulated stepper (include/moby_hip_artic.h, "Episodes on the device"): the CPU reference of a reset between two
launches and the cases shared by the CPU tests (tests/test_artic_reset.py, which prove their coverage on the reference alone) and the GPU tests
(tests/test_artic_reset_gpu.py).  The rule under test: after a reset, world w steps as world w of a batch would after upload and set_base_pose had
written the same values and a fresh aux record into it -- so the reset here is plain array assignment and the stepping is the per-world reference loop
of tests/artic_params_ref.py (tests/native/artic_report_ref.cpp, unchanged)."""
import numpy as np

from moby_amd import scene as S
from tests import artic_params_ref as P

B = P.B
RESET_WORLDS = (1, 3, 4)
MASK = np.array([0, 1, 0, -7, 1, 0], dtype=np.int32)                  # the GPU tests' mask: "nonzero", not "one"
assert tuple(np.flatnonzero(MASK)) == RESET_WORLDS
# no-slip and Drumwright-Shell worlds in one batch with the stabiliser, FSAB, pose coordinates, a drive; the no-slip route in angles; a floating box in
# pose coordinates; the plain kernels on a chain without geometry
CASES = [
    ("mixed_all", "pose", True, True, P.MIXED, P.FSAB, 6),
    ("mixed_all", "angles", False, False, P.NOSLIP, P.CRB, 5),
    ("floating_box_pendulum", "pose", False, False, P.NOSLIP, P.CRB, 1),
    ("chain6", "angles", False, False, None, P.CRB, 20),
]
assert all(c in P.CASES for c in CASES)
# the worlds of the mask are {1, 3, 4} except where the reference's own run misses a condition of tests/test_artic_reset.py with them: world 4 of the
# floating box pendulum meets nothing in its first launch (no LCP after its reset), so that case resets {1, 3, 5}
MASK_OF = {("floating_box_pendulum", "pose"): np.array([0, 1, 0, -7, 0, 1], dtype=np.int32)}


def mask_of(case):
    """the case's mask (B int32) and the worlds it resets"""
    mk = MASK_OF.get(case[:2], MASK)
    return mk, tuple(int(w) for w in np.flatnonzero(mk))


def reset_worlds(worlds, q, qd, aux, pose, q0, qd0, pose0):
    """the reset as array assignment, in place: each world of `worlds` back to its own start state with a fresh aux record"""
    for w in worlds:
        q[w] = q0[w]; qd[w] = qd0[w]; aux[w] = S.new_aux(1)[0]
        if pose is not None:
            pose[w] = pose0[w]


_runs = {}


def box_family_run(ref):
    """the box family proper (mh_artic_box.hip: a plain batch of a model with boxes only) with the stabiliser, whose Cn / Cn X rows and distances live
    in the batch's workspace: R's four_feet scene, one shared model, two launches with worlds RESET_WORLDS reset between them, once per process ->
    (m, q0, qd0, dt, n, [launch 0, launch 1] dicts of q, qd, aux)"""
    if "box_family" not in _runs:
        from moby_amd import artic as A
        from tests import artic_report_ref as R
        m, q, qd, dt = R._BUILD["four_feet"](ref, 100.0)
        m.cp_nk = m.cp_nk or 4
        m.cstab_max_iterations = 10
        q0, qd0, n = q[:B].copy(), qd[:B].copy(), R.STEPS["four_feet"]
        p = A.make_params(m, B)                                      # records equal to the model: the per-world loop steps the shared model
        q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(B)
        out = []
        for launch in range(2):
            if launch == 1:
                reset_worlds(RESET_WORLDS, q, qd, aux, None, q0, qd0, None)
            P.step_worlds(ref, m, p, q, qd, aux, dt, n)
            out.append(dict(q=q.copy(), qd=qd.copy(), aux=aux.copy()))
        _runs["box_family"] = (m, q0, qd0, dt, n, out)
    return _runs["box_family"]


def reset_run(ref, case):
    """P.reference_run's two launches (the same model, records, start state and drives) with the worlds of the case's mask reset between them, once per
    process -> (m, q0, qd0, dt, n, records, pose0, [launch 0, launch 1], the state right after the reset); the launch dicts as P.reference_run's"""
    worlds = mask_of(case)[1]
    key = P.case_id(case)
    if key not in _runs:
        m, q0, qd0, dt, n, p = P.case_model(ref, case)
        q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(B)
        pose0 = P.world_pose(m, p) if case[1] == "pose" else None
        Pp = None if pose0 is None else pose0.copy()
        rng = np.random.default_rng(len(case[0]))                    # P.reference_run's drives: the uninterrupted run differs by the reset alone
        out, after = [], None
        for launch in range(2):
            d = P.case_drive(rng, m.nj, n, launch) if case[2] else None
            if launch == 1:
                reset_worlds(worlds, q, qd, aux, Pp, q0, qd0, pose0)
                after = dict(q=q.copy(), qd=qd.copy(), aux=aux.copy(), pose=None if Pp is None else Pp.copy())
            rep = P.step_worlds(ref, m, p, q, qd, aux, dt, n, pose=Pp, drive=d)
            out.append(dict(q=q.copy(), qd=qd.copy(), aux=aux.copy(), pose=None if Pp is None else Pp.copy(), report=rep, drive=d))
        _runs[key] = (m, q0, qd0, dt, n, p, pose0, out, after)
    return _runs[key]
