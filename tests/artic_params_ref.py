"""Per-world parameters of the articulated stepper (include/moby_hip_artic.h, "Per-world parameters"): the per-world reference loop and the cases
shared by the CPU tests (tests/test_artic_params.py, which prove their coverage on the reference alone) and the GPU tests
(tests/test_artic_params_gpu.py).  The rule under test: world w of a batch with records steps as a batch of the model with record w written into it
would -- so the reference is tests/native/artic_report_ref.cpp, run once per world on that model with the world's own rows of drive, pose and aux."""
import ctypes
import os

import numpy as np

from moby_amd import artic as A
from moby_amd import scene as S
from tests import artic_boxsphere_ref as BS
from tests import artic_report_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 6
RP = A.REPORT_PAIR
DBL_MAX = np.finfo(float).max


def model_of_world(model, params, w):
    """a copy of the model with record w written into it"""
    m = A.mh_artic_model.from_buffer_copy(model)
    for name in A.PARAMS_DTYPE.names:
        v = params[name][w]
        if v.ndim == 0:
            setattr(m, name, float(v))
        else:
            ctypes.memmove(ctypes.addressof(getattr(m, name)), np.ascontiguousarray(v).ctypes.data, v.nbytes)
    return m


def world_drive(d, w):
    """world w's rows of a Drive, as a one-world Drive"""
    if d is None:
        return None
    return A.Drive(**{k: (None if a is None else np.ascontiguousarray(a[..., w:w + 1, :])) for k, a in d.arrays.items()})


def step_worlds(ref, model, params, q, qd, aux, dt, n, pose=None, drive=None, worlds=None):
    """steps every world (or `worlds`) in place by the report reference with B = 1 on its own model; -> the launch's report (B, n, nslots, 8), rows of
    worlds not stepped NaN"""
    nB = q.shape[0]
    rep = np.full((nB, int(n), A.report_slots(model), RP), np.nan)
    for w in (range(nB) if worlds is None else worlds):
        mw = model_of_world(model, params, w)
        qw, qdw, aw = q[w:w + 1].copy(), qd[w:w + 1].copy(), aux[w:w + 1].copy()
        pw = None if pose is None else pose[w:w + 1].copy()
        rep[w] = ref.step_report(mw, qw, qdw, aw, dt, n, pose=pw, drive=world_drive(drive, w))[0]
        q[w], qd[w], aux[w] = qw[0], qdw[0], aw[0]
        if pose is not None: pose[w] = pw[0]
    return rep


def world_pose(model, params):
    """the base poses a params batch switched to pose coordinates at q = 0 starts from: each world's own trel[0] and the quaternion of its Rrel[3]"""
    return np.concatenate([R.model_pose(model_of_world(model, params, w), 1) for w in range(params.shape[0])])


# ---- the varied records ----
def vary(model, nB, seed, mus, geometry=True):
    """nB records around the model: masses, inertias, centres of mass, link offsets, limits (moved, never added), restitution, gravity, and with
    geometry sphere radii, box sizes and centres, the plane frame, restitution and friction of the contacts (mus: one mu per world).  World 0 is
    varied like the others (the coverage test compares every world with record 0's run)."""
    rng = np.random.default_rng(seed)
    p = A.make_params(model, nB)
    nj = model.nj
    body = np.arange(6 if model.floating_base else 0, nj)             # the virtual joints keep the entries the layout fixes
    f = rng.uniform(0.7, 1.3, (nB, A.MH_ARTIC_MAX_JOINTS))
    p["mass"] *= f; p["inertia"] *= f[:, :, None]
    p["com"][:, body] += rng.uniform(-0.02, 0.02, (nB, len(body), 3))
    p["trel"][:, body] += rng.uniform(-0.01, 0.01, (nB, len(body), 3))
    if model.floating_base:
        p["trel"][:, 0] += rng.uniform(0.0, 0.01, (nB, 3))            # the base's start (angle coordinates read it; a pose batch starts from it)
    lo_f = np.abs(p["lolimit"]) < DBL_MAX; hi_f = np.abs(p["hilimit"]) < DBL_MAX
    p["lolimit"] -= np.where(lo_f, rng.uniform(0.0, 0.05, lo_f.shape), 0.0)
    p["hilimit"] += np.where(hi_f, rng.uniform(0.0, 0.05, hi_f.shape), 0.0)
    # restitution on the joints that have one (a restitution pass over several coupled limits that leaves one of them approaching again is
    # MH_WORLD_UNSUPPORTED, which freezes the world: a model whose limits do not bounce keeps them so)
    bouncy = [i for i in range(nj) if model.limit_restitution[i] > 0.0]
    p["limit_restitution"][:, bouncy] = rng.uniform(0.0, 0.3, (nB, len(bouncy)))
    p["gravity"] *= rng.uniform(0.9, 1.1, (nB, 1))
    if geometry:
        ns, nb = model.nspheres, model.nboxes
        p["sphere_radius"][:, :ns] *= rng.uniform(0.96, 1.0, (nB, ns))          # (shrunk only: the aimed start states stay clear of their boxes)
        p["box_len"][:, :nb] *= rng.uniform(0.96, 1.0, (nB, nb, 3))
        static = np.array([model.box_link[k] < 0 for k in range(nb)], dtype=bool)
        p["box_center"][:, :nb] += np.where(static[None, :, None], rng.uniform(-0.01, 0.0, (nB, nb, 3)), 0.0)   # the crate, moved away and down
        n0 = np.array(list(model.plane_R)).reshape(3, 3)[:, 1]; o0 = np.array(list(model.plane_o))
        for w in range(nB):                                           # the ground, tilted by up to a degree and lowered by up to a centimetre
            n = n0 + rng.uniform(-0.02, 0.02, 3)
            p["plane_R"][w] = A._plane_frame(model, n, o0, False).reshape(9)
            p["plane_o"][w] = o0 - n0 * rng.uniform(0.0, 0.01)
        p["cp_epsilon"] = rng.uniform(0.1, 0.4, nB)
        p["cp_mu_coulomb"] = np.asarray(mus, dtype=float)
        p["cp_mu_viscous"] = np.where(p["cp_mu_coulomb"] < 100.0, rng.uniform(0.0, 0.05, nB), 0.0)
    return p


# ---- the cases ----
CRB, FSAB = A.MH_ARTIC_CRB, A.MH_ARTIC_FSAB
NOSLIP = [100.0] * B
MIXED = [0.5, 100.0, 0.4, 120.0, 0.6, 100.0]                        # worlds on either side of mu = 100 in one batch
# (scene, coordinates, driven, stabiliser, per-world mu, algorithm, seed of the records -- picked so that the reference's runs meet the conditions of
# tests/test_artic_params.py): between them all eight step kernels (plain / stab x angles / pose x undriven /
# driven) with both CRB and FSAB, on the mixed model, the floating box pendulum, a sphere-only arm, the 16-joint arm and a chain with no geometry
CASES = [
    ("mixed_all", "pose", True, True, MIXED, FSAB, 6),
    ("mixed_all", "angles", False, False, NOSLIP, CRB, 5),
    ("mixed_all", "pose", False, True, NOSLIP, CRB, 5),
    ("floating_box_pendulum", "pose", False, False, NOSLIP, CRB, 1),
    ("floating_box_pendulum", "angles", True, True, MIXED, FSAB, 1),
    ("floating_box_pendulum", "pose", True, False, NOSLIP, FSAB, 1),
    ("arm_on_table", "angles", True, False, NOSLIP, CRB, 2),
    ("long_arm_16", "angles", False, True, NOSLIP, FSAB, 6),
    ("chain6", "angles", False, False, None, CRB, 20),
    ("chain6", "angles", True, True, None, FSAB, 6),
]
STEPS = dict(R.STEPS, arm_on_table=200, chain6=100)                 # the existing scenes' step counts or fewer


def case_id(c):
    mu = "nomu" if c[4] is None else "mixedmu" if c[4] is MIXED else "noslip"
    return "%s-%s-%s-%s-%s-%s" % (c[0], c[1], "driven" if c[2] else "undriven", "stab" if c[3] else "plain", mu, "fsab" if c[5] else "crb")


def chain6():
    """chain_model(6): the robot alone, no geometry at all -- limits, restitution and gravity are what its records vary"""
    m = A.chain_model(6, lo=-0.6, hi=0.6)
    rng = np.random.default_rng(66)
    sg = rng.choice([-1.0, 1.0], (R.B, 6))                           # every joint starts near one of its limits and moves towards it
    return m, sg * rng.uniform(0.4, 0.59, (R.B, 6)), sg * rng.uniform(0.5, 2.5, (R.B, 6)), 1e-3


def case_model(ref, case):
    """-> (model with the case's switches, q0, qd0 (B worlds), dt, steps per launch, records)"""
    name, _, _, stab, mus, algorithm, seed = case
    if name == "chain6":
        m, q, qd, dt = chain6()
    else:
        m, q, qd, dt = R._BUILD[name](ref, 100.0)
        m.cp_nk = m.cp_nk or 4
    m.cstab_max_iterations = 10 if stab else 0
    m.algorithm = algorithm
    p = vary(m, B, seed, mus, geometry=mus is not None)
    return m, q[:B].copy(), qd[:B].copy(), dt, STEPS[name], p


def case_drive(rng, nj, n, launch):
    from tests.test_artic_box_gpu import virtual_drive
    return virtual_drive(rng, B, nj, rows=1 if launch == 0 else n)


_runs = {}


def reference_run(ref, case, params_of_launch=None, key=None):
    """the per-world reference's run of a case, once per process: two launches as the GPU test makes them (a held drive row, then a row per step) -> (m,
    q0, qd0, dt, n, records, [per-launch dicts q, qd, aux, pose, report, drive]).  params_of_launch(launch, records) -> the records of that launch
    (the setter tests switch some between the launches)"""
    key = (case_id(case), key, case[6])
    if key not in _runs:
        m, q0, qd0, dt, n, p = case_model(ref, case)
        q, qd, aux = q0.copy(), qd0.copy(), S.new_aux(B)
        Pp = world_pose(m, p) if case[1] == "pose" else None
        rng = np.random.default_rng(len(case[0]))
        out = []
        for launch in range(2):
            pl = p if params_of_launch is None else params_of_launch(launch, p)
            d = case_drive(rng, m.nj, n, launch) if case[2] else None
            rep = step_worlds(ref, m, pl, q, qd, aux, dt, n, pose=Pp, drive=d)
            out.append(dict(q=q.copy(), qd=qd.copy(), aux=aux.copy(), pose=None if Pp is None else Pp.copy(), report=rep, drive=d, params=pl))
        _runs[key] = (m, q0, qd0, dt, n, p, out)
    return _runs[key]


def switched(launch, p):
    """the setter tests' records: worlds 2..4 take the records of worlds 5, 0, 1 for the second launch"""
    if launch == 0:
        return p
    p2 = p.copy(); p2[2:5] = p[[5, 0, 1]]
    return p2
